"""The statistics of tests/philox_indel_stats.py, held to their own contract without a GPU: the replay is exact on the plain
sampler (which knows every test that fired), on the oracle's reference-compatible (MT) sample with rows -- it equals the real
reference byte for byte, which ties the replay, the row order and both quirks to what the reference does -- and on the oracle's
Philox sample; the statistics accept all three, and they reject every kept planted defect at the recorded sizes."""
import os

import numpy as np
import pytest

import philox_indel_stats as IS
import philox_stats as PS
from helpers import dense_model, random_genome
from philox_indel_stats import GENOME, all_stats, assert_accepted, case_model

STEP = 1 << 13  # pairs of a slice
THREADS = max(1, min(8, os.cpu_count() or 1))


def sample_slices(t, genome, sample, positions=None, step=STEP):
    n = len(sample["coords"])
    for a in range(0, n, step):
        m = min(step, n - a)
        yield IS.indel_slice(t, genome, sample["coords"][a:a + m], sample["bases"][a:a + m], sample["quals"][a:a + m],
                             IS.rows_of(sample["rows"], a, m), positions)


def oracle_sample(d, genome, n, mode, seed=77, first_ordinal=0):
    from oracle import oracle as O

    O.build()
    RL = d.read_length
    rng = O.Rng().seed_mt(seed) if mode == "mt" else O.Rng().seed_philox(seed)
    res = O.Oracle(d).simulate(rng, genome, n, first_ordinal=first_ordinal, want_coords=True, store_mutations=True)
    assert res["status"] == 0 and res["n_done"] == n
    return {"coords": res["coords"], "bases": PS.stack_mates(res["r1_base"][:, :RL], res["r2_base"][:, :RL]),
            "quals": PS.stack_mates(res["r1_qual"][:, :RL], res["r2_qual"][:, :RL]), "rows": res["mutations"]}


@pytest.mark.parametrize("case,n", [("flat", 1 << 15), ("patterned", 1 << 14)])
def test_the_replay_is_exact_and_the_statistics_accept_the_sampler(case, n):
    """I0 .. I5 and S5 .. S7 on ``sample_model``; the replayed events are the sampler's own, all but the hidden deletions, and
    those sit at hidden steps; the excluded-step condition holds."""
    d, genome, mixed = case_model(case)
    t, x = IS.Tables(d), PS.Expect(d)
    s = IS.sample_model(d, n, 2024, genome)
    stats = all_stats(d, t, x, mixed)
    truth = np.zeros((n, 2, t.NS, 5), dtype=np.uint8)
    f = s["fired"]
    truth[f[:, 0], f[:, 1], f[:, 2], f[:, 3]] = 1
    a = 0
    for sl in sample_slices(t, genome, s):
        rep, m = sl["rep"], len(sl["coords"])
        diff = truth[a:a + m] != rep["X"]
        assert not (diff[..., :4].any() or (diff[..., 4] & ~rep["hidden"]).any()), "the replay's events are not the sampler's"
        assert not (diff[..., 4] & (rep["X"][..., 4] > 0)).any()
        off = (rep["pre"] != s["pre"][a:a + m]).any(axis=2)  # the replayed sequence is the sampler's, but where the read fits both
        assert not (off & ~rep["either"]).any() and off.sum() <= 2  # (of 16 384 reads; the replay takes the candidate nearer the read)
        a += m
        for st in stats:
            st.add(sl)
    assert_accepted(stats)
    print(case, "excluded share %.4f" % stats[1].excluded_share(), dict(stats[0].i0))


@pytest.mark.parametrize("mode", ["mt", "philox"])
@pytest.mark.parametrize("case,n", [("flat", 1 << 16), ("patterned", 1 << 15)])
def test_the_statistics_accept_the_oracle(case, n, mode):
    """Every position of the oracle's sample with its rows, in the reference-compatible mode and on the Philox address map."""
    d, genome, mixed = case_model(case)
    t, x = IS.Tables(d), PS.Expect(d)
    s = oracle_sample(d, genome, n, mode)
    stats = PS.run_stats(lambda: all_stats(d, t, x, mixed), sample_slices(t, genome, s), THREADS)
    assert_accepted(stats)
    assert stats[0].i0["hidden reads"] > 0
    print(case, mode, "excluded share %.4f" % stats[1].excluded_share(), dict(stats[0].i0))


def test_the_oracle_with_the_shipped_indel_tables():
    """NovaSeq as shipped: nine non-zero insertion entries of 2e-6.  I0, and I1 over the non-zero cells (an event anywhere
    else rejects by itself)."""
    d, genome = dense_model("novaseq"), random_genome(99, GENOME)
    t = IS.Tables(d)
    assert 0 < (t.ins > 0).sum() < 20
    s = oracle_sample(d, genome, 1 << 16, "philox")
    stats = PS.run_stats(lambda: [IS.I0(), IS.I1(t)], sample_slices(t, genome, s), THREADS)
    assert_accepted(stats)
    assert sum(r.m for r in stats[1].results()) == int((t.ins[:, :t.NS] > 0).sum() + (t.dele[:, :t.NS] > 0).sum())


def families(RL):
    """Hypotheses of the GPU case that runs a statistic over every column (upper bounds)."""
    CE, C = 4 * (RL - 1), 2 * RL
    return {"I1": 16 * (RL - 1), "I2": CE * C, "I3": CE * C, "I4": CE * (CE - 1) // 2 + len(PS.LAGS) * CE * CE, "I5": CE * 72, "S7": 8}


MEANT_FOR = {"i": "I2", "j": "I3", "k": "I4", "l": "I4", "m": "I4", "n": "I5", "o": "I1", "p": "S7", "hi": "I2", "hm": "I4"}
MARGIN = 100.0
STANDING_AT_HALF = {"flat": "i", "patterned": "k"}
POSITIONS = np.array([0, 1, 2, 50, 100])


def verdicts(case, n, defects, seed=None):
    """{(defect, statistic): (accepted against the GPU case's family, smallest p)} of ``sample_model`` at n pairs with each of
    ``defects`` planted (None: the sample as it is); phreds at POSITIONS only."""
    d, genome, mixed = case_model(case)
    t, x = IS.Tables(d), PS.Expect(d)
    fam = families(d.read_length)
    base = IS.sample_model(d, n, 100 + n.bit_length() - 1 if seed is None else seed, genome, positions=POSITIONS, keep=True)
    out = {}
    for defect in defects:
        s = base if defect is None else IS.plant(d, base, defect)
        keys = ("I1", "I2", "I3", "I4", "I5", "S7") if defect is None else (MEANT_FOR[defect],)
        make = {"I1": lambda: IS.I1(t), "I2": lambda: IS.I2(d, POSITIONS, x, t), "I3": lambda: IS.I3(d, POSITIONS, x, t, letters_only=mixed),
                "I4": lambda: IS.I4(t), "I5": lambda: IS.I5(d, t, GENOME, x), "S7": lambda: PS.S7(d, POSITIONS, x)}
        stats = PS.run_stats(lambda: [IS.I0()] + [make[k]() for k in keys], sample_slices(t, genome, s, POSITIONS), THREADS)
        if defect is None:
            assert not stats[0].failures(), stats[0].i0
        for key, st in zip(keys, stats[1:]):
            res = st.results()
            out[(defect, key)] = (PS.accept(res, alpha=PS.ALPHA / (1.0 if defect is None else MARGIN), m=fam[key])[0], min(r.p for r in res))
    return out


@pytest.mark.parametrize("case", ["flat", "patterned"])
def test_every_planted_defect_is_rejected(case):
    """At N_PAIRS[case] pairs of ``sample_model`` every defect of ``plant`` (but those listed in DROPPED) is rejected by the
    statistic meant for it, against the bound of the whole family the GPU case tests and a factor 100 inside it -- and at half
    that size one is not: N_PAIRS is the smallest such power of two."""
    kept = [k for k in IS.DEFECTS if k not in IS.DROPPED[case]]
    n = IS.N_PAIRS[case]
    got = verdicts(case, n, [None] + kept)
    print(case, n, {k: "%.3g" % v[1] for k, v in got.items()})
    for (defect, key), (ok, p) in got.items():
        if defect is None:
            assert ok, ("the undamaged sample is rejected", key, p)
        else:
            assert not ok, ("defect %s is not rejected by %s at %d pairs" % (defect, key, n), p)
    half = verdicts(case, n >> 1, [STANDING_AT_HALF[case]])  # (the one the power check saw standing there: a run, not four)
    print(case, n >> 1, {k: "%.3g" % v[1] for k, v in half.items()})
    assert any(ok for ok, _ in half.values()), "N_PAIRS is not the smallest size"


def cap_verdicts(n, defects):
    """``verdicts`` for the case "flat-cap": I4 over the first CAP_STEPS steps of both mates (the sampler's loop ends there: a
    step's state depends on nothing behind it), against the family of that GPU case."""
    d, genome, _ = case_model("flat")
    t = IS.Tables(d, steps=IS.CAP_STEPS)
    fam = t.CE * (t.CE - 1) // 2 + len(PS.LAGS) * t.CE * t.CE
    base = IS.sample_model(d, n, 300 + n.bit_length(), genome, positions=POSITIONS[:2], keep=True, steps=IS.CAP_STEPS)
    out = {}
    for defect in defects:
        s = base if defect is None else IS.plant(d, base, defect)
        stats = PS.run_stats(lambda: [IS.I0(), IS.I4(t)], sample_slices(t, genome, s, step=1 << 16), THREADS)
        assert not stats[0].failures(), stats[0].i0
        res = stats[1].results()
        out[defect] = (PS.accept(res, alpha=PS.ALPHA / (1.0 if defect is None else MARGIN), m=fam)[0], min(r.p for r in res))
    return out


def test_one_read_in_a_hundred_on_the_draw_before_is_rejected_at_the_cap():
    """Defect hm needs the cap of 2^20 pairs; the GPU case "flat-cap" looks at the first CAP_STEPS steps there, and so does this:
    rejected at N_PAIRS["flat-cap"], not at half of it."""
    n = IS.N_PAIRS["flat-cap"]
    got = cap_verdicts(n, [None, "hm", "m"])
    print(n, {k: "%.3g" % v[1] for k, v in got.items()})
    assert got[None][0] and not got["hm"][0] and not got["m"][0], got
    half = cap_verdicts(n >> 1, ["hm"])
    print(n >> 1, {k: "%.3g" % v[1] for k, v in half.items()})
    assert half["hm"][0], "N_PAIRS of the cap case is not the smallest size"


def test_patterned_tables_are_what_the_case_says():
    d = IS.patterned_indel(dense_model("miseq"))
    t = IS.Tables(d)
    rows_per_read = (t.ins[:, :t.NS].sum() + t.dele[:, :t.NS].mean(axis=2).sum()) / 2
    assert 1.6 < rows_per_read < 2.0
    assert set(np.unique(d.ins)) == set(np.unique(d.dele)) == {0.0, 1e-4, 1e-3, 1e-2}
    assert not np.array_equal(d.ins[0], d.ins[1])
