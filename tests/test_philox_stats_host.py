"""The statistics of tests/philox_stats.py, held to their own contract without a GPU: they accept the plain numpy sampler of the
model at the sizes the GPU cases use, they accept the oracle's reference-compatible (MT) sample -- which equals the real
reference byte for byte, so it ties every expectation (reverse orientation, the side of every search, the order of the
alternatives) to what the reference does -- and the oracle's Philox sample, and they reject every planted defect at the
recorded sizes."""
import os

import numpy as np
import pytest

import philox_stats as PS
from helpers import dense_model, mixed_genome, random_genome

MODELS = ("hiseq", "miseq", "novaseq", "nextseq")
GENOME = 400_000


def _needed_positions(name, RL):
    """The positions the structural pairs touch (both mates alike)."""
    return sorted({p for a, b in PS.structural_pairs(name, RL) for _, p in (a, b)})


def _all_stats(d, name, pos, x, genome_length):
    in_pos = set(pos)
    pairs = [(a, b) for a, b in PS.structural_pairs(name, d.read_length) if a[1] in in_pos and b[1] in in_pos]
    return [PS.S1(d, pos, x), PS.S2(d, pos, x), PS.S3(d, pairs, pos, x), PS.S4(d, pos, x), PS.S5(d, pos, x), PS.S6(d, pos, x),
            PS.S7(d, pos, x), PS.S8(d, genome_length, None, x)]


def _assert_accepted(stats):
    """One family per statistic class, as the GPU cases have it."""
    for st in stats:
        ok, text = PS.accept(st.results())
        assert ok, text


@pytest.mark.parametrize("name", MODELS)
def test_the_statistics_accept_the_reference_sampler(name):
    """S1 .. S8 on ``sample_model`` at the size of the model's GPU cases; only the positions of the structural pairs are drawn."""
    d = dense_model(name, indel=(0.0, 0.0))
    x, genome = PS.Expect(d), random_genome(5, GENOME)
    pos = _needed_positions(name, d.read_length)
    stats = _all_stats(d, name, pos, x, GENOME)
    rng = np.random.RandomState(2024)
    step = 1 << 17
    for _ in range(0, PS.N_PAIRS[name], step):
        s = PS.sample_model(d, step, rng, genome, positions=pos)
        for st in stats:
            st.add(s)
    _assert_accepted(stats)


@pytest.mark.parametrize("mode", ["mt", "philox"])
@pytest.mark.parametrize("name,n", [("hiseq", 100_000), ("miseq", 60_000)])
def test_the_statistics_accept_the_oracle(name, n, mode):
    """Every position of the oracle's sample, in the reference-compatible mode and on the Philox address map."""
    from oracle import oracle as O

    O.build()
    d = dense_model(name, indel=(0.0, 0.0))
    genome = random_genome(6, GENOME)
    rng = O.Rng().seed_mt(77) if mode == "mt" else O.Rng().seed_philox(77)
    rows = O.Oracle(d).simulate(rng, genome, n, want_coords=True)
    assert rows["status"] == 0 and rows["n_done"] == n
    x, step = PS.Expect(d), 1 << 13

    def slices():
        for a in range(0, n, step):
            yield PS.slice_of({k: v[a:a + step] for k, v in rows.items() if k.startswith("r")}, rows["coords"][a:a + step], genome, d.read_length)

    _assert_accepted(PS.run_stats(lambda: _all_stats(d, name, np.arange(d.read_length), x, GENOME), slices(), min(8, os.cpu_count() or 1)))


def test_the_statistics_accept_the_oracle_on_a_mixed_genome():
    """Lower-case and ambiguous template letters (S5 .. S7 count upper-case A, C, G, T only; an ambiguous letter never changes):
    the reverse template keeps the case of the genome, as rev_comp does."""
    from oracle import oracle as O

    O.build()
    d = dense_model("hiseq", indel=(0.0, 0.0))
    genome = mixed_genome(7, GENOME)
    rows = O.Oracle(d).simulate(O.Rng().seed_philox(78), genome, 30_000, want_coords=True)
    assert rows["status"] == 0 and rows["n_done"] == 30_000
    x = PS.Expect(d)
    stats = [PS.S5(d, None, x, letters_only=True), PS.S6(d, None, x, letters_only=True), PS.S7(d, None, x)]
    s = PS.slice_of(rows, rows["coords"], genome, d.read_length)
    for st in stats:
        st.add(s)
    _assert_accepted(stats)
    plain = [PS.S5(d, None, x)]  # and the restriction matters: counted as they are, the ambiguous templates show too few errors
    plain[0].add(s)
    assert not PS.accept(plain[0].results())[0]


def families(RL, name):
    """Hypotheses of the GPU case that runs a statistic over every column (upper bounds: a degenerate column tests less)."""
    C = 2 * RL
    return {"S2": C * (C - 1) // 2, "S3": len(PS.structural_pairs(name, RL)), "S4": len(PS.LAGS) * C * C,
            "S6": C * C + C * (C - 1) // 2, "S7": 8}


MEANT_FOR = {"a": "S2", "b": "S3", "c": "S2", "d": "S4", "e": "S6", "f": "S6", "g": "S7", "ha": "S3", "hf": "S6"}
MARGIN = 100.0  # a defect counts as rejected where its p-value is this factor inside the bound: another seed would not flip it


@pytest.mark.parametrize("name", MODELS)
def test_every_planted_defect_is_rejected(name):
    """At N_PAIRS[name] pairs of ``sample_model`` every defect of ``plant`` (but those listed in DROPPED) is rejected by the
    statistic meant for it, against the bound of the whole family the GPU case tests -- and at half that size one is not:
    N_PAIRS is the smallest such power of two."""
    d = dense_model(name, indel=(0.0, 0.0))
    RL = d.read_length
    x, genome = PS.Expect(d), random_genome(5, GENOME)
    (_, a), (_, b) = PS.structural_pairs(name, RL)[0]
    pos, fam = [a, b], families(RL, name)

    def verdicts(n):
        base = PS.sample_model(d, n, np.random.RandomState(100 + n.bit_length() - 1), genome, positions=pos, keep=True)
        out = {}
        for defect in (None,) + PS.DEFECTS:
            if defect in PS.DROPPED[name]:
                continue
            s = base if defect is None else PS.plant(d, base, defect)
            for key in ("S2", "S3", "S4", "S6", "S7") if defect is None else (MEANT_FOR[defect],):
                st = {"S2": lambda: PS.S2(d, pos, x), "S3": lambda: PS.S3(d, [((0, a), (0, b))], pos, x), "S4": lambda: PS.S4(d, pos, x),
                      "S6": lambda: PS.S6(d, pos, x), "S7": lambda: PS.S7(d, pos, x)}[key]()
                st.add(s)
                res = st.results()
                out[(defect, key)] = (PS.accept(res, alpha=PS.ALPHA / (1.0 if defect is None else MARGIN), m=fam[key])[0], min(r.p for r in res))
        return out

    n = PS.N_PAIRS[name]
    got = verdicts(n)
    print(name, n, {k: "%.3g" % v[1] for k, v in got.items()})
    for (defect, key), (ok, p) in got.items():
        if defect is None:
            assert ok, ("the undamaged sample is rejected", key, p)
        else:
            assert not ok, ("defect %s is not rejected by %s at %d pairs" % (defect, key, n), p)
    half = verdicts(n >> 1)
    assert any(ok for (defect, _), (ok, _) in half.items() if defect is not None), "N_PAIRS is not the smallest size"


def test_chi_square_pools_until_every_cell_expects_five():
    """Cells merge in ascending order of expectation (the function asserts that every merged cell expects at least 5); under the
    null the p-values of tables with many tiny cells are uniform, and a count where the model has no mass is a rejection."""
    rng = np.random.RandomState(7)
    pmf = np.concatenate([rng.gamma(0.2, size=300) * 1e-4, rng.random_sample(6)])
    pmf /= pmf.sum()
    ps = []
    for _ in range(400):
        stat, df, p = PS.chi_square(rng.multinomial(20000, pmf), 20000 * pmf)
        assert 5 <= df < 306
        ps.append(p)
    ps = np.asarray(ps)
    assert ps.min() > 1e-5 and 0.4 < ps.mean() < 0.6 and 0.03 < (ps < 0.1).mean() < 0.2
    assert PS.chi_square([10, 0, 3], [6.5, 6.5, 0.0])[2] == 0.0
    assert PS.chi_square([3, 2], [2.0, 3.0]) == (0.0, 0, 1.0)  # nothing to test: one pooled cell
    stat, df, p = PS.chi_square([50, 50, 1, 2], [48.0, 49.0, 3.0, 3.0])  # 3 + 3 pooled, then two cells of their own
    assert df == 2 and abs(stat - (4 / 48.0 + 1 / 49.0 + 9 / 6.0)) < 1e-12


def test_fragment_pmf_truncates_toward_zero():
    """``int(normal(mu, sd)) - 2 RL``: the cell of fragment length 0 is two units wide, negative lengths round up."""
    ins, pmf = PS.fragment_pmf(1.0, 3.0, 2, -20, 20)
    assert abs(pmf.sum() - 1.0) < 1e-9
    draws = np.trunc(np.random.RandomState(3).normal(1.0, 3.0, 400_000)).astype(np.int64) - 4
    obs = np.bincount(draws + 20, minlength=41)[:41]
    assert PS.chi_square(obs, 400_000 * pmf)[2] > 1e-4
    assert pmf[list(ins).index(-4)] > 1.5 * pmf[list(ins).index(-5)]  # the double cell at fragment length 0


def test_expectations_are_distributions():
    for name in MODELS:
        x = PS.Expect(dense_model(name))
        assert np.allclose(x.marg.sum(axis=2), 1.0) and np.allclose(x.w.sum(axis=1), 1.0)
        assert np.allclose(x.alt_pmf.sum(axis=3), 1.0) and abs(x.isize_pmf.sum() - 1.0) < 1e-9
        assert np.abs(np.einsum("opk,opk->op", x.marg, x.score)).max() < 1e-12  # a score has mean 0 under its marginal
