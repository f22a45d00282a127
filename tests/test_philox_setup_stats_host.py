"""tests/philox_setup_stats.py, held to its own contract without a GPU: the rule C0 by hand at its edges; the statistics accept
the plain sampler on every case at its GPU size, the oracle's reference-compatible (MT) sample -- byte-equal to the reference, so
it ties the rule, the side of every search and the truncation of a custom fragment length to what the reference does -- and the
oracle's Philox sample; and they reject every planted defect at the recorded sizes, by the statistic meant for it, while half
the size leaves one standing.

Oracle legs (about 30 us a pair): 2^14 pairs per case and mode, 2^16 for the two runs of a gc_bias case in Philox mode (G1's
null needs that many, see philox_setup_stats.SIZED_BY_VALIDITY)."""
import numpy as np
import pytest

import philox_setup_stats as SS
import philox_stats as PS

ORACLE_PAIRS = 1 << 14
ORACLE_GC_PAIRS = 1 << 16
MARGIN = 100.0  # a defect counts as rejected where its p-value is this factor inside the bound: another seed would not flip it


def _accepted(results, m=None):
    ok, text = PS.accept(results, m=m)
    assert ok, text


# ------------------------------------------------------------------ C0 by hand
def _rule(rows, L, RL, sequence_type="metagenomics"):
    return SS.pair_rule(np.asarray(rows, dtype=np.int64).reshape(-1, 4), L, RL, sequence_type)


def _violates(row, L, RL, sequence_type="metagenomics"):
    with pytest.raises(AssertionError, match="C0: pair 0"):
        _rule([row], L, RL, sequence_type)


def test_pair_rule_at_the_widths_around_zero():
    L, RL = 100, 10
    s = L - 2 * RL - 1  # width 1: the start is randrange(0, 1)
    r = _rule([(0, L - 1 - RL, L - 1, s)], L, RL)
    assert r.regular[0] and not r.fell[0] and r.n1[0] == 1
    _violates((1, L - RL, L, s), L, RL)
    s = L - 2 * RL  # width 0: randrange(0, 0) raises, the start is randrange(0, L - RL); fs == 0 ends at L and does not fall back
    r = _rule([(0, L - RL, L, s), (3, 40, 50, s), (L - RL - 1, 0, RL, s)], L, RL)
    assert not r.regular.any() and r.fell.tolist() == [False, True, True] and (r.n1 == L - RL).all()
    _violates((0, 40, 50, s), L, RL)  # fell back where nothing asks for it
    _violates((3, L - RL + 3, L + 3, s), L, RL)  # the natural end beyond the record, kept
    _violates((L - RL, 40, 50, s), L, RL)  # fs == n1
    s = L - 2 * RL + 1  # width -1: every pair falls back
    r = _rule([(0, 0, RL, s), (5, L - 1 - RL, L - 1, s)], L, RL)
    assert r.fell.all() and not r.regular.any()
    _violates((0, L - RL, L, s), L, RL)  # randrange(RL, L) never gives L
    _violates((0, -1, RL - 1, s), L, RL)  # nor RL - 1


def test_pair_rule_on_a_record_one_base_longer_than_a_read():
    L, RL = 11, 10  # n = 1 in both loops: fs = 0, re = RL
    r = _rule([(0, 0, RL, 0), (0, 0, RL, 7)], L, RL)
    assert r.fell.all() and (r.n1 == 1).all() and not r.irregular.any()
    _violates((1, 0, RL, 0), L, RL)
    _violates((0, 1, RL + 1, 0), L, RL)
    with pytest.raises(AssertionError):
        _rule([(0, 0, RL, 0)], RL, RL)  # generator.py:130


def test_pair_rule_at_fragment_lengths_around_zero():
    L, RL = 100, 10
    for frag in (-1, 0, 1):
        s = frag - 2 * RL  # width = L - frag: the start may stand at or beyond the record's end
        fs = L - frag - 1
        r = _rule([(fs, fs + frag - RL, fs + frag, s), (0, frag - RL, frag, s)], L, RL)
        assert r.regular.all() and not r.fell.any() and r.irregular.all() and (r.n1 == L - frag).all()
        _violates((L - frag, L - RL, L, s), L, RL)
        _violates((0, frag - RL + 1, frag + 1, s), L, RL)


def test_pair_rule_names_the_irregular_pairs():
    L, RL = 100, 10
    rows = []
    for rs in (-1, 0):  # a reverse start before the record / at its first base
        re = rs + RL
        rows.append((2, rs, re, re - 2 - 2 * RL))
    for fe in (L, L + 1):  # a forward template that ends with the record / one base beyond
        fs, frag = fe - RL, 5
        rows.append((fs, fs + frag - RL, fs + frag, frag - 2 * RL))
    r = _rule(rows, L, RL)
    assert r.irregular.tolist() == [True, False, False, True] and not r.fell.any()
    _violates((2, 0, RL - 1, RL - 1 - 2 - 2 * RL), L, RL)  # rs != re - RL


def test_pair_rule_for_amplicons():
    L, RL = 100, 10
    r = _rule([(0, L - RL, L, 5), (0, L - RL, L, 500)], L, RL, "amplicon")
    assert not r.fell.any()
    _violates((1, L - RL, L, 5), L, RL, "amplicon")
    _violates((0, 30, 40, 500), L, RL, "amplicon")


def test_bins_count_values():
    """#{v < w in bin b} against the bins of every value, widths from 1 on."""
    for nb in (8, 64):
        for w in list(range(1, 200)) + [255, 256, 257, 642, 399_547]:
            got = SS.bin_counts(w, nb)[0]
            assert (got == np.bincount(SS.bin_of(np.arange(w), w, nb), minlength=nb)).all() and got.sum() == w
    p = SS.bin_probs([5, 5], 8, [0, 1])
    assert np.allclose(p.sum(axis=1), 1.0) and p[1, 0] == 0.0 and p[0, 0] == 0.2


def test_randbelow_is_cpythons():
    """k = n.bit_length(), candidates word >> (32 - k), the first below n: against random.Random, which takes the same words."""
    import random

    r = random.Random(5)
    state = random.Random(5)
    for n in (1, 2, 3, 64, 96, 97, 642, 399_547, 2**31 + 5):
        words = np.array([[state.getrandbits(32) for _ in range(SS.WORDS)]], dtype=np.uint32)
        got, rejected = SS._randbelow(words, np.array([n]))
        assert got[0] == r.randrange(0, n)
        for _ in range(SS.WORDS - 1 - int(rejected[0])):  # (line both generators up again)
            r.getrandbits(32)


# ------------------------------------------------------------------ the sampler, the oracle
@pytest.mark.parametrize("case", list(SS.CASES))
def test_the_statistics_accept_the_sampler(case):
    """Every case at its GPU size, one family."""
    res = SS.run_sampler(case, SS.N_PAIRS[case], seed=2024)
    _accepted([r for v in res.values() for r in v])


def _oracle_slices(case, mode, n, gc_bias, step=1 << 13, seed=77):
    from oracle import oracle as O

    O.build()
    c = SS.CASES[case]
    dense, genome, geo = SS.case_setup(case)
    rng = O.Rng().seed_mt(seed) if mode == "mt" else O.Rng().seed_philox(seed)
    kw = dict(fragment_length=c.fragment[0], fragment_sd=c.fragment[1]) if c.fragment else {}
    rows = O.Oracle(dense).simulate(rng, genome, n, want_coords=True, gc_bias=gc_bias, **kw)
    assert rows["status"] == 0 and rows["n_done"] == n
    want_rows = c.gc or "C6" in c.stats
    out = []
    for a in range(0, n, step):
        coords = rows["coords"][a:a + step]
        out.append(PS.slice_of({k: v[a:a + step] for k, v in rows.items() if k.startswith("r")}, coords, genome, dense.read_length)
                   if want_rows else {"coords": coords})
    return dense, geo, out


@pytest.mark.parametrize("mode", ["mt", "philox"])
@pytest.mark.parametrize("case", [c for c in SS.CASES if not SS.CASES[c].gc])
def test_the_statistics_accept_the_oracle(case, mode):
    dense, geo, slices = _oracle_slices(case, mode, ORACLE_PAIRS, False)
    stats = SS.case_stats(case, dense, geo, None, SS.CASES[case].mixed)
    for s in slices:
        for st in stats:
            st.add(s)
    _accepted([r for st in stats for r in st.results()])


@pytest.mark.parametrize("case", [c for c in SS.CASES if SS.CASES[c].gc])
def test_the_statistics_accept_the_oracle_with_gc_bias(case):
    """Philox mode: G1 on the plain and the gc_bias run of one seed.  MT mode: the two runs share no draw (one stream, drawn in
    order), so the gc_bias run goes through C0 .. C3 alone."""
    dense, geo, plain = _oracle_slices(case, "philox", ORACLE_GC_PAIRS, False)
    _, _, gc = _oracle_slices(case, "philox", ORACLE_GC_PAIRS, True)
    g1 = SS.G1(dense, geo)
    for a, b in zip(plain, gc):
        g1.add({"a": a, "b": b})
    res = g1.results()
    assert 0.88 < g1.k / float(g1.n) < 0.92
    _accepted(res)
    _, _, mt = _oracle_slices(case, "mt", ORACLE_PAIRS, True)
    stats = [SS.C1(geo), SS.C2(geo), SS.C3(geo)]
    for s in mt:
        for st in stats:
            st.add({"coords": s["coords"]})
    _accepted([r for st in stats for r in st.results()])


def test_the_oracle_takes_every_branch_the_cases_claim():
    """The shares the cases are built for, on the oracle's Philox sample: all of a fallback case falls back, about half of a
    mixed one; negative inserts, irregular pairs and fragment lengths of 0 and below where the fragment is cut."""
    shares = {}
    for case in ("fallback-pow2", "fallback-3q", "mixed-hiseq", "mixed-miseq", "fragment-overlap", "fragment-cut"):
        dense, geo, slices = _oracle_slices(case, "philox", ORACLE_PAIRS, False)
        coords = np.concatenate([s["coords"] for s in slices])
        shares[case] = SS.shares(geo, coords) + (float((coords[:, 3] < 0).mean()), float((coords[:, 3] + 2 * dense.read_length <= 0).mean()))
    print(shares)
    assert shares["fallback-pow2"][:2] == (0.0, 1.0) and shares["fallback-3q"][:2] == (0.0, 1.0)
    for case in ("mixed-hiseq", "mixed-miseq"):
        assert 0.3 < shares[case][0] < 0.7 and abs(shares[case][0] + shares[case][1] - 1.0) < 0.01
    assert 0.2 < shares["fragment-overlap"][3] < 0.4 and shares["fragment-overlap"][2] == 0.0
    assert shares["fragment-cut"][3] > 0.999 and 0.25 < shares["fragment-cut"][2] < 0.45 and 0.02 < shares["fragment-cut"][4] < 0.08


# ------------------------------------------------------------------ the defects
def _verdicts(case, n):
    """{(defect, statistic): (accepted, smallest p)}: the undamaged sample against the case's family, every defect of the case
    by the statistic meant for it against the same family, a factor MARGIN inside."""
    dense, _, _ = SS.case_setup(case)
    fam = SS.family(case, dense.read_length)
    out = {}
    clean = SS.run_sampler(case, n)
    out[(None, "all")] = (PS.accept([r for v in clean.values() for r in v], m=fam)[0], min(r.p for v in clean.values() for r in v))
    for defect, key in SS.CASES[case].defects:
        if defect in SS.DROPPED.get(case, ()):
            continue
        res = SS.run_sampler(case, n, defect)[key]
        out[(defect, key)] = (PS.accept(res, alpha=PS.ALPHA / MARGIN, m=fam)[0], min(r.p for r in res))
    return out


@pytest.mark.parametrize("case", list(SS.CASES))
def test_every_planted_defect_is_rejected(case):
    """At N_PAIRS[case] pairs of ``sample_setup`` every defect of the case is rejected by the statistic meant for it, against
    the bound of the whole family the GPU case tests -- and at half that size one is not: N_PAIRS is the smallest such power
    of two.  The gc_bias cases are sized by the validity of G1's null instead (SIZED_BY_VALIDITY): there the half size is not
    looked at."""
    n = SS.N_PAIRS[case]
    got = _verdicts(case, n)
    print(case, n, {k: "%.3g" % v[1] for k, v in got.items()})
    for (defect, key), (ok, p) in got.items():
        if defect is None:
            assert ok, ("the undamaged sample is rejected", p)
        else:
            assert not ok, ("defect %s is not rejected by %s at %d pairs" % (defect, key, n), p)
    if case not in SS.SIZED_BY_VALIDITY:
        half = _verdicts(case, n >> 1)
        print(case, n >> 1, {k: "%.3g" % v[1] for k, v in half.items()})
        assert any(ok for (defect, _), (ok, _) in half.items() if defect is not None), "N_PAIRS is not the smallest size"


def test_plant_damages_the_same_words():
    """``plant`` re-derives a sample from its own raw material: with (q) every reverse end is the start's word again, with (r)
    the rule still holds; and the case is what it says -- n = 64 has k = 7, half of all candidates are rejected, and one pair in
    sixteen rejects four and reaches the second block of four words."""
    from scipy import stats as sps

    dense, genome, geo = SS.case_setup("fallback-pow2")
    RL, n = dense.read_length, 1 << 14
    s = SS.sample_setup(dense, n, 3, genome)
    assert SS.pair_rule(s["coords"], geo.L, RL).fell.all()
    q = SS.plant(s, "q")["coords"]
    assert (q[:, 0] == s["coords"][:, 0]).all() and (q[:, 2] == q[:, 0] + RL).all()
    assert (s["coords"][:, 2] == s["coords"][:, 0] + RL).mean() < 0.05
    SS.pair_rule(SS.plant(s, "r")["coords"], geo.L, RL)
    for loop in range(2):
        rejected = s["rejected"][:, loop]
        k = int((rejected >= 4).sum())
        assert min(sps.binom.cdf(k, n, 1 / 16.0), sps.binom.sf(k - 1, n, 1 / 16.0)) > PS.ALPHA, k
        k = int((rejected >= 1).sum())
        assert min(sps.binom.cdf(k, n, 0.5), sps.binom.sf(k - 1, n, 0.5)) > PS.ALPHA, k


def test_every_defect_has_a_case():
    held = {d for c in SS.CASES.values() for d, _ in c.defects} - {d for v in SS.DROPPED.values() for d in v}
    assert held == set(SS.DEFECTS)
