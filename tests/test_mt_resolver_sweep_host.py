"""The cases of tests/mt_resolver_cases.py are what their comments say -- from the CPU oracle and numpy alone, no GPU.

Per case, from the oracle's MT sample: the call is complete, at most a fifth of its pairs touch an N (the condition under which
the GPU test may demand that three pairs in four were resolved), and its flavour holds (clean: the first guess of the second
mate's numpy offset mostly holds; noisy: it never does; worst: every ACGT base is substituted).  The two cases with indel rates
really have a few dozen reads with an insertion or a deletion, and stay below the bounce rate that keeps the resolver eligible.

For the worst flavour the words a pair takes from the two streams are measured from the oracle's stream positions, one pair at a
time, and held to what the arrays say -- numpy words: 2 (insert size) + per mate 2 (bin) + 2 RL (phreds) + 2 per substitution
+ 2 per gc draw -- and to the two `need` formulas the rings of k_mt_resolve are sized by, restated here.  Their maximum is
8 RL + 6 without a custom fragment length (2 + 2 (2 + 4 RL)); with one, the insert-size draw is the polar loop's 4 words a round,
every second pair, and with the gc draw a full pair after one round takes 8 RL + 10.

The pick table: mt_pick_resolver restated in a few lines reproduces every case's literal; over every model the engine takes
(RL 2 .. 1024, 1 .. 4 bin slots, n_q 1 .. 60, 1 .. 4096 insert sizes) it never picks (4, 4, rows), (4, 2, no rows) or
(4, 4, no rows), which is why ISS_MT_RESOLVERS -- read from the source here -- holds five instantiations and not eight."""
import os
import re

import numpy as np
import pytest

import mt_resolver_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------ the rule, restated (iss_api_mt.hip.h, iss_mt_compat.hip.h)
LDS_BUDGET = 160 * 1024 - 256
ALL_EIGHT = tuple((py, nw, rows) for rows in (True, False) for (py, nw) in ((8, 2), (4, 2), (8, 4), (4, 4)))  # rows in LDS first


def need_py(RL):
    return 24 * RL + 236  # 256 + 2 * (10 * (RL - 1) + 2 * RL) python words: a pair's two mates and its randrange candidates


def need_np(RL):
    return 8 * RL + 80  # 16 + 64 (polar loop) + 8 RL numpy words


def row_words(n_q):
    w = (n_q + 2) // 2  # n_q 16-bit digits and at least one of padding, in an odd number of 32-bit words
    return w if w % 2 else w + 1


def lds_bytes(RL, NB, n_q, n_isize, py_k, np_k, rows):
    b = (2 * py_k + 2 * np_k) * 1024 * 4 + 2 * 16 * 4  # two rings of two halves, their 16-word mirrors
    b += (64 + 8 + n_isize) * 8 + 2 * RL * 5 * 4 + 16 * 4  # thresholds, indel limits, scratch
    return b + (2 * NB * RL * row_words(n_q) * 4 if rows else 0)


def pick(RL, NB, n_q, n_isize, candidates):
    """The first candidate whose ring halves hold a whole pair and whose LDS fits; None: the walker only."""
    for (py_k, np_k, rows) in candidates:
        if need_py(RL) <= py_k * 1024 and need_np(RL) <= np_k * 1024 and lds_bytes(RL, NB, n_q, n_isize, py_k, np_k, rows) <= LDS_BUDGET:
            return (py_k, np_k, rows)
    return None


def source_candidates():
    text = open(os.path.join(ROOT, "insilicoseq_amd", "csrc", "iss_api_mt.hip.h")).read()
    line = re.search(r"#define ISS_MT_RESOLVERS\(X\)(.*)", text).group(1)
    return tuple((int(a), int(b), r == "true") for a, b, r in re.findall(r"X\((\d+), (\d+), (true|false)\)", line))


def test_the_source_holds_the_reachable_instantiations_in_order():
    assert source_candidates() == M.REACHED
    assert [c for c in ALL_EIGHT if c in M.REACHED] == list(M.REACHED)  # (the order of preference is unchanged)


def test_pick_table_is_reproduced_by_the_rule():
    for c in M.CASES:
        for cands in (ALL_EIGHT, M.REACHED):
            assert pick(c.RL, c.NB, c.n_q, M.N_ISIZE, cands) == c.pick, c.id
    assert {c.pick for c in M.CASES} == set(M.REACHED) | {None}
    assert {M.case(cid).pick for cid in M.WORKER_CASES} == set(M.REACHED)
    # the boundaries the case table names, for 41 phreds: every length at which the pick changes has a case on either side
    for NB in (1, 2, 4):
        changes = [RL for RL in range(3, 400) if pick(RL, NB, 41, M.N_ISIZE, ALL_EIGHT) != pick(RL - 1, NB, 41, M.N_ISIZE, ALL_EIGHT)]
        assert changes == {1: [247, 309, 332], 2: [215, 247, 332], 4: [114, 160, 247, 332]}[NB]
        have = {c.RL for c in M.CASES if c.NB == NB and c.n_q == 41}
        for RL in changes:
            # (332, the end of the python ring, is the same at every bin layout: one slot; 247 at two slots: one and four)
            assert RL == 332 or NB == 2 and RL == 247 or {RL - 1, RL} <= have, (NB, RL)
    assert {331, 332} <= {c.RL for c in M.CASES if c.NB == 1}
    # zero slack: 246 positions fill a numpy half to the word, 331 leave 12 words of a python half
    assert need_np(246) == 2048 and need_np(247) > 2048 and need_py(331) == 8192 - 12 and need_py(332) > 8192 and need_py(160) == 4076


def test_three_of_the_eight_are_never_picked():
    """Over every model the engine takes.  The LDS need grows with n_isize, so candidate k is picked on an interval of n_isize: from
    one past the largest n_isize an earlier eligible candidate fits, to the largest it fits itself."""
    reached = set()
    for RL in range(2, 1025):
        eligible = [c for c in ALL_EIGHT if need_py(RL) <= c[0] * 1024 and need_np(RL) <= c[1] * 1024]
        for NB in range(1, 5):
            for w in sorted({row_words(n_q) for n_q in range(1, 61)}):
                n_q = next(q for q in range(1, 61) if row_words(q) == w)
                lo = 1  # the smallest n_isize no earlier candidate fits
                for c in eligible:
                    hi = min(4096, (LDS_BUDGET - lds_bytes(RL, NB, n_q, 0, *c)) // 8)
                    if hi >= lo:
                        reached.add(c)
                        assert pick(RL, NB, n_q, lo, ALL_EIGHT) == c and pick(RL, NB, n_q, hi, ALL_EIGHT) == c
                        lo = hi + 1
    assert reached == set(M.REACHED)
    assert set(ALL_EIGHT) - reached == {(4, 4, True), (4, 2, False), (4, 4, False)}


# ------------------------------------------------------------------ the cases, from the oracle
def _events(c, res):
    """Substitutions per (pair, mate) from the arrays: read letters that differ from the template (without indels a read is its
    template but for them; an N is never substituted).  Also the templates."""
    fwd, rev = M.templates(c, res["coords"])
    e0, e1 = res["r1_base"] != fwd, res["r2_base"] != rev
    assert not (e0 & (fwd == ord("N"))).any() and not (e1 & (rev == ord("N"))).any()
    return e0, e1, fwd, rev


@pytest.mark.parametrize("cid", [c.id for c in M.CASES])
def test_case_is_what_it_says(cid):
    c = M.case(cid)
    n = M.PAIRS + M.PAIRS_SECOND
    res, _ = M.oracle_sample(c)
    assert res["status"] == 0 and res["n_done"] == n
    touched = M.touches_n(c, res["coords"])
    assert 0 < touched.mean() <= M.TOUCH_CAP, touched.mean()
    if c.indels:
        # about 0.03 indel candidates a pair: a few dozen reads with an insertion or a deletion, every one of them the walker's
        rows = res["mutations"]
        assert {1, 2} <= set(np.unique(rows["type"])) and 20 <= len(M.indel_pairs(rows)) <= 0.05 * n
        # (mt_bounce_rate: four insertion tests and the largest deletion rate a position, each rounded up to 2^-27)
        d = M.model(c)
        assert d.ins.sum() + d.dele.max(axis=2).sum() + 10 * c.RL / 2.0 ** 27 < 0.05
        return
    e0, e1, fwd, rev = _events(c, res)
    quiet = ~e0.any(axis=1)  # forward mates without a substitution
    if c.flavour == "clean":
        assert quiet.mean() >= 0.70, quiet.mean()
        assert min(res["r1_qual"].min(), res["r2_qual"].min()) >= 30
    elif c.flavour == "noisy":
        assert not quiet.any()
    else:
        assert res["r1_qual"].max() == 0 and res["r2_qual"].max() == 0
        assert (e0 == (fwd != ord("N"))).all() and (e1 == (rev != ord("N"))).all()
    rows = res["mutations"]
    assert len(rows) == e0.sum() + e1.sum() and (rows["type"] == 0).all()  # (every substitution of these tables changes the letter)


def test_a_case_of_noisy_tables_is_not_a_worst_case():
    """What the worst flavour asserts fails on the noisy tables of the same model: the flavour is not decoration."""
    c = M.case("RL246-NB1-noisy")
    res, _ = M.oracle_sample(c, n=200)
    e0, e1, fwd, rev = _events(c, res)
    assert res["r1_qual"].max() > 0 and not (e0 == (fwd != ord("N"))).all()
    assert (2 + 2 * (2 + 2 * c.RL) + 2 * (e0.sum(axis=1) + e1.sum(axis=1))).max() < 8 * c.RL + 6


def _pair_by_pair(c, n):
    """n pairs of the case one call at a time: the sample and the (python, numpy) words every pair took."""
    from oracle import oracle as O

    rng, orc = O.Rng().seed_mt(M.MT_SEED), O.Oracle(M.model(c))
    mu, sd = M.fragment(c)
    keys = ("r1_base", "r2_base", "coords")
    got = {k: [] for k in keys}
    used = [rng.words_used()]
    for _ in range(n):
        r = orc.simulate(rng, M.genome(c.RL), 1, fragment_length=mu, fragment_sd=sd, gc_bias=c.gc_frag, want_coords=True)
        assert r["status"] == 0 and r["n_done"] == 1
        for k in keys:
            got[k].append(r[k][0])
        used.append(rng.words_used())
    used = np.diff(np.asarray(used, dtype=np.int64), axis=0)
    return {k: np.stack(v) for k, v in got.items()}, used[:, 0], used[:, 1]


@pytest.mark.parametrize("cid", [c.id for c in M.CASES if c.flavour == "worst" and not c.mutations])
def test_worst_case_words_meet_the_bound_exactly(cid):
    c = M.case(cid)
    RL, n = c.RL, M.PAIRS + M.PAIRS_SECOND
    res, py_w, np_w = _pair_by_pair(c, n)
    whole, _ = M.oracle_sample(c)
    for k in res:  # one pair a call is the same sample
        assert np.array_equal(res[k], whole[k]), k
    e0, e1, _, _ = _events(c, res)
    mates = 2 * (2 + 2 * RL) + 2 * (e0.sum(axis=1) + e1.sum(axis=1))  # numpy words of the two mates, from the arrays
    assert mates.max() == 8 * RL + 4  # a pair that touches no N: one substitution a base
    if not c.gc_frag:
        assert np.array_equal(np_w, 2 + mates)
        assert np_w.max() == 8 * RL + 6 <= need_np(RL)
        # python words of a pair that touches no N: a randrange of one candidate or a few, then 10 (RL - 1) + 2 RL a mate
        plain = ~M.touches_n(c, res["coords"])
        assert (py_w[plain] >= 1 + 2 * (12 * RL - 10)).all() and py_w.max() <= need_py(RL)
    else:
        # a rejected attempt costs a whole pair more; the pairs taken at the first attempt: the polar loop's rounds of 4 words
        # (none when the second value of the last round was kept), the mates, the gc draw
        polar = np_w - mates - 2
        first = polar < 4 * RL
        assert 0.8 * n < first.sum() < n
        assert (polar[first] % 4 == 0).all() and polar[first].min() == 0
        full = first & (mates == 8 * RL + 4)
        assert 8 * RL + 6 in np_w[full] and 8 * RL + 10 in np_w[full]  # the cached value; one round of the loop
        assert np_w[first].max() <= need_np(RL) and polar[first].max() <= 64
        assert 8 * RL + 6 + 64 <= need_np(RL)  # sixteen rounds, past which the resolver hands the pair to the walker
