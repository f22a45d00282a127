"""tests/table_edges.py without a GPU: for every case the restated draws, inverted with np.searchsorted on the f64 CDFs, equal the
oracle on every pair (insert size, both bins through the phreds, every phred, every substitution and its letter); the ledger of
the draws meets its floor in every class the case names, and its counts are the literal numbers below (a change of the generator,
the address map or the tables is seen); the model passes validate().  Plus one hand-checked row per quality row type, and the
refusal of a bin CDF that ends below 1.0 over an empty last bin."""
import numpy as np
import pytest

import table_edges as E
from helpers import synthetic_model
from insilicoseq_amd.model import DenseModel, ModelError

# the ledger of every case, in the order of table_edges.named(case); Q9: then the classes of DROPPED (below the floor at 2^16 pairs)
LEDGER = {
    "Q33-6": (943, 497, 412, 34, 25556, 46, 72, 13, 66327, 8506, 2546, 267, 1773, 10),
    "Q33-7": (841, 430, 385, 26, 9032, 36, 74, 13, 66327, 8325, 2610, 267, 555, 10),
    "Q33-8": (878, 424, 428, 26, 2872, 37, 72, 13, 66327, 8368, 2598, 267, 380, 10),
    "Q33-6-mixed": (943, 497, 412, 34, 25556, 46, 72, 13, 66327, 8506, 2546, 267, 1775, 10),
    "Q65-6": (1156, 578, 544, 34, 12591, 85, 93, 11, 8965, 8300, 5134, 40, 343, 16),
    "Q65-7": (1067, 532, 504, 31, 4070, 79, 99, 11, 8965, 8249, 4886, 40, 129, 16),
    "Q65-8": (1047, 535, 475, 37, 1467, 89, 98, 11, 8965, 8305, 4951, 40, 132, 16),
    "Q9": (46, 28, 18, 162, 11, 39710, 4583, 2032, 2032, 146, 469, 10) + (0, 4, 4, 0),
    "S33": (183, 185, 21, 60, 986),
    "I33-0": (4086, 4106), "I33-1": (), "I33-2": (1417,), "I33-3": (4806, 4106),
    "B33-0": (6465,), "B33-1": (7381,), "B33-2": (16384,), "B33-3": (3253, 8192),
}


def test_every_case_is_pinned():
    assert sorted(LEDGER) == sorted(E.PHILOX_CASES)


@pytest.mark.parametrize("cid", E.PHILOX_CASES)
def test_restated_draws_equal_the_oracle_and_reach_the_edges(cid):
    c = E.case(cid)
    c.dense.validate()
    assert c.dense.read_length == c.RL and c.dense.n_q == c.n_q
    d, exp = E.case_draws(cid), E.oracle_rows(cid)
    r = E.restate(c.dense, d, c.genome, exp["coords"])
    assert np.array_equal(r["isize"], exp["coords"][:, 3]), "insert sizes"
    for o, (kq, kb) in enumerate((("r1_qual", "r1_base"), ("r2_qual", "r2_base"))):
        bad = np.argwhere(r["phred"][:, o] != exp[kq])
        assert bad.size == 0, (kq, bad[:5].tolist(), len(bad))  # (a wrong bin shows here: the rows of the four bins differ)
        bad = np.argwhere(r["bases"][:, o] != exp[kb])
        assert bad.size == 0, (kb, bad[:5].tolist(), len(bad))
    L, exact = E.ledger(c.info, d, r["bi"])
    # the integer thresholds and the f64 CDFs invert alike (DenseModel.device_tables' claim, on these tables)
    assert np.array_equal(exact["isize"], r["isize"]) and np.array_equal(exact["bins"], r["bins"])
    assert np.array_equal(exact["phred"], r["phred"])
    names = E.named(cid)
    low = {k: L[k] for k in names if L[k] < E.FLOOR}
    assert not low, (cid, "classes below the floor", low)
    dropped = E.DROPPED.get(cid.split("-")[0], ())
    assert tuple(L[k] for k in names + dropped) == LEDGER[cid], (cid, [(k, L[k]) for k in names + dropped])
    assert all(L[k] < E.FLOOR for k in dropped), "a dropped class reaches the floor: name it"


def test_the_cases_hold_what_they_are_named_for():
    """Every quality row type on every Q case (Q33, Q65: at either mate; Q9 has 36 rows a mate); the phred thresholds of the two
    clamp cases; the shapes."""
    for cid in ("Q33-6", "Q65-8", "Q9"):
        info = E.case(cid).info
        for types in ([info["q_type"]] if cid == "Q9" else info["q_type"]):
            assert set(int(x) for x in np.unique(types)) == set(range(len(E.ROW_TYPES))), cid
        short = info["q_type"] == E.ROW_TYPES.index("short")
        assert (info["q_thr"][short][:, -1] < E.TWO53).all() and (info["q_thr"][~short][:, -1] == E.TWO53).all()
    assert E.case("Q65-6").info["mut_thr"][60] == 0 and E.case("Q9").info["mut_thr"][0] == E.TWO53
    s = E.case("S33").info
    assert set(np.unique(s["s_type"])) == set(range(len(E.SUBST_TYPES)))
    assert [len(E.case("I33-%d" % k).info["isize_thr"]) for k in range(4)] == [1, 7, 8000, 8000]
    assert E.case("I33-3").info["isize_thr"][-1] == E.TWO53 // 2 and E.case("B33-3").info["bin_thr"][0, 3] == 8 * E.TWO53 // 10


def _m(digit, low):
    return (digit << 37) | low


ONE = E.TWO53
LOW = (1 << 37) - 1
# row type -> (thresholds as (leading digit, trailing 37 bits) or ONE, [(draw digit, trailing bits, expected phred)])
HAND_ROWS = {
    "gamma": ([(100, 0), (200, 5), (300, 0), (400, 0), ONE], [(199, LOW, 1), (200, 5, 1), (200, 6, 2), (201, 0, 2)]),
    "boundary": ([(1023, 7), (1024, 7), ONE], [(1022, LOW, 0), (1023, 7, 0), (1023, 8, 1), (1024, 7, 1), (1024, 8, 2), (1025, 0, 2)]),
    "cluster": ([(2049, 1), (2050, 1), (2051, 1), (2052, 1), ONE], [(2048, LOW, 0), (2050, 1, 1), (2050, 2, 2), (2053, 0, 4)]),
    "ones_early": ([(50, 0), (60, 0), ONE, ONE, ONE], [(59, LOW, 1), (60, 0, 1), (60, 1, 2), (0xFFFF, LOW, 2)]),
    "zeros_lead": ([(0, 0), (0, 0), (70, 9), (80, 0), ONE], [(0, 0, 0), (0, 1, 2), (70, 9, 2), (70, 10, 3), (71, 0, 3)]),
    "duplicates": ([(90, 3), (90, 3), (90, 3), (95, 0), ONE], [(89, LOW, 0), (90, 3, 0), (90, 4, 3), (91, 0, 3)]),
    "same_digit": ([(500, 10), (500, 20), (500, 30), (500, 40), ONE], [(499, LOW, 0), (500, 10, 0), (500, 11, 1), (500, 25, 2),
                                                                        (500, 41, 4), (501, 0, 4)]),
    "constant": ([ONE, ONE, ONE, ONE, ONE], [(0, 0, 0), (0x8000, 1, 0), (0xFFFF, LOW, 0)]),
    "constant-zero": ([(0, 0), (0, 0), (0, 0), (0, 0), ONE], [(0, 0, 0), (0, 1, 4), (0xFFFF, LOW, 4)]),
    "short": ([(100, 0), (200, 0), (300, 0), (400, 0), (0xE666, 5)], [(0xE665, LOW, 4), (0xE666, 5, 4), (0xE666, 6, 5), (0xFFFF, LOW, 5)]),
}


@pytest.mark.parametrize("kind", sorted(HAND_ROWS))
def test_hand_checked_row(kind):
    """Draws below, on and above a threshold of a hand-made row of each type, with the phred written out: the f64 inversion
    of restate() and the integer count of ledger() both give it."""
    row, probes = HAND_ROWS[kind]
    T = np.array([t if t == ONE else _m(*t) for t in row], dtype=np.int64)
    cdf = T / float(E.TWO53)
    assert np.array_equal(np.floor(cdf * E.TWO53).astype(np.int64), T) and (np.diff(T) >= 0).all()
    for digit, low, phred in probes:
        m = _m(digit, low)
        assert int(np.searchsorted(cdf, m / float(E.TWO53), "left")) == phred, (kind, digit, low)
        assert int((T < m).sum()) == phred, (kind, digit, low)


def test_generated_rows_are_of_their_type():
    rng = np.random.RandomState(5)
    for gb in E.GUIDE_BITS:
        W = 1 << (16 - gb)
        for n_q in (3, 41, 60):
            rows = {k: E.quality_row(k, n_q, rng, W) for k in E.ROW_TYPES}
            for k, T in rows.items():
                assert len(T) == n_q and (np.diff(T) >= 0).all() and T[0] >= 0 and T[-1] <= E.TWO53, k
                assert (T[-1] < E.TWO53) == (k == "short"), k
            d = rows["boundary"][:-1] >> 37
            assert (((d % W) == 0) | ((d % W) == W - 1)).all()
            d = rows["cluster"][:-1] >> 37
            assert len(set(d // W)) == 1 and len(set(d)) == n_q - 1
            assert (rows["ones_early"][n_q // 2:] == E.TWO53).all() and (rows["zeros_lead"][:n_q // 2] == 0).all()
            d = rows["same_digit"][:-1]
            assert len(set(d)) == n_q - 1 and len(set(d >> 37)) == (n_q - 1 + 3) // 4
            assert len(set(rows["duplicates"][:-1])) == (n_q - 1 + 2) // 3
            assert set(rows["constant"][:-1]) <= {0, E.TWO53} and len(set(rows["constant"][:-1])) == 1


def test_philox_restatement_matches_the_oracles_generator():
    """The numpy Philox4x32 against the oracle's, 7 and 10 rounds."""
    from oracle import oracle as O

    rng = np.random.RandomState(9)
    ctr = rng.randint(0, 2**32, size=(50, 4), dtype=np.uint64)
    key = int(rng.randint(0, 2**62))
    for rounds in (7, 10):
        got = np.stack(E.philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key, rounds), axis=1)
        for i in range(len(ctr)):
            exp = O.philox4x32([int(x) for x in ctr[i]], [key & 0xFFFFFFFF, key >> 32], rounds)
            assert [int(x) for x in got[i]] == [int(x) for x in exp], (rounds, i)


# ------------------------------------------------------------------ the refusal: a bin CDF that ends below 1.0 over an empty last bin
def test_validate_refuses_a_short_bin_cdf_over_an_empty_last_bin():
    """Such a model sends a tenth of the draws to bin 3 (the clamp of kde.py:77-78), which has no histograms; np.random.choice
    refuses its probabilities.  A short CDF over a last bin WITH histograms (the clamp proper) and a full CDF over an empty last
    bin stay valid."""
    d = synthetic_model(20, 5, 7, seed=1, nonempty=((1, 1, 0, 0), (1, 1, 1, 1)))
    d.validate()
    d.bin_cdf[0] = [0.5, 0.9, 0.9, 0.9]
    with pytest.raises(ModelError, match="ends below 1.0"):
        d.validate()
    with pytest.raises(ModelError, match="ends below 1.0"):
        DenseModel(d.read_length, d.isize_cdf, d.bin_cdf, d.bin_nonempty, d.qcdf, d.subst_cdf, d.subst_alt, d.ins, d.ins_letter,
                   d.dele, d.phred_thr)
    d.bin_cdf[0] = [0.5, 1.0, 1.0, 1.0]
    d.validate()
    d.bin_cdf[1] = [0.2, 0.4, 0.6, 0.8]
    d.validate()
    d.bin_cdf[1] = [0.2, 0.4, 0.6, np.nan]
    d.bin_nonempty[1] = [1, 1, 1, 0]
    with pytest.raises(ModelError):
        d.validate()
