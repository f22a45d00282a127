"""Edge-built model tables, a plain restatement of the Philox draws, and the ledger of the edges those draws reach.

iss_model_upload compresses five tables on the host, each with hand-made edge rules: the quality rows (merged 16-bit leading
digits, 2^53 clamped to 0xffff, two closing sentinels with phred n_q, padding to s_max, guide bytes), te8 (mut_thr >> 45 clamped
to 255), subst13 (two 13-bit digits clamped to 0x1fff), mt_rows (un-merged digits, 0xffff padding) and the insert-size / bin
thresholds k_setup reads.  The device is held to the oracle byte for byte, so an error in a table shows -- if a draw lands on it.
This module builds tables whose edges draws do land on, and proves it:

* edge_model(): thresholds built as exact integers T in [0, 2^53] and stored as T / 2^53 (exact in f64), so that
  DenseModel.device_tables() gives T back (asserted).
* Draws: a vectorised numpy Philox4x32 and the address map of the oracle's comments (K_PAIR, K_QM, K_QM_LO, K_SUB), giving the
  53-bit numerators of the insert-size, bin, quality, error-test and substitution-choice draws of every base of a call.
  restate() inverts the plain f64 CDFs with np.searchsorted -- never the integer thresholds -- into insert sizes, bins, phreds
  and bases: an independent reference of the oracle (tests/test_table_edges_host.py holds the oracle to it on every pair).
* ledger(): from the numerators and the INTEGER thresholds alone (no library code), how many bases / pairs of a case land on
  each edge class.  FLOOR hits per class a case names, pinned as literal numbers in the host test.

The MT path draws from other streams: the ledger says nothing about its hits (the MT legs run the same tables for mt_rows'
un-clamped-digit and padding rules)."""
import collections

import numpy as np

from helpers import SLOTS_TWO, mixed_genome, random_genome, synthetic_model

TWO53 = 1 << 53
FLOOR = 8  # hits a case must have in every class it names
K_PAIR, K_QM, K_SUB, K_QM_LO = 0, 3, 4, 7
ROW_TYPES = ("gamma", "boundary", "cluster", "ones_early", "zeros_lead", "duplicates", "same_digit", "constant", "short")
# h16 == 0xffff and h16 == 0 are one draw in 65536 each: a class that needs one of them on a given row type gets FLOOR hits from
# the two million bases of a case only if three rows in ten are of that type.  Two such types fit one mix, not three: mix A
# (Q33 and the cases on its shape) has ones_early and short, mix B (Q65) ones_early and zeros_lead.
ROW_WEIGHTS = {"A": (0.04, 0.06, 0.06, 0.29, 0.04, 0.05, 0.12, 0.05, 0.29),
               "B": (0.04, 0.06, 0.06, 0.29, 0.29, 0.05, 0.12, 0.05, 0.04)}
SUBST_TYPES = ("ordinary", "001", "111", "011", "equal", "same_digit", "short")
SEED, FIRST_ORDINAL = 77, 5


# ------------------------------------------------------------------ Philox4x32 and the address map
def philox4x32(c0, c1, c2, c3, key, rounds):
    """Philox4x32-R of counters (arrays that broadcast) under one 64-bit key; four uint32 arrays."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & m32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _block(key, ordinals, kind, index, sub):
    """The block (kind, index, sub) of every pair: counter = (ordinal low, ordinal high 16 bits | attempt 0 << 16,
    kind << 24 | index, sub); 7 rounds for K_QM, 10 for everything else."""
    o = np.asarray(ordinals, dtype=np.uint64)
    return philox4x32(o & np.uint64(0xFFFFFFFF), (o >> np.uint64(32)) & np.uint64(0xFFFF),
                      np.uint64((kind << 24) | index), np.uint64(sub), key, 7 if kind == K_QM else 10)


def _mk53(w0, w1):
    return ((w0 >> np.uint64(5)) << np.uint64(26)) | (w1 >> np.uint64(6))


Draws = collections.namedtuple("Draws", "pair h16 qm e8 em sm")


def draws(seed, first_ordinal, n, RL):
    """The numerators of a call of n pairs.  pair [n, 3]: insert size, forward bin, reverse bin (K_PAIR: word s of sub-blocks 0
    and 1).  Per (pair, mate, position): h16 and qm = h16 << 37 | l37 (quality: the 16-bit half cc & 1 of word
    mate * 2 + (cc >> 1) of K_QM block (p >> 3, 2 * half); l37 from words 0, 1 of K_QM_LO block (p, mate)), e8 and
    em = e8 << 45 | l45 (error test: byte cc of word half * 2 + mate of K_QM block (p >> 3, 1); l45 from words 2, 3 of K_SUB
    block (p, mate)), sm (substitution choice: words 0, 1 of that K_SUB block).  c = p & 7, half = c >> 2, cc = c & 3."""
    ords = np.uint64(first_ordinal) + np.arange(n, dtype=np.uint64)
    a, b = _block(seed, ords, K_PAIR, 0, 0), _block(seed, ords, K_PAIR, 0, 1)
    pair = np.stack([_mk53(a[s], b[s]) for s in range(3)], axis=1)
    h16, qm, e8, em, sm = (np.zeros((n, 2, RL), dtype=np.uint64) for _ in range(5))
    for s in range((RL + 7) // 8):
        blk = [_block(seed, ords, K_QM, s, sub) for sub in range(3)]
        for p in range(8 * s, min(8 * s + 8, RL)):
            c = p & 7
            half, cc = c >> 2, c & 3
            for o in range(2):
                h16[:, o, p] = (blk[2 * half][o * 2 + (cc >> 1)] >> np.uint64(16 * (cc & 1))) & np.uint64(0xFFFF)
                e8[:, o, p] = (blk[1][half * 2 + o] >> np.uint64(8 * cc)) & np.uint64(0xFF)
    for p in range(RL):
        for o in range(2):
            lo, sb = _block(seed, ords, K_QM_LO, p, o), _block(seed, ords, K_SUB, p, o)
            qm[:, o, p] = (h16[:, o, p] << np.uint64(37)) | (lo[0] << np.uint64(5)) | (lo[1] >> np.uint64(27))
            em[:, o, p] = (e8[:, o, p] << np.uint64(45)) | ((sb[2] & np.uint64(0x1FFF)) << np.uint64(32)) | sb[3]
            sm[:, o, p] = _mk53(sb[0], sb[1])
    return Draws(pair, h16, qm, e8, em, sm)


# ------------------------------------------------------------------ the restated simulation (f64 CDFs, np.searchsorted)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTYRWSKMNBVDHacgtyrwskmnbvdh", b"TGCARYWSMKNVBHDtgcarywsmknvbhd"):
    _COMP[_a] = _b
_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[97:123] -= 32
_BASE_INDEX = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate(b"ATCG"):
    _BASE_INDEX[_c] = _i
_AMBIGUOUS = np.zeros(256, dtype=bool)
_AMBIGUOUS[list(b"RYWSMKHBVDN")] = True


def u_of(m):
    return m.astype(np.float64) * (1.0 / 9007199254740992.0)


def restate(dense, d, genome, coords):
    """Insert sizes, bins [n, 2], phreds [n, 2, RL], bases [n, 2, RL] and the substitution mask of the draws `d`, inverted with
    np.searchsorted on the model's f64 CDFs (kde.py:72-85, :97; __init__.py:94-97).  The templates come from the pair
    coordinates (fs, rs, re, insert size) -- the models of this module have no indels."""
    n, RL = d.qm.shape[0], dense.read_length
    isize = np.searchsorted(dense.isize_cdf, u_of(d.pair[:, 0]), "left")
    bins = np.stack([np.minimum(np.searchsorted(dense.bin_cdf[o], u_of(d.pair[:, 1 + o]), "right"), 3) for o in range(2)], axis=1)
    g = np.frombuffer(genome.encode() if isinstance(genome, str) else genome, dtype=np.uint8)
    fs, rs, re = coords[:, 0], coords[:, 1], coords[:, 2]
    assert (fs >= 0).all() and (fs + RL <= len(g)).all() and (rs >= 0).all() and (re == rs + RL).all() and (re <= len(g)).all()
    ar = np.arange(RL)
    bases = np.stack([g[fs[:, None] + ar], _COMP[g[re[:, None] - 1 - ar]]], axis=1)
    phred = np.zeros((n, 2, RL), dtype=np.int64)
    uq = u_of(d.qm)
    for o in range(2):
        for b in np.unique(bins[:, o]):
            sel = np.flatnonzero(bins[:, o] == b)
            for p in range(RL):
                phred[sel, o, p] = np.searchsorted(dense.qcdf[o, b, p], uq[sel, o, p], "left")
    bi = _BASE_INDEX[_UPPER[bases]]
    subst = (u_of(d.em) > dense.phred_thr[phred]) & ~_AMBIGUOUS[_UPPER[bases]]
    assert (bi[subst] >= 0).all()
    us = u_of(d.sm)
    choice = np.zeros((n, 2, RL), dtype=np.int64)
    for o in range(2):
        for p in range(RL):
            for x in range(4):
                sel = np.flatnonzero(subst[:, o, p] & (bi[:, o, p] == x))
                if sel.size:
                    k = np.minimum(np.searchsorted(dense.subst_cdf[o, p, x], us[sel, o, p], "right"), 2)
                    choice[sel, o, p] = k
                    bases[sel, o, p] = dense.subst_alt[o, p, x, k]
    return {"isize": isize, "bins": bins, "phred": phred, "bases": bases, "subst": subst, "bi": bi, "choice": choice}


# ------------------------------------------------------------------ the edge-built tables
def _rand53(rng, k):
    return np.sort(rng.randint(0, TWO53, size=k, dtype=np.int64))


def quality_row(kind, n_q, rng, W):
    """One quality row of n_q integer thresholds, ascending (W = 2^(16 - guide bits) leading digits per guide bucket).  All but
    `short` end at 2^53."""
    k = n_q - 1
    if kind == "gamma":
        w = rng.gamma(0.3, size=n_q) + 1e-12
        t = np.floor(np.cumsum(w) / w.sum() * TWO53).astype(np.int64)[:k]
    elif kind == "boundary":  # leading digits b * W and b * W - 1, random trailing 37 bits
        b = rng.choice(np.arange(1, 65536 // W), size=(k + 1) // 2, replace=False)
        digits = np.concatenate([b * W, b * W - 1])[:k]
        t = (digits.astype(np.int64) << 37) | rng.randint(0, 1 << 37, size=k, dtype=np.int64)
    elif kind == "cluster":  # every threshold inside one guide bucket, distinct digits
        b = int(rng.randint(0, 65536 // W))
        digits = b * W + rng.choice(W, size=k, replace=False)
        t = (digits.astype(np.int64) << 37) | rng.randint(0, 1 << 37, size=k, dtype=np.int64)
    elif kind == "ones_early":  # 1.0 from index n_q / 2 on
        t = np.concatenate([_rand53(rng, n_q // 2), np.full(k - n_q // 2, TWO53, dtype=np.int64)])
    elif kind == "zeros_lead":  # 0.0 up to n_q / 2
        t = np.concatenate([np.zeros(n_q // 2, dtype=np.int64), _rand53(rng, k - n_q // 2)])
    elif kind == "duplicates":  # runs of three equal thresholds
        t = np.repeat(_rand53(rng, (k + 2) // 3), 3)[:k]
    elif kind == "same_digit":  # groups of four that share their leading 16 bits and differ below
        digits = np.repeat(rng.choice(65535, size=(k + 3) // 4, replace=False), 4)[:k]
        low = rng.randint(0, 1 << 37, size=k, dtype=np.int64)
        while len(np.unique(low)) < k:
            low = rng.randint(0, 1 << 37, size=k, dtype=np.int64)
        t = (digits.astype(np.int64) << 37) | low
    elif kind == "constant":  # all 1.0, or all 0.0 with a last entry of 1.0
        t = np.full(k, TWO53 if rng.randint(2) else 0, dtype=np.int64)
    elif kind == "short":  # the last entry below 1.0: a gamma row scaled by 0.9
        w = rng.gamma(0.3, size=n_q) + 1e-12
        full = np.floor(np.cumsum(w) / w.sum() * TWO53).astype(np.int64)
        full[-1] = TWO53
        return np.sort(full // 10 * 9)
    else:
        raise ValueError(kind)
    return np.concatenate([np.sort(t), [TWO53]]).astype(np.int64)


def subst_row(kind, rng):
    """The three integer thresholds of one substitution row."""
    a, b = (int(x) for x in _rand53(rng, 2))
    if kind == "ordinary":
        return a, b, TWO53
    if kind == "001":
        return 0, 0, TWO53
    if kind == "111":
        return TWO53, TWO53, TWO53
    if kind == "011":
        return 0, TWO53, TWO53
    if kind == "equal":  # t0 == t1 strictly inside (0, 1)
        a = max(1, min(a, TWO53 - 1))
        return a, a, TWO53
    if kind == "same_digit":  # both thresholds on one 13-bit digit, different trailing bits
        lo, hi = sorted(int(x) for x in rng.randint(0, 1 << 39, size=2, dtype=np.int64))
        return (a >> 40 << 40) | lo, (a >> 40 << 40) | (hi + 1), TWO53
    if kind == "short":  # the last entry below 1.0
        return a // 10 * 9, b // 10 * 9, TWO53 // 10 * 9
    raise ValueError(kind)


def isize_cdfs(rng):
    """The four insert-size tables of case I33 as integer thresholds: one entry of 0.5 (the draw returns 0 or n_isize == 1);
    seven entries with leading zeros, a pair of equal entries and 1.0 before the end; 8000 entries with leading zeros, flat runs
    of 100 equal entries and 1.0 from entry 7000 on; the same scaled to a last entry of 0.5 (the draw returns up to 8000)."""
    a, b = (int(x) for x in _rand53(rng, 2))
    seven = np.array([0, 0, a, a, b, TWO53, TWO53], dtype=np.int64)
    steps = np.zeros(8000)
    steps[50:3000] = rng.gamma(0.3, size=2950) + 1e-12          # smooth, behind 50 leading zeros
    steps[3000:7001:100] = rng.gamma(0.3, size=41) * 30 + 1e-3  # then steps behind flat runs of 100 equal entries
    long_ = np.floor(np.cumsum(steps) / steps.sum() * TWO53).astype(np.int64)
    long_[7000:] = TWO53
    return [np.array([TWO53 // 2], dtype=np.int64), seven, long_, long_ // 2]


# bin tables of case B33: (what, CDFs [2][4] in tenths, histograms [2][4])
BIN_CASES = (
    ("empty_middle", ((3, 3, 7, 10), (2, 6, 6, 10)), ((1, 0, 1, 1), (1, 1, 0, 1))),
    ("empty_first", ((0, 4, 7, 10), (0, 0, 5, 10)), ((0, 1, 1, 1), (0, 0, 1, 1))),
    ("only_last", ((0, 0, 0, 10), (0, 0, 0, 10)), ((0, 0, 0, 1), (0, 0, 0, 1))),
    ("clamped", ((2, 4, 6, 8), (0, 3, 3, 8)), ((1, 1, 1, 1), (0, 1, 0, 1))),  # bin_cdf[3] == 0.8: the clamp of kde.py:77-78
)


def edge_model(RL, n_q, seed, guide_bits, subst_edges=False, phred="plain", isize=None, bins=None, mix="A", nonempty=((1, 1, 1, 1), (1, 0, 1, 1))):
    """synthetic_model(RL, n_q, 7, seed, indel=(0, 0)) with its tables replaced row by row from a seeded generator.  Returns
    (dense, info): info holds the integer thresholds (q_thr [2][4][RL][n_q], subst_thr, isize_thr, bin_thr, mut_thr), the type of
    every quality row ([2][4][RL] indices into ROW_TYPES) and of every substitution row ([2][RL][4] into SUBST_TYPES).
    phred: "plain" (1 - 10^(-q/10)), "halved", "nq_zero" (phred_thr[n_q] = 0.0) or "q0_one" (phred_thr[0] = 1.0: mut_thr 2^53).
    isize: integer thresholds of the insert-size table; bins: a row of BIN_CASES; mix: the row types' shares (ROW_WEIGHTS);
    nonempty: the mean-quality bins with histograms (synthetic_model's)."""
    nonempty = bins[2] if bins else nonempty
    dense = synthetic_model(RL, n_q, 7, seed, indel=(0.0, 0.0), nonempty=nonempty)
    rng = np.random.RandomState(seed + 1)
    W = 1 << (16 - guide_bits)
    q_type = rng.choice(len(ROW_TYPES), size=(2, 4, RL), p=ROW_WEIGHTS[mix])
    q_thr = np.zeros((2, 4, RL, n_q), dtype=np.int64)
    for idx in np.ndindex(2, 4, RL):
        q_thr[idx] = quality_row(ROW_TYPES[q_type[idx]], n_q, rng, W)
    s_type = rng.randint(0, len(SUBST_TYPES), size=(2, RL, 4)) if subst_edges else np.zeros((2, RL, 4), dtype=np.int64)
    s_thr = np.zeros((2, RL, 4, 3), dtype=np.int64)
    for idx in np.ndindex(2, RL, 4):
        s_thr[idx] = subst_row(SUBST_TYPES[s_type[idx]], rng)
    i_thr = np.asarray(isize if isize is not None else np.floor(dense.isize_cdf * TWO53), dtype=np.int64)
    b_thr = (np.asarray(bins[1], dtype=np.int64) * TWO53) // 10 if bins else np.ceil(dense.bin_cdf * TWO53).astype(np.int64)
    dense.qcdf = q_thr / float(TWO53)
    dense.subst_cdf = s_thr / float(TWO53)
    dense.isize_cdf = i_thr / float(TWO53)
    dense.bin_cdf = b_thr / float(TWO53)
    if phred == "halved":
        dense.phred_thr = dense.phred_thr / 2.0
    elif phred == "nq_zero":
        dense.phred_thr[n_q] = 0.0
    elif phred == "q0_one":
        dense.phred_thr[0] = 1.0
    else:
        assert phred == "plain"
    dense.validate()
    t = dense.device_tables()
    for name, T in (("q_thr", q_thr), ("subst_thr", s_thr), ("isize_thr", i_thr), ("bin_thr", b_thr)):
        assert np.array_equal(t[name].astype(np.int64), T), name  # T / 2^53 is exact: the device's integers are these
    info = {"q_thr": q_thr, "subst_thr": s_thr, "isize_thr": i_thr, "bin_thr": b_thr, "mut_thr": t["mut_thr"].astype(np.int64),
            "q_type": q_type, "s_type": s_type, "guide_bits": guide_bits, "n_q": n_q, "RL": RL}
    return dense, info


# ------------------------------------------------------------------ the ledger
def ledger(info, d, genome_bases_index=None):
    """How many bases (or pairs) of the draws `d` land on each edge class of the tables `info`, by integer arithmetic on the
    thresholds.  `genome_bases_index`: base index (A, T, C, G -> 0..3, -1: no substitution test row) of every base
    [n, 2, RL] -- with it the substitution classes are counted, over the bases whose error test fires."""
    n, _, RL = d.qm.shape
    n_q, gb = info["n_q"], info["guide_bits"]
    W = 1 << (16 - gb)
    isz = np.searchsorted(info["isize_thr"], d.pair[:, 0].astype(np.int64), "left")  # count(thr < m), on integers
    cle = np.stack([(info["bin_thr"][o][None, :] <= d.pair[:, 1 + o:2 + o].astype(np.int64)).sum(axis=1) for o in range(2)], axis=1)
    bins = np.minimum(cle, 3)
    L = collections.OrderedDict()
    it = info["isize_thr"]
    run = np.zeros(len(it) + 1, dtype=bool)  # run[r]: entries r - 100 .. r - 1 are equal and entry r (if any) is larger
    for r in range(100, len(it) + 1):
        run[r] = it[r - 100] == it[r - 1] and (r == len(it) or it[r] > it[r - 1])
    L["isize_after_run"] = int(run[isz].sum())
    L["isize_zero"] = int((isz == 0).sum())
    L["isize_n"] = int((isz == len(it)).sum())
    L["bin_clamped"] = int((cle == 4).sum())
    prob = np.diff(np.concatenate([np.zeros((2, 1), dtype=np.int64), info["bin_thr"]], axis=1), axis=1)
    after_empty = np.zeros((2, 4), dtype=bool)
    after_empty[:, 1:] = prob[:, :-1] == 0
    L["bin_after_empty"] = int(sum(after_empty[o][bins[:, o]].sum() for o in range(2)))
    h = d.h16.astype(np.int64)
    m = d.qm.astype(np.int64)
    phred = np.zeros((n, 2, RL), dtype=np.int64)
    first, past, below = (np.zeros((n, 2, RL), dtype=np.int64) for _ in range(3))
    rtype = np.zeros((n, 2, RL), dtype=np.int64)
    for o in range(2):
        rtype[:, o] = info["q_type"][o][bins[:, o]]
        for p in range(RL):
            T = info["q_thr"][o, bins[:, o], p]  # [n, n_q]
            t16 = np.minimum(T >> 37, 0xFFFF)
            ho, mo = h[:, o, p, None], m[:, o, p, None]
            phred[:, o, p] = (T < mo).sum(axis=1)
            first[:, o, p] = (t16 < ho).sum(axis=1)
            past[:, o, p] = (t16 <= ho).sum(axis=1)
            distinct = np.concatenate([np.ones((n, 1), dtype=bool), t16[:, 1:] != t16[:, :-1]], axis=1)
            below[:, o, p] = ((t16 < ho) & ((t16 // W) == (ho // W)) & distinct).sum(axis=1)
    tie = past > first
    L["tie"] = int(tie.sum())
    L["tie_first"] = int((tie & (phred == first)).sum())
    L["tie_past"] = int((tie & (phred == past)).sum())
    L["same_digit_between"] = int((tie & (phred > first) & (phred < past)).sum())
    L["more"] = int((below >= 3).sum())
    L["bucket_first"] = int((tie & (h % W == 0)).sum())
    L["bucket_last"] = int((tie & (h % W == W - 1)).sum())
    L["h_ffff_on_ones_early"] = int(((h == 0xFFFF) & (rtype == ROW_TYPES.index("ones_early"))).sum())
    L["h_ffff_on_short"] = int(((h == 0xFFFF) & (rtype == ROW_TYPES.index("short"))).sum())
    L["h_zero_on_zeros_lead"] = int(((h == 0) & (rtype == ROW_TYPES.index("zeros_lead"))).sum())
    L["phred_n_q"] = int((phred == n_q).sum())
    mt = info["mut_thr"][phred]
    e8 = d.e8.astype(np.int64)
    e8_tie = e8 == np.minimum(mt >> 45, 255)
    L["e8_tie"] = int(e8_tie.sum())
    L["e8_tie_at_255"] = int((e8_tie & (e8 == 255)).sum())
    L["e8_tie_clamped"] = int((e8_tie & (mt == TWO53)).sum())
    L["e8_on_phred_n_q"] = int((e8_tie & (phred == n_q)).sum())
    edge = tie | (below >= 3) | e8_tie
    if genome_bases_index is not None:
        bi = genome_bases_index
        fires = (d.em.astype(np.int64) > mt) & (bi >= 0)
        o_i, p_i = np.arange(2)[None, :, None], np.arange(RL)[None, None, :]
        S = info["subst_thr"][o_i, p_i, np.maximum(bi, 0)]  # [n, 2, RL, 3]
        d0, d1 = np.minimum(S[..., 0] >> 40, 0x1FFF), np.minimum(S[..., 1] >> 40, 0x1FFF)
        hs = d.sm.astype(np.int64) >> 40
        L["subst_tested"] = int(fires.sum())
        L["subst_tie_t0"] = int((fires & (hs == d0)).sum())
        L["subst_tie_t1"] = int((fires & (hs == d1)).sum())
        L["subst_tie_equal"] = int((fires & (hs == d0) & (S[..., 0] == S[..., 1]) & (S[..., 0] > 0) & (S[..., 0] < TWO53)).sum())
        L["subst_1fff"] = int((fires & (hs == 0x1FFF) & ((S[..., 0] == TWO53) | (S[..., 1] == TWO53))).sum())
        edge = edge | (fires & ((hs == d0) | (hs == d1)))
    L["padding_superitem"] = int(edge[:, :, RL // 8 * 8:].sum()) if RL % 8 else 0
    return L, {"isize": isz, "bins": bins, "phred": phred}


# ------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "id RL n_q pairs guide_bits genome what dense info")
GUIDE_BITS = (6, 7, 8)


def _genome(kind, RL, length=None):
    n = length or 8 * RL + 1007
    return mixed_genome(600 + RL, n) if kind == "mixed" else random_genome(600 + RL, n)


def sprinkled_genome(RL, n=20000):
    """A plain record with an N every thousand letters or so: the MT resolver hands the pairs that touch one to the walker."""
    g = np.frombuffer(random_genome(700 + RL, n).encode(), dtype=np.uint8).copy()
    g[np.random.RandomState(701 + RL).randint(0, n, size=n // 1000)] = ord("N")
    return g.tobytes().decode()


_cases = {}


def case(cid):
    """The case `cid`, built once: Q33-<gb>, Q33-<gb>-mixed, Q65-<gb>, Q9, S33, I33-<0..3>, B33-<0..3>."""
    if cid in _cases:
        return _cases[cid]
    parts = cid.split("-")
    name = parts[0]
    kind = "mixed" if parts[-1] == "mixed" else "plain"
    if name == "Q33":
        gb = int(parts[1])
        c = Case(cid, 33, 41, 1 << 15, gb, _genome(kind, 33), "five superitems, one valid position in the last", *edge_model(33, 41, 3301, gb))
    elif name == "Q65":
        gb = int(parts[1])
        # (two bins with histograms a mate: four would need two position tiles at any guide-bit value, and ni == 2)
        c = Case(cid, 65, 60, 1 << 14, gb, _genome(kind, 65), "63 entries a row: the largest guide byte; ni == 3; phred_thr[n_q] == 0.0",
                 *edge_model(65, 60, 6507, gb, phred="nq_zero", mix="B", nonempty=SLOTS_TWO))
    elif name == "Q9":
        c = Case(cid, 9, 3, 1 << 16, 6, _genome(kind, 9), "rows shorter than a guide bucket is wide; phred_thr[0] == 1.0",
                 *edge_model(9, 3, 901, 6, phred="q0_one"))
    elif name == "S33":
        c = Case(cid, 33, 41, 1 << 15, 6, _genome(kind, 33), "substitution patterns, phred_thr halved",
                 *edge_model(33, 41, 3302, 6, subst_edges=True, phred="halved"))
    elif name == "I33":
        k = int(parts[1])
        c = Case(cid, 33, 41, 1 << 13, 6, _genome(kind, 33, 20000), "insert-size table %d" % k,
                 *edge_model(33, 41, 3303, 6, isize=isize_cdfs(np.random.RandomState(3304))[k]))
    elif name == "B33":
        k = int(parts[1])
        c = Case(cid, 33, 41, 1 << 13, 6, _genome(kind, 33), "bin tables: " + BIN_CASES[k][0], *edge_model(33, 41, 3305, 6, bins=BIN_CASES[k]))
    else:
        raise KeyError(cid)
    _cases[cid] = c
    return c


PHILOX_CASES = (["Q33-%d" % gb for gb in GUIDE_BITS] + ["Q33-6-mixed"] + ["Q65-%d" % gb for gb in GUIDE_BITS] + ["Q9", "S33"]
                + ["I33-%d" % k for k in range(4)] + ["B33-%d" % k for k in range(4)])

_oracles = {}


def oracle_rows(cid, store_mutations=False):
    """The oracle's reads of case `cid` (Philox seed SEED, first ordinal FIRST_ORDINAL), computed once and never written to."""
    key = (cid, store_mutations)
    if key not in _oracles:
        from oracle import oracle as O

        c = case(cid)
        exp = O.Oracle(c.dense).simulate(O.Rng().seed_philox(SEED), c.genome, c.pairs, first_ordinal=FIRST_ORDINAL, want_coords=True,
                                         store_mutations=store_mutations)
        assert exp["status"] == 0 and exp["n_done"] == c.pairs
        for k in ("r1_base", "r1_qual", "r2_base", "r2_qual", "coords"):
            exp[k].setflags(write=False)
        _oracles[key] = exp
    return _oracles[key]


_draws = {}


def case_draws(cid):
    """The numerators of case `cid` (the cases of one shape share them: same seed, ordinals and read length)."""
    c = case(cid)
    key = (c.pairs, c.RL)
    if key not in _draws:
        _draws[key] = draws(SEED, FIRST_ORDINAL, c.pairs, c.RL)
    return _draws[key]


# the classes a case names (each must count FLOOR), by the case id's first part or the whole id
_QUALITY = ("tie", "tie_first", "tie_past", "same_digit_between", "more", "bucket_first", "bucket_last", "h_ffff_on_ones_early",
            "phred_n_q", "e8_tie", "e8_tie_at_255", "e8_on_phred_n_q", "padding_superitem")
NAMED = {
    "Q33": _QUALITY + ("h_ffff_on_short",),
    "Q65": _QUALITY + ("h_zero_on_zeros_lead",),
    "Q9": ("tie", "tie_first", "tie_past", "more", "bucket_last", "phred_n_q", "e8_tie", "e8_tie_at_255", "e8_tie_clamped",
           "e8_on_phred_n_q", "padding_superitem", "h_ffff_on_short"),
    "S33": ("subst_tie_t0", "subst_tie_t1", "subst_tie_equal", "subst_1fff", "padding_superitem"),
    "I33-0": ("isize_zero", "isize_n"), "I33-1": (), "I33-2": ("isize_after_run",), "I33-3": ("isize_after_run", "isize_n"),
    "B33-0": ("bin_after_empty",), "B33-1": ("bin_after_empty",), "B33-2": ("bin_after_empty",),
    "B33-3": ("bin_clamped", "bin_after_empty"),
}
# classes a shape cannot bring to FLOOR below 2^16 pairs (DESIGN.md section 4 lists them with their counts)
DROPPED = {"Q9": ("same_digit_between", "bucket_first", "h_ffff_on_ones_early", "h_zero_on_zeros_lead")}


def named(cid):
    return NAMED[cid] if cid in NAMED else NAMED[cid.split("-")[0]]
