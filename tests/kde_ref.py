"""The yardstick of the `model` KDE tests: the quality and insert-size CDFs of iss/modeller.py:12-38, 99-134 from their definition at
60 significant digits (stdlib decimal), the same through scipy's gaussian_kde the way the reference calls it, an a-priori bound
for float64's rounding in between, and the records that put a chosen histogram into a chosen (mate, bin, position).

Definition, for data x_1..x_n (the reference adds 1 to the last datum when all are equal, modeller.py:127-128):
mean m = sum(x) / n; variance v = sum((x - m)^2) / (n - 1); factor f = 0.2 / sqrt(v); bandwidth h = f * sqrt(v);
density d(y) = sum_i exp(-((y - x_i) / h)^2 / 2) / (n h sqrt(2 pi)); cdf_k = sum_{j <= k} d(y_j) / sum_j d(y_j).
The grid y is data: range(41) for qualities, np.linspace(min, max, 2000) as float64 computes it for insert sizes."""
from decimal import Decimal, getcontext

import numpy as np

import bam_synth

PREC = 60
EPS = 2.0 ** -53
Q_GRID = list(range(41))


def _hist(data):
    h = {}
    for x in data:
        h[int(x)] = h.get(int(x), 0) + 1
    return sorted(h.items())


def moved(data):
    """The reference's np.std == 0 branch: the last datum plus one."""
    data = list(data)
    if len(set(data)) == 1:
        data[-1] += 1
    return data


def cdf_decimal(data, grid, with_bound=False):
    """The CDF on `grid` from the definition, as floats rounded from 60 digits; with_bound: also the a-priori bound of what a
    float64 evaluation may be off by (see rounding_bound)."""
    getcontext().prec = PREC
    hist = [(Decimal(v), Decimal(c)) for v, c in _hist(data)]
    n = sum(c for _, c in hist)
    mean = sum(c * v for v, c in hist) / n
    var = sum(c * (v - mean) ** 2 for v, c in hist) / (n - 1)
    std = var.sqrt()
    factor = Decimal("0.2") / std
    h = factor * std
    norm = 1 / (n * h * (2 * Decimal("3.14159265358979323846264338327950288419716939937510582097494")).sqrt())
    dens, errs = [], []
    for y in grid:
        y = Decimal(float(y))  # exact
        d = e = Decimal(0)
        for v, c in hist:
            r = (y - v) / h
            term = c * (-(r * r) / 2).exp() * norm
            d += term
            if with_bound:
                e += term * rounding_bound(r, v, y, h)
        dens.append(d)
        errs.append(e)
    total = sum(dens)
    cum, out = Decimal(0), []
    for d in dens:
        cum += d
        out.append(float(cum / total))
    if not with_bound:
        return np.array(out)
    # numerator and denominator each carry at most the summed term errors, plus one rounding per addition of the running sum
    bound = float(2 * sum(errs) / total) + 2 * len(grid) * EPS
    return np.array(out), bound


def rounding_bound(r, v, y, h):
    """Relative error a float64 evaluation of exp(-r^2 / 2) may carry, r = v/h - y/h.  Both quotients round, (|v| + |y|) / h * eps
    between them, which moves r^2 / 2 by |r| times that (doubled here).  The bandwidth comes from a sum of non-negative terms over
    the histogram, at most 95 of them non-zero (pairwise over the data in numpy: fewer roundings still), each rounding once: 128 eps
    on the covariance, 64 eps on h, 128 eps on r^2, so 64 r^2 eps on r^2 / 2.  exp, the products and the weight: 16 eps."""
    eps = Decimal(EPS)
    return eps * (2 * abs(r) * (abs(v) + abs(y)) / h + 64 * r * r + 16)


def cdf_scipy(data, grid):
    """scipy's gaussian_kde as iss/modeller.py:33-37 and :121-132 call it."""
    from scipy import stats

    data = np.asarray(data, dtype=np.float64)
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        try:
            kde = stats.gaussian_kde(data, bw_method=0.2 / np.std(data, ddof=1))
        except np.linalg.LinAlgError:
            data = np.asarray(moved(data), dtype=np.float64)
            kde = stats.gaussian_kde(data, bw_method=0.2 / np.std(data, ddof=1))
        cdf = np.cumsum(kde.evaluate(grid))
        return cdf / cdf[-1]


def isize_grid(tlens, read_length):
    isd = np.asarray(tlens) - 2 * read_length
    return isd, np.linspace(min(isd), max(isd), 2000)


# ---- quality cases: name -> the qualities of one position over the reads of its slice
# The largest count in one bin.  scipy evaluates the reference's call over every datum: 1.3 s for 2^21 of them, 12 s for 2^24, and
# 2^32 is out of reach, for the feeds too.  So 2^21 + 1 it is, fed as 16 blocks of 2^17 records and a last small one.
BIG = (1 << 21) + 1
BIG_DATA = [20] * BIG + [25] * 3 + [29]
BIG_SLICE = (0, 2)  # reads of one base: position 0 is all there is
# 96 reads: a count at which scipy's weighted mean of 96 equal values is that value, so that the reference reaches its LinAlgError
# branch (at most other counts, 84 among them, the covariance is a rounding residue times inf and the reference ends in a ValueError)
N_MANY = 96
DENSE = [v % 42 for v in range(N_MANY)]
Q_SLICES = {
    # slice (mate, bin): {case: column}; every column of a slice has the slice's number of reads
    (0, 1): {"two_distinct": [3, 17], "two_equal_0": [0, 0], "two_equal_40": [40, 40], "two_equal_93": [93, 93],
             "two_far_48_50": [48, 50], "two_far_47_49": [47, 49], "two_far_equal_60": [60, 60], "two_adjacent": [20, 21]},
    (1, 2): {"single_value_many": [30] * N_MANY, "bimodal_0_41": [0] * 48 + [41] * 48, "dense_0_41": DENSE,
             "one_outlier": [35] * (N_MANY - 1) + [2], "far_dense_48_93": [48 + (i * 5) % 46 for i in range(N_MANY)]},
    (0, 3): {"three_reads": [38, 36, 39]},
}
NAN_CASES = ("two_equal_93", "two_far_48_50", "two_far_equal_60", "far_dense_48_93")  # every grid term underflows to 0: scipy's row is 0 / 0
ISIZE_CASES = {
    "two_values_1_apart": [300] * 40 + [301] * 25,
    "1_and_1999": [1] * 3 + [1999] * 2,
    "peak_and_outlier": [500] * 50 + [1500],
}


def slice_reads(mate, b, columns, name):
    """Records of slice (mate, b) whose first positions hold `columns` (in order) and whose further positions bring every read's
    mean quality to the middle of the bin.  Returns (records, {case: position})."""
    cols = list(columns.items())
    n = len(cols[0][1])
    assert all(len(c) == n for _, c in cols)
    heads = [[c[i] for _, c in cols] for i in range(n)]
    k = 0
    while True:  # the fewest padding positions with which every read's mean lands in [10 b, 10 b + 10)
        L = len(cols) + k
        if all(10 * b * L <= sum(h) + 93 * k and sum(h) <= (10 * b + 10) * L - 1 for h in heads):
            break
        k += 1
    reads = []
    for i, h in enumerate(heads):
        want = min(max((10 * b + 5) * L - sum(h), max(0, 10 * b * L - sum(h))), 93 * k, (10 * b + 10) * L - 1 - sum(h))
        pad = [want // k + (1 if j < want % k else 0) for j in range(k)] if k else []
        q = h + pad
        assert 10 * b <= sum(q) // L < 10 * b + 10 and max(q) <= 93
        reads.append(bam_synth.edge_read("%s_%d" % (name, i), [(0, L)], qual=q, flag=bam_synth.R1 if mate == 0 else bam_synth.R2R & ~16))
    return reads, {case: p for p, (case, _) in enumerate(cols)}


def q_case_data():
    """{case: the column}, the data of every quality case."""
    return {case: col for cols in Q_SLICES.values() for case, col in cols.items()}


def big_block(n):
    """(bytes, offsets) of n copies of the one-base read that adds 20 to position 0 of BIG_SLICE."""
    rec = bam_synth.encode_record(bam_synth.edge_read("big", [(0, 1)], qual=[20], flag=bam_synth.R1 & ~1))
    return np.tile(np.frombuffer(rec, np.uint8), n), np.arange(n, dtype=np.int64) * len(rec)


def big_tail():
    """The records behind the blocks: one more 20, and the 25s and the 29 of BIG_DATA."""
    return [bam_synth.edge_read("big_%d" % i, [(0, 1)], qual=[q], flag=bam_synth.R1 & ~1) for i, q in enumerate([20, 25, 25, 25, 29])]


def shape_reads():
    """Slices that differ in shape: (1, 0) holds reads of 6, 6 and 4 bases (position 3 is a number, position 4 is not), (1, 3) holds
    one read (no row at all) and (1, 1) next to it holds two.  Returns (records, {(mate, bin): [the reads' qualities]})."""
    quals = {(1, 0): [[5, 9, 2, 7, 1, 3], [8, 1, 6, 2, 9, 4], [0, 4, 9, 9]], (1, 3): [[30, 35, 38, 33]], (1, 1): [[12, 18, 11], [19, 10, 15]]}
    recs = [bam_synth.edge_read("shape_%d%d_%d" % (m, b, i), [(0, len(q))], qual=q, flag=bam_synth.R2R & ~16)
            for (m, b), qs in quals.items() for i, q in enumerate(qs)]
    return recs, quals
