"""The model's joint distribution, and the statistics that hold a sample of read pairs to it (no GPU, no library code).

What the parity tests cannot see: the oracle and the device restate the same Philox address map, so an error
of the map -- two consumers on one half-word, a byte select off by a lane, a `sub` that collides -- is in both and every
comparison of the two stays green.  Here the expectations come from the dense tables alone (``Expect``), a plain float64 numpy
sampler of the reference's text stands beside them (``sample_model``: iss/error_models/kde.py:52-86, __init__.py:69-112,
generator.py:121-190), ``plant`` turns a sample of it into what a map error would have produced, and the statistics S1 .. S8
accumulate over slices of a sample (count tables by np.bincount on a combined index, matrix sums by BLAS), so the caller never
holds more than a slice.

Arrays of a slice: ``Q`` phreds, ``B`` letters, ``T`` template letters -- uint8 [n, 2, P], P = len(positions), mate 0 forward,
mate 1 reverse; a column c = mate * P + j of the flattened [n, 2 P] view is position positions[j] of that mate.

The decision rule is in one place, ``accept``: all hypotheses of a test function share ALPHA by Bonferroni, two-sided tests use
ALPHA / 2.  Seeds are fixed, so a verdict never changes between runs; ALPHA is the chance that a CORRECT implementation would
fail under a fresh seed -- a condition, not a measurement."""
import collections

import numpy as np
from scipy import stats as sps

ALPHA = 1e-6
SLICE = 1 << 18  # pairs of a download
CHUNK = 1 << 16  # rows of one matrix product (float32 in, float64 accumulated)
LAGS = (1, 63, 64, 256)
BASES = b"ATCG"  # the dense tables' base order

# Pairs of a GPU case, per model: the smallest power of two at which every defect of ``plant`` is rejected on ``sample_model``
# by the statistic meant for it, with a p-value a factor 100 inside the bound so that another seed would not flip the verdict
# (tests/test_philox_stats_host.py::test_every_planted_defect_is_rejected runs exactly these, and shows that half the size
# leaves a defect standing; DESIGN section 4 records each defect's p-value).  Cap 2^21: a defect that needs more is DROPPED.
N_PAIRS = {"hiseq": 1 << 19, "miseq": 1 << 18, "novaseq": 1 << 20, "nextseq": 1 << 19}
# "hf" (1 % of the reads share the error-test uniform of two positions) adds about 1 % of n E[min(pe, pe')] double errors to
# n E[pe pe'] expected ones: two standard deviations at 2^20 pairs of any shipped model, seven -- what the family of every
# pair of columns asks -- near 2^24.  Dropped for every model; "ha" stays.
DROPPED = {"hiseq": ("hf",), "miseq": ("hf",), "novaseq": ("hf",), "nextseq": ("hf",)}
# iterations of 4 superitems per pass of a position tile (tests/test_gpu_grouped.py FORCED); a split model's tiles are whole
# multiples of 4 superitems, so a tile of a model with several holds 4 * ni superitems = 32 * ni positions
MAIN_NI = {"novaseq": 5, "hiseq": 2, "miseq": 2, "nextseq": 4}

Result = collections.namedtuple("Result", "stat p where m sides value")
# stat: name; p: the smallest one-tail p-value; where: what it belongs to; m: hypotheses tested; sides: 1 or 2; value: the
# statistic itself (chi-square, z or count) for the record


def accept(results, alpha=ALPHA, m=None):
    """(ok, text).  Every hypothesis of ``results`` shares alpha (Bonferroni over sum(m), or over ``m`` where the caller tests a
    part of a larger family and has to answer for the whole); a two-sided test rejects below alpha / 2."""
    total = int(m) if m is not None else sum(r.m for r in results)
    bad = [r for r in results if r.m > 0 and r.p < alpha / (r.sides * max(total, 1))]
    text = "; ".join("%s p %.3g (bound %.3g) at %s, value %s, %d hypotheses" % (r.stat, r.p, alpha / (r.sides * max(total, 1)), r.where, r.value, r.m)
                     for r in results)
    return not bad, text


# ------------------------------------------------------------------ expectations, from the dense tables alone
class Expect(object):
    def __init__(self, dense):
        d = dense
        RL, nq = d.read_length, d.n_q
        self.RL, self.nq, self.K = RL, nq, nq + 1
        w = np.diff(np.concatenate([np.zeros((2, 1)), d.bin_cdf], axis=1), axis=1) * (d.bin_nonempty != 0)
        self.w = w / w.sum(axis=1, keepdims=True)  # [mate][bin]
        # searchsorted(cdf, u) (side="left") = #{cdf < u}: P(k) = cdf[k] - cdf[k - 1], and k == n_q where u passes the last entry
        edges = np.concatenate([np.zeros(d.qcdf.shape[:3] + (1,)), d.qcdf, np.ones(d.qcdf.shape[:3] + (1,))], axis=3)
        self.pm = np.clip(np.diff(edges, axis=3), 0.0, None) * (d.bin_nonempty != 0)[:, :, None, None]  # [mate][bin][p][k]
        self.marg = np.einsum("ob,obpk->opk", self.w, self.pm)  # [mate][p][k]
        self.pe = 10.0 ** (-np.arange(nq + 1) / 10.0)
        F = np.cumsum(self.marg, axis=2)
        self.score = F - self.marg / 2 - 0.5  # mid-distribution score: mean 0 under the marginal
        self.mu = np.einsum("obpk,opk->obp", self.pm, self.score)  # E[score | bin]
        self.alt_pmf = np.diff(np.concatenate([np.zeros(d.subst_cdf.shape[:3] + (1,)), d.subst_cdf], axis=3), axis=3)  # [mate][p][base][3]
        self.alt = d.subst_alt
        self.isize_pmf = np.clip(np.diff(np.concatenate([[0.0], d.isize_cdf, [1.0]])), 0.0, None)  # (+ the cell past the table)


def expectations(dense):
    return Expect(dense)


def fragment_pmf(mu, sd, RL, lo, hi):
    """PMF of ``int(normal(mu, sd)) - 2 RL`` on the insert sizes lo .. hi (generator.py:122-123); int() truncates toward zero:
    int(x) == f for f > 0 on [f, f + 1), for f < 0 on (f - 1, f], and 0 on (-1, 1)."""
    f = np.arange(lo, hi + 1) + 2 * RL
    a = np.where(f > 0, f, f - 1).astype(np.float64)
    b = np.where(f >= 0, f + 1, f).astype(np.float64)
    return np.arange(lo, hi + 1), sps.norm.cdf(b, mu, sd) - sps.norm.cdf(a, mu, sd)


_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTYRWSKMNBVDH", b"TGCARYWSMKNVBHD"):
    _COMP[_a] = _b
    _COMP[_a + 32] = _b + 32
_CODE = np.full(256, 4, dtype=np.int64)  # letter -> index in BASES; 4: not one of the four (upper case only)
for _i, _a in enumerate(BASES):
    _CODE[_a] = _i
_AMBIGUOUS = np.zeros(256, dtype=bool)
for _a in b"RYWSMKHBVDN":
    _AMBIGUOUS[_a] = _AMBIGUOUS[_a + 32] = True


def templates(genome, coords, RL, positions):
    """Template letters [n, 2, P]: genome[fs + p] forward, rev_comp(genome[re - RL:re])[p] = comp(genome[re - 1 - p]) reverse."""
    g = np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)
    pos = np.asarray(positions, dtype=np.int64)
    T = np.empty((len(coords), 2, len(pos)), dtype=np.uint8)
    assert len(g) < 2**31
    pos, fs, re = pos.astype(np.int32), coords[:, 0].astype(np.int32), coords[:, 2].astype(np.int32)
    np.take(g, fs[:, None] + pos[None, :], out=T[:, 0])
    np.take(_COMP[g], (re - 1)[:, None] - pos[None, :], out=T[:, 1])
    return T


def slice_of(rows, coords, genome, RL, positions=None):
    """A slice for the statistics from what a download (or the oracle) gives."""
    pos = np.arange(RL) if positions is None else np.asarray(positions)
    return {"Q": stack_mates(rows["r1_qual"], rows["r2_qual"], positions), "B": stack_mates(rows["r1_base"], rows["r2_base"], positions),
            "T": templates(genome, coords, RL, pos), "coords": coords}


def stack_mates(r1, r2, positions=None):
    """[n, 2, P] (C order) of two [n, >= RL] arrays."""
    P = r1.shape[1] if positions is None else len(positions)
    out = np.empty((r1.shape[0], 2, P), dtype=r1.dtype)
    out[:, 0] = r1 if positions is None else r1[:, positions]
    out[:, 1] = r2 if positions is None else r2[:, positions]
    return out


# ------------------------------------------------------------------ the reference sampler and the defects
def _derive(dense, U, positions):
    """Phreds, error events and letters from the uniforms, as the reference does."""
    d = dense
    n, P = U["uq"].shape[0], len(positions)
    Q = np.zeros((n, 2, P), dtype=np.uint8)
    B = U["T"].copy()
    for o in range(2):
        sub = U.get("subst_mate", (0, 1))[o]
        for j, p in enumerate(positions):
            q = np.zeros(n, dtype=np.int64)
            for b in range(4):
                sel = U["bin"][:, o] == b
                if sel.any():
                    q[sel] = np.searchsorted(d.qcdf[o, b, p], U["uq"][sel, o, j])  # kde.py:84
            Q[:, o, j] = q
            err = U["ue"][:, o, j] > 1 - 10 ** (-q / 10)  # __init__.py:94, util.phred_to_prob
            code = _CODE[U["T"][:, o, j]]
            for c in range(4):
                sel = np.flatnonzero(err & (code == c))
                if sel.size:  # np.random.choice(letters, p=): searchsorted(cdf, u, side="right")
                    k = np.minimum(np.searchsorted(d.subst_cdf[sub, p, c], U["ua"][sel, o, j], side="right"), 2)
                    B[sel, o, j] = d.subst_alt[sub, p, c][k]
    return Q, B


def sample_model(dense, n, rng, genome, positions=None, keep=False):
    """One set of n pairs of the model, float64 throughout: insert size by searchsorted(isize_cdf, u), forward start uniform on
    range(L - fragment) (the genome must be long enough that no pair falls back), per mate a mean-quality bin by choice, per
    position a phred, an error test and an alternative.  No indels.  Only ``positions`` are drawn."""
    d = dense
    RL = d.read_length
    pos = np.arange(RL) if positions is None else np.asarray(positions)
    g = np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)
    L, P = len(g), len(pos)
    isize = np.searchsorted(d.isize_cdf, rng.random_sample(n))
    width = L - (isize + 2 * RL)
    assert (width > 0).all()
    fs = np.floor(rng.random_sample(n) * width).astype(np.int64)
    coords = np.stack([fs, fs + RL + isize, fs + 2 * RL + isize, isize], axis=1)
    w = np.diff(np.concatenate([np.zeros((2, 1)), d.bin_cdf], axis=1), axis=1)
    U = {"bin": np.stack([rng.choice(4, size=n, p=w[o] / w[o].sum()) for o in range(2)], axis=1),
         "uq": rng.random_sample((n, 2, P)), "ue": rng.random_sample((n, 2, P)), "ua": rng.random_sample((n, 2, P)),
         "T": templates(g, coords, RL, pos)}
    Q, B = _derive(d, U, pos)
    out = {"Q": Q, "B": B, "T": U["T"], "coords": coords}
    if keep:
        out["U"], out["positions"] = U, pos
    return out


DEFECTS = ("a", "b", "c", "d", "e", "f", "g", "ha", "hf")


def plant(dense, sample, defect, rng=None):
    """The sample a map error would have given, re-derived from shared uniforms; the defect sits at the sample's first two
    positions (a = column 0, b = column 1), mate 0 unless it is about the mates:
    a   b uses a's quality uniform;                       b   b shares only the leading 8 bits of a's 16-bit digit;
    c   the two mates share the quality uniform at a;      d   pair i + 1 reuses pair i's quality uniform at a;
    e   the error test's leading 8 bits are the quality uniform's, same position;
    f   the error-test uniforms of a and b are shared;     g   the reverse mate reads the forward substitution table;
    ha, hf   a and f in 1 % of the reads."""
    U = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sample["U"].items()}
    n = U["uq"].shape[0]
    some = (rng or np.random.RandomState(1)).random_sample(n) < 0.01

    def lead8(hi, lo):
        return (np.floor(hi * 256) + (lo * 256 - np.floor(lo * 256))) / 256

    if defect == "a":
        U["uq"][:, 0, 1] = U["uq"][:, 0, 0]
    elif defect == "b":
        U["uq"][:, 0, 1] = lead8(U["uq"][:, 0, 0], U["uq"][:, 0, 1])
    elif defect == "c":
        U["uq"][:, 1, 0] = U["uq"][:, 0, 0]
    elif defect == "d":
        U["uq"][1::2, 0, 0] = U["uq"][0:n - 1:2, 0, 0][: len(U["uq"][1::2])]
    elif defect == "e":
        U["ue"][:, 0, 0] = lead8(U["uq"][:, 0, 0], U["ue"][:, 0, 0])
    elif defect == "f":
        U["ue"][:, 0, 1] = U["ue"][:, 0, 0]
    elif defect == "g":
        U["subst_mate"] = (0, 0)
    elif defect == "ha":
        U["uq"][some, 0, 1] = U["uq"][some, 0, 0]
    elif defect == "hf":
        U["ue"][some, 0, 1] = U["ue"][some, 0, 0]
    else:
        raise ValueError(defect)
    Q, B = _derive(dense, U, sample["positions"])
    return {"Q": Q, "B": B, "T": U["T"], "coords": sample["coords"]}


# ------------------------------------------------------------------ tools of the statistics
def chi_square(obs, expected):
    """(statistic, degrees of freedom, p) of counts against expectations, cells merged in ascending order of expectation until
    every merged cell expects at least 5 (the rest joins the last one).  A count in a cell the model gives no mass is a
    rejection by itself (p = 0)."""
    obs = np.asarray(obs, dtype=np.float64).ravel()
    expected = np.asarray(expected, dtype=np.float64).ravel()
    if (obs[expected <= 0] > 0).any():
        return np.inf, 0, 0.0
    keep = expected > 0
    order = np.argsort(expected[keep], kind="stable")
    e, o = expected[keep][order], obs[keep][order]
    ce = np.cumsum(e)
    cuts, last = [], 0.0  # ends of the merged cells
    i = 0
    while i < len(e):
        j = int(np.searchsorted(ce, last + 5.0 * (1 - 1e-12), side="left"))
        if j >= len(e):
            break
        cuts.append(j)
        last = ce[j]
        i = j + 1
    if len(cuts) < 2:
        return 0.0, 0, 1.0
    cuts[-1] = len(e) - 1
    idx = np.concatenate([[0], np.asarray(cuts[:-1]) + 1])
    E, O = np.add.reduceat(e, idx), np.add.reduceat(o, idx)
    assert (E >= 5.0 * (1 - 1e-9)).all(), "a pooled chi-square cell expects less than 5"
    stat = float(((O - E) ** 2 / E).sum())
    df = len(E) - 1
    return stat, df, float(sps.chi2.sf(stat, df))


def gram(A, B):
    """A^T B over chunks of rows: float32 products, float64 sums."""
    out = np.zeros((A.shape[1], B.shape[1]))
    for i in range(0, A.shape[0], CHUNK):
        out += A[i:i + CHUNK].T @ B[i:i + CHUNK]
    return out


def _worst_z(Z, tested, names, stat):
    if not tested.any():
        return Result(stat, 1.0, None, 0, 2, 0.0)
    A = np.where(tested, np.abs(Z), -1.0)
    at = np.unravel_index(int(np.argmax(A)), A.shape)
    return Result(stat, float(sps.norm.sf(A[at])), tuple(nm[i] for nm, i in zip(names, at)), int(tested.sum()), 2, round(float(Z[at]), 3))


class _Stat(object):
    def __init__(self, dense, positions=None, expect=None):
        self.d, self.x = dense, expect or Expect(dense)
        self.pos = np.arange(dense.read_length) if positions is None else np.asarray(positions)
        self.P, self.K = len(self.pos), self.x.K
        self.C = 2 * self.P
        self.names = [(o, int(p)) for o in range(2) for p in self.pos]
        self.n = 0
        self.score32 = np.ascontiguousarray(self.x.score[:, self.pos].reshape(self.C, self.K), dtype=np.float32)
        self.pe32 = self.x.pe.astype(np.float32)

    ACC = ()  # names of the sums a statistic accumulates (besides n)

    def merge(self, other):
        """Take over what another instance of the same statistic accumulated from other slices."""
        for name in self.ACC + ("n",):
            setattr(self, name, getattr(self, name) + getattr(other, name))

    def flat(self, X):
        return X.reshape(X.shape[0], self.C)

    def errors(self, s, letters_only):
        """Kept with the slice: err (base != template, counted cells only), the model's error probability per cell as float32
        (0 where the template takes no substitution) and the cells counted (None: all).  ``letters_only``: upper-case A, C, G,
        T templates only; an ambiguous template must come out unchanged."""
        key = ("errors", self.pos.tobytes(), bool(letters_only))
        if key not in s:
            Q, B, T = self.flat(s["Q"]), self.flat(s["B"]), self.flat(s["T"])
            assert int(Q.max()) < self.K, "a phred beyond the model's"
            err = B != T
            pe = np.take(self.pe32, Q)
            counted = None
            if letters_only:
                assert not (err & _AMBIGUOUS[T]).any(), "a substitution at an ambiguous template letter"
                counted = _CODE[T] < 4
                err &= counted
                pe *= counted
            s[key] = (err, pe, counted)
        return s[key]

    def scores(self, s):
        """(S, S * S) of a slice, float32 [n, 2 P]; kept with the slice for the next statistic over the same positions."""
        key = ("scores", self.pos.tobytes())
        if key not in s:
            q = self.flat(s["Q"])
            assert int(q.max()) < self.K, "a phred beyond the model's"
            S = np.take(self.score32.ravel(), q.astype(np.int32) + (np.arange(self.C, dtype=np.int32) * self.K)[None, :])
            s[key] = (S, S * S)
        return s[key]


class S1(_Stat):
    """Marginal phred PMF at every (mate, position): chi-square."""
    ACC = ("cnt",)

    def __init__(self, dense, positions=None, expect=None):
        _Stat.__init__(self, dense, positions, expect)
        self.cnt = np.zeros((self.C, self.K), dtype=np.int64)

    def add(self, s):
        q = self.flat(s["Q"])
        assert int(q.max()) < self.K, "a phred beyond the model's"
        n = q.shape[0]
        cnt = np.bincount((q.astype(np.int32) + (np.arange(self.C, dtype=np.int32) * self.K)[None, :]).ravel(), minlength=self.C * self.K)
        self.cnt += cnt.reshape(self.C, self.K)
        self.n += n

    def results(self):
        marg = self.x.marg[:, self.pos].reshape(self.C, self.K)
        best, m = Result("S1 marginal", 1.0, None, 0, 1, 0.0), 0
        for c in range(self.C):
            stat, df, p = chi_square(self.cnt[c], self.n * marg[c])
            m += df > 0 or p == 0.0
            if p < best.p:
                best = Result("S1 marginal", p, self.names[c], 0, 1, round(stat, 2))
        return [best._replace(m=m)]


class S2(_Stat):
    """Every pair of positions of a pair of reads: covariance of the mid-distribution scores against the bin mixture's."""

    ACC = ("c", "v")

    def __init__(self, dense, positions=None, expect=None):
        _Stat.__init__(self, dense, positions, expect)
        self.c = np.zeros((self.C, self.C))
        self.v = np.zeros((self.C, self.C))

    def add(self, s):
        S, S2_ = self.scores(s)
        self.c += gram(S, S)
        self.v += gram(S2_, S2_)
        self.n += S.shape[0]

    def results(self):
        n, P = self.n, self.P
        C, V = self.c / n, self.v / n
        E = np.zeros((self.C, self.C))
        for o in range(2):
            mu = self.x.mu[o][:, self.pos]
            E[o * P:(o + 1) * P, o * P:(o + 1) * P] = np.einsum("b,bp,bq->pq", self.x.w[o], mu, mu)
        se = np.sqrt(np.maximum(V - C * C, 0.0) / n)
        tested = np.triu(np.ones_like(C, dtype=bool), 1) & (se > 0)
        Z = np.where(se > 0, (C - E) / np.where(se > 0, se, 1.0), 0.0)
        return [_worst_z(Z, tested, (self.names, self.names), "S2 pairs")]


def structural_pairs(name, RL):
    """The structurally distinct pairs of the address map: ((mate, p), (mate', p')), s from the read's tail."""
    s = (RL - 2) // 8 - 1 if (RL - 2) // 8 >= 1 else 0
    within = [(8 * s, 8 * s + 1), (8 * s + 1, 8 * s + 2), (8 * s + 3, 8 * s + 4), (8 * s + 7, 8 * s + 8), (0, RL - 1)]
    tile = 32 * MAIN_NI.get(name, 0)
    if tile and tile < RL:  # a model of several tiles: the last position of a tile and the first of the next (the last boundary)
        t = (RL - 1) // tile * tile
        within.append((t - 1, t))
    within = [(a, b) for a, b in within if 0 <= a < b < RL]
    pairs = [((o, a), (o, b)) for o in range(2) for a, b in within]
    pairs += [((0, p), (1, p)) for p in sorted({0, min(5, RL - 1), RL - 1})]
    return pairs


class S3(_Stat):
    """Full joint tables of chosen pairs of columns against the bin mixture: chi-square (dependence of any shape)."""

    def __init__(self, dense, pairs, positions=None, expect=None):
        _Stat.__init__(self, dense, positions, expect)
        col = {nm: c for c, nm in enumerate(self.names)}
        self.pairs = [(a, b) for a, b in pairs]
        self.cols = [(col[a], col[b]) for a, b in self.pairs]
        self.tab = np.zeros((len(self.cols), self.K * self.K), dtype=np.int64)

    ACC = ("tab",)

    def add(self, s):
        q = self.flat(s["Q"])
        assert int(q.max()) < self.K, "a phred beyond the model's"
        for i, (a, b) in enumerate(self.cols):
            self.tab[i] += np.bincount(q[:, a].astype(np.int64) * self.K + q[:, b], minlength=self.K * self.K)
        self.n += q.shape[0]

    def results(self):
        best, m = Result("S3 joint", 1.0, None, 0, 1, 0.0), 0
        for i, ((oa, pa), (ob, pb)) in enumerate(self.pairs):
            if oa == ob:
                e = np.einsum("b,bi,bj->ij", self.x.w[oa], self.x.pm[oa][:, pa], self.x.pm[oa][:, pb])
            else:
                e = np.outer(self.x.marg[oa, pa], self.x.marg[ob, pb])
            stat, df, p = chi_square(self.tab[i], self.n * e)
            m += df > 0 or p == 0.0
            if p < best.p:
                best = Result("S3 joint", p, self.pairs[i], 0, 1, round(stat, 2))
        return [best._replace(m=m)]


class S4(_Stat):
    """Across reads: every entry of the cross matrix of the scores of two sets of rows has expectation 0.  ``add`` takes the
    pair lags inside a slice, ``add_cross`` two slices of equal length (two seeds, two calls)."""

    def __init__(self, dense, positions=None, expect=None, lags=LAGS):
        _Stat.__init__(self, dense, positions, expect)
        self.acc = collections.OrderedDict()
        self.lags = lags

    def _acc(self, key, A, A2, B, B2):
        a = self.acc.setdefault(key, [0, 0, 0])
        a[0] = a[0] + gram(A, B)
        a[1] = a[1] + gram(A2, B2)
        a[2] += A.shape[0]

    def add(self, s):
        S, S2_ = self.scores(s)
        for k in self.lags:
            if S.shape[0] > k:
                self._acc("lag %d" % k, S[:-k], S2_[:-k], S[k:], S2_[k:])

    def add_cross(self, key, sa, sb):
        self._acc(key, *(self.scores(sa) + self.scores(sb)))

    def merge(self, other):
        for key, (x, v, n) in other.acc.items():
            a = self.acc.setdefault(key, [0, 0, 0])
            a[0], a[1], a[2] = a[0] + x, a[1] + v, a[2] + n

    def results(self):
        out = []
        for key, (x, v, n) in self.acc.items():
            X, V = x / n, v / n
            se = np.sqrt(np.maximum(V - X * X, 0.0) / n)
            Z = np.where(se > 0, X / np.where(se > 0, se, 1.0), 0.0)
            out.append(_worst_z(Z, se > 0, (self.names, self.names), "S4 " + key))
        return out


class S5(_Stat):
    """Error given phred: per mate and phred value, the count of base != template against N * pe[q], exact binomial tails."""

    def __init__(self, dense, positions=None, expect=None, letters_only=False):
        _Stat.__init__(self, dense, positions, expect)
        self.letters_only = letters_only
        self.N = np.zeros((2, self.K), dtype=np.int64)
        self.k = np.zeros((2, self.K), dtype=np.int64)

    ACC = ("N", "k")

    def add(self, s):
        err, _, counted = self.errors(s, self.letters_only)
        Q = self.flat(s["Q"])
        for o in range(2):
            sl = slice(o * self.P, (o + 1) * self.P)
            q = Q[:, sl].reshape(-1) if counted is None else Q[:, sl][counted[:, sl]]
            self.N[o] += np.bincount(q, minlength=self.K)[: self.K]
            self.k[o] += np.bincount(Q[:, sl][err[:, sl]], minlength=self.K)[: self.K]

    def results(self):
        best, m = Result("S5 error|phred", 1.0, None, 0, 2, 0), 0
        for o in range(2):
            for q in range(self.K):
                N, k, pe = int(self.N[o, q]), int(self.k[o, q]), min(float(self.x.pe[q]), 1.0)
                if N * pe < 5:
                    continue
                m += 1
                p = float(min(sps.binom.cdf(k, N, pe), sps.binom.sf(k - 1, N, pe)))
                if p < best.p:
                    best = Result("S5 error|phred", p, (o, "phred %d" % q, "N %d, expected %.1f" % (N, N * pe)), 0, 2, k)
        return [best._replace(m=m)]


class S6(_Stat):
    """Error residuals r = err - pe[q].  Every entry of R^T S, the diagonal included, has expectation 0 given the phreds, with
    variance sum pe (1 - pe) s^2 (the error tests are independent of every quality draw); tested where the column expects at
    least MIN_ERRORS errors: the entry is a sum over a Poisson-like number of error events, and the normal tail at the z of 7
    that the family's bound asks is only as good as that number is large (third-moment correction of the quantile: about
    z^2 / (6 sqrt(events)), 0.8 at 100 events; the shipped models expect hundreds to thousands per column at N_PAIRS).  Double errors of every pair of columns against lambda = sum pe pe': Poisson tails."""

    def __init__(self, dense, positions=None, expect=None, letters_only=False):
        _Stat.__init__(self, dense, positions, expect)
        self.letters_only = letters_only
        self.rs, self.vrs, self.dd, self.lam = (np.zeros((self.C, self.C)) for _ in range(4))
        self.expected_errors = np.zeros(self.C)

    ACC = ("rs", "vrs", "dd", "lam", "expected_errors")
    MIN_ERRORS = 100.0

    def add(self, s):
        err, PE, _ = self.errors(s, self.letters_only)
        S, S2_ = self.scores(s)
        E = err.astype(np.float32)
        self.rs += gram(E - PE, S)
        self.vrs += gram(PE - PE * PE, S2_)
        self.dd += gram(E, E)
        self.lam += gram(PE, PE)
        self.expected_errors += PE.sum(axis=0, dtype=np.float64)
        self.n += S.shape[0]

    def results(self):
        ok = (self.vrs > 0) & (self.expected_errors >= self.MIN_ERRORS)[:, None]
        Z = np.where(ok, self.rs / np.sqrt(np.where(ok, self.vrs, 1.0)), 0.0)
        out = [_worst_z(Z, ok, (self.names, self.names), "S6 residual")]
        iu = np.triu_indices(self.C, 1)
        D, lam = np.rint(self.dd[iu]), self.lam[iu]
        tested = lam > 0
        if (D[~tested] > 0).any():
            i = int(np.flatnonzero(~tested & (D > 0))[0])
            return out + [Result("S6 double errors", 0.0, (self.names[iu[0][i]], self.names[iu[1][i]]), 1, 2, float(D[i]))]
        if not tested.any():
            return out + [Result("S6 double errors", 1.0, None, 0, 2, 0.0)]
        lam_ = np.where(tested, lam, 1.0)
        p = np.where(tested, np.minimum(sps.poisson.cdf(D, lam_), sps.poisson.sf(D - 1, lam_)), 1.0)
        i = int(np.argmin(p))
        where = (self.names[iu[0][i]], self.names[iu[1][i]], "expected %.2f" % lam[i])
        return out + [Result("S6 double errors", float(p[i]), where, int(tested.sum()), 2, float(D[i]))]


class S7(_Stat):
    """Alternative choice: per (mate, template base) the counts of the three alternatives against
    sum_p n_err(p, base) * P(alt | p, base) -- conditional on where the errors fell: chi-square."""

    def __init__(self, dense, positions=None, expect=None):
        _Stat.__init__(self, dense, positions, expect)
        self.cnt = np.zeros((2, 4, 3), dtype=np.int64)
        self.nerr = np.zeros((2, self.P, 4), dtype=np.int64)
        self.impossible = 0

    ACC = ("cnt", "nerr", "impossible")

    def add(self, s):
        for o in range(2):
            B, T = s["B"][:, o], s["T"][:, o]
            i, j = np.nonzero(B != T)
            c, b = _CODE[T[i, j]], B[i, j]
            i, j, c, b = i[c < 4], j[c < 4], c[c < 4], b[c < 4]
            match = self.x.alt[o][self.pos[j], c] == b[:, None]  # [errors, 3]
            self.impossible += int((~match.any(axis=1)).sum())
            k = np.argmax(match, axis=1)
            good = match.any(axis=1)
            self.cnt[o] += np.bincount((c * 3 + k)[good], minlength=12).reshape(4, 3)
            self.nerr[o] += np.bincount((j * 4 + c)[good], minlength=self.P * 4).reshape(self.P, 4)

    def results(self):
        if self.impossible:
            return [Result("S7 alternative", 0.0, "a letter that is no alternative of its template base", 1, 1, self.impossible)]
        best, m = Result("S7 alternative", 1.0, None, 0, 1, 0.0), 0
        for o in range(2):
            e = np.einsum("pc,pck->ck", self.nerr[o].astype(np.float64), self.x.alt_pmf[o][self.pos])
            for c in range(4):
                stat, df, p = chi_square(self.cnt[o, c], e[c])
                m += df > 0 or p == 0.0
                if p < best.p:
                    best = Result("S7 alternative", p, (o, chr(BASES[c]), self.cnt[o, c].tolist(), np.round(e[c], 1).tolist()), 0, 1, round(stat, 2))
        return [best._replace(m=m)]


class S8(object):
    """Coordinates: insert-size PMF (chi-square; the truncated normal's with a custom fragment length), the forward start
    (fs + 0.5) / (L - fragment) over 64 equal bins, an 8 x 8 table of it against the insert size's octile, and its lag-1
    covariance across pairs.  The forward start is a uniform integer below W = L - fragment, so a bin of the 64 holds 1/64 of
    the mass up to 1/W: with W above 1e5 that moves a cell's expectation by less than 1e-3 of its standard deviation at 2^21
    pairs."""

    def __init__(self, dense, genome_length, fragment=None, expect=None):
        self.d, self.x, self.L, self.fragment = dense, expect or Expect(dense), genome_length, fragment
        RL = dense.read_length
        if fragment is None:
            self.lo, pmf = 0, self.x.isize_pmf
        else:
            lo, hi = int(fragment[0] - 12 * fragment[1]) - 2 * RL, int(fragment[0] + 12 * fragment[1]) - 2 * RL
            self.lo, pmf = lo, fragment_pmf(fragment[0], fragment[1], RL, lo, hi)[1]
        self.pmf = pmf
        F = np.cumsum(pmf) - pmf / 2
        self.octile = np.minimum((F * 8).astype(np.int64), 7)
        self.oct_p = np.bincount(self.octile, weights=pmf, minlength=8)
        self.isz = np.zeros(len(pmf), dtype=np.int64)
        self.u64 = np.zeros(64, dtype=np.int64)
        self.tab = np.zeros(64, dtype=np.int64)
        self.lag, self.nlag, self.n = 0.0, 0, 0

    def add(self, s):
        c = s["coords"]
        RL = self.d.read_length
        k = c[:, 3] - self.lo
        assert (k >= 0).all() and (k < len(self.pmf)).all(), "an insert size outside the model's"
        W = self.L - (c[:, 3] + 2 * RL)
        assert (W > 1e5).all() and (c[:, 0] >= 0).all() and (c[:, 0] < W).all()
        assert (c[:, 2] == c[:, 0] + 2 * RL + c[:, 3]).all(), "a pair that fell back"
        u = (c[:, 0] + 0.5) / W
        self.isz += np.bincount(k, minlength=len(self.pmf))
        self.u64 += np.bincount((u * 64).astype(np.int64), minlength=64)
        self.tab += np.bincount((u * 8).astype(np.int64) * 8 + self.octile[k], minlength=64)
        v = u - 0.5
        self.lag += float((v[:-1] * v[1:]).sum())
        self.nlag += len(v) - 1
        self.n += len(c)

    def merge(self, other):
        for name in ("isz", "u64", "tab", "lag", "nlag", "n"):
            setattr(self, name, getattr(self, name) + getattr(other, name))

    def results(self):
        n = self.n
        out = []
        for name, obs, e in (("S8 insert size", self.isz, n * self.pmf), ("S8 forward start", self.u64, np.full(64, n / 64.0)),
                             ("S8 start x insert", self.tab, n * np.outer(np.full(8, 0.125), self.oct_p).ravel())):
            stat, df, p = chi_square(obs, e)
            out.append(Result(name, p, "df %d" % df, int(df > 0 or p == 0.0), 1, round(stat, 2)))
        z = self.lag / np.sqrt(self.nlag / 144.0)
        out.append(Result("S8 start lag 1", float(sps.norm.sf(abs(z))), None, 1, 2, round(z, 3)))
        return out


def run(make, slices, threads=1):
    """The results of ``run_stats``, one list."""
    return [r for st in run_stats(make, slices, threads) for r in st.results()]


def run_stats(make, slices, threads=1):
    """Feed every slice to every statistic of ``make()`` and hand the statistics back.  With threads, each worker thread owns a set of
    statistics and takes one slice at a time (numpy and BLAS release the interpreter lock); the sets are merged at the end, and
    no more than ``threads`` slices are alive at once."""
    import concurrent.futures
    import contextlib
    import queue

    single_blas = contextlib.nullcontext()
    if threads > 1:  # every worker thread with a BLAS of one thread, or the workers' products fight over the cores
        try:
            from threadpoolctl import threadpool_limits

            single_blas = threadpool_limits(limits=1, user_api="blas")
        except ImportError:
            threads = 1
    sets = [make() for _ in range(max(1, threads))]
    free = queue.Queue()
    for st in sets:
        free.put(st)

    def work(stats, s):
        try:
            for st in stats:
                st.add(s)
        finally:
            free.put(stats)

    with single_blas, concurrent.futures.ThreadPoolExecutor(len(sets)) as pool:
        jobs = []
        for s in slices:
            jobs.append(pool.submit(work, free.get(), s))
        for j in jobs:
            j.result()
    for other in sets[1:]:
        for a, b in zip(sets[0], other):
            a.merge(b)
    return sets[0]
