"""The pair setup of a sample of read pairs, held to the model on short records (no GPU, no library code; beside
tests/philox_stats.py and tests/philox_indel_stats.py).

tests/philox_stats.py holds the per-base draws, and of the coordinates one regime: S8 asserts ``W > 1e5`` and "a pair that fell
back" away, so it sees long records on which no branch of simulate_read (iss/generator.py:121-176) is taken.  What `K_PAIR`,
`K_FS`, `K_RS`, `K_FRAG` and the `attempt` field do elsewhere -- the fallback start, the reverse-end fallback, the rejection loop
of randbelow, custom fragment lengths below 2 RL, gc_bias, a batch over short records -- oracle and device restate alike, so an
error of those rows of the map passes every parity test.  Here:

``pair_rule``     C0, exact, every pair: what (fs, rs, re, isz) may be on a record of L bases.
``sample_setup``  a plain float64 / integer numpy sampler written from the reference's text (generator.py:69-95, :121-176,
                  kde.py:74, :97, CPython's Random._randbelow_with_getrandbits), which keeps its raw material -- 32-bit candidate
                  words of the two rejection loops, the uniforms of insert size, bins, gc and the polar candidates -- so that
                  ``defect`` plants what a map error would have produced on words.
C1 .. C6, G1      statistics that accumulate over slices; expectations of a bin count VALUES, they are never 1 / bins: a
                  uniform integer below w puts #{v < w: bin(v) = b} / w into bin b, which is exact at any w, 1 included.

Coordinates of a slice: ``coords`` int64 [n, 4] = (fs, rs, re, isz), record coordinates.  PITs: insert size F(s) - pmf(s) / 2,
start (fs + 1/2) / n1(s), end (re - RL + 1/2) / (L - RL) where the reverse end fell back (0 after centring elsewhere): each has
mean 1/2 exactly, given everything drawn before it."""
import collections

import numpy as np
from scipy import stats as sps

import philox_stats as PS
from helpers import dense_model, mixed_genome, random_genome
from philox_stats import LAGS, Result, chi_square, fragment_pmf, gram

WORDS = 40       # candidate words kept per rejection loop: a loop rejects at most half, 2^-40 a pair that it needs more
POLAR = 24       # polar candidates kept per pair (a candidate is rejected with 1 - pi / 4: 1e-16 a pair that it needs more)
ATTEMPTS = 14    # gc_bias attempts of a pair at most (0.1^14)
GC_KEEP = 0.90   # generator.py:88, the double

# The cases of tests/test_gpu_philox_setup_stats.py.  ``L``: record length from the read length; ``stats``: what the case holds
# besides C0; ``defects``: the defects of ``sample_setup`` the case answers for, each with the statistic meant for it.
Case = collections.namedtuple("Case", "model L mixed fragment gc stats defects")
CASES = collections.OrderedDict([
    ("fallback-pow2", Case("novaseq", lambda RL: RL + 64, False, None, False, "C1 C2 C3 C4 C5", (("q", "C4"), ("t", "C5"), ("hq", "C4")))),
    ("fallback-3q", Case("novaseq", lambda RL: RL + 96, False, None, False, "C1 C2 C3 C4", (("q", "C4"), ("r", "C3")))),
    ("mixed-hiseq", Case("hiseq", lambda RL: 2 * RL + 516, False, None, False, "C1 C2 C3 C4 C5 C6",
                         (("q", "C4"), ("s", "C4"), ("t", "C5"), ("u", "C6"), ("v", "C6")))),
    ("mixed-miseq", Case("miseq", lambda RL: 2 * RL + 154, True, None, False, "C1 C2 C3 C4 C5 C6",
                         (("q", "C4"), ("s", "C4"), ("t", "C5"), ("u", "C6"), ("v", "C6")))),
    ("fragment-overlap", Case("novaseq", lambda RL: 1000, False, (322.0, 40.0), False, "C1 C2 C3 C5", (("r", "C2"),))),
    ("fragment-cut", Case("novaseq", lambda RL: 400, False, (100.0, 60.0), False, "C1 C2 C3", (("r", "C2"),))),
    ("long", Case("novaseq", lambda RL: 400_000, False, None, False, "C6", (("u", "C6"), ("v", "C6")))),
    ("gc", Case("hiseq", lambda RL: 20_000, False, None, True, "G1", (("w", "G1"), ("x", "G1")))),
    ("gc-fallback", Case("hiseq", lambda RL: 2 * RL + 516, False, None, True, "G1", (("w", "G1"), ("x", "G1")))),
])
# Pairs of a GPU case: the smallest power of two at which every defect of the case is rejected on ``sample_setup`` by the
# statistic meant for it, p a factor 100 inside the Bonferroni bound of the whole family the GPU test function tests
# (tests/test_philox_setup_stats_host.py::test_every_planted_defect_is_rejected, which also shows that half the size leaves one
# standing; DESIGN section 4 has every p).  Cap 2^21.
N_PAIRS = {"fallback-pow2": 1 << 17, "fallback-3q": 1 << 10, "mixed-hiseq": 1 << 12, "mixed-miseq": 1 << 12, "fragment-overlap": 1 << 10,
           "fragment-cut": 1 << 12, "long": 1 << 20, "gc": 1 << 16, "gc-fallback": 1 << 16}
# The gc_bias cases are sized by what their null needs, not by the defects ((w) and (x) are rejected from 2^9 pairs on): the
# redrawn pairs are a tenth of a case, and S4's normal tail at the |z| of 7 its family asks is wrong on a thousand rows of
# products of skewed scores -- the undamaged sampler shows a worst p of 2e-13 at 2^14 pairs where 1.6e-5 is expected, 2.2e-6 at
# 2^15, 1.5e-5 at 2^16, 2.9e-5 at 2^17 (measured, seed 7).  2^16 is the first size at which it is what it should be.
SIZED_BY_VALIDITY = ("gc", "gc-fallback")
DROPPED = {}
DEFECTS = ("q", "r", "s", "t", "u", "v", "w", "x", "hq")


# ------------------------------------------------------------------ C0
Rule = collections.namedtuple("Rule", "regular fell irregular n1")


def pair_rule(coords, L, RL, sequence_type="metagenomics"):
    """C0, every pair.  With s = isz, frag = s + 2 RL, width = L - frag and n1 = width where width > 0, else L - RL:
    0 <= fs < n1; with nat = fs + frag, re == nat where nat <= L (the edge width == 0, fs == 0 included: re == L and nothing
    falls back), else RL <= re < L; rs == re - RL.  Amplicon: fs == 0, re == L.  Returns the masks ``regular`` (the start was
    drawn below width), ``fell`` (the reverse end was drawn anew), ``irregular`` (a template cut by a record end) and n1; a
    violated pair is an AssertionError that names the first one."""
    c = np.asarray(coords, dtype=np.int64)
    fs, rs, re, s = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    assert RL < L, "the reference skips a record no longer than a read (generator.py:130)"
    frag = s + 2 * RL
    width = L - frag
    regular = width > 0
    n1 = np.where(regular, width, L - RL)
    if sequence_type == "amplicon":
        fell = np.zeros(len(c), dtype=bool)
        bad = (fs != 0) | (re != L)
    else:
        nat = fs + frag
        fell = nat > L
        bad = (fs < 0) | (fs >= n1) | np.where(fell, (re < RL) | (re >= L), re != nat)
    bad |= rs != re - RL
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("C0: pair %d of %d violates the rule (%d in all): fs %d rs %d re %d isz %d, L %d RL %d %s"
                             % (i, len(c), int(bad.sum()), fs[i], rs[i], re[i], s[i], L, RL, sequence_type))
    return Rule(regular, fell, (fs + RL > L) | (rs < 0), n1)


# ------------------------------------------------------------------ bins of a uniform integer
def bin_of(v, w, nb):
    """The bin of nb that (v + 1/2) / w falls into."""
    return ((2 * np.asarray(v, dtype=np.int64) + 1) * nb) // (2 * np.asarray(w, dtype=np.int64))


def bin_counts(w, nb):
    """#{0 <= v < w: bin_of(v, w, nb) == b}, int64 [len(w), nb]: v is in bin b or above iff v >= (2 w b + nb - 1) // (2 nb)."""
    w = np.atleast_1d(np.asarray(w, dtype=np.int64))
    lo = (2 * w[:, None] * np.arange(nb + 1)[None, :] + nb - 1) // (2 * nb)
    return np.diff(lo, axis=1)


def bin_probs(w, nb, drop0=None):
    """The PMF over nb bins of a uniform integer below w; ``drop0``: of one uniform on 1 .. w - 1 where set."""
    w = np.atleast_1d(np.asarray(w, dtype=np.int64))
    cnt = bin_counts(w, nb).astype(np.float64)
    den = w.astype(np.float64)
    if drop0 is not None:
        d = np.atleast_1d(drop0).astype(np.float64)
        cnt[:, 0] -= d
        den = den - d
    return cnt / den[:, None]


def _sum_probs(w, nb, drop0=None):
    """Sum of ``bin_probs`` over pairs, by distinct w."""
    if len(w) == 0:
        return np.zeros(nb)
    if drop0 is None:
        u, c = np.unique(w, return_counts=True)
        return c @ bin_probs(u, nb)
    u, c = np.unique(np.asarray(w, dtype=np.int64) * 2 + drop0, return_counts=True)
    return c @ bin_probs(u >> 1, nb, u & 1)


# ------------------------------------------------------------------ the geometry of a case
class Geo(object):
    """Record length, insert-size law and the PITs of a case."""

    def __init__(self, dense, L, fragment=None, sequence_type="metagenomics", expect=None):
        self.d, self.x, self.L, self.RL, self.fragment, self.sequence_type = dense, expect or PS.Expect(dense), int(L), dense.read_length, fragment, sequence_type
        if fragment is None:
            self.lo, self.pmf = 0, self.x.isize_pmf
        else:
            lo, hi = int(fragment[0] - 12 * fragment[1]) - 2 * self.RL, int(fragment[0] + 12 * fragment[1]) - 2 * self.RL
            self.lo, self.pmf = lo, fragment_pmf(fragment[0], fragment[1], self.RL, lo, hi)[1]
        self.F = np.cumsum(self.pmf) - self.pmf / 2
        self.octile = np.minimum((self.F * 8).astype(np.int64), 7)
        self.key = ("setup", id(self))

    def of(self, s):
        """C0 and the PITs of a slice, kept with it."""
        if self.key not in s:
            c = np.asarray(s["coords"], dtype=np.int64)
            rule = pair_rule(c, self.L, self.RL, self.sequence_type)
            k = c[:, 3] - self.lo
            assert (k >= 0).all() and (k < len(self.pmf)).all(), "an insert size outside the model's"
            n = self.L - self.RL
            P = np.zeros((len(c), 3))
            P[:, 0] = self.F[k] - 0.5
            P[:, 1] = (c[:, 0] + 0.5) / rule.n1 - 0.5
            P[:, 2] = np.where(rule.fell, (c[:, 2] - self.RL + 0.5) / n - 0.5, 0.0)
            s[self.key] = {"rule": rule, "k": k, "P": P, "oct": self.octile[k], "drop0": (rule.fell & (c[:, 3] + 2 * self.RL == self.L)).astype(np.int64)}
        return s[self.key]


# ------------------------------------------------------------------ the reference sampler and the defects
def _randbelow(words, n, fold=False):
    """CPython's Random._randbelow_with_getrandbits over rows: k = n.bit_length(), candidates word >> (32 - k), redraw while
    r >= n.  ``fold``: the defect (r), r mod n instead of a redraw.  (value, candidates rejected)."""
    n = np.asarray(n, dtype=np.int64)
    if len(n) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    assert (n >= 1).all() and (n < 2**32).all()
    k = np.frexp(n.astype(np.float64))[1].astype(np.int64)  # bit_length
    cand = words.astype(np.int64) >> (32 - k)[:, None]
    if fold:
        return cand[:, 0] % n, np.zeros(len(n), dtype=np.int64)
    ok = cand < n[:, None]
    assert ok.any(axis=1).all(), "a rejection loop longer than the words kept"
    first = np.argmax(ok, axis=1)
    return cand[np.arange(len(n)), first], first


def _draw_raw(rng, m, P, fragment):
    raw = {"u_isz": rng.random_sample(m), "u_bin": rng.random_sample((m, 2)), "u_gc": rng.random_sample(m),
           "fs_words": rng.randint(0, 2**32, size=(m, WORDS), dtype=np.uint32),
           "rs_words": rng.randint(0, 2**32, size=(m, WORDS), dtype=np.uint32)}
    if fragment is not None:
        raw["polar"] = rng.random_sample((m, POLAR, 2))
    if P:
        raw.update(uq=rng.random_sample((m, 2, P)), ue=rng.random_sample((m, 2, P)), ua=rng.random_sample((m, 2, P)))
    return raw


def _lead16(hi16, lo):
    """A uniform whose leading 16 bits are ``hi16`` and whose trailing bits are ``lo``'s."""
    return (hi16 + (lo * 65536 - np.floor(lo * 65536))) / 65536


def _damage(raw, defect, some):
    """What a map error does to the raw material of one attempt (see ``sample_setup``)."""
    if defect == "q":
        raw["rs_words"] = raw["fs_words"].copy()
    elif defect == "hq":
        raw["rs_words"][some] = raw["fs_words"][some]
    elif defect == "s":
        raw["fs_words"][:, 0] = (np.floor(raw["u_isz"] * 65536).astype(np.uint32) << 16) | (raw["fs_words"][:, 0] & 0xFFFF)
    elif defect == "t":
        m = len(raw["rs_words"])
        raw["rs_words"][1::2] = raw["rs_words"][0:m - 1:2][: len(raw["rs_words"][1::2])]
    elif defect == "u":
        raw["u_bin"][:, 0] = raw["u_isz"]
    elif defect == "v":
        raw["uq"][:, 0, 0] = _lead16((raw["fs_words"][:, 0] >> 16).astype(np.float64), raw["uq"][:, 0, 0])
    elif defect == "w":
        raw["u_gc"] = raw["u_isz"].copy()
    elif defect not in (None, "r", "x"):
        raise ValueError(defect)


def _setup(dense, raw, L, fragment, sequence_type, fold):
    """generator.py:121-176 on the raw material of m pairs: coords [m, 4] and the candidates each loop rejected."""
    d, RL = dense, dense.read_length
    m = len(raw["u_isz"])
    if fragment is not None:  # :122-123, np.random.normal: the legacy polar method, a fresh draw returns f * x2
        x = 2.0 * raw["polar"] - 1.0
        r2 = x[:, :, 0] ** 2 + x[:, :, 1] ** 2
        ok = (r2 < 1.0) & (r2 != 0.0)
        assert ok.any(axis=1).all(), "a polar loop longer than the candidates kept"
        t = np.argmax(ok, axis=1)
        r2, x2 = r2[np.arange(m), t], x[np.arange(m), t, 1]
        g = np.sqrt(-2.0 * np.log(r2) / r2) * x2
        frag = np.trunc(fragment[0] + fragment[1] * g).astype(np.int64)  # int()
        s = frag - 2 * RL
    else:
        s = np.searchsorted(d.isize_cdf, raw["u_isz"]).astype(np.int64)  # kde.py:97
        frag = s + 2 * RL
    rej = np.zeros((m, 2), dtype=np.int64)
    if sequence_type == "amplicon":  # :137, :168
        fs, rs, re = np.zeros(m, dtype=np.int64), np.full(m, L - RL, dtype=np.int64), np.full(m, L, dtype=np.int64)
    else:
        width = L - frag  # :135: randrange(0, width) raises ValueError where width <= 0; :144 then
        fs, rej[:, 0] = _randbelow(raw["fs_words"], np.where(width > 0, width, L - RL), fold)
        fs = np.maximum(fs, 0)
        rs = fs + RL + s  # :165
        re = rs + RL
    over = re > L  # :172-176
    re = re.copy()
    re[over], rej[over, 1] = _randbelow(raw["rs_words"][over], np.full(int(over.sum()), L - RL, dtype=np.int64), fold)
    re[over] += RL
    rs = re - RL
    return np.stack([fs, rs, re, s], axis=1), rej


def sample_setup(dense, n, seed, genome, positions=(), fragment=None, gc_bias=False, sequence_type="metagenomics", defect=None):
    """n pairs of the model on the record ``genome``: coordinates, and phreds, letters and templates at ``positions`` (through
    philox_stats._derive).  With ``gc_bias`` every candidate pair costs one uniform and is kept below 0.90, a rejected pair is
    drawn anew from fresh material (generator.py:82-92; the 40 < gc < 60 window is dead, gc_fraction is a fraction), and
    ``plain`` is the run of the same material without gc_bias.  ``seed``: an integer; the sample is a function of the
    arguments, so ``plant`` re-derives it with a defect:
    q   K_RS reads K_FS's words;                            r   a rejected candidate is folded (r mod n), not redrawn;
    s   the start's leading 16 bits are the insert-size uniform's;    t   pair i + 1 reuses pair i's K_RS words;
    u   the forward bin is drawn from the insert-size uniform;
    v   the quality digit of mate 0, position 0 is the leading 16 bits of K_FS word 0;
    w   the gc uniform is the insert-size uniform;          x   a redraw keeps attempt 0's K_FS words;
    hq  q in 1 % of the pairs."""
    d, RL = dense, dense.read_length
    g = np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)
    L, pos = len(g), np.asarray(positions, dtype=np.int64)
    args = dict(dense=dense, n=n, seed=seed, genome=genome, positions=positions, fragment=fragment, gc_bias=gc_bias, sequence_type=sequence_type)

    def attempt(a, m, keep_fs=None):
        rng = np.random.RandomState([int(seed), a])
        raw = _draw_raw(rng, m, len(pos), fragment)
        some = rng.random_sample(m) < 0.01
        if keep_fs is not None:
            raw["fs_words"] = keep_fs
        _damage(raw, defect, some)
        coords, rej = _setup(d, raw, L, fragment, sequence_type, defect == "r")
        out = {"coords": coords, "rejected": rej, "u_gc": raw["u_gc"]}
        if len(pos):
            U = {"bin": np.stack([np.minimum(np.searchsorted(d.bin_cdf[o], raw["u_bin"][:, o], side="right"), 3) for o in range(2)], axis=1),  # kde.py:74-78
                 "uq": raw["uq"], "ue": raw["ue"], "ua": raw["ua"], "T": PS.templates(g, coords, RL, pos)}
            out["Q"], out["B"] = PS._derive(d, U, pos)
            out["T"] = U["T"]
        if defect == "x":
            out["fs_words"] = raw["fs_words"]
        return out

    first = attempt(0, n)
    keys = [k for k in ("coords", "Q", "B", "T") if k in first]
    out = {k: first[k].copy() for k in keys}
    out.update(rejected=first["rejected"], args=args)
    if gc_bias:
        out["plain"] = {k: first[k] for k in keys}
        idx = np.flatnonzero(~(first["u_gc"] < GC_KEEP))
        for a in range(1, ATTEMPTS):
            if not len(idx):
                break
            nxt = attempt(a, len(idx), first["fs_words"][idx] if defect == "x" else None)
            for k in keys:
                out[k][idx] = nxt[k]
            idx = idx[~(nxt["u_gc"] < GC_KEEP)]
        assert not len(idx), "more gc_bias attempts than ATTEMPTS"
    return out


def plant(sample, defect):
    """The sample a map error would have given, from the same raw material."""
    return sample_setup(defect=defect, **sample["args"])


# ------------------------------------------------------------------ the statistics
class _C(object):
    ACC = ()

    def __init__(self, geo):
        self.g, self.n = geo, 0

    def merge(self, other):
        for name in self.ACC + ("n",):
            setattr(self, name, getattr(self, name) + getattr(other, name))


def _chi(name, obs, e):
    stat, df, p = chi_square(obs, e)
    return Result(name, p, "df %d" % df, int(df > 0 or p == 0.0), 1, round(stat, 2))


class C1(_C):
    """Insert sizes against the model's PMF (``fragment_pmf`` with a custom fragment length: the cells around frag = 0 are where
    int() folds two unit intervals): chi-square."""
    ACC = ("isz",)

    def __init__(self, geo):
        _C.__init__(self, geo)
        self.isz = np.zeros(len(geo.pmf), dtype=np.int64)

    def add(self, s):
        t = self.g.of(s)
        self.isz += np.bincount(t["k"], minlength=len(self.isz))
        self.n += len(t["k"])

    def results(self):
        return [_chi("C1 insert size", self.isz, self.n * self.g.pmf)]


class _Values(_C):
    """A uniform integer over 64 bins of its PIT, and value by value where every pair has the same w <= 128."""
    ACC = ("u64", "e64", "val")
    VALUES = 128

    def __init__(self, geo):
        _C.__init__(self, geo)
        self.u64, self.e64, self.val = np.zeros(64, dtype=np.int64), np.zeros(64), np.zeros(self.VALUES, dtype=np.int64)
        self.wmin, self.wmax = None, None

    def take(self, v, w):
        if not len(v):
            return
        self.u64 += np.bincount(bin_of(v, w, 64), minlength=64)
        self.e64 += _sum_probs(w, 64)
        self.wmin = int(w.min()) if self.wmin is None else min(self.wmin, int(w.min()))
        self.wmax = int(w.max()) if self.wmax is None else max(self.wmax, int(w.max()))
        if self.wmax <= self.VALUES:
            self.val += np.bincount(v, minlength=self.VALUES)
        self.n += len(v)

    def merge(self, other):
        _C.merge(self, other)
        for name, f in (("wmin", min), ("wmax", max)):
            a, b = getattr(self, name), getattr(other, name)
            setattr(self, name, b if a is None else a if b is None else f(a, b))

    def value_level(self):
        return self.n > 0 and self.wmin == self.wmax and self.wmax <= self.VALUES

    def results(self):
        if not self.n:
            return [Result(self.NAME, 1.0, "no pair", 0, 1, 0.0)]
        out = [_chi(self.NAME, self.u64, self.e64)]
        if self.value_level():
            out.append(_chi(self.NAME + " values", self.val[: self.wmax], np.full(self.wmax, self.n / float(self.wmax))))
        return out


class C2(_Values):
    """The forward start given the insert size: PIT (fs + 1/2) / n1(s) in 64 bins against sum_s N_s #{v < n1(s) in the bin} /
    n1(s) over the observed N_s."""
    NAME = "C2 start"

    def add(self, s):
        t = self.g.of(s)
        self.take(np.asarray(s["coords"])[:, 0], t["rule"].n1)


class C3(_Values):
    """The reverse end of the pairs that fell back: re - RL over its L - RL values, or over 64 bins above 128."""
    NAME = "C3 end"

    def add(self, s):
        t = self.g.of(s)
        f = t["rule"].fell
        self.take(np.asarray(s["coords"])[f, 2] - self.g.RL, np.full(int(f.sum()), self.g.L - self.g.RL, dtype=np.int64))


class C4(_C):
    """8 x 8 tables, expectations by counting values: start bin x end bin and end bin x insert-size octile among the pairs that
    fell back (given that, a start at width == 0 is uniform on 1 .. n1 - 1), start bin x insert-size octile over all pairs."""
    ACC = ("se", "e_se", "eo", "so", "e_so", "nf")

    def __init__(self, geo):
        _C.__init__(self, geo)
        self.se, self.eo, self.so = (np.zeros(64, dtype=np.int64) for _ in range(3))
        self.e_se, self.e_so, self.nf = np.zeros(64), np.zeros(64), 0

    def add(self, s):
        t, c = self.g.of(s), np.asarray(s["coords"])
        r, n = t["rule"], self.g.L - self.g.RL
        f = r.fell
        a8 = bin_of(c[:, 0], r.n1, 8)
        e8 = bin_of(c[f, 2] - self.g.RL, n, 8)
        self.se += np.bincount(a8[f] * 8 + e8, minlength=64)
        self.e_se += np.outer(_sum_probs(r.n1[f], 8, t["drop0"][f]), bin_probs(n, 8)[0]).ravel()
        self.eo += np.bincount(e8 * 8 + t["oct"][f], minlength=64)
        self.so += np.bincount(a8 * 8 + t["oct"], minlength=64)
        e = np.zeros((8, 8))
        for o in range(8):
            e[:, o] = _sum_probs(r.n1[t["oct"] == o], 8)
        self.e_so += e.ravel()
        self.nf += int(f.sum())
        self.n += len(c)

    def results(self):
        n_o = self.eo.reshape(8, 8).sum(axis=0)  # the octiles of the pairs that fell back, as observed
        return [_chi("C4 start x end", self.se, self.e_se),
                _chi("C4 end x insert", self.eo, np.outer(bin_probs(self.g.L - self.g.RL, 8)[0], n_o).ravel()),
                _chi("C4 start x insert", self.so, self.e_so)]


C5_PAIRS = (("start", 1, "start", 1), ("end", 2, "end", 2), ("start", 1, "end", 2), ("insert", 0, "insert", 0))


class C5(object):
    """Across pairs: the covariance of the centred PITs of pair i and pair i + k, k in LAGS, for (start, start), (end, end),
    (start, end), (insert, insert); ``add_cross`` the same between two sets at equal rows (two seeds, two calls, a redraw and
    the plain pair), ``add_rows`` over PIT rows the caller put together (a seam of two items).  Expectation 0, variance from
    the second-moment product as in S4."""

    def __init__(self, geo, lags=LAGS):
        self.g, self.lags, self.acc = geo, lags, collections.OrderedDict()

    def _acc(self, key, A, B):
        if not len(A):
            return
        a = self.acc.setdefault(key, [np.zeros(len(C5_PAIRS)), np.zeros(len(C5_PAIRS)), 0])
        for j, (_, ia, _, ib) in enumerate(C5_PAIRS):
            xy = A[:, ia] * B[:, ib]
            a[0][j] += xy.sum()
            a[1][j] += (xy * xy).sum()
        a[2] += len(A)

    def add_rows(self, P, prefix=""):
        for k in self.lags:
            if len(P) > k:
                self._acc("%slag %d" % (prefix, k), P[:-k], P[k:])

    def add(self, s):
        self.add_rows(self.g.of(s)["P"])

    def add_cross(self, key, sa, sb):
        self._acc(key, self.g.of(sa)["P"], self.g.of(sb)["P"])

    def merge(self, other):
        for key, (x, v, n) in other.acc.items():
            a = self.acc.setdefault(key, [np.zeros(len(C5_PAIRS)), np.zeros(len(C5_PAIRS)), 0])
            a[0], a[1], a[2] = a[0] + x, a[1] + v, a[2] + n

    def results(self):
        out = []
        names = ["%s x %s" % (a, b) for a, _, b, _ in C5_PAIRS]
        for key, (x, v, n) in self.acc.items():
            X, V = x / n, v / n
            se = np.sqrt(np.maximum(V - X * X, 0.0) / n)
            Z = np.where(se > 0, X / np.where(se > 0, se, 1.0), 0.0)
            out.append(PS._worst_z(Z, se > 0, (names,), "C5 " + key))
        return out


class C6(PS._Stat):
    """Setup against per-base draws: every phred column's mid-distribution score, and every column's error residual err -
    pe[q], against the three centred PITs -- [2 P x 3] each, every entry 0; score entries with the variance of the
    second-moment product (S4), residual entries with sum pe (1 - pe) pit^2 given phreds and setup (S6), counted where the
    column expects S6.MIN_ERRORS errors."""
    ACC = ("sx", "sv", "rx", "rv", "expected_errors")
    PITS = ("insert", "start", "end")

    def __init__(self, dense, geo, positions=None, expect=None, letters_only=False, errors=True):
        PS._Stat.__init__(self, dense, positions, expect or geo.x)
        self.g, self.letters_only, self.with_errors = geo, letters_only, errors
        self.sx, self.sv, self.rx, self.rv = (np.zeros((self.C, 3)) for _ in range(4))
        self.expected_errors = np.zeros(self.C)

    def add(self, s):
        P = self.g.of(s)["P"].astype(np.float32)
        P2 = P * P
        S, S2_ = self.scores(s)
        self.sx += gram(S, P)
        self.sv += gram(S2_, P2)
        if self.with_errors:
            err, PE, _ = self.errors(s, self.letters_only)
            self.rx += gram(err.astype(np.float32) - PE, P)
            self.rv += gram(PE - PE * PE, P2)
            self.expected_errors += PE.sum(axis=0, dtype=np.float64)
        self.n += S.shape[0]

    def results(self):
        n = self.n
        X, V = self.sx / n, self.sv / n
        se = np.sqrt(np.maximum(V - X * X, 0.0) / n)
        Z = np.where(se > 0, X / np.where(se > 0, se, 1.0), 0.0)
        out = [PS._worst_z(Z, se > 0, (self.names, self.PITS), "C6 score x setup")]
        if self.with_errors:
            ok = (self.rv > 0) & (self.expected_errors >= PS.S6.MIN_ERRORS)[:, None]
            Z = np.where(ok, self.rx / np.sqrt(np.where(ok, self.rv, 1.0)), 0.0)
            out.append(PS._worst_z(Z, ok, (self.names, self.PITS), "C6 residual x setup"))
        return out


def _rows_equal(a, b, keys):
    return [np.all(a[k].reshape(len(a[k]), -1) == b[k].reshape(len(b[k]), -1), axis=1) for k in keys]


def _take(s, idx, keys=("coords", "Q")):
    return {k: s[k][idx] for k in keys if k in s}


class G1(object):
    """gc_bias: a slice is {"a": the plain run, "b": the gc_bias run} of the same seed, ordinals and record (coords, Q, B).
    ``same``: coordinates and all four rows equal; a pair equal in part is a failure.  sum(same) against Binomial(n, 0.90),
    two-sided exact (a redraw equals the plain pair by chance with probability below 2^-100); the 2 x 2 table of same_i,
    same_{i+1} against independence at 0.90; same against the plain run's insert-size octile, start bin and every phred
    column's score (the rejection uniform shares its two Philox blocks with the insert size and both bins); and over the
    redrawn pairs, which are fresh draws of the model: C0 .. C3 and S1, and S4's cross matrix and C5 against the plain run's
    pair at the same ordinal (``attempt`` must change every stream)."""

    def __init__(self, dense, geo, positions=None, expect=None):
        x = expect or geo.x
        self.g, self.n, self.k, self.partial = geo, 0, 0, []
        self.t22, self.oct, self.st8 = np.zeros(4, dtype=np.int64), np.zeros((2, 8), dtype=np.int64), np.zeros((2, 8), dtype=np.int64)
        self.c1, self.c2, self.c3, self.c5 = C1(geo), C2(geo), C3(geo), C5(geo, lags=())
        self.s1, self.s4 = PS.S1(dense, positions, x), PS.S4(dense, positions, x, lags=())
        self.sc, self.sc2 = np.zeros(self.s1.C), np.zeros(self.s1.C)

    def add(self, s):
        a, b = s["a"], s["b"]
        eq = _rows_equal(a, b, ("coords", "Q", "B"))
        same = eq[0] & eq[1] & eq[2]
        some = np.zeros(len(same), dtype=bool)  # a mate's phreds equal, and not the whole pair
        for o in range(2):
            some |= np.all(a["Q"][:, o] == b["Q"][:, o], axis=1)
        if (some & ~same).any():
            self.partial.append(int(np.flatnonzero(some & ~same)[0]) + self.n)
        t = self.g.of(a)
        self.g.of(b)  # C0 on every pair of the gc_bias run
        self.k += int(same.sum())
        self.t22 += np.bincount(same[:-1] * 2 + same[1:], minlength=4)
        self.oct += np.bincount(same * 8 + t["oct"], minlength=16).reshape(2, 8)
        self.st8 += np.bincount(same * 8 + bin_of(np.asarray(a["coords"])[:, 0], t["rule"].n1, 8), minlength=16).reshape(2, 8)
        S, S2_ = self.s1.scores(a)
        r = (same - GC_KEEP).astype(np.float32)
        self.sc += r @ S
        self.sc2 += (r * r) @ S2_
        idx = np.flatnonzero(~same)
        ra, rb = _take(a, idx), _take(b, idx)
        if len(idx):
            for st in (self.c1, self.c2, self.c3, self.s1):
                st.add(rb)
            self.s4.add_cross("redraw x plain", ra, rb)
            self.c5.add_cross("redraw x plain", ra, rb)
        self.n += len(same)

    def merge(self, other):
        for name in ("n", "k", "partial", "t22", "oct", "st8", "sc", "sc2"):
            setattr(self, name, getattr(self, name) + getattr(other, name))
        for name in ("c1", "c2", "c3", "c5", "s1", "s4"):
            getattr(self, name).merge(getattr(other, name))

    def results(self):
        if self.partial:
            return [Result("G1 a pair equal in part", 0.0, "pair %d" % self.partial[0], 1, 1, len(self.partial))]
        n, k, p = self.n, self.k, GC_KEEP
        out = [Result("G1 share kept", float(min(sps.binom.cdf(k, n, p), sps.binom.sf(k - 1, n, p))), "%d of %d" % (k, n), 1, 2, round(k / float(n), 5))]
        out.append(_chi("G1 same_i x same_i+1", self.t22, self.t22.sum() * np.outer([1 - p, p], [1 - p, p]).ravel()))
        for name, tab in (("G1 same x insert octile", self.oct), ("G1 same x start bin", self.st8)):
            out.append(_chi(name, tab, np.outer([1 - p, p], tab.sum(axis=0)).ravel()))
        ok = self.sc2 > 0
        Z = np.where(ok, self.sc / np.sqrt(np.where(ok, self.sc2, 1.0)), 0.0)
        out.append(PS._worst_z(Z, ok, (self.s1.names,), "G1 same x score"))
        for st in (self.c1, self.c2, self.c3, self.s1, self.s4, self.c5):
            out += [r._replace(stat="G1 redrawn " + r.stat) for r in st.results()]
        return out


def case_stats(case, dense, geo, positions=None, letters_only=False):
    """The statistics of a case, in the order of its ``stats``."""
    make = {"C1": lambda: C1(geo), "C2": lambda: C2(geo), "C3": lambda: C3(geo), "C4": lambda: C4(geo), "C5": lambda: C5(geo),
            "C6": lambda: C6(dense, geo, positions, None, letters_only), "G1": lambda: G1(dense, geo, positions)}
    return [make[k]() for k in CASES[case].stats.split()]


def family(case, RL):
    """Hypotheses of the GPU test function of a case, every column read (an upper bound: a degenerate cell tests less)."""
    C = 2 * RL
    m = {"C1": 1, "C2": 2, "C3": 2, "C4": 3, "C5": len(C5_PAIRS) * len(LAGS), "C6": 2 * 3 * C,
         "G1": 1 + 1 + 2 + C + (1 + 2 + 2 + C + C * C + len(C5_PAIRS))}
    return sum(m[k] for k in CASES[case].stats.split())


def shares(geo, coords):
    """(regular, fell back, irregular) shares of a set of pairs."""
    r = pair_rule(coords, geo.L, geo.RL, geo.sequence_type)
    return float(r.regular.mean()), float(r.fell.mean()), float(r.irregular.mean())


def case_setup(case, sequence_type="metagenomics"):
    """(dense, genome, geo) of a case: the model without indels (the fix-up then holds the irregular pairs alone), the record
    random_genome(99) or mixed_genome(98) of the case's length."""
    c = CASES[case]
    dense = dense_model(c.model, indel=(0.0, 0.0))
    L = c.L(dense.read_length)
    genome = mixed_genome(98, L) if c.mixed else random_genome(99, L)
    return dense, genome, Geo(dense, L, c.fragment, sequence_type)


def sampler_positions(case, RL):
    """What ``run_sampler`` draws of the reads: nothing where the case reads coordinates, three positions for C6 (the defects
    sit at position 0), every position for G1 (rows that are equal in part must not be equal by chance)."""
    if CASES[case].gc:
        return tuple(range(RL))
    return (0, 1, RL - 1) if "C6" in CASES[case].stats else ()


def run_sampler(case, n, defect=None, seed=7, step=1 << 15):
    """{statistic: results} of the case's statistics over n pairs of ``sample_setup``, in slices."""
    c = CASES[case]
    dense, genome, geo = case_setup(case)
    pos = sampler_positions(case, dense.read_length)
    stats = case_stats(case, dense, geo, np.asarray(pos) if pos else None, c.mixed)
    for a in range(0, n, step):
        s = sample_setup(dense, min(step, n - a), seed * 1000003 + a, genome, pos, c.fragment, c.gc, defect=defect)
        if c.gc:
            s = {"a": s["plain"], "b": s}
        for st in stats:
            st.add(s)
    return collections.OrderedDict((k, st.results()) for k, st in zip(c.stats.split(), stats))
