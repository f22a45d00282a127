"""The indel events of a sample of read pairs, held to the model's tables (no GPU, no library code; beside tests/philox_stats.py).

tests/philox_stats.py stops where indels begin.  The event draws (`K_EV` of DESIGN section 4) are restated by oracle and device
alike, so an error of that row of the map -- a block that collides with a quality or error-test block, mate 1 on mate 0's draws,
draw j + 1 on draw j, a substitution table indexed by the position before the shift -- passes every parity test.  Here the
--store_mutations rows make the reference's loop observable:

``replay``  rebuilds, from the template (coordinates + genome) and a read's indel rows alone, the sequence as it stood before
mut_sequence and the state of every step of introduce_indels (iss/error_models/__init__.py:114-228): whether the step was live
(n < len, letter not ambiguous), which letter stood there, which of the five tests fired.  Written from the reference's text;
vectorised over reads by event rank (the k-th indel row of every read), only reads with rows are shifted.  Its exact assertions
are I0 (the counts ``i0`` of a slice: every one must be 0).

The one thing the rows cannot show: a deletion that pops the LAST element fails on ``mutable_seq[position]`` (:216) before its
row is recorded, and every later step fails on ``mutable_seq[nucl]`` (:190).  The deletion test at the last live element is
therefore left out of every at-risk set (``hidden``), and the read must equal one of the two candidates.

A test's outcome is independent of everything settled before it, so with p read from the tables at the replayed state the
residual X - p has mean 0 given the history.  Counts of two rare events together (event x event, event x error, event x
coordinate bin) are, given the history, sums of independent Bernoulli(p) over reads: their tails are bounded by the Poisson
tails at lambda = sum p (Hoeffding 1956: a Poisson-binomial sum is smaller in convex order), which is what I3 .. I5 use -- a
normal approximation would be wrong for cells that expect a handful of events.

Columns of the event matrices: c = ((mate * (RL - 1)) + step) * 2 + kind, kind 0 "any of the four insertion tests fired", kind
1 "the deletion fired".  In this order a column a < b of the same pair is settled before b."""
import collections

import numpy as np
from scipy import sparse
from scipy import stats as sps

import philox_stats as PS
from philox_stats import BASES, Result, _AMBIGUOUS, _CODE, _COMP, gram

PAD = 32  # letters of the template beyond the read: what adjust_seq_length may append, and room for insertions
MUT_DTYPE = np.dtype([("pair", "<i4"), ("mate", "i1"), ("type", "i1"), ("position", "<i2"), ("ref", "u1"), ("alt", "u1"),
                      ("quality", "<i2")], align=True)  # include/iss_mi355x.h: iss_mutation
EXCLUDED_SHARE = 0.005  # the hidden deletion tests are at most this share of a case's live steps (asserted)

# Pairs of a GPU case: the smallest power of two at which every kept defect of ``plant`` is rejected on ``sample_model`` by the
# statistic meant for it, p a factor 100 inside the bound of the family the GPU case tests
# (tests/test_philox_indel_stats_host.py::test_every_planted_defect_is_rejected).  Cap 2^20.
N_PAIRS = {"flat": 1 << 15, "patterned": 1 << 16, "patterned-plain": 1 << 16, "flat-cap": 1 << 20}
# "hm" reaches its bound at the cap only: the case "flat-cap" holds it there, over the first CAP_STEPS steps of both mates (cut by
# positions: the replay of a step needs nothing behind it, so the case needs no reads, only coordinates and early rows).
CAP_STEPS = 4
# Dropped, with the p-values at the cap in DESIGN section 4: "j" (a deletion and an error exclude each other: a LOWER tail at an
# expectation of a few), "p" (S7 pools over positions, and neighbouring positions' tables are close), "hi" (1 % of 0.1 %); flat:
# "o" cannot show (both mates have the same tables); patterned: the entries at steps 0 and 1 of mate 0 are 0 or 1e-4 for six of
# the ten tests, so "i", "n" and their kin expect too few events there -- the flat case holds them.
DROPPED = {"flat": ("j", "o", "p", "hi", "hm"), "patterned": ("i", "j", "n", "p", "hi", "hm")}
DEFECTS = ("i", "j", "k", "l", "m", "n", "o", "p", "hi", "hm")


def _bytes(genome):
    return np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)


def _upper_code(letters):
    """Index in BASES of ``.upper()`` of a letter, 4 for any other."""
    return _CODE[np.where((letters >= 97) & (letters <= 122), letters - 32, letters)]


def templates_ext(g, coords, W):
    """Template letters [n, 2, W], W >= RL: the perfect read and what adjust_seq_length appends behind it (:142-155) --
    full_sequence[read_end + i] forward, rev_comp(full_sequence[read_start - 1 - i]) reverse, "A" beyond either end."""
    j = np.arange(W, dtype=np.int64)
    fi = coords[:, 0].astype(np.int64)[:, None] + j
    ri = (coords[:, 2].astype(np.int64) - 1)[:, None] - j
    T = np.empty((len(coords), 2, W), dtype=np.uint8)
    T[:, 0] = np.where(fi < len(g), g[np.minimum(fi, len(g) - 1)], 65)
    T[:, 1] = np.where(ri >= 0, _COMP[g][np.maximum(ri, 0)], 65)
    return T


class Tables(object):
    """The model's indel tables by letter code (BASES order): ins[mate][step][code], dele[mate][step][code].  ``steps``: the
    statistics look at the first ``steps`` steps of the loop only (NS, CE follow)."""

    def __init__(self, dense, steps=None):
        d = dense
        self.RL, self.NS = d.read_length, d.read_length - 1 if steps is None else int(steps)  # steps: the first steps only
        self.steps = steps
        self.CE = 4 * self.NS
        self.ins = np.zeros((2, d.read_length, 4))
        for x in range(4):
            c = _CODE[d.ins_letter[:, :, x]]
            assert (c < 4).all()
            np.put_along_axis(self.ins, c[:, :, None], d.ins[:, :, x:x + 1], axis=2)
        self.dele = np.asarray(d.dele, dtype=np.float64)
        self.any_ins = 1.0 - np.prod(1.0 - self.ins, axis=2)

    def name(self, c):
        return (int(c) // 2 // self.NS, int(c) // 2 % self.NS, "del" if c & 1 else "ins")


# ------------------------------------------------------------------ the replay
def _shift_right(buf, r, p, letter):
    """mutable_seq.insert(p + 1, letter) on rows r."""
    J = np.arange(buf.shape[1])[None, :]
    new = np.take_along_axis(buf[r], J - (J > p[:, None]), axis=1)
    new[np.arange(len(r)), p + 1] = letter
    buf[r] = new


def _shift_left(buf, r, p):
    """mutable_seq.pop(p) on rows r."""
    J = np.arange(buf.shape[1])[None, :]
    buf[r] = np.take_along_axis(buf[r], np.minimum(J + (J >= p[:, None]), buf.shape[1] - 1), axis=1)


def replay(genome, coords, rows, RL, reads=None, steps=None):
    """The pre-substitution sequences and the per-step state of introduce_indels for the pairs of ``coords``, from the rows
    (MUT_DTYPE, ``pair`` counted from the slice's first pair, in the order iss_mutations_download documents).

    The work buffer of a read is its template followed by the letters adjust_seq_length would append: an insertion shifts both
    to the right, a pop to the left, so buffer[len + i] is always the i-th letter to append and the first RL letters are the
    adjusted sequence whether the loop left it longer (:137-139) or shorter (:140-155).

    Returns a dict: ``pre`` [n, 2, RL]; ``exam`` [n, 2, RL - 1] the letter the step looked at; ``live``, ``hidden`` (live, and
    the deletion test popped the last element if it fired); ``X`` uint8 [n, 2, RL - 1, 5] (insertion of A, T, C, G; deletion);
    ``i0`` the counts of the exact assertions.  ``reads`` [n, 2, RL]: the reads as they came out, for the substitution rows and
    the choice between the two candidates of a read with a hidden step.

    ``steps``: the state of the first ``steps`` steps only, from the indel rows below that position (a step's state depends on
    nothing behind it); no ``pre``, no ``reads``."""
    g = _bytes(genome)
    n, NS = len(coords), RL - 1 if steps is None else int(steps)
    W = NS + 1 + PAD
    if steps is not None:
        assert reads is None
        rows = rows[(rows["type"] != 0) & (rows["position"] < NS)]
    R = 2 * n
    i0 = collections.OrderedDict((k, 0) for k in ("row order", "row range", "indel ref", "event at a dead step", "sub row",
                                                  "read differs from replay", "hidden reads", "second candidate"))
    Text = templates_ext(g, coords, W)
    buf = Text.reshape(R, W).copy()
    X = np.zeros((R, NS, 5), dtype=np.uint8)
    popped = np.zeros((R, NS), dtype=np.uint8)
    rid_all = rows["pair"].astype(np.int64) * 2 + rows["mate"]
    is_sub = rows["type"] == 0
    key = rid_all * 2 + is_sub  # reads ascending, a read's indel rows before its substitution rows
    i0["row order"] += int((np.diff(key) < 0).sum())
    i0["row range"] += int(((rid_all < 0) | (rid_all >= R) | (rows["type"] < 0) | (rows["type"] > 2) | (rows["position"] < 0)
                            | (rows["position"] >= np.where(is_sub, RL, NS))).sum())
    ind, rid = rows[~is_sub], rid_all[~is_sub]
    pos = ind["position"].astype(np.int64)
    if len(ind):
        same = np.r_[False, rid[1:] == rid[:-1]]
        i0["row order"] += int((same & (np.r_[0, np.diff(pos)] < 0)).sum())  # loop order: positions never fall
        start = np.flatnonzero(~same)
        rank = np.arange(len(rid)) - np.repeat(start, np.diff(np.r_[start, len(rid)]))
        ln = np.full(R, RL, dtype=np.int64)
        for k in range(int(rank.max()) + 1):
            e = np.flatnonzero(rank == k)
            ins = ind["type"][e] == 1
            r, p, ref, alt = rid[e][ins], pos[e][ins], ind["ref"][e][ins], ind["alt"][e][ins]
            if r.size:
                i0["indel ref"] += int((buf[r, p] != ref).sum() + (_CODE[alt] > 3).sum() + (p >= ln[r]).sum())  # :202
                _shift_right(buf, r, p, alt)
                X[r, p, np.minimum(_CODE[alt], 3)] = 1
                ln[r] += 1
            r, p, ref = rid[e][~ins], pos[e][~ins], ind["ref"][e][~ins]
            if r.size:
                popped[r, p] = buf[r, p]
                _shift_left(buf, r, p)
                ln[r] -= 1
                i0["indel ref"] += int((buf[r, p] != ref).sum() + (p >= ln[r]).sum() + (ind["alt"][e][~ins] != 46).sum())  # :216
                X[r, p, 4] = 1
    nins, ndel = X[:, :, :4].sum(axis=2, dtype=np.int16), X[:, :, 4].astype(np.int16)
    lenat = RL + np.cumsum(nins - ndel, axis=1) - (nins - ndel)  # len(mutable_seq) when step n begins
    exam = np.where(popped > 0, popped, buf[:, :NS])
    step = np.arange(NS)[None, :]
    live = (step < lenat) & ~_AMBIGUOUS[exam]
    hidden = live & (step == lenat + nins - 1)
    i0["event at a dead step"] += int((X.any(axis=2) & ~live).sum() + (X[:, :, 4].astype(bool) & hidden).sum())
    pre = buf[:, :RL].copy() if steps is None else None
    either = np.zeros(R, dtype=bool)  # reads that both candidates explain (an unrecorded substitution can stand for the pop)
    if reads is not None:
        read = reads.reshape(R, RL)
        orig = Text.reshape(R, W)[:, :RL]
        sub, srid = rows[is_sub], rid_all[is_sub]
        spos = sub["position"].astype(np.int64)
        truth = read.copy()
        truth[srid, spos] = sub["ref"]
        has_row = np.zeros((R, RL), dtype=bool)
        has_row[srid, spos] = True
        i0["sub row"] += int((read[srid, spos] != sub["alt"]).sum() + (sub["ref"] == sub["alt"]).sum())

        def unexplained(cand, rr):  # a differing position without a row carries the original letter (:98)
            return ((truth[rr] != cand) & ~((read[rr] == orig[rr]) & ~has_row[rr])).any(axis=1)

        hr = np.flatnonzero(hidden.any(axis=1))
        i0["hidden reads"] += int(hr.size)
        if hr.size:
            h = np.argmax(hidden[hr], axis=1)
            candB = buf[hr].copy()
            _shift_left(candB, np.arange(hr.size), h)
            # the candidate that differs from the read at fewer positions: the other one's tail is off by a letter, and "carries
            # the original letter" explains a wrong tail by chance in one read of sixteen
            fewer = (truth[hr] != candB[:, :RL]).sum(axis=1) < (truth[hr] != pre[hr]).sum(axis=1)
            okA, okB = ~unexplained(pre[hr], hr), ~unexplained(candB[:, :RL], hr)
            takeB = okB & (~okA | fewer)
            either[hr[okA & okB & (candB[:, :RL] != pre[hr]).any(axis=1)]] = True
            pre[hr[takeB]] = candB[takeB][:, :RL]
            i0["second candidate"] += int(takeB.sum())
        i0["read differs from replay"] += int(unexplained(pre, np.arange(R)).sum())
    shape = (n, 2, NS)
    return {"pre": None if pre is None else pre.reshape(n, 2, RL), "exam": exam.reshape(shape), "live": live.reshape(shape), "hidden": hidden.reshape(shape),
            "X": X.reshape(n, 2, NS, 5), "i0": i0, "either": either.reshape(n, 2), "orig": Text[:, :, :RL] if steps is None else None}


def rows_of(rows, first, n):
    """The rows of pairs [first, first + n) of a call's rows, ``pair`` counted from ``first``."""
    a, b = np.searchsorted(rows["pair"], [first, first + n])
    out = rows[a:b].copy()
    out["pair"] -= first
    return out


def indel_slice(tables, genome, coords, bases, quals, rows, positions=None):
    """A slice for the statistics: the replay, and S5 .. S7's arrays with the replayed sequence as template.  ``bases``,
    ``quals`` [n, 2, RL]; ``positions``: the columns the phred statistics look at (None: all).  With ``tables.steps`` the
    events of the first steps alone (I1, I4, I5): no reads needed, ``bases`` and ``quals`` may be None."""
    t = tables
    rep = replay(genome, coords, rows, t.RL, reads=bases if t.steps is None else None, steps=t.steps)
    n = len(coords)
    pos = np.arange(t.RL) if positions is None else np.asarray(positions)
    i0 = rep["i0"]
    if t.steps is None:
        sub = rows[rows["type"] == 0]
        i0["sub row"] += int((quals[sub["pair"], sub["mate"], sub["position"]] != sub["quality"]).sum())
    live, at_del = rep["live"], rep["live"] & ~rep["hidden"]
    code = np.minimum(_upper_code(rep["exam"]), 3)
    X2 = np.empty((n, 2, t.NS, 2), dtype=np.float32)
    X2[..., 0] = rep["X"][..., :4].any(axis=3)
    X2[..., 1] = rep["X"][..., 4]
    P2 = np.empty((n, 2, t.NS, 2), dtype=np.float32)
    P2[..., 0] = live * t.any_ins[None, :, :t.NS]
    for o in range(2):
        P2[:, o, :, 1] = at_del[:, o] * t.dele[o][np.arange(t.NS)[None, :], code[:, o]]
    s = {"coords": coords, "rep": rep, "code": code, "at_del": at_del, "E2": sparse.csr_matrix(X2.reshape(n, t.CE)),
         "P2": P2.reshape(n, t.CE), "i0": i0}
    if t.steps is None:
        s.update({"Q": np.ascontiguousarray(quals[:, :, pos]), "B": np.ascontiguousarray(bases[:, :, pos]),
                  "T": np.ascontiguousarray(rep["pre"][:, :, pos])})
    return s


# ------------------------------------------------------------------ the plain sampler and the defects
def patterned_indel(dense, seed=11):
    """Indel tables that differ by mate, position and letter: every entry of ``ins`` and ``dele`` from {0, 1e-4, 1e-3, 1e-2} with
    weights (0.4, 0.3, 0.2, 0.1) -- about 1.8 events a read at RL 301."""
    rng = np.random.RandomState(seed)
    values = np.array([0.0, 1e-4, 1e-3, 1e-2])
    dense.ins[:] = values[rng.choice(4, size=dense.ins.shape, p=(0.4, 0.3, 0.2, 0.1))]
    dense.dele[:] = values[rng.choice(4, size=dense.dele.shape, p=(0.4, 0.3, 0.2, 0.1))]
    return dense


def _event_uniforms(seed, o, step, n):
    """The five uniforms of step ``step`` of mate ``o`` for n reads, in the reference's order (four insertion tests in the order
    of the model's dict, the deletion test): addressable, so that ``plant`` can hand one step another step's."""
    return np.random.RandomState([int(seed) & 0x7FFFFFFF, 7919, o, step]).random_sample((n, 5))


def _loop(dense, Text, U, defect, some, want_origin, steps=None):
    """introduce_indels + adjust_seq_length (:158-228, :114-156) for all reads at once, one loop step at a time."""
    d = dense
    n, RL, W = Text.shape[0], d.read_length, Text.shape[2]
    pre = np.empty((n, 2, RL), dtype=np.uint8)
    origin = np.zeros((n, 2, RL), dtype=np.int16) if want_origin else None
    events, fired = [], []
    planted = defect[1:] if defect in ("hi", "hm") else defect
    who = some if defect in ("hi", "hm") else np.ones(n, dtype=bool)
    for o in range(2):
        tab = 0 if defect == "o" else o
        buf = Text[:, o].copy()
        idx = np.tile(np.arange(W, dtype=np.int16), (n, 1)) if want_origin else None
        ln = np.full(n, RL, dtype=np.int64)
        for step in range(RL - 1 if steps is None else steps):
            u = _event_uniforms(U["ev_seed"], o, step, n)
            if step < 2 and planted in ("i", "j", "k", "l", "m", "n"):
                v = u.copy()
                if planted == "i" and o == 0:
                    v[:, 0] = U["uq"][:, 0, step]
                elif planted == "j" and o == 0:
                    v[:, 4] = U["ue"][:, 0, step]
                elif planted == "k" and o == 1:
                    v = _event_uniforms(U["ev_seed"], 0, step, n)
                elif planted == "l" and o == 0:
                    v[1::2] = u[0:n - 1:2][: len(v[1::2])]
                elif planted == "m" and o == 0 and step == 1:
                    v = _event_uniforms(U["ev_seed"], 0, 0, n)
                elif planted == "n" and o == 0 and step == 0:
                    v[:, 0] = U["ufs"]
                u = np.where(who[:, None], v, u)
            let = buf[:, step]
            live = (step < ln) & ~_AMBIGUOUS[let]  # :188-192 (IndexError on mutable_seq[nucl]: every later step fails too)
            thr = np.empty((n, 5))
            thr[:, :4] = d.ins[tab, step]
            thr[:, 4] = d.dele[tab, step][np.minimum(_upper_code(let), 3)]  # :209
            fire = (u < thr) & live[:, None]
            hit = np.flatnonzero(fire.any(axis=1))
            if not hit.size:
                continue
            for x in range(4):  # :193-207
                r = hit[fire[hit, x]]
                if r.size:
                    p = np.full(r.size, step)
                    _shift_right(buf, r, p, d.ins_letter[tab, step, x])
                    if want_origin:
                        _shift_right(idx, r, p, -1)
                    ln[r] += 1
                    events.append((r, o, step * 5 + x, 1, step, buf[r, step], np.full(r.size, d.ins_letter[tab, step, x])))
                    fired.append((r, o, step, int(_CODE[d.ins_letter[tab, step, x]])))
            r = hit[fire[hit, 4]]
            if r.size:  # :209-221
                p = np.full(r.size, step)
                _shift_left(buf, r, p)
                if want_origin:
                    _shift_left(idx, r, p)
                ln[r] -= 1
                rec = r[step < ln[r]]  # mutable_seq[position] of an emptied tail: IndexError, no row (:216)
                events.append((rec, o, step * 5 + 4, 2, step, buf[rec, step], np.full(rec.size, 46)))
                fired.append((r, o, step, 4))
        pre[:, o] = buf[:, :RL]
        if want_origin:
            origin[:, o] = idx[:, :RL]
    return pre, origin, events, fired


def _finish(dense, U, pre, origin, events, positions, Text):
    d = dense
    n, RL = pre.shape[0], d.read_length
    V = dict(U)
    V["T"] = np.ascontiguousarray(pre[:, :, positions])
    if origin is not None:  # defect p: the substitution table of the position the letter had before the shift
        V["subst_pos"] = np.clip(np.where(origin[:, :, positions] >= 0, origin[:, :, positions], positions[None, None, :]), 0, RL - 1)
    Q, Bp = _derive(d, V, positions)
    B = pre.copy()
    B[:, :, positions] = Bp
    quals = np.zeros((n, 2, RL), dtype=np.uint8)
    quals[:, :, positions] = Q
    orig = Text[:, :, :RL]
    i, o, j = np.nonzero((Bp != V["T"]) & (Bp != orig[:, :, positions]))  # :98: recorded unless it restores the original letter
    parts = [np.zeros(0, dtype=MUT_DTYPE)]
    order = [np.zeros(0, dtype=np.int64)]
    for r, oo, ordr, typ, p, ref, alt in events:
        a = np.zeros(len(r), dtype=MUT_DTYPE)
        a["pair"], a["mate"], a["type"], a["position"], a["ref"], a["alt"], a["quality"] = r, oo, typ, p, ref, alt, -1
        parts.append(a)
        order.append((r.astype(np.int64) * 2 + oo) * 100000 + ordr)
    a = np.zeros(len(i), dtype=MUT_DTYPE)
    a["pair"], a["mate"], a["type"], a["position"] = i, o, 0, positions[j]
    a["ref"], a["alt"], a["quality"] = V["T"][i, o, j], Bp[i, o, j], Q[i, o, j]
    parts.append(a)
    order.append((i.astype(np.int64) * 2 + o) * 100000 + 50000 + positions[j])
    rows = np.concatenate(parts)[np.argsort(np.concatenate(order), kind="stable")]
    return {"bases": B, "quals": quals, "rows": rows, "pre": pre}


def _derive(dense, U, positions):
    """philox_stats._derive with the substitution table's position of its own (``subst_pos``)."""
    if "subst_pos" not in U:
        return PS._derive(dense, U, positions)
    d = dense
    Q, B = PS._derive(d, U, positions)
    B = U["T"].copy()
    for o in range(2):
        for j, p in enumerate(positions):
            q = Q[:, o, j].astype(np.int64)
            err = U["ue"][:, o, j] > 1 - 10 ** (-q / 10)
            code = _CODE[U["T"][:, o, j]]
            sel = np.flatnonzero(err & (code < 4))
            if sel.size:
                pp, c = U["subst_pos"][sel, o, j], code[sel]
                cdf = d.subst_cdf[o][pp, c]  # [sel, 3]
                k = np.minimum((cdf <= U["ua"][sel, o, j][:, None]).sum(axis=1), 2)  # searchsorted(cdf, u, side="right")
                B[sel, o, j] = d.subst_alt[o][pp, c, k]
    return Q, B


def sample_model(dense, n, seed, genome, positions=None, keep=False, defect=None, steps=None):
    """n pairs of the model with its indels, float64 throughout: philox_stats.sample_model's coordinates and bins, then per mate
    the reference's loop (five uniforms per step, in its order; they are drawn for dead steps too and not looked at),
    adjust_seq_length, and the phreds, error tests and alternatives of ``positions`` on the shifted sequence.  Returns coords,
    bases, quals and ``pre`` (the sequence before mut_sequence) [n, 2, RL] and the rows in MUT_DTYPE, in the order iss_mutations_download documents; ``fired``: every test
    that fired as (pair, mate, step, slot), the hidden deletions included.  ``keep``: the uniforms, for ``plant``.
    ``steps``: the loop ends after that many steps -- for statistics over the first steps alone (Tables(steps=)), whose state
    nothing behind them changes."""
    d = dense
    RL = d.read_length
    rng = np.random.RandomState(seed)
    pos = np.arange(RL) if positions is None else np.asarray(positions)
    g = _bytes(genome)
    L, P = len(g), len(pos)
    isize = np.searchsorted(d.isize_cdf, rng.random_sample(n))
    width = L - (isize + 2 * RL)
    assert (width > 0).all()
    ufs = rng.random_sample(n)
    fs = np.floor(ufs * width).astype(np.int64)
    coords = np.stack([fs, fs + RL + isize, fs + 2 * RL + isize, isize], axis=1)
    w = np.diff(np.concatenate([np.zeros((2, 1)), d.bin_cdf], axis=1), axis=1)
    U = {"bin": np.stack([rng.choice(4, size=n, p=w[o] / w[o].sum()) for o in range(2)], axis=1),
         "uq": rng.random_sample((n, 2, P)), "ue": rng.random_sample((n, 2, P)), "ua": rng.random_sample((n, 2, P)),
         "ufs": ufs, "ev_seed": seed, "some": rng.random_sample(n) < 0.01, "steps": steps}
    out = _run(d, U, g, coords, pos, defect)
    if keep:
        out["U"], out["positions"], out["genome"] = U, pos, g
    return out


def _run(d, U, g, coords, pos, defect):
    if defect in ("i", "j", "hi"):
        assert pos[0] == 0 and pos[1] == 1, "defects i and j sit at positions 0 and 1"
    Text = templates_ext(g, coords, d.read_length + PAD)
    pre, origin, events, fired = _loop(d, Text, U, defect, U["some"], defect == "p", U.get("steps"))
    out = _finish(d, U, pre, origin, events, pos, Text)
    out["coords"] = coords
    out["fired"] = np.concatenate([np.stack([r, np.full(len(r), o), np.full(len(r), s), np.full(len(r), x)], axis=1)
                                   for r, o, s, x in fired] or [np.zeros((0, 4), dtype=np.int64)])
    return out


def plant(dense, sample, defect):
    """The sample a map error would have given, re-derived from the kept uniforms.  The defect sits at the first two steps of
    mate 0 unless it is about the mates:
    i   an insertion test (slot 0) on its position's quality uniform;   j   the deletion test on its position's error-test uniform;
    k   mate 1 on mate 0's event uniforms;                             l   pair i + 1 on pair i's;
    m   step 1 on step 0's uniforms;                                   n   step 0's first insertion test on the forward-start uniform;
    o   the reverse mate on the forward indel tables (every step);     p   the substitution table indexed by the position before
    the shift (every position);                                        hi, hm   i and m in 1 % of the reads."""
    if defect not in DEFECTS:
        raise ValueError(defect)
    return _run(dense, sample["U"], sample["genome"], sample["coords"], sample["positions"], defect)


# ------------------------------------------------------------------ the statistics
def _poisson(stat, D, lam, tested, name):
    """Two-sided Poisson tails of the counts D against lam over the cells ``tested``; a count where lam is 0 rejects."""
    D = np.rint(np.asarray(D, dtype=np.float64))
    lam = np.asarray(lam, dtype=np.float64)
    tested = tested & (lam > 0)
    wrong = (D > 0) & (lam <= 0)
    if wrong.any():
        at = tuple(int(v[0]) for v in np.nonzero(wrong))
        return Result(stat, 0.0, name(at) + ("expected 0",), int(tested.sum()) + 1, 2, float(D[at]))
    if not tested.any():
        return Result(stat, 1.0, None, 0, 2, 0.0)
    lam_ = np.where(tested, lam, 1.0)
    p = np.where(tested, np.minimum(sps.poisson.cdf(D, lam_), sps.poisson.sf(D - 1, lam_)), 1.0)
    at = np.unravel_index(int(np.argmin(p)), p.shape)
    return Result(stat, float(p[at]), name(at) + ("expected %.2f" % lam[at],), int(tested.sum()), 2, float(D[at]))


class _IStat(PS._Stat):
    def __init__(self, dense, positions=None, expect=None, tables=None):
        PS._Stat.__init__(self, dense, positions, expect)
        self.t = tables or Tables(dense)


class I1(object):
    """Rates.  Per (mate, step, inserted letter): fired against Binomial(live, ins); per (mate, step, letter looked at): fired
    against Binomial(live with that letter and not hidden, dele); exact two-sided binomial tails, every cell with p > 0 (an event
    in a cell with p = 0 rejects by itself).  The inserted letter's distribution is the slot dimension.  The nesting of the four
    bases' deletion events (one uniform in the reference) cannot be seen in rows -- a read shows one letter -- and stays with
    tests/test_oracle_golden.py::test_indel_event_process_is_the_product_of_the_reference_tests."""
    ACC = ("Ni", "Ki", "Nd", "Kd", "hidden", "live", "n")

    def __init__(self, tables):
        t = self.t = tables
        self.Ni, self.Ki = np.zeros((2, t.NS), dtype=np.int64), np.zeros((2, t.NS, 4), dtype=np.int64)
        self.Nd, self.Kd = np.zeros((2, t.NS, 4), dtype=np.int64), np.zeros((2, t.NS, 4), dtype=np.int64)
        self.hidden = self.live = self.n = 0

    def add(self, s):
        rep = s["rep"]
        self.Ni += rep["live"].sum(axis=0)
        self.Ki += rep["X"][..., :4].sum(axis=0, dtype=np.int64)
        fired = rep["X"][..., 4].astype(bool)
        for c in range(4):
            is_c = s["code"] == c
            self.Nd[:, :, c] += (s["at_del"] & is_c).sum(axis=0)
            self.Kd[:, :, c] += (fired & is_c).sum(axis=0)
        self.hidden += int(rep["hidden"].sum())
        self.live += int(rep["live"].sum())
        self.n += len(s["coords"])

    def merge(self, other):
        for name in self.ACC:
            setattr(self, name, getattr(self, name) + getattr(other, name))

    def excluded_share(self):
        return self.hidden / max(self.live, 1)

    def results(self):
        t, out = self.t, []
        for stat, N, K, p in (("I1 insertion rate", np.repeat(self.Ni[:, :, None], 4, axis=2), self.Ki, t.ins[:, :t.NS]),
                              ("I1 deletion rate", self.Nd, self.Kd, t.dele[:, :t.NS])):
            wrong = (K > 0) & (p <= 0)
            if wrong.any():
                at = tuple(int(v[0]) for v in np.nonzero(wrong))
                out.append(Result(stat, 0.0, at + ("a table entry of 0",), 1, 2, int(K[at])))
                continue
            tested = (p > 0) & (N > 0)
            if not tested.any():
                out.append(Result(stat, 1.0, None, 0, 2, 0))
                continue
            p_ = np.where(tested, p, 0.5)
            pv = np.where(tested, np.minimum(sps.binom.cdf(K, N, p_), sps.binom.sf(K - 1, N, p_)), 1.0)
            at = np.unravel_index(int(np.argmin(pv)), pv.shape)
            where = (int(at[0]), int(at[1]), chr(BASES[at[2]]), "N %d, expected %.1f" % (N[at], N[at] * p[at]))
            out.append(Result(stat, float(pv[at]), where, int(tested.sum()), 2, int(K[at])))
        return out


class I2(_IStat):
    """Events against phreds: every entry of R^T S, R the residuals X - p of the 4 (RL - 1) event columns, S the mid-distribution
    scores of the phred columns, has expectation 0 and variance sum s^2 p (1 - p) (the phreds do not depend on the sequence).
    Tested where the event column expects at least MIN_EVENTS events, as S6 does and for its reason."""
    ACC = ("rs", "vrs", "expected")
    MIN_EVENTS = 100.0

    def __init__(self, dense, positions=None, expect=None, tables=None):
        _IStat.__init__(self, dense, positions, expect, tables)
        self.rs, self.vrs = np.zeros((self.t.CE, self.C)), np.zeros((self.t.CE, self.C))
        self.expected = np.zeros(self.t.CE)

    def add(self, s):
        S, S2_ = self.scores(s)
        P = s["P2"]
        self.rs += np.asarray(s["E2"].T @ S, dtype=np.float64) - gram(P, S)
        self.vrs += gram(P - P * P, S2_)
        self.expected += P.sum(axis=0, dtype=np.float64)
        self.n += S.shape[0]

    def results(self):
        ok = (self.vrs > 0) & (self.expected >= self.MIN_EVENTS)[:, None]
        Z = np.where(ok, self.rs / np.sqrt(np.where(ok, self.vrs, 1.0)), 0.0)
        return [PS._worst_z(Z, ok, ([self.t.name(c) for c in range(self.t.CE)], self.names), "I2 event x phred")]


class I3(_IStat):
    """Events against the error path: the errors err = (base != replayed template) of every phred column among the reads in
    which an event column fired, against lambda = sum pe[q] over those reads (the events are settled before mut_sequence; given
    events and phreds the error tests are independent Bernoulli(pe)): Poisson tails, every cell with lambda > 0."""
    ACC = ("D", "lam")

    def __init__(self, dense, positions=None, expect=None, tables=None, letters_only=False):
        _IStat.__init__(self, dense, positions, expect, tables)
        self.letters_only = letters_only
        self.D, self.lam = np.zeros((self.t.CE, self.C)), np.zeros((self.t.CE, self.C))

    def add(self, s):
        err, PE, _ = self.errors(s, self.letters_only)
        self.D += np.asarray((s["E2"].T @ sparse.csr_matrix(err.astype(np.float32))).todense(), dtype=np.float64)
        self.lam += np.asarray(s["E2"].T @ PE, dtype=np.float64)
        self.n += err.shape[0]

    def results(self):
        return [_poisson("I3 event x error", self.D, self.lam, np.ones(self.D.shape, dtype=bool),
                         lambda at: (self.t.name(at[0]), self.names[at[1]]))]


class I4(object):
    """Events against events: the reads in which columns a and b both fired against lambda = sum over the reads in which a
    fired of p_b at the replayed state -- a settled before b: a < b inside a pair (an earlier step, insertions before the
    deletion of a step, mate 0 before mate 1), every (a, b) for pair i against pair i + k, another seed or another call.
    Poisson tails, every cell with lambda > 0."""

    def __init__(self, tables, lags=PS.LAGS, within=True):
        self.t, self.lags, self.within = tables, lags, within
        self.acc = collections.OrderedDict()

    def _acc(self, key, Ea, Eb, Pb):
        a = self.acc.setdefault(key, [0, 0])
        a[0] = a[0] + np.asarray((Ea.T @ Eb).todense(), dtype=np.float64)
        a[1] = a[1] + np.asarray(Ea.T @ Pb, dtype=np.float64)

    def add(self, s):
        E, P = s["E2"], s["P2"]
        if self.within:
            self._acc("within", E, E, P)
        for k in self.lags:
            if E.shape[0] > k:
                self._acc("lag %d" % k, E[:-k], E[k:], P[k:])

    def add_cross(self, key, sa, sb):
        self._acc(key, sa["E2"], sb["E2"], sb["P2"])

    def merge(self, other):
        for key, (D, lam) in other.acc.items():
            a = self.acc.setdefault(key, [0, 0])
            a[0], a[1] = a[0] + D, a[1] + lam

    def results(self):
        out = []
        for key, (D, lam) in self.acc.items():
            tested = np.triu(np.ones(D.shape, dtype=bool), 1) if key == "within" else np.ones(D.shape, dtype=bool)
            out.append(_poisson("I4 " + key, np.where(tested, D, 0.0), lam, tested, lambda at: (self.t.name(at[0]), self.t.name(at[1]))))
        return out


class I5(object):
    """Events against coordinates: the events of every column by forward-start bin (64) and by insert-size octile against
    lambda = sum p over the reads of the bin (the coordinates are drawn before the events): Poisson tails."""

    def __init__(self, dense, tables, genome_length, expect=None):
        self.t, self.s8 = tables, PS.S8(dense, genome_length, None, expect)
        self.D, self.lam = np.zeros((tables.CE, 72)), np.zeros((tables.CE, 72))

    def add(self, s):
        c, s8 = s["coords"], self.s8
        W = s8.L - (c[:, 3] + 2 * self.t.RL)
        u = (c[:, 0] + 0.5) / W
        n = len(c)
        G = sparse.csr_matrix((np.ones(2 * n, dtype=np.float32),
                               (np.r_[np.arange(n), np.arange(n)], np.r_[(u * 64).astype(np.int64), 64 + s8.octile[c[:, 3] - s8.lo]])),
                              shape=(n, 72))
        self.D += np.asarray((s["E2"].T @ G).todense(), dtype=np.float64)
        self.lam += np.asarray((G.T @ s["P2"]).T, dtype=np.float64)

    def merge(self, other):
        self.D, self.lam = self.D + other.D, self.lam + other.lam

    def results(self):
        return [_poisson("I5 event x coordinate", self.D, self.lam, np.ones(self.D.shape, dtype=bool),
                         lambda at: (self.t.name(at[0]), "start bin %d" % at[1] if at[1] < 64 else "insert octile %d" % (at[1] - 64)))]


class I0(object):
    """The exact assertions of the replay, summed over slices: every count but the last two must be 0."""

    def __init__(self):
        self.i0 = collections.OrderedDict()

    def add(self, s):
        for k, v in s["i0"].items():
            self.i0[k] = self.i0.get(k, 0) + v

    def merge(self, other):
        for k, v in other.i0.items():
            self.i0[k] = self.i0.get(k, 0) + v

    def failures(self):
        return {k: v for k, v in self.i0.items() if v and k not in ("hidden reads", "second candidate")}

    def results(self):
        return []


# ------------------------------------------------------------------ the cases, shared by the host and the GPU tests
GENOME = 400_000
FLAT = (0.001, 0.003)  # BASELINE configs[4]'s indel rates


def case_model(case):
    """(dense model, genome, mixed) of a case of tests/test_gpu_philox_indel_stats.py."""
    from helpers import dense_model, mixed_genome, random_genome

    if case == "flat":
        return dense_model("novaseq", FLAT), random_genome(99, GENOME), False
    if case == "patterned":
        return patterned_indel(dense_model("miseq")), mixed_genome(98, GENOME), True
    if case == "patterned-plain":  # the patterned tables on a record k_indel_script can work on: both indel routes
        return patterned_indel(dense_model("miseq")), random_genome(99, GENOME), False
    raise ValueError(case)


def all_stats(d, t, x, mixed, positions=None):
    return [I0(), I1(t), I2(d, positions, x, t), I3(d, positions, x, t, letters_only=mixed), I4(t),
            I5(d, t, GENOME, x), PS.S5(d, positions, x, letters_only=mixed), PS.S6(d, positions, x, letters_only=mixed),
            PS.S7(d, positions, x)]


def assert_accepted(stats):
    """One family per statistic class, as the GPU cases have it; I0 exact; the hidden steps within their share."""
    for st in stats:
        if isinstance(st, I0):
            assert not st.failures(), st.i0
        else:
            ok, text = PS.accept(st.results())
            assert ok, text
        if isinstance(st, I1):
            assert st.live > 0 and st.excluded_share() <= EXCLUDED_SHARE, st.excluded_share()
