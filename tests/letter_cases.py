"""Records with IUPAC and lower-case letters placed on purpose, the ledger of what the sampled pairs meet on them, and the cases
that hold every reader of genome letters to the oracle there.

Every kernel that turns genome positions into read letters has a route for plain A/C/G/T and one for "exception" letters (IUPAC
codes, lower case), and chooses between them from the exception mask (one bit a base, 32-bit words): k_setup's scan of the mask
words of both windows (meta bits 4/5), the funnel shift over two mask words in k_main<*, false, *>, main_slow_base's re-fetch,
k_indel_fixup's whole-read rebuild with padding from beyond the template, k_perfect's 64-bit window, the MT resolver's first- and
last-word masks (exceptions_in) and complement_ascii for the reverse mate.  helpers.mixed_genome makes one base in five an
exception: every window of every pair is flagged, and no off-by-one of a window scan can show.  A few N at arbitrary places
(mt_resolver_cases.genome, table_edges.sprinkled_genome) put a window's only exception on its first or last base less than once a
case.  The records here are what an assembly looks like -- isolated codes, scaffold gaps, soft-masked repeats -- with the letters
on the mask-word boundaries:

  bit0      one letter at every k * P, P = 32 * ceil((RL + 9) / 32): each is bit 0 of its mask word, at most one in a window
  bit31     one letter at every k * P + 31
  odd       one letter every RL + 10 (+ 1 if that is even) from position 5 on: the residues mod 32 cycle
  runs      runs of N of length 2 RL + 7, every 6 RL + 13: whole reads inside a run
  soft      the same geometry, the runs lower-case a/c/g/t
  sparse0   as bit0 / bit31 with period 32 * ceil(4 RL / 32).  For the MT legs: about half the pairs touch a letter (the rest are
  sparse31  the resolver's).  For the Philox legs: a pair meets one letter at most, so its route hangs on that one mask bit -- on
            bit0 / bit31 the neighbouring letter is always inside the whole mask words that k_setup scans for the other mate, and
            a window scan that stops a word short changes nothing (tried: see test_gpu_letter_cases.py)
  ends      small records for ONE generate_batch call in amplicon mode (fs = 0, re = L): lengths RL + 1 and 2 RL + k, k in 0, 1,
            31, 32, 33, each with one exception at one of 0, RL - 1, RL, L - RL - 1, L - RL, L - 1; a plain record before,
            between and behind them

The placed letters cycle through NRYWSMKHBVD, nrywsmkhbvd and acgt; the sample puts every one of them on both strands.

ledger() is plain numpy over the oracle's pair coordinates (no library code): per mate, how many windows have no exception
(none), a single one on their lowest / highest genome position (lo_only, hi_only), none inside and one on the base just outside
(below, above), nothing else (all); lo_only / hi_only with no other exception within ALONE bases of either window of the
pair (lo_alone, hi_alone); how many reads have an 8-base lane group that straddles two mask words with its exceptions in
the upper word only (group_upper_word); how many pairs have exactly one flagged mate (one_mate_only).  With mutation rows: reads
with net deletions whose adjust_seq_length padding holds an exception (pad_takes_exception) and substitution rows whose ref is
lower case (lower_substituted).  Every class a case names counts FLOOR per mate (tests/test_letter_cases_host.py)."""
import collections
import functools

import numpy as np

from helpers import dense_model, random_genome, synthetic_model

FLOOR = 16  # hits per mate a case must have in every class it names
SEED, FIRST_ORDINAL, MT_SEED = 77, 5, 4321
LETTERS = b"NRYWSMKHBVD" + b"nrywsmkhbvd" + b"acgt"
PLAIN = np.zeros(256, dtype=bool)
PLAIN[list(b"ACGT")] = True
WORKER_SEEDS = (40, 41, 42)


# ------------------------------------------------------------------ the records
def period(RL):
    return 32 * ((RL + 9 + 31) // 32)


def sparse_period(RL):
    return 32 * ((4 * RL + 31) // 32)


def _place(g, positions, first_letter=0):
    for k, p in enumerate(positions):
        g[p] = LETTERS[(first_letter + k) % len(LETTERS)]
    return g


def _plain(seed, n):
    return np.frombuffer(random_genome(seed, n).encode(), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def record(kind, RL):
    """The record `kind` for reads of RL bases, as a str."""
    P = period(RL)
    if kind == "plain":
        g = _plain(900 + RL, 40 * P)
    elif kind in ("bit0", "bit31"):
        g = _plain(901 + RL, 40 * P)
        _place(g, range(31 if kind == "bit31" else 0, len(g), P))
    elif kind in ("sparse0", "sparse31"):
        Q = sparse_period(RL)
        g = _plain(902 + RL, 48 * Q)
        _place(g, range(31 if kind == "sparse31" else 0, len(g), Q))
    elif kind == "odd":
        step = RL + 10 + (RL + 10 + 1) % 2
        g = _plain(903 + RL, 40 * P)
        _place(g, range(5, len(g), step))
        assert step % 2 == 1 and len({p % 32 for p in range(5, len(g), step)}) == 32
    elif kind in ("runs", "soft"):
        g = _plain(904 + RL, 40 * P)
        for a in range(2 * RL + 3, len(g) - (2 * RL + 7), 6 * RL + 13):
            if kind == "runs":
                g[a:a + 2 * RL + 7] = ord("N")
            else:
                g[a:a + 2 * RL + 7] |= 0x20
    else:
        raise KeyError(kind)
    return g.tobytes().decode()


ENDS_PAIRS = 1 << 11


@functools.lru_cache(maxsize=None)
def ends(RL):
    """The `ends` work list for reads of RL bases: (records, pair counts, exception position or None per record).  In amplicon
    mode every pair of a record has fs = 0 and re = L, so a record's exception is the first / last base of a window (0, RL - 1,
    L - RL, L - 1) or the base just outside one (RL, L - RL - 1) for every pair of it."""
    recs, where = [], []
    letter = 0
    for L in [RL + 1] + [2 * RL + k for k in (0, 1, 31, 32, 33)]:
        for p in sorted({0, RL - 1, RL, L - RL - 1, L - RL, L - 1}):
            recs.append(_plain(905 + RL + len(recs), L).tobytes().decode())
            where.append(None)
            recs.append(_place(_plain(905 + RL + len(recs), L), [p], letter).tobytes().decode())
            where.append(p)
            letter += 1
    recs.append(_plain(905 + RL + len(recs), RL + 1).tobytes().decode())
    where.append(None)
    n = len(recs)
    counts = [ENDS_PAIRS // n + (1 if k < ENDS_PAIRS % n else 0) for k in range(n)]
    assert sum(counts) == ENDS_PAIRS and min(counts) >= FLOOR
    return tuple(recs), tuple(counts), tuple(where)


# ------------------------------------------------------------------ the ledger
MATE_CLASSES = ("none", "lo_only", "hi_only", "below", "above", "all", "group_upper_word", "lo_alone", "hi_alone")
ALONE = 64  # two mask words


def _bytes(genome):
    return np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)


def ledger(genome, coords, RL, mutations=None, alone=None):
    """(counts, masks) of the pairs `coords` ([n, 4]: fs, rs, re, insert size) on the record `genome`.  counts: class -> [forward
    mates, reverse mates] (one_mate_only: pairs).  masks: class -> bool [n, 2] (one_mate_only: bool [n]), plus "count": the
    exceptions in every window.  The forward window is [fs, fs + RL), the reverse one [rs, re); forward lane groups start at
    fs + 8 s, reverse ones at re - 8 - 8 s (both cut to the window).  mutations: the oracle's rows of the same call."""
    g = _bytes(genome)
    L = len(g)
    exc = ~PLAIN[g]
    S = np.concatenate([[0], np.cumsum(exc)]).astype(np.int64)  # S[b] - S[a]: exceptions in [a, b)
    c = np.asarray(coords, dtype=np.int64)
    n = len(c)
    lo = np.stack([c[:, 0], c[:, 1]], axis=1)
    hi = np.stack([c[:, 0] + RL, c[:, 2]], axis=1)
    assert (lo >= 0).all() and (hi <= L).all() and (hi - lo == RL).all(), "a template cut by the record's ends"
    cnt = S[hi] - S[lo]
    e_pad = np.concatenate([exc, [False]])  # e_pad[L] and e_pad[-1]: no base, no exception
    m = collections.OrderedDict()
    m["none"] = cnt == 0
    m["lo_only"] = (cnt == 1) & e_pad[lo]
    m["hi_only"] = (cnt == 1) & e_pad[hi - 1]
    m["below"] = (cnt == 0) & e_pad[lo - 1]
    m["above"] = (cnt == 0) & e_pad[hi]
    m["all"] = cnt == RL
    up = np.zeros((n, 2), dtype=bool)
    for s in range((RL + 7) // 8):
        for o in range(2):
            a = np.maximum(lo[:, o], hi[:, o] - 8 - 8 * s) if o else lo[:, o] + 8 * s
            b = hi[:, o] - 8 * s if o else np.minimum(hi[:, o], lo[:, o] + 8 * s + 8)
            word = ((b - 1) >> 5) << 5  # first base of the mask word the group's last base lies in
            up[:, o] |= (a < word) & (S[b] - S[word] > 0) & (S[word] - S[a] == 0)
    m["group_upper_word"] = up
    # lo_alone, hi_alone: lo_only / hi_only, and that exception is the only one within `alone` bases of either window of the pair
    # (the widened windows may overlap: then their union is one interval)
    alone = ALONE if alone is None else alone
    wide_lo, wide_hi = np.maximum(lo - alone, 0), np.minimum(hi + alone, L)
    near = S[wide_hi] - S[wide_lo]
    overlap = np.minimum(wide_hi[:, 0], wide_hi[:, 1]) > np.maximum(wide_lo[:, 0], wide_lo[:, 1])
    union = S[np.maximum(wide_hi[:, 0], wide_hi[:, 1])] - S[np.minimum(wide_lo[:, 0], wide_lo[:, 1])]
    single = np.where(overlap, union, near.sum(axis=1)) == 1
    m["lo_alone"] = m["lo_only"] & single[:, None]
    m["hi_alone"] = m["hi_only"] & single[:, None]
    counts = collections.OrderedDict((k, [int(v[:, 0].sum()), int(v[:, 1].sum())]) for k, v in m.items())
    m["one_mate_only"] = (cnt[:, 0] > 0) != (cnt[:, 1] > 0)
    counts["one_mate_only"] = int(m["one_mate_only"].sum())
    m["count"] = cnt
    if mutations is not None:
        rows = mutations
        net = np.zeros((n, 2), dtype=np.int64)
        np.add.at(net, (rows["pair"][rows["type"] == 2], rows["mate"][rows["type"] == 2]), 1)
        np.add.at(net, (rows["pair"][rows["type"] == 1], rows["mate"][rows["type"] == 1]), -1)
        net = np.maximum(net, 0)
        pad_lo = np.stack([np.minimum(hi[:, 0], L), np.maximum(lo[:, 1] - net[:, 1], 0)], axis=1)
        pad_hi = np.stack([np.minimum(hi[:, 0] + net[:, 0], L), lo[:, 1]], axis=1)
        m["pad_takes_exception"] = S[pad_hi] - S[pad_lo] > 0
        sub = rows[(rows["type"] == 0) & (rows["ref"] >= 97)]
        low = np.zeros((n, 2), dtype=np.int64)
        np.add.at(low, (sub["pair"], sub["mate"]), 1)
        m["lower_substituted"] = low > 0
        counts["pad_takes_exception"] = [int(m["pad_takes_exception"][:, o].sum()) for o in range(2)]
        counts["lower_substituted"] = [int(low[:, o].sum()) for o in range(2)]
        touched = np.zeros((n, 2), dtype=bool)
        touched[rows["pair"], rows["mate"]] = True
        m["has_rows"] = touched
    return counts, m


def letters_met(genome, coords, RL):
    """The exception letters of the record that lie in a forward window, and in a reverse window, of the pairs `coords`: two
    sets of byte values (the reverse mate shows their complements)."""
    g = _bytes(genome)
    c = np.asarray(coords, dtype=np.int64)
    met = []
    for lo, hi in ((c[:, 0], c[:, 0] + RL), (c[:, 1], c[:, 2])):
        cover = np.zeros(len(g) + 1, dtype=np.int64)
        np.add.at(cover, lo, 1)
        np.add.at(cover, hi, -1)
        met.append(set(g[(np.cumsum(cover)[:-1] > 0) & ~PLAIN[g]].tolist()))
    return met


# ------------------------------------------------------------------ the models
@functools.lru_cache(maxsize=None)
def model(name):
    """The dense model of a case.  Never written to."""
    if name == "novaseq-indel":
        return dense_model("novaseq", (0.01, 0.03))
    if name == "novaseq-batch":
        return dense_model("novaseq", (0.001, 0.003))
    if name == "syn33":
        return synthetic_model(33, 9, 7, 3300, indel=(0.0, 0.0))
    if name == "hiseq-fires":  # every substitution test fires: u > 0 (the quality rows, and the position tiles, stay HiSeq's)
        d = dense_model("hiseq")
        d.phred_thr[:] = 0.0
        return d
    if name.startswith("perfect"):
        from insilicoseq_amd.model import DenseModel

        return DenseModel.perfect(int(name[7:]))
    if name.startswith("RL"):
        import mt_resolver_cases as M

        return M.model(M.case(name))
    return dense_model(name)


def oracle_of(name):
    from oracle import oracle as O

    d = model(name)
    if name.startswith("perfect"):  # (k_perfect's reference: quality mode 1 on the degenerate tables, as in test_gpu_perfect.py)
        return O.Oracle(d, quality_mode=1, basic_insert_size=d.basic_insert_size)
    return O.Oracle(d)


# ------------------------------------------------------------------ the cases
BOUNDARY = ("lo_only", "hi_only", "below", "above")
SINGLE = BOUNDARY + ("none", "one_mate_only")
NAMED_BY_RECORD = {"bit0": SINGLE + ("group_upper_word",), "bit31": SINGLE, "odd": SINGLE + ("group_upper_word",),
                   "runs": ("all", "none", "one_mate_only"), "soft": ("all", "none", "one_mate_only"),
                   "sparse0": SINGLE + ("lo_alone", "hi_alone"), "sparse31": SINGLE + ("lo_alone", "hi_alone")}
Case = collections.namedtuple("Case", "id model record pairs rng mutations named")


def _case(model_name, rec, pairs, rng="philox", mutations=False, extra=(), tag=""):
    cid = "%s-%s%s" % (model_name, rec, tag)
    return Case(cid, model_name, rec, pairs, rng, mutations, NAMED_BY_RECORD[rec] + tuple(extra))


PHILOX_PAIRS, MT_PAIRS, FIRES_PAIRS = 1 << 14, 1 << 15, 1 << 11
PLAIN_MODELS = ("novaseq", "miseq", "syn33")
PLAIN_RECORDS = ("bit0", "bit31", "odd", "runs", "soft")
ALONE_MODELS = ("novaseq", "perfect151")
MT_MODELS = ("RL159-NB4-noisy", "RL246-NB1-noisy")
CASES = tuple(
    [_case(mo, rec, PHILOX_PAIRS) for mo in PLAIN_MODELS for rec in PLAIN_RECORDS]
    # (2^14 pairs leave lo_alone / hi_alone of NovaSeq at 12 to 25 a mate)
    + [_case(mo, rec, 2 * PHILOX_PAIRS) for mo in ALONE_MODELS for rec in ("sparse0", "sparse31")]
    + [_case("novaseq", "odd", PHILOX_PAIRS, mutations=True, tag="-vcf"),
       _case("novaseq", "soft", PHILOX_PAIRS, mutations=True, extra=("lower_substituted",), tag="-vcf")]
    + [_case("novaseq-indel", "odd", PHILOX_PAIRS, mutations=True, extra=("pad_takes_exception",)),
       _case("novaseq-indel", "runs", PHILOX_PAIRS, mutations=True, extra=("pad_takes_exception",))]
    # (2^11 pairs reach the floor of `none` and `one_mate_only` only, and `all` on the runs: the legs of this model are about
    #  what is substituted, not about the window scans)
    + [Case("hiseq-fires-odd", "hiseq-fires", "odd", FIRES_PAIRS, "philox", False, ("none", "one_mate_only")),
       Case("hiseq-fires-runs", "hiseq-fires", "runs", FIRES_PAIRS, "philox", False, ("all", "none", "one_mate_only"))]
    + [_case("perfect%d" % RL, rec, PHILOX_PAIRS) for RL in (151, 33) for rec in ("bit0", "bit31", "runs")]
    + [_case(mo, rec, MT_PAIRS, rng="mt") for mo in MT_MODELS for rec in ("sparse0", "sparse31")]
)
assert len({c.id for c in CASES}) == len(CASES)


def case(cid):
    return next(c for c in CASES if c.id == cid)


def case_record(c):
    return record(c.record, model(c.model).read_length)


_oracles = {}


def _freeze(res):
    for k in ("r1_base", "r1_qual", "r2_base", "r2_qual", "coords"):
        res[k].setflags(write=False)
    return res


def oracle_rows(cid, mutations=None):
    """The oracle's reads of case `cid` -- Philox: seed SEED from ordinal FIRST_ORDINAL; MT: seed MT_SEED, and the next four
    doubles of both of the oracle's streams behind the sample as "next_words" (what the device's streams must show) -- with
    coordinates and, where the case has them (or `mutations` asks), mutation rows.  Computed once, never written to."""
    c = case(cid)
    mutations = c.mutations if mutations is None else mutations
    if (cid, mutations) not in _oracles:
        from oracle import oracle as O

        rng = O.Rng().seed_mt(MT_SEED) if c.rng == "mt" else O.Rng().seed_philox(SEED)
        res = oracle_of(c.model).simulate(rng, case_record(c), c.pairs, first_ordinal=FIRST_ORDINAL, want_coords=True,
                                         store_mutations=mutations)
        assert res["status"] == 0 and res["n_done"] == c.pairs
        if c.rng == "mt":
            res["next_words"] = ([rng.py_random() for _ in range(4)], [rng.np_random() for _ in range(4)])
        _oracles[cid, mutations] = _freeze(res)
    return _oracles[cid, mutations]


def case_ledger(cid, mutations=None):
    c = case(cid)
    res = oracle_rows(cid, mutations)
    return ledger(case_record(c), res["coords"], model(c.model).read_length, res.get("mutations"))


# ---- the batches: one oracle run per item, ordinals running on
ENDS_MODELS = ("novaseq", "perfect151", "perfect33")
ENDS_NAMED = {0: ("lo_only", "hi_only", "above"), 1: ("lo_only", "hi_only", "below")}  # (fs = 0: nothing below; re = L: nothing above)
BATCH_COUNTS = (5003, 6011, PHILOX_PAIRS - 5003 - 6011)  # plain, bit31, plain: the seams inside a wavefront's 16 pairs


def batch_records(RL):
    return (record("plain", RL), record("bit31", RL), record("plain", RL)[::-1])


def _batch(key, name, recs, counts, sequence_type, mutations=False):
    if key not in _oracles:
        from oracle import oracle as O

        orc, rng, out, ordinal = oracle_of(name), O.Rng().seed_philox(SEED), [], FIRST_ORDINAL
        for seq, n in zip(recs, counts):
            res = orc.simulate(rng, seq, n, first_ordinal=ordinal, sequence_type=sequence_type, want_coords=True, store_mutations=mutations)
            assert res["status"] == 0 and res["n_done"] == n
            out.append(_freeze(res))
            ordinal += n
        _oracles[key] = out
    return _oracles[key]


def ends_oracle(name):
    """The oracle's reads of every item of the `ends` batch under model `name`, amplicon mode."""
    recs, counts, _ = ends(model(name).read_length)
    return _batch(("ends", name), name, recs, counts, "amplicon")


def ends_ledger(name):
    """The ledger's counts summed over the items of the `ends` batch."""
    RL = model(name).read_length
    recs, _, _ = ends(RL)
    total = collections.Counter()
    for seq, res in zip(recs, ends_oracle(name)):
        counts, _ = ledger(seq, res["coords"], RL)
        for k in MATE_CLASSES:
            total[k, 0] += counts[k][0]
            total[k, 1] += counts[k][1]
    return total


def batch_oracle():
    """The oracle's reads of the metagenomics batch (plain, bit31, plain) under NovaSeq with indel rates (0.001, 0.003)."""
    return _batch(("batch",), "novaseq-batch", batch_records(151), BATCH_COUNTS, "metagenomics")


WORKER_MODEL, WORKER_RECORD = MT_MODELS[0], "sparse31"
WORKER_PAIRS = (11000, 10922, 10846)  # 2^15 pairs over the three workers
assert sum(WORKER_PAIRS) == MT_PAIRS and len(WORKER_PAIRS) == len(WORKER_SEEDS)


def worker_oracle(w):
    """Worker w of the worker-set case: WORKER_MODEL on WORKER_RECORD, WORKER_PAIRS[w] pairs from WORKER_SEEDS[w]."""
    key = ("worker", w)
    if key not in _oracles:
        from oracle import oracle as O

        rng = O.Rng().seed_mt(WORKER_SEEDS[w])
        res = oracle_of(WORKER_MODEL).simulate(rng, record(WORKER_RECORD, model(WORKER_MODEL).read_length), WORKER_PAIRS[w], want_coords=True)
        assert res["status"] == 0 and res["n_done"] == WORKER_PAIRS[w]
        res["next_words"] = ([rng.py_random() for _ in range(4)], [rng.np_random() for _ in range(4)])
        _oracles[key] = _freeze(res)
    return _oracles[key]
