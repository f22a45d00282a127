"""The cases and expectations of the readers of a noisy generate call at scale (no GPU; DESIGN section 4, "What holds the readers
of a call at scale"; tests/test_outputs_at_scale_host.py, tests/test_gpu_outputs_at_scale.py).

A case is one call: a model and records of tests/philox_indel_stats.case_model, seed 2024, 2^14 pairs (2^13 on the sequential MT
path) -- the smallest power of two at which a wavefront of k_indel_fixup records read after read.  ``expected(case)`` runs the
oracle ONCE for the call (once per item of the batch, the ordinals running on) and keeps its arrays; every builder below makes one
reader's expected output from those arrays alone, with the plain host code the project has for that reader.  Nothing here
takes anything a device produced.

``LEDGER`` pins what a case contains -- rows by type, the most rows of a pair and of a read, the reads with an indel row, the
VCF text's size and SHA-256, its BGZF members, one mate's FASTQ size -- so that a change of a case cannot pass unseen; the host
file asserts it, the GPU file asserts that the readers saw it."""
import collections
import hashlib

import numpy as np

import philox_indel_stats as IS
import philox_setup_stats as SS
from helpers import fastq_text, mixed_genome, random_genome, vcf_lines

SEED = 2024
MT_SEED = 77
N_PAIRS = 1 << 14
CPU = 3  # the worker number of every text
BGZF_BLOCK = 32768  # text bytes of a member (insilicoseq_amd.bgzf.BLOCK, asserted by the host file)
DEPTH_BIN = 1000
# cuts of the error tally's three windows: no multiple of 64, the first one odd
WINDOW_CUTS = (5001, 11003)
# batch: pairs of the three items -- multiples of neither 16 nor 64, so both seams fall inside a wavefront's 16 pairs and inside an
# export tile -- and the short record's length: about one fragment (2 x 301 + the median insert size of 154 is 756), where three
# pairs in ten do not fit and fall back
BATCH_PAIRS = (9003, 1382, 5999)
BATCH_SHORT = 800
BATCH_LONG = 120_000
BATCH_FIRST_ORDINAL = 5
BATCH_IDS = ("plain.0", "short.1", "mixed.2")
BATCH_FIRST_I = (0, 99990, 7)  # (the short item's pair numbers pass from five digits to six)

Case = collections.namedtuple("Case", "kind model n_pairs first_ordinal readers")
ALL_READERS = tuple(range(1, 11))
CASES = collections.OrderedDict((
    ("fixup", Case("generate", "patterned", N_PAIRS, 11, ALL_READERS)),
    ("scripted", Case("generate", "patterned-plain", N_PAIRS, 0, ALL_READERS)),
    ("batch", Case("batch", "patterned", N_PAIRS, BATCH_FIRST_ORDINAL, (1, 2, 3, 6, 7, 8, 9))),
    ("mt", Case("mt", "flat", N_PAIRS // 2, 0, (1, 2, 4, 5, 8))),
))


def cases_with(reader):
    return [name for name, c in CASES.items() if reader in c.readers]


class Call(object):
    """A case's inputs and the oracle's arrays for it: ``dense``, ``records`` [(id, sequence)], ``items`` [(record id, first pair
    number, first output row, pairs)] and ``record_of`` (the record of every item), ``bases`` / ``qual`` uint8 [n, 2, RL],
    ``coords`` int64 [n, 4], ``item`` int32 [n] and ``rows`` (iss_mutation, ``pair`` counted from the call's first pair)."""

    def __init__(self, name):
        from oracle import oracle as O

        c = self.case = CASES[name]
        self.name, self.n = name, c.n_pairs
        self.dense, genome, _ = IS.case_model(c.model)
        self.RL = self.dense.read_length
        if c.kind == "batch":
            seqs = (random_genome(96, BATCH_LONG), random_genome(97, BATCH_SHORT), mixed_genome(98, BATCH_LONG))
            self.records = list(zip(BATCH_IDS, seqs))
            counts, first_i = BATCH_PAIRS, BATCH_FIRST_I
        else:
            self.records = [("rec.1", genome)]
            counts, first_i = (c.n_pairs,), (0,)
        assert sum(counts) == self.n
        self.record_of = list(range(len(counts)))
        first_row = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.items = [(self.records[k][0], first_i[k], int(first_row[k]), int(counts[k])) for k in range(len(counts))]
        self.lengths = [len(self.records[k][1]) for k in self.record_of]
        orc = O.Oracle(self.dense)
        rng = O.Rng().seed_mt(MT_SEED) if c.kind == "mt" else O.Rng().seed_philox(SEED)
        parts, ordinal = [], c.first_ordinal
        for k, (_rid, _i, row, n) in enumerate(self.items):
            res = orc.simulate(rng, self.records[self.record_of[k]][1], n, first_ordinal=ordinal, store_mutations=True, want_coords=True)
            assert res["status"] == 0 and res["n_done"] == n, (name, k, res["status"], res["n_done"])
            ordinal += n
            rows = res["mutations"].copy()
            rows["pair"] += row
            parts.append((res, rows))
        RL = self.RL
        self.bases = np.concatenate([np.stack([r["r1_base"][:, :RL], r["r2_base"][:, :RL]], axis=1) for r, _ in parts])
        self.qual = np.concatenate([np.stack([r["r1_qual"][:, :RL], r["r2_qual"][:, :RL]], axis=1) for r, _ in parts])
        self.coords = np.concatenate([r["coords"] for r, _ in parts])
        self.rows = np.concatenate([rows for _, rows in parts])
        self.item = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
        for a in (self.bases, self.qual, self.coords, self.rows, self.item):
            a.setflags(write=False)  # shared by the tests of a case, left unchanged

    def rows_of_item(self, k):
        _rid, _i, row, n = self.items[k]
        return IS.rows_of(self.rows, row, n)


_CALLS = {}


def expected(name):
    """The Call of a case, made once per process."""
    if name not in _CALLS:
        _CALLS[name] = Call(name)
    return _CALLS[name]


# ------------------------------------------------------------------ the expectation builders, one per reader
def vcf_text(call, cpu=CPU):
    """Reader 2: helpers.vcf_lines over the oracle's rows, item after item."""
    return "".join("".join(vcf_lines(rid, first_i, cpu, call.rows_of_item(k))) for k, (rid, first_i, _row, _n) in enumerate(call.items)).encode()


def truth_and_events(call, first, n, encoding):
    """Reader 3: the derivation of tests/test_gpu_truth.py::test_truth_and_events_equal_the_oracle, taken from there."""
    from test_gpu_truth import _expected

    return _expected(call.bases, call.rows, first, n, encoding)


def error_tally(call, first, n):
    """Reader 4."""
    from insilicoseq_amd import errtally

    return errtally.errors_host(call.rows, first, n, call.RL)


def read_tally(call):
    """Reader 5."""
    from insilicoseq_amd.tally import tally_host

    return tally_host(call.bases, call.qual, call.coords[:, 3], call.RL)


def depth(call, bin=DEPTH_BIN):
    """Reader 6: (record table of the items, words, difference array, depth, statistics, window sums)."""
    from insilicoseq_amd import depth as D

    table, n_words = D.depth_table(call.lengths)
    diff = D.mark_host(np.zeros(n_words, dtype=np.int32), call.coords, call.item, table, call.RL)
    return (table, n_words, diff) + D.finish_host(diff, table, bin)


def origins_text(call, cpu=CPU):
    """Reader 7."""
    from insilicoseq_amd import origins

    return origins.lines_host(call.items, call.lengths, cpu, call.coords, call.RL)


def fastq_texts(call, cpu=CPU):
    """Reader 8: the two files' text."""
    return [b"".join(fastq_text(rid, first_i, cpu, mate, call.bases[row:row + n, mate - 1], call.qual[row:row + n, mate - 1])
                     for rid, first_i, row, n in call.items) for mate in (1, 2)]


def ubam_records(call, cpu=CPU):
    """Reader 9: the record bytes."""
    import ubam_twin

    return ubam_twin.records(call.items, cpu, call.bases[:, 0], call.qual[:, 0], call.bases[:, 1], call.qual[:, 1])


def bgzf_inflate(raw):
    """BGZF bytes a device appended -> every member's data: every member carries ``BC``, the chain ends at the end, every member
    inflates ALONE with its CRC-32 and ISIZE (insilicoseq_amd.bgzf.members_of raises otherwise)."""
    from insilicoseq_amd import bgzf

    return [m[2] for m in bgzf.members_of(raw)]


def bgzf_members(raw, text):
    """The same, and together the members inflate to ``text``.  Returns the number of members."""
    data = bgzf_inflate(raw)
    got = b"".join(data)
    assert got == text, first_difference(got, text)
    return len(data)


def windows(call):
    """The error tally's three windows [(first pair, pairs)]: the cuts are no multiple of 64 (halved on the half-sized MT case)."""
    cuts = WINDOW_CUTS if call.n >= N_PAIRS else tuple(c // 2 for c in WINDOW_CUTS)
    assert all(0 < c < call.n and c % 64 for c in cuts)
    edges = (0,) + cuts + (call.n,)
    return [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d bytes against %d, first difference at byte %d: %r against %r" % (len(got), len(want), k, got[k:k + 40], want[k:k + 40])


# ------------------------------------------------------------------ the ledger
def ledger(call):
    """What the case contains, from the oracle's arrays."""
    rows = call.rows
    read = rows["pair"].astype(np.int64) * 2 + rows["mate"]
    text = vcf_text(call)
    return collections.OrderedDict((
        ("rows", len(rows)),
        ("by type", tuple(int((rows["type"] == t).sum()) for t in range(3))),
        ("most rows of a pair", int(np.bincount(rows["pair"], minlength=call.n).max())),
        ("most rows of a read", int(np.bincount(read, minlength=2 * call.n).max())),
        ("reads with an indel row", int(np.unique(read[rows["type"] != 0]).size)),
        ("vcf bytes", len(text)),
        ("vcf members", -(-len(text) // BGZF_BLOCK)),
        ("vcf sha256", hashlib.sha256(text).hexdigest()),
        ("fastq bytes of mate 1", len(fastq_texts(call)[0])),
    ))


def short_item(call):
    """The batch's fragment-long record: the shares of its pairs whose start fell back (the fragment does not fit: the start is
    drawn from [0, L - RL)) and whose reverse read was cut by the record's end (the natural end lies behind it: the end is drawn
    anew), by philox_setup_stats.pair_rule (which holds every pair to the reference's rule on the way), and the reads with an
    indel row whose template window (8 positions beyond the read, iss_kernels.hip.h: ap_win) leaves the record."""
    _rid, _i, row, n = call.items[1]
    c, L, RL = call.coords[row:row + n], call.lengths[1], call.RL
    rule = SS.pair_rule(c, L, RL)
    rows = call.rows_of_item(1)
    has = np.zeros((n, 2), dtype=bool)
    ind = rows[rows["type"] != 0]
    has[ind["pair"], ind["mate"]] = True
    leaves = np.stack([c[:, 0] + RL + 8 > L, c[:, 1] - 8 < 0], axis=1)
    return {"fell back": float((~rule.regular).mean()), "cut by the end": float(rule.fell.mean()), "windows that leave": int((has & leaves).sum())}


def _entry(rows, by_type, pair, read, indel_reads, vcf_bytes, members, sha, fastq):
    return collections.OrderedDict((("rows", rows), ("by type", by_type), ("most rows of a pair", pair), ("most rows of a read", read),
                                    ("reads with an indel row", indel_reads), ("vcf bytes", vcf_bytes), ("vcf members", members),
                                    ("vcf sha256", sha), ("fastq bytes of mate 1", fastq)))


# as the oracle gives them (found on the CPU).  fixup: 82.5 % of the 32 768 reads carry an indel row.
LEDGER = {
    "fixup": _entry(141009, (84635, 45607, 10767), 26, 23, 27029, 4196128, 129,
                    "70d0c692a50b513a1f99df7726bff3ae5165649b3b42c576c3384837744cfc02", 10196122),
    "scripted": _entry(148982, (87859, 49536, 11587), 29, 23, 27779, 4433362, 136,
                       "c108d673dc03daad143f08c3ce856dfe83b3a240a27a1dbc9e7414726c7337cf", 10196122),
    "batch": _entry(146287, (86683, 48078, 11526), 29, 23, 27570, 4604022, 141,
                    "4aee2f902ab3f41d1b91af7d2d91a4d07ed8f46aa6c54a92ba29ca9e81c9af93", 10224171),
    "mt": _entry(20882, (3748, 9768, 7366), 12, 9, 10630, 601580, 19,
                 "2996f703555380727cd827003198e75c73a1fc0a9d7611e1562e107a27bbe858", 2636714),
}
# The same model, record and seed from ordinal 0 -- the call of test_the_rows_are_the_oracles_when_a_wavefront_records_many_reads,
# whose figures the case was sized by: rows, rows by type, VCF bytes under id rec.1, first pair number 0, worker 3.
FIXUP_FROM_ORDINAL_0 = (140992, (84614, 45607, 10771), 4195639)
