"""The three work loops -- Worker.simulate_reads, _simulate_work_batched, worker_set_iterator -- as the sequence of engine
calls they make and the VCF text they write, with a recording stand-in for ReadEngine (no GPU): which genomes are uploaded
(alone, in groups), when they are dropped, what every generate call is given, and which way the --store_mutations rows go."""
import numpy as np
import pytest

from insilicoseq_amd import _native
from insilicoseq_amd import generator as G
from insilicoseq_amd.engine import MUT_DTYPE
from insilicoseq_amd.model import BasicErrorModel

BIG = (1 << 20) + 5  # letters of a record above SMALL_RECORD


class RecordingEngine(object):
    """Every call of the work loops that reaches the device, in order, in ONE list (the loops make their engine themselves)."""

    trace = []
    arena_ok = True   # False: generate_batch refuses (records too long for one arena)
    overflow = set()  # "vcf" / "rows": the next vcf_emit / mutations overflows its row buffer, once

    def __init__(self, device=0):
        self.lengths, self.last, self.mutations_capacity, self.pitch = [], [], 0, 128

    def _log(self, *call):
        RecordingEngine.trace.append(call)

    def load_model(self, dense):
        self.read_length = dense.read_length

    def seed_mt(self, seed):
        pass

    def seed_mt_workers(self, seeds):
        pass

    def set_fragment(self, *a):
        pass

    mt_set_fragment = set_fragment

    def add_genome(self, seq):
        self._log("add", len(seq))
        if "!" in seq:
            raise _native.EngineError(_native.E_INVALID, "letter outside the alphabet")
        self.lengths.append(len(seq))
        return len(self.lengths) - 1

    def add_genomes(self, seqs):
        self._log("group", [len(s) for s in seqs])
        gids = []
        for s in seqs:
            gids.append(-1 if "!" in s else len(self.lengths))
            if gids[-1] >= 0:
                self.lengths.append(len(s))
        return gids

    def clear_genomes(self):
        self._log("clear")
        self.lengths = []

    def reserve(self, n):
        self._log("reserve", n)

    def generate(self, gid, n, first_ordinal, seed, sequence_type, gc_bias, out_first_pair):
        self._log("gen", gid, n, first_ordinal, out_first_pair)
        self.last = [(0, n)]  # (rows are numbered from the call's first pair)

    def generate_batch(self, gids, counts, first_ordinal, seed, sequence_type, gc_bias, out_first_pair):
        self._log("batch", list(gids), list(counts), first_ordinal)
        if not self.arena_ok:
            raise _native.EngineError(_native.E_INVALID, "iss_generate_batch: the records of one call must stay below 2^34 - 4096 bases")
        starts = np.cumsum([0] + list(counts))
        self.last = [(int(s), n) for s, n in zip(starts, counts)]

    def generate_mt(self, gid, n, sequence_type="metagenomics", gc_bias=False, out_first_pair=0):
        self._log("mt", gid, n)
        if not self.read_length < self.lengths[gid]:
            raise _native.EngineError(_native.E_SHORT_RECORD, "short record")
        self.last = [(0, n)]
        return n

    def generate_mt_workers(self, g, n, row, sequence_type="metagenomics", gc_bias=False):
        self._log("mt_workers", [int(x) for x in g], [int(x) for x in n], [int(x) for x in row])
        short = np.array([k > 0 and not self.read_length < self.lengths[gid] for gid, k in zip(g, n)])
        return np.where(short, 0, n).astype(np.int64), np.where(short, _native.E_SHORT_RECORD, 0).astype(np.int32)

    def _overflows(self, what):
        if what in RecordingEngine.overflow:
            RecordingEngine.overflow.discard(what)
            self.mutation_slots_needed = 1 << 20
            raise _native.EngineError(_native.E_NOMEM, "mutation rows overflow")

    def _rows(self):
        """Two substitutions per item of the last call: on its first pair and on its last."""
        rows = np.zeros(2 * len(self.last), dtype=MUT_DTYPE)
        rows["pair"] = [p for row, n in self.last for p in (row, row + n - 1)]
        rows["ref"], rows["alt"] = ord("A"), ord("C")
        return rows

    def mutations_reserve(self, cap):
        self._log("mutations_reserve", cap)
        self.mutations_capacity = cap

    mt_mutations_reserve = mutations_reserve

    def mutations(self):
        self._log("rows")
        self._overflows("rows")
        return self._rows()

    def mt_mutations(self):
        self._log("mt_rows")
        return self._rows()

    def vcf_emit(self, fd, items, cpu, source="philox"):
        self._log("vcf", list(items), cpu, source)
        self._overflows("vcf")

    def fastq_emit(self, fd1, fd2, rid, first_i, cpu, first_pair, n_pairs, n_threads=1):
        self._log("emit", rid, first_i, cpu, first_pair, n_pairs)

    def fastq_emit_batch(self, fd1, fd2, items, cpu):
        self._log("emit_batch", list(items), cpu)

    def fastq_emit_scatter(self, fd1, fd2, items, n_threads=1):
        self._log("scatter", list(items))

    def fastq_compress(self, on=True):
        pass

    def fastq_flush(self):
        self._log("flush")

    def vcf_flush(self):
        self._log("vcf_flush")

    def close(self):
        pass


@pytest.fixture
def rec(monkeypatch):
    for name in ("ISS_HOST_FASTQ", "ISS_HOST_VCF", "ISS_ITEMWISE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(G, "ReadEngine", RecordingEngine)
    monkeypatch.setattr(RecordingEngine, "trace", [])
    monkeypatch.setattr(RecordingEngine, "arena_ok", True)
    monkeypatch.setattr(RecordingEngine, "overflow", set())
    monkeypatch.setattr(G.Worker, "BATCH_PAIRS", 32)
    monkeypatch.setattr(G.Worker, "GROUP_BASES", 750)
    return monkeypatch


def _records():
    """s1, s2, s3: small records; short: not longer than the basic model's reads (125); big: above SMALL_RECORD."""
    return {"s1": G.Record("A" * 300, id="s1"), "s2": G.Record("C" * 400, id="s2"), "s3": G.Record("G" * 500, id="s3"),
            "short": G.Record("T" * 100, id="short"), "big": G.Record("A" * BIG, id="big")}


def _work(spec, records=None):
    records = records or _records()
    return [(records[name], n, "default") for name, n in spec]


def _worker(tmp_path, spec, rng, store=False):
    """worker_iterator as worker 3 with seed 5 -> (the engine calls, the ids of the .vcf file's lines)"""
    prefix = str(tmp_path / "w")
    G.worker_iterator(_work(spec), BasicErrorModel(None, None, store), 3, prefix, 5, "metagenomics", False, device=0, rng=rng)
    trace = list(RecordingEngine.trace)
    if store:  # (the first call sizes the row buffer from the model: not part of the loops)
        assert trace[0][0] == "mutations_reserve"
        del trace[0]
    return trace, [line.split("\t")[0] for line in open(prefix + ".vcf").read().splitlines()]


# s1 comes back after other records; short and big stand between small ones
MIXED = [("s1", 10), ("s2", 20), ("short", 5), ("big", 7), ("s3", 30), ("s1", 4)]


def test_philox_worker_groups_small_records_and_never_uploads_a_short_one(rec, tmp_path):
    """GROUP_BASES = 750: s1 + s2 are one group, s3 (with nothing left to join it: s1 is resident) the next, at its first
    use; big is uploaded alone; short is skipped before any upload; batches of 32 pairs are cut across the items."""
    trace, _vcf = _worker(tmp_path, MIXED, "philox")
    assert trace == [
        ("group", [300, 400]),
        ("add", BIG),
        ("batch", [0, 1, 2], [10, 20, 2], 0),
        ("emit_batch", [("s1", 0, 0, 10), ("s2", 0, 10, 20), ("big", 0, 30, 2)], 3),
        ("group", [500]),
        ("batch", [2, 3], [5, 27], 32),
        ("emit_batch", [("big", 2, 0, 5), ("s3", 0, 5, 27)], 3),
        ("batch", [3, 0], [3, 4], 64),
        ("emit_batch", [("s3", 27, 0, 3), ("s1", 0, 3, 4)], 3),
        ("flush",),
    ]


def test_mt_worker_uploads_the_short_record_and_consumes_one_draw(rec, tmp_path):
    """The MT worker needs the short record on the device (the engine consumes the reference's insert-size draw): it is part
    of the groups -- s1 + s2 (short would pass GROUP_BASES), then short + s3 at short's turn -- and one pair is asked of it."""
    trace, _vcf = _worker(tmp_path, MIXED, "mt")
    assert trace == [
        ("group", [300, 400]),
        ("mt", 0, 10), ("emit", "s1", 0, 3, 0, 10),
        ("mt", 1, 20), ("emit", "s2", 0, 3, 0, 20),
        ("group", [100, 500]),
        ("mt", 2, 1),
        ("add", BIG),
        ("mt", 4, 7), ("emit", "big", 0, 3, 0, 7),
        ("mt", 3, 30), ("emit", "s3", 0, 3, 0, 30),
        ("mt", 0, 4), ("emit", "s1", 0, 3, 0, 4),
        ("flush",),
    ]


def test_mt_worker_cuts_an_item_into_batches(rec, tmp_path):
    trace, _vcf = _worker(tmp_path, [("s1", 70)], "mt")
    assert trace == [
        ("group", [300]),
        ("mt", 0, 32), ("emit", "s1", 0, 3, 0, 32),
        ("mt", 0, 32), ("emit", "s1", 32, 3, 0, 32),
        ("mt", 0, 6), ("emit", "s1", 64, 3, 0, 6),
        ("flush",),
    ]


def test_short_record_without_pairs_draws_nothing(rec, tmp_path):
    trace, _vcf = _worker(tmp_path, [("short", 0), ("s1", 2)], "mt")
    assert trace == [("group", [300]), ("mt", 0, 2), ("emit", "s1", 0, 3, 0, 2), ("flush",)]


OVER_BUDGET = [("s1", 10), ("s2", 20), ("s3", 30), ("s1", 4)]


def test_philox_worker_over_budget_runs_the_pending_items_then_drops(rec, tmp_path):
    """GENOME_BUDGET = 1000: the first group stops before s3; at s3 the pending pairs of s1 and s2 are generated, then every
    genome is dropped and the worker groups again from s3 on (s1, no longer resident, joins it)."""
    rec.setattr(G.Worker, "GENOME_BUDGET", 1000)
    rec.setattr(G.Worker, "GROUP_BASES", 1000)
    rec.setattr(G.Worker, "BATCH_PAIRS", 64)
    trace, _vcf = _worker(tmp_path, OVER_BUDGET, "philox")
    assert trace == [
        ("group", [300, 400]),
        ("batch", [0, 1], [10, 20], 0),
        ("emit_batch", [("s1", 0, 0, 10), ("s2", 0, 10, 20)], 3),
        ("clear",),
        ("group", [500, 300]),
        ("batch", [0, 1], [30, 4], 30),
        ("emit_batch", [("s3", 0, 0, 30), ("s1", 0, 30, 4)], 3),
        ("flush",),
    ]


def test_mt_worker_over_budget_drops_just_before_the_upload(rec, tmp_path):
    rec.setattr(G.Worker, "GENOME_BUDGET", 1000)
    rec.setattr(G.Worker, "GROUP_BASES", 1000)
    trace, _vcf = _worker(tmp_path, OVER_BUDGET, "mt")
    assert trace == [
        ("group", [300, 400]),
        ("mt", 0, 10), ("emit", "s1", 0, 3, 0, 10),
        ("mt", 1, 20), ("emit", "s2", 0, 3, 0, 20),
        ("clear",),
        ("group", [500, 300]),
        ("mt", 0, 30), ("emit", "s3", 0, 3, 0, 30),
        ("mt", 1, 4), ("emit", "s1", 0, 3, 0, 4),
        ("flush",),
    ]


def test_worker_uploads_alone_the_record_its_group_did_not_take(rec, tmp_path):
    """A record with a letter outside the alphabet gets no id from its group: the single upload raises the error."""
    records = _records()
    records["bad"] = G.Record("AC!T" * 50, id="bad")
    work = _work([("s1", 3), ("bad", 2)], records)
    with pytest.raises(_native.EngineError, match="outside the alphabet"):
        G.worker_iterator(work, BasicErrorModel(), 3, str(tmp_path / "w"), 5, "metagenomics", False, device=0)
    assert RecordingEngine.trace == [("group", [300, 200]), ("add", 200)]


# ---------------------------------------------------------------------------------------------------- --store_mutations
STORE = [("s1", 40), ("s2", 25)]  # batches of 32: (s1: 32), (s1: 8, s2: 24), (s2: 1)
STORE_VCF_IDS = ["s1_0_3/1", "s1_31_3/1", "s1_32_3/1", "s1_39_3/1", "s2_0_3/1", "s2_23_3/1", "s2_24_3/1", "s2_24_3/1"]


def test_philox_store_mutations_device_route(rec, tmp_path):
    trace, vcf = _worker(tmp_path, STORE, "philox", store=True)
    assert trace == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("vcf", [("s1", 0, 0, 32)], 3, "philox"), ("emit_batch", [("s1", 0, 0, 32)], 3),
        ("batch", [0, 1], [8, 24], 32), ("vcf", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3, "philox"),
        ("emit_batch", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3),
        ("batch", [1], [1], 64), ("vcf", [("s2", 24, 0, 1)], 3, "philox"), ("emit_batch", [("s2", 24, 0, 1)], 3),
        ("flush",), ("vcf_flush",),
    ]
    assert vcf == []


def test_philox_store_mutations_host_route_splits_the_rows_per_item(rec, tmp_path):
    rec.setenv("ISS_HOST_VCF", "1")
    trace, vcf = _worker(tmp_path, STORE, "philox", store=True)
    assert trace == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("rows",), ("emit_batch", [("s1", 0, 0, 32)], 3),
        ("batch", [0, 1], [8, 24], 32), ("rows",), ("emit_batch", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3),
        ("batch", [1], [1], 64), ("rows",), ("emit_batch", [("s2", 24, 0, 1)], 3),
        ("flush",),
    ]
    assert vcf == STORE_VCF_IDS


def test_philox_store_mutations_device_route_overflow_repeats_the_call_once(rec, tmp_path):
    rec.setattr(RecordingEngine, "overflow", {"vcf"})
    trace, _vcf = _worker(tmp_path, STORE, "philox", store=True)
    need = 1 << 20
    assert trace[:7] == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("vcf", [("s1", 0, 0, 32)], 3, "philox"),
        ("mutations_reserve", need + need // 8 + (1 << 16)),
        ("batch", [0], [32], 0), ("vcf", [("s1", 0, 0, 32)], 3, "philox"), ("emit_batch", [("s1", 0, 0, 32)], 3),
    ]
    assert [c[0] for c in trace[7:]] == ["batch", "vcf", "emit_batch", "batch", "vcf", "emit_batch", "flush", "vcf_flush"]


def test_philox_store_mutations_host_route_overflow_repeats_the_call_once(rec, tmp_path):
    rec.setenv("ISS_HOST_VCF", "1")
    rec.setattr(RecordingEngine, "overflow", {"rows"})
    trace, vcf = _worker(tmp_path, STORE, "philox", store=True)
    need = 1 << 20
    assert trace[:7] == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("rows",),
        ("mutations_reserve", need + need // 8 + (1 << 16)),
        ("batch", [0], [32], 0), ("rows",), ("emit_batch", [("s1", 0, 0, 32)], 3),
    ]
    assert [c[0] for c in trace[7:]] == ["batch", "rows", "emit_batch", "batch", "rows", "emit_batch", "flush"]
    assert vcf == STORE_VCF_IDS


def test_arena_fallback_device_route_is_one_call_and_one_emit_per_item(rec, tmp_path):
    rec.setattr(RecordingEngine, "arena_ok", False)
    trace, vcf = _worker(tmp_path, STORE, "philox", store=True)
    assert trace == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("reserve", 32),
        ("gen", 0, 32, 0, 0), ("vcf", [("s1", 0, 0, 32)], 3, "philox"), ("emit_batch", [("s1", 0, 0, 32)], 3),
        ("batch", [0, 1], [8, 24], 32), ("reserve", 32),
        ("gen", 0, 8, 32, 0), ("vcf", [("s1", 32, 0, 8)], 3, "philox"),
        ("gen", 1, 24, 40, 8), ("vcf", [("s2", 0, 8, 24)], 3, "philox"),
        ("emit_batch", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3),
        ("batch", [1], [1], 64), ("reserve", 1),
        ("gen", 1, 1, 64, 0), ("vcf", [("s2", 24, 0, 1)], 3, "philox"), ("emit_batch", [("s2", 24, 0, 1)], 3),
        ("flush",), ("vcf_flush",),
    ]
    assert vcf == []


def test_arena_fallback_host_route_writes_the_rows_of_every_item(rec, tmp_path):
    rec.setenv("ISS_HOST_VCF", "1")
    rec.setattr(RecordingEngine, "arena_ok", False)
    rec.setattr(RecordingEngine, "overflow", {"rows"})
    trace, vcf = _worker(tmp_path, STORE, "philox", store=True)
    need = 1 << 20
    assert trace == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("reserve", 32),
        ("gen", 0, 32, 0, 0), ("rows",), ("mutations_reserve", need + need // 8 + (1 << 16)), ("gen", 0, 32, 0, 0), ("rows",),
        ("emit_batch", [("s1", 0, 0, 32)], 3),
        ("batch", [0, 1], [8, 24], 32), ("reserve", 32),
        ("gen", 0, 8, 32, 0), ("rows",), ("gen", 1, 24, 40, 8), ("rows",),
        ("emit_batch", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3),
        ("batch", [1], [1], 64), ("reserve", 1),
        ("gen", 1, 1, 64, 0), ("rows",), ("emit_batch", [("s2", 24, 0, 1)], 3),
        ("flush",),
    ]
    assert vcf == STORE_VCF_IDS


def test_itemwise_philox_store_mutations_both_routes(rec, tmp_path):
    """ISS_ITEMWISE=1: the Philox worker through Worker.simulate_reads, one call per batch of one item."""
    rec.setenv("ISS_ITEMWISE", "1")
    rec.setattr(RecordingEngine, "overflow", {"vcf"})
    trace, vcf = _worker(tmp_path, [("s1", 40)], "philox", store=True)
    need = 1 << 20
    assert trace == [
        ("group", [300]),
        ("gen", 0, 32, 0, 0), ("vcf", [("s1", 0, 0, 32)], 3, "philox"), ("mutations_reserve", need + need // 8 + (1 << 16)),
        ("gen", 0, 32, 0, 0), ("vcf", [("s1", 0, 0, 32)], 3, "philox"), ("emit", "s1", 0, 3, 0, 32),
        ("gen", 0, 8, 32, 0), ("vcf", [("s1", 32, 0, 8)], 3, "philox"), ("emit", "s1", 32, 3, 0, 8),
        ("flush",), ("vcf_flush",),
    ]
    assert vcf == []
    rec.setenv("ISS_HOST_VCF", "1")
    rec.setattr(RecordingEngine, "trace", [])
    trace, vcf = _worker(tmp_path, [("s1", 40)], "philox", store=True)
    assert trace == [
        ("group", [300]),
        ("gen", 0, 32, 0, 0), ("rows",), ("emit", "s1", 0, 3, 0, 32),
        ("gen", 0, 8, 32, 0), ("rows",), ("emit", "s1", 32, 3, 0, 8),
        ("flush",),
    ]
    assert vcf == ["s1_0_3/1", "s1_31_3/1", "s1_32_3/1", "s1_39_3/1"]


def test_mt_store_mutations_both_routes(rec, tmp_path):
    trace, vcf = _worker(tmp_path, [("s1", 40), ("short", 2)], "mt", store=True)
    assert trace == [
        ("group", [300, 100]),
        ("mt", 0, 32), ("vcf", [("s1", 0, 0, 32)], 3, "mt"), ("emit", "s1", 0, 3, 0, 32),
        ("mt", 0, 8), ("vcf", [("s1", 32, 0, 8)], 3, "mt"), ("emit", "s1", 32, 3, 0, 8),
        ("mt", 1, 1),
        ("flush",), ("vcf_flush",),
    ]
    assert vcf == []
    rec.setenv("ISS_HOST_VCF", "1")
    rec.setattr(RecordingEngine, "trace", [])
    trace, vcf = _worker(tmp_path, [("s1", 40), ("short", 2)], "mt", store=True)
    assert trace == [
        ("group", [300, 100]),
        ("mt", 0, 32), ("mt_rows",), ("emit", "s1", 0, 3, 0, 32),
        ("mt", 0, 8), ("mt_rows",), ("emit", "s1", 32, 3, 0, 8),
        ("mt", 1, 1),
        ("flush",),
    ]
    assert vcf == ["s1_0_3/1", "s1_31_3/1", "s1_32_3/1", "s1_39_3/1"]


# ---------------------------------------------------------------------------------------------------- the worker set
def _set(tmp_path, specs, final):
    records = _records()
    works = [_work(spec, records) for spec in specs]
    cpus = [0, 9, 10][:len(works)]
    wrote_final = G.worker_set_iterator(works, BasicErrorModel(), cpus, [str(tmp_path / ("t%d" % k)) for k in range(len(works))], 7,
                                        "metagenomics", False, batch_pairs=16, final_prefix=str(tmp_path / "out") if final else None)
    assert wrote_final is final
    return list(RecordingEngine.trace)


def test_set_groups_every_small_record_at_the_start(rec, tmp_path):
    """The set groups the small records of all work lists before the first round, the short one among them (its draw is
    consumed: one pair asked, none made); big is uploaded alone when its piece comes; a round is one call and one text job."""
    trace = _set(tmp_path, [[("s1", 20), ("short", 3), ("s3", 10)], [("s2", 40), ("big", 5)], [("s1", 8)]], final=True)
    assert trace == [
        ("group", [300, 100]), ("group", [500]), ("group", [400]),
        ("mt_workers", [0, 3, 0], [16, 16, 8], [0, 16, 32]),
        ("scatter", [("s1", 0, 0, 16, 0, 0), ("s2", 0, 16, 16, 9, 7930), ("s1", 0, 32, 8, 10, 19845)]),
        ("mt_workers", [0, 3, 0], [4, 16, 0], [0, 4, 20]),
        ("scatter", [("s1", 16, 0, 4, 0, 4230), ("s2", 16, 4, 16, 9, 12160)]),
        ("mt_workers", [1, 3, 0], [1, 8, 0], [0, 1, 9]),
        ("scatter", [("s2", 32, 1, 8, 9, 16400)]),
        ("add", BIG),
        ("mt_workers", [2, 4, 0], [10, 5, 0], [0, 10, 15]),
        ("scatter", [("s3", 0, 0, 10, 0, 5290), ("big", 0, 10, 5, 9, 18520)]),
        ("flush",),
    ]


def test_set_over_budget_drops_between_rounds_and_uploads_singly_again(rec, tmp_path):
    """GENOME_BUDGET = 2000 (the set keeps half of it): the groups stop before s2; the round that uploads s2 past the budget
    still runs with every genome resident, the drop comes before the next round, and from then on records come back one by one."""
    rec.setattr(G.Worker, "GENOME_BUDGET", 2000)
    rec.setattr(G.Worker, "GROUP_BASES", 1000)
    trace = _set(tmp_path, [[("s1", 20), ("s3", 20)], [("s2", 40), ("s1", 10)]], final=False)
    assert trace == [
        ("group", [300, 500]),
        ("add", 400),
        ("mt_workers", [0, 2], [16, 16], [0, 16]), ("emit", "s1", 0, 0, 0, 16), ("emit", "s2", 0, 9, 16, 16),
        ("clear",),
        ("add", 300), ("add", 400),
        ("mt_workers", [0, 1], [4, 16], [0, 4]), ("emit", "s1", 16, 0, 0, 4), ("emit", "s2", 16, 9, 4, 16),
        ("add", 500),
        ("mt_workers", [2, 1], [16, 8], [0, 16]), ("emit", "s3", 0, 0, 0, 16), ("emit", "s2", 32, 9, 16, 8),
        ("clear",),
        ("add", 500), ("add", 300),
        ("mt_workers", [0, 1], [4, 10], [0, 4]), ("emit", "s3", 16, 0, 0, 4), ("emit", "s1", 0, 9, 4, 10),
        ("flush",),
    ]


def test_set_uploads_alone_the_record_its_group_did_not_take(rec, tmp_path):
    records = _records()
    records["bad"] = G.Record("AC!T" * 50, id="bad")
    works = [_work([("s1", 3)], records), _work([("bad", 2)], records)]
    with pytest.raises(_native.EngineError, match="outside the alphabet"):
        G.worker_set_iterator(works, BasicErrorModel(), [0, 1], [str(tmp_path / "t0"), str(tmp_path / "t1")], 7, "metagenomics",
                              False, batch_pairs=16)
    assert RecordingEngine.trace == [("group", [300, 200]), ("add", 200)]


def test_set_groups_count_the_letters_of_earlier_groups_twice(rec, tmp_path):
    """GENOME_BUDGET = 2000 (the set keeps 1000), GROUP_BASES = 350: with s1 uploaded (300 resident) and short picked, s2 is
    weighed as 300 + (300 + 100) + 400 > 1000 -- the grouping ends before the letters do, and s2 comes alone with its piece."""
    rec.setattr(G.Worker, "GENOME_BUDGET", 2000)
    rec.setattr(G.Worker, "GROUP_BASES", 350)
    trace = _set(tmp_path, [[("s1", 4), ("short", 1), ("s2", 4)]], final=False)
    assert trace == [
        ("group", [300]), ("group", [100]),
        ("mt_workers", [0], [4], [0]), ("emit", "s1", 0, 0, 0, 4),
        ("mt_workers", [1], [1], [0]),
        ("add", 400),
        ("mt_workers", [2], [4], [0]), ("emit", "s2", 0, 0, 0, 4),
        ("flush",),
    ]
