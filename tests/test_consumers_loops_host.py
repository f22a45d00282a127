"""Every reader of a settled generate call at once (no GPU; the recording engine of tests/test_work_loops_host.py and a stand-in for
torch): the COMPLETE sequence of engine calls of worker_iterator with --report, --error_report, --depth, --origins and --bgzip
together, with FASTQ and with uBAM output, through each of the four work loops -- batched, the arena fall-back, item-wise Philox
and MT.  The order is tally, error tally, depth, origins, reads; a reader of the output rows (tally, reads) runs once per batch, a
reader of what the next generate call overwrites (error tally, depth, origins) behind every call; the pipes are flushed as uBAM,
origins, FASTQ, VCF and the three accumulators saved behind them.  Without the flags: the same trace less those calls."""
import contextlib
import os

import numpy as np
import pytest

import test_work_loops_host as W
from insilicoseq_amd import generator as G
from insilicoseq_amd.model import BasicErrorModel


class AllEngine(W.RecordingEngine):
    device = 0

    def tally_words(self):
        self._log("tally_words")
        return 16

    def error_tally_words(self):
        self._log("error_tally_words")
        return 8

    def tally(self, first_pair, n_pairs, ptr):
        self._log("tally", first_pair, n_pairs)

    def error_tally(self, first_pair, n_pairs, ptr, source="philox"):
        self._log("errtally", first_pair, n_pairs, source)

    def depth_mark(self, first_pair, n_pairs, table_ptr, n_table, diff_ptr):
        self._log("depth", first_pair, n_pairs, n_table)

    def origins_emit_batch(self, fd, items, record_lengths, cpu):
        self._log("origins", list(items), list(record_lengths), cpu)

    def origins_flush(self):
        self._log("origins_flush")

    def origins_compress(self, on=True):
        self._log("origins_compress", on)

    def vcf_compress(self, on=True):
        self._log("vcf_compress", on)

    def ubam_emit_batch(self, fd, items, cpu):
        self._log("ubam", list(items), cpu)

    def ubam_flush(self):
        self._log("ubam_flush")

    def synchronize(self):
        self._log("sync")


class FakeTensor(object):
    def __init__(self, array):
        self.array = array

    def data_ptr(self):
        return 4096

    def cpu(self):
        return self

    def numpy(self):
        return self.array

    def to(self, device):
        return self


class FakeStream(object):
    def synchronize(self):
        pass


class FakeCuda(object):
    @staticmethod
    def device(index):
        return contextlib.nullcontext()

    @staticmethod
    def synchronize():
        pass

    @staticmethod
    def current_stream():
        return FakeStream()


class FakeTorch(object):
    int32, int64, cuda = np.int32, np.int64, FakeCuda

    @staticmethod
    def device(kind, index):
        return (kind, index)

    @staticmethod
    def zeros(n, dtype, device):
        return FakeTensor(np.zeros(n, dtype=dtype))

    @staticmethod
    def from_numpy(array):
        return FakeTensor(array)


@pytest.fixture
def rec(monkeypatch):
    for name in ("ISS_HOST_FASTQ", "ISS_HOST_VCF", "ISS_ITEMWISE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(G, "ReadEngine", AllEngine)
    monkeypatch.setattr("insilicoseq_amd.tensors._torch", lambda: FakeTorch)
    monkeypatch.setattr(W.RecordingEngine, "trace", [])
    monkeypatch.setattr(W.RecordingEngine, "arena_ok", True)
    monkeypatch.setattr(W.RecordingEngine, "overflow", set())
    monkeypatch.setattr(G.Worker, "BATCH_PAIRS", 32)
    monkeypatch.setattr(G.Worker, "GROUP_BASES", 750)
    return monkeypatch


SPEC = [("s1", 40), ("s2", 25)]  # s1: 300 bases, s2: 400; batches of 32: (s1: 32), (s1: 8, s2: 24), (s2: 1)
CPU = 3
LOOPS = ["batched", "fallback", "itemwise", "mt"]
CONSUMER_CALLS = ("tally_words", "error_tally_words", "tally", "errtally", "depth", "origins", "origins_flush", "origins_compress",
                  "vcf_compress", "sync")
EXTRA_FILES = ("w.tally.npy", "w.errtally.npy", "w.depth.npz", "w_origins.bedpe", "w.bam")


def _run(rec, tmp_path, loop, ubam=False, on=True):
    """worker_iterator as worker 3 with seed 5 through ``loop`` -> the engine calls (the row buffer's size aside)"""
    if loop == "fallback":
        rec.setattr(W.RecordingEngine, "arena_ok", False)
    if loop == "itemwise":
        rec.setenv("ISS_ITEMWISE", "1")
    flags = dict(report=True, depth=True, origins=True, bgzip=True, error_report=True) if on else {}
    G.worker_iterator(W._work(SPEC), BasicErrorModel(None, None, True), CPU, str(tmp_path / "w"), 5, "metagenomics", False, device=0,
                      rng="mt" if loop == "mt" else "philox", ubam=ubam, **flags)
    return [c[:1] if c[0] == "mutations_reserve" else c for c in W.RecordingEngine.trace]


HEAD = [("origins_compress", True), ("vcf_compress", True), ("tally_words",), ("error_tally_words",), ("mutations_reserve",),
        ("group", [300, 400])]


def _tail(ubam):
    return ([("ubam_flush",)] if ubam else []) + [("origins_flush",), ("flush",), ("vcf_flush",), ("sync",), ("sync",), ("sync",)]


def _reads(ubam, items, item_wise=False):
    """The call that takes the rows of ``items`` as reads: one uBAM job, one FASTQ text job, or fastq_emit of the one item."""
    if ubam:
        return ("ubam", items, CPU)
    if item_wise:
        (rid, first_i, row, n), = items
        return ("emit", rid, first_i, CPU, row, n)
    return ("emit_batch", items, CPU)


def _batched(ubam):
    def batch(gids, counts, ordinal, items, lengths):
        n = sum(counts)
        return [("batch", gids, counts, ordinal), ("vcf", items, CPU, "philox"), ("tally", 0, n), ("errtally", 0, n, "philox"),
                ("depth", 0, n, len(items)), ("origins", items, lengths, CPU), _reads(ubam, items)]

    return (batch([0], [32], 0, [("s1", 0, 0, 32)], [300]) +
            batch([0, 1], [8, 24], 32, [("s1", 32, 0, 8), ("s2", 0, 8, 24)], [300, 400]) +
            batch([1], [1], 64, [("s2", 24, 0, 1)], [400]))


def _fallback(ubam):
    def batch(gids, counts, ordinal, items, lengths):
        calls, at = [("batch", gids, counts, ordinal), ("reserve", sum(counts))], ordinal
        for gid, item, length in zip(gids, items, lengths):
            _rid, _first_i, row, n = item
            calls += [("gen", gid, n, at, row), ("vcf", [item], CPU, "philox"), ("errtally", row, n, "philox"), ("depth", row, n, 1),
                      ("origins", [item], [length], CPU)]
            at += n
        return calls + [("tally", 0, sum(counts)), _reads(ubam, items)]

    return (batch([0], [32], 0, [("s1", 0, 0, 32)], [300]) +
            batch([0, 1], [8, 24], 32, [("s1", 32, 0, 8), ("s2", 0, 8, 24)], [300, 400]) +
            batch([1], [1], 64, [("s2", 24, 0, 1)], [400]))


def _item_wise(ubam, rng):
    def piece(gid, ordinal, item, length):
        _rid, _first_i, _row, n = item
        gen = ("mt", gid, n) if rng == "mt" else ("gen", gid, n, ordinal, 0)
        return [gen, ("vcf", [item], CPU, rng), ("tally", 0, n), ("errtally", 0, n, rng), ("depth", 0, n, 1),
                ("origins", [item], [length], CPU), _reads(ubam, [item], item_wise=True)]

    return piece(0, 0, ("s1", 0, 0, 32), 300) + piece(0, 32, ("s1", 32, 0, 8), 300) + piece(1, 40, ("s2", 0, 0, 25), 400)


def _expected(loop, ubam):
    body = {"batched": lambda: _batched(ubam), "fallback": lambda: _fallback(ubam), "itemwise": lambda: _item_wise(ubam, "philox"),
            "mt": lambda: _item_wise(ubam, "mt")}[loop]()
    return HEAD + body + _tail(ubam)


def test_the_second_batch_spelled_out():
    """(the expectation's own arithmetic, once by hand: the batch that holds the end of s1 and the start of s2)"""
    items = [("s1", 32, 0, 8), ("s2", 0, 8, 24)]
    assert _batched(False)[7:14] == [
        ("batch", [0, 1], [8, 24], 32), ("vcf", items, 3, "philox"), ("tally", 0, 32), ("errtally", 0, 32, "philox"),
        ("depth", 0, 32, 2), ("origins", items, [300, 400], 3), ("emit_batch", items, 3)]
    assert _fallback(True)[9:23] == [
        ("batch", [0, 1], [8, 24], 32), ("reserve", 32),
        ("gen", 0, 8, 32, 0), ("vcf", items[:1], 3, "philox"), ("errtally", 0, 8, "philox"), ("depth", 0, 8, 1),
        ("origins", items[:1], [300], 3),
        ("gen", 1, 24, 40, 8), ("vcf", items[1:], 3, "philox"), ("errtally", 8, 24, "philox"), ("depth", 8, 24, 1),
        ("origins", items[1:], [400], 3),
        ("tally", 0, 32), ("ubam", items, 3)]
    assert _item_wise(False, "mt")[7:14] == [
        ("mt", 0, 8), ("vcf", items[:1], 3, "mt"), ("tally", 0, 8), ("errtally", 0, 8, "mt"), ("depth", 0, 8, 1),
        ("origins", items[:1], [300], 3), ("emit", "s1", 32, 3, 0, 8)]


@pytest.mark.parametrize("ubam", [False, True])
@pytest.mark.parametrize("loop", LOOPS)
def test_every_reader_at_once(rec, tmp_path, loop, ubam):
    assert _run(rec, tmp_path, loop, ubam) == _expected(loop, ubam)
    reads = ["w.bam"] if ubam else ["w_R1.fastq", "w_R2.fastq"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(["w.tally.npy", "w.errtally.npy", "w.depth.npz", "w.vcf", "w_origins.bedpe"] + reads)
    tally, errtally = np.load(str(tmp_path / "w.tally.npy")), np.load(str(tmp_path / "w.errtally.npy"))
    assert (tally.dtype, tally.shape, errtally.dtype, errtally.shape) == (np.uint64, (16,), np.uint64, (8,))
    z = np.load(str(tmp_path / "w.depth.npz"))
    assert sorted(z.files) == ["diff", "ordinals", "table"] and z["diff"].dtype == np.int32
    assert z["ordinals"].dtype == np.int64 and z["ordinals"].tolist() == [0, 1] and len(z["table"]) == 2


@pytest.mark.parametrize("loop", LOOPS)
def test_without_the_flags_the_same_trace_less_the_readers(rec, tmp_path, loop):
    trace = _run(rec, tmp_path, loop, on=False)
    assert trace == [c for c in _expected(loop, False) if c[0] not in CONSUMER_CALLS]
    assert not [name for name in EXTRA_FILES if os.path.exists(str(tmp_path / name))]
    assert sorted(os.listdir(str(tmp_path))) == ["w.vcf", "w_R1.fastq", "w_R2.fastq"]
