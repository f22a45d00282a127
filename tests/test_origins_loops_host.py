"""Where the work loops make the --origins call (no GPU; the recording engine of tests/test_work_loops_host.py): exactly where the
text job is handed over, with the text job's items and the records' lengths -- once per item in the arena fall-back, where every
generate call moves on to the other set of descriptors -- and flushed where the other pipes are; without the flag, no call."""
import os

import pytest

import test_work_loops_host as W
from insilicoseq_amd import generator as G
from insilicoseq_amd.model import BasicErrorModel


class OriginsEngine(W.RecordingEngine):
    def origins_emit_batch(self, fd, items, record_lengths, cpu):
        assert os.fstat(fd).st_size == 0  # (the worker's own file: the stand-in writes nothing)
        self._log("origins", list(items), list(record_lengths), cpu)

    def origins_flush(self):
        self._log("origins_flush")


@pytest.fixture
def rec(monkeypatch):
    for name in ("ISS_HOST_FASTQ", "ISS_HOST_VCF", "ISS_ITEMWISE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(G, "ReadEngine", OriginsEngine)
    monkeypatch.setattr(W.RecordingEngine, "trace", [])
    monkeypatch.setattr(W.RecordingEngine, "arena_ok", True)
    monkeypatch.setattr(W.RecordingEngine, "overflow", set())
    monkeypatch.setattr(G.Worker, "BATCH_PAIRS", 32)
    monkeypatch.setattr(G.Worker, "GROUP_BASES", 750)
    return monkeypatch


SPEC = [("s1", 40), ("s2", 25)]  # s1: 300 bases, s2: 400


def _run(tmp_path, rng, origins=True):
    prefix = str(tmp_path / "w")
    G.worker_iterator(W._work(SPEC), BasicErrorModel(None, None, False), 3, prefix, 5, "metagenomics", False, device=0, rng=rng,
                      origins=origins)
    assert os.path.exists(prefix + "_origins.bedpe") == origins
    return list(W.RecordingEngine.trace)


def test_batched_loop_emits_beside_the_text_job(rec, tmp_path):
    assert _run(tmp_path, "philox") == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("origins", [("s1", 0, 0, 32)], [300], 3), ("emit_batch", [("s1", 0, 0, 32)], 3),
        ("batch", [0, 1], [8, 24], 32), ("origins", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], [300, 400], 3),
        ("emit_batch", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3),
        ("batch", [1], [1], 64), ("origins", [("s2", 24, 0, 1)], [400], 3), ("emit_batch", [("s2", 24, 0, 1)], 3),
        ("origins_flush",), ("flush",),
    ]


def test_arena_fallback_emits_once_per_item(rec, tmp_path):
    rec.setattr(W.RecordingEngine, "arena_ok", False)
    assert _run(tmp_path, "philox") == [
        ("group", [300, 400]),
        ("batch", [0], [32], 0), ("reserve", 32),
        ("gen", 0, 32, 0, 0), ("origins", [("s1", 0, 0, 32)], [300], 3), ("emit_batch", [("s1", 0, 0, 32)], 3),
        ("batch", [0, 1], [8, 24], 32), ("reserve", 32),
        ("gen", 0, 8, 32, 0), ("origins", [("s1", 32, 0, 8)], [300], 3),
        ("gen", 1, 24, 40, 8), ("origins", [("s2", 0, 8, 24)], [400], 3),
        ("emit_batch", [("s1", 32, 0, 8), ("s2", 0, 8, 24)], 3),
        ("batch", [1], [1], 64), ("reserve", 1),
        ("gen", 1, 1, 64, 0), ("origins", [("s2", 24, 0, 1)], [400], 3), ("emit_batch", [("s2", 24, 0, 1)], 3),
        ("origins_flush",), ("flush",),
    ]


def test_mt_loop_emits_in_front_of_every_text_job(rec, tmp_path):
    trace = [c for c in _run(tmp_path, "mt") if c[0] in ("mt", "origins", "emit", "origins_flush", "flush")]
    assert trace == [
        ("mt", 0, 32), ("origins", [("s1", 0, 0, 32)], [300], 3), ("emit", "s1", 0, 3, 0, 32),
        ("mt", 0, 8), ("origins", [("s1", 32, 0, 8)], [300], 3), ("emit", "s1", 32, 3, 0, 8),
        ("mt", 1, 25), ("origins", [("s2", 0, 0, 25)], [400], 3), ("emit", "s2", 0, 3, 0, 25),
        ("origins_flush",), ("flush",),
    ]


@pytest.mark.parametrize("rng", ["philox", "mt"])
def test_without_the_flag_no_call_is_added(rec, tmp_path, rng):
    assert not [c for c in _run(tmp_path, rng, origins=False) if c[0].startswith("origins")]
