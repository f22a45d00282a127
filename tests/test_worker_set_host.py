"""The worker set's host logic with a stand-in engine (no GPU): final files removed after a failure, and the process-pool
fallback of `generate` taken only when the set could not be set up."""
import logging
import os
import types

import numpy as np
import pytest

from helpers import dense_model, random_genome


class FakeEngine(object):
    """The calls worker_set_iterator makes, with no device behind them.  `fail`: {(method, call number): EngineError}."""

    fail = {}
    read_length_delta = 0

    def __init__(self, device=0):
        self.n = {}

    def _count(self, name):
        self.n[name] = self.n.get(name, 0) + 1
        err = self.fail.get((name, self.n[name]))
        if err is not None:
            raise err

    def load_model(self, dense):
        self.read_length = dense.read_length + self.read_length_delta

    def seed_mt_workers(self, seeds):
        self._count("seed_mt_workers")

    def mt_set_fragment(self, *a):
        pass

    def add_genome(self, seq):
        self.lengths = getattr(self, "lengths", []) + [len(seq)]
        return len(self.lengths) - 1

    def add_genomes(self, seqs):
        return [self.add_genome(s) for s in seqs]

    def clear_genomes(self):
        pass

    def generate_mt_workers(self, g, n, row, sequence_type="metagenomics", gc_bias=False):
        from insilicoseq_amd._native import E_SHORT_RECORD

        self._count("generate_mt_workers")
        short = np.array([k > 0 and not self.read_length < self.lengths[gid] for gid, k in zip(g, n)])
        return np.where(short, 0, n).astype(np.int64), np.where(short, E_SHORT_RECORD, 0).astype(np.int32)

    def fastq_emit_scatter(self, fd_r1, fd_r2, items, n_threads=1):
        self._count("fastq_emit_scatter")

    def fastq_emit(self, *a, **k):
        pass

    def fastq_compress(self, on=True):
        pass

    def fastq_flush(self):
        pass

    def close(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    from insilicoseq_amd import generator

    monkeypatch.setattr(generator, "ReadEngine", FakeEngine)
    monkeypatch.setattr(FakeEngine, "fail", {})
    return FakeEngine


def _works():
    from insilicoseq_amd.generator import Record

    recs = [Record(random_genome(1, 3000), id="a"), Record(random_genome(2, 151), id="b")]  # (b: exactly one read long)
    return [[(recs[0], 300, "default")], [(recs[0], 40, "default"), (recs[1], 5, "default")], [(recs[0], 700, "default")]]


def _set(tmp_path, final=True):
    from insilicoseq_amd.generator import worker_set_iterator

    return worker_set_iterator(_works(), dense_model("novaseq"), [0, 9, 10], [str(tmp_path / ("t%d" % k)) for k in range(3)], 7,
                               "metagenomics", False, batch_pairs=64, final_prefix=str(tmp_path / "out") if final else None)


def _left(tmp_path):
    return sorted(os.listdir(str(tmp_path)))


def test_fake_set_writes_final_files(fake, tmp_path):
    assert _set(tmp_path) is True
    assert _left(tmp_path) == ["out_R1.fastq", "out_R2.fastq"]


@pytest.mark.parametrize("method, call", [("generate_mt_workers", 2), ("generate_mt_workers", 5), ("fastq_emit_scatter", 1),
                                          ("fastq_emit_scatter", 3)])
def test_failure_after_the_final_files_exist_removes_them(fake, method, call, tmp_path):
    from insilicoseq_amd._native import E_INVALID, EngineError

    fake.fail[(method, call)] = EngineError(E_INVALID, "injected")
    with pytest.raises(EngineError, match="injected"):
        _set(tmp_path)
    assert _left(tmp_path) == []


def test_io_error_removes_the_final_files(fake, tmp_path):
    fake.fail[("fastq_emit_scatter", 2)] = OSError(28, "No space left on device")
    with pytest.raises(OSError):
        _set(tmp_path)
    assert _left(tmp_path) == []


def test_size_check_failure_removes_the_final_files(fake, monkeypatch, tmp_path):
    """A record exactly one read long is skipped by the size plan (RL < len(record) is false) -- an engine that takes it
    anyway writes text the plan did not count: the end-of-run check fails and no final file stays."""
    monkeypatch.setattr(FakeEngine, "read_length_delta", -1)
    with pytest.raises(RuntimeError, match="not the size computed"):
        _set(tmp_path)
    assert _left(tmp_path) == []


def test_failure_in_temp_file_mode_keeps_the_temp_files(fake, tmp_path):
    """(Temp-file mode leaves what the reference leaves: its workers' temp files.)"""
    from insilicoseq_amd._native import E_INVALID, EngineError

    fake.fail[("generate_mt_workers", 2)] = EngineError(E_INVALID, "injected")
    with pytest.raises(EngineError):
        _set(tmp_path, final=False)
    assert len(_left(tmp_path)) == 9


def _run_set(tmp_path):
    from insilicoseq_amd.app import _run_worker_set
    from insilicoseq_amd.generator import Record

    records = [Record(random_genome(1, 3000), id="a"), Record(random_genome(2, 4000), id="b")]
    spec = [[(0, 300)], [(0, 40), (1, 20)], [(1, 700)]]
    jobs = [(k, 0, None, spec[k], None, 7, str(tmp_path / ("t%d" % k))) for k in range(3)]
    args = types.SimpleNamespace(seed=7, sequence_type="metagenomics", gc_bias=False, output=str(tmp_path / "out"))
    return _run_worker_set(jobs, records, dense_model("novaseq"), args, False, 3)


@pytest.mark.parametrize("code", ["E_NOMEM", "E_INVALID", "E_HIP"])
def test_fallback_when_seeding_fails(fake, code, tmp_path, caplog):
    from insilicoseq_amd import _native

    fake.fail[("seed_mt_workers", 1)] = _native.EngineError(getattr(_native, code), "seed refused")
    with caplog.at_level(logging.WARNING):
        assert _run_set(tmp_path) is None
    assert "seed refused" in caplog.text and "one process per worker instead" in caplog.text
    assert _left(tmp_path) == []


def test_fallback_when_the_first_call_has_no_memory(fake, tmp_path, caplog):
    from insilicoseq_amd._native import E_NOMEM, EngineError

    fake.fail[("generate_mt_workers", 1)] = EngineError(E_NOMEM, "no memory for the workers' stream buffers")
    with caplog.at_level(logging.WARNING):
        assert _run_set(tmp_path) is None
    assert "no memory for the workers' stream buffers" in caplog.text
    assert _left(tmp_path) == []


@pytest.mark.parametrize("code, call", [("E_INVALID", 1), ("E_HIP", 1), ("E_NOMEM", 2), ("E_INVALID", 2)])
def test_no_fallback_when_the_set_fails(fake, code, call, tmp_path, caplog):
    """Any other engine error is a failure of the set, not a reason to run the pool: it propagates, and no final file stays."""
    from insilicoseq_amd import _native

    fake.fail[("generate_mt_workers", call)] = _native.EngineError(getattr(_native, code), "injected")
    with caplog.at_level(logging.WARNING), pytest.raises(_native.EngineError, match="injected"):
        _run_set(tmp_path)
    assert "one process per worker" not in caplog.text
    assert _left(tmp_path) == []
