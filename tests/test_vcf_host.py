"""The worker loop's route to the device-built VCF text (ReadEngine.vcf_emit), with stand-in engines: no GPU."""
import io
import os
import re

import pytest

from insilicoseq_amd import _native
from insilicoseq_amd import generator as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeEngine:
    read_length = 100

    def __init__(self, arena_ok=True, nomem=0, broken=False):
        self.calls, self.arena_ok, self.nomem, self.broken = [], arena_ok, nomem, broken
        self.mutations_capacity = 1 << 17

    def generate_batch(self, gids, counts, **k):
        if not self.arena_ok:
            raise _native.EngineError(_native.E_INVALID, "iss_generate_batch: the records of one call must stay below 2^34 - 4096 bases")
        self.calls.append(("batch", list(gids), list(counts), k["first_ordinal"]))

    def reserve(self, n):
        self.calls.append(("reserve", n))

    def generate(self, gid, n, first_ordinal, seed, sequence_type, gc_bias, out_first_pair):
        self.calls.append(("gen1", gid, n, first_ordinal, out_first_pair))

    def mutations(self):
        raise AssertionError("mutations() called on the device route")

    def mutations_reserve(self, cap):
        self.calls.append(("mreserve", cap))
        self.mutations_capacity = cap

    def vcf_emit(self, fd, items, cpu, source="philox"):
        self.calls.append(("vcf", fd, list(items), cpu, source))
        if self.broken:
            raise _native.EngineError(_native.E_IO, "write failed")
        if self.nomem:
            self.mutation_slots_needed, self.nomem = self.nomem, 0
            raise _native.EngineError(_native.E_NOMEM, "mutation rows overflow")

    def fastq_emit_batch(self, fd1, fd2, items, cpu):
        self.calls.append(("emit", list(items)))


class FakeWorker:
    BATCH_PAIRS = 50
    device_vcf = True

    def __init__(self, engine):
        self.engine = engine
        self.ordinal, self.seed, self.cpu_number, self.store_mutations = 0, 1, 4, True
        self.consumers = [G.Reads(engine, self.cpu_number)]

    def needs_room_for(self, record):
        return False

    def genome_id(self, record):
        return {"a": 0, "b": 1}[record.id]


class Handle:
    """A .vcf handle of which only the descriptor is used."""
    def fileno(self):
        return 77

    def write(self, text):
        raise AssertionError("the handle is written on the device route")


WORK = [(G.Record("A" * 500, id="a"), 40, "default"), (G.Record("C" * 500, id="b"), 25, "default")]


def _run(engine):
    w = FakeWorker(engine)
    with open(os.devnull, "wb") as f1, open(os.devnull, "wb") as f2:
        G._simulate_work_batched(w, WORK, f1, f2, Handle(), "metagenomics", False)
    return w


def test_batched_loop_hands_vcf_emit_the_fastq_items_once_per_call():
    w = _run(FakeEngine())
    calls = w.engine.calls
    emits = [c[1] for c in calls if c[0] == "emit"]
    vcfs = [c for c in calls if c[0] == "vcf"]
    # BATCH_PAIRS = 50: (a: 40, b: 10) and (b: 15, pair ids from 10)
    assert emits == [[("a", 0, 0, 40), ("b", 0, 40, 10)], [("b", 10, 0, 15)]]
    assert [c[2] for c in vcfs] == emits and all(c[1] == 77 and c[3] == 4 and c[4] == "philox" for c in vcfs)
    assert [c[0] for c in calls] == ["batch", "vcf", "emit", "batch", "vcf", "emit"] and w.ordinal == 65


def test_arena_fallback_emits_once_per_single_call_at_its_rows():
    w = _run(FakeEngine(arena_ok=False))
    calls = [c for c in w.engine.calls if c[0] in ("gen1", "vcf", "emit")]
    assert [c[0] for c in calls] == ["gen1", "vcf", "gen1", "vcf", "emit", "gen1", "vcf", "emit"]
    assert [c[2] for c in calls if c[0] == "vcf"] == [[("a", 0, 0, 40)], [("b", 0, 40, 10)], [("b", 10, 0, 15)]]
    assert [c for c in calls if c[0] == "gen1"] == [("gen1", 0, 40, 0, 0), ("gen1", 1, 10, 40, 40), ("gen1", 1, 15, 50, 0)]


def test_overflow_reserves_once_regenerates_once_and_emits_again():
    w = _run(FakeEngine(nomem=1 << 20))
    kinds = [c[0] for c in w.engine.calls]
    assert kinds[:6] == ["batch", "vcf", "mreserve", "batch", "vcf", "emit"]
    need = 1 << 20
    assert [c[1] for c in w.engine.calls if c[0] == "mreserve"] == [need + need // 8 + (1 << 16)]
    assert w.engine.calls[0] == w.engine.calls[3] and w.engine.calls[1] == w.engine.calls[4]  # the same call, the same items
    assert kinds.count("vcf") == 3 and kinds.count("batch") == 3  # (the second batch: no overflow)


def test_another_error_propagates():
    with pytest.raises(_native.EngineError) as e:
        _run(FakeEngine(broken=True))
    assert e.value.code == _native.E_IO


def test_host_route_with_device_vcf_off():
    """A worker whose `device_vcf` is False (ISS_HOST_VCF=1; the stand-ins of test_host_cpu.py) takes the host route."""
    from insilicoseq_amd.engine import MUT_DTYPE
    import numpy as np

    class HostEngine(FakeEngine):
        def mutations(self):
            rows = np.zeros(1, dtype=MUT_DTYPE)
            rows["ref"], rows["alt"] = ord("A"), ord("C")
            return rows

        def vcf_emit(self, *a, **k):
            raise AssertionError("vcf_emit called on the host route")

    class HostWorker(FakeWorker):
        device_vcf = False

    w = HostWorker(HostEngine())
    vcf = io.StringIO()
    with open(os.devnull, "wb") as f1, open(os.devnull, "wb") as f2:
        G._simulate_work_batched(w, WORK, f1, f2, vcf, "metagenomics", False)
    assert [line.split("\t")[0] for line in vcf.getvalue().splitlines()] == ["a_0_4/1", "b_10_4/1"]


def test_abi_names_both_entries():
    assert "iss_vcf_emit" in _native.EXPORTS and "iss_vcf_flush" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    assert re.search(r"\bint iss_vcf_emit\(iss_ctx \*ctx, int fd, int32_t source,", header)
    assert re.search(r"\bint iss_vcf_flush\(iss_ctx \*ctx\);", header)
    assert "#define ISS_ABI_VERSION 8" in header
    from insilicoseq_amd.engine import ReadEngine
    assert callable(ReadEngine.vcf_emit) and callable(ReadEngine.vcf_flush)


def test_engine_error_survives_the_process_pool():
    """`generate --gpus N` runs one process per worker: a worker's EngineError (an overflow that cannot be met, a failed write of
    the VCF text) reaches the parent pickled.  It must come out as itself -- an exception that cannot be rebuilt kills the pool's
    result thread and the command never ends."""
    import pickle

    e = pickle.loads(pickle.dumps(_native.EngineError(_native.E_IO, "write failed: No space left on device")))
    assert isinstance(e, _native.EngineError) and e.code == _native.E_IO
    assert str(e) == "write failed: No space left on device (iss error -5)"


def test_vcf_emit_on_a_library_without_the_entries_raises():
    """A library from before iss_vcf_emit still loads (A/B runs against an older build); the device route then raises
    instead of falling back."""
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine.__new__(ReadEngine)
    eng._lib, eng._ctx = object(), None
    with pytest.raises(_native.NativeLibraryError):
        eng.vcf_emit(3, [("a", 0, 0, 1)], 0)
    with pytest.raises(_native.NativeLibraryError):
        eng.vcf_flush()
