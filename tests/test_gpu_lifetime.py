"""What a context allocates goes back when it is closed, and a refused allocation leaves a context that works (DESIGN.md
section 26: every device and pinned buffer, stream and event of the host side belongs to one owning handle).

The first test sees buffers of MB size -- the output rows, the pipes' text and member buffers, the worker set's pools -- not a
lost 4 KB table: hipMemGetInfo counts in granules of DRIFT_GRANULE bytes."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import helpers as H

pytestmark = pytest.mark.gpu

CYCLES = 5
# Measured with this test on the commit before the handles (hand-written frees), three runs on an MI355X: free memory after cycle
# 1 minus free memory after cycle 5 was 58 720 256 bytes (56 MiB) every time -- one step between the first and the second cycle,
# none after it: what a process's second context costs once, not what a cycle loses -- and the smallest non-zero step between two
# readings of hipMemGetInfo was 2 097 152 bytes, its granule.  The bound is the largest drift seen plus one granule (one rounding).
# An engine held 1 189 085 184 bytes while it lived, 19.5 times the bound.
DRIFT_SEEN = 58720256
DRIFT_GRANULE = 2 << 20
DRIFT_BOUND = DRIFT_SEEN + DRIFT_GRANULE


def _zeros(n, dtype):
    return torch.zeros(int(n), dtype=dtype, device="cuda")


def _cycle(dense, genome, group, tmp_path, k, bufs, marks):
    """One engine that touches every owner of the host side once, one BamTally, one FastqTally; returns the free device memory
    while they were alive."""
    import bam_synth
    import fastq_cases as FC
    from insilicoseq_amd import modeller
    from insilicoseq_amd.engine import BamTally, ReadEngine
    from insilicoseq_amd.fastq_report import FastqTally

    def fd(name):
        return os.open(str(tmp_path / ("c%d_%s" % (k, name))), os.O_CREAT | os.O_TRUNC | os.O_WRONLY, 0o644)

    def mark():
        marks.append(torch.cuda.mem_get_info()[0])

    fds = {name: fd(name) for name in ("r1", "r2", "z1", "z2", "vcf", "vcfz", "bam", "org", "orgz")}
    mark()
    eng = ReadEngine(0)
    mark()
    try:
        eng.load_model(dense)
        mark()
        gid = eng.add_genome(genome)
        mark()
        gids = eng.add_genomes(group)
        assert min(gids) >= 0
        eng.reserve(8192)
        mark()
        eng.mutations_reserve(1 << 16)
        mark()
        n = 2048
        eng.generate(gid, n, seed=3 + k)
        items = [("one", 0, 0, n)]
        eng.fastq_emit_batch(fds["r1"], fds["r2"], items, 0)
        eng.fastq_flush()
        mark()
        eng.fastq_compress(True)
        eng.fastq_emit_batch(fds["z1"], fds["z2"], items, 0)
        eng.fastq_flush()
        mark()
        eng.vcf_emit(fds["vcf"], items, 0)
        eng.vcf_flush()
        mark()
        eng.vcf_compress(True)
        eng.vcf_emit(fds["vcfz"], items, 0)
        eng.vcf_flush()
        mark()
        eng.ubam_emit_batch(fds["bam"], items, 0)
        eng.ubam_flush()
        mark()
        eng.origins_emit_batch(fds["org"], items, [len(genome)], 0)
        eng.origins_flush()
        mark()
        eng.origins_compress(True)
        eng.origins_emit_batch(fds["orgz"], items, [len(genome)], 0)
        eng.origins_flush()
        mark()
        torch.cuda.synchronize()
        tally, err = _zeros(eng.tally_words(), torch.int64), _zeros(eng.error_tally_words(), torch.int64)
        eng.tally(0, n, tally.data_ptr())
        eng.error_tally(0, n, err.data_ptr())
        table = torch.tensor([[0, len(genome)]], dtype=torch.int64, device="cuda")
        n_words = len(genome) + 1
        torch.cuda.synchronize()
        eng.depth_mark(0, n, table.data_ptr(), 1, bufs["diff"].data_ptr())
        eng.depth_finish(bufs["diff"].data_ptr(), n_words, bufs["depth"].data_ptr(), table.data_ptr(), 1, 64, bufs["stats"].data_ptr(),
                         bufs["bins"].data_ptr())
        eng.export(0, n, bases_ptr=bufs["bases"].data_ptr(), qual_ptr=bufs["qual"].data_ptr(), coords_ptr=bufs["coords"].data_ptr(),
                   item_ptr=bufs["item"].data_ptr())
        eng.export_mutations(0, n, truth_ptr=bufs["truth"].data_ptr(), events_ptr=bufs["events"].data_ptr(), capacity=1 << 16,
                             n_events_ptr=bufs["n_events"].data_ptr())
        eng.synchronize()
        assert int(tally.sum().item()) > 0 and int(bufs["n_events"].item()) > 0
        eng.generate_batch(gids, [300, 200, 100], first_ordinal=n, seed=3 + k)
        eng.synchronize()
        eng.seed_mt(5 + k)
        assert eng.generate_mt(gid, 512) == 512
        mark()
        eng.seed_mt_workers([31, 32, 35])
        mark()
        eng.mt_workers_mutations_reserve(4096)
        mark()
        done, status = eng.generate_mt_workers([gid] * 3, [200] * 3, [0, 400, 800])
        assert list(done) == [200] * 3 and not status.any()
        eng.synchronize()
        with BamTally(0) as bam:
            path = str(tmp_path / ("c%d.bam" % k))
            bam_synth.write_bam(path, 7, n_pairs=40)
            modeller.tally_bam(bam, path)
            assert bam.tallies()[1] == -1
            with FastqTally(0, 151) as fq:
                fq.feed(FC.mixed(30, 81, (10, 151)), 0)
                assert fq.download()["records"][0] == 30
                torch.cuda.synchronize()
                alive = torch.cuda.mem_get_info()[0]
    finally:
        eng.close()
        for f in fds.values():
            os.close(f)
    for name in ("r1", "z1", "vcf", "vcfz", "bam", "org", "orgz"):
        assert os.path.getsize(str(tmp_path / ("c%d_%s" % (k, name)))) > 0, name
    return alive


def test_contexts_give_their_memory_back(tmp_path, monkeypatch):
    """CYCLES engines one after the other, each with every pipe, work array, chain and worker set in use once, each closed: the
    device's free memory after the last cycle is that after the first (within DRIFT_BOUND: the 56 MiB of one-time drift measured
    on the commit before the handles in three runs, plus one granule of hipMemGetInfo, 2 MiB), and every engine held at least 16
    times the bound while it lived -- so a main buffer that stayed behind in every cycle would show."""
    import __graft_entry__ as ge

    ge.build()
    monkeypatch.setenv("ISS_MT_SET_TURN", "37")
    monkeypatch.setenv("ISS_MT_SET_BUF_TURNS", "3")
    dense = H.dense_model("novaseq")
    genome = H.random_genome(5, 100000)
    group = [H.random_genome(61 + i, 3000) for i in range(3)]
    RL, n = dense.read_length, 2048
    bufs = {"diff": _zeros(len(genome) + 1, torch.int32), "depth": _zeros(len(genome) + 1, torch.int32), "stats": _zeros(4, torch.int64),
            "bins": _zeros(len(genome) // 64 + 2, torch.int64), "bases": _zeros(n * 2 * RL, torch.uint8), "qual": _zeros(n * 2 * RL, torch.uint8),
            "coords": _zeros(n * 4, torch.int64), "item": _zeros(n, torch.int32), "truth": _zeros(n * 2 * RL, torch.uint8),
            "events": _zeros((1 << 16) * 6, torch.int32), "n_events": _zeros(1, torch.int64)}
    free, held, marks = [], [], []
    for k in range(CYCLES):
        bufs["diff"].zero_()
        alive = _cycle(dense, genome, group, tmp_path, k, bufs, marks)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
        marks.append(free[-1])
        held.append(free[-1] - alive)
    steps = sorted(set(abs(a - b) for a, b in zip(marks, marks[1:])) - {0})
    print("free after each cycle: %r; drift %d B; held while alive: %r; smallest non-zero steps of the readings: %r" % (free, free[0] - free[-1], held, steps[:4]))
    assert free[0] - free[-1] <= DRIFT_BOUND
    assert min(held) >= 16 * DRIFT_BOUND


def test_a_refused_reservation_leaves_a_working_engine():
    """A reservation whose first buffer alone is twice the device: E_NOMEM with the reservation's footprint, nothing held; the
    engine then reserves and generates as if nothing had happened, and closes."""
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import EngineError, ReadEngine
    from oracle import oracle as O

    dense = H.dense_model("novaseq")
    genome = H.random_genome(5, 100000)
    n = 4096
    eng = ReadEngine(0)
    try:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        row_bytes = eng._lib.iss_output_row(eng._ctx)
        assert row_bytes > 0
        with pytest.raises(EngineError) as e:
            eng.reserve(2 * torch.cuda.mem_get_info()[1] // row_bytes)
        assert e.value.code == _native.E_NOMEM
        assert "need" in str(e.value) and "GB of HBM" in str(e.value)
        eng.reserve(n)
        eng.generate(gid, n, first_ordinal=0, seed=42)
        eng.synchronize()
        got = eng.download(0, n)
        exp = O.Oracle(dense).simulate(O.Rng().seed_philox(42), genome, n)
        assert exp["status"] == 0
        for key in ("r1_base", "r1_qual", "r2_base", "r2_qual"):
            assert np.array_equal(got[key], exp[key]), key
    finally:
        eng.close()
