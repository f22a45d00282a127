"""CPU companion of tests/test_gpu_row_readers.py: the plain reference that module compares the row readers with is pinned
here, where the oracle runs -- helpers.fastq_text equals the host formatter (iss_fastq_write) on the oracle's arrays at every
read length of the sweep, the sweep's --store_mutations work lists yield the rows a VCF case needs from the oracle alone, and
the export tiles of the cases that are to start at different alignments do so by iss_export.hip.h's rule.  No GPU here."""
import numpy as np
import pytest

import helpers as H

IDS = ("g", "NZ_" + "k" * 294 + ".17")  # record ids of 1 and of 300 letters
EMITS = ((4, 13), (17, 187))             # (first pair id, pairs) of the two emits: 4 .. 16 crosses 9|10, 17 .. 203 crosses 99|100


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import _native

    return _native


def test_the_sweep_is_the_one_the_readers_need():
    assert H.ROW_SWEEP == (2, 5, 7, 8, 9, 16, 31, 32, 33, 64, 100, 128, 250, 256, 997, 1024)
    assert len(IDS[0]) == 1 and len(IDS[1]) == 300
    assert sum(n for _, n in EMITS) == 200 and EMITS[0][0] + EMITS[0][1] == EMITS[1][0]
    for RL in H.ROW_SWEEP:  # the models are of the sweep's read lengths, with indels, two empty bins, lower-case and IUPAC records
        d = H.row_sweep_model(RL)
        assert d.read_length == RL and (d.n_q == 1) == (RL == 2) and (d.ins > 0).any() and (d.dele > 0).any()
        assert (np.asarray(d.bin_nonempty) == 0).any()
        letters = set(H.row_sweep_genome(RL).encode())
        assert letters & set(b"acgt") and letters & set(b"NRYWSMKHBVD")


@pytest.mark.parametrize("RL", H.ROW_SWEEP)
def test_formatter_equals_host_fastq_write(native, RL, tmp_path):
    from insilicoseq_amd.engine import fastq_write
    from oracle import oracle as O

    dense = H.row_sweep_model(RL)
    exp = H.row_sweep_oracle_rows(dense, O.Rng().seed_philox(H.ROW_SWEEP_SEED), H.row_sweep_genome(RL), H.ROW_SWEEP_PAIRS,
                                  H.ROW_SWEEP_FIRST_ORDINAL)
    assert exp["bases"].shape == exp["qual"].shape == (H.ROW_SWEEP_PAIRS, 2, RL)
    for rid in IDS:
        paths = [tmp_path / ("%d_%d_%d.fq" % (RL, len(rid), m)) for m in (1, 2)]
        with open(paths[0], "wb") as f1, open(paths[1], "wb") as f2:
            row = 5
            for first_i, n in EMITS:
                b, q = np.ascontiguousarray(exp["bases"][row:row + n]), np.ascontiguousarray(exp["qual"][row:row + n])
                # rows of pitch 2 RL: mate 1 then mate 2 of a pair side by side, mate 2's arrays start RL bytes in
                fastq_write(f1.fileno(), f2.fileno(), rid, first_i, H.ROW_SWEEP_CPU, n, RL, 2 * RL, b.reshape(-1), q.reshape(-1),
                            b.reshape(-1)[RL:], q.reshape(-1)[RL:], n_threads=2)
                row += n
        for m in (1, 2):
            row, text = 5, []
            for first_i, n in EMITS:
                text.append(H.fastq_text(rid, first_i, H.ROW_SWEEP_CPU, m, exp["bases"][row:row + n, m - 1], exp["qual"][row:row + n, m - 1]))
                row += n
            text = b"".join(text)
            assert paths[m - 1].read_bytes() == text
            assert text.count(b"\n") == 4 * 200 and len(text) == 200 * (len(rid) + 2 * RL + 11) + 6 * 1 + 90 * 2 + 104 * 3


@pytest.mark.parametrize("RL", H.ROW_SWEEP)
def test_the_oracle_alone_yields_the_mutation_rows_of_a_vcf_case(RL):
    (ids, seqs, counts), r1, r2, vcf, types = H.row_sweep_worker_files(H.row_sweep_model(RL), RL)
    assert len(ids) == 3 and counts[1] == 0 and sum(counts) == 200
    assert types.count(0) >= 1, "no substitution row"
    if RL >= 16:
        assert types.count(1) >= 1 and types.count(2) >= 1, "no insertion / deletion row"
    assert vcf.count("\n") == len(types) and r1.count(b"\n") == r2.count(b"\n") == 800
    first = vcf.split("\n")[0].split("\t")
    assert first[0].startswith("w%d.0_" % RL) and first[0].endswith("_%d/1" % H.ROW_SWEEP_CPU) and len(first) == 8


def test_export_tiles_that_start_at_different_alignments():
    """tile * 2 RL bytes lie between two tile starts.  With 64 pairs a tile (read lengths up to 191) that is a multiple of 128,
    and at 256 and 1024 a row itself is a multiple of 16 bytes: all tiles of a launch start at the buffer's own alignment there,
    and only the buffer's shift moves it.  250 (49 pairs) and 997 (12 pairs) are the read lengths of the sweep whose
    neighbouring tiles meet inside a 16-byte chunk at changing offsets."""
    tiles = {RL: H.export_tile_pairs(RL) for RL in H.ROW_SWEEP}
    assert tiles[997] == 12 and tiles[1024] == 11 and tiles[250] == 49 and tiles[256] == 47
    assert all(tiles[RL] == 64 for RL in H.ROW_SWEEP if RL <= 128)
    for RL in H.ROW_SWEEP:
        assert -(-200 // tiles[RL]) >= 4  # at least four tiles in 200 pairs
        for shift in (0, 1, 8, 15):
            starts = set(H.export_tile_alignments(RL, 200, shift))
            assert (len(starts) > 1) == (RL in (250, 997)), (RL, shift, starts)
    assert set(H.export_tile_alignments(997, 200, 1)) == {1, 9} and set(H.export_tile_alignments(250, 200, 0)) == {0, 4, 8, 12}
