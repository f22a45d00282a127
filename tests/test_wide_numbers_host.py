"""Pair ids beyond 32 bits without a GPU: the plain references of tests/wide_numbers.py against literal bytes, and the three host
formatters the GPU tests trust (iss_fastq_write, iss_ubam_host_records, iss_origins_host_text) against those references on every item
of WIDE_ITEMS -- the item across x* included, where the character count of all smaller ids (iss::digits_before) passes 2^64."""
import os
import struct

import numpy as np
import pytest

import ubam_twin as U
import wide_numbers as W

RL, N_ROWS = 21, 40  # (an odd read length: the half-filled last nibble of a BAM record)


@pytest.fixture(scope="module")
def rows():
    return W.synthetic_rows(N_ROWS, RL, 9)


@pytest.fixture(scope="module")
def native():
    from insilicoseq_amd import _native

    return _native


def test_cases_hold_their_boundaries():
    assert W.chars_before(0) == 0 and W.chars_before(1) == 1 and W.chars_before(10) == 10 and W.chars_before(11) == 12
    assert W.chars_before(1000) == len("".join(str(k) for k in range(1000)))
    assert W.chars_before(W.X_STAR - 1) < 2 ** 64 <= W.chars_before(W.X_STAR) and 1.02e18 < W.X_STAR < 1.04e18
    assert len(W.WIDE_ITEMS) == 8 and W.WIDE_ROWS <= 200 and max(n for _, n in W.WIDE_ITEMS) <= N_ROWS
    for (a, n), (lo, hi) in zip(W.WIDE_ITEMS, [(10 ** 9 - 1, 10 ** 9), (2 ** 31 - 1, 2 ** 31), (2 ** 32 - 1, 2 ** 32), (10 ** 10 - 1, 10 ** 10),
                                                 (10 ** 15 - 1, 10 ** 15), (10 ** 18 - 1, 10 ** 18), (W.X_STAR - 1, W.X_STAR)]):
        assert a <= lo and hi < a + n, (a, n)
    assert W.WIDE_ITEMS[-1][0] + W.WIDE_ITEMS[-1][1] == 2 ** 63 - 1
    assert [len(str(c)) for c in W.WIDE_CPUS] == [1, 1, 10]


def test_references_against_literal_bytes():
    """Three hand-written ids: 4294967296 (2^32), 10000000000 (the first of eleven digits) and 9223372036854775806 (2^63 - 2)."""
    b = np.frombuffer(b"ACgTN", dtype=np.uint8).reshape(1, 5)
    q = np.asarray([[0, 1, 40, 41, 9]], dtype=np.uint8)
    assert W.fastq_text("g", 4294967296, 7, b, q, 1) == b"@g_4294967296_7/1\nACgTN\n+\n!\"IJ*\n"
    assert W.fastq_text(b"chr|1", 10000000000, 2147483647, b, q, 2) == b"@chr|1_10000000000_2147483647/2\nACgTN\n+\n!\"IJ*\n"
    two = W.fastq_text("g", 9223372036854775805, 0, np.repeat(b, 2, axis=0), np.repeat(q, 2, axis=0), 1)
    assert two == b"@g_9223372036854775805_0/1\nACgTN\n+\n!\"IJ*\n@g_9223372036854775806_0/1\nACgTN\n+\n!\"IJ*\n"
    rows = np.zeros(4, dtype=[("pair", "<i4"), ("mate", "i1"), ("type", "i1"), ("position", "<i2"), ("ref", "u1"), ("alt", "u1"), ("quality", "<i2")])
    rows[0] = (3, 0, 0, 0, ord("A"), ord("T"), 37)    # substitution
    rows[1] = (3, 1, 1, 150, ord("C"), ord("G"), 0)   # insertion: alt = ref + letter, no phred
    rows[2] = (4, 0, 2, 9, ord("G"), ord("."), 0)     # deletion
    rows[3] = (9, 1, 0, 5, ord("t"), ord("T"), 2)     # outside the item below
    assert W.vcf_lines("g", 4294967296, 7, rows[:3], pair0=3) == [
        "g_4294967296_7/1\t1\t.\tA\tT\t37\t\t\n", "g_4294967296_7/2\t151\t.\tC\tCG\t.\t\t\n", "g_4294967297_7/1\t10\t.\tG\t.\t.\t\t\n"]
    assert W.vcf_items_text([("a", 10000000000 - 1, 13, 2), ("b", 9223372036854775806 - 6, 15, 7)], 2147483647, rows, row0=10) == (
        b"a_9999999999_2147483647/1\t1\t.\tA\tT\t37\t\t\na_9999999999_2147483647/2\t151\t.\tC\tCG\t.\t\t\n"
        b"a_10000000000_2147483647/1\t10\t.\tG\t.\t.\t\t\nb_9223372036854775804_2147483647/2\t6\t.\tt\tT\t2\t\t\n")
    # a BAM record: block_size and l_read_name by hand (36 fixed bytes - 4, name + NUL, ceil(5 / 2) nibble bytes, 5 phreds)
    rec = W.ubam_records([("g", 10000000000, 0, 1)], 7, b, q, b, q)
    name = b"g_10000000000_7\0"
    assert struct.unpack_from("<i", rec, 0)[0] == 32 + len(name) + 3 + 5 and rec[12] == len(name) and rec[36:36 + len(name)] == name
    assert rec[36 + len(name):36 + len(name) + 3] == bytes([0x12, 0x48, 0xf0]) and len(rec) == 2 * (36 + len(name) + 8)
    coords = np.asarray([[4294967296, 4294967500, 4294967505, 199]], dtype=np.int64)
    assert W.bedpe_text([("g", 9223372036854775806, 0, 1)], [2 ** 34 - 4096], 7, coords, 5) == \
        b"g\t4294967296\t4294967301\tg\t4294967500\t4294967505\tg_9223372036854775806_7\t.\t+\t-\t199\n"


def _pitched(rows, pitch):
    wide = [np.zeros((len(r), pitch), dtype=np.uint8) for r in rows]
    for w, r in zip(wide, rows):
        w[:, :r.shape[1]] = r
    return wide


@pytest.mark.parametrize("cpu", W.WIDE_CPUS)
@pytest.mark.parametrize("k", range(len(W.WIDE_ITEMS)))
def test_host_formatters_equal_the_references(native, rows, tmp_path, k, cpu):
    """Every item, both id lengths: FASTQ, BAM records and BEDPE of the host formatters, byte for byte; the files' sizes are the
    references' sizes (per item, and summed: the closed form chars_before gives for FASTQ and BAM)."""
    first_i, n = W.WIDE_ITEMS[k]
    pitch = 24
    wide = _pitched([r[:n] for r in rows], pitch)
    coords = np.stack([np.arange(n) * 4294967311 % (2 ** 34 - 5000), np.arange(n) * 977 + 2 ** 32 - 50, np.arange(n) * 977 + 2 ** 32 - 50 + RL,
                       np.arange(n) - 7], axis=1).astype(np.int64)
    rec_len = 2 ** 34 - 4096
    for rid in W.WIDE_IDS:
        paths = [str(tmp_path / ("%d_%s" % (len(rid), s))) for s in ("1.fq", "2.fq", "u.bam", "o.bedpe")]
        fh = [open(p, "wb") for p in paths]
        try:
            L = native.lib()
            assert L.iss_fastq_write(fh[0].fileno(), fh[1].fileno(), rid.encode(), first_i, cpu, n, RL, pitch, *[w.ctypes.data for w in wide], 2) == 0
            assert L.iss_ubam_host_records(fh[2].fileno(), rid.encode(), first_i, cpu, n, RL, pitch, *[w.ctypes.data for w in wide]) == 0
            assert L.iss_origins_host_text(fh[3].fileno(), rid.encode(), first_i, cpu, n, RL, rec_len, coords.ctypes.data) == 0
        finally:
            for f in fh:
                f.close()
        got = [open(p, "rb").read() for p in paths]
        want = [W.fastq_text(rid, first_i, cpu, rows[0][:n], rows[1][:n], 1), W.fastq_text(rid, first_i, cpu, rows[2][:n], rows[3][:n], 2),
                W.ubam_records([(rid, first_i, 0, n)], cpu, *rows), W.bedpe_text([(rid, first_i, 0, n)], [rec_len], cpu, coords, RL)]
        for g, w, p in zip(got, want, paths):
            assert len(g) == len(w) == os.path.getsize(p), (p, len(g), len(w))
            assert g == w, (p, next(i for i, (x, y) in enumerate(zip(g, w)) if x != y))
        # the sizes in closed form: pairs * constant + the characters of the ids (the difference that stays right mod 2^64)
        id_chars = W.chars_before(first_i + n) - W.chars_before(first_i)
        assert id_chars == sum(len(str(first_i + j)) for j in range(n))
        assert len(got[0]) == n * (len(rid) + len(str(cpu)) + 2 * RL + 10) + id_chars
        assert len(got[2]) == 2 * (n * U.record_length(rid, 0, cpu, RL) - n + id_chars)
        names = [r[0] for r in U.parse_records(got[2])]
        assert names[0] == names[1] == b"%s_%d_%d" % (rid.encode(), first_i, cpu) and names[-1] == b"%s_%d_%d" % (rid.encode(), first_i + n - 1, cpu)


def test_host_formatters_refuse_a_negative_first_id(native, rows, tmp_path):
    wide = _pitched([r[:2] for r in rows], RL)
    coords = np.zeros((2, 4), dtype=np.int64)
    with open(tmp_path / "t", "wb") as fh:
        L = native.lib()
        for first_i in (-1, -2 ** 63):
            assert L.iss_fastq_write(fh.fileno(), fh.fileno(), b"r", first_i, 0, 2, RL, RL, *[w.ctypes.data for w in wide], 1) == native.E_INVALID
            assert L.iss_ubam_host_records(fh.fileno(), b"r", first_i, 0, 2, RL, RL, *[w.ctypes.data for w in wide]) == native.E_INVALID
            assert L.iss_origins_host_text(fh.fileno(), b"r", first_i, 0, 2, RL, 1000, coords.ctypes.data) == native.E_INVALID
    assert os.path.getsize(tmp_path / "t") == 0
