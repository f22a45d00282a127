"""The parts of the tensor route that need no GPU: the ABI entry, the numpy twin of k_rows_export (row layout, recode table,
coordinates from descriptors), the cutting of a work list into batches, multinomial_work."""
import os
import re

import numpy as np
import pytest

from insilicoseq_amd import _native
from insilicoseq_amd import tensors as T
from insilicoseq_amd.engine import ReadEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_names_the_export_entry():
    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    assert "#define ISS_ABI_VERSION 8" in header
    assert re.search(r"\bint iss_output_export\(iss_ctx \*ctx, int64_t first_pair, int64_t n_pairs, int32_t encoding,\s*"
                     r"void \*d_bases, void \*d_qual,\s*int64_t \*d_coords, int32_t \*d_item\);", header)
    assert "#define ISS_EXPORT_ASCII 0" in header and "#define ISS_EXPORT_CODES 1" in header
    assert "iss_output_export" in _native.EXPORTS
    assert _native.EXPORT_ENCODINGS == {"ascii": 0, "codes": 1}
    assert callable(ReadEngine.export)


def test_package_does_not_import_torch_by_itself():
    import subprocess
    import sys

    code = "import sys, insilicoseq_amd, insilicoseq_amd.tensors; sys.exit(1 if 'torch' in sys.modules else 0)"
    assert subprocess.call([sys.executable, "-c", code], cwd=ROOT) == 0


def _header_formula(i, p, k, row):
    # include/iss_mi355x.h, iss_output_reserve, written out once more with plain integers
    return i * row + 128 * (p // 32) + 64 * (k // 2) + 16 * ((p // 8) % 4) + 8 * (k % 2) + p % 8


@pytest.mark.parametrize("read_length", [1, 8, 125, 151, 301])
def test_numpy_twin_follows_the_row_layout(read_length):
    RL = read_length
    pitch = T.pitch_of(RL)
    row = T.row_bytes(pitch)
    assert pitch == 8 * -(-RL // 8) and row == 128 * -(-pitch // 32)
    n = 5
    rng = np.random.RandomState(RL)
    arrays = rng.randint(0, 256, size=(4, n, RL)).astype(np.uint8)
    rows = np.full((n, row), 0xEE, dtype=np.uint8)  # (padding bytes the export must not pick up)
    flat = rows.reshape(-1)
    seen = set()
    for k in range(4):
        for i in range(n):
            for p in range(RL):
                at = _header_formula(i, p, k, row)
                assert i * row <= at < (i + 1) * row and at not in seen
                seen.add(at)
                flat[at] = arrays[k, i, p]
    bases, qual = T.export_rows_host(rows, RL, "ascii")
    assert bases.shape == qual.shape == (n, 2, RL) and bases.dtype == np.uint8
    assert np.array_equal(bases[:, 0], arrays[0]) and np.array_equal(qual[:, 0], arrays[1])
    assert np.array_equal(bases[:, 1], arrays[2]) and np.array_equal(qual[:, 1], arrays[3])
    codes, qual2 = T.export_rows_host(rows, RL, "codes")
    assert np.array_equal(qual2, qual) and np.array_equal(codes, T.recode(bases))
    with pytest.raises(ValueError):
        T.export_rows_host(rows, RL, "2bit")


def test_recode_table():
    expect = np.full(256, 4, dtype=np.uint8)
    for code, letters in enumerate(("Aa", "Cc", "Gg", "Tt")):  # alphabetical, not the engine's A, T, C, G
        for c in letters:
            expect[ord(c)] = code
    assert np.array_equal(T.recode(np.arange(256, dtype=np.uint8)), expect)
    assert T.recode(np.frombuffer(b"ACGTacgtNnRYU-", dtype=np.uint8)).tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4, 4, 4, 4]


def test_coordinates_from_descriptors():
    RL = 151
    fs = np.array([10, 2**33 + 5, 100, -3], dtype=np.int64)      # (a custom fragment length can make a coordinate negative)
    re_ = np.array([400, 2**33 + 700, 90, 250], dtype=np.int64)
    off = np.array([0, 0, 64, 0], dtype=np.int64)                # record coordinates = arena coordinates - the item's offset
    isz = np.array([390, 695, -10, 253], dtype=np.int32)
    meta = (((fs + off) >> 32) & 15) << 8 | (((re_ + off) >> 32) & 15) << 12 | 0x5  # low bits: bin slots, ignored here
    lo = lambda v: ((v + off) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    got = T.coords_from_descriptors(lo(fs), lo(re_), meta.astype(np.uint32), isz, RL, arena_off=off)
    assert got.dtype == np.int64 and got.shape == (4, 4)
    assert np.array_equal(got, np.stack([fs, re_ - RL, re_, isz.astype(np.int64)], axis=1))


def _flatten(batches):
    """(item, ordinal) of every pair, batch after batch."""
    out = []
    for first_ordinal, first_item, counts in batches:
        o = first_ordinal
        for j, c in enumerate(counts):
            out += [(first_item + j, o + t) for t in range(c)]
            o += c
    return out


@pytest.mark.parametrize("counts", [[5, 0, 130], [0, 0, 7, 0], [1], [64, 64, 64], [3, 1000, 2], [0], []])
@pytest.mark.parametrize("batch_pairs", [1, 2, 64, 65, 333, 10**6])
def test_cut_batches(counts, batch_pairs):
    batches = T.cut_batches(counts, batch_pairs)
    total = sum(counts)
    # every pair once, in the order and with the ordinal one call over the whole list gives it
    expect = [(k, None) for k, c in enumerate(counts) for _ in range(c)]
    got = _flatten(batches)
    assert [k for k, _ in got] == [k for k, _ in expect]
    assert [o for _, o in got] == list(range(total))
    sizes = [sum(c) for _, _, c in batches]
    assert sum(sizes) == total and all(s == batch_pairs for s in sizes[:-1]) and all(0 < s <= batch_pairs for s in sizes)
    assert len(batches) == -(-total // batch_pairs)
    for first_ordinal, first_item, c in batches:
        assert first_item + len(c) <= len(counts) and c[0] > 0 and all(x >= 0 for x in c)
        assert all(x <= counts[first_item + j] for j, x in enumerate(c))


def test_cut_batches_rejects_nonsense():
    with pytest.raises(ValueError):
        T.cut_batches([1, 2], 0)
    with pytest.raises(ValueError):
        T.cut_batches([1, -2], 4)


def test_multinomial_work():
    shares = [0.5, 0.25, 0.0, 0.25]
    a = T.multinomial_work(shares, 1000, seed=11)
    assert a == T.multinomial_work(shares, 1000, seed=11)
    assert a != T.multinomial_work(shares, 1000, seed=12)
    assert [k for k, _ in a] == [0, 1, 2, 3] and sum(n for _, n in a) == 1000 and a[2][1] == 0
    assert all(isinstance(n, int) and n >= 0 for _, n in a)
    rng = np.random.Generator(np.random.Philox(11))
    assert [n for _, n in a] == rng.multinomial(1000, np.asarray(shares) / sum(shares)).tolist()
    assert sum(n for _, n in T.multinomial_work([3, 1], 0, seed=1)) == 0
    with pytest.raises(ValueError):
        T.multinomial_work([], 10, seed=1)
    with pytest.raises(ValueError):
        T.multinomial_work([0.0, 0.0], 10, seed=1)
