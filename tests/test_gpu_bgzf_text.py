"""`generate --bgzip` on the device (iss_origins_compress / iss_vcf_compress, iss_bgzf_text.hip.h) against the host twin
tests/bgzf_text_twin.py, bit for bit.

Every case emits the same rows twice -- in mode 0 (text) and in mode 1 (the text's BGZF members).  The mode-1 bytes must be
members that inflate alone, with their CRC-32 and ISIZE and a BSIZE chain that ends at the file's end; inflated they must be
exactly the mode-0 bytes; and they must be the twin's bytes for that text.  The twin itself is held to the contract without a GPU
(tests/test_bgzf_text_host.py)."""
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import bgzf_text_twin as T
import helpers as H
from insilicoseq_amd import bgzf
from insilicoseq_amd import origins as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 32768
FRONT = b"in front\n"


def check_members(raw, text):
    pos, out = 0, []
    while pos < len(raw):
        assert raw[pos:pos + 4] == b"\x1f\x8b\x08\x04" and raw[pos + 10:pos + 16] == b"\x06\x00BC\x02\x00", pos
        size = struct.unpack_from("<H", raw, pos + 16)[0] + 1
        assert pos + size <= len(raw), "BSIZE leads past the end"
        d = zlib.decompressobj(-15)
        data = d.decompress(raw[pos + 18:pos + size - 8])
        assert d.eof and d.unused_data == b"", "the member's deflate stream does not end with the member"
        crc, isize = struct.unpack_from("<II", raw, pos + size - 8)
        assert crc == zlib.crc32(data) & 0xffffffff and isize == len(data)
        out.append(data)
        pos += size
    assert pos == len(raw) and b"".join(out) == text
    return out


def against_twin(got, texts):
    """`got`: what the device appended for the calls whose texts are `texts`, in order."""
    want = b"".join(T.members(t) for t in texts)
    print("%d calls, %d bytes of text: device %d bytes, twin %d" % (len(texts), sum(map(len, texts)), len(got), len(want)))
    check_members(got, b"".join(texts))
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("the device's members are not the twin's: %d bytes against %d, first difference at byte %d" % (len(got), len(want), k))


# ---------------------------------------------------------------------------------------------------- origins
class Rows(object):
    """One engine with generated rows on one record and their coordinates (left unchanged: every case's reference)."""

    def __init__(self, model, length, rows, seed, fragment=None):
        from insilicoseq_amd.engine import ReadEngine

        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(H.dense_model(model))
            self.RL, self.length, self.n = eng.read_length, length, rows
            self.gid = eng.add_genome(H.random_genome(900 + rows, length))
            if fragment is not None:
                eng.set_fragment(*fragment)
            eng.generate(self.gid, rows, first_ordinal=3, seed=seed)
            eng.synchronize()
            self.coords = eng.coords(0, rows).copy()
        except Exception:
            eng.close()
            raise


@pytest.fixture(scope="module")
def rows():
    made = {}

    def get(model="novaseq", length=20000, rows=2600, seed=77, fragment=None):
        key = (model, length, rows, seed, fragment)
        if key not in made:
            made[key] = Rows(model, length, rows, seed, fragment)
        return made[key]

    yield get
    for r in made.values():
        r.eng.close()


def call_text(r, call, cpu):
    items, lengths = call
    return G.lines_host(items, lengths, cpu, np.concatenate([r.coords[row:row + n] for _r, _i, row, n in items] +
                                                            [np.zeros((0, 4), dtype=np.int64)]), r.RL)


def emit_file(eng, calls, cpu, path, mode):
    """Some bytes in front, every call through origins_emit_batch in `mode`, ONE flush -> the appended bytes."""
    eng.origins_compress(bool(mode))
    try:
        with open(path, "wb") as fh:
            fh.write(FRONT)
            fh.flush()
            for items, lengths in calls:
                eng.origins_emit_batch(fh.fileno(), items, lengths, cpu)
            eng.origins_flush()
            assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(path)  # (the descriptor stands at the end)
    finally:
        eng.origins_flush()
        eng.origins_compress(False)
    data = open(path, "rb").read()
    assert data[:len(FRONT)] == FRONT
    return data[len(FRONT):]


def check_origins(r, calls, cpu, tmp_path):
    text = emit_file(r.eng, calls, cpu, str(tmp_path / "text.bedpe"), 0)
    texts = [call_text(r, c, cpu) for c in calls]
    assert text == b"".join(texts)  # (mode 0 is what it was: the formatter's twin)
    got = emit_file(r.eng, calls, cpu, str(tmp_path / "members.bedpe"), 1)
    against_twin(got, [t for t in texts if t])
    return texts, got


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_origins_shapes(rows, tmp_path, n):
    r = rows()
    texts, got = check_origins(r, [([("NZ_CP012345.1", 0, 5, n)], [r.length])], 2, tmp_path)
    assert texts[0].count(b"\n") == n and len(check_members(got, texts[0])) == 1


def _ends_on_a_block(r, most):
    """(first row, pairs, first pair id) of an item with a one-character id whose text has exactly 32 768 bytes, found with the
    formatter's twin: lines are about 45 bytes, so about one start in 45 ends a line on the boundary."""
    base = np.array([len(x) for x in call_text(r, ([("x", 0, 0, r.n)], [r.length]), 0).split(b"\n")[:-1]]) - np.array(
        [len(str(j)) for j in range(r.n)]) + 1  # a line's bytes without the digits of its pair number
    for first_i in (0, 7, 95, 990):
        digits = np.array([len(str(first_i + j)) for j in range(most)])
        for row in range(0, r.n - most):
            hit = np.nonzero(np.cumsum(base[row:row + most] + digits) == BLOCK)[0]
            if len(hit):
                return row, int(hit[0]) + 1, first_i
    raise AssertionError("no item of these rows ends on a block boundary")


def test_origins_one_block_exactly_and_three_blocks(rows, tmp_path):
    """A one-character id: about 900 pairs whose text ends exactly on the first block boundary, and about 2 000 pairs (three
    blocks, the last one short)."""
    r = rows()
    row, n, first_i = _ends_on_a_block(r, 1100)
    texts, got = check_origins(r, [([("x", first_i, row, n)], [r.length])], 0, tmp_path)
    assert len(texts[0]) == BLOCK and len(check_members(got, texts[0])) == 1 and 500 < n <= 1100
    texts, got = check_origins(r, [([("x", 0, 3, 2000)], [r.length])], 0, tmp_path)
    assert [len(m) for m in check_members(got, texts[0])][:-1] == [BLOCK, BLOCK] and 2 * BLOCK < len(texts[0]) < 3 * BLOCK
    # the copies pay: smaller than the runs-only code of the same text
    assert len(got) < T.size(texts[0], runs_only=True)


def test_origins_ids_and_record_lengths(rows, tmp_path):
    """A 200-character id; two items with different id lengths and record lengths (10 bp: every interval clamped to one or two
    digits; 10^9 nominal) in one call, so that the distances change in the middle of the text."""
    r = rows()
    check_origins(r, [([("c" * 200, 0, 0, 300)], [r.length])], 3, tmp_path)
    texts, _ = check_origins(r, [([("ab", 99990, 0, 400), ("a_much_longer_record_id.1", 5, 400, 400)], [10, 10 ** 9])], 12, tmp_path)
    lens = set(len(x) for x in texts[0].split(b"\n")[:-1])
    assert len(lens) > 6


def test_origins_custom_fragments(rows, tmp_path):
    """Fragments of 300 +- 200 on 700 bases: clamped intervals of every width."""
    r = rows(length=700, rows=333, seed=1234, fragment=(300, 200))
    texts, _ = check_origins(r, [([("frag", 0, 0, 333)], [700])], 0, tmp_path)
    p = [x.split(b"\t") for x in texts[0].split(b"\n")[:-1]]
    assert len(set(int(f[5]) - int(f[4]) for f in p)) > 5


def test_origins_calls_without_a_flush(rows, tmp_path):
    """More calls than slots, a call of no pairs in between: every call is compressed on its own (its first line has no candidate
    and its code is its own), the file holds the calls' members in order."""
    r = rows()
    ln = [r.length]
    calls = [([("first", 0, 0, 900)], ln), ([("second", 998, 900, 3)], ln), ([("none", 0, 0, 0)], ln), ([], []),
             ([("third", 50, 903, 1200)], ln), ([("4", 0, 2103, 40)], ln)]
    check_origins(r, calls, 2, tmp_path)


def test_origins_buffers_grow_mid_run(tmp_path):
    """One pair, then a call far past what the first one allocated, then a small one, no flush in between (an engine of its own:
    its buffers are the first call's)."""
    r = Rows("novaseq", 20000, 1500, 78)
    try:
        ln = [r.length]
        calls = [([("one", 0, 0, 1)], ln), ([("L" * 300, 7, 1, 1400)], ln), ([("small", 0, 1401, 20)], ln)]
        # mode 1 first: the text's and the stage's buffers are allocated by the one-pair call and replaced by the second
        got = emit_file(r.eng, calls, 2, str(tmp_path / "m.bedpe"), 1)
        text = emit_file(r.eng, calls, 2, str(tmp_path / "t.bedpe"), 0)
        assert len(text) > 1_000_000  # (far more than bound + bound / 8 + 64 KiB of the first call)
        check_members(got, text)
        ms = bgzf.members_of(got)
        assert len(ms) == 1 + (len(call_text(r, calls[1], 2)) + BLOCK - 1) // BLOCK + 1
        # the twin on the two small calls (the large one is checked through its members: a megabyte is slow in plain Python)
        assert got.startswith(T.members(call_text(r, calls[0], 2))) and got.endswith(T.members(call_text(r, calls[2], 2)))
    finally:
        r.eng.close()


def test_origins_tile_does_not_matter(rows, tmp_path, monkeypatch):
    r = rows()
    call = ([("x" * 17, 95, 7, 700)], [r.length])
    monkeypatch.setenv("ISS_ORIGINS_TILE", "1")
    _texts, one = check_origins(r, [call], 3, tmp_path)
    monkeypatch.delenv("ISS_ORIGINS_TILE")
    _texts, default = check_origins(r, [call], 3, tmp_path)
    assert one == default


# ---------------------------------------------------------------------------------------------------- VCF
def vcf_both_modes(eng, items, cpu, source, tmp_path):
    """The rows of the last generate call through vcf_emit in mode 0 and in mode 1 -> (text, members)."""
    out = []
    for mode in (0, 1):
        eng.vcf_compress(bool(mode))
        path = str(tmp_path / ("mode%d.vcf" % mode))
        try:
            with open(path, "wb") as fh:
                fh.write(FRONT)
                fh.flush()
                eng.vcf_emit(fh.fileno(), items, cpu, source=source)
                eng.vcf_flush()
                assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(path)
        finally:
            eng.vcf_flush()
            eng.vcf_compress(False)
        data = open(path, "rb").read()
        assert data[:len(FRONT)] == FRONT
        out.append(data[len(FRONT):])
    return out


@pytest.fixture(scope="module")
def vcf_engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    eng.load_model(H.dense_model("novaseq", (0.01, 0.03)))  # (the indel-heavy model of tests/test_gpu_vcf.py)
    gid = eng.add_genome(H.mixed_genome(304, 20000))
    eng.mutations_reserve(2_000_000)
    eng.mt_mutations_reserve(400_000)
    yield eng, gid
    eng.close()


@pytest.mark.parametrize("source", ["philox", "mt"])
@pytest.mark.parametrize("n", [8, 220])
def test_vcf_rows(vcf_engine, tmp_path, source, n):
    """A handful of rows, and enough of them for three blocks or more."""
    eng, gid = vcf_engine
    if source == "philox":
        eng.generate(gid, n, first_ordinal=11, seed=6)
    else:
        eng.seed_mt(77)
        assert eng.generate_mt(gid, n) == n
    text, got = vcf_both_modes(eng, [("rec.%d" % n, 99_990, 0, n)], 12, source, tmp_path)
    assert text.count(b"\n") > 5 and text.endswith(b"\t\t\n")
    against_twin(got, [text])
    if n > 100:
        assert len(text) > 2 * BLOCK and len(bgzf.members_of(got)) >= 3


def test_vcf_no_rows_append_nothing(tmp_path):
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.model import DenseModel

    with ReadEngine(0) as eng:
        eng.load_model(DenseModel.perfect())
        gid = eng.add_genome(H.random_genome(360, 30000))
        eng.mutations_reserve(1_000_000)
        eng.generate(gid, 5000, first_ordinal=0, seed=1)
        text, got = vcf_both_modes(eng, [("p", 0, 0, 5000)], 0, "philox", tmp_path)
        assert text == b"" and got == b""


# ---------------------------------------------------------------------------------------------------- errors
def test_mode_switch_needs_a_flush(rows, tmp_path):
    from insilicoseq_amd._native import E_INVALID, EngineError

    r = rows()
    with open(tmp_path / "a.bedpe", "wb") as fh:
        r.eng.origins_emit_batch(fh.fileno(), [("a", 0, 0, 50)], [r.length], 0)
        with pytest.raises(EngineError) as e:
            r.eng.origins_compress(True)
        assert e.value.code == E_INVALID
        r.eng.origins_compress(False)  # (the mode it has: nothing to switch)
        r.eng.origins_flush()
        r.eng.origins_compress(True)
        r.eng.origins_compress(False)
    assert open(tmp_path / "a.bedpe", "rb").read() == call_text(r, ([("a", 0, 0, 50)], [r.length]), 0)


def test_vcf_mode_switch_and_the_worker_set(vcf_engine, tmp_path):
    from insilicoseq_amd._native import E_INVALID, EngineError

    eng, gid = vcf_engine
    eng.generate(gid, 50, first_ordinal=0, seed=2)
    path = tmp_path / "w.vcf"
    with open(path, "wb") as fh:
        fh.write(b"untouched")
        fh.flush()
        eng.vcf_compress(True)
        try:
            with pytest.raises(EngineError) as e:
                eng.vcf_emit_workers([(fh.fileno(), "w", 0, 0, 50, 0)])
            assert e.value.code == E_INVALID and "iss_vcf_compress" in e.value.message
            eng.vcf_emit(fh.fileno(), [("w", 0, 0, 50)], 0)
            with pytest.raises(EngineError) as e:
                eng.vcf_compress(False)  # (a job was queued: flush first)
            assert e.value.code == E_INVALID
        finally:
            eng.vcf_flush()
            eng.vcf_compress(False)
    data = path.read_bytes()
    assert data.startswith(b"untouched") and len(check_members(data[9:], bgzf.members_of(data[9:])[0][2])) == 1


def test_a_write_error_surfaces_once(rows, tmp_path):
    """A descriptor opened read-only: the next flush raises E_IO "write failed ...", the one after returns, the file is as it was
    and the next emit appends the twin's bytes."""
    from insilicoseq_amd._native import E_IO, EngineError

    r = rows()
    call = ([("rec", 3, 10, 120)], [r.length])
    path = tmp_path / "readonly.bedpe"
    path.write_bytes(b"read only\n")
    r.eng.origins_compress(True)
    try:
        with open(path, "rb") as fh:
            r.eng.origins_emit_batch(fh.fileno(), call[0], call[1], 0)
            with pytest.raises(EngineError) as e:
                r.eng.origins_flush()
            assert e.value.code == E_IO and e.value.message.startswith("write failed"), e.value.message
            r.eng.origins_flush()
    finally:
        r.eng.origins_flush()
        r.eng.origins_compress(False)
    assert path.read_bytes() == b"read only\n"
    check_origins(r, [call], 0, tmp_path)


# ---------------------------------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("workers", [("--gpus", "1"), ("--gpus", "2", "--devices", "1")], ids=["one_worker", "two_workers_one_device"])
def test_cli(tmp_path, workers):
    """`generate --origins --store_mutations` with and without --bgzip (Philox mode): the .bedpe.gz parses and inflates to the
    .bedpe, the .vcf.gz inflates to the .vcf, the FASTQ files are the same, both BGZF files end with the EOF block."""
    outs = {}
    for flag in ("plain", "bgzip"):
        d = tmp_path / flag
        d.mkdir()
        subprocess.check_call([sys.executable, "-m", "insilicoseq_amd", "generate", "--genomes", os.path.join(H.GOLDEN, "genomes.fasta"),
                               "--model", "novaseq", "-n", "3000", "--seed", "42", "--store_mutations", "--origins", "-o", str(d / "run"),
                               "--quiet"] + list(workers) + (["--bgzip"] if flag == "bgzip" else []), cwd=ROOT, timeout=90)
        outs[flag] = str(d / "run")
        assert not [f for f in os.listdir(str(d)) if ".iss.tmp." in f]
    made = sorted(os.listdir(str(tmp_path / "bgzip")))
    assert "run.vcf.gz" in made and "run_origins.bedpe.gz" in made and "run.vcf" not in made and "run_origins.bedpe" not in made
    for suffix in ("_R1.fastq", "_R2.fastq"):
        assert open(outs["bgzip"] + suffix, "rb").read() == open(outs["plain"] + suffix, "rb").read()
    vcf = open(outs["plain"] + ".vcf", "rb").read()
    assert bgzf.read(outs["bgzip"] + ".vcf.gz") == vcf and vcf.count(b"\n") > 10
    assert gzip.open(outs["bgzip"] + ".vcf.gz", "rb").read() == vcf
    assert bgzf.read(outs["bgzip"] + G.SUFFIX + ".gz") == open(outs["plain"] + G.SUFFIX, "rb").read()
    p, q = G.parse(outs["bgzip"] + G.SUFFIX + ".gz"), G.parse(outs["plain"] + G.SUFFIX)
    assert p["name"].tolist() == q["name"].tolist() and len(p["name"]) > 500 and np.array_equal(p["s1"], q["s1"])
    for suffix in (".vcf.gz", G.SUFFIX + ".gz"):
        assert open(outs["bgzip"] + suffix, "rb").read()[-28:] == bgzf.EOF_BLOCK
