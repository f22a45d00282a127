"""Unaligned BAM built on the device (iss_ubam_emit_batch, `generate --ubam`) against the host twin (tests/ubam_twin.py).

The bytes a call appends must be ubam_twin.members(ubam_twin.records(rows of iss_output_download), dist) bit for bit -- the
record layout, the call's one Huffman code, the tokens of the member rule, every member's frame, CRC-32 and ISIZE -- and the
framed file must come back through insilicoseq_amd.bam.BamReader record for record.  The twin's own shape (every member inflates
alone, the size cap) is asserted without a GPU in tests/test_ubam_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import helpers as H
import ubam_twin as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {20: "ecoli", 125: "basic", 126: "hiseq", 301: "miseq"}
ROWS = 400  # rows generated per read length (the largest case takes 333)


class Rows(object):
    """One engine with ``rows`` rows of the shipped model at RL over a lower-case / IUPAC genome, and their downloaded arrays (left
    unchanged: every case's reference)."""

    def __init__(self, RL, rows=ROWS):
        from insilicoseq_amd.engine import ReadEngine

        self.RL = RL
        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(H.dense_model(MODELS[RL]))
            assert eng.read_length == RL
            self.gid = eng.add_genome(H.mixed_genome(700 + RL, 20000))
            eng.generate(self.gid, rows, first_ordinal=3, seed=77)
            eng.synchronize()
            d = eng.download(0, rows)
            self.rows = [d[k].copy() for k in ("r1_base", "r1_qual", "r2_base", "r2_qual")]
        except Exception:
            eng.close()
            raise


@pytest.fixture(scope="module")
def rows():
    made = {}

    def get(RL):
        if RL not in made:
            made[RL] = Rows(RL)
        return made[RL]

    yield get
    for r in made.values():
        r.eng.close()


@pytest.fixture(scope="module")
def native():
    from insilicoseq_amd import _native

    return _native


def emit_file(r, calls, cpu, path, between=None):
    """header, every call's items through ReadEngine.ubam_emit_batch, one flush, the EOF block -> the record blocks' bytes.
    between(k): called behind emit call k, before the flush."""
    from insilicoseq_amd import ubam

    head = ubam.header_block()
    with open(path, "wb") as fh:
        fh.write(head)
        fh.flush()
        for k, items in enumerate(calls):
            r.eng.ubam_emit_batch(fh.fileno(), items, cpu)
            if between:
                between(k)
        r.eng.ubam_flush()
        assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(path)  # (the descriptor stands at the end)
        fh.seek(0, os.SEEK_END)
        fh.write(ubam.EOF_BLOCK)
    data = open(path, "rb").read()
    assert data[:len(head)] == head and data[-28:] == ubam.EOF_BLOCK
    return data[len(head):-28]


def check(r, native, calls, cpu, path, between=None):
    from insilicoseq_amd import bam

    got = emit_file(r, calls, cpu, path, between)
    texts = [U.records(items, cpu, *r.rows) for items in calls]
    want = b"".join(U.members(native, t, U.record_distance(items, r.RL, cpu)) for items, t in zip(calls, texts))
    print("RL %d, %d calls: %d record bytes, device %d bytes, twin %d" % (r.RL, len(calls), sum(map(len, texts)), len(got), len(want)))
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        try:
            same = b"".join(U.inflate_member(m) for m in U.split_members(got)) == b"".join(texts)
            what = "inflates to the records" if same else "inflates to OTHER bytes"
        except Exception as e:  # noqa: BLE001  (what zlib says belongs in the message)
            what = "does not inflate (%s)" % e
        raise AssertionError("the device's stream %s, but is not the twin's: %d bytes against %d, first difference at byte %d: %r "
                             "against %r" % (what, len(got), len(want), k, got[k:k + 24], want[k:k + 24]))
    # back through the project's reader, record for record against the rows
    reader = bam.BamReader(str(path))
    data = b"".join(c.data.tobytes() for c in reader.chunks())
    parsed = U.parse_records(data)
    j = 0
    for items in calls:
        for rid, first_i, row, n in items:
            for k in range(n):
                for mate in (0, 1):
                    name, flag, bases, qual = parsed[j]
                    j += 1
                    assert name == b"%s_%d_%d" % (U.T.as_bytes(rid), first_i + k, cpu) and flag == (141 if mate else 77)
                    assert bases == r.rows[2 * mate][row + k].tobytes().upper().translate(NOT_IUPAC_TO_N)
                    assert np.array_equal(qual, r.rows[2 * mate + 1][row + k])
    assert j == len(parsed)
    return got


NOT_IUPAC_TO_N = bytes(c if chr(c) in U.IUPAC else ord("N") for c in range(256))


@pytest.mark.parametrize("RL", sorted(MODELS))
@pytest.mark.parametrize("n", [1, 2, 333])
def test_shapes(rows, native, tmp_path, RL, n):
    """1 and 2 pairs (less than one block), 333 pairs (several blocks with a short last one; RL 125: the half-filled last nibble)."""
    check(rows(RL), native, [[("NZ_CP012345.1", 0, 5, n)]], 2, tmp_path / "shape.bam")


@pytest.mark.parametrize("cpu", [0, 123])
def test_items(rows, native, tmp_path, cpu):
    """Several items in one call: ids of 1, 17 and 200 characters, a zero-pair item between two others, pair numbers whose digit
    count changes inside the item."""
    calls = [[("a", 0, 0, 3), ("b" * 17, 7, 3, 5), ("zero", 4, 8, 0), ("c" * 200, 95, 8, 10)]]
    check(rows(126), native, calls, cpu, tmp_path / "items.bam")


def test_letters(rows, native, tmp_path):
    """The rows hold lower-case and IUPAC letters; the records hold their capitals' codes."""
    r = rows(125)
    seen = set(np.unique(np.concatenate([r.rows[0][:40].ravel(), r.rows[2][:40].ravel()])).tolist())
    assert seen & set(b"acgt") and seen & set(b"RYWSMKHBVDN") and seen & set(b"rywsmkhbvdn")
    got = check(r, native, [[("letters", 0, 0, 40)]], 0, tmp_path / "letters.bam")
    data = b"".join(U.inflate_member(m) for m in U.split_members(got))
    for j, (_name, _flag, bases, _qual) in enumerate(U.parse_records(data)):
        assert bases == r.rows[2 * (j & 1)][j >> 1].tobytes().upper() and bases.isupper()
    # the codes at their place in the first record: first base in the high nibble, the low nibble past the odd length 0
    packed, first = np.frombuffer(data, dtype=np.uint8), U.base_codes(r.rows[0][0])
    at = 36 + len(b"letters_0_0") + 1
    assert packed[at] == (first[0] << 4 | first[1]) and packed[at + 62] == (first[124] << 4)


def test_name_limit(rows, native, tmp_path):
    """A 254-character name is accepted; 255 characters: ISS_E_INVALID naming the record id, the file unchanged."""
    from insilicoseq_amd._native import E_INVALID, EngineError

    r = rows(20)
    ok = "k" * (254 - len("_9_3"))
    got = check(r, native, [[(ok, 8, 0, 2)]], 3, tmp_path / "ok.bam")
    assert got
    path = tmp_path / "long.bam"
    with open(path, "wb") as fh:
        fh.write(b"untouched")
        fh.flush()
        with pytest.raises(EngineError) as e:
            r.eng.ubam_emit_batch(fh.fileno(), [("fine", 0, 0, 2), (ok, 9, 2, 2)], 3)  # (pair 10: one digit more)
        assert e.value.code == E_INVALID and ok[:40] in e.value.message
        r.eng.ubam_flush()
    assert open(path, "rb").read() == b"untouched"


def test_slot_reuse(rows, native, tmp_path):
    """Emit calls back to back (more than the two slots), then one flush."""
    calls = [[("first", 0, 0, 150)], [("second_of_four", 998, 150, 3)], [("third", 50, 153, 120)], [("4", 0, 273, 40)]]
    check(rows(126), native, calls, 2, tmp_path / "slots.bam")


def test_generation_behind_an_emit(rows, native, tmp_path):
    """The rows are generated anew right behind an emit: the blocks hold the rows as they were when the call was made."""
    r = rows(301)

    def regenerate(k):
        r.eng.generate(r.gid, ROWS, first_ordinal=3, seed=78 + k)  # (other rows; no wait on the host)

    try:
        check(r, native, [[("before", 0, 0, 200)]], 1, tmp_path / "behind.bam", between=regenerate)
    finally:
        r.eng.generate(r.gid, ROWS, first_ordinal=3, seed=77)  # the module's rows again
        r.eng.synchronize()
        d = r.eng.download(0, ROWS)
        for have, k in zip(r.rows, ("r1_base", "r1_qual", "r2_base", "r2_qual")):
            assert np.array_equal(have, d[k])


def test_buffers_grow_mid_run(native, tmp_path):
    """One pair, then a call whose record bytes are past what the first one allocated (bytes + bytes / 8 + 1 MiB), then a small
    one; no flush in between, the file stays attached while the record, member and block buffers are replaced."""
    r = Rows(301, rows=800)  # (an engine no other case has emitted from: its buffers are the first call's)
    try:
        calls = [[("one", 0, 0, 1)], [("L" * 240, 7, 1, 760)], [("small", 0, 761, 20)]]
        size = [sum(U.record_length(rid, first_i + k, 2, 301) for rid, first_i, _row, n in items for k in range(n)) * 2 for items in calls]
        allocated = size[0] + size[0] // 8 + (1 << 20)
        assert size[1] > allocated > size[2]
        check(r, native, calls, 2, tmp_path / "grow.bam")
    finally:
        r.eng.close()


def test_a_new_descriptor_without_a_flush(rows, native, tmp_path):
    """File A, then file B, one flush: the emit to B lands A's members and leaves A's descriptor at A's end; B is appended to where
    B stood, whatever A's offset was."""
    r = rows(126)
    calls = {"a": [("to_a", 0, 0, 150)], "b": [("to_b", 5, 150, 90)]}
    front = {"a": b"A: in front", "b": b"B: other bytes, and more of them, in front"}
    with open(tmp_path / "a.bam", "wb") as fa, open(tmp_path / "b.bam", "wb") as fb:
        for k, fh in (("a", fa), ("b", fb)):
            fh.write(front[k])
            fh.flush()
            r.eng.ubam_emit_batch(fh.fileno(), calls[k], 2)
        r.eng.ubam_flush()
        for k, fh in (("a", fa), ("b", fb)):
            assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(str(tmp_path / (k + ".bam"))), k
    for k in "ab":
        want = U.members(native, U.records(calls[k], 2, *r.rows), U.record_distance(calls[k], r.RL, 2))
        assert open(tmp_path / (k + ".bam"), "rb").read() == front[k] + want, k


def test_a_write_error_surfaces_once(rows, native, tmp_path):
    """A descriptor opened read-only (EBADF on the host, nothing on the device): the next flush raises E_IO "write failed ...",
    the one after returns, the file is as it was and the next emit appends the twin's bytes."""
    from insilicoseq_amd._native import E_IO, EngineError

    r = rows(126)
    path = tmp_path / "readonly.bam"
    path.write_bytes(b"read only")
    with open(path, "rb") as fh:
        r.eng.ubam_emit_batch(fh.fileno(), [("rec", 3, 10, 120)], 0)
        with pytest.raises(EngineError) as e:
            r.eng.ubam_flush()
        assert e.value.code == E_IO and e.value.message.startswith("write failed"), e.value.message
        r.eng.ubam_flush()
    assert path.read_bytes() == b"read only"
    check(r, native, [[("rec", 3, 10, 120)]], 0, tmp_path / "good.bam")


def _read(path):
    """A file's bytes; `path`.gz gunzipped where `--compress` left that instead."""
    import gzip

    return gzip.open(path + ".gz", "rb").read() if os.path.exists(path + ".gz") else open(path, "rb").read()


def _fastq_records(path):
    lines = _read(path).split(b"\n")
    return list(zip(lines[0::4], lines[1::4], lines[3::4]))[:len(lines) // 4]


@pytest.mark.parametrize("flags", [["--gpus", "1"], ["--gpus", "2", "--devices", "1"], ["--gpus", "1", "--rng", "mt"],
                                   ["--gpus", "1", "--store_mutations", "--compress", "--report", "--depth"]],
                         ids=["one_worker", "two_workers_one_device", "mt_one_worker", "side_outputs"])
def test_generate_ubam(tmp_path, flags):
    """`generate --ubam` against the same command without it: the .bam's names (+ /1, /2 by flag), bases and chr(33 + q) phreds are
    the two FASTQ files line for line, in order; the header text and the EOF block are as specified.  With the flags that read
    the rows and not the text, their files are the same ones, and --compress applies to the .vcf only."""
    from insilicoseq_amd import bam, ubam

    fasta = str(tmp_path / "genomes.fasta")
    with open(fasta, "w") as fh:
        for k in range(5):
            fh.write(">rec%d\n%s\n" % (k, H.random_genome(31 + k, 2000 + 500 * k)))
    outs = {}
    for tag, extra in (("ubam", ["--ubam"]), ("plain", [])):
        out = str(tmp_path / tag)
        subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", "2000",
                        "--seed", "42", "--output", out] + flags + extra, cwd=ROOT, check=True, timeout=600)
        outs[tag] = out
    assert not [f for f in os.listdir(str(tmp_path)) if ".iss.tmp." in f]
    made = sorted(f[len("ubam"):] for f in os.listdir(str(tmp_path)) if f.startswith("ubam"))
    assert ".bam" in made and not [f for f in made if "fastq" in f]
    raw = open(outs["ubam"] + ".bam", "rb").read()
    assert raw[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert all(len(m) <= U.BGZF_MAX for m in U.split_members(raw))
    reader = bam.BamReader(outs["ubam"] + ".bam")
    data = b"".join(c.data.tobytes() for c in reader.chunks())
    assert reader.header == ubam.HEADER_TEXT == "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@PG\tID:insilicoseq_amd\tPN:insilicoseq_amd\n"
    assert reader.references == []
    parsed = U.parse_records(data)
    r1, r2 = _fastq_records(outs["plain"] + "_R1.fastq"), _fastq_records(outs["plain"] + "_R2.fastq")
    assert len(r1) == len(r2) == 1000 and len(parsed) == 2000
    assert [f for _n, f, _b, _q in parsed] == [77, 141] * 1000
    for mate, fq in ((0, r1), (1, r2)):
        mine = parsed[mate::2]
        assert [b"@" + n + b"/%d" % (mate + 1) for n, _f, _b, _q in mine] == [h for h, _s, _q in fq]
        assert [b for _n, _f, b, _q in mine] == [s for _h, s, _q in fq]
        assert [(q + 33).tobytes() for _n, _f, _b, q in mine] == [q for _h, _s, q in fq]
    if "--store_mutations" in flags:
        assert ".vcf.gz" in made and ".vcf" not in made
        vcf = _read(outs["ubam"] + ".vcf")
        assert vcf == _read(outs["plain"] + ".vcf") and vcf.count(b"\n") > 2
        for suffix in ("_report.json", "_depth.txt"):
            assert open(outs["ubam"] + suffix, "rb").read() == open(outs["plain"] + suffix, "rb").read()
