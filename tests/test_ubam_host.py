"""`generate --ubam` without a GPU: the record layout (iss_ubam_host_records against tests/ubam_twin.py and an independent parser),
the twin's BGZF stream (every member a complete gzip member that inflates ALONE), the command line and the file's frame."""
import io
import os
import struct

import numpy as np
import pytest

import deflate_twin as T
import ubam_twin as U


@pytest.fixture(scope="module")
def native():
    from insilicoseq_amd import _native

    return _native


def host_rows(n, RL, seed, letters=b"ACGT"):
    rng = np.random.RandomState(seed)
    alphabet = np.frombuffer(letters, dtype=np.uint8)
    return [alphabet[rng.randint(0, len(alphabet), size=(n, RL))] if k % 2 == 0 else rng.randint(0, 42, size=(n, RL)).astype(np.uint8)
            for k in range(4)]


def host_records(native, path, rid, first_i, cpu, rows, pitch=None):
    """iss_ubam_host_records over rows [n, RL] (copied into arrays of `pitch` columns) -> the bytes it appended to the file."""
    n, RL = rows[0].shape
    pitch = pitch or RL
    wide = [np.zeros((n, pitch), dtype=np.uint8) for _ in rows]
    for w, r in zip(wide, rows):
        w[:, :RL] = r
    with open(path, "ab") as fh:
        fh.flush()
        rc = native.lib().iss_ubam_host_records(fh.fileno(), T.as_bytes(rid), first_i, cpu, n, RL, pitch, *[w.ctypes.data for w in wide])
    return rc


@pytest.mark.parametrize("RL,n,rid,first_i,cpu", [(20, 1, "g", 0, 0), (125, 7, "NZ_CP012345.1", 95, 123), (126, 12, "x" * 200, 7, 2),
                                                  (301, 3, "r", 998, 0), (1, 3, "one", 9, 1)])
def test_host_records_equal_the_twin(native, tmp_path, RL, n, rid, first_i, cpu):
    rows = host_rows(n, RL, seed=RL + n)
    path = tmp_path / "rec.bin"
    assert host_records(native, path, rid, first_i, cpu, rows, pitch=RL + 5) == 0
    got = path.read_bytes()
    want = U.records([(rid, first_i, 0, n)], cpu, *rows)
    assert got == want
    assert len(got) == sum(2 * U.record_length(rid, first_i + k, cpu, RL) for k in range(n))
    # iss_bam_scan walks the block_size chain: exactly 2 n records, all bytes covered
    from insilicoseq_amd import bam

    offs, used = bam.scan(got)
    assert len(offs) == 2 * n and used == len(got)
    # the independent parser: names, flags, bases and phreds come back
    parsed = U.parse_records(got)
    assert len(parsed) == 2 * n
    for k in range(n):
        for mate in (0, 1):
            name, flag, bases, qual = parsed[2 * k + mate]
            assert name == b"%s_%d_%d" % (rid.encode(), first_i + k, cpu)
            assert flag == (141 if mate else 77)
            assert bases == rows[2 * mate][k].tobytes()
            assert np.array_equal(qual, rows[2 * mate + 1][k])


def test_letters_are_upper_cased_and_coded(native, tmp_path):
    """Lower case counts as upper case (BAM has no case), the IUPAC letters keep their codes, anything else is N."""
    letters = b"ACGTacgtNnRYWSMKHBVDrywsmkhbvd=*x.U"
    rows = [np.frombuffer(letters, dtype=np.uint8).reshape(1, -1).copy(), np.arange(len(letters), dtype=np.uint8).reshape(1, -1)] * 2
    path = tmp_path / "letters.bin"
    assert host_records(native, path, "L", 0, 0, rows) == 0
    got = path.read_bytes()
    assert got == U.records([("L", 0, 0, 1)], 0, *rows)
    _name, _flag, bases, qual = U.parse_records(got)[0]
    assert bases == b"ACGTACGTNNRYWSMKHBVDRYWSMKHBVDNNNNN"
    assert qual.tolist() == list(range(len(letters)))
    # the codes themselves, first base in the high nibble, the low nibble past the odd length 0
    seq = got[36 + len(b"L_0_0") + 1:][:(len(letters) + 1) // 2]
    nib = [x for b in seq for x in (b >> 4, b & 15)]
    assert nib[:8] == [1, 2, 4, 8, 1, 2, 4, 8] and nib[len(letters)] == 0
    assert nib[8:20] == [15, 15, 5, 10, 9, 6, 3, 12, 11, 14, 7, 13]


def test_name_limit(native, tmp_path):
    """254 characters fit l_read_name, 255 do not: ISS_E_INVALID naming the record id, nothing written."""
    rows = host_rows(2, 8, seed=1)
    path = tmp_path / "names.bin"
    ok = "k" * (254 - len("_9_3"))
    assert host_records(native, path, ok, 8, 3, rows) == 0
    size = os.path.getsize(path)
    assert [len(r[0]) for r in U.parse_records(path.read_bytes())] == [254] * 4
    assert host_records(native, path, ok, 9, 3, rows) == native.E_INVALID  # (pair 10: one digit more)
    assert ok[:40].encode() in native.lib().iss_last_error(None)
    assert os.path.getsize(path) == size


# ------------------------------------------------------------------ the BGZF stream
def record_text(n=200, RL=126, rid="NZ_CP012345.1_Esche_K", first_i=95, cpu=2):
    rows = host_rows(n, RL, seed=5)
    rows[1][:] = 37  # (top-quality phred lines: runs, and previous-record matches in the constant fields)
    rows[3][:, : RL // 2] = 37
    return U.records([(rid, first_i, 0, n)], cpu, *rows), U.record_distance([(rid, first_i, 0, n)], RL, cpu)


def stream_cases():
    rec, dist = record_text()
    rng = np.random.RandomState(1)
    cases = {
        "empty": (b"", 0),
        "one_byte": (b"Q", 0),
        "one_block": (bytes(rng.randint(65, 70, size=T.BLOCK).astype(np.uint8)), 0),
        "block_plus_one": (bytes(rng.randint(65, 70, size=T.BLOCK + 1).astype(np.uint8)), 37),
        "three_blocks_and_five": (bytes(rng.randint(65, 70, size=3 * T.BLOCK + 5).astype(np.uint8)), 37),
        "one_repeated_byte": (b"\x25" * (2 * T.BLOCK + 100), 64),
        "random_64k": (np.random.RandomState(1).bytes(65536), 0),
        "records": (rec, dist),
    }
    return cases


CASES = stream_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_members(native, name):
    from insilicoseq_amd import bam

    text, dist = CASES[name]
    lay = U.layout(native, text, dist)
    stream = lay["bytes"]
    if not text:
        assert stream == b"" and lay["members"] == []  # (an emit of no records appends nothing)
        return
    n_blocks = (len(text) + T.BLOCK - 1) // T.BLOCK
    assert len(lay["members"]) == n_blocks
    # the project's own reader: block chain, then CRC and ISIZE of every member
    groups = list(bam._block_groups(io.BytesIO(stream), 1 << 20, 1 << 16))
    assert sum(len(g) for g in groups) == n_blocks
    assert b"".join(bam._inflate_group(g) for g in groups) == text
    # every BSIZE within the cap; no member decodes differently ALONE (a match behind the block's start would fail here)
    parts = U.split_members(stream)
    assert parts == lay["members"]
    for b, m in enumerate(parts):
        assert len(m) <= U.BGZF_MAX
        assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m)
        assert U.inflate_member(m) == text[b * T.BLOCK:(b + 1) * T.BLOCK]
    print("%s: %d text bytes, %d members, %d bytes (largest member %d)" % (name, len(text), n_blocks, len(stream), max(map(len, parts))))


def test_member_rule_is_visible():
    """The record text is a case that can see the rule: tokenized as ONE text (the gzip path's rule) its later blocks start with
    other tokens than tokenized alone -- matches whose source lies in the block before."""
    text, dist = CASES["records"]
    assert len(text) > 2 * T.BLOCK and dist
    whole = T.token_table(text, dist)
    second = T.token_table(text[T.BLOCK:2 * T.BLOCK], dist)
    in_second = whole[(whole[:, 4] >= T.BLOCK) & (whole[:, 4] < 2 * T.BLOCK)]
    assert (in_second[:, 1] == 2).sum() > (second[:, 1] == 2).sum()
    first_chunks = in_second[in_second[:, 4] < T.BLOCK + dist]
    assert (first_chunks[:, 1] == 2).any() and not (second[second[:, 4] < dist][:, 1] == 2).any()


def test_random_text_stays_under_the_cap(native):
    """64 KB of incompressible bytes: two members, each far under 65 536 bytes although no byte is saved."""
    text, dist = CASES["random_64k"]
    parts = U.layout(native, text, dist)["members"]
    assert len(parts) == 2 and all(T.BLOCK < len(m) <= U.BGZF_MAX for m in parts)


# ------------------------------------------------------------------ the command line and the frame
def test_cli_parses_ubam():
    from insilicoseq_amd import app

    p = app.build_parser()
    assert p.parse_args(["generate", "-g", "x.fa", "-o", "out"]).ubam is False
    args = p.parse_args(["generate", "-g", "x.fa", "-o", "out", "--ubam", "--compress"])
    assert args.ubam is True and args.compress is True


def test_cli_refuses_the_worker_set(tmp_path, caplog):
    """--rng mt --cpus W --devices 1 runs the workers side by side through iss_fastq_emit_scatter: one error line, nothing written."""
    from insilicoseq_amd import app

    out = str(tmp_path / "o")
    with pytest.raises(SystemExit) as e:
        app.main(["generate", "-g", str(tmp_path / "none.fa"), "-o", out, "--ubam", "--rng", "mt", "--cpus", "4", "--devices", "1",
                  "--seed", "3", "--mode", "basic"])
    assert e.value.code == 1
    lines = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(lines) == 1 and "--ubam" in lines[0] and "\n" not in lines[0]
    assert os.listdir(tmp_path) == []


def test_frame_of_an_empty_run(tmp_path):
    """No record blocks: the header member, then the 28-byte EOF block; the project's reader finds the text and no record."""
    from insilicoseq_amd import bam, ubam

    target = str(tmp_path / "empty.bam")
    ubam.assemble(target, [])
    data = open(target, "rb").read()
    assert data[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000") == ubam.EOF_BLOCK
    parts = U.split_members(data)
    assert len(parts) == 2
    text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@PG\tID:insilicoseq_amd\tPN:insilicoseq_amd\n"
    assert U.inflate_member(parts[0]) == b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 0)
    assert U.inflate_member(parts[1]) == b""
    r = bam.BamReader(target)
    assert list(r.chunks()) == [] and r.header == text and r.references == []


def test_frame_around_blocks(native, tmp_path):
    """Two workers' block files in worker order between header and EOF; the block files are removed; a missing one is an
    error before anything is written."""
    from insilicoseq_amd import bam, ubam

    rows = host_rows(3, 20, seed=9)
    texts = [U.records([("w%d" % k, 0, 0, 3)], k, *rows) for k in range(2)]
    paths = []
    for k, t in enumerate(texts):
        paths.append(str(tmp_path / ("w%d.bam" % k)))
        with open(paths[-1], "wb") as fh:
            fh.write(U.members(native, t, 0))
    target = str(tmp_path / "two.bam")
    with pytest.raises(FileNotFoundError):
        ubam.assemble(target, paths + [str(tmp_path / "absent.bam")])
    assert not os.path.exists(target) and all(os.path.exists(p) for p in paths)
    ubam.assemble(target, paths)
    assert not any(os.path.exists(p) for p in paths)
    chunks = list(bam.BamReader(target).chunks())
    assert b"".join(c.data.tobytes() for c in chunks) == b"".join(texts)
    assert sum(len(c.offsets) for c in chunks) == 12
    assert open(target, "rb").read()[-28:] == ubam.EOF_BLOCK


def test_failure_leaves_no_bam(tmp_path, monkeypatch):
    """Whatever fails behind the first byte: neither a half-written <output>.bam nor the workers' block files stay."""
    from insilicoseq_amd import app
    from insilicoseq_amd.distributed import temp_prefix

    out = str(tmp_path / "o")

    def fails(args, ubam):
        assert ubam
        for path in (out + ".bam", temp_prefix(out, 0) + ".bam", temp_prefix(out, 1) + ".bam"):
            open(path, "wb").write(b"partial")
        raise RuntimeError("a worker failed")

    monkeypatch.setattr(app, "_generate_reads", fails)
    with pytest.raises(RuntimeError):
        app.main(["generate", "-g", "x.fa", "-o", out, "--ubam", "--gpus", "2", "--quiet"])
    assert os.listdir(tmp_path) == []
