"""`generate --bgzip` without a GPU: the twin of the device's BGZF members (tests/bgzf_text_twin.py) on texts that exercise the
distance rule, the library's code builder against the twin's, the host writer and reader (insilicoseq_amd/bgzf.py) and the command
line's plumbing with the workers replaced by stand-ins."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import bgzf_text_twin as T
from helpers import GOLDEN
from insilicoseq_amd import bgzf

BLOCK = 32768
# the SAM specification's EOF marker (section 4.1.2), byte for byte
SPEC_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def check_members(raw, text, one_call=True):
    """Every member: the BC subfield, a BSIZE chain that ends at the end, inflates ALONE, CRC-32 and ISIZE; together: the text."""
    pos, out = 0, []
    while pos < len(raw):
        assert raw[pos:pos + 4] == b"\x1f\x8b\x08\x04" and raw[pos + 10:pos + 12] == b"\x06\x00", pos
        assert raw[pos + 12:pos + 16] == b"BC\x02\x00", pos
        size = struct.unpack_from("<H", raw, pos + 16)[0] + 1
        assert pos + size <= len(raw), "BSIZE leads past the end"
        d = zlib.decompressobj(-15)
        data = d.decompress(raw[pos + 18:pos + size - 8])
        assert d.eof and d.unused_data == b"", "the member's deflate stream does not end with the member"
        crc, isize = struct.unpack_from("<II", raw, pos + size - 8)
        assert crc == zlib.crc32(data) & 0xffffffff and isize == len(data)
        assert len(data) <= BLOCK
        out.append(data)
        pos += size
    assert pos == len(raw)
    assert b"".join(out) == text
    if one_call:  # the members of ONE call: every block but the last is full
        assert [len(x) for x in out[:-1]] == [BLOCK] * (len(out) - 1)
    return out


def random_lines(seed, n_bytes, lo, hi, alphabet=b"ACGT\t0123456789._+-"):
    """Lines of lo..hi bytes (line feed included) of random letters until n_bytes are reached."""
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    out, total = [], 0
    while total < n_bytes:
        n = int(rng.randint(lo, hi + 1))
        out.append(letters[rng.randint(0, len(letters), size=n - 1)].tobytes() + b"\n")
        total += n
    return b"".join(out)


def bedpe_like(seed, n, rid=b"NZ_CP012345.1", first=0):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        s = int(rng.randint(0, 4_000_000))
        e = s + int(rng.randint(200, 500))
        out.append(b"%s\t%d\t%d\t%s\t%d\t%d\t%s_%d_0\t.\t+\t-\t%d\n" % (rid, s, s + 125, rid, e - 125, e, rid, first + i, e - s - 250))
    return b"".join(out)


def exact(text, n):
    """`text` cut or padded (whole last line grown) to exactly n bytes, ending with a line feed."""
    text = text[:n - 1]
    return text + b"x" * (n - 1 - len(text)) + b"\n"


CASES = {
    "empty": b"",
    "one_line": b"chr1\t100\t225\tchr1\t300\t425\tchr1_0_0\t.\t+\t-\t75\n",
    "one_line_no_feed": b"chr1\t100\t225",
    "bare_feeds": b"\n" * 1000,
    "mixed_lengths": random_lines(1, 150_000, 1, 12_500),
    "long_ids": b"".join(b"%s\t%d\t%d\t%s\t%d\t%d\t%s_%d_3\t.\t+\t-\t%d\n" % (b"K" * 4096, 10 * i, 10 * i + 100, b"K" * 4096, 10 * i + 50, 10 * i + 150, b"K" * 4096, i, 50) for i in range(9)),
    "block_exact": exact(bedpe_like(2, 700), BLOCK),
    "block_minus_1": exact(bedpe_like(3, 700), BLOCK - 1),
    "block_plus_1": exact(bedpe_like(4, 700), BLOCK + 1),
    # a 300-byte line that starts 100 bytes before the block boundary
    "straddle": exact(bedpe_like(5, 600), BLOCK - 100) + b"S" * 299 + b"\n" + bedpe_like(6, 50),
    # block 1 starts exactly with a line: its predecessor lies in block 0
    "line_at_block_start": exact(bedpe_like(7, 700), BLOCK) + bedpe_like(7, 400, first=700),
    "all_equal": b"same\tline\t12345\tevery\ttime\n" * 3000,
    "nothing_shared": b"".join(bytes(((17 * k + j) % 64) + 33 for j in range(40)) + b"\n" for k in range(900)),
    "over_32768": b"A" * 40_000 + b"\n" + b"A" * 40_000 + b"\n" + bedpe_like(8, 20),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_round_trip(name):
    text = CASES[name]
    lay = T.layout(text)
    raw = lay["bytes"]
    if name == "empty":
        assert raw == b""
        return
    check_members(raw, text)
    assert len(lay["members"]) == (len(text) + BLOCK - 1) // BLOCK
    dists, toks = lay["dists"], lay["tokens"]
    offs = T.line_offsets(text)
    # the distance rule, spelled out per chunk from the text alone
    for c, d in enumerate(dists):
        pos = 32 * c
        nl = text.rfind(b"\n", 0, pos)  # the line feed that ends the line in front of the chunk's line
        if nl < 0:
            assert d == 0
            continue
        want = nl - text.rfind(b"\n", 0, nl)
        assert d == (want if want <= BLOCK and pos % BLOCK >= want else 0), (c, d, want)
    # no token reaches back past its member's first byte
    for sym, kind, _xb, _xv, dsym, _eb, _ev, at in toks:
        if kind == 2:
            assert (at % BLOCK) >= dists[at // 32] > 0
        if kind == 1:
            assert at % BLOCK > 0
    if name == "bare_feeds":  # distance 1 is the run's distance: one distance code for both kinds
        assert set(toks[toks[:, 1] > 0, 4].tolist()) == {0} and lay["code"]["hdist"] <= 2
    if name == "line_at_block_start":
        assert dists[BLOCK // 32] == 0 and text[BLOCK - 1:BLOCK] == b"\n" and max(dists[BLOCK // 32 + 1:]) > 0
    if name == "straddle":
        assert text[BLOCK - 101:BLOCK - 100] == b"\n" and dists[BLOCK // 32] == 0
    if name == "all_equal":
        assert len(raw) < len(text) // 8
    if name == "nothing_shared":
        assert not (toks[:, 1] == 2).any()
    if name == "over_32768":
        assert dists[40_001 // 32 + 1] == 0  # the second line: its predecessor is longer than a window
    if name == "mixed_lengths":
        assert len(set(dists)) > 10 and len(offs) > 10
    # offsets with empty lines in between (a VCF slot without a row) change nothing
    if len(offs) > 2:
        padded = sorted(offs + [offs[1], offs[1], offs[-1]] + [len(text)] * 3)
        assert T.members(text, padded) == raw


def test_runs_only_is_a_valid_stream_and_line_copies_pay():
    """The size condition on the committed fixtures: the twin with line copies is no larger than the twin with runs only."""
    for name in ("origins.bedpe", "mutations.vcf"):
        with open(os.path.join(GOLDEN, "bgzip", name), "rb") as fh:
            text = fh.read()
        assert 40_000 < len(text) < 200_000 and text.endswith(b"\n")
        with_copies, runs_only = T.members(text), T.members(text, runs_only=True)
        check_members(with_copies, text)
        check_members(runs_only, text)
        print("%s: %d bytes of text, %d with line copies, %d runs only, zlib 1: %d, zlib 6: %d" % (
            name, len(text), len(with_copies), len(runs_only), len(zlib.compress(text, 1)), len(zlib.compress(text, 6))))
        assert len(with_copies) <= len(runs_only)


def test_library_code_builder_is_the_twins():
    """bgzf_text_build_code (the function the device runs with 64 lanes) on the host, against the twin's plain-Python builder."""
    from insilicoseq_amd import _native

    lib = _native.lib()
    hists = [T.layout(CASES[k])["hist"] for k in ("one_line", "bare_feeds", "mixed_lengths", "all_equal", "nothing_shared", "block_plus_1")]
    rng = np.random.RandomState(5)
    deep = np.zeros(303, dtype=np.uint32)  # a histogram whose unlimited tree is deeper than 15 bits, all 30 distance codes in use
    deep[:40] = (1.6 ** np.arange(40)).astype(np.uint32)
    deep[273:] = (1.7 ** np.arange(30)).astype(np.uint32) + 1
    hists += [deep, rng.randint(0, 1000, size=303).astype(np.uint32)]
    one = np.zeros(303, dtype=np.uint32)
    one[65], one[256], one[273 + 7] = 50, 1, 9  # a single distance code in use
    hists.append(one)
    for h in hists:
        h = np.ascontiguousarray(h, dtype=np.uint32)
        entry, dentry, hdr, nbits = np.zeros(273, np.uint32), np.zeros(30, np.uint32), np.zeros(80, np.uint32), C.c_uint32(0)
        assert lib.iss_bgzf_text_code_build(h.ctypes.data, entry.ctypes.data, dentry.ctypes.data, C.byref(nbits), hdr.ctypes.data) == 0
        code = T.build_code(h)
        assert (entry >> 16).tolist() == code["len"] and (entry & 0xffff).tolist() == code["code"]
        assert (dentry >> 16).tolist() == code["dlen"] and (dentry & 0xffff).tolist() == code["dcode"]
        want = 0
        n = 0
        for v, w in code["hdr"]:
            want |= v << n
            n += w
        got = sum(int(x) << (32 * k) for k, x in enumerate(hdr))
        assert nbits.value == n and got == want
        used = [x for x in code["dlen"] if x]
        assert not used or sum(2.0 ** -x for x in used) == 1.0  # complete, as inflate requires


def test_bgzf_writer_and_reader(tmp_path):
    assert bgzf.EOF_BLOCK == SPEC_EOF and len(bgzf.EOF_BLOCK) == 28
    text = CASES["mixed_lengths"]
    path = str(tmp_path / "a.gz")
    with open(path, "wb") as fh:
        bgzf.write_member(fh, b"")  # nothing
        bgzf.write_member(fh, b"header line\n")
        bgzf.write_member(fh, text)
        fh.write(bgzf.EOF_BLOCK)
    ms = bgzf.members(path)
    assert [len(m[2]) for m in ms] == [12] + [BLOCK] * (len(text) // BLOCK) + [len(text) % BLOCK, 0]
    assert ms[-1][1] == 28 and sum(m[1] for m in ms) == os.path.getsize(path)
    assert bgzf.read(path) == b"header line\n" + text
    assert gzip.open(path, "rb").read() == b"header line\n" + text
    check_members(open(path, "rb").read(), b"header line\n" + text, one_call=False)
    # the twin's members are members to the reader too
    with open(path, "wb") as fh:
        fh.write(T.members(text) + bgzf.EOF_BLOCK)
    assert bgzf.read(path) == text and gzip.open(path, "rb").read() == text
    # a file without the EOF block, a broken chain, a wrong CRC
    raw = open(path, "rb").read()
    for bad in (raw[:-28], raw[:100] + raw[101:], raw[:-36] + b"\0" + raw[-35:]):
        with open(path, "wb") as fh:
            fh.write(bad)
        with pytest.raises(bgzf.BgzfError):
            bgzf.read(path)
    # the host route of the same container
    plain = str(tmp_path / "t.vcf")
    with open(plain, "wb") as fh:
        fh.write(text)
    assert bgzf.compress_file(plain, threads=3) == plain + ".gz" and not os.path.exists(plain)
    assert bgzf.read(plain + ".gz") == text
    open(plain, "wb").close()
    bgzf.compress_file(plain)
    assert open(plain + ".gz", "rb").read() == bgzf.EOF_BLOCK
    # assemble: header member, the parts in order, the EOF block; the parts are removed; no parts: the EOF block alone
    parts = [str(tmp_path / ("p%d" % k)) for k in range(3)]
    for k, p in enumerate(parts):
        with open(p, "wb") as fh:
            fh.write(T.members(b"part %d\n" % k) if k != 1 else b"")
    bgzf.assemble(str(tmp_path / "all.gz"), parts, header=b"#head\n")
    assert bgzf.read(str(tmp_path / "all.gz")) == b"#head\npart 0\npart 2\n"
    assert not any(os.path.exists(p) for p in parts)
    bgzf.assemble(str(tmp_path / "none.gz"), [])
    assert open(str(tmp_path / "none.gz"), "rb").read() == bgzf.EOF_BLOCK
    with pytest.raises(FileNotFoundError):
        bgzf.assemble(str(tmp_path / "x.gz"), parts)
    assert not os.path.exists(str(tmp_path / "x.gz"))


# ------------------------------------------------------------------ the command line, workers replaced by stand-ins
def test_cli_parses_bgzip():
    from insilicoseq_amd import app

    p = app.build_parser()
    assert p.parse_args(["generate", "-g", "x.fa", "-o", "out"]).bgzip is False
    args = p.parse_args(["generate", "-g", "x.fa", "-o", "out", "--bgzip", "--origins", "--store_mutations", "--compress", "--ubam"])
    assert args.bgzip is True and args.compress is True and args.ubam is True


@pytest.mark.parametrize("switch", ["ISS_HOST_FASTQ", "ISS_HOST_VCF"])
def test_cli_refuses_the_host_routes(switch, tmp_path, caplog, monkeypatch):
    from insilicoseq_amd import app

    monkeypatch.delenv("ISS_HOST_FASTQ", raising=False)
    monkeypatch.delenv("ISS_HOST_VCF", raising=False)
    monkeypatch.setenv(switch, "1")
    with pytest.raises(SystemExit) as e:
        app.main(["generate", "-g", str(tmp_path / "none.fa"), "-o", str(tmp_path / "out"), "--bgzip", "--store_mutations", "--seed", "3",
                  "--mode", "basic"])
    assert e.value.code == 1
    lines = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(lines) == 1 and "--bgzip" in lines[0] and switch in lines[0]
    assert os.listdir(tmp_path) == []


def test_worker_iterator_refuses_the_host_routes(tmp_path, monkeypatch):
    from insilicoseq_amd.generator import worker_iterator

    monkeypatch.delenv("ISS_HOST_FASTQ", raising=False)
    monkeypatch.setenv("ISS_HOST_VCF", "1")
    with pytest.raises(ValueError):
        worker_iterator([], None, 0, str(tmp_path / "w"), 1, "metagenomics", False, bgzip=True)
    assert os.listdir(tmp_path) == []


GENOMES = os.path.join(GOLDEN, "genomes.fasta")
VCF_ROW = b"r_%d_%d/1\t7\t.\tA\tC\t30\t\t\n"


class StandIn:
    """_worker and _run_worker_set of app.py without an engine: they write what a worker's files would hold and note how they
    were called."""

    def __init__(self, set_result=None):
        self.calls, self.set_calls, self.set_result = [], 0, set_result

    def worker(self, rank, device, genome_file, work_spec, npz, seed, prefix, sequence_type, gc_bias, rng, store_mutations, fragment,
               compress=False, mode=None, report=False, depth=False, records=None, ubam=False, origins=False, bgzip=False):
        self.calls.append({"rank": rank, "bgzip": bgzip, "origins": origins, "compress": compress})
        for mate in (1, 2):
            with open("%s_R%d.fastq" % (prefix, mate), "wb") as fh:
                fh.write(b"@r%d/%d\nA\n+\nI\n" % (rank, mate))
        vcf = b"".join(VCF_ROW % (i, rank) for i in range(3)) if store_mutations else b""
        with open(prefix + ".vcf", "wb") as fh:
            fh.write(T.members(vcf) if bgzip else vcf)
        if origins:
            text = bedpe_like(rank, 4, rid=b"rec%d" % rank)
            with open(prefix + "_origins.bedpe", "wb") as fh:
                fh.write(T.members(text) if bgzip else text)

    def worker_set(self, jobs, records, error_model, args, device_gzip, workers):
        self.set_calls += 1
        if self.set_result is None:
            return None
        for j in jobs:  # the set's text route: plain .vcf files beside temporary FASTQ files
            self.worker(*j[:12], bgzip=False)
        return False


def run_cli(tmp_path, monkeypatch, extra, stand_in, workers=1):
    from insilicoseq_amd import app

    monkeypatch.delenv("ISS_HOST_FASTQ", raising=False)
    monkeypatch.delenv("ISS_HOST_VCF", raising=False)
    monkeypatch.setattr(app, "_worker", stand_in.worker)
    monkeypatch.setattr(app, "_run_worker_set", stand_in.worker_set)

    class InlinePool:  # (the stand-ins are not picklable and there is nothing to run side by side)
        def __init__(self, n):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def starmap(self, fn, jobs):
            return [fn(*j) for j in jobs]

    class Ctx:
        Pool = InlinePool

    monkeypatch.setattr(app.mp, "get_context", lambda kind: Ctx)
    out = str(tmp_path / "run")
    argv = ["generate", "-g", GENOMES, "-o", out, "--mode", "basic", "--seed", "7", "-n", "400", "--cpus", str(workers)] + extra
    assert app.main(argv) == 0
    return out, sorted(f for f in os.listdir(tmp_path) if not f.endswith(("_abundance.txt", "_coverage.txt")))


def test_cli_single_worker_files(tmp_path, monkeypatch):
    from insilicoseq_amd import origins as G
    from insilicoseq_amd.distributed import VCF_HEADER

    s = StandIn()
    out, files = run_cli(tmp_path, monkeypatch, ["--bgzip", "--store_mutations", "--origins"], s)
    assert s.calls == [{"rank": 0, "bgzip": True, "origins": True, "compress": False}]
    assert files == ["run.vcf.gz", "run_R1.fastq", "run_R2.fastq", "run_origins.bedpe.gz"]
    assert bgzf.read(out + ".vcf.gz") == (VCF_HEADER + "\n").encode() + b"".join(VCF_ROW % (i, 0) for i in range(3))
    ms = bgzf.members(out + ".vcf.gz")
    assert ms[0][2] == (VCF_HEADER + "\n").encode() and ms[-1][2] == b"" and len(ms) == 3  # the header is a member of its own
    assert bgzf.read(out + "_origins.bedpe.gz") == bedpe_like(0, 4, rid=b"rec0")
    assert G.parse(out + "_origins.bedpe.gz")["name"].tolist() == ["rec0_%d_0" % i for i in range(4)]
    for name in ("run.vcf.gz", "run_origins.bedpe.gz"):
        assert open(str(tmp_path / name), "rb").read()[-28:] == bgzf.EOF_BLOCK


def test_cli_pool_compress_beside_bgzip(tmp_path, monkeypatch):
    """Two workers, --compress too: the two text outputs take the --bgzip route, the FASTQ files --compress's."""
    s = StandIn()
    out, files = run_cli(tmp_path, monkeypatch, ["--bgzip", "--store_mutations", "--origins", "--compress"], s, workers=2)
    assert [c["bgzip"] for c in s.calls] == [True, True] and [c["compress"] for c in s.calls] == [True, True]
    assert files == ["run.vcf.gz", "run_R1.fastq.gz", "run_R2.fastq.gz", "run_origins.bedpe.gz"]
    assert bgzf.read(out + "_origins.bedpe.gz") == bedpe_like(0, 4, rid=b"rec0") + bedpe_like(1, 4, rid=b"rec1")
    assert bgzf.read(out + ".vcf.gz").count(b"\n") == 2 + 6
    assert len(bgzf.members(out + ".vcf.gz")) == 4  # header, one member per worker, EOF


def test_cli_warns_without_outputs(tmp_path, monkeypatch, caplog):
    s = StandIn()
    _out, files = run_cli(tmp_path, monkeypatch, ["--bgzip"], s)
    assert s.calls[0]["bgzip"] is False and files == ["run_R1.fastq", "run_R2.fastq"]
    warnings = [r.getMessage() for r in caplog.records if r.levelname == "WARNING" and "--bgzip" in r.getMessage()]
    assert len(warnings) == 1


def test_cli_origins_alone_and_vcf_alone(tmp_path, monkeypatch):
    s = StandIn()
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    _out, files = run_cli(tmp_path / "a", monkeypatch, ["--bgzip", "--origins"], s)
    assert files == ["run_R1.fastq", "run_R2.fastq", "run_origins.bedpe.gz"]
    _out, files = run_cli(tmp_path / "b", monkeypatch, ["--bgzip", "--store_mutations"], s)
    assert files == ["run.vcf.gz", "run_R1.fastq", "run_R2.fastq"]


def test_cli_worker_set_vcf_falls_to_host_bgzf(tmp_path, monkeypatch):
    """--rng mt --cpus W --devices 1: the set writes its VCF as text (iss_vcf_emit_workers); the parent makes the same container."""
    from insilicoseq_amd.distributed import VCF_HEADER

    s = StandIn(set_result=False)
    out, files = run_cli(tmp_path, monkeypatch, ["--bgzip", "--store_mutations", "--rng", "mt", "--devices", "1"], s, workers=2)
    assert s.set_calls == 1 and [c["bgzip"] for c in s.calls] == [False, False]
    assert files == ["run.vcf.gz", "run_R1.fastq", "run_R2.fastq"]
    assert bgzf.read(out + ".vcf.gz") == (VCF_HEADER + "\n").encode() + b"".join(VCF_ROW % (i, r) for r in range(2) for i in range(3))
    # the set could not be set up: the pool, whose workers compress on the device
    (tmp_path / "p").mkdir()
    s = StandIn(set_result=None)
    out, files = run_cli(tmp_path / "p", monkeypatch, ["--bgzip", "--store_mutations", "--rng", "mt", "--devices", "1"], s, workers=2)
    assert s.set_calls == 1 and [c["bgzip"] for c in s.calls] == [True, True]
    assert files == ["run.vcf.gz", "run_R1.fastq", "run_R2.fastq"]
    assert len(bgzf.members(out + ".vcf.gz")) == 4
