"""`report --bam`: the tallies of BAM records built on the device (iss_br_*: k_br_records, k_br_positions) against the numpy twin
(insilicoseq_amd.bam_report.bam_reads_host), word for word, with the records taken and skipped and the first bad record; the
launch geometry, the layout of a record, the feeds, the error paths and the round trips through the command line."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import bam_report_cases as BC
import bam_synth
from helpers import mixed_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 151, 301, 1024)

_contexts = {}


def _context(max_len):
    """One context per max_len for the whole module, reset before every use."""
    from insilicoseq_amd.bam_report import BamReadTally

    if max_len not in _contexts:
        _contexts[max_len] = BamReadTally(0, max_len)
    _contexts[max_len].reset()
    return _contexts[max_len]


def _device(chunks, max_len):
    dev = _context(max_len)
    for chunk in chunks:
        dev.feed(chunk)
    return dev.download()


def _same(got, exp, max_len):
    from insilicoseq_amd.fastq_report import split_fq_words

    assert got["records"] == exp["records"] and got["skipped"] == exp["skipped"]
    assert (got["bad_record"], got["bad_code"]) == (exp["bad_record"], exp["bad_code"])
    g, e = split_fq_words(got["tally"], max_len), split_fq_words(exp["tally"], max_len)
    assert [k for k in g if not np.array_equal(g[k], e[k])] == []  # (the fields that differ)


def _check(records, max_len, per=None):
    """The records as one feed (per: that many records a feed) on the device and in the twin."""
    from insilicoseq_amd.bam_report import bam_reads_host

    chunks = [BC.chunk_of(records)] if per is None else BC.split(BC.chunk_of(records), per)
    got = _device(chunks, max_len)
    _same(got, bam_reads_host(chunks, max_len), max_len)
    return got


def _fields(got, max_len):
    from insilicoseq_amd.fastq_report import split_fq_words

    return split_fq_words(got["tally"], max_len)


# ---------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("lengths,max_len", [(LENGTHS, 1024), (LENGTHS[:-1], 301), (LENGTHS[:-1], 1024)])
def test_mixed_lengths(lengths, max_len):
    records = BC.mixed(lengths, 240, 11)
    got = _check(records, max_len)
    t = _fields(got, max_len)
    assert got["bad_record"] == -1 and got["skipped"] == [0, 0] and sum(got["records"]) == 240 == int(t["length"].sum())
    assert int(t["pairs"][0]) == got["records"][0] and t["insert"].any()
    for n in lengths:  # every length on both strands and both mates
        flags = {r["flag"] for r in records if len(r["seq"]) == n}
        assert flags == {BC.R1F, BC.R1R, BC.R2F, BC.R2R}, n
        assert int(t["length"][0][n]) > 0 and int(t["length"][1][n]) > 0
    assert t["qual"][:, :, 0].any() and t["qual"][:, :, 93].any() and t["base"][:, :, 4].any()
    assert int(t["qual"][0, max(lengths) - 1].sum()) == int(t["length"][0][max(lengths)])  # the last position: the longest reads


@pytest.mark.parametrize("n_records", [1, 63, 64, 65, 1000])
def test_record_counts(n_records):
    got = _check(BC.mixed((0, 1, 63, 64, 65, 151), n_records, 20 + n_records), 151)
    assert sum(got["records"]) == n_records


@pytest.mark.parametrize("wgs", ["1", "3", "4096"])
def test_launch_geometry(wgs, monkeypatch):
    records = BC.mixed((0, 1, 63, 64, 65, 151, 301), 300, 31)
    plain = _device([BC.chunk_of(records)], 301)
    monkeypatch.setenv("ISS_BR_WGS", wgs)
    forced = _check(records, 301)
    assert np.array_equal(plain["tally"], forced["tally"])


# ---------------------------------------------------------------------------------------------------- layout of a record
def test_seq_at_every_alignment():
    """Names of 1 .. 8 and 254 characters, 0, 1 and 65 CIGAR operations, no tags and 300 bytes of them, odd and even read lengths:
    block_size fields, SEQ and QUAL at every alignment."""
    rnd = random.Random(41)
    records = []
    for name_len in (1, 2, 3, 4, 5, 6, 7, 8, 254):
        for n_cigar in (0, 1, 65):
            for tags in ((), [("XX", "Z", "t" * 296)]):  # 2 + 1 + 296 + 1 = 300 bytes
                for l in (9, 10, 151):
                    seq = BC.random_seq(rnd, l, "ACGT" * 4 + BC.LETTERS)
                    records.append(BC.rec(seq, [rnd.randint(0, 93) for _ in range(l)], rnd.choice((BC.R1F, BC.R1R, BC.R2F, BC.R2R)),
                                          name="n" * name_len, n_cigar=n_cigar, tags=tags))
    chunk = BC.chunk_of(records)
    assert {int(o) % 4 for o in chunk.offsets} == {0, 1, 2, 3}
    got = _check(records, 151)
    assert sum(got["records"]) == len(records) and got["bad_record"] == -1


def test_every_code_at_both_ends():
    """All sixteen codes at position 0 and at the last position, forward and reverse, at even and odd lengths -- the last base of an
    odd-length read is the high half of a byte whose low half is padding; phreds 0 and 93 at both ends."""
    records = []
    for c in range(16):
        for l in (1, 2, 7, 8, 65, 66):
            for flag in (BC.R1F, BC.R1R, BC.R2F, BC.R2R):
                seq = BC.LETTERS[c] + ("A" * (l - 2) + BC.LETTERS[(7 * c + 3) % 16] if l > 1 else "")
                records.append(BC.rec(seq, [93 if (k + c) % 2 else 0 for k in range(l)], flag))
    got = _check(records, 66)
    t = _fields(got, 66)
    assert int(t["base"][:, 0].sum()) == len(records) and t["qual"][:, 0, 0].all() and t["qual"][:, 0, 93].all()
    # sixteen codes, four of them A C G T: three of four reads show "other" at position 0, and what the last position of the
    # 66-base reads shows is one of 16 codes too, forward (code 7 c + 3) or reverse (the complement of c)
    assert int(t["base"][:, 0, 4].sum()) == len(records) * 12 // 16 and int(t["base"][:, 65].sum()) == 16 * 4
    assert int(t["base"][:, 65, 4].sum()) == 16 * 4 * 12 // 16


def test_flags():
    rnd = random.Random(51)
    flags = [0, 0x10, 0x40, 0x80, 0x41, 0x81, 0xC1, 0x01, 0x141, 0x841, 0x941, 0x100, 0x800, 0x45, 0x49, 0x4D, 0x85, 0x51, 0x91, 0x91 | 4,
             0xC1 | 0x10, 0x11, 0x181, 0x881, 0x43, 0x83, 0x41 | 0x200, 0x41 | 0x400]
    records = [BC.rec(BC.random_seq(rnd, 30 + k % 7), flag=f, tlen=rnd.choice((300, -400))) for k, f in enumerate(flags * 3)]
    got = _check(records, 64)
    assert got["skipped"] == [3 * sum(1 for f in flags if f & 0x900), 3 * sum(1 for f in flags if not f & 0x900 and f & 1 and (f & 0xC0) in (0, 0xC0))]
    assert got["skipped"][0] > 0 and got["skipped"][1] > 0 and sum(got["records"]) + sum(got["skipped"]) == len(records)


def test_insert_sizes():
    """tlen 0, +-1, +-2 l, +-(2 l + 2046), +-(2 l + 2047), +-(2 l + 5000), INT32_MIN, different references, next_refID -1, ..."""
    cases = BC.insert_cases()
    got = _check([r for r, _ in cases], 16)
    t = _fields(got, 16)
    assert np.array_equal(t["insert"], np.bincount([e for _, e in cases if e is not None], minlength=2048))
    assert int(t["insert"][0]) >= 4 and int(t["insert"][2046]) == 2 and int(t["insert"][2047]) >= 6
    for l, max_len in ((151, 151), (1024, 1024)):  # 2 l_seq at the lengths that matter
        seq = "ACGT" * (l // 4) + "ACG"[:l % 4]
        recs = [BC.rec(seq, tlen=s * (2 * l + d)) for s in (1, -1) for d in (-1, 0, 1, 2046, 2047, 5000)]
        t = _fields(_check(recs, max_len), max_len)
        assert [int(t["insert"][b]) for b in (0, 1, 2046, 2047)] == [4, 2, 2, 4] and int(t["insert"].sum()) == 12


# ---------------------------------------------------------------------------------------------------- feeds
def test_feeds_do_not_change_the_words():
    records = bam_synth.records(61, n_pairs=50, var_lengths=(4, 301))
    whole = _check(records, 301)
    assert sum(whole["skipped"]) > 0
    for per in (4, 1):
        got = _check(records, 301, per)
        assert np.array_equal(got["tally"], whole["tally"]) and got["records"] == whole["records"] and got["skipped"] == whole["skipped"]


def test_reset():
    from insilicoseq_amd.bam_report import bam_reads_host

    records = BC.mixed((10, 151), 50, 81)
    dev = _context(151)
    dev.feed(BC.chunk_of([BC.rec("ACGT", "none")] + records))
    dev.feed(BC.chunk_of(records))
    first = dev.download()
    assert sum(first["records"]) == 100 and (first["bad_record"], first["bad_code"]) == (0, 3)
    assert dev.kernel_ms() > 0.0  # (HIP events around the two feeds' launches)
    dev.reset()
    zero = dev.download()
    assert dev.kernel_ms() == 0.0
    assert not zero["tally"].any() and zero["records"] == [0, 0] and zero["skipped"] == [0, 0] and (zero["bad_record"], zero["bad_code"]) == (-1, 0)
    dev.feed(BC.chunk_of(records))
    _same(dev.download(), bam_reads_host(BC.chunk_of(records), 151), 151)


# ---------------------------------------------------------------------------------------------------- bad records
def _spoiled(r, code, variant=0):
    if code == 1:
        return (dict(r, l_read_name=0), dict(r, l_seq=-1), dict(r, truncate=7), dict(r, l_seq=2 ** 31 - 1))[variant]
    if code == 2:
        return BC.rec(r["seq"] * 2, flag=r["flag"])  # 80 > max_len 64
    if code == 3:
        return dict(r, qual=None)
    return dict(r, qual=r["qual"][:20] + [94 if variant == 0 else 255] + r["qual"][21:])


@pytest.mark.parametrize("where", [0, 64, 129])
@pytest.mark.parametrize("code", [1, 2, 3, 4])
def test_bad_record_codes(code, where):
    records = BC.mixed((40,), 130, 90 + code)
    records[where] = _spoiled(records[where], code)
    got = _check(records, 64)
    assert (got["bad_record"], got["bad_code"]) == (where, code) and sum(got["records"]) == 129
    assert int(_fields(got, 64)["length"][:, 40].sum()) == 129  # the good records beside it are tallied


def test_bad_record_variants():
    for code, variant in ((1, 1), (1, 2), (1, 3), (4, 1)):
        records = BC.mixed((40,), 20, 95)
        records[7] = _spoiled(records[7], code, variant)
        got = _check(records, 64)
        assert (got["bad_record"], got["bad_code"]) == (7, code), (code, variant)


def test_first_bad_record_wins():
    a, b = BC.mixed((40,), 130, 7), BC.mixed((40,), 130, 8)
    a[100], b[30] = _spoiled(a[100], 4), _spoiled(b[30], 3)
    got = _check(a + b, 64)
    assert (got["bad_record"], got["bad_code"]) == (100, 4)
    got = _check(b + a, 64, 65)  # (over four feeds: the index counts the records of the feeds before)
    assert (got["bad_record"], got["bad_code"]) == (30, 3)
    got = _check(b + a, 64, 1)
    assert (got["bad_record"], got["bad_code"]) == (30, 3)
    two = BC.mixed((40,), 10, 9)
    two[7] = dict(BC.rec(two[7]["seq"] * 2, "none"))  # too long and without qualities: the smaller code
    got = _check(two, 64)
    assert (got["bad_record"], got["bad_code"]) == (7, 2)
    two[7] = BC.rec("ACGT", [255, 94, 0, 0])            # without qualities and out of range
    assert _check(two, 64)["bad_code"] == 3
    sec = BC.mixed((40,), 10, 10)
    sec[4] = dict(_spoiled(sec[4], 4), flag=BC.R1F | 0x100)  # a bad secondary record is reported, not skipped
    got = _check(sec, 64)
    assert (got["bad_record"], got["bad_code"]) == (4, 4) and got["skipped"] == [0, 0]
    sec[2] = dict(sec[2], flag=BC.R2R | 0x800)               # (a good one in front of it counts in the index)
    got = _check(sec, 64)
    assert (got["bad_record"], got["bad_code"]) == (4, 4) and got["skipped"] == [1, 0]


def test_buffers_grow_in_the_middle_of_a_pipeline():
    """A fresh context, so that nothing has grown before: the second feed passes the 2^16-record floor of its slot's offsets and of
    the descriptors and the 1 MiB floor of its slot's bytes while the first is still in flight, and the third follows it at once
    (the module's shared contexts only ever grow on their first feed)."""
    from insilicoseq_amd.bam_report import BamReadTally, bam_reads_host

    chunks = [BC.chunk_of(BC.mixed(tuple(range(1, 9)), n, 130 + k)) for k, n in enumerate((40, 70000, 40))]
    assert chunks[1].offsets.size > (1 << 16) and chunks[1].data.size > (1 << 20) and chunks[0].data.size < 4096
    with BamReadTally(0, 16) as dev:
        for chunk in chunks:
            dev.feed(chunk)
        got = dev.download()
    _same(got, bam_reads_host(chunks, 16), 16)
    assert sum(got["records"]) == 70080 and got["bad_record"] == -1


# ---------------------------------------------------------------------------------------------------- invalid arguments
def test_invalid_arguments_launch_nothing():
    from insilicoseq_amd import _native
    from insilicoseq_amd.bam_report import bam_reads_host

    lib = _native.lib()
    dev = _context(64)
    records = BC.mixed((40,), 6, 111)
    chunk = BC.chunk_of(records)
    dev.feed(chunk)
    before = dev.download()
    data = np.ascontiguousarray(chunk.data)
    n = data.size
    p, o = data.ctypes.data, np.ascontiguousarray(chunk.offsets, dtype=np.int64)

    def feed(ptr, n_bytes, offs, n_records):
        offs = None if offs is None else np.ascontiguousarray(offs, dtype=np.int64)
        rc = lib.iss_br_feed(dev._h, ptr, n_bytes, None if offs is None else offs.ctypes.data, n_records)
        return rc

    big = data.copy()
    big[int(o[5]):int(o[5]) + 4] = np.frombuffer(np.int32(n).tobytes(), dtype=np.uint8)  # a block_size past the chunk
    small = data.copy()
    small[int(o[2]):int(o[2]) + 4] = np.frombuffer(np.int32(31).tobytes(), dtype=np.uint8)
    for args in ((None, n, o, 6), (p, n, None, 6), (p, -1, o, 6), (p, n, o, -1), (p, 1 << 31, o, 6), (p, (1 << 40) + n, o, 6),
                 (p, n, [0, n], 2), (p, n, [0, n - 35], 2), (p, n, [-1], 1), (p, n, [0, -8], 2),  # an offset past the chunk, or in front of it
                 (p, n - 1, o, 6),                                                               # the last record's end past the chunk
                 (big.ctypes.data, n, o, 6), (small.ctypes.data, n, o, 6),
                 (p, n, o[::-1], 6), (p, n, [o[0], o[2], o[1]], 3), (p, n, [o[0], o[1], o[1]], 3)):  # offsets out of order, or twice
        assert feed(*args) == _native.E_INVALID, args[1:]
        assert b"iss_br_feed" in lib.iss_br_last_error(dev._h)
    assert lib.iss_br_feed(None, p, n, o.ctypes.data, 6) == _native.E_INVALID
    assert feed(None, 0, None, 0) == 0 and feed(p, n, o, 0) == 0
    after = dev.download()
    _same(after, before, 64)  # the context's tally is unchanged
    _same(after, bam_reads_host(chunk, 64), 64)
    h = C.c_void_p()
    for max_len in (0, -1, 1025):
        assert lib.iss_br_create(0, max_len, C.byref(h)) == _native.E_INVALID and not h
    assert lib.iss_br_create(99, 64, C.byref(h)) == _native.E_INVALID and not h
    assert lib.iss_br_create(1 << 20, 64, C.byref(h)) == _native.E_INVALID and not h
    assert b"device ordinal out of range" in lib.iss_br_last_error(None)
    assert lib.iss_br_create(0, 64, None) == _native.E_INVALID
    assert lib.iss_br_tally_words(None) == -1 and lib.iss_br_tally_words(dev._h) == 1 + 64 * 200 + 2 + 188 + 2048 + 2 * 65
    rec, skip, bad, code = (C.c_int64 * 2)(), (C.c_int64 * 2)(), C.c_int64(), C.c_int32()
    words = np.zeros(lib.iss_br_tally_words(dev._h), dtype=np.uint64)
    for k in range(5):
        a = [words.ctypes.data, C.addressof(rec), C.addressof(skip), C.byref(bad), C.byref(code)]
        a[k] = None
        assert lib.iss_br_download(dev._h, *a) == _native.E_INVALID
    assert lib.iss_br_reset(None) == _native.E_INVALID and lib.iss_br_kernel_ms(dev._h, None) == _native.E_INVALID
    lib.iss_br_destroy(None)


# ---------------------------------------------------------------------------------------------------- files and the command line
def test_feed_file_and_result(tmp_path):
    from insilicoseq_amd.bam_report import BamReadTally, bam_reads_host, finish

    records = bam_synth.records(121, n_pairs=120, var_lengths=(20, 75))
    path = str(tmp_path / "a.bam")
    bam_synth.write_records(path, records)
    exp = finish(bam_reads_host(BC.chunk_of(records), 1024), 1024)
    with BamReadTally(0) as dev:
        dev.feed_file(path, chunk_bytes=777)
        got = dev.result()
    assert got["read_length"] == exp["read_length"] <= 75 and got["records"] == exp["records"] and got["skipped"] == exp["skipped"]
    assert got["bad_record"] == -1 and np.array_equal(got["tally"], exp["tally"]) and np.array_equal(got["lengths"], exp["lengths"])


def test_round_trip_generate_ubam_report(tmp_path):
    """What `report --bam` says of the unaligned BAM of a run is what `generate --report` said of the run, but for the insert sizes."""
    from insilicoseq_amd.tally import split_tally

    fasta = str(tmp_path / "genomes.fasta")
    with open(fasta, "w") as fh:
        for k in range(3):
            fh.write(">rec%d\n%s\n" % (k, mixed_genome(121 + k, 5000 + 1000 * k)))
    x, y = str(tmp_path / "X"), str(tmp_path / "Y")
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", "2000",
                    "--seed", "5", "--ubam", "--report", "--output", x], cwd=ROOT, check=True, timeout=600)
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "report", "--quiet", "--bam", x + ".bam", "-o", y, "--against", x + "_tally.npy"],
                   cwd=ROOT, check=True, timeout=600)
    tx, ty = split_tally(np.load(x + "_tally.npy"), 151), split_tally(np.load(y + "_tally.npy"), 151)
    assert int(tx["pairs"][0]) == 1000 and tx["insert"].any() and not ty["insert"].any()  # (unmapped records have no template)
    for field in ("pairs", "qual", "base", "gc", "meanq"):
        assert np.array_equal(tx[field], ty[field]), field
    lengths = np.load(y + "_lengths.npy")
    assert lengths.shape == (2, 152) and lengths[:, 151].tolist() == [1000, 1000] and not lengths[:, :151].any()
    compare = json.load(open(y + "_compare.json"))
    assert compare["summary"] == {"max_abs_mean_phred_diff": 0.0, "max_base_l1": 0.0, "max_gc_tv": 0.0, "max_meanq_tv": 0.0,
                                  "insert_tv": None}
    report = json.load(open(y + "_report.json"))
    assert report["pairs"] == 1000 and report["records_skipped"] == {"secondary_or_supplementary": 0, "mate_flags": 0}
    assert report["mates"] == json.load(open(x + "_report.json"))["mates"]


def test_round_trip_both_inflate_routes(tmp_path):
    from insilicoseq_amd.bam_report import bam_reads_host, finish

    records = bam_synth.records(131, n_pairs=300)
    path = str(tmp_path / "a.bam")
    bam_synth.write_records(path, records)
    exp = finish(bam_reads_host(BC.chunk_of(records), 1024), 1024)
    env = {k: v for k, v in os.environ.items() if k not in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE")}
    outs = []
    for tag, extra in (("host", []), ("device", ["--device_inflate"])):
        out = str(tmp_path / tag)
        subprocess.run([sys.executable, "-m", "insilicoseq_amd", "report", "--quiet", "--bam", path, "-o", out] + extra, cwd=ROOT, check=True,
                       timeout=600, env=env)
        outs.append([open(out + suffix, "rb").read() for suffix in ("_tally.npy", "_lengths.npy", "_report.json")])
    assert outs[0] == outs[1]
    words = np.load(str(tmp_path / "host_tally.npy"))
    assert np.array_equal(words, exp["tally"]) and np.array_equal(np.load(str(tmp_path / "host_lengths.npy")), exp["lengths"])
    report = json.load(open(str(tmp_path / "host_report.json")))
    assert sum(report["insert_size_histogram"]) > 0
    assert report["records_skipped"] == {"secondary_or_supplementary": exp["skipped"][0], "mate_flags": exp["skipped"][1]}
