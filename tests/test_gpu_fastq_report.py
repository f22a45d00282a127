"""`report`: the tallies of FASTQ text built on the device (iss_fq_*: k_fq_count, k_fq_head, k_fq_lines, k_fq_records, k_fq_positions)
against the numpy twin (insilicoseq_amd.fastq_report.fastq_tally_host), word for word, with the records seen and the first bad
record; the chunk contract, the launch geometry, the error paths and the round trip `generate --report` -> `report`."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import fastq_cases as FC
from helpers import mixed_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEWLINE_TILE = 4096  # FQ_TILE of csrc/iss_fqtally.hip.h

_contexts = {}


def _context(max_len):
    """One context per max_len for the whole module, reset before every use."""
    from insilicoseq_amd.fastq_report import FastqTally

    if max_len not in _contexts:
        _contexts[max_len] = FastqTally(0, max_len)
    _contexts[max_len].reset()
    return _contexts[max_len]


def _device(feeds, max_len):
    """feeds: (mate, bytes) in feed order -> the download."""
    dev = _context(max_len)
    for mate, chunk in feeds:
        dev.feed(chunk, mate)
    return dev.download()


def _twin(feeds, max_len):
    from insilicoseq_amd.fastq_report import fastq_tally_host

    return fastq_tally_host([c for m, c in feeds if m == 0], [c for m, c in feeds if m == 1], max_len)


def _same(got, exp, max_len):
    from insilicoseq_amd.fastq_report import split_fq_words

    assert got["records"] == exp["records"]
    assert got["bad_record"] == exp["bad_record"] and got["bad_code"] == exp["bad_code"]
    g, e = split_fq_words(got["tally"], max_len), split_fq_words(exp["tally"], max_len)
    assert [k for k in g if not np.array_equal(g[k], e[k])] == []  # (the fields that differ)


def _check(feeds, max_len):
    got, exp = _device(feeds, max_len), _twin(feeds, max_len)
    _same(got, exp, max_len)
    return got


def _chunks_of(text, n_records):
    lines = text.split(b"\n")[:-1]
    return [b"\n".join(lines[k:k + 4 * n_records]) + b"\n" for k in range(0, len(lines), 4 * n_records)]


@pytest.mark.parametrize("lengths,max_len", [(FC.LENGTHS, 1024), (FC.LENGTHS[:-1], 301), (FC.LENGTHS[:-1], 1024)])
def test_mixed_lengths(lengths, max_len):
    from insilicoseq_amd.fastq_report import split_fq_words

    got = _check([(0, FC.mixed(200, 11, lengths)), (1, FC.mixed(200, 12, lengths))], max_len)
    t = split_fq_words(got["tally"], max_len)
    assert got["records"] == [200, 200] and got["bad_record"] == [-1, -1] and int(t["pairs"][0]) == 200
    assert all(int(t["length"][m][n]) > 0 for m in range(2) for n in lengths) and int(t["length"].sum()) == 400
    assert not t["insert"].any()
    assert t["qual"][:, :, 0].any() and t["qual"][:, :, 93].any()        # '!' and '~': the first and the last bin
    assert t["base"][:, :, 4].any() and (t["base"].sum(axis=1) > 0).all()  # N and IUPAC letters; every code in both cases
    assert int(t["qual"][0, max(lengths) - 1].sum()) == int(t["length"][0][max(lengths)])  # the last position: the longest reads


@pytest.mark.parametrize("n_records", [1, 63, 64, 65, 1000])
def test_record_counts(n_records):
    got = _check([(0, FC.mixed(n_records, 20 + n_records, (0, 1, 63, 64, 65, 151)))], 151)
    assert got["records"] == [n_records, 0]


@pytest.mark.parametrize("wgs", ["1", "3", "4096"])
def test_launch_geometry(wgs, monkeypatch):
    feeds = [(0, FC.mixed(300, 31, (0, 1, 63, 64, 65, 151, 301))), (1, FC.mixed(300, 32, (151,)))]
    plain = _device(feeds, 301)
    monkeypatch.setenv("ISS_FQTALLY_WGS", wgs)
    forced = _check(feeds, 301)
    assert np.array_equal(plain["tally"], forced["tally"])


@pytest.mark.parametrize("read_length", [100, 1])
def test_lines_straddle_every_newline_tile(read_length):
    text = FC.sized(3 * NEWLINE_TILE + 5, 41, read_length)
    assert len(text) == 3 * NEWLINE_TILE + 5 and all(text[k * NEWLINE_TILE - 1] != 10 for k in (1, 2, 3))
    _check([(0, text)], 128)


def test_only_newlines():
    """As many lines as bytes: the line table at its largest; every record is bad (no '@')."""
    got = _check([(0, b"\n" * (2 * NEWLINE_TILE + 8))], 16)
    assert got["records"] == [(2 * NEWLINE_TILE + 8) // 4, 0] and got["bad_record"][0] == 0 and got["bad_code"][0] == 1
    assert not got["tally"].any()


def test_crlf():
    from insilicoseq_amd.fastq_report import split_fq_words

    lf, crlf = FC.mixed(100, 51), FC.mixed(100, 51, eol=b"\r\n")
    assert crlf.count(b"\r\n") == 400 and len(crlf) == len(lf) + 400
    got = _check([(0, crlf)], 1024)
    assert np.array_equal(got["tally"], _device([(0, lf)], 1024)["tally"])
    assert int(split_fq_words(got["tally"], 1024)["length"][0][0]) > 0  # (an empty read's line is the '\r' alone)


def test_quality_lines_starting_with_at_and_plus():
    recs = [(b"r%d" % k, b"ACGTN", q) for k, q in enumerate((b"@@@@@", b"+++++", b"@+@+@", b"+@!~I"))]
    got = _check([(0, FC.text(recs))], 8)
    assert got["records"] == [4, 0] and got["bad_record"] == [-1, -1]


def test_chunking_does_not_change_the_words():
    text = FC.mixed(101, 61, (0, 1, 63, 64, 65, 151, 301))
    whole = _check([(0, text)], 301)
    for per in (4, 1):
        chunks = _chunks_of(text, per)
        assert b"".join(chunks) == text and len(chunks) == -(-101 // per)
        got = _check([(0, c) for c in chunks], 301)
        assert np.array_equal(got["tally"], whole["tally"]) and got["records"] == [101, 0]


def test_buffers_grow_in_the_middle_of_a_pipeline():
    """A fresh context, so that nothing has grown before: the second and the fourth feed pass the 1 MiB floor of their slot and of the
    work arrays while the feed before them is still in flight (the module's shared contexts only ever grow on their first feed)."""
    from insilicoseq_amd.fastq_report import FastqTally

    feeds = [(k % 2, FC.mixed(n, 120 + k, (151,))) for k, n in enumerate((8, 4000, 8, 8000, 8))]
    assert len(feeds[0][1]) < 4096 and (1 << 20) < len(feeds[1][1]) < (1 << 21) < len(feeds[3][1])
    with FastqTally(0, 151) as dev:
        for mate, chunk in feeds:
            dev.feed(chunk, mate)
        got = dev.download()
    _same(got, _twin(feeds, 151), 151)
    assert got["records"] == [24, 12000] and got["bad_record"] == [-1, -1]
    small = _device([(mate, c) for mate, chunk in feeds for c in _chunks_of(chunk, 16)], 151)
    assert np.array_equal(small["tally"], got["tally"]) and small["records"] == got["records"]


def test_two_mates_interleaved():
    from insilicoseq_amd.fastq_report import split_fq_words

    r1, r2 = _chunks_of(FC.mixed(90, 71, (100, 151)), 16), _chunks_of(FC.mixed(90, 72, (0, 75, 151)), 16)
    feeds = [f for pair in zip(r1, r2) for f in ((0, pair[0]), (1, pair[1]))]
    got = _check(feeds, 151)
    t = split_fq_words(got["tally"], 151)
    assert got["records"] == [90, 90] and int(t["length"][0].sum()) == 90 and int(t["length"][1][75]) > 0 and int(t["length"][0][75]) == 0
    one_after_the_other = _device([f for f in feeds if f[0] == 1] + [f for f in feeds if f[0] == 0], 151)
    assert np.array_equal(got["tally"], one_after_the_other["tally"])


def test_reset():
    text = FC.mixed(50, 81, (10, 151))
    dev = _context(151)
    dev.feed(b"@bad\nAC\n+\nI\n" + text, 0)
    dev.feed(text, 1)
    first = dev.download()
    assert first["records"] == [51, 50] and first["bad_record"] == [0, -1]
    assert dev.kernel_ms() > 0.0  # (HIP events around the two feeds' launches)
    dev.reset()
    zero = dev.download()
    assert dev.kernel_ms() == 0.0
    assert not zero["tally"].any() and zero["records"] == [0, 0] and zero["bad_record"] == [-1, -1] and zero["bad_code"] == [0, 0]
    dev.feed(text, 0)
    _same(dev.download(), _twin([(0, text)], 151), 151)


def _bad_text(n, k, code, seed):
    """n records of length 40, record k spoiled for `code` (1 .. 5)."""
    recs = FC.records([40] * n, seed)
    parts = []
    for i, (name, bases, quals) in enumerate(recs):
        head, plus = b"@" + name, b"+"
        if i == k:
            if code == 1:
                head = name            # no '@'
            elif code == 2:
                plus = b"-"
            elif code == 3:
                quals = quals[:-1]
            elif code == 4:
                bases, quals = bases * 2, quals * 2  # 80 > max_len 64
            elif code == 5:
                quals = quals[:20] + (b" " if seed % 2 else b"\x7f") + quals[21:]
        parts.append(b"\n".join((head, bases, plus, quals)) + b"\n")
    return b"".join(parts)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("code", [1, 2, 3, 4, 5])
def test_bad_record_codes(code, where):
    from insilicoseq_amd.fastq_report import split_fq_words

    n = 130
    k = {"first": 0, "middle": 64, "last": n - 1}[where]
    got = _check([(1, _bad_text(n, k, code, 90 + code))], 64)
    assert got["records"] == [0, n] and got["bad_record"] == [-1, k] and got["bad_code"] == [0, code]
    assert int(split_fq_words(got["tally"], 64)["length"][1][40]) == n - 1  # the good records beside it are tallied


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_truncated(where):
    from insilicoseq_amd.fastq_report import split_fq_words

    good = FC.mixed(20, 101, (40,))
    cut = {"first": [b"@r\nACGT\n", good, good], "middle": [good, good[:-1], good], "last": [good, good, good + b"@r\nAC\n+\n"]}[where]
    got = _check([(0, c) for c in cut], 64)
    index = {"first": 0, "middle": 39, "last": 60}[where]
    assert got["bad_record"] == [index, -1] and got["bad_code"] == [6, 0]
    # a chunk without its last '\n' has one whole record less: its last line is not a line
    whole = {"first": 40, "middle": 59, "last": 60}[where]
    assert got["records"] == [whole, 0] and int(split_fq_words(got["tally"], 64)["length"][0][40]) == whole


def test_first_bad_record_wins():
    a, b = _bad_text(130, 100, 5, 7), _bad_text(130, 30, 3, 8)
    got = _check([(0, a), (0, b)], 64)
    assert got["bad_record"] == [100, -1] and got["bad_code"] == [5, 0]
    got = _check([(0, b), (0, a)], 64)
    assert got["bad_record"] == [30, -1] and got["bad_code"] == [3, 0]
    lines = _bad_text(130, 7, 2, 9).split(b"\n")
    lines[4 * 7] = lines[4 * 7][1:]  # record 7: no '+' and no '@' -- the smallest code that applies
    got = _check([(0, b"\n".join(lines))], 64)
    assert got["bad_record"] == [7, -1] and got["bad_code"] == [1, 0]


def test_invalid_arguments_launch_nothing():
    from insilicoseq_amd import _native

    lib = _native.lib()
    dev = _context(64)
    text = FC.mixed(4, 111, (40,))
    for mate, ptr, n in ((2, text, len(text)), (-1, text, len(text)), (0, text, -1), (0, text, 1 << 31), (0, None, 5)):
        assert lib.iss_fq_feed(dev._h, mate, ptr, n) == _native.E_INVALID
        assert b"iss_fq_feed" in lib.iss_fq_last_error(dev._h)
    assert lib.iss_fq_feed(dev._h, 0, None, 0) == 0 and lib.iss_fq_feed(dev._h, 1, text, 0) == 0
    got = dev.download()
    assert not got["tally"].any() and got["records"] == [0, 0] and got["bad_record"] == [-1, -1]
    h = C.c_void_p()
    for max_len in (0, -1, 1025):
        assert lib.iss_fq_create(0, max_len, C.byref(h)) == _native.E_INVALID and not h
    assert lib.iss_fq_create(99, 64, C.byref(h)) == _native.E_INVALID and not h
    assert lib.iss_fq_create(1 << 20, 64, C.byref(h)) == _native.E_INVALID and not h
    assert b"device ordinal out of range" in lib.iss_fq_last_error(None)
    assert lib.iss_fq_tally_words(None) == -1 and lib.iss_fq_tally_words(dev._h) == 1 + 64 * 200 + 2 + 188 + 2048 + 2 * 65
    rec, bad, code = (C.c_int64 * 2)(), (C.c_int64 * 2)(), (C.c_int32 * 2)()
    assert lib.iss_fq_download(dev._h, None, C.addressof(rec), C.addressof(bad), C.addressof(code)) == _native.E_INVALID
    assert lib.iss_fq_reset(None) == _native.E_INVALID and lib.iss_fq_kernel_ms(dev._h, None) == _native.E_INVALID


def test_feed_file_and_result(tmp_path):
    """FastqTally.feed_file over small chunks, plain and multi-member gzip, and result(): the words at the longest read seen."""
    import gzip

    from insilicoseq_amd.fastq_report import FastqTally, fastq_tally_host, finish

    r1, r2 = FC.mixed(120, 121, (0, 30, 75)), FC.mixed(120, 122, (75,))
    p1, p2 = str(tmp_path / "a_R1.fastq"), str(tmp_path / "a_R2.fastq.gz")
    open(p1, "wb").write(r1[:-1])  # (no final newline)
    with open(p2, "wb") as fh:
        for k in range(0, len(r2), 1000):
            fh.write(gzip.compress(r2[k:k + 1000]))
    exp = finish(fastq_tally_host(r1, r2, 1024), 1024)
    with FastqTally(0) as dev:
        dev.feed_file(p1, 0, chunk_bytes=777)
        dev.feed_file(p2, 1, chunk_bytes=4096)
        got = dev.result()
    assert got["read_length"] == 75 and got["records"] == [120, 120] and got["bad_record"] == [-1, -1]
    assert np.array_equal(got["tally"], exp["tally"]) and np.array_equal(got["lengths"], exp["lengths"])
    assert got["tally"].size == 200 * 75 + 2239 and got["lengths"].shape == (2, 76)


@pytest.mark.parametrize("compress", [False, True])
def test_round_trip_generate_report(tmp_path, compress):
    """The feature's point: what `report` says of the files of a run is what `generate --report` said of the run."""
    from insilicoseq_amd.tally import split_tally

    fasta = str(tmp_path / "genomes.fasta")
    with open(fasta, "w") as fh:
        for k in range(3):
            fh.write(">rec%d\n%s\n" % (k, mixed_genome(121 + k, 5000 + 1000 * k)))
    x, y = str(tmp_path / "X"), str(tmp_path / "Y")
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", "2000",
                    "--seed", "5", "--report", "--output", x] + (["--compress"] if compress else []), cwd=ROOT, check=True, timeout=600)
    suffix = ".fastq.gz" if compress else ".fastq"
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "report", "--quiet", "-1", x + "_R1" + suffix, "-2", x + "_R2" + suffix,
                    "-o", y, "--against", x + "_tally.npy"], cwd=ROOT, check=True, timeout=600)
    tx, ty = split_tally(np.load(x + "_tally.npy"), 151), split_tally(np.load(y + "_tally.npy"), 151)
    assert int(tx["pairs"][0]) == 1000 and tx["insert"].any() and not ty["insert"].any()
    for field in ("pairs", "qual", "base", "gc", "meanq"):
        assert np.array_equal(tx[field], ty[field]), field
    lengths = np.load(y + "_lengths.npy")
    assert lengths.shape == (2, 152) and lengths[:, 151].tolist() == [1000, 1000] and not lengths[:, :151].any()
    compare = json.load(open(y + "_compare.json"))
    assert compare["summary"] == {"max_abs_mean_phred_diff": 0.0, "max_base_l1": 0.0, "max_gc_tv": 0.0, "max_meanq_tv": 0.0,
                                  "insert_tv": None}
    report = json.load(open(y + "_report.json"))
    assert report["pairs"] == 1000 and report["read_length"] == 151 and report["read_length_histogram"] == [[0] * 151 + [1000]] * 2
    assert report["mates"] == json.load(open(x + "_report.json"))["mates"]
