"""`report` without a GPU (insilicoseq_amd.fastq_report, app.report_from_fastq): the numpy twin of the device tallies against a tally
worked out by hand and against tally.tally_host on the FASTQ text of a golden run, the host side of the chunk contract, gzip
input, the re-layout to the longest read seen, compare_tallies, and the command line with the binding stubbed."""
import gzip
import io
import json
import os

import numpy as np
import pytest

import fastq_cases as FC
from insilicoseq_amd import fastq_report as F
from insilicoseq_amd.tally import split_tally, tally_host, tally_words

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate")


def _parse(text):
    lines = text.split(b"\n")
    n = len(lines) // 4
    return (np.stack([np.frombuffer(lines[4 * k + 1], dtype=np.uint8) for k in range(n)]),
            np.stack([np.frombuffer(lines[4 * k + 3], dtype=np.uint8) for k in range(n)]))


def test_twin_against_a_hand_computed_tally():
    """fastq_cases.SIX at max_len 8.  Good records (bases; phreds): 0 ACGT; 31 40 40 40 -- 1 GGCC; 0 0 0 93 (CRLF) -- 2 AC; 10 20
    -- 3 empty -- 5 acgNn; 20 20 20 20 93.  Record 4 has four bases and three qualities: LENGTHS, not tallied."""
    res = F.fastq_tally_host(FC.SIX, None, 8)
    assert res["records"] == [6, 0] and res["bad_record"] == [4, -1] and res["bad_code"] == [F.REC_LENGTHS, 0]
    t = F.split_fq_words(res["tally"], 8)
    exp = F.split_fq_words(np.zeros(F.fq_words(8), dtype=np.uint64), 8)
    exp["pairs"][0] = 5
    for pos, phreds in enumerate(((31, 0, 10, 20), (40, 0, 20, 20), (40, 0, 20), (40, 93, 20), (93,))):
        for ph in phreds:
            exp["qual"][0, pos, ph] += 1
    for pos, codes in enumerate(((0, 2, 0, 0), (1, 2, 1, 1), (2, 1, 2), (3, 1, 4), (4,))):  # A C G T other = 0 .. 4
        for c in codes:
            exp["base"][0, pos, c] += 1
    np.add.at(exp["gc"][0], [2, 4, 1, 0, 2], 1)          # G / C letters of records 0, 1, 2, 3, 5
    np.add.at(exp["meanq"][0], [151 // 4, 93 // 4, 30 // 2, 173 // 5], 1)  # (the empty read has no mean)
    np.add.at(exp["length"][0], [4, 4, 2, 0, 5], 1)
    for field in exp:
        assert np.array_equal(t[field], exp[field]), field
    assert res["tally"].size == tally_words(8) + 2 * 9 and not t["insert"].any() and not t["length"][1].any()


@pytest.mark.parametrize("case", ["genomes_hiseq_n600_seed42_cpus1", "syn3_novaseq_n3000_seed7_cpus8"])
def test_twin_on_a_golden_run_equals_tally_host(case):
    z = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    r1, r2 = z["r1"].tobytes(), z["r2"].tobytes()
    (b1, q1), (b2, q2) = _parse(r1), _parse(r2)
    n, L = b1.shape
    res = F.finish(F.fastq_tally_host(r1, r2), F.MAX_LEN)
    assert res["read_length"] == L and res["records"] == [n, n] and res["bad_record"] == [-1, -1]
    assert res["lengths"][:, L].tolist() == [n, n] and int(res["lengths"].sum()) == 2 * n
    ref = split_tally(tally_host(np.stack([b1, b2], axis=1), np.stack([q1, q2], axis=1) - 33, np.zeros(n, dtype=np.int64), L), L)
    got = split_tally(res["tally"], L)
    for field in ("pairs", "qual", "base", "gc", "meanq"):
        assert np.array_equal(got[field], ref[field]), field
    assert not got["insert"].any()


TRICKY = (b"@a\r\nACGT\r\n+\r\n@III\r\n"   # CRLF; a quality line starting with '@'
          b"@b\r\nAC\r\n+b\r\n+5\r\n"      # one starting with '+'
          b"@c\r\n\r\n+\r\n\r\n"
          b"@d\r\nGGGGGGGG\r\n+\r\n@+@+@+@+\r\n"
          b"@e\r\nN\r\n+\r\n~")             # no final newline


@pytest.mark.parametrize("chunk_bytes", [1, 2, 7, 64, 4096])
def test_split_chunks(chunk_bytes):
    chunks = list(F.split_chunks(io.BytesIO(TRICKY), chunk_bytes))
    assert b"".join(chunks) == TRICKY + b"\n"
    for c in chunks:
        assert c.endswith(b"\n") and c.count(b"\n") % 4 == 0 and c.count(b"\n") >= 4
    assert len(chunks) == {1: 5, 2: 5, 7: 5, 64: 2, 4096: 1}[chunk_bytes]  # (a chunk as soon as a record is whole)
    whole, fed = F.fastq_tally_host(TRICKY + b"\n", None, 8), F.fastq_tally_host(chunks, None, 8)
    assert fed["records"] == [5, 0] and fed["bad_record"] == [-1, -1] and np.array_equal(fed["tally"], whole["tally"])


def test_split_chunks_leaves_a_truncated_record_last():
    text = TRICKY + b"\n@f\nACGT\n+"
    chunks = list(F.split_chunks(io.BytesIO(text), 16))
    assert b"".join(chunks) == text + b"\n" and chunks[-1] == b"@f\nACGT\n+\n" and all(c.count(b"\n") % 4 == 0 for c in chunks[:-1])
    res = F.fastq_tally_host(chunks, None, 8)
    assert res["records"] == [5, 0] and res["bad_record"] == [5, -1] and res["bad_code"] == [F.REC_TRUNCATED, 0]
    assert list(F.split_chunks(io.BytesIO(b""), 16)) == []


def test_multi_member_gzip(tmp_path):
    text = FC.mixed(40, 3, (0, 10, 75))
    path = str(tmp_path / "reads.fastq.gz")
    with open(path, "wb") as fh:
        for k in range(0, len(text), 500):  # members cut anywhere, as `generate --compress` writes one per batch
            fh.write(gzip.compress(text[k:k + 500]))
    with F.open_fastq(path) as fh:
        chunks = list(F.split_chunks(fh, 333))
    assert b"".join(chunks) == text and len(chunks) > 5
    plain = str(tmp_path / "reads.fastq")
    open(plain, "wb").write(text)
    with F.open_fastq(plain) as fh:
        assert fh.read() == text


def test_relayout_to_the_longest_read_seen():
    r1, r2 = FC.mixed(30, 5, (0, 7, 20)), FC.mixed(30, 6, (20,))
    at64, at20 = F.fastq_tally_host(r1, r2, 64), F.fastq_tally_host(r1, r2, 20)
    assert F.longest_read(at64["tally"], 64) == 20
    words, lengths = F.relayout(at64["tally"], 64, 20)
    assert words.size == tally_words(20) and lengths.shape == (2, 21)
    same, same_lengths = F.relayout(at20["tally"], 20, 20)
    assert np.array_equal(words, same) and np.array_equal(lengths, same_lengths)
    assert np.array_equal(same, at20["tally"][:tally_words(20)]) and int(lengths[1, 20]) == 30
    res = F.finish(at64, 64)
    assert res["read_length"] == 20 and np.array_equal(res["tally"], words)
    with pytest.raises(ValueError):
        F.relayout(at64["tally"], 64, 19)  # would cut reads off
    empty = F.finish(F.fastq_tally_host(b"", None, 64), 64)
    assert empty["read_length"] == 1 and empty["records"] == [0, 0] and not empty["tally"].any()
    assert [F.read_length_of_words(tally_words(L)) for L in (1, 20, 151, 1024)] == [1, 20, 151, 1024]
    assert F.read_length_of_words(tally_words(20) + 1) is None and F.read_length_of_words(2239) is None


def _tally_of(r1, r2, max_len=64):
    res = F.finish(F.fastq_tally_host(r1, r2, max_len), max_len)
    return res["tally"], res["read_length"]


def test_compare_tallies():
    a, La = _tally_of(FC.mixed(60, 7, (30,)), FC.mixed(60, 8, (30,)))
    same = F.compare_tallies(a, La, a, La)
    json.dumps(same)
    assert same["positions"] == 30 and same["summary"] == {"max_abs_mean_phred_diff": 0.0, "max_base_l1": 0.0, "max_gc_tv": 0.0,
                                                          "max_meanq_tv": 0.0, "insert_tv": None}  # (no insert sizes in a FASTQ file)
    assert all(x == 0.0 for m in same["mates"] for x in m["mean_phred_diff"] + m["base_l1"])
    # insert sizes on both sides: a distance; on one side only: None
    with_insert, other = a.copy(), a.copy()
    split_tally(with_insert, La)["insert"][[100, 200]] = 5
    split_tally(other, La)["insert"][[100, 300]] = 5
    assert F.compare_tallies(with_insert, La, other, La)["insert_tv"] == 0.5
    assert F.compare_tallies(with_insert, La, with_insert, La)["summary"]["insert_tv"] == 0.0
    assert F.compare_tallies(with_insert, La, a, La)["insert_tv"] is None
    # different read lengths: the first 20 positions; reads of G and C alone have GC fraction 1 at either length
    gc = lambda n, L: FC.text([(b"r%d" % k, b"GC" * (L // 2), b"I" * L) for k in range(n)])  # noqa: E731
    b, Lb = _tally_of(gc(10, 20), None)
    c, Lc = _tally_of(gc(10, 30), None)
    cmp = F.compare_tallies(b, Lb, c, Lc)
    assert (Lb, Lc) == (20, 30) and cmp["positions"] == 20 and cmp["read_lengths"] == [20, 30] and cmp["pairs"] == [10, 10]
    assert cmp["mates"][0]["gc_tv"] == 0.0 and cmp["mates"][0]["meanq_tv"] == 0.0 and cmp["mates"][0]["mean_phred_diff"] == [0.0] * 20
    assert cmp["mates"][1] == {"mean_phred_diff": [None] * 20, "base_l1": [None] * 20, "gc_tv": None, "meanq_tv": None}  # no mate 2
    at = lambda L: FC.text([(b"r%d" % k, b"AT" * (L // 2), b"I" * L) for k in range(10)])  # noqa: E731
    d, Ld = _tally_of(at(30), None)
    far = F.compare_tallies(b, Lb, d, Ld)
    assert far["mates"][0]["gc_tv"] == 1.0 and far["mates"][0]["base_l1"] == [2.0] * 20 and far["summary"]["max_base_l1"] == 2.0


def test_compare_tallies_shows_a_shift_where_it_is():
    """Every mate-1 read one phred lower at position 7: -1 there, 0 everywhere else (10 reads of one quality each way)."""
    recs = FC.records([30] * 10, 9)
    a, L = _tally_of(FC.text(recs), None)
    shifted = [(name, bases, quals[:7] + bytes([max(quals[7] - 1, 33)]) + quals[8:]) for name, bases, quals in recs]
    assert all(q[7] > 33 for _, _, q in recs)
    b, _ = _tally_of(FC.text(shifted), None)
    cmp = F.compare_tallies(b, L, a, L)
    diff = cmp["mates"][0]["mean_phred_diff"]
    assert diff[7] == pytest.approx(-1.0, abs=1e-12) and all(x == 0.0 for k, x in enumerate(diff) if k != 7)
    assert cmp["summary"]["max_abs_mean_phred_diff"] == pytest.approx(1.0, abs=1e-12) and cmp["summary"]["max_base_l1"] == 0.0
    assert cmp["summary"]["max_gc_tv"] == 0.0


def test_parser_has_report():
    from insilicoseq_amd.app import build_parser

    args = build_parser().parse_args(["report", "-1", "a_R1.fastq.gz", "-2", "a_R2.fastq.gz", "-o", "out", "--against", "run_tally.npy",
                                      "--max_length", "301", "--device", "2", "--quiet"])
    assert (args.cmd, args.read1, args.read2, args.output, args.against, args.max_length, args.device, args.quiet) == (
        "report", "a_R1.fastq.gz", "a_R2.fastq.gz", "out", "run_tally.npy", 301, 2, True)
    args = build_parser().parse_args(["report", "-1", "a.fastq", "-o", "out"])
    assert (args.read2, args.against, args.max_length, args.device, args.quiet) == (None, None, 1024, 0, False)


class FakeTally:
    """FastqTally with the twin in the device's place."""

    def __init__(self, device=0, max_len=F.MAX_LEN):
        self.max_len, self.feeds = max_len, ([], [])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def feed_file(self, path, mate, chunk_bytes=64 << 20):
        with F.open_fastq(path) as fh:
            self.feeds[mate].extend(F.split_chunks(fh, 1000))

    def result(self):
        return F.finish(F.fastq_tally_host(self.feeds[0], self.feeds[1], self.max_len), self.max_len)


@pytest.fixture
def cli(monkeypatch, tmp_path):
    from insilicoseq_amd import app

    monkeypatch.setattr(F, "FastqTally", FakeTally)

    def run(r1, r2=None, extra=()):
        paths = []
        for tag, text in (("R1", r1), ("R2", r2)):
            if text is not None:
                paths.append(str(tmp_path / ("in_%s.fastq" % tag)))
                open(paths[-1], "wb").write(text)
        argv = ["report", "--quiet", "-1", paths[0]] + (["-2", paths[1]] if r2 is not None else []) + ["-o", str(tmp_path / "out")]
        return app.main(argv + list(extra)), paths

    return run


def test_cli_writes_its_files(cli, tmp_path, capsys):
    r1, r2 = FC.mixed(40, 13, (0, 20, 50)), FC.mixed(40, 14, (50,))
    other = str(tmp_path / "other_tally.npy")
    np.save(other, _tally_of(r1, r2, 1024)[0])
    rc, _ = cli(r1, r2, ["--against", other])
    assert rc == 0 and capsys.readouterr().err == ""
    out = str(tmp_path / "out")
    words, lengths = np.load(out + "_tally.npy"), np.load(out + "_lengths.npy")
    assert words.size == tally_words(50) and lengths.shape == (2, 51) and lengths.sum(axis=1).tolist() == [40, 40]
    report = json.load(open(out + "_report.json"))
    assert report["pairs"] == 40 and report["read_length"] == 50 and report["read_length_histogram"][1] == [0] * 50 + [40]
    assert sum(report["read_length_histogram"][0]) == 40 and report["insert_size_histogram"] == []
    assert json.load(open(out + "_compare.json"))["summary"]["max_base_l1"] == 0.0
    # without -2 mate 2's fields are zero, and nothing is compared without --against
    os.remove(out + "_compare.json")
    rc, _ = cli(r1)
    t = split_tally(np.load(out + "_tally.npy"), 50)
    assert rc == 0 and int(t["pairs"][0]) == 40 and not t["qual"][1].any() and not t["gc"][1].any() and not np.load(out + "_lengths.npy")[1].any()
    assert not os.path.exists(out + "_compare.json")


def test_cli_unequal_record_counts(cli, tmp_path, capsys):
    rc, paths = cli(FC.mixed(12, 15, (20,)), FC.mixed(11, 16, (20,)))
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: ") and err.count("\n") == 1 and "12 records" in err and "holds 11" in err
    assert paths[0] in err and paths[1] in err and not os.path.exists(str(tmp_path / "out_tally.npy"))


def test_cli_word_count_that_fits_no_read_length(cli, tmp_path, capsys):
    other = str(tmp_path / "other_tally.npy")
    np.save(other, np.zeros(tally_words(50) + 3, dtype=np.uint64))
    rc, _ = cli(FC.mixed(4, 17, (20,)), None, ["--against", other])
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + other) and err.count("\n") == 1 and "fit no read length" in err
    assert not os.path.exists(str(tmp_path / "out_tally.npy"))


def test_cli_names_a_bad_record(cli, tmp_path, capsys):
    text = FC.mixed(9, 18, (20,))
    rc, paths = cli(text, text.replace(b"\n+\n", b"\n-\n", 6).replace(b"\n-\n", b"\n+\n", 5))  # record 5 of R2: no '+'
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + paths[1] + ": record 5: ") and "'+'" in err and err.count("\n") == 1
    rc, paths = cli(text[:-5])
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + paths[0] + ": record 8: ") and "the bases and the quality line differ" in err
    rc, paths = cli(text + b"@r\nAC\n")
    assert rc == 1 and capsys.readouterr().err.startswith("ERROR: " + paths[0] + ": record 9: truncated record")
