"""`report --bam` without a GPU (insilicoseq_amd.bam_report, app.report_from_fastq): the numpy twin of the device tallies against a
tally worked out by hand, against fastq_tally_host on the FASTQ text the records stand for, every insert rule, chunking, and the
command line with the twin in the device's place."""
import json
import os

import numpy as np
import pytest

import bam_report_cases as BC
import bam_synth
from insilicoseq_amd import bam_report as B
from insilicoseq_amd import fastq_report as F
from insilicoseq_amd.bam import BamReader
from insilicoseq_amd.tally import split_tally, tally_words


def _empty(max_len):
    return F.split_fq_words(np.zeros(F.fq_words(max_len), dtype=np.uint64), max_len)


EIGHT = [
    BC.rec("ACGTN", [10, 20, 30, 40, 0], BC.R1F, tlen=20),        # 0  forward, mate 0; insert 20 - 10
    BC.rec("AAC", [1, 2, 3], BC.R2R),                              # 1  reverse, odd length, mate 1: as sequenced GTT; 3 2 1
    BC.rec("=N", [93, 0], 0, tlen=500),                            # 2  unpaired: mate 0, no insert
    BC.rec("ACGT", [30] * 4, BC.R1F | 0x100, tlen=20),             # 3  secondary
    BC.rec("ACGT", [30] * 4, 0xC1, tlen=20),                       # 4  first and second read at once
    BC.rec("", [], BC.R1F),                                        # 5  zero-length
    BC.rec("ACGT", [30, 30, 94, 30], BC.R1F, tlen=20),             # 6  bad: a quality above 93
    BC.rec("GC=A", [5, 6, 7, 8], BC.R1R, tlen=-9),                 # 7  reverse, mate 0: as sequenced T=GC; 8 7 6 5; insert 9 - 8
]


def test_twin_against_a_hand_computed_tally():
    res = B.bam_reads_host(BC.chunk_of(EIGHT), 8)
    assert res["records"] == [4, 1] and res["skipped"] == [1, 1] and (res["bad_record"], res["bad_code"]) == (6, B.REC_QUAL_RANGE)
    exp = _empty(8)
    exp["pairs"][0] = 4
    for pos, phreds in enumerate(((10, 93, 8), (20, 0, 7), (30, 6), (40, 5), (0,))):
        for ph in phreds:
            exp["qual"][0, pos, ph] += 1
    for pos, codes in enumerate(((0, 4, 3), (1, 4, 4), (2, 2), (3, 1), (4,))):  # A C G T other = 0 .. 4
        for c in codes:
            exp["base"][0, pos, c] += 1
    for pos, (ph, c) in enumerate(((3, 2), (2, 3), (1, 3))):
        exp["qual"][1, pos, ph] += 1
        exp["base"][1, pos, c] += 1
    np.add.at(exp["gc"][0], [2, 0, 0, 2], 1)    # records 0, 2, 5, 7
    exp["gc"][1, 1] = 1
    np.add.at(exp["meanq"][0], [20, 46, 6], 1)  # 100 // 5, 93 // 2, 26 // 4; the empty read has no mean
    exp["meanq"][1, 2] = 1
    np.add.at(exp["length"][0], [5, 2, 0, 4], 1)
    exp["length"][1, 3] = 1
    exp["insert"][10] = exp["insert"][1] = 1
    got = F.split_fq_words(res["tally"], 8)
    for name in exp:
        assert np.array_equal(got[name], exp[name]), name


def test_complement_is_the_bit_reversal():
    letters = "=ACMGRSVTWYHKDBN"
    comp = dict(zip("=ACMGRSVTWYHKDBN", "=TGKCYSBAWRDMHVN"))  # IUPAC complements
    assert [letters[c] for c in B._COMPLEMENT] == [comp[x] for x in letters]


def _cross_check(records, max_len):
    chunk = BC.chunk_of(records)
    res = B.bam_reads_host(chunk, max_len)
    r1, r2 = B.bam_to_fastq(chunk, max_len)
    fq = F.fastq_tally_host(r1, r2, max_len)
    assert fq["bad_record"] == [-1, -1] and fq["records"] == res["records"]
    got, exp = F.split_fq_words(res["tally"].copy(), max_len), F.split_fq_words(fq["tally"], max_len)
    got["insert"][:] = 0
    for name in exp:
        assert np.array_equal(got[name], exp[name]), name
    return res


def _fastq_by_hand(records, max_len):
    """The two texts from the record dicts themselves, nothing of bam_report in it."""
    comp = str.maketrans("=ACMGRSVTWYHKDBN", "=TGKCYSBAWRDMHVN")
    out = ([], [])
    for r in records:
        f, q = r["flag"], r["qual"]
        if (q is None and r["seq"]) or len(r["seq"]) > max_len or any(x > 93 for x in q or ()):
            continue
        if f & 0x900 or (f & 1 and bool(f & 0x40) == bool(f & 0x80)):
            continue
        seq, q = (r["seq"].translate(comp)[::-1], q[::-1]) if f & 0x10 else (r["seq"], q)
        out[1 if f & 1 and f & 0x80 else 0].append("@%s\n%s\n+\n%s\n" % (r["name"], seq, "".join(chr(x + 33) for x in q or ())))
    return "".join(out[0]).encode(), "".join(out[1]).encode()


@pytest.mark.parametrize("seed,var_lengths", [(3, None), (4, (30, 151)), (5, (4, 40))])
def test_cross_check_on_synthetic_records(seed, var_lengths):
    records = bam_synth.records(seed, n_pairs=200, var_lengths=var_lengths)
    res = _cross_check(records, 301)
    assert res["bad_record"] == -1 and sum(res["skipped"]) > 0 and F.split_fq_words(res["tally"], 301)["insert"].sum() > 0
    assert B.bam_to_fastq(BC.chunk_of(records), 301) == _fastq_by_hand(records, 301)


def test_cross_check_on_the_edge_table():
    table = bam_synth.edge_table()
    good = [r for r in table if not (r["qual"] is None and r["seq"]) and all(q <= 93 for q in r["qual"] or ())]
    assert len(good) >= len(table) - 1
    res = _cross_check(good, 301)
    assert res["bad_record"] == -1
    assert B.bam_to_fastq(BC.chunk_of(good), 301) == _fastq_by_hand(good, 301)
    whole = B.bam_reads_host(BC.chunk_of(table), 301)  # the one record without qualities is reported and changes nothing else
    bad = [k for k, r in enumerate(table) if r["qual"] is None and r["seq"]]
    assert (whole["bad_record"], whole["bad_code"]) == (bad[0], B.REC_NO_QUAL) and np.array_equal(whole["tally"], res["tally"])


def test_every_insert_case():
    cases = BC.insert_cases()
    for r, exp in cases:
        t = F.split_fq_words(B.bam_reads_host(BC.chunk_of([r]), 16)["tally"], 16)
        assert t["insert"].sum() == (exp is not None) and (exp is None or t["insert"][exp] == 1), (r["flag"], r["tlen"], exp)
    t = F.split_fq_words(B.bam_reads_host(BC.chunk_of([r for r, _ in cases]), 16)["tally"], 16)
    assert np.array_equal(t["insert"], np.bincount([e for _, e in cases if e is not None], minlength=2048))


def test_bad_codes_and_their_order():
    ok = BC.rec("ACGTA", name="ok")
    cases = [
        (dict(ok, l_read_name=0), B.REC_SHORT), (dict(ok, l_seq=-1), B.REC_SHORT), (dict(ok, l_seq=-2 ** 31), B.REC_SHORT),
        (dict(ok, l_seq=2 ** 31 - 1), B.REC_SHORT), (dict(ok, truncate=1), B.REC_SHORT), (dict(ok, l_seq=6), B.REC_SHORT),
        (BC.rec("ACGTACGTA"), B.REC_TOO_LONG), (BC.rec("ACGT", "none"), B.REC_NO_QUAL), (BC.rec("ACGT", [0, 0, 0, 94]), B.REC_QUAL_RANGE),
        (BC.rec("ACGT", [255, 94, 0, 0]), B.REC_NO_QUAL), (BC.rec("ACGTACGTA", "none"), B.REC_TOO_LONG),  # two faults: the smaller code
        (BC.rec("ACGT", [0, 255, 0, 0]), B.REC_QUAL_RANGE),  # 0xFF behind the first byte is a quality out of range
        (BC.rec("ACGT", [0, 0, 0, 94], flag=BC.R1F | 0x100), B.REC_QUAL_RANGE),  # checked before the skip rules
        (BC.rec("", []), 0), (BC.rec("ACGTACGT"), 0), (dict(ok, tags=[("XX", "Z", "x" * 300)]), 0),
    ]
    alone = B.bam_reads_host(BC.chunk_of([ok, ok]), 8)["tally"]
    for r, code in cases:
        res = B.bam_reads_host(BC.chunk_of([ok, r, ok]), 8)
        assert (res["bad_record"], res["bad_code"]) == ((1, code) if code else (-1, 0)), (r, code)
        assert not code or (np.array_equal(res["tally"], alone) and res["skipped"] == [0, 0])
    res = B.bam_reads_host([BC.chunk_of([ok, ok]), BC.chunk_of([ok, cases[8][0], cases[6][0]])], 8)  # the first one, over all feeds
    assert (res["bad_record"], res["bad_code"]) == (3, B.REC_QUAL_RANGE)


def test_chunking_gives_the_same_words(tmp_path):
    records = bam_synth.records(8, n_pairs=60, var_lengths=(20, 90))
    whole = BC.chunk_of(records)
    exp = B.bam_reads_host(whole, 128)
    for per in (1, 4, 37):
        got = B.bam_reads_host(BC.split(whole, per), 128)
        assert np.array_equal(got["tally"], exp["tally"]) and got["records"] == exp["records"] and got["skipped"] == exp["skipped"]
    path = str(tmp_path / "a.bam")
    bam_synth.write_records(path, records)
    for chunk_bytes in (1, 700, 64 << 20):
        chunks = list(BamReader(path, chunk_bytes, 2).chunks())
        assert sum(len(c.offsets) for c in chunks) == len(records)
        assert np.array_equal(B.bam_reads_host(chunks, 128)["tally"], exp["tally"])
    bad = list(records)
    bad[77] = dict(bad[77], qual=[94] * len(bad[77]["seq"]))
    for per in (1, 4, 1000):
        got = B.bam_reads_host(BC.split(BC.chunk_of(bad), per), 128)
        assert (got["bad_record"], got["bad_code"]) == (77, B.REC_QUAL_RANGE)


def test_finish_relays_to_the_longest_read():
    res = B.finish(B.bam_reads_host(BC.chunk_of(EIGHT), 8), 8)
    assert res["read_length"] == 5 and res["tally"].size == tally_words(5) and res["lengths"].shape == (2, 6)
    assert res["records"] == [4, 1] and res["skipped"] == [1, 1] and (res["bad_record"], res["bad_code"]) == (6, 4)
    assert int(split_tally(res["tally"], 5)["insert"].sum()) == 2


def test_max_len_is_checked():
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            B.bam_reads_host(BC.chunk_of(EIGHT), bad)


# ---------------------------------------------------------------------------------------------------- command line
def test_parser_takes_bam():
    from insilicoseq_amd.app import build_parser

    args = build_parser().parse_args(["report", "--bam", "a.bam", "-o", "out", "--against", "t.npy", "--max_length", "301", "--device", "1",
                                      "--device_inflate"])
    assert (args.bam, args.read1, args.read2, args.output, args.against, args.max_length, args.device, args.device_inflate) == (
        "a.bam", None, None, "out", "t.npy", 301, 1, True)
    args = build_parser().parse_args(["report", "-1", "a.fastq", "-o", "out"])
    assert (args.bam, args.read1, args.device_inflate) == (None, "a.fastq", False)


class FakeBamTally:
    """BamReadTally with the twin in the device's place."""
    seen = []

    def __init__(self, device=0, max_len=B.MAX_LEN):
        self.max_len, self.chunks = max_len, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def feed_file(self, path, inflater=None, chunk_bytes=64 << 20, threads=None):
        FakeBamTally.seen.append(inflater)
        self.chunks.extend(BamReader(path, 1000, 2).chunks())

    def result(self):
        return B.finish(B.bam_reads_host(self.chunks, self.max_len), self.max_len)


@pytest.fixture
def cli(monkeypatch, tmp_path):
    from insilicoseq_amd import app

    monkeypatch.setattr(B, "BamReadTally", FakeBamTally)
    for name in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE"):
        monkeypatch.delenv(name, raising=False)

    def run(records, extra=(), blob=None):
        path = str(tmp_path / "in.bam")
        if blob is None:
            bam_synth.write_records(path, records)
        else:
            open(path, "wb").write(blob)
        return app.main(["report", "--quiet", "--bam", path, "-o", str(tmp_path / "out")] + list(extra)), path

    return run


def test_cli_writes_its_files(cli, tmp_path, capsys):
    records = bam_synth.records(11, n_pairs=80, var_lengths=(20, 50))
    exp = B.finish(B.bam_reads_host(BC.chunk_of(records), 1024), 1024)
    other = str(tmp_path / "other_tally.npy")
    np.save(other, exp["tally"])
    rc, _ = cli(records, ["--against", other])
    assert rc == 0 and capsys.readouterr().err == "" and FakeBamTally.seen[-1] is None  # (the host pool is the default)
    out = str(tmp_path / "out")
    assert np.array_equal(np.load(out + "_tally.npy"), exp["tally"]) and np.array_equal(np.load(out + "_lengths.npy"), exp["lengths"])
    report = json.load(open(out + "_report.json"))
    assert report["records_skipped"] == {"secondary_or_supplementary": exp["skipped"][0], "mate_flags": exp["skipped"][1]}
    assert sum(exp["skipped"]) > 0 and report["pairs"] == exp["records"][0] and report["read_length"] == exp["read_length"]
    assert sum(report["insert_size_histogram"]) > 0 and [sum(h) for h in report["read_length_histogram"]] == exp["records"]
    cmp = json.load(open(out + "_compare.json"))
    assert cmp["insert_tv"] == 0.0 and cmp["summary"]["insert_tv"] == 0.0 and cmp["summary"]["max_base_l1"] == 0.0
    # unequal mate counts are no error: a BAM without its second reads
    os.remove(out + "_compare.json")
    rc, _ = cli([r for r in records if not r["flag"] & 0x80 or not r["flag"] & 1])
    assert rc == 0 and capsys.readouterr().err == "" and not os.path.exists(out + "_compare.json")
    assert not np.load(out + "_lengths.npy")[1].any()


def test_cli_argument_errors(cli, tmp_path, capsys):
    from insilicoseq_amd import app

    out = str(tmp_path / "out")
    for argv in (["-o", out], ["--bam", "a.bam", "-1", "a.fastq", "-o", out], ["--bam", "a.bam", "-2", "b.fastq", "-o", out]):
        assert app.main(["report", "--quiet"] + argv) == 1
        err = capsys.readouterr().err
        assert err.startswith("ERROR: ") and err.count("\n") == 1
    assert not os.path.exists(out + "_tally.npy")


def test_cli_error_lines(cli, tmp_path, capsys, monkeypatch):
    records = bam_synth.records(12, n_pairs=20, quirks=False)
    records[13] = dict(records[13], qual=None)
    rc, path = cli(records)
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + path + ": record 13: ") and "without qualities" in err and err.count("\n") == 1
    assert not os.path.exists(str(tmp_path / "out_tally.npy"))
    rc, path = cli(None, blob=b"@r\nACGT\n+\nIIII\n")  # a BamError
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + path + ": not a BAM file") and err.count("\n") == 1
    rc, path = cli(None, blob=bam_synth.bgzf(bam_synth.header_bytes() + BC.encode(BC.rec("ACGT"))[:-3]))
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + path + ": truncated BAM record") and err.count("\n") == 1

    from insilicoseq_amd.inflate import InflateError

    def broken(self, path, inflater=None, **kw):
        raise InflateError("%s: member 3 does not inflate\nsecond line" % path)

    monkeypatch.setattr(FakeBamTally, "feed_file", broken)
    rc, path = cli(bam_synth.records(12, n_pairs=2))
    err = capsys.readouterr().err
    assert rc == 1 and err == "ERROR: %s: member 3 does not inflate\n" % path
    other = str(tmp_path / "other_tally.npy")
    np.save(other, np.zeros(tally_words(50) + 3, dtype=np.uint64))
    rc, _ = cli(bam_synth.records(12, n_pairs=2), ["--against", other])
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("ERROR: " + other) and "fit no read length" in err


def test_cli_inflate_route(cli, monkeypatch, capsys):
    """--device_inflate and ISS_DEVICE_INFLATE=1 ask for the device, ISS_HOST_INFLATE=1 wins over both."""
    from insilicoseq_amd import inflate

    class FakeInflater:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

    monkeypatch.setattr(inflate, "BgzfInflater", FakeInflater)
    records = bam_synth.records(12, n_pairs=2)
    for extra, env, device in (((), {}, False), (("--device_inflate",), {}, True), ((), {"ISS_DEVICE_INFLATE": "1"}, True),
                               (("--device_inflate",), {"ISS_HOST_INFLATE": "1"}, False),
                               ((), {"ISS_DEVICE_INFLATE": "1", "ISS_HOST_INFLATE": "1"}, False)):
        for name in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        rc, _ = cli(records, extra)
        assert rc == 0 and isinstance(FakeBamTally.seen[-1], FakeInflater) == device, (extra, env)


def test_library_exports_the_entries():
    from insilicoseq_amd import _native

    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iss_mi355x.h")).read()
    for name in ("iss_br_create", "iss_br_destroy", "iss_br_last_error", "iss_br_reset", "iss_br_tally_words", "iss_br_feed",
                 "iss_br_download", "iss_br_kernel_ms"):
        assert name in _native.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "#define ISS_ABI_VERSION 8" in header and _native.BR_MAX_LEN == _native.FQ_MAX_LEN == B.MAX_LEN
    for code, name in ((B.REC_SHORT, "SHORT"), (B.REC_TOO_LONG, "TOO_LONG"), (B.REC_NO_QUAL, "NO_QUAL"), (B.REC_QUAL_RANGE, "QUAL_RANGE")):
        assert "#define ISS_BR_REC_%s %d " % (name, code) in header and code in _native.BR_REC_ERRORS
