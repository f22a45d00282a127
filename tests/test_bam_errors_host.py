"""`report --bam --errors` without a GPU: the twin (insilicoseq_amd.bam_errors.bam_errors_host) against the constructions of
bam_error_cases.py, its substitution rows against errtally.errors_host, the layout, the report, the comparison and the command line
with the twin in the device's place."""
import json
import os

import numpy as np
import pytest

import bam_error_cases as EC
import bam_synth
from insilicoseq_amd import bam_errors as E
from insilicoseq_amd import bam_report as B
from insilicoseq_amd import errtally
from insilicoseq_amd.bam import BamReader


def _same(got, exp, max_len):
    assert got["error_counts"] == exp["error_counts"]
    assert (got["bad_alignment"], got["bad_alignment_code"]) == (exp["bad_alignment"], exp["bad_alignment_code"])
    g, e = E.split(got["errors"], max_len), E.split(exp["errors"], max_len)
    assert [k for k in g if not np.array_equal(g[k], e[k])] == []  # (the fields that differ)


def test_layout():
    for L in (1, 151, 1024):
        lay = E.layout(L)
        assert lay["words"] == 2 + 446 * L + 384 == E.words(L) and lay["bases"] == (errtally.words(L), (2, L, 94))
        assert [lay[k] for k in errtally.FIELDS] == [errtally.layout(L)[k] for k in errtally.FIELDS]
    with pytest.raises(ValueError):
        E.split(np.zeros(7, dtype=np.uint64), 4)


@pytest.mark.parametrize("max_len", [1024, 301])
def test_twin_equals_the_construction(max_len):
    records = [r for r in EC.valid_cases() if len(r["seq"]) <= max_len]
    for r in records:  # each alone: a difference names its record
        _same(E.bam_errors_host(EC.chunk_of([r]), max_len), EC.expected([r], max_len), max_len), r["name"]
    got = E.bam_errors_host(EC.chunk_of(records), max_len)
    _same(got, EC.expected(records, max_len), max_len)
    t = E.split(got["errors"], max_len)
    assert got["bad_alignment"] == -1 and not t["dropped"][0] and sum(got["error_counts"][:2]) == len(records)
    assert t["per_read"][:, :, 63].all() and t["sub_mat"][:, :, 4, 4].any() and t["del"][:, :, 4].any() and t["ins"].any()
    top = max(len(r["seq"]) for r in records)
    assert t["bases"][:, top - 1].any() and t["sub_q"][:, top - 1].any() and not t["bases"][:, top:].any()


def test_every_damaged_record_adds_nothing_but_dropped():
    cases = EC.damaged_cases()
    assert {r["_case"]["expect"] for r in cases} == {E.ALN_CIGAR, E.ALN_TAGS, E.ALN_MD, "no_md", "unaligned", "skipped"}
    for r in cases:
        what = r["_case"]["expect"]
        got = E.bam_errors_host(EC.chunk_of([r]), 64)
        _same(got, EC.expected([r], 64), 64)
        assert not got["errors"][1:].any(), r["name"]
        if isinstance(what, int):
            assert int(got["errors"][0]) == 1 and (got["bad_alignment"], got["bad_alignment_code"]) == (0, what), r["name"]
        else:
            assert not got["errors"][0] and got["bad_alignment"] == -1, r["name"]
        for k in range(3):  # between two good ones and at both ends
            three = EC.between_good(r, k)
            _same(E.bam_errors_host(EC.chunk_of(three), 64), EC.expected(three, 64), 64)
        # the read tally does not know of any of this
        assert B.bam_reads_host(EC.chunk_of([r]), 64)["bad_record"] == -1


def test_first_bad_alignment_wins_across_feeds():
    bad = {r["name"]: r for r in EC.damaged_cases()}
    records = EC.between_good(bad["secondary"], 0) + EC.between_good(bad["md_too_long"], 2) + EC.between_good(bad["op9"], 1)
    exp = EC.expected(records, 64)
    assert (exp["bad_alignment"], exp["bad_alignment_code"]) == (5, E.ALN_MD) and int(exp["errors"][0]) == 2
    for per in (None, 4, 1):
        chunks = [EC.chunk_of(records)] if per is None else EC.split(EC.chunk_of(records), per)
        _same(E.bam_errors_host(chunks, 64), exp, 64)


def test_feeds_do_not_change_the_words():
    records = bam_synth.records(7, n_pairs=40, var_lengths=(4, 120))
    records[5]["flag"] |= 4
    whole = E.bam_errors_host(EC.chunk_of(records), 128)
    assert whole["bad_alignment"] == -1 and whole["error_counts"][2] > 0 and sum(whole["error_counts"][:2]) > 60
    t = E.split(whole["errors"], 128)
    assert t["sub_q"].any() and t["ins"].any() and t["del"].any()
    for per in (7, 1):
        _same(E.bam_errors_host(EC.split(EC.chunk_of(records), per), 128), whole, 128)


def test_substitution_rows_as_mutation_rows_give_errtallys_fields():
    """The twin's substitutions, written as iss_mutation rows (position and letters as sequenced), through errtally.errors_host."""
    from insilicoseq_amd.engine import MUT_DTYPE

    L = 129
    records = [r for r in EC.valid_cases() if len(r["seq"]) <= L and not any(op in (1, 2) for op, _ in r["cigar"])]
    pairs = [(a, b) for a, b in zip([r for r in records if EC.mate_of(r["flag"]) == 0], [r for r in records if EC.mate_of(r["flag"]) == 1])]
    rows = []
    for k, pair in enumerate(pairs):
        for m, r in enumerate(pair):
            n, rev = len(r["seq"]), bool(r["flag"] & 0x10)
            comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
            for q, ref in r["_case"]["mism"].items():
                ref, alt = ref.encode(), r["seq"][q].encode()
                rows.append((k, m, 0, n - 1 - q if rev else q, (ref.translate(comp) if rev else ref)[0], (alt.translate(comp) if rev else alt)[0],
                             r["qual"][q]))
    assert len(rows) > 100
    exp = errtally.split(errtally.errors_host(np.array(rows, dtype=MUT_DTYPE), 0, len(pairs), L), L)
    got = E.split(E.bam_errors_host(EC.chunk_of([r for pair in pairs for r in pair]), L)["errors"], L)
    for name in ("pairs", "sub_q", "sub_mat"):
        assert np.array_equal(got[name], exp[name]), name
    assert np.array_equal(got["per_read"][:, 0], exp["per_read"][:, 0])


# ------------------------------------------------------------------------------------------------------------ small tallies by hand
def _hand():
    """max_len 4, mate 0: 10 bases at each of positions 0 .. 2 (phred 20 at 0 and 1, phred 30 at 2); substitutions 2 at position 0
    (A->C, A->G), 1 at position 2 (T->A); 1 insertion at 1; 2 deletions at 2; 10 pairs."""
    flat = np.zeros(E.words(4), dtype=np.uint64)
    t = E.split(flat, 4)
    t["pairs"][0] = 10
    t["bases"][0, 0, 20] = t["bases"][0, 1, 20] = t["bases"][0, 2, 30] = 10
    t["sub_q"][0, 0, 20], t["sub_q"][0, 2, 30] = 2, 1
    t["sub_mat"][0, 0, 0, 1] = t["sub_mat"][0, 0, 0, 2] = t["sub_mat"][0, 2, 3, 0] = 1
    t["ins"][0, 1, 2] = 1
    t["del"][0, 2, 4] = 2
    t["per_read"][0, 0, 0], t["per_read"][0, 0, 1], t["per_read"][0, 0, 2] = 8, 1, 1
    t["per_read"][0, 1, 0], t["per_read"][0, 1, 1] = 9, 1
    t["per_read"][0, 2, 0], t["per_read"][0, 2, 2] = 9, 1
    return flat


def test_relayout():
    flat = _hand()
    out = E.relayout(flat, 4, 3)
    assert out.size == E.words(3)
    a, b = E.split(flat, 4), E.split(out, 3)
    for name in E.FIELDS:
        assert np.array_equal(b[name], a[name][:, :3] if a[name].ndim > 2 and name != "per_read" else a[name]), name
    assert np.array_equal(E.relayout(flat, 4, 4), flat)
    for L in (0, 5):
        with pytest.raises(ValueError):
            E.relayout(flat, 4, L)
    with pytest.raises(ValueError):  # position 2 holds counts
        E.relayout(flat, 4, 2)
    err, bases = E.errors_and_bases(out, 3)
    assert err.size == errtally.words(3) and np.array_equal(err, out[:err.size]) and bases.shape == (2, 3, 94) and int(bases.sum()) == 30


def test_report_dict():
    rep = E.report_dict(_hand(), 4, [10, 0, 3, 1])
    json.dumps(rep)
    m0, m1 = rep["mates"]
    assert rep["pairs"] == 10 and rep["dropped"] == 0 and rep["read_length"] == 4
    assert rep["counts"] == {"tallied": [10, 0], "unaligned": 3, "no_md": 1}
    assert m0["rates"] == {"substitution": [0.2, 0.0, 0.1, None], "insertion": [0.0, 0.1, 0.0, None], "deletion": [0.0, 0.0, 0.2, None]}
    assert m1["rates"]["substitution"] == [None] * 4 and m0["aligned_bases"] == [10, 10, 10, 0]
    assert m0["substitution_matrix"]["A"] == {"A": 0, "C": 1, "G": 1, "T": 0, "other": 0} and m0["substitution_matrix"]["T"]["A"] == 1
    assert m0["substitutions_by_phred"] == [0] * 20 + [2] + [0] * 9 + [1]
    assert m0["per_read"] == {"substitution": [8, 1, 1], "insertion": [9, 1], "deletion": [9, 0, 1]}
    assert rep["calibration"][1] == [] and rep["calibration"][0] == [
        {"phred": 20, "bases": 20, "substitutions": 2, "nominal": 0.01, "empirical": 0.1},
        {"phred": 30, "bases": 10, "substitutions": 1, "nominal": 0.001, "empirical": 0.1}]


def test_compare_errors():
    a = _hand()
    a_err, a_bases = E.errors_and_bases(a, 4)
    same = E.compare_errors(a_err, a_bases, 4, a_err, a_bases, 4)
    json.dumps(same)
    assert same["summary"] == {"max_abs_substitution_rate_diff": 0.0, "max_abs_insertion_rate_diff": 0.0, "max_abs_deletion_rate_diff": 0.0,
                               "max_substitution_matrix_tv": 0.0, "max_per_read_tv": 0.0, "max_abs_calibration_diff": 0.0}
    # the other side: read length 3, 20 pairs and no bases array -- 4 substitutions at position 0 (all A->C), nothing else
    b = np.zeros(errtally.words(3), dtype=np.uint64)
    tb = errtally.split(b, 3)
    tb["pairs"][0] = 20
    tb["sub_q"][0, 0, 20] = 4
    tb["sub_mat"][0, 0, 0, 1] = 4
    tb["per_read"][0, 0, 0], tb["per_read"][0, 0, 1] = 16, 4
    tb["per_read"][0, 1, 0] = tb["per_read"][0, 2, 0] = 20
    cmp = E.compare_errors(a_err, a_bases, 4, b, None, 3)
    assert cmp["positions"] == 3 and cmp["read_lengths"] == [4, 3] and cmp["calibration_diff"] is None
    m0 = cmp["mates"][0]
    assert m0["rate_diff"]["substitution"] == [0.2 - 0.2, 0.0, 0.1] and m0["rate_diff"]["insertion"] == [0.0, 0.1, 0.0]
    assert m0["rate_diff"]["deletion"] == [0.0, 0.0, 0.2]
    assert cmp["mates"][1]["rate_diff"]["substitution"] == [None] * 3  # mate 1 of a has no bases
    assert m0["substitution_matrix_tv"] == pytest.approx(2 / 3)         # (1/3, 1/3, 1/3) against (1, 0, 0)
    assert m0["per_read_tv"]["substitution"] == pytest.approx(0.5 * (0.0 + 0.1 + 0.1))  # (.8, .1, .1) against (.8, .2, 0)
    assert m0["per_read_tv"]["insertion"] == pytest.approx(0.1) and cmp["mates"][1]["per_read_tv"]["deletion"] is None
    assert cmp["summary"]["max_abs_substitution_rate_diff"] == pytest.approx(0.1) and cmp["summary"]["max_abs_calibration_diff"] is None
    assert cmp["summary"]["max_substitution_matrix_tv"] == pytest.approx(2 / 3) and cmp["summary"]["max_per_read_tv"] == pytest.approx(0.1)
    # with bases on both sides: per phred
    b_bases = np.zeros((2, 3, 94), dtype=np.uint64)
    b_bases[0, :, 20] = 20
    cmp = E.compare_errors(a_err, a_bases, 4, b, b_bases, 3)
    assert cmp["calibration_diff"] == [[{"phred": 20, "diff": pytest.approx(2 / 20 - 4 / 60)}], []]
    with pytest.raises(ValueError):
        E.compare_errors(a_err, a_bases[:, :3], 4, b, None, 3)


# ------------------------------------------------------------------------------------------------------------ the command line
class FakeBamTally:
    """BamReadTally with the twins in the device's place."""

    def __init__(self, device=0, max_len=B.MAX_LEN, errors=False):
        self.max_len, self.errors, self.chunks = max_len, errors, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def feed_file(self, path, inflater=None, chunk_bytes=64 << 20, threads=None):
        self.chunks.extend(BamReader(path, 1000, 2).chunks())

    def result(self):
        res = B.finish(B.bam_reads_host(self.chunks, self.max_len), self.max_len)
        if self.errors:
            raw = E.bam_errors_host(self.chunks, self.max_len)
            res.update(raw, errors=E.relayout(raw["errors"], self.max_len, res["read_length"]))
        return res


@pytest.fixture
def cli(monkeypatch, tmp_path):
    from insilicoseq_amd import app

    monkeypatch.setattr(B, "BamReadTally", FakeBamTally)
    for name in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE"):
        monkeypatch.delenv(name, raising=False)

    def run(records, extra=(), quiet=True):
        path = str(tmp_path / "in.bam")
        bam_synth.write_records(path, records)
        return app.main(["report"] + (["--quiet"] if quiet else []) + ["--bam", path, "-o", str(tmp_path / "out")] + list(extra))

    return run


def test_cli_argument_errors(tmp_path, capsys):
    from insilicoseq_amd import app

    out = str(tmp_path / "out")
    for argv in (["-1", "a.fastq", "--errors", "-o", out], ["--bam", "a.bam", "--against_errors", "x_errtally.npy", "-o", out],
                 ["-1", "a.fastq", "--against_errors", "x_errtally.npy", "-o", out]):
        assert app.main(["report", "--quiet"] + argv) == 1
        err = capsys.readouterr().err
        assert err.startswith("ERROR: ") and err.count("\n") == 1 and ("--bam" in err or "--errors" in err)
    assert not os.listdir(str(tmp_path))
    args = app.build_parser().parse_args(["report", "--bam", "a.bam", "-o", "o", "--errors", "--against_errors", "e.npy"])
    assert args.errors is True and args.against_errors == "e.npy"
    args = app.build_parser().parse_args(["report", "--bam", "a.bam", "-o", "o"])
    assert args.errors is False and args.against_errors is None


def test_cli_writes_the_error_files(cli, tmp_path, capsys):
    records = bam_synth.records(13, n_pairs=60, var_lengths=(20, 50))
    raw = E.bam_errors_host(EC.chunk_of(records), 1024)
    L = B.finish(B.bam_reads_host(EC.chunk_of(records), 1024), 1024)["read_length"]
    exp_err, exp_bases = E.errors_and_bases(E.relayout(raw["errors"], 1024, L), L)
    out = str(tmp_path / "out")
    assert cli(records) == 0 and not os.path.exists(out + "_errtally.npy")  # without --errors: today's three files
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam", "out_lengths.npy", "out_report.json", "out_tally.npy"]
    assert cli(records, ["--errors"]) == 0 and capsys.readouterr().err == ""
    assert np.array_equal(np.load(out + "_errtally.npy"), exp_err) and np.array_equal(np.load(out + "_errbases.npy"), exp_bases)
    assert exp_err.size == errtally.words(L) and not os.path.exists(out + "_errors_compare.json")
    rep = json.load(open(out + "_errors.json"))
    assert rep["counts"]["tallied"] == raw["error_counts"][:2] and rep["bad_alignment"] == {"record": -1, "code": 0}
    assert rep["pairs"] == raw["error_counts"][0] and rep["read_length"] == L and len(rep["calibration"][0]) > 5
    # against itself: through OTHER_errbases.npy beside the file, through --against, and with pairs alone
    for stem, extra, calibrated in (("a", [], True), ("b", ["--against", out + "_tally.npy"], True), ("c", [], False)):
        other = str(tmp_path / stem) + "_errtally.npy"
        np.save(other, exp_err)
        if stem == "a":
            np.save(str(tmp_path / "a_errbases.npy"), exp_bases)
        assert cli(records, ["--errors", "--against_errors", other] + extra) == 0 and capsys.readouterr().err == ""
        cmp = json.load(open(out + "_errors_compare.json"))
        assert cmp["summary"]["max_substitution_matrix_tv"] == 0.0 and cmp["summary"]["max_per_read_tv"] == 0.0
        assert (cmp["calibration_diff"] is not None) == calibrated
        assert (cmp["summary"]["max_abs_substitution_rate_diff"] == 0.0) == (stem == "a")  # (b: all bases of the reads; c: pairs)
    for bad_file, content in (("short_errtally.npy", np.zeros(100, dtype=np.uint64)), ("nofile_errtally.npy", None)):
        if content is not None:
            np.save(str(tmp_path / bad_file), content)
        assert cli(records, ["--errors", "--against_errors", str(tmp_path / bad_file)]) == 1
        err = capsys.readouterr().err
        assert err.startswith("ERROR: ") and err.count("\n") == 1 and bad_file in err


def test_cli_warns_of_a_bad_alignment_and_goes_on(cli, tmp_path, caplog):
    bad = {r["name"]: r for r in EC.damaged_cases()}
    records = EC.between_good(bad["md_too_long"], 1)
    assert cli(records, ["--errors"], quiet=False) == 0
    lines = [r.getMessage() for r in caplog.records if r.levelname == "WARNING" and " reads" not in r.getMessage()]  # (2 + 1 mates)
    assert len(lines) == 1 and "in.bam" in lines[0] and "record 1" in lines[0] and "MD" in lines[0]
    rep = json.load(open(str(tmp_path / "out_errors.json")))
    assert rep["dropped"] == 1 and rep["bad_alignment"] == {"record": 1, "code": E.ALN_MD} and rep["counts"]["tallied"] == [1, 1]


def test_cli_without_md_tags_names_calmd(cli, tmp_path, capsys):
    bad = {r["name"]: r for r in EC.damaged_cases()}
    assert cli([bad["no_md"], bad["no_tags"], bad["unmapped"]], ["--errors"]) == 1
    err = capsys.readouterr().err
    assert err.startswith("ERROR: ") and err.count("\n") == 1 and "MD" in err and "samtools calmd" in err and "in.bam" in err
    assert not os.path.exists(str(tmp_path / "out_errors.json"))


def test_the_new_exports_are_declared():
    from insilicoseq_amd import _native

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iss_mi355x.h")).read()
    for name in ("iss_br_errors_enable", "iss_br_error_words", "iss_br_errors_download"):
        assert name in _native.EXPORTS and name + "(" in header
    for name, value in (("ISS_BR_ALN_CIGAR", 1), ("ISS_BR_ALN_TAGS", 2), ("ISS_BR_ALN_MD", 3)):
        assert "#define %s %d" % (name, value) in header
    assert (E.ALN_CIGAR, E.ALN_TAGS, E.ALN_MD) == (1, 2, 3) and set(_native.BR_ALN_ERRORS) == {1, 2, 3}
