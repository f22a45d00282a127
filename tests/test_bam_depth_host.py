"""`report --bam --depth` without a GPU: the numpy twin (insilicoseq_amd.bam_depth.mark_chunk_host) against a base-by-base loop
over hand-made records, the accumulator's invariants, the coverage file, the comparison of two depth tables, the parser, and the
two entries in the header, the binding and the library."""
import json
import os
import re

import numpy as np
import pytest

import bam_depth_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(skip=True):
    from insilicoseq_amd.depth import depth_table

    table, n_words = depth_table([ln for _name, ln in DC.REFS])
    if skip:  # row 3 skipped: the accumulator ends behind row 2
        table[DC.SKIPPED_ROW, 0] = -1
        n_words -= DC.REFS[DC.SKIPPED_ROW][1] + 1
    return table, n_words


def _twin(records, table, n_words, flags=0, min_mapq=0, per=None):
    from insilicoseq_amd.bam_depth import mark_host

    diff = np.zeros(n_words, dtype=np.int32)
    chunk = DC.chunk_of(records)
    res = mark_host(diff, [chunk] if per is None else DC.split(chunk, per), table, flags, min_mapq)
    return diff, res


def _check(records, table, n_words, flags=0, min_mapq=0, per=None):
    diff, res = _twin(records, table, n_words, flags, min_mapq, per)
    depth, counts, bad = DC.expected(records, table, bool(flags & 1), min_mapq)
    assert np.array_equal(np.cumsum(diff.astype(np.int64)), depth[:n_words])
    assert res["depth_counts"] == counts and (res["bad_depth_record"], res["bad_depth_code"]) == bad
    return diff, res


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("min_mapq", [0, 20, 255])
def test_twin_equals_the_base_by_base_loop(flags, min_mapq):
    table, n_words = _table()
    records = DC.valid_cases()
    diff, res = _check(records, table, n_words, flags, min_mapq)
    c = res["depth_counts"]
    assert res["bad_depth_record"] == -1 and c[1] == 5 and c[2] == 3
    assert (c[0], c[3], c[4]) == {0: (24, 0, 2), 20: (22, 2, 2), 255: (1, 25, 0)}[min_mapq]
    assert sum(c[:5]) == sum(DC.taken(r["flag"]) for r in records)


def test_each_case_alone_and_the_named_properties():
    table, n_words = _table()
    by_name = {r["name"]: r for r in DC.valid_cases()}
    depth_of = lambda names, flags=0: np.cumsum(_check([by_name[n] for n in names], table, n_words, flags)[0])
    for r in by_name.values():
        _check([r], table, n_words)
        _check([r], table, n_words, 1)
    r50, r1, r300 = (int(table[k, 0]) for k in range(3))
    d = depth_of(["M_to_the_end"])
    assert d[r50 + 29] == 0 and d[r50 + 30:r50 + 50].tolist() == [1] * 20 and d[r50 + 50] == 0
    assert _twin([by_name["M_to_the_end"]], table, n_words)[0][r50 + 50] == -1  # the sink took the -1
    assert depth_of(["ref1_covered"])[r1:r1 + 2].tolist() == [1, 0]
    assert np.flatnonzero(depth_of(["clips_and_pads"])).tolist() == list(range(r50 + 5, r50 + 13))
    assert np.flatnonzero(depth_of(["D_splits"])).tolist() == [r300 + k for k in list(range(10, 15)) + list(range(18, 23))]
    assert np.flatnonzero(depth_of(["D_splits"], 1)).tolist() == list(range(r300 + 10, r300 + 23))
    for flags in (0, 1):
        assert np.flatnonzero(depth_of(["N_splits"], flags)).tolist() == [r300 + k for k in list(range(40, 45)) + list(range(65, 70))]
    assert np.flatnonzero(depth_of(["eq_and_X"])).tolist() == list(range(r300 + 100, r300 + 110))
    assert np.flatnonzero(depth_of(["M_then_eq"])).tolist() == list(range(r300 + 120, r300 + 128))
    d = depth_of(["twice_a", "twice_b"])
    assert d[r300 + 200:r300 + 240].tolist() == [1] * 10 + [2] * 20 + [1] * 10
    assert depth_of(["ops300_MD"])[r300:r300 + 300].tolist() == [1, 0] * 150
    assert depth_of(["ops300_MD"], 1)[r300:r300 + 301].tolist() == [1] * 300 + [0]
    assert depth_of(["ops300_MX"])[r50:r50 + 51].tolist() == [1] * 50 + [0]
    assert not depth_of(["only_N_and_D"]).any() and depth_of(["only_N_and_D"], 1)[r300 + 263:r300 + 265].tolist() == [1, 1]


def test_every_records_words_sum_to_zero_and_covered_bases_are_the_sum_of_depth():
    from insilicoseq_amd.depth import finish_host

    table, n_words = _table()
    for flags in (0, 1):
        for r in DC.valid_cases():
            diff, _res = _twin([r], table, n_words, flags)
            for off, ln in table[:3].tolist():
                assert int(diff[off:off + ln + 1].sum()) == 0, r["name"]
        diff, res = _twin(DC.valid_cases(), table, n_words, flags)
        _depth, stats, _bins = finish_host(diff, table)
        assert res["depth_counts"][5] == int(stats[:, 0].sum()) > 500
        assert not stats[DC.SKIPPED_ROW].any()


def test_bad_records_add_nothing_and_the_first_one_is_kept():
    table, n_words = _table()
    assert sorted({code for _r, code in DC.bad_cases()}) == [1, 2, 3]
    for bad, code in DC.bad_cases():
        for k in range(3):
            three = DC.between_good(bad, k)
            diff, res = _check(three, table, n_words)
            assert (res["bad_depth_record"], res["bad_depth_code"]) == (k, code), bad["name"]
            assert np.array_equal(diff, _twin([r for r in three if r is not bad], table, n_words)[0])
            assert res["depth_counts"][0] == 2 and sum(res["depth_counts"][1:5]) == 0
        diff, res = _twin([bad], table, n_words)
        assert not diff.any() and res["depth_counts"] == [0] * 6
    records = []
    for k, (bad, _code) in enumerate(DC.bad_cases()):
        records += DC.between_good(bad, k % 3)
    for per in (None, 1, 7):
        _diff, res = _check(records, table, n_words, per=per)
        assert (res["bad_depth_record"], res["bad_depth_code"]) == (0, 1)
    swapped = records[3:] + records[:3]
    _diff, res = _check(swapped, table, n_words, per=2)
    assert (res["bad_depth_record"], res["bad_depth_code"]) == (1, 1)  # bad_op15_last, at place 1 of its three


def test_skipped_row_and_real_row():
    """Row 3 as a row like any other: its records mark, and the one past its end is a bad span."""
    table, n_words = _table(skip=False)
    by_name = {r["name"]: r for r in DC.valid_cases()}
    diff, res = _check([by_name["on_row_3"], by_name["on_row_3_past_its_end"]], table, n_words)
    assert res["depth_counts"] == [1, 0, 0, 0, 0, 10] and (res["bad_depth_record"], res["bad_depth_code"]) == (1, 3)
    off = int(table[3, 0])
    assert np.flatnonzero(diff).tolist() == [off, off + 10]


def test_feeds_do_not_change_the_array():
    table, n_words = _table()
    records = DC.valid_cases()
    whole, res = _twin(records, table, n_words)
    for per in (1, 7):
        diff, r = _twin(records, table, n_words, per=per)
        assert np.array_equal(diff, whole) and r == res


def test_twin_argument_errors():
    from insilicoseq_amd.bam_depth import mark_chunk_host

    table, n_words = _table()
    diff = np.zeros(n_words, dtype=np.int32)
    with pytest.raises(ValueError):
        mark_chunk_host(diff, DC.chunk_of([]), table, flags=2)
    with pytest.raises(ValueError):
        mark_chunk_host(diff, DC.chunk_of([]), table, min_mapq=256)
    counts, bad, code = mark_chunk_host(diff, DC.chunk_of([]), table)
    assert counts.tolist() == [0] * 6 and (bad, code) == (-1, 0)


# ---------------------------------------------------------------------------------------------------- files
def test_coverage_file_reads_back_as_an_abundance_file(tmp_path):
    from insilicoseq_amd.app import parse_abundance_file
    from insilicoseq_amd.bam_depth import coverage_rows, write_coverage_file
    from insilicoseq_amd.depth import finish_host

    table, n_words = _table()
    diff, _res = _twin(DC.valid_cases(), table, n_words)
    _depth, stats, _bins = finish_host(diff, table)
    ids = [name for name, _ln in DC.REFS]
    rows = coverage_rows(stats, table, ids)
    assert [rid for rid, _m in rows] == ids and rows[1][1] == 1.0 and rows[3][1] == 0.0
    assert rows[0][1] == int(stats[0, 0]) / 50.0 and rows[2][1] == int(stats[2, 0]) / 300.0
    path = str(tmp_path / "x_coverage.txt")
    write_coverage_file(path, rows)
    assert parse_abundance_file(path) == dict(rows)
    assert open(path).read().splitlines()[1] == "ref1\t1.0"


def test_compare_of_two_hand_made_tables(tmp_path):
    from insilicoseq_amd.bam_depth import compare_depth_tables, read_depth_table
    from insilicoseq_amd.depth import write_depth_table

    a = str(tmp_path / "a_depth.txt")
    b = str(tmp_path / "b_depth.txt")
    write_depth_table(a, [("x", 100, 3.0, 1.0, 0.5, 7), ("y", 50, 1.0, 0.0, 1.0, 1), ("only_a", 10, 2.0, 0.0, 1.0, 2)])
    write_depth_table(b, [("y", 50, 3.0, 0.0, 0.75, 3), ("x", 100, 1.0, 0.0, 0.25, 2), ("only_b", 10, 0.0, 0.0, 0.0, 0)])
    ta, tb = read_depth_table(a), read_depth_table(b)
    assert ta["x"] == (100, 3.0, 1.0, 0.5, 7) and list(ta) == ["x", "y", "only_a"]
    cmp = compare_depth_tables(ta, tb)
    assert cmp["records"] == {"x": {"mean_depth": 2.0, "covered_fraction": 0.25}, "y": {"mean_depth": -2.0, "covered_fraction": 0.25}}
    assert cmp["summary"] == {"max_abs_mean_depth": 2.0, "max_abs_covered_fraction": 0.25, "total_variation_mean_depth": 0.5}
    assert cmp["only_here"] == ["only_a"] and cmp["only_there"] == ["only_b"]
    same = compare_depth_tables(ta, ta)
    assert set(same["summary"].values()) == {0.0} and same["only_here"] == same["only_there"] == []
    json.dumps(cmp)
    zero = compare_depth_tables({"x": (5, 0.0, 0.0, 0.0, 0)}, {"x": (5, 1.0, 0.0, 1.0, 1)})
    assert zero["summary"]["total_variation_mean_depth"] is None
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("id\tmean\nx\t1\n")
    with pytest.raises(ValueError):
        read_depth_table(bad)


# ---------------------------------------------------------------------------------------------------- the command line
def test_parser_takes_the_flags():
    from insilicoseq_amd.app import build_parser

    args = build_parser().parse_args(["report", "--bam", "a.bam", "-o", "p", "--depth", "--depth_bin", "7", "--depth_deletions",
                                      "--min_mapq", "20", "--against_depth", "o_depth.txt"])
    assert args.depth and args.depth_bin == 7 and args.depth_deletions and args.min_mapq == 20 and args.against_depth == "o_depth.txt"
    args = build_parser().parse_args(["report", "--bam", "a.bam", "-o", "p"])
    assert not args.depth and args.depth_bin is None and not args.depth_deletions and args.min_mapq is None and args.against_depth is None


@pytest.mark.parametrize("flags", [["--depth"], ["--depth_bin", "7"], ["--depth_deletions"], ["--min_mapq", "3"], ["--against_depth", "x"]])
def test_depth_without_bam_is_one_error_line(flags, capsys, tmp_path):
    from insilicoseq_amd.app import main

    assert main(["report", "-1", str(tmp_path / "none.fastq"), "-o", str(tmp_path / "p"), "--quiet"] + flags) == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("ERROR: ") and "--bam" in err
    assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------------------------------------------- the entries
def test_header_binding_and_library_name_the_entries():
    from insilicoseq_amd import _native

    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    for name in ("iss_br_depth_enable", "iss_br_depth_download"):
        assert re.search(r"^int %s\(iss_br \*br, " % name, header, re.M), name
        assert name in _native.EXPORTS
        assert hasattr(_native.lib(), name), name
    for name, value in (("ISS_BR_DEPTH_COUNT_DEL", "1u"), ("ISS_BR_DEPTH_CIGAR", "1"), ("ISS_BR_DEPTH_REF", "2"), ("ISS_BR_DEPTH_SPAN", "3")):
        assert re.search(r"^#define %s %s\b" % (name, value), header, re.M), name
    assert sorted(_native.BR_DEPTH_ERRORS) == [1, 2, 3] and _native.BR_DEPTH_COUNT_DEL == 1
    assert _native.lib().iss_abi_version() == 8
    api = open(os.path.join(ROOT, "insilicoseq_amd", "csrc", "iss_api_bamreads.hip.h")).read()
    assert "int iss_br_depth_enable(" in api and "int iss_br_depth_download(" in api
