"""The yardsticks of tests/test_gpu_model_edges.py, checked where no GPU exists: the Python twin on hand-worked records of the edge
table, the table's reach, and the 60-digit KDE reference against scipy's gaussian_kde on every case the GPU test uses."""
import numpy as np
import pytest

import bam_synth
import bam_twin
import kde_ref

TABLE = bam_synth.edge_table()
BY_NAME = {r["name"]: r for r in TABLE}
COL = {"A": 0, "T": 1, "C": 2, "G": 3}


def twin(recs):
    return bam_twin.tallies(bam_twin.from_dicts(recs))


def indel_entries(t):
    return sorted((int(m), int(p), int(c), int(t["indel"][m, p, c])) for m, p, c in zip(*np.nonzero(t["indel"])))


def test_twin_wraps_negative_indel_positions_by_hand():
    """neg_I_D is 2M 10D 1I 3M 2D 5M on 11 bases (iss/modeller.py:281-313): the first D reads query_alignment_sequence[2] into row 2 and
    moves to -8; the I reads query_sequence[-8] = [3] into row 301 - 8; 3M later the second D reads [-4] = [7] into row 301 - 4."""
    r = BY_NAME["neg_I_D"]
    s = r["seq"]
    assert indel_entries(twin([r])) == sorted([(0, 2, 5 + COL[s[2]], 1), (0, 293, 1 + COL[s[3]], 1), (0, 297, 5 + COL[s[7]], 1)])
    # with 2S in front and 3S behind, the deletions index the sequence without its clips, the insertion the whole of it
    r = BY_NAME["neg_clipped"]
    s = r["seq"]
    assert indel_entries(twin([r])) == sorted([(0, 2, 5 + COL[s[2 + 2]], 1), (0, 293, 1 + COL[s[16 - 8]], 1), (0, 297, 5 + COL[s[2 + 7]], 1)])


def test_twin_hard_then_soft_clip_by_hand():
    """5H 3S 10M 2D 5M 1I 4M 2S 4H: pysam's query_alignment_start passes the hard clip over, so D reads [3 + 10]; I reads [13]."""
    r = BY_NAME["clip_HSMSH"]
    s = r["seq"]
    t = twin([r])
    assert indel_entries(t) == sorted([(0, 10, 5 + COL[s[13]], 1), (0, 13, 1 + COL[s[13]], 1)])
    # the aligned query positions are 3..17 and 19..22 (18 is the insertion); 22 holds the reference letter N, which is no substitution
    assert np.flatnonzero(t["subst"][0].sum(axis=1)).tolist() == list(range(3, 18)) + [19, 20, 21]


def test_twin_bins_and_template_lengths_by_hand():
    t = twin(TABLE)
    for l, mate in ((7, 0), (301, 1)):
        rows = twin([BY_NAME["mean%s_l%d" % (w, l)] for w in ("9", "10", "19", "30", "39", "40")])
        assert rows["nread"][mate].tolist() == [1, 2, 0, 2] and rows["taken"] == 6  # 9 | 10, 19 | 30, 39 | no bin for 40
    assert t["tlen"][[0, 1, 1999]].tolist() == [0, 2, 2] and t["tlen"][[333, 444, 556]].tolist() == [1, 1, 1] and t["tlen"][[555, 557]].sum() == 0
    assert twin([BY_NAME["qual_all_93"]])["nread"].sum() == 0
    rev = twin([BY_NAME["qual_93_and_0"]])  # reversed: the 93 of query position 0 lands at position 10
    assert rev["qhist"][0, 0, 10, 93] == 1 and rev["qhist"][0, 0, 0, 0] == 1
    both = twin([BY_NAME["flag_both"]])  # read1 and read2: `if is_read1 ... elif is_read2` (iss/bam.py:133, 143)
    assert both["nread"][0].sum() == 1 and both["nread"][1].sum() == 0 and both["indel"][0].sum() == 1 and both["indel"][1].sum() == 0
    neither = twin([BY_NAME["flag_neither"]])
    assert neither["nread"].sum() == 0 and neither["subst"].sum() == 0 and neither["indel"].sum() == 0 and neither["tlen"][333] == 1


def test_table_reaches_what_it_is_for():
    t = twin(TABLE)
    assert t["indel"][:, 200:].sum() >= 10 and t["indel"][:, :200].sum() > 300  # five reads put two wrapped rows each past 200
    assert (t["nread"] > 0).sum() >= 6 and t["nread"].sum() < t["taken"] == sum(1 for r in TABLE if not r["flag"] & 4)
    assert max(len(r["cigar"]) for r in TABLE) == 301 and {len(r["seq"]) for r in TABLE} >= {1, 2, 63, 64, 65, 300, 301}
    assert {len(r["cigar"]) for r in TABLE} >= {64, 65, 129, 301}
    codes = [c for c, _ in bam_synth.edge_bad_records()]
    assert set(codes) == set(range(1, 10))


def test_edge_records_survive_a_bam_round_trip(tmp_path):
    path = str(tmp_path / "edge.bam")
    bam_synth.write_records(path, TABLE)
    got, exp = bam_twin.tallies(bam_twin.read_records(path)), twin(TABLE)
    for k in ("subst", "indel", "qhist", "tlen", "nread", "minlen"):
        assert np.array_equal(got[k], exp[k]), k
    s = bam_twin.read_records(path)[[r["name"] for r in TABLE].index("tags_all_md_last")]
    assert s.tags["Xf"] == 1.5 and s.tags["XI"] == 4000000000 and s.tags["Be"] == [1, 65535, 77, 0, 5] and s.tags["Ba"] == []


def _agree(label, data, grid):
    ref = kde_ref.cdf_scipy(data, grid)
    hp, bound = kde_ref.cdf_decimal(kde_ref.moved(data), grid, with_bound=True)
    assert np.all(np.diff(hp) >= 0) and hp[-1] == 1.0
    if np.isnan(ref).all():
        print("%-28s scipy all NaN (every term underflows)" % label)
        return None
    e_ref = float(np.max(np.abs(ref - hp)))
    print("%-28s e_ref %.3g a-priori bound %.3g" % (label, e_ref, bound))
    assert e_ref <= max(1e-12, bound), (label, e_ref, bound)
    return e_ref


def test_decimal_reference_agrees_with_scipy_on_quality_cases():
    seen = {case: _agree(case, col, kde_ref.Q_GRID) for case, col in kde_ref.q_case_data().items()}
    assert sorted(case for case, e in seen.items() if e is None) == sorted(kde_ref.NAN_CASES)
    recs, quals = kde_ref.shape_reads()
    assert _agree("varlen_minlen_minus_1", [q[3] for q in quals[(1, 0)]], kde_ref.Q_GRID) is not None
    assert _agree("count_%d" % kde_ref.BIG, kde_ref.BIG_DATA, kde_ref.Q_GRID) is not None


@pytest.mark.parametrize("case", sorted(kde_ref.ISIZE_CASES))
def test_decimal_reference_agrees_with_scipy_on_insert_sizes(case):
    for read_length in (1, 301):
        isd, grid = kde_ref.isize_grid(kde_ref.ISIZE_CASES[case], read_length)
        assert _agree("%s rl=%d" % (case, read_length), isd, grid) is not None


def test_slice_reads_put_the_columns_where_they_say():
    for (mate, b), cols in kde_ref.Q_SLICES.items():
        recs, pos = kde_ref.slice_reads(mate, b, cols, "s")
        t = twin(recs)
        assert t["nread"][mate, b] == len(recs) and t["nread"].sum() == len(recs)
        for case, col in cols.items():
            assert np.array_equal(t["qhist"][mate, b, pos[case]], np.bincount(col, minlength=94).astype(np.uint64)), case
