"""`model` on the host: the BGZF reader and record scan against the pysam stand-in, the synthetic BAM writer, the host finish
(substitution / indel choices, read length, the .npz schema) against the reference's own `iss model` output, the subsample's
selection law and stop rule, and the errors the CLI reports before it needs a GPU.  No GPU compute here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_synth
import bam_twin
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, "bam", "cases.json")))
ECOLI_BAM = os.path.join(GOLDEN, "bam", "ecoli.bam")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import _native

    return _native


def case_bam(tmp_path, name):
    path = str(tmp_path / ("case_%s.bam" % name))
    assert bam_synth.write_records(path, bam_synth.case_records(CASES[name]["parts"])) == CASES[name]["sha256"]
    return path


def reader_records(path, chunk_bytes):
    from insilicoseq_amd.bam import BamReader

    out = []
    for ch in BamReader(path, chunk_bytes=chunk_bytes).chunks():
        for o in ch.offsets:
            bs = int(np.frombuffer(ch.data[o:o + 4].tobytes(), "<i4")[0])
            out.append(ch.data[o + 4:o + 4 + bs].tobytes())
    return out


@pytest.mark.parametrize("name", ["ecoli", "a", "b", "c", "d"])
def test_reader_agrees_with_pysam_shim(native, tmp_path, name):
    path = ECOLI_BAM if name == "ecoli" else case_bam(tmp_path, name)
    pysam = bam_twin.shim()
    ref = pysam._parse(path)[1]
    for chunk_bytes in (4096, 64 << 20):  # many chunks (records straddle chunk ends) and one
        got = reader_records(path, chunk_bytes)
        assert len(got) == len(ref)
        for raw, r in zip(got, ref):
            s = pysam.AlignedSegment(raw)
            assert (s.flag, s.template_length, s.cigartuples, s.query_sequence, list(s.query_qualities), s.tags) == \
                   (r.flag, r.template_length, r.cigartuples, r.query_sequence, list(r.query_qualities), r.tags)


def test_mapped_count_matches_index_stats(native, tmp_path):
    from insilicoseq_amd.bam import BamReader, mapped_mask

    for path in (ECOLI_BAM, case_bam(tmp_path, "a")):
        n = sum(int(mapped_mask(ch).sum()) for ch in BamReader(path).chunks())
        stats = bam_twin.shim().idxstats(path)
        assert n == sum(int(line.split("\t")[2]) for line in stats.splitlines())


def test_synthetic_bam_is_deterministic(tmp_path):
    a, b, c = (str(tmp_path / x) for x in "abc")
    assert bam_synth.write_bam(a, 7, n_pairs=300) == bam_synth.write_bam(b, 7, n_pairs=300)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert bam_synth.write_bam(c, 8, n_pairs=300) != bam_synth.write_bam(a, 7, n_pairs=300)
    blob = open(a, "rb").read()
    assert blob.endswith(bam_synth.BGZF_EOF) and blob[12:16] == b"BC\x02\x00"


def _finish_from_golden(name, tmp_path):
    """The host finish on the twin's tallies of a golden case, with the golden's own CDFs in place of the device's."""
    from insilicoseq_amd import modeller

    path = ECOLI_BAM if name == "ecoli" else case_bam(tmp_path, name)
    t = bam_twin.tallies(bam_twin.read_records(path))
    z = np.load(os.path.join(GOLDEN, "models", "bam_%s.npz" % name), allow_pickle=True)
    rl = modeller.read_length_of(t["nread"], t["minlen"])
    qcdf = np.full((2, 4, 301, 41), np.nan)
    for m, key in enumerate(("quality_hist_forward", "quality_hist_reverse")):
        for b in range(4):
            rows = list(z[key][b])
            if len(rows):
                qcdf[m, b, :len(rows)] = np.array(rows, dtype=np.float64)
    f = modeller.finish(t, qcdf, z["insert_size"], rl)
    return f, z


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_finish_matches_reference_on_count_inputs(tmp_path, name):
    f, z = _finish_from_golden(name, tmp_path)
    assert f["read_length"] == int(z["read_length"])
    assert f["mean_f"] == list(z["mean_count_forward"]) and f["mean_r"] == list(z["mean_count_reverse"])
    for mine, key in (("sub_f", "subst_choices_forward"), ("sub_r", "subst_choices_reverse"), ("ins_f", "ins_forward"),
                      ("ins_r", "ins_reverse"), ("del_f", "del_forward"), ("del_r", "del_reverse")):
        ref = list(z[key])
        assert len(f[mine]) == len(ref)
        for a, b in zip(f[mine], ref):
            assert list(a) == list(b)
            for k in a:
                va, vb = (a[k], b[k]) if mine.startswith("sub") else (([], [a[k]]), ([], [b[k]]))
                assert va[0] == vb[0]
                assert np.array_equal(np.array(va[1], dtype=np.float64), np.array(vb[1], dtype=np.float64), equal_nan=True), (mine, k)


def test_written_schema_matches_reference(tmp_path):
    from insilicoseq_amd import modeller

    f, z = _finish_from_golden("a", tmp_path)
    out = str(tmp_path / "m.npz")
    modeller.write_npz(out, f)
    m = np.load(out, allow_pickle=True)
    assert m.files == z.files
    for k in z.files:
        assert m[k].dtype == z[k].dtype and m[k].shape == z[k].shape, k
    for key in ("subst_choices_forward", "ins_forward", "del_reverse"):
        for a, b in zip(m[key], z[key]):
            assert list(a) == list(b)
            assert [type(v) for v in a.values()] == [type(v) for v in b.values()]
    a, b = m["subst_choices_forward"][0], z["subst_choices_forward"][0]
    assert [a[k][0] for k in a] == [b[k][0] for k in b] == [["T", "C", "G"], ["A", "C", "G"], ["A", "T", "G"], ["A", "T", "C"]]
    assert [type(x) for x in a["A"][1]] == [type(x) for x in b["A"][1]]


def test_subst_choices_zero_row_is_one_third():
    from insilicoseq_amd.modeller import subst_matrix_to_choices

    m = np.zeros((2, 16))
    m[1, 1:4] = [1, 0, 3]
    c = subst_matrix_to_choices(m, 2)
    assert c[0]["A"] == (["T", "C", "G"], [1 / 3, 1 / 3, 1 / 3]) and type(c[0]["A"][1][0]) is float
    assert c[1]["A"][1] == [0.25, 0.0, 0.75] and isinstance(c[1]["A"][1][0], np.float64)


def test_subsample_law_and_stop_rule():
    from insilicoseq_amd.bam import Subsample

    rng = np.random.RandomState(3)
    mapped = rng.rand(50000) < 0.9
    total = int(mapped.sum())
    # fraction >= 1: every mapped record, whatever the seed
    s = Subsample(total, total, seed=5)
    assert np.array_equal(s.select(mapped).astype(bool), mapped)
    n_reads = total // 3
    sels = []
    for seed in (11, 11, 12):
        s = Subsample(total, n_reads, seed)
        sel = np.concatenate([s.select(mapped[i:i + 7000]) for i in range(0, mapped.size, 7000)]).astype(bool)
        assert not (sel & ~mapped).any()
        sels.append(sel)
        p = n_reads / total
        sd = (total * p * (1 - p)) ** 0.5
        k = int(sel.sum())
        assert k <= n_reads + 1 or abs(k - n_reads) < 6 * sd
        # the stop rule: nothing is taken after the first record that is not taken once n_reads were taken
        c = np.cumsum(sel) - sel
        stops = np.flatnonzero(~sel & (c >= n_reads))
        if stops.size:
            assert not sel[stops[0]:].any()
    assert np.array_equal(sels[0], sels[1]) and not np.array_equal(sels[0], sels[2])
    # a fraction of 1/2 over a long file: the count stays within binomial bounds of n * fraction while it runs
    s = Subsample(200000, 100000, 1)
    sel = s.select(np.ones(150000, bool))
    assert abs(int(sel.sum()) - 75000) < 6 * (150000 * 0.25) ** 0.5


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "insilicoseq_amd", "model", "-q"] + args, cwd=cwd, env=env, capture_output=True, text=True)


def test_cli_not_a_bam_exits_1_with_one_line(native, tmp_path):
    for content in (b"", b"this is not a bam file\n" * 10, bam_synth.bgzf(b"SAM\x01" + b"\0" * 64)):
        p = tmp_path / "x.bam"
        p.write_bytes(content)
        r = _cli(["-b", str(p), "-o", str(tmp_path / "out")], str(tmp_path))
        assert r.returncode == 1, r.stderr
        assert len(r.stderr.strip().splitlines()) == 1 and "not a BAM" in r.stderr, r.stderr
    r = _cli(["-b", str(tmp_path / "missing.bam"), "-o", str(tmp_path / "out")], str(tmp_path))
    assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1 and "Traceback" not in r.stderr
