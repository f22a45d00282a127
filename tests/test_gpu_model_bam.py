"""`model` on the MI355X: the device tallies against a plain-Python twin, the models against the reference's own `iss model`
(exact where the fields come from integer tallies, within 1e-12 where they come from the KDEs), the subsample, reproducibility,
the errors the reference fails on, and `generate` with a model built here."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import bam_synth
import bam_twin
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, "bam", "cases.json")))
ECOLI_BAM = os.path.join(GOLDEN, "bam", "ecoli.bam")
KDE_TOL = 1e-12
EXACT = ("read_length", "bin_cdf", "bin_nonempty", "subst_cdf", "subst_alt", "ins", "ins_letter", "dele")
KDE = ("qcdf", "isize_cdf")


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd.engine import BamTally

    with BamTally(0) as d:
        yield d


def case_bam(tmp_path, name):
    path = str(tmp_path / ("case_%s.bam" % name))
    assert bam_synth.write_records(path, bam_synth.case_records(CASES[name]["parts"])) == CASES[name]["sha256"]
    return path


def device_tallies(dev, path, **kw):
    from insilicoseq_amd import modeller

    modeller.tally_bam(dev, path, **kw)
    words, bad, code = dev.tallies()
    assert bad == -1, (bad, code)
    return modeller.unpack_tallies(words)


def assert_tallies_equal(got, exp):
    for k in ("subst", "indel", "qhist", "tlen", "nread", "minlen"):
        assert np.array_equal(got[k], exp[k]), k
    assert got["taken"] == exp["taken"]


def compare_dense(got, exp, label):
    worst = 0.0
    assert got.read_length == exp.read_length, label
    for k in EXACT[1:]:
        assert np.array_equal(getattr(got, k), getattr(exp, k), equal_nan=True), (label, k)
    for k in KDE:
        a, b = getattr(got, k), getattr(exp, k)
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (label, k)
        d = float(np.nanmax(np.abs(a - b))) if a.size else 0.0
        assert d <= KDE_TOL, (label, k, d)
        worst = max(worst, d)
    print("%s: KDE fields within %.3g of the reference" % (label, worst))
    return worst


def test_ecoli_bam_matches_reference_model(dev, tmp_path):
    from insilicoseq_amd.model import DenseModel
    from insilicoseq_amd.modeller import to_model

    out = to_model(ECOLI_BAM, str(tmp_path / "ecoli"), dense=True)
    got = DenseModel.from_reference_npz(out)
    compare_dense(got, DenseModel.load(os.path.join(GOLDEN, "models", "ecoli-bam.dense.npz")), "ecoli.bam")
    compare_dense(DenseModel.load(str(tmp_path / "ecoli.dense.npz")), got, "ecoli.bam dense file")


def _cdf_rows(x):
    return [np.asarray(r, dtype=np.float64) for r in x]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_golden_cases_match_reference_npz(dev, tmp_path, name):
    from insilicoseq_amd.modeller import to_model

    out = to_model(case_bam(tmp_path, name), str(tmp_path / name))
    m = np.load(out, allow_pickle=True)
    z = np.load(os.path.join(GOLDEN, "models", "bam_%s.npz" % name), allow_pickle=True)
    assert m.files == z.files
    assert int(m["read_length"]) == int(z["read_length"])
    for k in ("mean_count_forward", "mean_count_reverse"):
        assert np.array_equal(m[k], z[k]), k
    for k in ("subst_choices_forward", "subst_choices_reverse", "ins_forward", "ins_reverse", "del_forward", "del_reverse"):
        assert pickle.dumps(list(m[k])) == pickle.dumps(list(z[k])) or all(
            str(a) == str(b) for a, b in zip(m[k], z[k])), k  # NaN != NaN: compare the printed values then
        assert len(m[k]) == len(z[k])
    worst = float(np.max(np.abs(m["insert_size"] - z["insert_size"])))
    for k in ("quality_hist_forward", "quality_hist_reverse"):
        for b in range(4):
            a, r = _cdf_rows(m[k][b]), _cdf_rows(z[k][b])
            assert len(a) == len(r), (k, b)
            for x, y in zip(a, r):
                assert np.array_equal(np.isnan(x), np.isnan(y))
                if x.size:
                    worst = max(worst, float(np.nanmax(np.abs(x - y))))
    print("case %s: KDE fields within %.3g of the reference" % (name, worst))
    assert worst <= KDE_TOL


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_tallies_equal_python_twin(dev, tmp_path, seed):
    kw = [dict(n_pairs=1500), dict(n_pairs=1500, var_lengths=(30, 301), long_del_rate=0.05),
          dict(n_pairs=1200, read_length=250, qual_mode="binned", p_indel=0.05, p_sub=0.05, p_n=0.02),
          dict(n_pairs=1500, read_length=36, qual_mode="uniform")][seed - 1]
    path = str(tmp_path / "r.bam")
    bam_synth.write_bam(path, 1000 + seed, **kw)
    assert_tallies_equal(device_tallies(dev, path, chunk_bytes=1 << 16), bam_twin.tallies(bam_twin.read_records(path)))


def test_subsample_on_device(dev, tmp_path):
    from insilicoseq_amd.bam import BamReader, Subsample, mapped_mask

    path = str(tmp_path / "s.bam")
    bam_synth.write_bam(path, 77, n_pairs=3000)
    reads = bam_twin.read_records(path)
    total = sum(1 for r in reads if not r.is_unmapped)
    n_reads = total // 4
    t1 = device_tallies(dev, path, n_reads=n_reads, seed=9, chunk_bytes=1 << 15)
    t2 = device_tallies(dev, path, n_reads=n_reads, seed=9, chunk_bytes=1 << 17)
    assert_tallies_equal(t1, t2)
    t3 = device_tallies(dev, path, n_reads=n_reads, seed=10)
    assert not np.array_equal(t1["subst"], t3["subst"])
    # the selection on the host, chunk by chunk as the driver makes it; the tallies equal a full run over just those records
    sub = Subsample(total, n_reads, 9)
    sel = np.concatenate([sub.select(mapped_mask(ch)) for ch in BamReader(path, 1 << 15).chunks()]).astype(bool)
    k = int(sel.sum())
    p = n_reads / total
    assert abs(k - min(n_reads, total * p)) <= 6 * (total * p * (1 - p)) ** 0.5 + 1
    assert t1["taken"] == k
    c = np.cumsum(sel) - sel
    stops = np.flatnonzero(~sel & (c >= n_reads))
    if stops.size:
        assert not sel[stops[0]:].any()
    recs = [r for r, s in zip(bam_synth.records(77, n_pairs=3000), sel) if s]
    path2 = str(tmp_path / "sel.bam")
    bam_synth.write_records(path2, recs)
    assert_tallies_equal(t1, device_tallies(dev, path2))


def test_same_bam_twice_gives_identical_tables(dev, tmp_path):
    from insilicoseq_amd.modeller import to_model

    path = case_bam(tmp_path, "c")
    a = np.load(to_model(path, str(tmp_path / "one")), allow_pickle=True)
    b = np.load(to_model(path, str(tmp_path / "two"), chunk_bytes=1 << 14), allow_pickle=True)
    for k in a.files:
        assert pickle.dumps(a[k]) == pickle.dumps(b[k]), k


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "insilicoseq_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=600)


def _edit(rec, **kw):
    r = dict(rec)
    r.update(kw)
    return r


def test_cli_errors_exit_1_with_one_line(dev, tmp_path):
    base = bam_synth.records(5, n_pairs=60, quirks=False)
    r0 = base[0]
    bad = {
        "no MD": [_edit(r0, tags=[("NM", "i", 0)])],
        "qualities": [_edit(r0, qual=None)],
        "longer than 301": [_edit(r0, seq="A" * 302, qual=[30] * 302, cigar=[(0, 302)], tags=[("MD", "Z", "302")])],
        "CIGAR operation": [_edit(r0, cigar=[(7, len(r0["seq"]))], tags=[("MD", "Z", str(len(r0["seq"])))])],
        "indel position": [_edit(r0, seq="ACGTACGTAN" + "A" * 10, qual=[30] * 20, cigar=[(0, 2), (2, 30), (1, 3), (0, 15)],
                                 tags=[("MD", "Z", "2^" + "A" * 30 + "0N14")])],
        "no paired": [_edit(r, flag=r["flag"] & ~1) for r in base],
    }
    for what, recs in bad.items():
        path = str(tmp_path / "bad.bam")
        bam_synth.write_records(path, base[1:] + recs if what != "no paired" else recs)
        res = _cli(["model", "-q", "-b", path, "-o", str(tmp_path / "out")], str(tmp_path))
        lines = res.stderr.strip().splitlines()
        assert res.returncode == 1 and len(lines) == 1 and lines[0].startswith("ERROR"), (what, res.stderr)
        assert what.split()[-1].lower() in lines[0].lower() or what == "indel position" and "indel" in lines[0], (what, lines[0])


def test_model_then_generate(dev, tmp_path):
    from helpers import random_genome
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.model import DenseModel

    res = _cli(["model", "-q", "-b", case_bam(tmp_path, "a"), "-o", str(tmp_path / "m"), "--dense"], str(tmp_path))
    assert res.returncode == 0, res.stderr
    ours = DenseModel.load(str(tmp_path / "m.dense.npz"))
    ref = DenseModel.load(os.path.join(GOLDEN, "models", "bam_a.dense.npz"))
    genome = random_genome(3, 50000)
    rows = []
    for d in (ours, ref):
        with ReadEngine(0) as eng:
            eng.load_model(d)
            gid = eng.add_genome(genome)
            eng.generate(gid, 2000, first_ordinal=0, seed=123)
            eng.synchronize()
            rows.append(eng.download(0, 2000))
    for k in ("r1_base", "r1_qual", "r2_base", "r2_qual"):
        assert np.array_equal(rows[0][k], rows[1][k]), k
    fasta = tmp_path / "g.fasta"
    fasta.write_text(">g\n" + genome.decode() + "\n" if isinstance(genome, bytes) else ">g\n" + genome + "\n")
    res = _cli(["generate", "-q", "-g", str(fasta), "-m", str(tmp_path / "m.npz"), "-n", "200", "--rng", "mt", "--seed", "1",
                "-o", str(tmp_path / "reads")], str(tmp_path))
    assert res.returncode == 0, res.stderr
    assert os.path.getsize(str(tmp_path / "reads_R1.fastq")) > 0
