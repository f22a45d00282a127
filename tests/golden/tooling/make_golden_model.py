#!/usr/bin/env python3
"""Goldens of `model`: the reference's own `iss model` (iss/app.py:147-169 -> iss/bam.py:103-227 -> iss/modeller.py, scipy's
gaussian_kde) on synthetic BAM files of tests/bam_synth.py, run on the pysam stand-in like make_golden_bam_model.py.

Cases (tests/golden/bam/cases.json holds each case's recipe and the sha256 of its BAM; the BAMs are rebuilt by the tests):
  a  2 x 151, 8000 pairs with every quirk of tests/bam_synth.py (secondary / supplementary / unmapped / neither-mate / unpaired
     records, clips, N, long early deletions whose wrapped rows fall past read_length)
  b  301-base reads with many long early deletions (read_length == 301 keeps the wrapped indel rows), plus variable-length reads
     the model does not bin (mean quality 40 and above, records flagged neither read1 nor read2)
  c  every read holds quality 35 at positions 0..4 (np.std == 0 there: the reference's LinAlgError branch) and one read1 sits
     alone in the lowest mean-quality bin (a bin with exactly one read)
  d  the valid hand-built records of bam_synth.edge_table() (CIGARs of up to 301 operations, reads of 1 to 301 bases, clips, wrapped
     indel rows, MD and optional-field variants, mean qualities at the bin borders, template lengths at the limits, flag
     combinations) and edge_fillers(): short pairs that give every (mate, bin) two reads and the template lengths a spread

Outputs: tests/golden/models/bam_{a,b,c,d}.npz (the reference's raw .npz), tests/golden/models/bam_a.dense.npz,
tests/golden/bam/cases.json.

Usage:  python tests/golden/tooling/make_golden_model.py [case ...]   (from the repo root, build container only; no case: all)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
REPO = os.path.dirname(os.path.dirname(GOLDEN))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import bam_synth  # noqa: E402

CASES = {
    "a": [dict(seed=101, n_pairs=8000, read_length=151)],
    "b": [dict(seed=202, n_pairs=1200, read_length=301, long_del_rate=0.08, p_indel=0.02),
          dict(seed=203, n_pairs=150, read_length=151, var_lengths=[40, 300], qual_mode="high", quirks=False),
          dict(seed=204, n_pairs=100, read_length=151, var_lengths=[40, 300], quirks=True, neither=True)],
    "c": [dict(seed=303, n_pairs=400, read_length=101, qual_mode="const_head"),
          dict(seed=304, n_pairs=1, read_length=101, qual_mode="const_head", quirks=False, read1_level=5)],
    "d": [dict(edge_table=True)],
}


def main():
    work = tempfile.mkdtemp(prefix="iss_ref_model_")
    refcopy = os.path.join(work, "refcopy")
    shutil.copytree(REF, refcopy)
    subprocess.check_call(["chmod", "-R", "u+w", refcopy])
    paths = [os.path.join(HERE, "pysam_shim"), os.path.join(HERE, "bio_shim"), refcopy]
    env = dict(os.environ, PYTHONPATH=":".join(paths))
    # the reference's own tests of the BAM reader and the modeller must pass on the stand-in
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "iss/test/test_bam.py", "iss/test/test_modeller.py"],
                          env=env, cwd=refcopy)
    cases_json = os.path.join(GOLDEN, "bam", "cases.json")
    meta = json.load(open(cases_json)) if os.path.exists(cases_json) else {}
    for name, parts in CASES.items():
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        bam = os.path.join(work, "case_%s.bam" % name)
        sha = bam_synth.write_records(bam, bam_synth.case_records(parts))
        out = os.path.join(work, "case_%s" % name)
        subprocess.check_call([sys.executable, "-m", "iss", "model", "-b", bam, "-o", out], env=env, cwd=refcopy)
        shutil.copy(out + ".npz", os.path.join(GOLDEN, "models", "bam_%s.npz" % name))
        meta[name] = dict(parts=parts, sha256=sha)
        print("case", name, sha)
    if not sys.argv[1:] or "a" in sys.argv[1:]:
        from insilicoseq_amd.model import DenseModel

        DenseModel.from_reference_npz(os.path.join(GOLDEN, "models", "bam_a.npz")).save(os.path.join(GOLDEN, "models", "bam_a.dense.npz"))
    with open(cases_json, "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
