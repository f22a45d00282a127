#!/usr/bin/env python3
"""Golden vectors of the reference's PerfectErrorModel (`iss generate --mode perfect`), captured by running the
reference like make_golden_basic.py does (same stand-in Bio package, a private copy of the reference).

The pinned reference's PerfectErrorModel never sets ``store_mutations``, which ``mut_sequence`` reads at its first error
event (iss/error_models/__init__.py:98): the copy gets ``PerfectErrorModel.store_mutations = False`` appended to
iss/error_models/perfect.py before anything runs -- in the source, so that the worker processes of ``--cpus N`` see it too.
Nothing else of the reference changes.

Outputs: tests/golden/generate/perfect_*.npz (R1, R2, _abundance.txt of each run, its command line) and
tests/golden/generate/perfect_mixed.fasta (the mixed-case / IUPAC genome of the `mixed` case).

Usage:  python tests/golden/tooling/make_golden_perfect.py   (from the repo root, build container only)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
REPO = os.path.dirname(os.path.dirname(GOLDEN))
SHIM = os.path.join(HERE, "bio_shim")
REF = "/root/reference"
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from helpers import mixed_genome  # noqa: E402

work = tempfile.mkdtemp(prefix="iss_ref_")
REFCOPY = os.path.join(work, "refcopy")
shutil.copytree(REF, REFCOPY)
subprocess.check_call(["chmod", "-R", "u+w", REFCOPY])
with open(os.path.join(REFCOPY, "iss", "error_models", "perfect.py"), "a") as fh:
    fh.write("\n\nPerfectErrorModel.store_mutations = False  # (golden tooling: the attribute the pinned reference lacks)\n")
env = dict(os.environ, PYTHONPATH=SHIM + ":" + REFCOPY)

# the mixed-case / IUPAC genome: two records, short enough that the reads overlap (the files compress to tens of kB) and
# with enough lower-case a/c/g/t that several of them are upper-cased (about 1e-4 per base)
MIXED = os.path.join(GOLDEN, "generate", "perfect_mixed.fasta")
with open(MIXED, "w") as fh:
    for rid, seed, n in (("mixed_a", 11, 1500), ("mixed_b", 12, 900)):
        seq = mixed_genome(seed, n)
        fh.write(">%s seeded mixed-case / IUPAC record\n" % rid)
        for k in range(0, n, 60):
            fh.write(seq[k:k + 60] + "\n")
GENOMES = os.path.join(REPO, "tests", "golden", "genomes.fasta")

# (case, fasta, extra arguments); every run: --mode perfect --seed 42 (mixed: 7)
CASES = [
    ("perfect_genomes_cpus1", GENOMES, ["-n", "600", "--seed", "42", "--cpus", "1"]),
    ("perfect_genomes_cpus2", GENOMES, ["-n", "600", "--seed", "42", "--cpus", "2"]),
    ("perfect_genomes_cpus3", GENOMES, ["-n", "600", "--seed", "42", "--cpus", "3"]),
    ("perfect_mixed", MIXED, ["-n", "8000", "--seed", "7", "--cpus", "2"]),
    ("perfect_frag300", GENOMES, ["-n", "400", "--seed", "43", "--cpus", "2", "-l", "300", "-s", "30"]),
    ("perfect_amplicon", GENOMES, ["-n", "200", "--seed", "44", "--cpus", "1", "--sequence_type", "amplicon"]),
    ("perfect_gcbias", GENOMES, ["-n", "400", "--seed", "45", "--cpus", "2", "--gc_bias"]),
]

for case, fasta, extra in CASES:
    outp = os.path.join(work, case)
    subprocess.check_call([sys.executable, "-m", "iss", "generate", "--genomes", fasta, "--mode", "perfect", "-o", outp,
                           "--quiet"] + extra, env=env, cwd=REFCOPY)
    blobs = {}
    for suffix in ("_R1.fastq", "_R2.fastq", "_abundance.txt"):
        with open(outp + suffix, "rb") as fh:
            blobs[suffix] = np.frombuffer(fh.read(), dtype=np.uint8)
    meta = dict(case=case, fasta=os.path.relpath(fasta, os.path.join(REPO, "tests", "golden")), args=extra)
    np.savez_compressed(os.path.join(GOLDEN, "generate", case + ".npz"), r1=blobs["_R1.fastq"], r2=blobs["_R2.fastq"],
                        abundance=blobs["_abundance.txt"], meta=np.array(json.dumps(meta)))
    r1 = blobs["_R1.fastq"].tobytes().decode()
    print(case, r1.count("\n") // 4, "pairs;", os.path.getsize(os.path.join(GOLDEN, "generate", case + ".npz")), "bytes")
shutil.rmtree(work, ignore_errors=True)
