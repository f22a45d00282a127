#!/usr/bin/env python3
"""Golden outputs of `iss generate --cpus 12` and `--cpus 11`: the reference's own parallelism with two-digit worker numbers
(read ids "{id}_{i}_{cpu}/m" with cpu 10 and 11), captured by running the reference like make_golden_cpus8.py does (same
stand-in Bio package).  The worker set (iss_fastq_emit_scatter: one text job holds items of workers 9, 10 and 11, every one
at its own offset of the final files) must reproduce the files byte for byte.

Outputs: tests/golden/generate/syn3_novaseq_n3000_seed7_cpus12.npz  (the three 20 kbp records of the cpus8 fixture: twelve
                                                                      chunks of 125 pairs, records split across workers)
         tests/golden/generate/genomes_hiseq_n1600_seed42_cpus11.npz (data/genomes.fasta: uneven chunks, worker 10 alone at
                                                                      width 2)

Usage:  python tests/golden/tooling/make_golden_cpus12.py   (from the repo root, build container only)
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
SHIM = os.path.join(HERE, "bio_shim")
REF = "/root/reference"

work = tempfile.mkdtemp(prefix="iss_ref_")
REFCOPY = os.path.join(work, "refcopy")
shutil.copytree(REF, REFCOPY)
subprocess.check_call(["chmod", "-R", "u+w", REFCOPY])
env = dict(os.environ, PYTHONPATH=SHIM + ":" + REFCOPY)
os.makedirs(os.path.join(GOLDEN, "generate"), exist_ok=True)


def run(name, fasta, model, n, seed, cpus):
    outp = os.path.join(work, name)
    subprocess.check_call([sys.executable, "-m", "iss", "generate", "--genomes", fasta, "--model", model, "-n", str(n),
                           "--seed", str(seed), "--cpus", str(cpus), "-o", outp, "--quiet"], env=env, cwd=REFCOPY)
    blob = lambda suffix: np.frombuffer(open(outp + suffix, "rb").read(), dtype=np.uint8)  # noqa: E731
    r1, r2, ab = blob("_R1.fastq"), blob("_R2.fastq"), blob("_abundance.txt")
    # every worker wrote a chunk (else the reference fails on the missing temp file and this run takes the temp-file path)
    last = {int(line.rsplit(b"_", 1)[1].split(b"/")[0]) for line in r1.tobytes().split(b"\n")[0::4] if line}
    assert last == set(range(cpus)), (name, sorted(last))
    return r1, r2, ab


syn = np.load(os.path.join(GOLDEN, "generate", "syn3_novaseq_n3000_seed7_cpus8.npz"))
fasta = os.path.join(work, "syn3.fasta")
with open(fasta, "wb") as fh:
    fh.write(syn["fasta"].tobytes())
r1, r2, ab = run("s12", fasta, "novaseq", 3000, 7, 12)
np.savez_compressed(os.path.join(GOLDEN, "generate", "syn3_novaseq_n3000_seed7_cpus12.npz"), r1=r1, r2=r2, abundance=ab,
                    fasta=syn["fasta"])
print("syn3_novaseq cpus12", len(r1), len(r2))

r1, r2, ab = run("g11", "data/genomes.fasta", "hiseq", 1600, 42, 11)
np.savez_compressed(os.path.join(GOLDEN, "generate", "genomes_hiseq_n1600_seed42_cpus11.npz"), r1=r1, r2=r2, abundance=ab)
print("genomes_hiseq cpus11", len(r1), len(r2))
shutil.rmtree(work, ignore_errors=True)
