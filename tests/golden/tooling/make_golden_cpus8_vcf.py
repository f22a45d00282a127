#!/usr/bin/env python3
"""Golden outputs of `iss generate --cpus 8 --store_mutations`: the two runs of make_golden_cpus8.py with the flag, captured
from the reference the same way (same stand-in Bio package).  The reference's parent concatenates its eight workers' .vcf
temp files behind the header (iss/app.py:125-133); the worker set (iss_generate_mt_workers with rows per worker,
iss_vcf_emit_workers) must reproduce all four files byte for byte.  The flag changes no draw: r1 / r2 equal the cpus8 goldens.

Outputs: tests/golden/generate/genomes_hiseq_n1600_seed42_cpus8_vcf.npz   r1, r2, vcf, abundance
         tests/golden/generate/syn3_novaseq_n3000_seed7_cpus8_vcf.npz     r1, r2, vcf, abundance, fasta

Usage:  python tests/golden/tooling/make_golden_cpus8_vcf.py   (from the repo root, build container only)
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
SHIM = os.path.join(HERE, "bio_shim")
REF = "/root/reference"
WORKERS = 8

work = tempfile.mkdtemp(prefix="iss_ref_vcf_")
REFCOPY = os.path.join(work, "refcopy")
shutil.copytree(REF, REFCOPY)
subprocess.check_call(["chmod", "-R", "u+w", REFCOPY])
env = dict(os.environ, PYTHONPATH=SHIM + ":" + REFCOPY)
os.makedirs(os.path.join(GOLDEN, "generate"), exist_ok=True)


def blob(path):
    return np.frombuffer(open(path, "rb").read(), dtype=np.uint8)


def run(name, fasta, model, n, seed):
    outp = os.path.join(work, name)
    subprocess.check_call([sys.executable, "-m", "iss", "generate", "--genomes", fasta, "--model", model, "-n", str(n),
                           "--seed", str(seed), "--cpus", str(WORKERS), "--store_mutations", "-o", outp, "--quiet"],
                          env=env, cwd=REFCOPY)
    out = {"r1": blob(outp + "_R1.fastq"), "r2": blob(outp + "_R2.fastq"), "vcf": blob(outp + ".vcf"),
           "abundance": blob(outp + "_abundance.txt")}
    # every worker contributes: a row's CHROM is "{record id}_{pair}_{worker}/{mate}"
    rows = [ln for ln in out["vcf"].tobytes().decode().splitlines() if ln and not ln.startswith("#")]
    seen = {int(re.match(r".*_\d+_(\d+)/[12]$", ln.split("\t")[0]).group(1)) for ln in rows}
    assert seen == set(range(WORKERS)), sorted(seen)
    return out, len(rows)


out, rows = run("g8", "data/genomes.fasta", "hiseq", 1600, 42)
np.savez_compressed(os.path.join(GOLDEN, "generate", "genomes_hiseq_n1600_seed42_cpus8_vcf.npz"), **out)
print("genomes_hiseq cpus8 vcf:", len(out["vcf"]), "bytes,", rows, "rows")

rng = np.random.RandomState(2024)  # (the records of make_golden_cpus8.py)
letters = np.frombuffer(b"ACGT", dtype=np.uint8)
fasta = os.path.join(work, "syn3.fasta")
text = b""
for k in range(3):
    seq = letters[rng.randint(0, 4, size=20000)].tobytes()
    text += b">syn_%d some description\n" % k + b"\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + b"\n"
with open(fasta, "wb") as fh:
    fh.write(text)
out, rows = run("s8", fasta, "novaseq", 3000, 7)
np.savez_compressed(os.path.join(GOLDEN, "generate", "syn3_novaseq_n3000_seed7_cpus8_vcf.npz"),
                    fasta=np.frombuffer(text, dtype=np.uint8), **out)
print("syn3_novaseq cpus8 vcf:", len(out["vcf"]), "bytes,", rows, "rows")
shutil.rmtree(work, ignore_errors=True)
