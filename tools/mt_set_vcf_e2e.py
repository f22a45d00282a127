#!/usr/bin/env python3
"""`generate --rng mt --model novaseq --cpus W --devices 1 --store_mutations` end to end: wall time of
the whole command on one random 5 Mbp record, FASTQ and VCF on /dev/shm.  `--tree DIR` runs the command of another checkout
(the parent commit built next to this one: there -M takes one GPU process per worker, so W <= 16 on a shared box); `--plain`
leaves --store_mutations out (the ceiling); `--profile DIR` runs the command under `rocprofv3 --kernel-trace --stats` (its
files under DIR; the wall time then means nothing).  The parent tree is made with
    mkdir -p build_ab/parent && git archive HEAD~1 | tar -x -C build_ab/parent && python build_ab/parent/__graft_entry__.py
and the runs of the trees to compare are made interleaved by the caller, e.g.
    for rep in 1 2 3; do python tools/mt_set_vcf_e2e.py 16 2; python tools/mt_set_vcf_e2e.py 16 2 --tree build_ab/parent; done
    python tools/mt_set_vcf_e2e.py [W] [million read pairs] [--tree DIR] [--plain] [--profile DIR]"""
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import random_genome  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
tree = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else ROOT
if "--tree" in sys.argv:
    args.remove(sys.argv[sys.argv.index("--tree") + 1])
profile = []
if "--profile" in sys.argv:
    args.remove(sys.argv[sys.argv.index("--profile") + 1])
    profile = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.abspath(sys.argv[sys.argv.index("--profile") + 1]), "-o", "set_vcf", "--"]
plain = "--plain" in sys.argv
W = int(args[0]) if args else 64
pairs = int(float(args[1]) * 1e6) if len(args) > 1 else 8_000_000
tmp = "/dev/shm/mt_set_vcf_e2e"
shutil.rmtree(tmp, ignore_errors=True)
os.makedirs(tmp)
fasta = os.path.join(tmp, "g.fasta")
with open(fasta, "wb") as fh:
    fh.write(b">rec0\n" + random_genome(11, 5_000_000).encode() + b"\n")
out = os.path.join(tmp, "run")
t0 = time.perf_counter()
p = subprocess.run(profile + [sys.executable, "-m", "insilicoseq_amd", "generate", "--genomes", fasta, "--model", "novaseq", "-n", str(2 * pairs),
                    "--seed", "7", "--cpus", str(W), "--devices", "1", "--rng", "mt", "-o", out] + ([] if plain else ["--store_mutations"]),
                   cwd=tree, stderr=subprocess.PIPE)
dt = time.perf_counter() - t0
if p.returncode != 0:
    sys.exit(p.stderr.decode(errors="replace")[-3000:])
fastq = sum(os.path.getsize(out + s) for s in ("_R1.fastq", "_R2.fastq"))
vcf = 0 if plain else os.path.getsize(out + ".vcf")
print("%s W = %d%s: %d pairs -> %.2f GB of FASTQ, %.1f MB of VCF in %.2f s: %.3g pairs/s for the command (%s)" % (
    os.path.relpath(tree, ROOT) if tree != ROOT else "this tree", W, " without -M" if plain else "", pairs, fastq / 1e9, vcf / 1e6, dt,
    pairs / dt, "worker set" if b"workers side by side on one device" in p.stderr else "one process per worker"))
shutil.rmtree(tmp, ignore_errors=True)
