#!/usr/bin/env python3
"""Per-contig cost of draft-genome inputs end to end: synthetic contigs of 2-20 kbp (log-uniform),
NovaSeq model, one worker, `generate` as a user runs it.

Every size runs as `--genomes contigs.fasta --abundance_file <one value per contig>` -- the same records and pairs as
`--draft contigs.fasta`, and a command line a tree without --draft takes too, so `--root` can point at another checkout for
an A/B.  `--draft` adds a `--draft` run of the same contigs (this tree only).  Prints one line per run: seconds end to end
(process start to exit) and microseconds per contig.

Usage:  python tools/draft_bench.py [--root TREE] [--sizes 1000,10000,30000] [--pairs 10,1000] [--rng philox|mt] [--repeat 3]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_contigs(path, n, seed=1):
    rng = np.random.RandomState(seed)
    lengths = np.exp(rng.uniform(np.log(2000), np.log(20000), size=n)).astype(np.int64)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as fh:
        for k, L in enumerate(lengths):
            fh.write(b">contig_%d\n" % k)
            fh.write(letters[rng.randint(0, 4, size=int(L))].tobytes())
            fh.write(b"\n")
    return lengths


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=HERE, help="tree whose `python -m insilicoseq_amd` runs (default: this one)")
    p.add_argument("--sizes", default="1000,10000,30000")
    p.add_argument("--pairs", default="10,1000", help="pairs per contig")
    p.add_argument("--rng", default="philox")
    p.add_argument("--repeat", type=int, default=1)
    p.add_argument("--draft", action="store_true", help="also time --draft with the same contigs (needs this tree)")
    p.add_argument("--workdir", default=None)
    a = p.parse_args()
    work = tempfile.mkdtemp(dir=a.workdir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    env = dict(os.environ, PYTHONPATH=os.path.abspath(a.root))
    try:
        for n in [int(x) for x in a.sizes.split(",")]:
            fasta = os.path.join(work, "contigs_%d.fasta" % n)
            write_contigs(fasta, n)
            with open(os.path.join(work, "ab_%d.txt" % n), "w") as fh:  # equal shares: n_reads / (2 n) pairs per contig
                fh.write("".join("contig_%d\t%s\n" % (k, 1.0 / n) for k in range(n)))
            with open(os.path.join(work, "draft_ab_%d.txt" % n), "w") as fh:
                fh.write("%s\t1.0\n" % fasta)
            for pairs in [int(x) for x in a.pairs.split(",")]:
                if a.rng == "mt" and n * pairs > 2000000:
                    continue  # (the sequential walker: minutes)
                n_reads = 2 * n * pairs
                runs = [("genomes", ["--genomes", fasta, "--abundance_file", os.path.join(work, "ab_%d.txt" % n)])]
                if a.draft:
                    runs.append(("draft", ["--draft", fasta, "--abundance_file", os.path.join(work, "draft_ab_%d.txt" % n)]))
                for name, inp in runs:
                    for rep in range(a.repeat):
                        out = os.path.join(work, "out")
                        cmd = [sys.executable, "-m", "insilicoseq_amd", "generate", "--model", "novaseq", "-n", str(n_reads), "--seed",
                               "3", "--cpus", "1", "--rng", a.rng, "-o", out, "--quiet"] + inp
                        t0 = time.perf_counter()
                        subprocess.check_call(cmd, cwd=work, env=env)
                        dt = time.perf_counter() - t0
                        size = os.path.getsize(out + "_R1.fastq")
                        print(json.dumps({"root": os.path.basename(os.path.abspath(a.root)), "input": name, "contigs": n,
                                          "pairs_per_contig": pairs, "rng": a.rng, "rep": rep, "seconds": round(dt, 3),
                                          "us_per_contig": round(dt / n * 1e6, 1), "r1_bytes": size}), flush=True)
                        for f in os.listdir(work):
                            if f.startswith("out"):
                                os.remove(os.path.join(work, f))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
