#!/usr/bin/env python3
"""`--mode perfect` on one GPU: k_perfect against the ISS_PERFECT_KERNEL=0 route (k_main on DenseModel.perfect()'s tables),
then `generate --mode perfect` end to end.  Prints one JSON line.

  python tools/perfect_bench.py [--pairs 10000000] [--rounds 5] [--e2e-reads 20000000] [--out-dir /dev/shm]

Kernel leg: ONE engine, a random 5 Mbp genome, every step one iss_generate call of --pairs pairs; HIP events around the main
kernel only (timing mode 2).  The two routes alternate step by step (the switch is read at every call), after one untimed step
each; per route the median and the minimum of the steps' main-kernel time, pairs/s, and the fraction of 8 TB/s that
bench.py's algorithmic_bytes_per_pair(125) makes of it.  End-to-end leg: the CLI on the same genome as a FASTA file in
--out-dir (tmpfs), Philox, one worker, wall time of the whole command."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import algorithmic_bytes_per_pair  # noqa: E402

PEAK = 8.0e12  # bytes/s, HBM3E of the MI355X


def kernel_leg(pairs, rounds, genome):
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.model import DenseModel

    dense = DenseModel.perfect()
    times = {"k_perfect": [], "k_main": []}
    names = {}
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        eng.reserve(pairs)
        eng.timing_enable(2)
        ordinal = 0
        for r in range(rounds + 1):
            for route, switch in (("k_perfect", "1"), ("k_main", "0")):
                os.environ["ISS_PERFECT_KERNEL"] = switch
                eng.timing_read()
                eng.generate(gid, pairs, first_ordinal=ordinal, seed=42)
                t = eng.timing_read()
                names[route] = eng.main_kernel()
                ordinal += pairs
                if r:  # (round 0: untimed)
                    times[route].append(t["main_ms"])
        os.environ.pop("ISS_PERFECT_KERNEL", None)
    bpp = algorithmic_bytes_per_pair(dense.read_length)
    out = {}
    for route, ms in times.items():
        med, best = float(np.median(ms)), float(np.min(ms))
        out[route] = {"kernel": names[route], "ms_median": round(med, 4), "ms_min": round(best, 4),
                      "ms_all": [round(x, 4) for x in ms], "pairs_per_s": round(pairs / (med * 1e-3), 1),
                      "frac_of_8TBps": round(pairs * bpp / (med * 1e-3) / PEAK, 4)}
    out["speedup_median"] = round(out["k_main"]["ms_median"] / out["k_perfect"]["ms_median"], 3)
    return out


def e2e_leg(reads, genome, out_dir):
    fasta = os.path.join(out_dir, "perfect_bench.fasta")
    with open(fasta, "w") as fh:
        fh.write(">bench\n")
        for k in range(0, len(genome), 80):
            fh.write(genome[k:k + 80] + "\n")
    prefix = os.path.join(out_dir, "perfect_bench_run")
    t0 = time.perf_counter()
    subprocess.check_call([sys.executable, "-m", "insilicoseq_amd", "generate", "--mode", "perfect", "--genomes", fasta,
                           "-n", str(reads), "--seed", "42", "-o", prefix, "--quiet"], cwd=ROOT)
    wall = time.perf_counter() - t0
    size = sum(os.path.getsize(prefix + s) for s in ("_R1.fastq", "_R2.fastq"))
    for f in (fasta, prefix + "_R1.fastq", prefix + "_R2.fastq", prefix + "_abundance.txt"):
        if os.path.exists(f):
            os.remove(f)
    return {"reads": reads, "wall_s": round(wall, 3), "pairs_per_s": round(reads / 2 / wall, 1), "fastq_bytes": size}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=10_000_000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--genome-bases", type=int, default=5_000_000)
    p.add_argument("--e2e-reads", type=int, default=20_000_000)
    p.add_argument("--out-dir", default="/dev/shm")
    a = p.parse_args()
    rng = np.random.RandomState(1)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, a.genome_bases)].tobytes().decode()
    res = {"pairs_per_step": a.pairs, "read_length": 125, "bytes_per_pair": algorithmic_bytes_per_pair(125)}
    res.update(kernel_leg(a.pairs, a.rounds, genome))
    if a.e2e_reads:
        res["e2e"] = e2e_leg(a.e2e_reads, genome, a.out_dir)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
