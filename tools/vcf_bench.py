#!/usr/bin/env python3
"""`generate --store_mutations` on one GPU, one worker, Philox mode: what the .vcf costs.  Prints one JSON line.

  python tools/vcf_bench.py --model novaseq [--route device|host|off] [--pairs 4000000] [--tree DIR] [--out-dir /dev/shm]

One worker_iterator call on a random 5 Mbp genome into --out-dir (tmpfs).  --route device: the VCF text built on the GPU
(ReadEngine.vcf_emit); host: ISS_HOST_VCF=1, rows to the host and write_mutations; off: no --store_mutations (the ceiling).
--tree: import the package from another checkout (the parent commit, built next to this one), so that both run interleaved in
one session: `for rep in 1 2 3; do for tree in . build_ab/parent; do python tools/vcf_bench.py --tree $tree ...; done; done`.
Reported: the steady state -- from the engine being ready (model uploaded) to the files being complete (worker_iterator's
`timings`) -- as pairs/s and VCF rows/s, and the start-up apart."""
import argparse
import json
import os
import sys

import numpy as np


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="novaseq")
    p.add_argument("--route", default="device", choices=("device", "host", "off"))
    p.add_argument("--pairs", type=int, default=4_000_000)
    p.add_argument("--genome-bases", type=int, default=5_000_000)
    p.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p.add_argument("--out-dir", default="/dev/shm")
    a = p.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    os.environ.pop("ISS_HOST_VCF", None)
    if a.route == "host":
        os.environ["ISS_HOST_VCF"] = "1"

    from insilicoseq_amd.generator import Record, worker_iterator
    from insilicoseq_amd.model import KDErrorModel

    rng = np.random.RandomState(1)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, a.genome_bases)].tobytes().decode()
    npz = os.path.join(tree, "insilicoseq_amd", "profiles", a.model + ".dense.npz")
    em = KDErrorModel(npz, None, None, a.route != "off")
    prefix = os.path.join(a.out_dir, "vcf_bench_%d" % os.getpid())
    timings = {}
    try:
        worker_iterator([(Record(genome, id="bench"), a.pairs, "default")], em, 0, prefix, 42, "metagenomics", False, device=0,
                        timings=timings)
        rows, vcf_bytes = 0, os.path.getsize(prefix + ".vcf")
        with open(prefix + ".vcf", "rb") as fh:
            for chunk in iter(lambda: fh.read(1 << 24), b""):
                rows += chunk.count(b"\n")
        fastq_bytes = sum(os.path.getsize(prefix + s) for s in ("_R1.fastq", "_R2.fastq"))
    finally:
        for s in ("_R1.fastq", "_R2.fastq", ".vcf"):
            if os.path.exists(prefix + s):
                os.remove(prefix + s)
    steady = timings["t_end"] - timings["t_ready"]
    print(json.dumps({"tree": os.path.relpath(tree), "model": a.model, "route": a.route, "pairs": a.pairs, "rows": rows,
                      "vcf_bytes": vcf_bytes, "fastq_bytes": fastq_bytes, "startup_s": round(timings["t_ready"] - timings["t_start"], 3),
                      "steady_s": round(steady, 4), "pairs_per_s": round(a.pairs / steady, 1), "rows_per_s": round(rows / steady, 1)}))


if __name__ == "__main__":
    main()
