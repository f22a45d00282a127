"""`generate --variants`: what splicing one record costs, once per record -- VariantTable.apply_host (numpy, one thread) against
ReadEngine.add_genome_variants (copies to the device, REF check, splice, pack, status read-back) on a synthetic record.
One JSON line per measurement; the two haplotypes are compared byte for byte.  DESIGN.md section 30 quotes a run.

    python tools/variants_bench.py [--bases 100000000] [--variants 1000000] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic(bases, n, seed=1):
    """A record of ``bases`` letters and about ``n`` variants: 80 % SNVs, 10 % insertions and 10 % deletions of 1 .. 10 letters."""
    from insilicoseq_amd.variants import VariantTable

    rng = np.random.RandomState(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, bases)]
    step = max(bases // max(n, 1), 24)
    pos0 = np.cumsum(rng.randint(step // 2, step + step // 2 + 1, n).astype(np.int64))
    pos0 = pos0[pos0 < bases - 16]
    n = pos0.size
    kind = rng.random_sample(n)
    size = rng.randint(1, 11, n).astype(np.int32)
    ref_len = np.where(kind < 0.8, 1, np.where(kind < 0.9, 0, size)).astype(np.int32)
    alt_len = np.where(kind < 0.8, 1, np.where(kind < 0.9, size, 0)).astype(np.int32)
    ref_off = np.concatenate(([0], np.cumsum(ref_len[:-1], dtype=np.int64)))
    idx = np.repeat(pos0 - ref_off, ref_len) + np.arange(int(ref_len.sum()), dtype=np.int64)  # pos0[i] + k for every REF letter
    ref = seq[idx]
    alt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, int(alt_len.sum()))]
    return seq, VariantTable(pos0, ref_len, alt_len, alt, ref, bases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--variants", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine

    def out(**kw):
        print(json.dumps(kw), flush=True)

    seq, table = synthetic(a.bases, a.variants)
    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), bases=int(seq.size), variants=len(table),
        haplotype_bases=int(table.out_pos[-1]), counts=table.counts())
    t0 = time.perf_counter()
    want = table.apply_host(seq)
    out(what="apply_host (numpy, one thread)", seconds=round(time.perf_counter() - t0, 3))
    t0 = time.perf_counter()
    native = table.apply_native(seq)
    out(what="iss_variants_host_apply (one thread)", seconds=round(time.perf_counter() - t0, 3), equal=bool(np.array_equal(native, want)))
    with ReadEngine(a.device) as eng:
        for k in range(a.repeat):
            eng.clear_genomes()
            eng.synchronize()
            t0 = time.perf_counter()
            gid = eng.add_genome_variants(seq, table)
            dt = time.perf_counter() - t0
            out(what="add_genome_variants (copies, check, splice, pack, read-back)", run=k, seconds=round(dt, 3))
        t0 = time.perf_counter()
        plain = eng.add_genome(want)
        out(what="add_genome of the finished haplotype (copy, pack, read-back)", seconds=round(time.perf_counter() - t0, 3))
        got = eng.genome_letters(gid)
        out(what="device haplotype against apply_host", equal=bool(np.array_equal(got, want)), plain_genome=plain)
        return 0 if np.array_equal(got, want) else 1


if __name__ == "__main__":
    sys.exit(main())
