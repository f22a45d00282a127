#!/usr/bin/env python3
"""Wall time of `model` (insilicoseq_amd.modeller.to_model) on a synthetic 2 x 151 BAM, split into inflate / boundary scan /
tally (host-to-device copy + k_bam_tally + k_bam_qhist) / KDE / write.  Prints one JSON line.

  python tools/model_bench.py --write /tmp/bench.bam --pairs 1000000   # the BAM only (no GPU)
  python tools/model_bench.py --bam /tmp/bench.bam                     # model it, timed
  python tools/model_bench.py --bam /tmp/bench.bam --compare           # the BGZF blocks inflated on the device against the host pool
                                                                       # (the default): alternating, three runs after a warm-up

The kernel times come from a separate run of the second form under `rocprofv3 --kernel-trace --stats`.
The records are built with numpy, all of one layout: 151M, MD with one reference letter at position 75 (a match, a substitution
or an N), random bases and qualities around a per-read level, paired, read1 / read2, every tenth reversed."""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RL = 151


def records(n_rec, seed):
    rng = np.random.default_rng(seed)
    md = b"75A75\0"
    l_name = 10
    head = 32 + l_name + 4 + (RL + 1) // 2 + RL
    aux = 3 + len(md)
    body = head + aux
    a = np.zeros((n_rec, 4 + body), dtype=np.uint8)

    def put(col, val, dtype):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val, dtype=np.dtype(dtype)), (n_rec,)))
        a[:, col:col + v.dtype.itemsize] = v.view(np.uint8).reshape(n_rec, v.dtype.itemsize)

    idx = np.arange(n_rec)
    put(0, body, "<i4")
    put(4, 0, "<i4")
    put(8, rng.integers(0, 4000000, n_rec), "<i4")
    a[:, 12] = l_name
    a[:, 13] = 60
    put(14, 4680, "<u2")
    put(16, 1, "<u2")
    mate = idx & 1
    rev = (mate == 1) ^ (rng.random(n_rec) < 0.1)
    put(18, 1 | 2 | np.where(mate == 0, 64, 128) | np.where(rev, 16, 32), "<u2")
    put(20, RL, "<i4")
    put(24, 0, "<i4")
    put(28, 0, "<i4")
    tlen = rng.integers(250, 700, n_rec)
    put(32, np.where(mate == 0, tlen, -tlen), "<i4")
    p = 36
    names = np.char.mod("r%08d", idx // 2).astype("S9")
    a[:, p:p + 9] = np.frombuffer(names.tobytes(), np.uint8).reshape(n_rec, 9)
    p += l_name
    put(p, RL << 4, "<u4")
    p += 4
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n_rec, RL + 1))]
    a[:, p:p + (RL + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    p += (RL + 1) // 2
    level = rng.integers(20, 38, n_rec)
    a[:, p:p + RL] = np.clip(level[:, None] + rng.integers(-5, 6, (n_rec, RL)), 2, 41)
    p += RL
    a[:, p:p + 3] = np.frombuffer(b"MDZ", np.uint8)
    a[:, p + 3:p + 3 + len(md)] = np.frombuffer(md, np.uint8)
    a[:, p + 5] = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n_rec)]
    return a


def write_bam(path, n_pairs, seed=1, threads=16):
    from bam_synth import BGZF_EOF, bgzf_block, header_bytes

    chunks = [header_bytes(ref_len=4000000)]
    step = 100000
    for i in range(0, 2 * n_pairs, step):
        chunks.append(records(min(step, 2 * n_pairs - i), seed + i).tobytes())
    data = b"".join(chunks)
    blocks = [data[i:i + 65280] for i in range(0, len(data), 65280)]
    with cf.ThreadPoolExecutor(threads) as pool, open(path, "wb") as fh:
        for b in pool.map(lambda x: bgzf_block(x, 6), blocks, chunksize=64):
            fh.write(b)
        fh.write(BGZF_EOF)
    return len(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--write", help="write the BAM here and stop")
    ap.add_argument("--bam", help="model this BAM (default: write one to a temp dir first)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--compare", action="store_true", help="time both inflate routes, alternating: a warm-up, then --reps runs each")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.write:
        t0 = time.perf_counter()
        n = write_bam(args.write, args.pairs)
        print(json.dumps(dict(written=args.write, pairs=args.pairs, inflated_bytes=n, seconds=round(time.perf_counter() - t0, 2))))
        return 0
    bam = args.bam
    if not bam:
        bam = os.path.join(tempfile.mkdtemp(prefix="model_bench_"), "bench.bam")
        write_bam(bam, args.pairs)
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd.modeller import to_model

    out = os.path.join(tempfile.mkdtemp(prefix="model_bench_out_"), "m")
    if args.compare:
        import statistics

        runs = {"device": [], "host_pool": []}
        for rep in range(args.reps + 1):
            for route in runs:
                timings = {}
                t0 = time.perf_counter()
                to_model(bam, out, device=args.device, timings=timings, device_inflate=route == "device")
                if rep:
                    runs[route].append(dict(wall_s=round(time.perf_counter() - t0, 3), **{k + "_s": round(v, 3) for k, v in sorted(timings.items())}))
        print(json.dumps(dict(bam=bam, bam_bytes=os.path.getsize(bam),
                              **{r + "_wall_s": statistics.median(x["wall_s"] for x in v) for r, v in runs.items()}, runs=runs)))
        return 0
    timings = {}
    t0 = time.perf_counter()
    to_model(bam, out, device=args.device, timings=timings)
    wall = time.perf_counter() - t0
    res = dict(bam=bam, bam_bytes=os.path.getsize(bam), wall_s=round(wall, 3), **{k + "_s": round(v, 3) for k, v in sorted(timings.items())})
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
