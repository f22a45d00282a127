#!/usr/bin/env python
"""What `generate --ubam` costs: one Philox worker end to end (worker_iterator: generation, the output's
kernels, the copy, the writer thread, the files) writing unaligned BAM, gzip members (`--compress`) and plain FASTQ text,
NovaSeq 2 x 151.

    python tools/ubam_bench.py                       # one JSON line per route, then the .bam's size against zlib level 1
    python tools/ubam_bench.py --pairs 20000000 --dir /dev/shm

The three routes alternate run by run in one process; times are medians of --reps runs after a warm-up.  The ratio reported for
the .bam is its size against zlib level 1 applied to the same 32 768-byte blocks of the same record bytes (raw deflate + the 26
bytes of a BGZF member's frame)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from insilicoseq_amd.generator import Record, worker_iterator  # noqa: E402
from insilicoseq_amd.model import KDErrorModel  # noqa: E402

ROUTES = {"ubam": {"ubam": True}, "compress": {"compress": True}, "plain": {}}
FILES = {"ubam": (".bam",), "compress": ("_R1.fastq", "_R2.fastq"), "plain": ("_R1.fastq", "_R2.fastq")}


def out(**kw):
    print(json.dumps(kw), flush=True)


def records(n=8, length=500000):
    rng = np.random.RandomState(5)
    return [Record(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, length)].tobytes().decode(), id="NZ_BENCH%04d.1" % k) for k in range(n)]


def run(route, model, work, prefix):
    timings = {}
    worker_iterator(work, model, 0, prefix, 3, "metagenomics", False, device=0, rng="philox", timings=timings, **ROUTES[route])
    size = sum(os.path.getsize(prefix + s) for s in FILES[route])
    return timings["t_end"] - timings["t_ready"], size


def zlib_level_1(path, block=32768):
    """(bytes of the file's members, bytes of zlib level 1 over the same blocks of the inflated bytes)"""
    from insilicoseq_amd import bam

    mine = os.path.getsize(path)
    ref = 0
    pending = b""
    with open(path, "rb") as fh:
        for group in bam._block_groups(fh, 16 << 20, 4 << 20):
            pending += bam._inflate_group(group)
            while len(pending) >= block:
                c = zlib.compressobj(1, zlib.DEFLATED, -15)
                ref += len(c.compress(pending[:block]) + c.flush()) + 26
                pending = pending[block:]
    if pending:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += len(c.compress(pending) + c.flush()) + 26
    return mine, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    a = ap.parse_args()
    from insilicoseq_amd import _native

    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode())
    model = KDErrorModel(os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz"), None, None, False)
    recs = records()
    per = a.pairs // len(recs)
    work = [(r, per, "default") for r in recs]
    total = per * len(recs)
    tmp = tempfile.mkdtemp(prefix="ubam_bench.", dir=a.dir)
    try:
        secs, sizes = {r: [] for r in ROUTES}, {}
        for rep in range(a.reps + 1):
            for route in ROUTES:
                t, sizes[route] = run(route, model, work, os.path.join(tmp, route))
                if rep:
                    secs[route].append(t)
        for route in ROUTES:
            t = statistics.median(secs[route])
            out(what="worker_iterator " + route, pairs=total, s=round(t, 4), pairs_per_s=round(total / t, 1), s_all=[round(x, 4) for x in secs[route]],
                bytes=sizes[route], bytes_per_pair=round(sizes[route] / total, 2))
        mine, ref = zlib_level_1(os.path.join(tmp, "ubam") + ".bam")
        out(what=".bam against zlib level 1 over the same blocks", bam_bytes=mine, zlib1_bytes=ref, ratio=round(mine / ref, 4))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
