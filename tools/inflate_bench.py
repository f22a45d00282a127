#!/usr/bin/env python
"""What the device inflate costs and what it buys, all in one process on one box:
  - the inflate itself, from compressed bytes in host memory to inflated bytes in host memory (scan, feeds, collects), the device
    against the host pool of 16 zlib threads (bam.inflate's) on the same bytes;
  - k_bgzf_inflate alone, from the HIP events around every launch (iss_inflate_kernel_ms);
  - `model` (modeller.to_model) end to end, device route (device_inflate=True) against host route, on model_bench's BAM;
  - `report` end to end on report_bench's two files written as BGZF, device route against gzip.open.

    python tools/inflate_bench.py                                  # 1 M pairs for model, 4 M reads for report
    python tools/inflate_bench.py --pairs 200000 --reads 1000000 --keep bench_inflate

Three runs after a warm-up each, alternating the routes; one JSON line per figure with the median and all three."""
import argparse
import collections
import concurrent.futures as cf
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from insilicoseq_amd import _native, app, bgzf  # noqa: E402
from insilicoseq_amd import inflate as Z  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return round(statistics.median(xs), 4)


def device_inflate(inf, raw, group_bytes):
    """raw (bytes of a whole BGZF file) -> inflated byte count; two groups in flight."""
    inf.reset()
    queue, at, total = collections.deque(), 0, 0
    view = memoryview(raw)
    while at < len(raw):
        members, used = Z.scan(view[at:at + group_bytes])
        assert used, "a member larger than a group"
        inf.feed(view[at:at + used], members)
        queue.append(members)
        at += used
        if len(queue) >= 2:
            data, status = inf.collect(copy=False)
            assert not status.any()
            queue.popleft()
            total += data.size
    while queue:
        data, status = inf.collect(copy=False)
        assert not status.any()
        queue.popleft()
        total += data.size
    return total


def host_inflate(raw, threads=16):
    """The same bytes through the host route's pool: zlib on 16 threads, groups of members."""
    members, used = Z.scan(raw)
    assert used == len(raw)

    def group(lo, hi):
        n = 0
        for k in range(lo, hi):
            data = zlib.decompress(raw[members.pay_off[k]:members.pay_off[k] + members.pay_len[k]], -15)
            assert zlib.crc32(data) & 0xFFFFFFFF == members.crc[k]
            n += len(data)
        return n

    step = 64
    with cf.ThreadPoolExecutor(threads) as pool:
        return sum(pool.map(lambda lo: group(lo, min(lo + step, members.offset.size)), range(0, members.offset.size, step)))


def bench_inflate(label, path, reps, group_bytes):
    raw = open(path, "rb").read()
    dev_s, ker_ms, host_s = [], [], []
    with Z.BgzfInflater(0) as inf:
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            n = device_inflate(inf, raw, group_bytes)
            t1 = time.perf_counter()
            k = inf.kernel_ms()
            t2 = time.perf_counter()
            assert host_inflate(raw) == n
            t3 = time.perf_counter()
            if rep:
                dev_s.append(t1 - t0)
                ker_ms.append(k)
                host_s.append(t3 - t2)
    gb = n / 1e9
    out(what="inflate, host memory to host memory", file=label, compressed_bytes=len(raw), inflated_bytes=n, group_bytes=group_bytes,
        device_s=med(dev_s), device_s_all=[round(t, 4) for t in dev_s], device_gb_per_s=round(gb / statistics.median(dev_s), 3),
        host_pool_s=med(host_s), host_pool_s_all=[round(t, 4) for t in host_s], host_pool_gb_per_s=round(gb / statistics.median(host_s), 3))
    out(what="k_bgzf_inflate alone (HIP events)", file=label, ms=med(ker_ms), ms_all=[round(t, 3) for t in ker_ms],
        gb_per_s=round(gb / (statistics.median(ker_ms) / 1e3), 3))


def alternate(reps, routes):
    """routes: {name: callable}; every callable runs reps + 1 times, the routes alternating, the first round dropped."""
    secs = {name: [] for name in routes}
    for rep in range(reps + 1):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                secs[name].append(time.perf_counter() - t0)
    return secs


def with_host_inflate(fn):
    def run():
        os.environ["ISS_HOST_INFLATE"] = "1"
        try:
            fn()
        finally:
            del os.environ["ISS_HOST_INFLATE"]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000, help="pairs of model_bench's BAM")
    ap.add_argument("--reads", type=int, default=4000000, help="reads of report_bench's two files")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--group-bytes", type=int, default=32 << 20)
    ap.add_argument("--keep", default=None, help="directory for the files (default: a temporary one, removed)")
    ap.add_argument("--skip-report", action="store_true")
    a = ap.parse_args()
    import model_bench
    import report_bench

    from insilicoseq_amd.modeller import to_model

    work = a.keep or tempfile.mkdtemp(prefix="inflate_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), inflate_wgs=os.environ.get("ISS_INFLATE_WGS", "default"))
        bam = os.path.join(work, "bench.bam")
        if not os.path.exists(bam):
            model_bench.write_bam(bam, a.pairs)
        bench_inflate("bam", bam, a.reps, a.group_bytes)
        prefix = os.path.join(work, "m")
        secs = alternate(a.reps, {"device": lambda: to_model(bam, prefix, device_inflate=True), "host": with_host_inflate(lambda: to_model(bam, prefix))})
        out(what="model end to end", bam_bytes=os.path.getsize(bam), pairs=a.pairs, device_s=med(secs["device"]), host_pool_s=med(secs["host"]),
            device_s_all=[round(t, 4) for t in secs["device"]], host_pool_s_all=[round(t, 4) for t in secs["host"]])
        if a.skip_report:
            return
        r1, r2 = os.path.join(work, "run_R1.fastq"), os.path.join(work, "run_R2.fastq")
        if not (os.path.exists(r1 + ".gz") and os.path.exists(r2 + ".gz")):
            report_bench.write_pair(os.path.join(work, "run"), a.reads)
            for path in (r1, r2):
                bgzf.compress_file(path)
        for path in (r1 + ".gz", r2 + ".gz"):
            assert Z.is_bgzf(path)
        bench_inflate("R1.fastq.gz", r1 + ".gz", a.reps, a.group_bytes)
        rep = os.path.join(work, "rep")
        run = lambda: app.main(["report", "--quiet", "-1", r1 + ".gz", "-2", r2 + ".gz", "-o", rep])  # noqa: E731
        secs = alternate(a.reps, {"device": run, "host": with_host_inflate(run)})
        out(what="report end to end", compressed_bytes=os.path.getsize(r1 + ".gz") + os.path.getsize(r2 + ".gz"), reads=a.reads,
            device_s=med(secs["device"]), gzip_open_s=med(secs["host"]), device_s_all=[round(t, 4) for t in secs["device"]],
            gzip_open_s_all=[round(t, 4) for t in secs["host"]])
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
