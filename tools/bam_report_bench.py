#!/usr/bin/env python
"""What `report --bam` costs: a synthetic 2 x 151 BAM of tools/model_bench.py's recipe, tallied
  - end to end: `report --bam` in this process on both inflate routes, alternating (the file read and inflated, the records cut,
    the copies, the kernels, the download, the outputs written), in GB of inflated BAM bytes per second;
  - the feeds alone: the inflated chunks held in memory, fed and waited for (copies and kernels, no file, no inflate);
  - the kernels alone, from the HIP events around every feed's launches (iss_br_kernel_ms);
  - by the host twin (bam_report.bam_reads_host) on a prefix of the records, scaled to the file -- the only baseline there is.

    python tools/bam_report_bench.py                    # 1 M pairs, one JSON line per figure
    python tools/bam_report_bench.py --pairs 4000000 --keep bench_bam

Times are given run by run, after one warm-up run each."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import model_bench  # noqa: E402
from insilicoseq_amd import _native, app  # noqa: E402
from insilicoseq_amd import bam_report as B  # noqa: E402
from insilicoseq_amd.bam import BamReader, Chunk  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--twin-records", type=int, default=100000, help="records of the file's start the host twin tallies")
    ap.add_argument("--keep", default=None, help="directory for the files (default: a temporary one, removed)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="bam_report_bench_")
    os.makedirs(work, exist_ok=True)
    for name in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE"):
        os.environ.pop(name, None)
    try:
        bam = os.path.join(work, "bench.bam")
        n_bytes = model_bench.write_bam(bam, a.pairs)
        gb = n_bytes / 1e9
        out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), pairs=a.pairs, bam_bytes=os.path.getsize(bam),
            inflated_bytes=n_bytes, br_wgs=os.environ.get("ISS_BR_WGS", "default"))
        prefix = os.path.join(work, "rep")
        secs = {"host_pool": [], "device": []}
        words = {}
        for rep in range(a.reps + 1):
            for route in secs:
                t0 = time.perf_counter()
                assert app.main(["report", "--quiet", "--bam", bam, "-o", prefix + "_" + route] +
                                (["--device_inflate"] if route == "device" else [])) == 0
                if rep:
                    secs[route].append(time.perf_counter() - t0)
                words[route] = np.load(prefix + "_" + route + "_tally.npy")
        assert np.array_equal(words["host_pool"], words["device"])
        for route, s in secs.items():
            out(what="report --bam end to end, inflate: " + route, s_all=[round(t, 4) for t in s],
                gb_per_s_all=[round(gb / t, 3) for t in s], gb_per_s=round(gb / statistics.median(s), 3))
        chunks = [Chunk(c.data.copy(), c.offsets.copy()) for c in BamReader(bam).chunks()]
        n_records = sum(len(c.offsets) for c in chunks)
        ms, feed_s = [], []
        with B.BamReadTally(0) as dev:
            for rep in range(a.reps + 1):
                dev.reset()
                t0 = time.perf_counter()
                for c in chunks:
                    dev.feed(c)
                k = dev.kernel_ms()
                if rep:
                    ms.append(k)
                    feed_s.append(time.perf_counter() - t0)
            got = dev.result()
        assert np.array_equal(got["tally"], words["host_pool"]) and sum(got["records"]) == n_records == 2 * a.pairs
        out(what="feeds alone (copies and kernels; no file, no inflate)", records=n_records, s_all=[round(t, 4) for t in feed_s],
            gb_per_s=round(gb / statistics.median(feed_s), 3))
        out(what="kernels alone (HIP events)", ms_all=[round(t, 3) for t in ms], gb_per_s_all=[round(gb / (t / 1e3), 2) for t in ms],
            gb_per_s=round(gb / (statistics.median(ms) / 1e3), 2), records_per_s=round(n_records / (statistics.median(ms) / 1e3)))
        first = chunks[0]
        n = min(a.twin_records, len(first.offsets))
        end = int(first.offsets[n]) if n < len(first.offsets) else first.data.size
        piece = Chunk(first.data[:end], first.offsets[:n])
        host = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            B.bam_reads_host(piece)
            if rep:
                host.append(time.perf_counter() - t0)
        rate = [end / 1e9 / t for t in host]
        out(what="host twin (numpy), a prefix of the file", records=n, bytes=end, s_all=[round(t, 4) for t in host],
            gb_per_s_all=[round(x, 4) for x in rate], gb_per_s=round(statistics.median(rate), 4),
            scaled_to_the_file_s=round(gb / statistics.median(rate), 2))
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
