#!/usr/bin/env python
"""What `report` costs: a FASTQ pair written by `generate` (NovaSeq 2 x 151), tallied
  - end to end: `report` in this process (the files read and cut into chunks, the copies, the kernels, the download, the outputs
    written), in GB of FASTQ text per second;
  - the kernels alone, from the HIP events around every feed's launches (iss_fq_kernel_ms);
  - by the host twin (fastq_report.fastq_tally_host) on a slice of R1, scaled to both files -- the only baseline there is.

    python tools/report_bench.py                       # 4 M reads, one JSON line per figure
    python tools/report_bench.py --reads 20000000 --keep bench_reads

Times are given run by run, after one warm-up run each."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from insilicoseq_amd import _native, app  # noqa: E402
from insilicoseq_amd import fastq_report as F  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def write_pair(prefix, reads):
    fasta = prefix + ".fasta"
    rng = np.random.RandomState(5)
    with open(fasta, "w") as fh:
        for k in range(4):
            fh.write(">rec%d\n%s\n" % (k, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, 500000)].tobytes().decode()))
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", str(reads),
                    "--seed", "1", "--report", "--output", prefix], cwd=ROOT, check=True)
    return prefix + "_R1.fastq", prefix + "_R2.fastq"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice-bytes", type=int, default=32 << 20, help="bytes of R1 the host twin tallies")
    ap.add_argument("--keep", default=None, help="directory for the files (default: a temporary one, removed)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="report_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        r1, r2 = write_pair(os.path.join(work, "run"), a.reads)
        n_bytes = os.path.getsize(r1) + os.path.getsize(r2)
        gb = n_bytes / 1e9
        out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), reads=a.reads, fastq_bytes=n_bytes,
            fqtally_wgs=os.environ.get("ISS_FQTALLY_WGS", "default"))
        prefix = os.path.join(work, "rep")
        secs = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            assert app.main(["report", "--quiet", "-1", r1, "-2", r2, "-o", prefix, "--against", os.path.join(work, "run_tally.npy")]) == 0
            if rep:
                secs.append(time.perf_counter() - t0)
        summary = json.load(open(prefix + "_compare.json"))["summary"]
        assert summary["max_base_l1"] == 0.0 and summary["max_abs_mean_phred_diff"] == 0.0, summary  # (the run's own tally)
        out(what="report end to end", s_all=[round(t, 4) for t in secs], gb_per_s_all=[round(gb / t, 3) for t in secs],
            gb_per_s=round(gb / statistics.median(secs), 3))
        ms, feed_s = [], []
        with F.FastqTally(0) as dev:
            for rep in range(a.reps + 1):
                dev.reset()
                t0 = time.perf_counter()
                dev.feed_file(r1, 0)
                dev.feed_file(r2, 1)
                k = dev.kernel_ms()
                if rep:
                    ms.append(k)
                    feed_s.append(time.perf_counter() - t0)
        out(what="kernels alone (HIP events)", ms_all=[round(t, 3) for t in ms], gb_per_s_all=[round(gb / (t / 1e3), 2) for t in ms],
            gb_per_s=round(gb / (statistics.median(ms) / 1e3), 2))
        out(what="feeds (read, cut, copy, kernels; no outputs)", s_all=[round(t, 4) for t in feed_s],
            gb_per_s=round(gb / statistics.median(feed_s), 3))
        with open(r1, "rb") as fh:
            piece = next(F.split_chunks(fh, a.slice_bytes))
        host = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            F.fastq_tally_host(piece, None)
            if rep:
                host.append(time.perf_counter() - t0)
        rate = [len(piece) / 1e9 / t for t in host]
        out(what="host twin (numpy), a slice of R1", slice_bytes=len(piece), s_all=[round(t, 4) for t in host],
            gb_per_s_all=[round(x, 4) for x in rate], gb_per_s=round(statistics.median(rate), 4),
            scaled_to_both_files_s=round(gb / statistics.median(rate), 2))
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
