#!/usr/bin/env python
"""What `report --bam --errors` adds: one synthetic 2 x 151 BAM of tests/bam_synth.py's records at their
default parameters (clips, indels, mismatches, N, unmapped / secondary / supplementary records, extra tags), scaled up, and on it
  - the kernels alone, from the HIP events around every feed's launches (iss_br_kernel_ms): the inflated chunks held in memory
    and fed to a context with the error stage and to one without, alternating, --reps runs each after a warm-up;
  - with --parent-lib: the same without-errors figure from another build of the library (the commit before the stage existed),
    in a process of its own in front of and behind the runs above -- the baseline that is not the code under test;
  - end to end: `report --bam` with and without --errors in this process, alternating.

    python tools/bam_errors_bench.py                          # 1 M pairs (2 M records), one JSON line per figure
    python tools/bam_errors_bench.py --write bench.bam        # the file only (no GPU)
    python tools/bam_errors_bench.py --bam bench.bam --parent-lib build_ab/libiss_parent.so
    rocprofv3 --kernel-trace --stats -d prof -- python tools/bam_errors_bench.py --bam bench.bam --kernels-only   # time per kernel

The records are made in a pool of processes, a seed each; the same arguments give the same file."""
import argparse
import concurrent.futures as cf
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLICE_PAIRS = 20000


def out(**kw):
    print(json.dumps(kw), flush=True)


def _slice(args):
    import bam_synth

    seed, n_pairs = args
    return b"".join(bam_synth.encode_record(r) for r in bam_synth.records(seed, n_pairs=n_pairs))


def _block(payload):
    import bam_synth

    return bam_synth.bgzf_block(payload, 1)


def write_bam(path, n_pairs, seed=1, procs=16):
    """bam_synth.records(seed + k, n_pairs=SLICE_PAIRS) for as many k as it takes; returns (inflated bytes, records)."""
    import bam_synth

    jobs = [(seed + k, min(SLICE_PAIRS, n_pairs - k * SLICE_PAIRS)) for k in range((n_pairs + SLICE_PAIRS - 1) // SLICE_PAIRS)]
    n_bytes = 0
    with cf.ProcessPoolExecutor(procs) as pool, cf.ThreadPoolExecutor(procs) as threads, open(path, "wb") as fh:
        data = bam_synth.header_bytes()
        for part in pool.map(_slice, jobs):
            data += part
            cut = len(data) - len(data) % 65280
            for b in threads.map(_block, [data[i:i + 65280] for i in range(0, cut, 65280)]):
                fh.write(b)
            n_bytes += cut
            data = data[cut:]
        if data:
            fh.write(_block(data))
            n_bytes += len(data)
        fh.write(bam_synth.BGZF_EOF)
    return n_bytes, 2 * n_pairs


def _chunks(bam):
    from insilicoseq_amd.bam import BamReader, Chunk

    return [Chunk(c.data.copy(), c.offsets.copy()) for c in BamReader(bam).chunks()]


def kernels(bam, reps, plain_only, label):
    """iss_br_kernel_ms of the file's feeds, with and without the error stage, alternating."""
    from insilicoseq_amd import _native
    from insilicoseq_amd import bam_report as B

    chunks = _chunks(bam)
    n_records = sum(len(c.offsets) for c in chunks)
    n_bytes = sum(c.data.size for c in chunks)
    kinds = ["plain"] if plain_only else ["plain", "errors"]
    devs = {k: B.BamReadTally(0, **({"errors": True} if k == "errors" else {})) for k in kinds}
    ms = {k: [] for k in kinds}
    for rep in range(reps + 1):
        for k in kinds:
            devs[k].reset()
            for c in chunks:
                devs[k].feed(c)
            t = devs[k].kernel_ms()
            if rep:
                ms[k].append(t)
    res = {k: devs[k].download() for k in kinds}
    for d in devs.values():
        d.close()
    line = dict(what="kernels alone (HIP events)", build=label, library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(),
                records=n_records, inflated_bytes=n_bytes, feeds=len(chunks), taken=res["plain"]["records"])
    for k in kinds:
        line[k + "_ms_all"] = [round(t, 3) for t in ms[k]]
        line[k + "_ms_median"] = round(statistics.median(ms[k]), 3)
        line[k + "_ms_spread"] = round(max(ms[k]) - min(ms[k]), 3)
    if not plain_only:
        import numpy as np

        assert np.array_equal(res["plain"]["tally"], res["errors"]["tally"]) and res["plain"]["records"] == res["errors"]["records"]
        line["ratio_errors_over_plain"] = round(line["errors_ms_median"] / line["plain_ms_median"], 3)
        line["error_counts"] = res["errors"]["error_counts"]
        line["dropped"] = int(res["errors"]["errors"][0])
        line["bad_alignment"] = [res["errors"]["bad_alignment"], res["errors"]["bad_alignment_code"]]
    out(**line)


def end_to_end(bam, reps, work):
    from insilicoseq_amd import app

    secs = {"plain": [], "errors": []}
    for rep in range(reps + 1):
        for k in secs:
            t0 = time.perf_counter()
            assert app.main(["report", "--quiet", "--bam", bam, "-o", os.path.join(work, "e2e_" + k)] + (["--errors"] if k == "errors" else [])) == 0
            if rep:
                secs[k].append(time.perf_counter() - t0)
    out(what="report --bam end to end (host inflate pool)", plain_s_all=[round(t, 3) for t in secs["plain"]],
        errors_s_all=[round(t, 3) for t in secs["errors"]], plain_s_median=round(statistics.median(secs["plain"]), 3),
        errors_s_median=round(statistics.median(secs["errors"]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=16, help="processes that make the records")
    ap.add_argument("--write", default=None, help="write the BAM here and stop")
    ap.add_argument("--bam", default=None, help="measure this BAM (default: write one to a temporary directory first)")
    ap.add_argument("--parent-lib", default=None, help="another build of the library: its without-errors kernel time, before and after")
    ap.add_argument("--kernels-only", action="store_true",
                    help="with --bam: the kernel runs of this build alone (under `rocprofv3 --kernel-trace --stats` for the time per kernel)")
    ap.add_argument("--plain-only", default=None, metavar="LABEL", help="(the child process of --parent-lib) the without-errors runs alone")
    a = ap.parse_args()
    for name in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE"):
        os.environ.pop(name, None)
    if a.write:
        t0 = time.perf_counter()
        n_bytes, n_records = write_bam(a.write, a.pairs, procs=a.procs)
        out(written=a.write, records=n_records, inflated_bytes=n_bytes, seconds=round(time.perf_counter() - t0, 1))
        return 0
    if a.plain_only or a.kernels_only:
        kernels(a.bam, a.reps, bool(a.plain_only), a.plain_only or "this build")
        return 0
    work = tempfile.mkdtemp(prefix="bam_errors_bench_")
    try:
        bam = a.bam
        if not bam:
            bam = os.path.join(work, "bench.bam")
            t0 = time.perf_counter()
            n_bytes, n_records = write_bam(bam, a.pairs, procs=a.procs)
            out(written=bam, records=n_records, inflated_bytes=n_bytes, file_bytes=os.path.getsize(bam), seconds=round(time.perf_counter() - t0, 1))

        def parent(label):
            if a.parent_lib:  # (a process of its own: a process holds one build of the library)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--bam", bam, "--reps", str(a.reps), "--plain-only", label],
                               env=dict(os.environ, ISS_MI355X_LIB=os.path.abspath(a.parent_lib)), check=True, timeout=600)

        parent("parent, before")
        kernels(bam, a.reps, False, "this build")
        parent("parent, after")
        end_to_end(bam, a.e2e_reps, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
