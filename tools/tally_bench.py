#!/usr/bin/env python
"""What the tally costs: iss_output_tally next to iss_output_export (bases + qual, all four outputs) of
the same rows -- NovaSeq 2 x 151, 5 M pairs, HIP events, the two alternating run by run in one process -- and
ReadTensorStream in pairs/s with tally=True next to tally=False.

    python tools/tally_bench.py                  # everything, one JSON line per figure
    ISS_TALLY_WGS=4096 python tools/tally_bench.py --kernels-only    # another launch geometry

Times are medians of --reps runs after a warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # before the engine's library (insilicoseq_amd/tensors.py: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from insilicoseq_amd import tensors as T  # noqa: E402
from insilicoseq_amd.engine import ReadEngine  # noqa: E402
from insilicoseq_amd.model import DenseModel  # noqa: E402


def records(n=8, length=500000):
    rng = np.random.RandomState(5)
    return [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, length)].tobytes() for _ in range(n)]


def out(**kw):
    print(json.dumps(kw), flush=True)


def kernels(dense, recs, n, reps):
    stream = torch.cuda.Stream()
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(recs[0])
        eng.generate(gid, n, seed=1)
        eng.set_stream(stream.cuda_stream)
        row = T.row_bytes(eng.pitch)
        with torch.cuda.stream(stream):
            batch = T._empty_batch(eng, n)
            words = torch.zeros(eng.tally_words(), dtype=torch.int64, device="cuda")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = {"tally": [], "export": []}
            for r in range(reps + 2):
                for what in ("tally", "export"):
                    ev[0].record(stream)
                    if what == "tally":
                        eng.tally(0, n, words.data_ptr())
                    else:
                        eng.export(0, n, batch.bases.data_ptr(), batch.qual.data_ptr(), batch.coords.data_ptr(), batch.record.data_ptr(), "codes")
                    ev[1].record(stream)
                    ev[1].synchronize()
                    if r >= 2:
                        ms[what].append(ev[0].elapsed_time(ev[1]))
            assert int(words[0].item()) == n * (reps + 2)
        eng.set_stream(None)
    for what in ("tally", "export"):
        t = statistics.median(ms[what])
        out(what="iss_output_tally" if what == "tally" else "iss_output_export", pairs=n, ms=round(t, 4), ms_all=[round(x, 4) for x in ms[what]],
            row_bytes=row, rows_tb_per_s=round(n * row / t / 1e9, 3), tally_wgs=os.environ.get("ISS_TALLY_WGS", "default"))


def run_stream(dense, recs, work, batch_pairs, **kw):
    with T.ReadTensorStream(recs, dense, work, batch_pairs, seed=3, **kw) as s:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in s:
            pass
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5000000)
    ap.add_argument("--total", type=int, default=20000000, help="pairs of a stream run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-pairs", type=int, default=1 << 20)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    dense = DenseModel.load(os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz"))
    recs = records()
    from insilicoseq_amd import _native

    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), device=torch.cuda.get_device_name(0))
    kernels(dense, recs, a.pairs, a.reps)
    if a.kernels_only:
        return
    work = T.multinomial_work([1.0 / (k + 1) for k in range(len(recs))], a.total, seed=9)
    legs = {"tally=False": {}, "tally=True": {"tally": True}}
    secs = {k: [] for k in legs}
    for rep in range(a.reps + 1):
        for k, kw in legs.items():
            t = run_stream(dense, recs, work, a.batch_pairs, **kw)
            if rep:
                secs[k].append(t)
    for k in legs:
        t = statistics.median(secs[k])
        out(what="ReadTensorStream " + k, batch_pairs=a.batch_pairs, pairs=a.total, s=round(t, 5), pairs_per_s=round(a.total / t, 1),
            s_all=[round(x, 5) for x in secs[k]])


if __name__ == "__main__":
    main()
