#!/usr/bin/env python
"""What the tensor route costs: k_rows_export by itself next to a device-to-device copy of the same
traffic, and ReadTensorStream next to the same work as bare generate_batch() calls without the export.

    python tools/tensor_bench.py                          # everything, one JSON line per figure
    ISS_MI355X_LIB=<older build> python tools/tensor_bench.py --bare-only    # the bare calls on another build of the library
    python tools/tensor_bench.py --truth                  # only: ReadTensorStream with truth=True next to truth=False (section 17)

Times are medians of --reps runs after a warm-up; the two routes of a comparison alternate run by run in one process."""
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


def export_alone(dense, recs, n, reps):
    stream = torch.cuda.Stream()
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(recs[0])
        eng.generate(gid, n, seed=1)
        eng.set_stream(stream.cuda_stream)
        RL, row = eng.read_length, T.row_bytes(eng.pitch)
        read_b, write_b = n * (row + 16), n * (4 * RL + 32 + 4)
        with torch.cuda.stream(stream):
            batch = T._empty_batch(eng, n)
            half = (read_b + write_b) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            src.zero_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = {"export": [], "copy": []}
            for r in range(reps + 2):
                for what in ("export", "copy"):
                    ev[0].record(stream)
                    if what == "export":
                        eng.export(0, n, batch.bases.data_ptr(), batch.qual.data_ptr(), batch.coords.data_ptr(), batch.record.data_ptr(), "codes")
                    else:
                        dst.copy_(src, non_blocking=True)  # (same device, same dtype, contiguous: one hipMemcpyAsync)
                    ev[1].record(stream)
                    ev[1].synchronize()
                    if r >= 2:
                        ms[what].append(ev[0].elapsed_time(ev[1]))
        eng.set_stream(None)
    for what in ("export", "copy"):
        t = statistics.median(ms[what])
        out(what="k_rows_export" if what == "export" else "hipMemcpyAsync D2D", pairs=n, ms=round(t, 4), ms_all=[round(x, 4) for x in ms[what]],
            bytes_read=read_b if what == "export" else half, bytes_written=write_b if what == "export" else half,
            tb_per_s=round((read_b + write_b if what == "export" else 2 * half) / t / 1e9, 3))


def run_stream(dense, recs, work, batch_pairs, **kw):
    with T.ReadTensorStream(recs, dense, work, batch_pairs, seed=3, **kw) as s:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in s:
            pass
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def run_bare(dense, recs, work, batch_pairs):
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gids = np.array(eng.add_genomes(recs), dtype=np.int32)[[k for k, _ in work]]
        batches = T.cut_batches([n for _, n in work], batch_pairs)
        eng.reserve(batch_pairs)
        eng.synchronize()
        t0 = time.perf_counter()
        for first_ordinal, first_item, counts in batches:
            eng.generate_batch(gids[first_item:first_item + len(counts)], counts, first_ordinal=first_ordinal, seed=3)
        eng.synchronize()
        return time.perf_counter() - t0


def truth_leg(dense, recs, work, total, batch_pairs, reps, events_capacity):
    """DESIGN.md section 17, "Measured: not yet": the stream with and without truth, alternating run by run in one process."""
    legs = {"truth=False": {}, "truth=True": {"truth": True}}
    if events_capacity:
        legs["truth=True, events"] = {"truth": True, "events_capacity": events_capacity}
    secs = {k: [] for k in legs}
    for rep in range(reps + 1):
        for k, kw in legs.items():
            t = run_stream(dense, recs, work, batch_pairs, **kw)
            if rep:
                secs[k].append(t)
    for k in legs:
        t = statistics.median(secs[k])
        out(what="ReadTensorStream " + k, batch_pairs=batch_pairs, pairs=total, s=round(t, 5), pairs_per_s=round(total / t, 1),
            s_all=[round(x, 5) for x in secs[k]],
            mutation_slots=T.default_mutation_slots(dense, batch_pairs, torch.cuda.get_device_properties(0).multi_processor_count) if legs[k] else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5000000)
    ap.add_argument("--total", type=int, default=20000000, help="pairs of a stream run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bare-only", action="store_true")
    ap.add_argument("--truth", action="store_true", help="only the truth=True / truth=False comparison of the stream")
    ap.add_argument("--batch-pairs", type=int, default=1 << 20, help="--truth: pairs of a batch")
    ap.add_argument("--events-capacity", type=int, default=0, help="--truth: a third leg with this many event rows per batch")
    a = ap.parse_args()
    dense = DenseModel.load(os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz"))
    recs = records()
    from insilicoseq_amd import _native

    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), device=torch.cuda.get_device_name(0))
    if not a.bare_only and not a.truth:
        export_alone(dense, recs, a.pairs, a.reps)
    work = T.multinomial_work([1.0 / (k + 1) for k in range(len(recs))], a.total, seed=9)
    if a.truth:
        truth_leg(dense, recs, work, a.total, a.batch_pairs, a.reps, a.events_capacity)
        return
    for batch_pairs in (1 << 16, 1 << 20, 5000000):
        routes = ("bare",) if a.bare_only else ("stream", "bare")
        secs = {r: [] for r in routes}
        for rep in range(a.reps + 1):
            for r in routes:
                t = (run_stream if r == "stream" else run_bare)(dense, recs, work, batch_pairs)
                if rep:
                    secs[r].append(t)
        for r in routes:
            t = statistics.median(secs[r])
            out(what="ReadTensorStream" if r == "stream" else "bare generate_batch", batch_pairs=batch_pairs, pairs=a.total, s=round(t, 5),
                pairs_per_s=round(a.total / t, 1), s_all=[round(x, 5) for x in secs[r]])


if __name__ == "__main__":
    main()
