#!/usr/bin/env python
"""What the coverage depth costs: iss_depth_mark next to iss_output_tally of the same rows -- NovaSeq
2 x 151, 5 M pairs of one generate_batch over bench.py's genomes (5 x 5 Mbp, 123), HIP events, the two alternating run by run
in one process; iss_depth_finish (depth, statistics, 1 000-base windows) on that 25 M-word array next to a device-to-device copy
of the same bytes; and ReadTensorStream in pairs/s with depth=True next to depth=False.

    python tools/depth_bench.py                  # everything, one JSON line per figure
    ISS_DEPTH_WGS=4096 python tools/depth_bench.py --kernels-only    # another launch geometry

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

from insilicoseq_amd import depth as D  # noqa: E402
from insilicoseq_amd import tensors as T  # noqa: E402
from insilicoseq_amd.engine import ReadEngine  # noqa: E402
from insilicoseq_amd.model import DenseModel  # noqa: E402


def records(n=5, length=5000000, seed=123):  # (bench.py: synthetic_genomes)
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [letters[rng.randint(0, 4, size=length)].tobytes() for _ in range(n)]


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def kernels(dense, recs, n, reps, bin):
    stream = torch.cuda.Stream()
    wgs = os.environ.get("ISS_DEPTH_WGS", "default")
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gids = [eng.add_genome(r) for r in recs]
        counts = [n // len(recs)] * len(recs)
        counts[0] += n - sum(counts)
        eng.generate_batch(gids, counts, seed=1)
        eng.set_stream(stream.cuda_stream)
        table, n_words = D.depth_table([len(r) for r in recs])
        with torch.cuda.stream(stream):
            d_table = torch.from_numpy(table).cuda()
            diff = torch.zeros(n_words, dtype=torch.int32, device="cuda")
            words = torch.zeros(eng.tally_words(), dtype=torch.int64, device="cuda")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = {"mark": [], "tally": [], "finish": [], "copy": []}
            for r in range(reps + 2):
                for what, fn in (("mark", lambda: eng.depth_mark(0, n, d_table.data_ptr(), len(recs), diff.data_ptr())),
                                 ("tally", lambda: eng.tally(0, n, words.data_ptr()))):
                    t = timed(stream, ev, fn)
                    if r >= 2:
                        ms[what].append(t)
            depth = torch.empty(n_words, dtype=torch.int32, device="cuda")
            stats = torch.empty((len(recs), 4), dtype=torch.int64, device="cuda")
            bins = torch.empty(int(D.n_windows(table, bin).sum()), dtype=torch.int64, device="cuda")
            for r in range(reps + 2):
                for what, fn in (("finish", lambda: eng.depth_finish(diff.data_ptr(), n_words, depth.data_ptr(), d_table.data_ptr(), len(recs), bin,
                                                                      stats.data_ptr(), bins.data_ptr())),
                                 ("copy", lambda: depth.copy_(diff, non_blocking=True))):  # (hipMemcpyAsync, device to device)
                    t = timed(stream, ev, fn)
                    if r >= 2:
                        ms[what].append(t)
            eng.depth_finish(diff.data_ptr(), n_words, depth.data_ptr(), d_table.data_ptr(), len(recs), bin, stats.data_ptr(), bins.data_ptr())
            stream.synchronize()
            st = stats.cpu().numpy().view(np.uint64)
            assert int(words[0].item()) == n * (reps + 2)
            whole = int(st[:, 0].sum()) == 2 * 151 * n * (reps + 2)  # every interval of these rows lies inside its record
        eng.set_stream(None)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out(what="iss_depth_mark", pairs=n, ms=round(med["mark"], 4), ms_all=[round(x, 4) for x in ms["mark"]],
        atomics_per_s=round(4 * n / med["mark"] * 1e3, 1), depth_wgs=wgs)
    out(what="iss_output_tally", pairs=n, ms=round(med["tally"], 4), ms_all=[round(x, 4) for x in ms["tally"]])
    out(what="iss_depth_finish", words=n_words, bin=bin, ms=round(med["finish"], 4), ms_all=[round(x, 4) for x in ms["finish"]],
        gb_per_s=round(8 * n_words / med["finish"] / 1e6, 2), depth_wgs=wgs, max_depth=int(st[:, 3].max()), depth_sum_is_all_bases=whole)
    out(what="hipMemcpyAsync device to device", bytes=4 * n_words, ms=round(med["copy"], 4), ms_all=[round(x, 4) for x in ms["copy"]],
        gb_per_s=round(8 * n_words / med["copy"] / 1e6, 2))


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
    ap.add_argument("--bin", type=int, default=1000)
    ap.add_argument("--batch-pairs", type=int, default=1 << 20)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    dense = DenseModel.load(os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz"))
    recs = records()
    from insilicoseq_amd import _native

    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), device=torch.cuda.get_device_name(0))
    kernels(dense, recs, a.pairs, a.reps, a.bin)
    if a.kernels_only:
        return
    work = T.multinomial_work([1.0] * len(recs), a.total, seed=9)
    legs = {"depth=False": {}, "depth=True": {"depth": True}}
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
