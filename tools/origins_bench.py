#!/usr/bin/env python
"""What `generate --origins` costs, NovaSeq 2 x 151.  One JSON line per figure:

  * the device side of one emit call -- k_origins_len, the three scan launches and k_origins_format (with the call's two small
    table copies in front) -- between two HIP events on the engine's stream, at --pairs pairs over --records records of --length
    bases, next to a device-to-device copy of the text's bytes between the same kind of events;
  * one Philox worker end to end (worker_iterator: generation, the outputs' kernels, the copies, the writer threads, the files)
    with and without the flag, alternating run by run in one process.

    python tools/origins_bench.py
    python tools/origins_bench.py --pairs 20000000 --dir /dev/shm

Times are medians of --reps runs after a warm-up.  Only figures of one box and one session compare."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from insilicoseq_amd import _native  # noqa: E402
from insilicoseq_amd.engine import ReadEngine  # noqa: E402
from insilicoseq_amd.generator import Record, worker_iterator  # noqa: E402
from insilicoseq_amd.model import DenseModel, KDErrorModel  # noqa: E402

MODEL = os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz")


def out(**kw):
    print(json.dumps(kw), flush=True)


def records(n, length):
    rng = np.random.RandomState(5)
    return [Record(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, length)].tobytes().decode(), id="NZ_BENCH%04d.1" % k) for k in range(n)]


def kernels(recs, per, reps, tmp):
    """HIP-event times of the emit call's device side and of a device-to-device copy of the same bytes."""
    n = per * len(recs)
    stream = torch.cuda.Stream()
    with ReadEngine(0) as eng:
        eng.load_model(DenseModel.load(MODEL))
        gids = [eng.add_genome(r.seq) for r in recs]
        eng.reserve(n)
        eng.set_stream(stream.cuda_stream)
        lengths = [len(r.seq) for r in recs]
        items = [(r.id, 0, k * per, per) for k, r in enumerate(recs)]
        try:
            eng.generate_batch(gids, [per] * len(recs), first_ordinal=0, seed=3, out_first_pair=0)
            calls = [(items, lengths)]
        except _native.EngineError:  # records too long to stand side by side in one arena: one generate and one emit call per record
            calls = None
        ms, size = [], 0
        path = os.path.join(tmp, "kernels.bedpe")
        for rep in range(reps + 1):
            with open(path, "wb") as fh:
                total = 0.0
                for k in range(1 if calls else len(recs)):
                    if calls:
                        call = calls[0]
                    else:
                        eng.generate(gids[k], per, first_ordinal=k * per, seed=3, out_first_pair=k * per)
                        call = ([items[k]], [lengths[k]])
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    eng.origins_emit_batch(fh.fileno(), call[0], call[1], 0)
                    t1.record(stream)
                    t1.synchronize()
                    total += t0.elapsed_time(t1)
                eng.origins_flush()
            size = os.path.getsize(path)
            if rep:
                ms.append(total)
        t = statistics.median(ms)
        out(what="k_origins_len + scan + k_origins_format (HIP events)", pairs=n, emit_calls=1 if calls else len(recs), text_bytes=size,
            bytes_per_pair=round(size / n, 2), ms=round(t, 4), ms_all=[round(x, 4) for x in ms], pairs_per_s=round(n / t * 1e3, 1),
            text_GB_per_s=round(size / t / 1e6, 2))
        with torch.cuda.stream(stream):
            src, dst = torch.zeros(size, dtype=torch.uint8, device="cuda:0"), torch.empty(size, dtype=torch.uint8, device="cuda:0")
            cp = []
            for rep in range(reps + 1):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                dst.copy_(src)
                t1.record(stream)
                t1.synchronize()
                if rep:
                    cp.append(t0.elapsed_time(t1))
        c = statistics.median(cp)
        out(what="device-to-device copy of the text's bytes (HIP events)", bytes=size, ms=round(c, 4), ms_all=[round(x, 4) for x in cp],
            GB_per_s=round(size / c / 1e6, 2), origins_over_copy=round(t / c, 2))
        eng.set_stream(None)


def end_to_end(recs, per, reps, tmp):
    model = KDErrorModel(MODEL, None, None, False)
    work = [(r, per, "default") for r in recs]
    n = per * len(recs)
    routes = {"plain": {}, "origins": {"origins": True}}
    secs, size = {r: [] for r in routes}, 0
    for rep in range(reps + 1):
        for route, kw in routes.items():
            timings, prefix = {}, os.path.join(tmp, route)
            worker_iterator(work, model, 0, prefix, 3, "metagenomics", False, device=0, rng="philox", timings=timings, **kw)
            if rep:
                secs[route].append(timings["t_end"] - timings["t_ready"])
            if kw:
                size = os.path.getsize(prefix + "_origins.bedpe")
    for route in routes:
        t = statistics.median(secs[route])
        out(what="worker_iterator " + route, pairs=n, s=round(t, 4), pairs_per_s=round(n / t, 1), s_all=[round(x, 4) for x in secs[route]],
            origins_bytes=size if route == "origins" else 0)
    out(what="worker_iterator origins / plain", ratio=round(statistics.median(secs["origins"]) / statistics.median(secs["plain"]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5000000)
    ap.add_argument("--records", type=int, default=5)
    ap.add_argument("--length", type=int, default=5000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    a = ap.parse_args()
    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode())
    recs = records(a.records, a.length)
    per = a.pairs // len(recs)
    tmp = tempfile.mkdtemp(prefix="origins_bench.", dir=a.dir)
    try:
        kernels(recs, per, a.reps, tmp)
        end_to_end(recs, per, a.reps, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
