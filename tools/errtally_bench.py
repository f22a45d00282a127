#!/usr/bin/env python
"""What the error tally costs: NovaSeq 2 x 151, --pairs pairs in ONE generate_batch call under the default
reservation (tensors.default_mutation_slots), HIP events, the legs alternating run by run in one process:

  iss_mutations_tally       the tally of the call's rows
  iss_mutations_export      the event rows at full capacity: the existing path that reads the same slots and orders them
  slot buffer copy          a device-to-device copy of as many bytes as the reserved slots hold

and worker_iterator with --store_mutations, with and without error_report, in pairs/s of the steady state.

    python tools/errtally_bench.py                       # everything, one JSON line per figure
    ISS_ERRTALLY_WGS=64 python tools/errtally_bench.py --kernels-only    # another launch geometry

Times are medians of --reps runs after a warm-up."""
import argparse
import json
import os
import statistics
import sys

import torch  # before the engine's library (insilicoseq_amd/tensors.py: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from insilicoseq_amd import errtally as E  # noqa: E402
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
        gids = [eng.add_genome(r) for r in recs]
        slots = T.default_mutation_slots(dense, n, torch.cuda.get_device_properties(0).multi_processor_count)
        eng.mutations_reserve(slots)
        counts = [n // len(gids)] * len(gids)
        counts[0] += n - sum(counts)
        eng.generate_batch(gids, counts, first_ordinal=0, seed=1)
        eng.synchronize()
        eng.set_stream(stream.cuda_stream)
        legs = ("tally", "export", "copy")
        with torch.cuda.stream(stream):
            words = torch.zeros(eng.error_tally_words(), dtype=torch.int64, device="cuda")
            events = torch.empty((slots, 6), dtype=torch.int32, device="cuda")
            n_events = torch.zeros((), dtype=torch.int64, device="cuda")
            src = torch.zeros(slots * 12, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = {k: [] for k in legs}
            for r in range(reps + 1):
                for what in legs:
                    ev[0].record(stream)
                    if what == "tally":
                        eng.error_tally(0, n, words.data_ptr())
                    elif what == "export":
                        eng.export_mutations(0, n, events_ptr=events.data_ptr(), capacity=slots, n_events_ptr=n_events.data_ptr())
                    else:
                        dst.copy_(src)
                    ev[1].record(stream)
                    ev[1].synchronize()
                    if r >= 1:
                        ms[what].append(ev[0].elapsed_time(ev[1]))
            t = E.split(words.cpu().numpy().view(np.uint64), eng.read_length)
            rows = int(n_events.item())
            assert int(t["pairs"][0]) == n * (reps + 1) and int(t["dropped"][0]) == 0
            assert rows == int(t["sub_q"].sum() + t["ins"].sum() + t["del"].sum()) // (reps + 1)
        eng.set_stream(None)
    names = {"tally": "iss_mutations_tally", "export": "iss_mutations_export (events)", "copy": "slot buffer copy"}
    for what in legs:
        t = statistics.median(ms[what])
        out(what=names[what], pairs=n, slots=slots, slot_bytes=slots * 12, rows=rows, ms=round(t, 4), ms_all=[round(x, 4) for x in ms[what]],
            slots_gb_per_s=round(slots * 12 / t / 1e6, 1), errtally_wgs=os.environ.get("ISS_ERRTALLY_WGS", "default"))


def worker(npz, genome, pairs, out_dir, error_report):
    from insilicoseq_amd.generator import Record, worker_iterator
    from insilicoseq_amd.model import KDErrorModel

    em = KDErrorModel(npz, None, None, True)
    prefix = os.path.join(out_dir, "errtally_bench_%d" % os.getpid())
    timings = {}
    try:
        worker_iterator([(Record(genome, id="bench"), pairs, "default")], em, 0, prefix, 42, "metagenomics", False, device=0,
                        timings=timings, **({"error_report": True} if error_report else {}))
    finally:
        for s in ("_R1.fastq", "_R2.fastq", ".vcf", ".errtally.npy"):
            if os.path.exists(prefix + s):
                os.remove(prefix + s)
    return timings["t_end"] - timings["t_ready"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out-dir", default="/dev/shm")
    a = ap.parse_args()
    npz = os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz")
    dense = DenseModel.load(npz)
    recs = records()
    from insilicoseq_amd import _native

    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode(), device=torch.cuda.get_device_name(0))
    kernels(dense, recs, a.pairs, a.reps)
    if a.kernels_only:
        return
    genome = recs[0].decode() + recs[1].decode()
    legs = {"store_mutations": False, "store_mutations + error_report": True}
    secs = {k: [] for k in legs}
    for rep in range(a.reps + 1):
        for k, flag in legs.items():
            t = worker(npz, genome, a.pairs, a.out_dir, flag)
            if rep:
                secs[k].append(t)
    for k in legs:
        t = statistics.median(secs[k])
        out(what="worker_iterator " + k, pairs=a.pairs, s=round(t, 5), pairs_per_s=round(a.pairs / t, 1), s_all=[round(x, 5) for x in secs[k]])


if __name__ == "__main__":
    main()
