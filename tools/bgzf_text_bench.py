#!/usr/bin/env python
"""What `generate --bgzip` costs and saves, NovaSeq 2 x 151.  One JSON line per figure, everything of one
box and one session, the routes alternating run by run:

  (a) the device side of one origins emit call between two HIP events on the engine's stream, in mode 0 (k_origins_len, the scan,
      k_origins_format) and in mode 1 (the same, then k_bgzt_dist / hist / build / len, the scan and k_bgzt_encode), at --pairs
      pairs over --records records of --length bases: the stage is the difference;
  (b) the whole command, `generate --origins --bgzip` against `generate --origins --compress`, same inputs, one worker and four
      on one device (wall time of the process);
  (c) the size of the members against zlib levels 1 and 6 of the same text, and against the runs-only code (no line copies:
      ISS_DEFLATE_RUNS_ONLY, the stream tests/bgzf_text_twin.py builds with runs_only=True).

    python tools/bgzf_text_bench.py
    python tools/bgzf_text_bench.py --pairs 1000000 --dir /dev/shm

Times are medians of --reps runs after a warm-up.  Only figures of one box and one session compare."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from insilicoseq_amd import _native  # noqa: E402
from insilicoseq_amd.engine import ReadEngine  # noqa: E402
from insilicoseq_amd.generator import Record  # noqa: E402
from insilicoseq_amd.model import DenseModel  # noqa: E402

MODEL = os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz")


def out(**kw):
    print(json.dumps(kw), flush=True)


def records(n, length):
    rng = np.random.RandomState(5)
    return [Record(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, length)].tobytes().decode(), id="NZ_BENCH%04d.1" % k) for k in range(n)]


def device_stage(recs, per, reps, tmp):
    """(a) and (c): HIP-event times of the emit call's device side in both modes; the files' sizes."""
    n = per * len(recs)
    stream = torch.cuda.Stream()
    paths = {0: os.path.join(tmp, "text.bedpe"), 1: os.path.join(tmp, "members.bedpe"), 2: os.path.join(tmp, "runs_only.bedpe")}
    with ReadEngine(0) as eng:
        eng.load_model(DenseModel.load(MODEL))
        gids = [eng.add_genome(r.seq) for r in recs]
        eng.reserve(n)
        eng.set_stream(stream.cuda_stream)
        lengths = [len(r.seq) for r in recs]
        items = [(r.id, 0, k * per, per) for k, r in enumerate(recs)]
        eng.generate_batch(gids, [per] * len(recs), first_ordinal=0, seed=3, out_first_pair=0)
        ms = {0: [], 1: [], 2: []}
        for rep in range(reps + 1):
            for mode in (0, 1, 2):  # 2: mode 1 without line copies
                if mode == 2:
                    os.environ["ISS_DEFLATE_RUNS_ONLY"] = "1"
                eng.origins_compress(mode > 0)
                with open(paths[mode], "wb") as fh:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    eng.origins_emit_batch(fh.fileno(), items, lengths, 0)
                    t1.record(stream)
                    t1.synchronize()
                    eng.origins_flush()
                os.environ.pop("ISS_DEFLATE_RUNS_ONLY", None)
                if rep:
                    ms[mode].append(t0.elapsed_time(t1))
        eng.origins_compress(False)
        eng.set_stream(None)
    size = {k: os.path.getsize(p) for k, p in paths.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    out(what="origins emit, device side, mode 0: k_origins_len + scan + k_origins_format (HIP events)", pairs=n, text_bytes=size[0],
        ms=round(med[0], 4), ms_all=[round(x, 4) for x in ms[0]])
    out(what="origins emit, device side, mode 1: the same + k_bgzt_* (HIP events)", pairs=n, member_bytes=size[1], ms=round(med[1], 4),
        ms_all=[round(x, 4) for x in ms[1]], stage_ms=round(med[1] - med[0], 4), stage_text_GB_per_s=round(size[0] / (med[1] - med[0]) / 1e6, 2),
        stage_over_format=round((med[1] - med[0]) / med[0], 2))
    with open(paths[0], "rb") as fh:
        text = fh.read()
    z = {}
    for level in (1, 6):
        t0 = time.perf_counter()
        z[level] = sum(len(zlib.compress(text[at:at + (32 << 20)], level)) for at in range(0, len(text), 32 << 20))
        z["s%d" % level] = time.perf_counter() - t0
    out(what="sizes of the origins text", text_bytes=size[0], bgzf_line_copies=size[1], bgzf_runs_only=size[2], zlib_1=z[1], zlib_6=z[6],
        ratio_line_copies=round(size[0] / size[1], 3), ratio_runs_only=round(size[0] / size[2], 3), ratio_zlib_1=round(size[0] / z[1], 3),
        ratio_zlib_6=round(size[0] / z[6], 3), zlib_1_one_thread_s=round(z["s1"], 2), zlib_6_one_thread_s=round(z["s6"], 2))


def whole_command(recs, per, reps, tmp):
    """(b): wall time of the two commands, alternating."""
    fasta = os.path.join(tmp, "genomes.fasta")
    with open(fasta, "w") as fh:
        for r in recs:
            fh.write(">%s\n%s\n" % (r.id, r.seq))
    n_reads = 2 * per * len(recs)
    for workers in (1, 4):
        secs, sizes = {"--bgzip": [], "--compress": []}, {}
        for rep in range(reps + 1):
            for flag in secs:
                d = tempfile.mkdtemp(prefix="cmd.", dir=tmp)
                t0 = time.perf_counter()
                subprocess.check_call([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq",
                                       "-n", str(n_reads), "--seed", "3", "--abundance", "uniform", "--origins", flag, "--gpus", str(workers),
                                       "--devices", "1", "-o", os.path.join(d, "run")], cwd=ROOT)
                t = time.perf_counter() - t0
                sizes[flag] = os.path.getsize(os.path.join(d, "run_origins.bedpe.gz"))
                shutil.rmtree(d, ignore_errors=True)
                if rep:
                    secs[flag].append(t)
        med = {k: statistics.median(v) for k, v in secs.items()}
        out(what="generate --origins --bgzip against --origins --compress (wall time of the command)", workers=workers, pairs=n_reads // 2,
            bgzip_s=round(med["--bgzip"], 3), compress_s=round(med["--compress"], 3), bgzip_all=[round(x, 3) for x in secs["--bgzip"]],
            compress_all=[round(x, 3) for x in secs["--compress"]], compress_over_bgzip=round(med["--compress"] / med["--bgzip"], 3), bgzip_bedpe_gz_bytes=sizes["--bgzip"],
            compress_bedpe_gz_bytes=sizes["--compress"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5000000)
    ap.add_argument("--records", type=int, default=5)
    ap.add_argument("--length", type=int, default=5000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-commands", action="store_true", help="(a) and (c) only")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    a = ap.parse_args()
    out(library=_native.LIB_PATH, build_id=_native.lib().iss_build_id().decode())
    recs = records(a.records, a.length)
    per = a.pairs // len(recs)
    tmp = tempfile.mkdtemp(prefix="bgzf_text_bench.", dir=a.dir)
    try:
        device_stage(recs, per, a.reps, tmp)
        if not a.skip_commands:
            whole_command(recs, per, a.reps, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
