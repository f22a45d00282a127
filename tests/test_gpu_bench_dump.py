"""bench.py --dump-outputs: a plain run writes the six .npy files of its last timed step, and their rows are what the engine
returns for that step -- regenerated here from the same model, genomes, work list, seed and first ordinal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("r1_base", "r1_qual", "r2_base", "r2_qual")


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    import bench
    from insilicoseq_amd.distributed import rank_work
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.generator import Record, lognormal_abundance
    from insilicoseq_amd.model import DenseModel

    reads, steps, warmup = 200_000, 2, 1
    out_dir = str(tmp_path / "dump")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", str(reads), "--steps", str(steps),
                          "--warmup", str(warmup), "--dump-outputs", out_dir], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["roofline"]["launches"] == steps and line["ms_per_step"] > 0
    assert "parity_window" not in line and "cpu_baseline" not in line  # (a plain run: those are --full's)
    total = line["config"]["pairs_per_step_per_gpu"]

    names = sorted(os.listdir(out_dir))
    assert names == sorted(k + ".npy" for k in KEYS + ("coords", "pair_index"))
    assert sum(os.path.getsize(os.path.join(out_dir, n)) for n in names) <= 64e6
    d = {n[:-4]: np.load(os.path.join(out_dir, n)) for n in names}
    idx = d["pair_index"]
    assert idx.dtype == np.float64 and d["coords"].dtype == np.float64 and d["coords"].shape == (len(idx), 4)
    # more pairs than the budget holds: a sample of whole 256-pair windows, in order, every pair once
    assert 0 < len(idx) < total and np.all(np.diff(idx) > 0) and idx[-1] < total
    win, count = np.unique(idx.astype(np.int64) // 256, return_counts=True)
    assert np.array_equal(count, np.minimum(256, total - win * 256))

    # the same step through the engine: bench.py's model, genomes, work divider, seed and the last timed step's first ordinal
    dense = DenseModel.load(os.path.join(ROOT, "insilicoseq_amd", "profiles", "novaseq.dense.npz"))
    genomes = bench.synthetic_genomes(bench.N_GENOMES, bench.GENOME_LEN, 123)
    records = [Record(bench._SeqLen(len(g)), id="genome_%d" % i) for i, g in enumerate(genomes)]
    abundance = lognormal_abundance([r.id for r in records], np.random.RandomState(123))
    chunk, _, _ = rank_work(records, None, abundance, reads, None, None, dense, "bench", 1, 0)
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid_of = {id(r): eng.add_genome(g) for r, g in zip(records, genomes)}
        ids, pairs = [gid_of[id(r)] for r, _, _ in chunk], [n for _, n, _ in chunk]
        assert sum(pairs) == total
        eng.generate_batch(ids, pairs, first_ordinal=(warmup + steps - 1) * total, seed=bench.SEED, out_first_pair=0)
        eng.synchronize()
        rows, coords = eng.download(0, total), eng.coords(0, total)
    at = idx.astype(np.int64)
    for k in KEYS:
        assert d[k].dtype == np.float32 and d[k].shape == (len(idx), dense.read_length), k
        assert np.array_equal(d[k], rows[k][at].astype(np.float32)), k
    assert np.array_equal(d["coords"], coords[at].astype(np.float64))
