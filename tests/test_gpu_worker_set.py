"""The worker set in final-file mode (worker_set_iterator(..., final_prefix=...): every round one text job whose items are
written at their places of the final files) against the same set in temp-file mode and against separate
worker_iterator(rng="mt") runs, which the reference goldens of test_gpu_mt_compat.py tie to `iss generate`: the final files
must be the temp files joined in worker order, and a worker's temp files its separate run's."""
import os

import numpy as np
import pytest

from helpers import dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

SEED = 77


def _records():
    from insilicoseq_amd.generator import Record

    return {"plain": Record(random_genome(201, 30000), id="plain"), "mixed": Record(mixed_genome(202, 9000), id="mixed"),
            "short": Record(random_genome(203, 120), id="short"), "s": Record(random_genome(204, 2500), id="s")}


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _three_ways(works, em, cpus, tmp_path, batch_pairs=None, separate=()):
    """Final files, temp files and (for the workers in `separate`) separate runs of the same works."""
    from insilicoseq_amd.generator import worker_iterator, worker_set_iterator

    unused = [str(tmp_path / ("u%d" % c)) for c in cpus]
    final = str(tmp_path / "final")
    assert worker_set_iterator(works, em, cpus, unused, SEED, "metagenomics", False, device=0, batch_pairs=batch_pairs,
                               final_prefix=final) is True
    assert not any(os.path.exists(u + "_R1.fastq") for u in unused)  # (no temp file in final mode)
    temp = [str(tmp_path / ("t%d" % c)) for c in cpus]
    assert worker_set_iterator(works, em, cpus, temp, SEED, "metagenomics", False, device=0, batch_pairs=batch_pairs) is False
    for suffix in ("_R1.fastq", "_R2.fastq"):
        parts = [_read(t + suffix) for t in temp]
        got = _read(final + suffix)
        assert len(got) == sum(len(p) for p in parts), suffix
        at = 0
        for c, p in zip(cpus, parts):  # worker by worker: the first that differs names the culprit
            assert got[at:at + len(p)] == p, (suffix, c)
            at += len(p)
    for k in separate:
        one = str(tmp_path / ("one%d" % cpus[k]))
        worker_iterator(works[k], em, cpus[k], one, SEED, "metagenomics", False, device=0, rng="mt")
        for suffix in ("_R1.fastq", "_R2.fastq"):
            assert _read(temp[k] + suffix) == _read(one + suffix), (cpus[k], suffix)
    return _read(final + "_R1.fastq")


@pytest.mark.parametrize("batch_pairs, pieces", [(10, None), (64, None), (300, "4")])
def test_final_files_many_rounds_mixed_widths(batch_pairs, pieces, tmp_path, monkeypatch):
    """Work lists of different lengths over worker numbers of one to four digits; one long item that keeps its worker busy
    after the others are done; pieces that start at pair 10, 100 and 1000 (batch_pairs 10); a record with IUPAC and lower-case
    letters (the walker), one shorter than a read, a worker whose items are all short records (it writes nothing) and a
    zero-pair item.  pieces: ISS_FASTQ_PIECES (writer threads per file)."""
    if pieces:
        monkeypatch.setenv("ISS_FASTQ_PIECES", pieces)
    r = _records()
    d = lambda *items: [(r[name], n, "default") for name, n in items]  # noqa: E731
    works = [d(("plain", 250), ("s", 30)),
             d(("short", 40)),
             d(("plain", 1500)),
             d(("mixed", 120), ("plain", 0), ("s", 101)),
             d(("s", 9), ("s", 11), ("plain", 100)),
             d(("mixed", 60), ("short", 5), ("plain", 200)),
             d(("plain", 1))]
    cpus = [3, 9, 10, 11, 99, 100, 1000]
    text = _three_ways(works, dense_model("novaseq"), cpus, tmp_path, batch_pairs=batch_pairs, separate=(2, 3, 5))
    assert text.count(b"\n") == 4 * (280 + 1500 + 221 + 120 + 260 + 1)
    assert b"_1499_10/1\n" in text and b"_0_1000/1\n" in text and b"_9/1\n" not in text


def test_final_files_a_hundred_workers_in_one_job(tmp_path):
    """W = 100, worker numbers 0, 11, ..., 1089: 100 items in one text job (k_fastq_format's binary search over the items),
    widths 1 to 4 in the same job; then the same works in rounds of 16 pairs."""
    r = _records()
    rng = np.random.RandomState(9)
    names = ["plain", "mixed", "s"]
    works = [[(r[names[int(k)]], int(rng.randint(1, 40)), "default") for k in rng.randint(0, 3, size=int(rng.randint(1, 4)))]
             for _ in range(100)]
    cpus = list(range(0, 1100, 11))
    em = dense_model("hiseq")
    for sub in ("one_job", "rounds"):
        os.makedirs(str(tmp_path / sub))
    _three_ways(works, em, cpus, tmp_path / "one_job")
    _three_ways(works, em, cpus, tmp_path / "rounds", batch_pairs=16)


def test_final_files_genome_budget_mid_run(tmp_path, monkeypatch):
    """A genome budget smaller than one record: the set drops its uploaded records between rounds (clear_genomes) and
    uploads them again -- in final mode as in temp-file mode."""
    from insilicoseq_amd import generator
    from insilicoseq_amd.engine import ReadEngine

    monkeypatch.setattr(generator.Worker, "GENOME_BUDGET", 2 * 12000)
    clears = [0]
    real = ReadEngine.clear_genomes

    def counting(self):
        clears[0] += 1
        return real(self)

    monkeypatch.setattr(ReadEngine, "clear_genomes", counting)
    r = _records()
    works = [[(r["plain"], 200, "default"), (r["s"], 50, "default")], [(r["mixed"], 150, "default")],
             [(r["s"], 20, "default"), (r["plain"], 180, "default")]]
    _three_ways(works, dense_model("novaseq"), [8, 9, 10], tmp_path, batch_pairs=64, separate=(0,))
    assert clears[0] >= 4


def test_failure_after_round_one_leaves_no_final_file(tmp_path, monkeypatch):
    """The engine fails in the second round: the error propagates and neither final file is left behind."""
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.generator import worker_set_iterator

    calls = [0]
    real = ReadEngine.generate_mt_workers

    def second_fails(self, *a, **k):
        calls[0] += 1
        if calls[0] == 2:
            raise _native.EngineError(_native.E_INVALID, "injected failure")
        return real(self, *a, **k)

    monkeypatch.setattr(ReadEngine, "generate_mt_workers", second_fails)
    r = _records()
    works = [[(r["plain"], 300, "default")], [(r["s"], 200, "default")]]
    final = str(tmp_path / "final")
    with pytest.raises(_native.EngineError, match="injected failure"):
        worker_set_iterator(works, dense_model("novaseq"), [0, 1], [str(tmp_path / "a"), str(tmp_path / "b")], SEED, "metagenomics",
                            False, device=0, batch_pairs=64, final_prefix=final)
    assert calls[0] == 2
    assert sorted(os.listdir(str(tmp_path))) == []
