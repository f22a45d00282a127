"""--store_mutations with eight workers (tests/golden/tooling/make_golden_cpus8_vcf.py): the fixtures the worker set has to
reproduce on the device (tests/test_gpu_worker_set_vcf.py), pinned here without one -- by the reference's own files and by the
CPU oracle -- and the three ABI entries of the feature."""
import io
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("genomes_hiseq_n1600_seed42", "hiseq", 1600, 42, 13793, 432), ("syn3_novaseq_n3000_seed7", "novaseq", 3000, 7, 22437, 808)]


@pytest.mark.parametrize("case,model,n_reads,seed,vcf_bytes,vcf_rows", CASES)
def test_fixture_sizes_and_fastq_equal_the_run_without_the_flag(case, model, n_reads, seed, vcf_bytes, vcf_rows):
    """The reference's .vcf sizes, and --store_mutations changes no draw: r1 / r2 / abundance are the cpus8 goldens'."""
    from insilicoseq_amd.distributed import VCF_HEADER

    z = np.load(os.path.join(GOLDEN, "generate", case + "_cpus8_vcf.npz"))
    plain = np.load(os.path.join(GOLDEN, "generate", case + "_cpus8.npz"))
    vcf = z["vcf"].tobytes()
    assert len(vcf) == vcf_bytes
    assert vcf.startswith((VCF_HEADER + "\n").encode())
    rows = vcf[len(VCF_HEADER) + 1:].decode().splitlines()
    assert len(rows) == vcf_rows
    workers = [int(re.match(r".*_\d+_(\d+)/[12]$", ln.split("\t")[0]).group(1)) for ln in rows]
    assert workers == sorted(workers) and set(workers) == set(range(8))  # worker after worker, every one of them
    for key in ("r1", "r2", "abundance") + (("fasta",) if "fasta" in plain.files else ()):
        assert np.array_equal(z[key], plain[key]), key


@pytest.mark.parametrize("case,model,n_reads,seed,vcf_bytes,vcf_rows", CASES)
def test_eight_oracle_workers_reproduce_the_vcf(case, model, n_reads, seed, vcf_bytes, vcf_rows, tmp_path):
    """Chunk r of the reference's divider, worker seed = seed + r, the CPU oracle in MT mode with store_mutations, its rows
    written by write_mutations and the workers' texts concatenated behind the header: the reference's .vcf byte for byte."""
    from insilicoseq_amd import distributed as D
    from insilicoseq_amd.generator import lognormal_abundance, parse_fasta, write_mutations
    from insilicoseq_amd.model import DenseModel
    from oracle import oracle as O

    z = np.load(os.path.join(GOLDEN, "generate", case + "_cpus8_vcf.npz"))
    fasta = os.path.join(GOLDEN, "genomes.fasta")
    if "fasta" in z.files:
        fasta = str(tmp_path / "in.fasta")
        with open(fasta, "wb") as fh:
            fh.write(z["fasta"].tobytes())
    dense = DenseModel.load(os.path.join(ROOT, "insilicoseq_amd", "profiles", model + ".dense.npz"))
    records = list(parse_fasta(fasta))
    abundance = lognormal_abundance([r.id for r in records], np.random.RandomState(seed))
    text = io.StringIO()
    text.write(D.VCF_HEADER + "\n")
    for rank in range(8):
        work, _, _n_chunks = D.rank_work(records, None, abundance, n_reads, None, None, dense, str(tmp_path / "out"), 8, rank)
        assert work is not None
        orc, rng = O.Oracle(dense), O.Rng().seed_mt(seed + rank)
        for rec, n, _ in work:
            res = orc.simulate(rng, rec.seq, n, store_mutations=True)
            if res["status"] == O.SKIP_RECORD:
                continue
            assert res["status"] == 0
            write_mutations(res["mutations"], text, rec.id, 0, rank)
    assert text.getvalue().encode() == z["vcf"].tobytes()


def test_abi_names_the_three_entries():
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine

    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    assert "#define ISS_ABI_VERSION 8" in header
    assert re.search(r"\bint iss_mt_workers_mutations_reserve\(iss_ctx \*ctx, int64_t rows_per_worker\);", header)
    assert re.search(r"\bint iss_mt_workers_mutations_download\(iss_ctx \*ctx, int32_t worker, iss_mutation \*out, int64_t capacity, int64_t \*n_total\);", header)
    assert re.search(r"\bint iss_vcf_emit_workers\(iss_ctx \*ctx, int32_t n_workers, const int \*fds,", header)
    for name in ("iss_mt_workers_mutations_reserve", "iss_mt_workers_mutations_download", "iss_vcf_emit_workers"):
        assert name in _native.EXPORTS
    for name in ("mt_workers_mutations_reserve", "mt_workers_mutations", "vcf_emit_workers"):
        assert callable(getattr(ReadEngine, name))


class _Recorder:
    """The calls worker_set_iterator makes, with no device behind them."""

    def __init__(self, n_rows):
        self.calls, self.n_rows, self.read_length, self.W = [], n_rows, 0, 0

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call

    def load_model(self, dense):
        self.read_length = int(dense.read_length)

    def add_genome(self, _seq):
        self.calls.append(("add_genome", (), {}))
        return sum(1 for c in self.calls if c[0] == "add_genome") - 1

    def add_genomes(self, seqs):
        return [self.add_genome(s) for s in seqs]

    def seed_mt_workers(self, seeds):
        self.W = len(seeds)
        self.calls.append(("seed_mt_workers", (list(seeds),), {}))

    def generate_mt_workers(self, g, n, row, **k):
        self.calls.append(("generate_mt_workers", (list(g), list(n), list(row)), k))
        return np.array(n, dtype=np.int64), np.zeros(len(n), dtype=np.int32)


def test_worker_set_iterator_takes_the_set_with_store_mutations(tmp_path, monkeypatch):
    """worker_set_iterator no longer goes worker by worker for --store_mutations: one engine, rows reserved per worker by
    worker_iterator's rule at the set's pairs per round, one vcf_emit_workers per round with an entry per worker, vcf_flush
    before the handles close; the FASTQ goes to the final files and the workers' .vcf temp files are there for the parent."""
    from helpers import dense_model, random_genome
    from insilicoseq_amd import generator as G

    em = dense_model("novaseq")
    em.store_mutations = True
    rec = G.Record(random_genome(1, 5000), id="r")
    works = [[(rec, 700, "default")], [(rec, 300, "default")], [(rec, 1100, "default")]]
    made = []

    def engine(_device):
        made.append(_Recorder(0))
        return made[-1]

    monkeypatch.setattr(G, "ReadEngine", engine)
    prefixes = [str(tmp_path / ("out.iss.tmp.%d" % k)) for k in range(3)]
    wrote_final = G.worker_set_iterator(works, em, [0, 1, 2], prefixes, 7, "metagenomics", False, device=0, batch_pairs=500,
                                        final_prefix=str(tmp_path / "out"))
    assert wrote_final is True and len(made) == 1
    names = [c[0] for c in made[0].calls]
    reserve = [c for c in made[0].calls if c[0] == "mt_workers_mutations_reserve"]
    assert len(reserve) == 1 and reserve[0][1] == (int(500 * (2.0 * G._dense_of(em).expected_mutation_rows_per_pair() + 4.0)),)
    assert names.index("seed_mt_workers") < names.index("mt_workers_mutations_reserve") < names.index("generate_mt_workers")
    rounds = [i for i, n in enumerate(names) if n == "generate_mt_workers"]
    emits = [i for i, n in enumerate(names) if n == "vcf_emit_workers"]
    assert len(rounds) == len(emits) == 3 and all(r < e for r, e in zip(rounds, emits))
    items = [made[0].calls[i][1][0] for i in emits]
    assert all(len(it) == 3 for it in items)
    assert [(it[2], it[4], it[5]) for it in items[0]] == [(0, 500, 0), (0, 300, 1), (0, 500, 2)]
    assert [(it[2], it[4], it[5]) for it in items[1]] == [(500, 200, 0), (0, 0, 1), (500, 500, 2)]  # (worker 1 is done: no pairs)
    assert names.index("vcf_flush") > emits[-1] and names.index("vcf_flush") < names.index("close")
    assert sorted(os.listdir(str(tmp_path))) == ["out.iss.tmp.0.vcf", "out.iss.tmp.1.vcf", "out.iss.tmp.2.vcf", "out_R1.fastq",
                                                 "out_R2.fastq"]


def test_failed_run_leaves_neither_final_files_nor_worker_vcfs(tmp_path, monkeypatch):
    from helpers import dense_model, random_genome
    from insilicoseq_amd import _native
    from insilicoseq_amd import generator as G

    em = dense_model("novaseq")
    em.store_mutations = True
    rec = G.Record(random_genome(1, 5000), id="r")

    class Failing(_Recorder):
        def vcf_emit_workers(self, items):
            raise _native.EngineError(_native.E_IO, "write failed")

    monkeypatch.setattr(G, "ReadEngine", lambda _device: Failing(0))
    with pytest.raises(_native.EngineError):
        G.worker_set_iterator([[(rec, 100, "default")], [(rec, 100, "default")]], em, [0, 1],
                              [str(tmp_path / ("out.iss.tmp.%d" % k)) for k in range(2)], 7, "metagenomics", False, device=0,
                              final_prefix=str(tmp_path / "out"))
    assert os.listdir(str(tmp_path)) == []


def test_no_room_for_the_row_pool_is_a_set_that_was_not_set_up(tmp_path, monkeypatch):
    """E_NOMEM from the reserve (W regions of rows do not fit the device) is WorkerSetNotSetUp, like a shortage of stream
    buffers: nothing ran, nothing is left, and the command takes one process per worker.  Any other error stays what it is."""
    from helpers import dense_model, random_genome
    from insilicoseq_amd import _native
    from insilicoseq_amd import generator as G

    em = dense_model("novaseq")
    em.store_mutations = True
    rec = G.Record(random_genome(1, 5000), id="r")
    for code, raised in ((_native.E_NOMEM, G.WorkerSetNotSetUp), (_native.E_HIP, _native.EngineError)):
        class NoRoom(_Recorder):
            def mt_workers_mutations_reserve(self, rows, code=code):
                raise _native.EngineError(code, "hipMalloc failed")

        made = []
        monkeypatch.setattr(G, "ReadEngine", lambda _device, cls=NoRoom: made.append(cls(0)) or made[-1])
        with pytest.raises(raised) as e:
            G.worker_set_iterator([[(rec, 100, "default")], [(rec, 100, "default")]], em, [0, 1],
                                  [str(tmp_path / ("out.iss.tmp.%d" % k)) for k in range(2)], 7, "metagenomics", False, device=0,
                                  final_prefix=str(tmp_path / "out"))
        assert e.value.code == code and (raised is G.WorkerSetNotSetUp or not isinstance(e.value, G.WorkerSetNotSetUp))
        assert "generate_mt_workers" not in [c[0] for c in made[0].calls]
        assert os.listdir(str(tmp_path)) == []


def test_command_that_asked_for_a_vcf_gets_the_workers_files_from_a_model_that_records_nothing(tmp_path, monkeypatch):
    """--mode perfect --store_mutations: the model records nothing (no rows reserved, no text job), but the parent concatenates
    the workers' .vcf files behind the header -- they must be there, empty."""
    from helpers import dense_model, random_genome
    from insilicoseq_amd import generator as G

    em = dense_model("novaseq")
    assert not getattr(em, "store_mutations", False)
    rec = G.Record(random_genome(1, 5000), id="r")
    made = []

    def engine(_device):
        made.append(_Recorder(0))
        return made[-1]

    monkeypatch.setattr(G, "ReadEngine", engine)
    prefixes = [str(tmp_path / ("out.iss.tmp.%d" % k)) for k in range(2)]
    assert G.worker_set_iterator([[(rec, 100, "default")], [(rec, 60, "default")]], em, [0, 1], prefixes, 7, "metagenomics", False,
                                 device=0, final_prefix=str(tmp_path / "out"), vcf_files=True) is True
    names = [c[0] for c in made[0].calls]
    assert "mt_workers_mutations_reserve" not in names and "vcf_emit_workers" not in names
    assert sorted(os.listdir(str(tmp_path))) == ["out.iss.tmp.0.vcf", "out.iss.tmp.1.vcf", "out_R1.fastq", "out_R2.fastq"]
    assert all(os.path.getsize(p + ".vcf") == 0 for p in prefixes)
