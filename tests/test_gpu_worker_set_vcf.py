"""--store_mutations in the side-by-side worker set: every worker of a set owns a region of the engine's
row pool, the rows of a turn are placed on the device (k_mt_mut_place_w), and the rows of all workers become one VCF text job
(iss_vcf_emit_workers).  A worker's rows, reads, coordinates and stream positions must be those of a context of its own; the
command's files must be the reference's."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_RAN = b"workers side by side on one device"
MUT_FIELDS = ("pair", "mate", "type", "position", "ref", "alt", "quality")
READ_KEYS = ("r1_base", "r1_qual", "r2_base", "r2_qual")


def _engine(case, genomes):
    from insilicoseq_amd.engine import ReadEngine

    model = {"hiseq_gc": "hiseq", "basic": "basic"}.get(case, "novaseq")
    eng = ReadEngine(0)
    eng.load_model(dense_model(model, (0.01, 0.03) if case == "indel_heavy" else None))
    if case == "novaseq_frag":
        eng.mt_set_fragment(420.0, 35.0)
    return eng, [eng.add_genome(g) for g in genomes]


def _same_rows(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in MUT_FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


@pytest.mark.parametrize("turn", [None, "37/3"])
@pytest.mark.parametrize("case", ["novaseq", "hiseq_gc", "indel_heavy", "basic", "novaseq_frag"])
def test_set_rows_equal_separate_contexts(case, turn, monkeypatch):
    """generate_mt_workers with reserved rows against one context per worker (seed_mt(seed_w), generate_mt, mt_mutations): rows,
    read bytes, coordinates and the next words of both streams.  The configurations of test_worker_set_equals_separate_workers:
    turn 37/3 = many short turns with buffers of three turns; indel_heavy = the walker only (insertion and deletion rows);
    hiseq_gc = rejected pairs rewind their rows; novaseq_frag / basic = the single-worker path into the worker's own region;
    a record shorter than a read and a record with IUPAC letters (resolver-to-walker handovers in the middle of a turn) in
    the workers' lists; unequal pairs per worker, 0 among them."""
    from insilicoseq_amd._native import E_SHORT_RECORD, EngineError

    if turn:
        monkeypatch.setenv("ISS_MT_SET_TURN", turn.split("/")[0])
        monkeypatch.setenv("ISS_MT_SET_BUF_TURNS", turn.split("/")[1])
    gc = case == "hiseq_gc"
    genomes = [random_genome(311, 30000), random_genome(313, 120), mixed_genome(312, 9000)]  # plain, short, mixed
    seeds = [31, 32, 35, 40]
    W, rounds, stride = len(seeds), 3, 700
    r = np.random.RandomState(11)
    scale = 1 if case in ("indel_heavy", "basic") else 2
    plan = [[((w + k) % 3, int(r.randint(1, 300 * scale))) for w in range(W)] for k in range(rounds)]
    plan[1][2] = (0, 0)  # a worker that sits a round out
    plan[2][0] = (0, 0)
    got = [[None] * W for _ in range(rounds)]
    eng, gids = _engine(case, genomes)
    with eng:
        eng.seed_mt_workers(seeds)
        eng.mt_workers_mutations_reserve(40000)
        for k, calls in enumerate(plan):
            done, status = eng.generate_mt_workers([gids[g] for g, _ in calls], [n for _, n in calls], [w * stride for w in range(W)],
                                                   gc_bias=gc)
            for w, (g, n) in enumerate(calls):
                if n == 0:
                    continue
                assert status[w] == (E_SHORT_RECORD if g == 1 else 0), (case, k, w)
                if status[w] == 0:
                    assert done[w] == n
                    rows = eng.download(w * stride, n)
                    got[k][w] = ({key: rows[key].copy() for key in READ_KEYS}, eng.coords(w * stride, n).copy(),
                                 eng.mt_workers_mutations(w).copy())
        peeks = [eng.mt_workers_peek(w, 16) for w in range(W)]
        resolved, walked = eng.mt_path_counts()
    n_rows, kinds = 0, set()
    for w, seed in enumerate(seeds):
        one, gids = _engine(case, genomes)
        with one:
            one.seed_mt(seed)
            one.mt_mutations_reserve(40000)
            for k, calls in enumerate(plan):
                g, n = calls[w]
                if n == 0:
                    continue
                try:
                    assert one.generate_mt(gids[g], n, gc_bias=gc) == n
                except EngineError as e:
                    assert e.code == E_SHORT_RECORD and got[k][w] is None, (case, k, w)
                    continue
                reads, coords, rows = got[k][w]
                exp = one.download(0, n)
                for key in READ_KEYS:
                    assert np.array_equal(reads[key], exp[key]), (case, k, w, key)
                assert np.array_equal(coords, one.coords(0, n)), (case, k, w)
                exp_rows = one.mt_mutations()
                _same_rows(rows, exp_rows, (case, k, w))
                n_rows += len(rows)
                kinds |= set(int(x) for x in np.unique(rows["type"]))
            py, npw = one.mt_peek(16)
        assert np.array_equal(py, peeks[w][0]) and np.array_equal(npw, peeks[w][1]), (case, w)
    assert n_rows > 300, n_rows
    if case == "indel_heavy":
        assert kinds == {0, 1, 2} and resolved == 0
    if case in ("novaseq", "hiseq_gc"):
        assert resolved > 0 and walked > 0  # (the mixed record: pairs handed from the resolver to the walker)


@pytest.mark.parametrize("turn", [None, 2001])
def test_set_rows_long_turns_equal_separate_contexts(turn, monkeypatch):
    """Turns of more than 1024 pairs: k_mt_mut_place_w scans 2048 counts per tile, so a worker's places are carried from tile to
    tile -- what every run of the command does (1536 pairs per turn at 64 workers).  Two workers on one plain 2 Mbp record (few
    templates reach its ends, so turns run to their full length): at the default turn (4096 pairs at W = 2) 3001 and 2345 pairs
    are 6002 and 4690 counts, three tiles each with tails of 1906 and 594 counts; at turns of 2001 pairs, 4002 counts are two
    tiles with a tail of 1954, and a shorter turn follows behind the running count.  No tail is a multiple of the eight counts
    a lane takes.
    That a turn longer than a tile ran is not taken on trust: a worker's turn ends at the turn length, at the call's end or at
    a pair handed to the walker, so the longest turn holds at least resolved / (walked + the full and last turns) pairs."""
    if turn:
        monkeypatch.setenv("ISS_MT_SET_TURN", str(turn))
    genomes = [random_genome(341, 2000000)]
    seeds, pairs, stride = [61, 62], [3001, 2345], 3008
    ch = turn or 4096
    eng, gids = _engine("novaseq", genomes)
    with eng:
        eng.seed_mt_workers(seeds)
        eng.mt_workers_mutations_reserve(40000)
        done, status = eng.generate_mt_workers([gids[0]] * 2, pairs, [0, stride])
        assert list(done) == pairs and list(status) == [0, 0]
        got = []
        for w in range(2):
            rows = eng.download(w * stride, pairs[w])
            got.append(({key: rows[key].copy() for key in READ_KEYS}, eng.coords(w * stride, pairs[w]).copy(),
                        eng.mt_workers_mutations(w).copy()))
        peeks = [eng.mt_workers_peek(w, 16) for w in range(2)]
        resolved, walked = eng.mt_path_counts()
    turns = walked + sum(n // ch + 1 for n in pairs)
    print("turn %s: %d pairs resolved, %d walked, at most %d turns: the longest holds at least %d pairs" % (
        turn, resolved, walked, turns, -(-resolved // turns)))
    assert -(-resolved // turns) > 1024, (resolved, walked, turns)  # (more than one tile of 2048 counts)
    for w, seed in enumerate(seeds):
        one, gids = _engine("novaseq", genomes)
        with one:
            one.seed_mt(seed)
            one.mt_mutations_reserve(40000)
            assert one.generate_mt(gids[0], pairs[w]) == pairs[w]
            exp = one.download(0, pairs[w])
            for key in READ_KEYS:
                assert np.array_equal(got[w][0][key], exp[key]), (w, key)
            assert np.array_equal(got[w][1], one.coords(0, pairs[w])), w
            _same_rows(got[w][2], one.mt_mutations(), w)
            assert len(got[w][2]) > 500, len(got[w][2])
            py, npw = one.mt_peek(16)
        assert np.array_equal(py, peeks[w][0]) and np.array_equal(npw, peeks[w][1]), w


def test_vcf_emit_workers_equals_write_mutations(tmp_path):
    """One text job per round for all workers, two rounds into the same descriptors: worker k's file holds what write_mutations
    makes of its downloaded rows, round after round.  Worker numbers of one and two digits, a worker that sits a round out."""
    from insilicoseq_amd.generator import write_mutations

    genomes = [random_genome(321, 30000), mixed_genome(322, 9000)]
    seeds, cpus = [5, 6, 7], [0, 3, 12]
    plan = [[(0, 500, "plain", 0), (1, 260, "mixed", 40), (0, 90, "plain", 7)],
            [(1, 300, "mixed", 300), (0, 0, "", 0), (0, 410, "chr|x", 97)]]  # (record, pairs, record id, first pair id)
    stride = 600
    eng, gids = _engine("novaseq", genomes)
    files = [open(str(tmp_path / ("w%d.vcf" % k)), "w") for k in range(3)]
    want = [io.StringIO() for _ in range(3)]
    with eng:
        eng.seed_mt_workers(seeds)
        eng.mt_workers_mutations_reserve(20000)
        for calls in plan:
            done, _status = eng.generate_mt_workers([gids[g] for g, _n, _i, _f in calls], [n for _g, n, _i, _f in calls],
                                                    [w * stride for w in range(3)])
            eng.vcf_emit_workers([(files[w].fileno(), rid, first, w * stride, n, cpus[w]) if n else (-1, "", 0, 0, 0, cpus[w])
                                  for w, (_g, n, rid, first) in enumerate(calls)])
            for w, (_g, n, rid, first) in enumerate(calls):
                if n:
                    assert done[w] == n
                    write_mutations(eng.mt_workers_mutations(w), want[w], rid, first, cpus[w])
        eng.vcf_flush()
        ends = [os.lseek(fh.fileno(), 0, os.SEEK_CUR) for fh in files]
    for fh in files:
        fh.close()
    for w in range(3):
        text = open(str(tmp_path / ("w%d.vcf" % w)), "rb").read()
        assert text == want[w].getvalue().encode(), w
        assert ends[w] == len(text) and len(text) > 2000, (w, ends[w], len(text))


def test_row_overflow_is_an_error_and_poisons_the_set():
    """A reserve of a few rows per worker: the call returns E_NOMEM (an error return: the rows past a region are dropped by the
    kernels' bounds checks), the next call is refused until the set is seeded again, and a fresh set generates correctly."""
    from insilicoseq_amd._native import E_INVALID, E_NOMEM, EngineError

    genomes = [random_genome(331, 30000)]
    seeds = [51, 52, 53]
    eng, gids = _engine("novaseq", genomes)
    with eng:
        eng.seed_mt_workers(seeds)
        eng.mt_workers_mutations_reserve(3)
        with pytest.raises(EngineError) as e:
            eng.generate_mt_workers([gids[0]] * 3, [400, 400, 400], [0, 400, 800])
        assert e.value.code == E_NOMEM, e.value
        with pytest.raises(EngineError) as e:
            eng.generate_mt_workers([gids[0]] * 3, [10, 10, 10], [0, 400, 800])
        assert e.value.code == E_INVALID and "iss_mt_workers_seed" in str(e.value)
        eng.seed_mt_workers(seeds)
        eng.mt_workers_mutations_reserve(20000)
        done, _status = eng.generate_mt_workers([gids[0]] * 3, [400, 400, 400], [0, 400, 800])
        assert list(done) == [400, 400, 400]
        got = [(eng.download(w * 400, 400)["r1_base"].copy(), eng.mt_workers_mutations(w).copy()) for w in range(3)]
    for w, seed in enumerate(seeds):
        one, gids = _engine("novaseq", genomes)
        with one:
            one.seed_mt(seed)
            one.mt_mutations_reserve(20000)
            assert one.generate_mt(gids[0], 400) == 400
            assert np.array_equal(one.download(0, 400)["r1_base"], got[w][0]), w
            _same_rows(got[w][1], one.mt_mutations(), w)
            assert len(got[w][1]) > 3


def _generate(argv, env=None):
    p = subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate"] + list(argv), cwd=ROOT, stderr=subprocess.PIPE,
                       env=None if env is None else dict(os.environ, **env))
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-4000:]
    return p.stderr


def _cli_cpus8(case, tmp_path, env):
    z = np.load(os.path.join(GOLDEN, "generate", case + "_cpus8_vcf.npz"))
    fasta = os.path.join(GOLDEN, "genomes.fasta")
    if "fasta" in z.files:
        fasta = str(tmp_path / "in.fasta")
        with open(fasta, "wb") as fh:
            fh.write(z["fasta"].tobytes())
    model, n, seed = case.split("_")[1], case.split("_")[2][1:], case.split("_")[3][4:]
    out = str(tmp_path / "run")
    err = _generate(["--genomes", fasta, "--model", model, "-n", n, "--seed", seed, "--cpus", "8", "--devices", "1", "--rng", "mt",
                     "--store_mutations", "-o", out], env=env)
    assert b"8 " + SET_RAN in err, err.decode(errors="replace")[-4000:]  # (the set ran, not one process per worker)
    assert open(out + ".vcf", "rb").read() == z["vcf"].tobytes()
    assert open(out + "_R1.fastq", "rb").read() == z["r1"].tobytes()
    assert open(out + "_R2.fastq", "rb").read() == z["r2"].tobytes()
    assert open(out + "_abundance.txt", "rb").read() == z["abundance"].tobytes()
    assert sorted(os.listdir(str(tmp_path))) == sorted(["run.vcf", "run_abundance.txt", "run_R1.fastq", "run_R2.fastq"] +
                                                       (["in.fasta"] if "fasta" in z.files else []))


@pytest.mark.parametrize("case", ["genomes_hiseq_n1600_seed42", "syn3_novaseq_n3000_seed7"])
def test_generate_cli_cpus8_store_mutations_equals_reference(case, tmp_path):
    """`generate --rng mt --cpus 8 --devices 1 --store_mutations`: the four files equal the reference's byte for byte, nothing
    else is left, and the log says that the worker set ran."""
    _cli_cpus8(case, tmp_path, None)


def test_generate_cli_cpus8_store_mutations_host_route(tmp_path):
    """The same with ISS_HOST_VCF=1: the rows fetched worker by worker and written by write_mutations."""
    _cli_cpus8("syn3_novaseq_n3000_seed7", tmp_path, {"ISS_HOST_VCF": "1"})


def test_generate_cli_cpus3_store_mutations_equals_worker_iterators(tmp_path):
    """`--cpus 3 --store_mutations` through the set against three worker_iterator(rng="mt") runs over the same chunks, their
    files concatenated as the parent does."""
    from insilicoseq_amd import app
    from insilicoseq_amd.distributed import VCF_HEADER
    from insilicoseq_amd.generator import generate_work_divider, parse_fasta, worker_iterator
    from insilicoseq_amd.model import KDErrorModel

    fasta = os.path.join(GOLDEN, "genomes.fasta")
    out = str(tmp_path / "run")
    err = _generate(["--genomes", fasta, "--model", "hiseq", "-n", "1500", "--seed", "9", "--cpus", "3", "--devices", "1", "--rng",
                     "mt", "--store_mutations", "--abundance", "uniform", "-o", out])
    assert b"3 " + SET_RAN in err, err.decode(errors="replace")[-4000:]
    records = list(parse_fasta(fasta))
    em = KDErrorModel(os.path.join(ROOT, "insilicoseq_amd", "profiles", "hiseq.dense.npz"), None, None, True)
    abundance = app.uniform([r.id for r in records])
    chunks = list(generate_work_divider(records, None, abundance, 1500, None, None, em, str(tmp_path / "ref"), -((1500 // 2) // -3)))
    want = {".vcf": (VCF_HEADER + "\n").encode(), "_R1.fastq": b"", "_R2.fastq": b""}
    for k, chunk in enumerate(chunks[:3]):
        prefix = str(tmp_path / ("one%d" % k))
        worker_iterator(chunk, em, k, prefix, 9, "metagenomics", False, device=0, rng="mt")
        for suffix in want:
            want[suffix] += open(prefix + suffix, "rb").read()
    for suffix, text in want.items():
        assert open(out + suffix, "rb").read() == text, suffix
    assert len(want[".vcf"]) > 2000
