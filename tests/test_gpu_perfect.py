"""`--mode perfect` on the GPU (PerfectErrorModel, quality mode 2).

Philox path: k_perfect's rows and coordinates equal the CPU oracle's on ``DenseModel.perfect()`` run as quality mode 1
(constant insert size, the degenerate quality rows inverted to 40 -- the same function of the same uniforms), bit for bit,
and so does the ``ISS_PERFECT_KERNEL=0`` route (k_main on the same tables).  Reference-identical mode: `generate --rng mt
--mode perfect` equals the reference's own files (tests/golden/tooling/make_golden_perfect.py) byte for byte, through the
process pool and through the worker set."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL = 125


def _perfect(read_length=RL):
    from insilicoseq_amd.model import DenseModel

    return DenseModel.perfect(read_length)


def _oracle(dense):
    from oracle import oracle as O

    return O.Oracle(dense, quality_mode=1, basic_insert_size=dense.basic_insert_size)


def _expect_kernel(eng):
    name = eng.main_kernel()
    if os.environ.get("ISS_PERFECT_KERNEL", "1") == "0":
        assert name.startswith("k_main"), name
    else:
        assert name == "k_perfect", name


def _check(got, coords, exp, frag=False):
    assert exp["status"] == 0
    if frag:  # (the reverse start of a cut-short template is the device's own: forward start, reverse end, insert size)
        assert np.array_equal(coords[:, [0, 2, 3]], exp["coords"][:, [0, 2, 3]])
    else:
        assert np.array_equal(coords, exp["coords"]), "pair coordinates differ"
    for k in ("r1_qual", "r2_qual", "r1_base", "r2_base"):
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, "%s differs at (pair, pos) %s ... (%d cells)" % (k, bad[:5].tolist(), len(bad))


CASES = [
    # (read length, genome builder, n_pairs, seed, first ordinal, sequence type, gc_bias, fragment (mu, sd), pairs per launch)
    (RL, lambda: random_genome(61, 200000), 6000, 42, 0, "metagenomics", False, None, None),
    (RL, lambda: mixed_genome(62, 50000), 40000, 2**40 + 17, 2**33 + 5, "metagenomics", False, None, None),
    (RL, lambda: mixed_genome(63, 30000), 20000, 7, 0, "metagenomics", True, None, None),
    (RL, lambda: random_genome(64, 200), 1500, 8, 100, "metagenomics", False, None, None),  # record < fragment: generator.py:144
    (RL, lambda: mixed_genome(65, 700), 1500, 9, 0, "amplicon", False, None, None),
    (RL, lambda: mixed_genome(66, 3000), 4000, 10, 0, "metagenomics", False, (300, 30), None),
    (RL, lambda: mixed_genome(67, 2000), 3000, 11, 3, "metagenomics", True, (200, 60), None),  # templates cut short
    (RL, lambda: mixed_genome(68, 40000), 9000, 12, 0, "metagenomics", False, None, 1000),  # nine launches
    (101, lambda: mixed_genome(69, 20000), 3000, 13, 0, "metagenomics", False, None, None),  # pitch 104: a short last piece
    (300, lambda: mixed_genome(70, 20000), 2000, 14, 0, "metagenomics", True, None, None),  # ten 128-byte lines per row
]


def _run_case(case):
    from insilicoseq_amd.engine import ReadEngine
    from oracle import oracle as O

    rl, mk, n, seed, first, seq_type, gc_bias, frag, chunk = CASES[case]
    dense = _perfect(rl)
    genome = mk()
    old = os.environ.get("ISS_CHUNK_PAIRS")
    if chunk:
        os.environ["ISS_CHUNK_PAIRS"] = str(chunk)
    try:
        with ReadEngine(0) as eng:
            eng.load_model(dense)
            gid = eng.add_genome(genome)
            if frag:
                eng.set_fragment(*frag)
            eng.generate(gid, n, first_ordinal=first, seed=seed, sequence_type=seq_type, gc_bias=gc_bias)
            eng.synchronize()
            got = eng.download(0, n)
            coords = eng.coords(0, n)
            _expect_kernel(eng)
    finally:
        if chunk:
            if old is None:
                os.environ.pop("ISS_CHUNK_PAIRS", None)
            else:
                os.environ["ISS_CHUNK_PAIRS"] = old
    exp = _oracle(dense).simulate(O.Rng().seed_philox(seed), genome, n, first_ordinal=first, sequence_type=seq_type,
                                  gc_bias=gc_bias, fragment_length=frag[0] if frag else None,
                                  fragment_sd=frag[1] if frag else None, want_coords=True)
    _check(got, coords, exp, frag is not None)
    return genome, got, coords


@pytest.mark.parametrize("case", range(len(CASES)))
def test_philox_matches_oracle(case):
    genome, got, coords = _run_case(case)
    if case == 1:  # the mixed-case genome: upper-casings really happened (~1e-4 per lower-case a/c/g/t: ~120 expected)
        g = np.frombuffer(genome.encode(), dtype=np.uint8)
        win = g[coords[:, 0:1] + np.arange(RL)]
        assert (got["r1_base"] != win).sum() > 10


def test_philox_batch_of_many_small_records_matches_oracle():
    """iss_generate_batch: many short records side by side in the arena (coordinates are the arena's) -- every item's rows
    equal the oracle's for its record, ordinals running across the items."""
    from insilicoseq_amd.engine import ReadEngine
    from oracle import oracle as O

    dense = _perfect()
    rng = np.random.RandomState(5)
    genomes = [mixed_genome(100 + k, int(rng.randint(130, 3000))) for k in range(60)]
    counts = [int(rng.randint(1, 300)) for _ in genomes]
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gids = [eng.add_genome(g) for g in genomes]
        eng.reserve(sum(counts))
        eng.generate_batch(gids, counts, first_ordinal=11, seed=77, out_first_pair=0)
        eng.synchronize()
        _expect_kernel(eng)
        row = 0
        for g, n in zip(genomes, counts):
            got = eng.download(row, n)
            coords = eng.coords(row, n)
            exp = _oracle(dense).simulate(O.Rng().seed_philox(77), g, n, first_ordinal=11 + row, want_coords=True)
            _check(got, coords, exp)
            row += n


def test_k_main_route_matches_oracle_in_a_child_process():
    """ISS_PERFECT_KERNEL=0: quality mode 2 through k_main on DenseModel.perfect()'s tables -- the A/B route -- gives the same
    rows (the oracle comparisons above, rerun in a fresh process with the switch set)."""
    env = dict(os.environ, ISS_PERFECT_KERNEL="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_philox_matches_oracle or test_philox_batch"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    tail = r.stdout.decode(errors="replace")[-3000:]
    assert r.returncode == 0, tail
    assert "%d passed" % (len(CASES) + 1) in tail, tail


def test_large_run_invariants():
    """1.5 M pairs on a mixed-case / IUPAC genome: R1 is the genome window and R2 its reverse complement up to case, every
    phred is 40, and only lower-case a/c/g/t change -- to their upper case, at about 1e-4 per such base."""
    from insilicoseq_amd.engine import ReadEngine

    genome = mixed_genome(71, 3_000_000)
    g = np.frombuffer(genome.encode(), dtype=np.uint8)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"acgtyrwskmnbvdhACGTYRWSKMNBVDH", b"tgcarywsmknvbhdTGCARYWSMKNVBHD"):
        comp[a] = b
    lower = np.zeros(256, dtype=bool)
    lower[list(b"acgt")] = True
    n = 1_500_000
    changed = lower_seen = 0
    with ReadEngine(0) as eng:
        eng.load_model(_perfect())
        gid = eng.add_genome(genome)
        eng.generate(gid, n, first_ordinal=0, seed=2024)
        eng.synchronize()
        _expect_kernel(eng)
        idx = np.arange(RL)
        for lo in range(0, n, 100_000):
            w = min(100_000, n - lo)
            got = eng.download(lo, w)
            c = eng.coords(lo, w)
            assert (got["r1_qual"] == 40).all() and (got["r2_qual"] == 40).all()
            assert (c[:, 3] == 200).all()
            for key, win in (("r1_base", g[c[:, 0:1] + idx]), ("r2_base", comp[g[c[:, 2:3] - 1 - idx]])):
                b = got[key]
                diff = b != win
                assert (lower[win[diff]] & (b[diff] == win[diff] - 32)).all()
                changed += int(diff.sum())
                lower_seen += int(lower[win].sum())
    rate = changed / lower_seen
    assert 0.5e-4 < rate < 1.5e-4, (changed, lower_seen)


# ---------------------------------------------------------------- reference-identical mode against the reference's files
GOLDEN_CASES = ["perfect_genomes_cpus1", "perfect_genomes_cpus2", "perfect_genomes_cpus3", "perfect_mixed", "perfect_frag300",
                "perfect_amplicon", "perfect_gcbias"]


def _golden(case):
    z = np.load(os.path.join(GOLDEN, "generate", case + ".npz"))
    return z, json.loads(str(z["meta"]))


def _generate(args, tmp_path, name="run", quiet=True, check=True):
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "insilicoseq_amd", "generate", "--mode", "perfect", "-o", out] + (["--quiet"] if quiet else []) + args
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if check:
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    return out, r


def _layouts():
    """(case, layout): every golden through the process pool (one process per worker; --store_mutations keeps a run of
    several workers off the worker set -- the perfect model records nothing, the VCF is the header alone); those of several
    workers through the worker set as well (--devices 1: the workers side by side on one GPU)."""
    out = []
    for case in GOLDEN_CASES:
        args = json.loads(str(np.load(os.path.join(GOLDEN, "generate", case + ".npz"))["meta"]))["args"]
        out.append((case, "pool"))
        if int(args[args.index("--cpus") + 1]) > 1:
            out.append((case, "set"))
    return out


@pytest.mark.parametrize("case,layout", _layouts())
def test_mt_mode_equals_reference(case, layout, tmp_path):
    z, meta = _golden(case)
    args = list(meta["args"])
    out, _ = _generate(["--genomes", os.path.join(GOLDEN, meta["fasta"]), "--rng", "mt", "--devices", "1"] + args +
                       (["--store_mutations"] if layout == "pool" else []), tmp_path)
    if layout == "pool":
        from insilicoseq_amd.distributed import VCF_HEADER

        assert open(out + ".vcf").read() == VCF_HEADER + "\n"  # (util.py:229-230: the header line, no row)
    assert open(out + "_abundance.txt", "rb").read() == z["abundance"].tobytes()
    assert open(out + "_R1.fastq", "rb").read() == z["r1"].tobytes()
    assert open(out + "_R2.fastq", "rb").read() == z["r2"].tobytes()


# ---------------------------------------------------------------- CLI, Philox
def test_cli_philox_equals_oracle(tmp_path):
    """Two workers, Philox: the abundance file is the reference's (same numpy stream), the FASTQ files the oracle's."""
    from insilicoseq_amd.distributed import rank_work
    from insilicoseq_amd.engine import fastq_write
    from insilicoseq_amd.generator import parse_fasta
    from oracle import oracle as O

    z, meta = _golden("perfect_genomes_cpus2")
    fasta = os.path.join(GOLDEN, "genomes.fasta")
    out, _ = _generate(["--genomes", fasta, "-n", "600", "--seed", "42", "--cpus", "2", "--devices", "1"], tmp_path)
    assert open(out + "_abundance.txt", "rb").read() == z["abundance"].tobytes()
    dense = _perfect()
    records = list(parse_fasta(fasta))
    abundance = {}
    for line in z["abundance"].tobytes().decode().splitlines():
        k, v = line.split("\t")
        abundance[k] = float(v)
    p1, p2 = tmp_path / "e1", tmp_path / "e2"
    with open(p1, "wb") as f1, open(p2, "wb") as f2:
        for rank in range(2):
            work, _, _ = rank_work(records, None, abundance, 600, None, None, dense, out, 2, rank)
            rng = O.Rng().seed_philox(42 + rank)
            ordinal = 0
            for rec, n, _ in work:
                if len(rec.seq) <= RL:
                    continue
                res = _oracle(dense).simulate(rng, rec.seq, n, first_ordinal=ordinal)
                assert res["status"] == 0
                fastq_write(f1.fileno(), f2.fileno(), rec.id, 0, rank, n, RL, RL, res["r1_base"], res["r1_qual"],
                            res["r2_base"], res["r2_qual"], 1)
                ordinal += n
    assert open(out + "_R1.fastq", "rb").read() == p1.read_bytes()
    assert open(out + "_R2.fastq", "rb").read() == p2.read_bytes()


def test_cli_philox_compress_and_store_mutations(tmp_path):
    """--compress: the .gz files gunzip to the uncompressed run's text.  --store_mutations: a VCF of the header alone (the
    reference's perfect model records nothing)."""
    from insilicoseq_amd.distributed import VCF_HEADER

    args = ["--genomes", os.path.join(GOLDEN, "generate", "perfect_mixed.fasta"), "-n", "20000", "--seed", "3", "--cpus", "2",
            "--devices", "1"]
    plain, _ = _generate(args, tmp_path, "plain")
    packed, _ = _generate(args + ["--compress"], tmp_path, "packed")
    for suffix in ("_R1.fastq", "_R2.fastq"):
        text = open(plain + suffix, "rb").read()
        assert text.count(b"\n") == 4 * 10000
        assert gzip.open(packed + suffix + ".gz").read() == text
        assert not os.path.exists(packed + suffix)
    muts, _ = _generate(args + ["--store_mutations"], tmp_path, "muts")
    assert open(muts + ".vcf").read() == VCF_HEADER + "\n"
    assert open(muts + "_R1.fastq", "rb").read() == open(plain + "_R1.fastq", "rb").read()


@pytest.mark.parametrize("rng", ["philox", "mt"])
def test_cli_short_records_are_skipped_with_the_reference_warnings(rng, tmp_path):
    fasta = tmp_path / "g.fasta"
    fasta.write_text(">short\n%s\n>long\n%s\n" % ("ACGT" * 25, random_genome(72, 5000)))
    abundance = tmp_path / "ab.txt"
    abundance.write_text("short\t0.5\nlong\t0.5\n")
    out, r = _generate(["--genomes", str(fasta), "-n", "200", "--seed", "5", "--abundance_file", str(abundance), "--rng", rng],
                       tmp_path, quiet=False)
    err = r.stderr.decode()
    assert "short shorter than read length for this ErrorModel" in err
    assert "Skipping short. You will have less reads than specified" in err
    r1 = open(out + "_R1.fastq").read().splitlines()
    assert len(r1) >= 4 * 40 and all(line.startswith("@long_") for line in r1[::4])
    assert all(q == "I" * RL for q in r1[3::4])
