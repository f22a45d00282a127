"""`generate --variants` on the device (iss_genome_upload_variants, iss_variants_lift) against the host twin
insilicoseq_amd.variants (VariantTable.apply_host / lift_host), byte for byte, and the command against itself: a run on
ref.fa + v.vcf writes the bytes a run on the haplotype's FASTA writes.  The twin is held to the naive splice without a GPU
(tests/test_variants_host.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import helpers as H
import variant_cases as VC
from insilicoseq_amd import origins as G
from insilicoseq_amd import variants as V
from insilicoseq_amd._native import EngineError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from insilicoseq_amd.engine import ReadEngine

    with ReadEngine(0) as e:
        e.load_model(H.dense_model("novaseq"))
        yield e


@pytest.fixture(scope="module")
def tile():
    return V.apply_tile()


def _device_equals_twin(eng, seq, variants):
    t = VC.table_of(seq, variants)
    want = t.apply_host(seq)
    gid = eng.add_genome_variants(seq, t)
    got = eng.genome_letters(gid)
    assert eng.genome_length(gid) == want.size == got.size
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("first difference at haplotype offset %d of %d: device %r, twin %r" % (
            at, want.size, got[max(at - 8, 0):at + 8].tobytes(), want[max(at - 8, 0):at + 8].tobytes()))
    return t, gid


# ---------------------------------------------------------------------- 1. device against twin
def test_hand_cases(eng):
    eng.clear_genomes()
    for _name, seq, variants in VC.hand_cases():
        _device_equals_twin(eng, seq, variants)


def test_lengths_around_a_tile(eng, tile):
    """Record and haplotype lengths of T - 1, T, T + 1 and 2 T + 3, reached with no change of length, by a deletion and by an
    insertion."""
    eng.clear_genomes()
    for X in (tile - 1, tile, tile + 1, 2 * tile + 3):
        for delta in (0, -5, 5):  # L' - L
            seq = H.random_genome(X + delta, X - delta)
            snv = (X // 2 + 9, seq[X // 2 + 9], "N")
            if delta == 0:
                variants = [snv, (X - 1, seq[X - 1], "a")]
            elif delta < 0:
                variants = [snv, (X - 7, seq[X - 7:X - 2], "")]
            else:
                variants = [snv, (X - 5, "", "acgtn")]  # (behind the record's last letter)
            t, _ = _device_equals_twin(eng, seq, variants)
            assert t.record_length == X - delta and int(t.out_pos[-1]) == X


def test_variants_across_tile_boundaries(eng, tile):
    eng.clear_genomes()
    T = tile
    seq = H.mixed_genome(31, 3 * T + 77)
    cases = {
        "deletion across an output boundary": [(T - 3, seq[T - 3:T + 4], "")],
        "deletion whose gap lies exactly on the boundary": [(T, seq[T:T + 9], "")],
        "substitution across a boundary": [(T - 2, seq[T - 2:T + 3], "TTTTT")],
        "insertion longer than a tile": [(50, "", "ACGTN" * (T // 5 + 20))],
        "insertion that ends on a boundary": [(100, "", "g" * (T - 100))],
        "insertion that starts on a boundary": [(T, "", "CC")],
        "sixteen one-base variants in one lane": [(64 + k, seq[64 + k], "acgtnACGTNacgtnA"[k]) for k in range(16)],
        "sixteen one-base indels in one lane": [(64 + k, seq[64 + k], "") if k % 2 else (64 + k, "", "t") for k in range(16)],
        "everything at once": [(5, "", "A" * (T + 3)), (T - 3, seq[T - 3:T + 4], ""), (2 * T - 1, seq[2 * T - 1:2 * T + 1], "NNNN"),
                               (3 * T, seq[3 * T:3 * T + 10], "c")],
    }
    for name, variants in cases.items():
        try:
            _device_equals_twin(eng, seq, variants)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


def test_a_record_above_small_record(eng):
    from insilicoseq_amd.generator import SMALL_RECORD

    eng.clear_genomes()
    rng = np.random.RandomState(77)
    L = SMALL_RECORD + 1234
    seq = H.random_genome(78, L)
    variants, at = [], 100
    while at < L - 100:
        kind = rng.randint(0, 3)
        if kind == 0:
            variants.append((at, seq[at], "N"))
        elif kind == 1:
            variants.append((at, seq[at:at + 40], ""))
        else:
            variants.append((at, "", "acgt" * 11))
        at += int(rng.randint(60, 9000))
    t, gid = _device_equals_twin(eng, seq, variants)
    assert len(t) > 100 and eng.genome_length(gid) > SMALL_RECORD
    eng.clear_genomes()


def test_random_cases(eng, tile):
    eng.clear_genomes()
    rng = np.random.RandomState(4242)
    for k in range(100):
        seq, variants = VC.random_case(rng, max_len=300 if k % 4 else 3 * tile)
        _device_equals_twin(eng, seq, variants)
        if k % 25 == 24:
            eng.clear_genomes()


# ---------------------------------------------------------------------- 2. the REF check
def test_ref_mismatch_is_one_line_and_the_context_lives_on(eng):
    eng.clear_genomes()
    seq = H.random_genome(5, 4000)
    good = [(10, seq[10], "N"), (2000, seq[2000:2003], "")]
    wrong = "A" if seq[3000] != "A" else "C"
    bad = VC.table_of(seq, good + [(3000, wrong + seq[3001], "TT"), (3500, wrong if seq[3500] != wrong else "G", "")])
    with pytest.raises(EngineError) as e:
        eng.add_genome_variants(seq, bad, record_id="chrT")
    msg = str(e.value)
    assert "\n" not in msg.strip() and "chrT" in msg and "POS 3001" in msg, msg
    assert wrong + seq[3001] in msg and seq[3000:3002] in msg, msg
    # a lower-case record against an upper-case REF passes
    t = VC.table_of(seq.lower(), [(p, r.upper(), a) for p, r, a in good])
    gid = eng.add_genome_variants(seq.lower(), t)
    assert np.array_equal(eng.genome_letters(gid), t.apply_host(seq.lower()))
    # ... and an ALT letter outside the alphabet is found by the pack
    with pytest.raises(EngineError) as e:
        eng.add_genome_variants(seq, VC.table_of(seq, [(77, seq[77], "Z")]))
    assert "0x5a" in str(e.value) and "offset 77" in str(e.value)
    # after the errors the context uploads and generates
    gid = eng.add_genome_variants(seq, VC.table_of(seq, good))
    eng.generate(gid, 256, first_ordinal=0, seed=3)
    eng.synchronize()
    c = eng.coords(0, 256)
    assert c[:, 0].min() >= 0 and c[:, 0].max() < 4000


def test_tables_that_break_a_rule_launch_nothing(eng):
    seq = H.random_genome(6, 500)
    t = VC.table_of(seq, [(10, seq[10], "N"), (200, seq[200:203], "")])
    t.pos0[1] = 499
    with pytest.raises(EngineError):
        eng.add_genome_variants(seq, t)
    t = VC.table_of(seq, [(10, seq[10], "N"), (200, seq[200:203], "")])
    t.out_pos[-1] += 1
    with pytest.raises(EngineError):
        eng.add_genome_variants(seq, t)


# ---------------------------------------------------------------------- 3. pack parity
def _rows(eng, n):
    eng.synchronize()
    d = eng.download(0, n)
    return {k: d[k].copy() for k in ("r1_base", "r1_qual", "r2_base", "r2_qual")}, eng.coords(0, n).copy()


def _parity_case(seed, mixed):
    rng = np.random.RandomState(seed)
    for _ in range(100):
        seq, variants = VC.random_case(rng, max_len=6000, min_len=5000, letters=VC.LETTERS if mixed else "ACGT", rate=0.02)
        if len(variants) > 20:
            return seq, variants
    raise AssertionError("no case")


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "iupac_lower"])
def test_rows_from_a_spliced_genome_equal_rows_from_its_haplotype(eng, mixed):
    eng.clear_genomes()
    seq, variants = _parity_case(90 + mixed, mixed)
    t = VC.table_of(seq, variants)
    a = eng.add_genome_variants(seq, t)
    b = eng.add_genome(t.apply_host(seq).tobytes())
    n = 3000
    eng.generate(a, n, first_ordinal=1000, seed=11)
    rows_a, coords_a = _rows(eng, n)
    eng.generate(b, n, first_ordinal=1000, seed=11)
    rows_b, coords_b = _rows(eng, n)
    assert np.array_equal(coords_a, coords_b)
    for k in rows_a:
        assert np.array_equal(rows_a[k], rows_b[k]), k


def test_mt_rows_from_a_spliced_genome_equal_rows_from_its_haplotype(eng):
    eng.clear_genomes()
    seq, variants = _parity_case(93, True)
    t = VC.table_of(seq, variants)
    a = eng.add_genome_variants(seq, t)
    b = eng.add_genome(t.apply_host(seq).tobytes())
    n = 1500
    eng.seed_mt(1234)
    assert eng.generate_mt(a, n) == n
    rows_a, coords_a = _rows(eng, n)
    eng.seed_mt(1234)
    assert eng.generate_mt(b, n) == n
    rows_b, coords_b = _rows(eng, n)
    assert np.array_equal(coords_a, coords_b)
    for k in rows_a:
        assert np.array_equal(rows_a[k], rows_b[k]), k


# ---------------------------------------------------------------------- 4. the lift
def test_lift_equals_the_twin(eng):
    eng.clear_genomes()
    rng = np.random.RandomState(8)
    seq, variants = _parity_case(95, False)
    t = VC.table_of(seq, variants)
    plain = eng.add_genome(H.random_genome(1, 700))
    gid = eng.add_genome_variants(seq, t)
    probe = VC.lift_probe(t, rng, 10000)
    assert np.array_equal(eng.lift(probe, gid=gid), t.lift_host(probe))
    assert np.array_equal(eng.lift(probe, gid=plain), probe)  # a genome without a table: the identity
    gids = np.where(rng.random_sample(probe.size) < 0.5, gid, plain).astype(np.int32)
    want = np.where(gids == gid, t.lift_host(probe), probe)
    assert np.array_equal(eng.lift(probe, gids=gids), want)
    # a second spliced genome, uploaded after the first lift: the tables follow
    seq2, variants2 = _parity_case(96, True)
    t2 = VC.table_of(seq2, variants2)
    gid2 = eng.add_genome_variants(seq2, t2)
    probe2 = VC.lift_probe(t2, rng, 1000)
    assert np.array_equal(eng.lift(probe2, gid=gid2), t2.lift_host(probe2))
    on_device = eng.lift(torch.from_numpy(probe2).to("cuda:0").reshape(-1, 1), gid=gid2)
    assert on_device.is_cuda and tuple(on_device.shape) == (probe2.size, 1)
    assert np.array_equal(on_device.cpu().numpy().ravel(), t2.lift_host(probe2))


# ---------------------------------------------------------------------- 5. the whole command
IDS = ("chrA", "chrB", "chrC")


def _genome_and_vcf(where):
    rng = np.random.RandomState(2024)
    seqs = [H.random_genome(41, 4000), H.mixed_genome(42, 3100), H.random_genome(43, 2500)]
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for rid, seq in zip(IDS[:2], seqs[:2]):  # (chrC has no variants)
        at = 30
        while at < len(seq) - 60:
            kind = int(rng.randint(0, 4))
            anchor = seq[at - 1]
            if kind == 0:
                lines.append("%s\t%d\t.\t%s\t%s\t.\t.\t." % (rid, at + 1, seq[at].upper(), "ACGT"[("ACGT".find(seq[at].upper()) + 1) % 4]))
            elif kind == 1:  # deletion, anchored
                lines.append("%s\t%d\t.\t%s\t%s\t.\t.\t." % (rid, at, anchor + seq[at:at + 7], anchor))
            elif kind == 2:  # insertion, anchored, and a second allele nobody asks for
                lines.append("%s\t%d\t.\t%s\t%s\t.\t.\t." % (rid, at, anchor, anchor + "GATTACA" * int(rng.randint(1, 30)) + ",<DUP>"))
            else:
                lines.append("%s\t%d\t.\t%s\t%s\t.\t.\t." % (rid, at + 1, seq[at:at + 3], "nnTA"))
            at += int(rng.randint(40, 400))
    lines.append("chrUn\t5\t.\tA\tC\t.\t.\t.")
    fasta, vcf = str(where / "ref.fa"), str(where / "v.vcf")
    with open(fasta, "w") as fh:
        for rid, seq in zip(IDS, seqs):
            fh.write(">%s some description\n" % rid)
            fh.write("\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + "\n")
    with open(vcf, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return fasta, vcf, seqs


def _generate(out, fasta, *flags):
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", "3000",
                    "--seed", "7", "--coverage", "uniform", "--output", out] + list(flags), cwd=ROOT, check=True, timeout=600)
    assert not [f for f in os.listdir(os.path.dirname(out)) if ".iss.tmp." in f]


def _same_files(a, b, suffixes):
    for suffix in suffixes:
        assert os.path.getsize(a + suffix) > 0, suffix
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix


@pytest.fixture(scope="module")
def command(tmp_path_factory):
    where = tmp_path_factory.mktemp("variants_cli")
    fasta, vcf, seqs = _genome_and_vcf(where)
    tables, skipped = V.read_vcf(vcf, dict(zip(IDS, (len(s) for s in seqs))))
    return {"where": where, "fasta": fasta, "vcf": vcf, "seqs": seqs, "tables": tables, "skipped": skipped}


OUTPUT_FLAGS = ("--store_mutations", "--origins", "--depth")
SHARED = ("_R1.fastq", "_R2.fastq", ".vcf", "_origins.bedpe", "_depth.txt", "_coverage.txt")


@pytest.mark.parametrize("rng", ["philox", "mt"])
def test_command_equals_a_run_on_the_haplotype(command, rng):
    a, b = str(command["where"] / ("a_" + rng)), str(command["where"] / ("b_" + rng))
    _generate(a, command["fasta"], "--variants", command["vcf"], "--write_haplotype", "--rng", rng, *OUTPUT_FLAGS)
    _generate(b, a + "_haplotype.fasta", "--rng", rng, *OUTPUT_FLAGS)
    _same_files(a, b, SHARED)
    assert open(a + "_R1.fastq").read().count("\n") // 4 > 1000
    # the haplotype file is the twin's, the summary the tables'
    from insilicoseq_amd.generator import parse_fasta

    hap = {r.id: r.seq for r in parse_fasta(a + "_haplotype.fasta")}
    for rid, seq in zip(IDS, command["seqs"]):
        t = command["tables"].get(rid)
        assert hap[rid] == (t.apply_host(seq).tobytes().decode() if t is not None else seq), rid
    summary = json.load(open(a + "_variants.json"))
    assert summary["skipped"] == command["skipped"] and summary["skipped"]["unknown_chrom"] == 1
    for rid, seq in zip(IDS, command["seqs"]):
        t = command["tables"].get(rid)
        entry = dict(summary["records"][rid])
        assert entry.pop("L") == len(seq) and entry.pop("L_haplotype") == len(hap[rid])
        assert entry == (t.counts() if t is not None else dict.fromkeys(entry, 0))
    if rng != "philox":
        return
    # the chain carries the origins back: the record's letters under a lifted interval, with the variants that touch it put in,
    # hold the template the read was cut from
    chains = V.read_chain(open(a + "_haplotype.chain"))
    assert sorted(chains) == sorted(command["tables"])
    raw = G.parse(a + G.SUFFIX)
    lifted = G.parse(a + G.SUFFIX, lift={rid: (lambda h, c=chains[rid]: V.lift_chain(c, h)) for rid in chains})
    seq_of = dict(zip(IDS, command["seqs"]))
    checked = 0
    for k in range(0, len(raw["id"]), 7):
        rid = raw["id"][k]
        t = command["tables"].get(rid)
        for s, e in (("s1", "e1"), ("s2", "e2")):
            hs, he, rs, re = (int(x[k]) for x in (raw[s], raw[e], lifted[s], lifted[e]))
            template = hap[rid][hs:he]
            if t is None:
                assert (rs, re) == (hs, he) and seq_of[rid][rs:re] == template
                continue
            assert (rs, re) == (int(t.lift_host([hs])[0]), int(t.lift_host([he])[0]))
            touching = [i for i in range(len(t)) if t.pos0[i] <= re and t.pos0[i] + t.ref_len[i] >= rs]
            lo = min([rs] + [int(t.pos0[i]) for i in touching])
            hi = max([re] + [int(t.pos0[i] + t.ref_len[i]) for i in touching])
            piece = seq_of[rid][lo:hi]
            sub = [(int(t.pos0[i]) - lo, piece[int(t.pos0[i]) - lo:int(t.pos0[i] + t.ref_len[i]) - lo],
                    bytes(t.alt[int(t.alt_off[i]):int(t.alt_off[i] + t.alt_len[i])]).decode()) for i in touching]
            assert template in VC.naive_splice(piece, sub), (rid, hs, he, rs, re)
            checked += 1
    assert checked > 100


def test_command_in_the_worker_set(command):
    """--rng mt --cpus 3 --devices 1: three workers side by side in one context (no --origins / --depth: those take the pool)."""
    a, b = str(command["where"] / "a_set"), str(command["where"] / "b_set")
    more = ("--rng", "mt", "--cpus", "3", "--devices", "1", "--store_mutations")
    _generate(a, command["fasta"], "--variants", command["vcf"], "--write_haplotype", *more)
    _generate(b, a + "_haplotype.fasta", *more)
    _same_files(a, b, ("_R1.fastq", "_R2.fastq", ".vcf", "_coverage.txt"))
    # with --origins the same workers run as one process each and read the records, and the VCF, again: the same reads
    c = str(command["where"] / "a_pool")
    _generate(c, command["fasta"], "--variants", command["vcf"], "--origins", *more)
    _same_files(c, a, ("_R1.fastq", "_R2.fastq", ".vcf"))
    assert os.path.getsize(c + G.SUFFIX) > 0


# ---------------------------------------------------------------------- 6. the tensor stream
def test_tensor_stream_ref_coords():
    from insilicoseq_amd.tensors import ReadTensorStream

    seq, variants = _parity_case(97, False)
    t = VC.table_of(seq, variants)
    other = H.random_genome(98, 3000)
    with ReadTensorStream([other, seq], H.dense_model("novaseq"), [(1, 300), (0, 200), (1, 100)], batch_pairs=400, seed=5,
                          variants={1: t}) as stream:
        batches = list(stream)
    assert [int(b.coords.shape[0]) for b in batches] == [400, 200]
    for b in batches:
        coords, record, ref_coords = b.coords.cpu().numpy(), b.record.cpu().numpy(), b.ref_coords.cpu().numpy()
        want = coords.copy()
        rows = record == 1
        want[rows, :3] = t.lift_host(coords[rows, :3])
        assert rows.any() and (~rows).any() and np.array_equal(ref_coords, want)
        assert np.array_equal(ref_coords[:, 3], coords[:, 3])
    with ReadTensorStream([other, seq], H.dense_model("novaseq"), [(1, 50)], batch_pairs=50, seed=5) as stream:
        assert next(iter(stream)).ref_coords is None
