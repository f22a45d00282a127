"""The --store_mutations VCF text built on the device (ReadEngine.vcf_emit, iss_vcf.hip.h), byte for byte against the host
route -- write_mutations applied to mutations() / mt_mutations() of the same call, which other tests pin to the oracle and to
the reference's own files -- and, for some cases, against the oracle's rows formatted here."""
import gzip
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.close()


def _host_text(rows, items, cpu, row0=0):
    """The host route: write_mutations per item, the rows' pairs counted from the call's first output row `row0`."""
    from insilicoseq_amd.generator import write_mutations

    buf = io.StringIO()
    for rid, first_i, first_pair, n in items:
        lo = first_pair - row0
        sel = rows[(rows["pair"] >= lo) & (rows["pair"] < lo + n)].copy()
        sel["pair"] -= lo
        write_mutations(sel, buf, rid, first_i, cpu)
    return buf.getvalue().encode()


def _oracle_text(rows, rid, first_i, cpu):
    """iss/generator.py:598-620, row by row, for the oracle's mutation records."""
    lines = []
    for m in rows:
        ref, alt = chr(m["ref"]), chr(m["alt"])
        alt = ref + alt if m["type"] == 1 else alt
        qual = str(int(m["quality"])) if m["type"] == 0 else "."
        lines.append("\t".join(["%s_%d_%d/%d" % (rid, first_i + int(m["pair"]), cpu, 1 + int(m["mate"])), str(int(m["position"]) + 1),
                                ".", ref, alt, qual, "", ""]) + "\n")
    return "".join(lines).encode()


def _device_text(eng, path, items, cpu, source="philox"):
    with open(path, "wb") as fh:
        eng.vcf_emit(fh.fileno(), items, cpu, source=source)
        eng.vcf_flush()
        assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(path)  # the descriptor stands at the end
    return open(path, "rb").read()


SINGLE = [
    # (model, indel, genome, pairs, seed, first_i, cpu, compare with the oracle too)
    ("novaseq", None, lambda: random_genome(301, 100000), 20000, 3, 0, 0, True),
    ("hiseq", None, lambda: mixed_genome(302, 30000), 8000, 4, 5, 12, False),            # pair ids cross 9 -> 10 (and on)
    ("miseq", None, lambda: random_genome(303, 50000), 3000, 5, 99990, 1023, False),     # read length 301; 99999 -> 100000
    ("novaseq", (0.01, 0.03), lambda: mixed_genome(304, 20000), 3000, 6, 7, 12, True),   # indel rows, lower case and IUPAC refs
]


@pytest.mark.parametrize("case", range(len(SINGLE)))
def test_philox_single_call(engine, case, tmp_path):
    from oracle import oracle as O

    model, indel, mk, n, seed, first_i, cpu, with_oracle = SINGLE[case]
    dense = dense_model(model, indel)
    if model == "miseq":
        assert dense.read_length == 301
    genome = mk()
    engine.load_model(dense)
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.mutations_reserve(6_000_000)
    try:
        engine.generate(gid, n, first_ordinal=11, seed=seed)
        items = [("rec.%d" % case, first_i, 0, n)]
        got = _device_text(engine, str(tmp_path / "d.vcf"), items, cpu)
        rows = engine.mutations()
    finally:
        engine.mutations_reserve(0)
    exp = _host_text(rows, items, cpu)
    print("case %d: %d rows, %d bytes" % (case, len(rows), len(exp)))
    assert len(rows) > 100
    assert got == exp
    if with_oracle:
        res = O.Oracle(dense).simulate(O.Rng().seed_philox(seed), genome, n, first_ordinal=11, store_mutations=True)
        assert res["status"] == 0
        assert got == _oracle_text(res["mutations"], "rec.%d" % case, first_i, cpu)
    if indel:
        assert b"\t.\t\t\n" in got and re.search(rb"\t[A-Za-z]\t[A-Za-z]{2}\t\.\t\t\n", got)  # deletions and insertions
        assert re.search(rb"\t[a-z]\t", got) and re.search(rb"\t[NRYWSMKHBVD]\t", got)


def test_philox_batch_call(engine, tmp_path):
    """Several items in one generate_batch call whose rows start at output row 7: a 4096-byte id, an id with '|' and spaces,
    an item of no pairs, pair ids that start at different numbers."""
    dense = dense_model("hiseq")
    engine.load_model(dense)
    engine.clear_genomes()
    gids = [engine.add_genome(random_genome(310 + k, 20000 + 1000 * k)) for k in range(3)]
    counts = [500, 700, 300]
    items = [("L" * 4096, 95, 7, 500), ("none", 3, 507, 0), ("rec|1 a b", 99990, 507, 700), ("c", 0, 1207, 300)]
    engine.mutations_reserve(2_000_000)
    try:
        engine.generate_batch(gids, counts, first_ordinal=5, seed=9, out_first_pair=7)
        got = _device_text(engine, str(tmp_path / "d.vcf"), items, 12)
        rows = engine.mutations()
    finally:
        engine.mutations_reserve(0)
    exp = _host_text(rows, items, 12, row0=7)
    assert got == exp
    # (every item has rows, under its own id and numbers: five and six digits for the item that starts at 99990)
    assert got.count(b"L" * 4096 + b"_") > 50 and re.search(rb"\nrec\|1 a b_999\d\d_12/", got) and re.search(rb"\nrec\|1 a b_100\d\d\d_12/", got)
    assert re.search(rb"\nc_\d+_12/", got)
    assert b"none_" not in got


def test_philox_rebuilt_reads_leave_no_stale_rows(tmp_path, monkeypatch, capfd):
    """A custom fragment length on a genome barely longer than a read, and a model with indels that counts as light
    (ISS_LIGHT_INDELS=1: every read with an indel is rebuilt by the fix-up after k_main wrote its rows): many pairs are rebuilt
    and stale rows exist.  (The fragment length alone rebuilds 17 000 of 60 000 NovaSeq pairs and leaves no stale row: k_main
    writes none for pairs that are irregular from the start.)  The host route (iss_mutations_download) reports only the rows it
    keeps, so that it drops some in this case is read from the device filter's counters (ISS_VCF_DEBUG: slots that hold a row /
    rows that stay); the second figure must be the host route's row count."""
    from insilicoseq_amd.engine import ReadEngine

    monkeypatch.setenv("ISS_LIGHT_INDELS", "1")
    monkeypatch.setenv("ISS_VCF_DEBUG", "1")
    dense = dense_model("novaseq", (0.001, 0.003))
    genome = random_genome(320, dense.read_length + 40)
    n = 6000
    items = [("short", 0, 0, n)]
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        eng.mutations_reserve(4_000_000)
        eng.set_fragment(200, 60)
        eng.generate(gid, n, first_ordinal=3, seed=21)
        capfd.readouterr()
        got = _device_text(eng, str(tmp_path / "d.vcf"), items, 4)
        err = capfd.readouterr().err
        rows = eng.mutations()
        stats = eng.stats_read()
    m = re.search(r"\[vcf\] slot \d+: (\d+) slots hold a row, (\d+) rows stay", err)
    assert m, err
    used, kept = int(m.group(1)), int(m.group(2))
    print("rebuilt reads: %d; slots with a row %d, rows kept %d (host route: %d)" % (stats["fixup_reads"], used, kept, len(rows)))
    assert kept == len(rows) and used > kept, "no stale row in this case: it does not test what it claims"
    assert stats["fixup_reads"] > 0
    assert got == _host_text(rows, items, 4)


def test_philox_every_base_substituted(engine, tmp_path):
    """More than 64 rows per mate: every base of a 301-base read is substituted (602 rows per pair)."""
    dense = dense_model("miseq", (0.0, 0.0))
    dense.phred_thr[:] = 0.0
    genome = random_genome(330, 40000)
    n = 700
    engine.load_model(dense)
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.mutations_reserve(2_000_000)
    try:
        engine.generate(gid, n, first_ordinal=0, seed=2)
        items = [("all", 0, 0, n)]
        got = _device_text(engine, str(tmp_path / "d.vcf"), items, 0)
        rows = engine.mutations()
    finally:
        engine.mutations_reserve(0)
    assert len(rows) == 2 * 301 * n
    assert got == _host_text(rows, items, 0)


def test_two_emits_without_a_flush_and_a_growing_buffer(tmp_path):
    """Three calls emitted back to back on one descriptor, the third twenty times the first -- whose text slot it takes over, so
    that slot's buffer grows between the two: the file holds the texts in order."""
    from insilicoseq_amd.engine import ReadEngine

    dense = dense_model("hiseq")
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(random_genome(340, 60000))
        eng.mutations_reserve(4_000_000)
        path = str(tmp_path / "d.vcf")
        exp = b""
        with open(path, "wb") as fh:
            fh.write(b"##header\n")
            fh.flush()
            ordinal = 0
            for k, n in enumerate((2000, 4000, 40000)):
                eng.generate(gid, n, first_ordinal=ordinal, seed=8)
                items = [("g%d" % k, 10 * k, 0, n)]
                eng.vcf_emit(fh.fileno(), items, 3)
                # (the host route of the same call, read back after the emit was queued: it waits for the device itself)
                exp += _host_text(eng.mutations(), items, 3)
                ordinal += n
            eng.vcf_flush()
        assert open(path, "rb").read() == b"##header\n" + exp and len(exp) > 100000


def test_overflow_reports_the_slots_needed_and_appends_nothing(tmp_path):
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine

    dense = dense_model("hiseq")
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(random_genome(350, 60000))
        eng.mutations_reserve(1000)
        n, items = 20000, [("o", 0, 0, 20000)]
        path = str(tmp_path / "d.vcf")
        with open(path, "wb") as fh:
            fh.write(b"#kept\n")
            fh.flush()
            eng.generate(gid, n, first_ordinal=0, seed=1)
            with pytest.raises(_native.EngineError) as e:
                eng.vcf_emit(fh.fileno(), items, 0)
            assert e.value.code == _native.E_NOMEM and eng.mutation_slots_needed > 1000
            eng.vcf_flush()
            assert os.path.getsize(path) == 6
            need = eng.mutation_slots_needed
            eng.mutations_reserve(need + need // 8 + (1 << 16))
            eng.generate(gid, n, first_ordinal=0, seed=1)
            eng.vcf_emit(fh.fileno(), items, 0)
            assert eng.mutation_slots_needed == 0
            eng.vcf_flush()
            rows = eng.mutations()
        assert open(path, "rb").read() == b"#kept\n" + _host_text(rows, items, 0) and len(rows) > 1000


def test_no_rows_append_nothing(tmp_path):
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.model import DenseModel

    with ReadEngine(0) as eng:
        eng.load_model(DenseModel.perfect())
        gid = eng.add_genome(random_genome(360, 30000))
        eng.mutations_reserve(1_000_000)
        path = str(tmp_path / "d.vcf")
        with open(path, "wb") as fh:
            eng.generate(gid, 5000, first_ordinal=0, seed=1)
            eng.vcf_emit(fh.fileno(), [("p", 0, 0, 5000)], 0)
            eng.vcf_flush()
            assert len(eng.mutations()) == 0
            eng.generate(gid, 0, first_ordinal=0, seed=1)
            eng.vcf_emit(fh.fileno(), [("p", 0, 0, 0)], 0)
            eng.vcf_emit(fh.fileno(), [], 0)
            eng.vcf_flush()
        assert os.path.getsize(path) == 0


def test_a_write_error_surfaces_once(tmp_path):
    """A descriptor opened read-only (EBADF on the host, nothing on the device): the next flush raises E_IO "write failed ...",
    the one after returns, the file is as it was and the next emit appends the host route's bytes."""
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine

    n, items = 3000, [("w", 0, 0, 3000)]
    path, good = str(tmp_path / "readonly.vcf"), str(tmp_path / "good.vcf")
    with open(path, "wb") as fh:
        fh.write(b"#read only\n")
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("hiseq"))
        gid = eng.add_genome(random_genome(370, 30000))
        eng.mutations_reserve(1_000_000)
        eng.generate(gid, n, first_ordinal=0, seed=1)
        with open(path, "rb") as fh:
            eng.vcf_emit(fh.fileno(), items, 0)
            with pytest.raises(_native.EngineError) as e:
                eng.vcf_flush()
            assert e.value.code == _native.E_IO and e.value.message.startswith("write failed"), e.value.message
            eng.vcf_flush()
        assert open(path, "rb").read() == b"#read only\n"
        got = _device_text(eng, good, items, 0)
        rows = eng.mutations()
    assert got == _host_text(rows, items, 0) and len(rows) > 100


@pytest.mark.parametrize("model", ["novaseq", "basic"])
def test_mt_mode(model, tmp_path):
    """generate_mt rows (already in the reference's order) through the same length / offset / format kernels: several work items
    in a row on one handle; the KDE case against the oracle's rows too."""
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine
    from oracle import oracle as O

    dense = dense_model(model, (0.01, 0.03) if model == "novaseq" else None)
    genomes = [mixed_genome(370, 20000), random_genome(371, 9000)]
    path = str(tmp_path / "d.vcf")
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gids = [eng.add_genome(g) for g in genomes]
        eng.mt_mutations_reserve(400000)
        eng.seed_mt(77)
        rng = O.Rng().seed_mt(77)
        exp, exp_oracle = b"", b""
        with open(path, "wb") as fh:
            for k, (gid, n, first_i, row0) in enumerate([(gids[0], 1500, 0, 0), (gids[1], 700, 99500, 40), (gids[0], 300, 8, 0)]):
                assert eng.generate_mt(gid, n, out_first_pair=row0) == n
                items = [("mt|%d x" % k, first_i, row0, n)]
                eng.vcf_emit(fh.fileno(), items, 12, source="mt")
                exp += _host_text(eng.mt_mutations(), items, 12, row0=row0)
                if model == "novaseq":
                    res = O.Oracle(dense).simulate(rng, genomes[gid - gids[0]], n, store_mutations=True)
                    exp_oracle += _oracle_text(res["mutations"], "mt|%d x" % k, first_i, 12)
            eng.vcf_flush()
            got = open(path, "rb").read()
            assert got == exp and len(exp) > 5000
            if model == "novaseq":
                assert got == exp_oracle
            # too small a reservation: refused like mt_mutations()
            eng.mt_mutations_reserve(10)
            assert eng.generate_mt(gids[0], 1500) == 1500
            with pytest.raises(_native.EngineError) as e:
                eng.vcf_emit(fh.fileno(), [("x", 0, 0, 1500)], 0, source="mt")
            assert e.value.code == _native.E_INVALID
            eng.vcf_flush()
        assert os.path.getsize(path) == len(got)


def _worker_case(rng_mode):
    from insilicoseq_amd.generator import Record

    dense = dense_model("hiseq")
    dense.store_mutations = True
    dense.fragment_length = dense.fragment_sd = None
    recs = [Record(random_genome(380 + i, L), id="w%d" % i) for i, L in enumerate([6000, 100, 30000])]
    counts = [900, 50, 2500] if rng_mode == "philox" else [300, 50, 700]
    return dense, recs, counts


def _oracle_worker_vcf(dense, recs, counts, seed, cpu, rng_mode):
    from oracle import oracle as O

    rng = O.Rng().seed_philox(seed + cpu) if rng_mode == "philox" else O.Rng().seed_mt(seed + cpu)
    out, ordinal = b"", 0
    for r, n in zip(recs, counts):
        kw = dict(first_ordinal=ordinal) if rng_mode == "philox" else {}
        res = O.Oracle(dense).simulate(rng, r.seq, n, store_mutations=True, **kw)
        if res["status"] == O.SKIP_RECORD:
            continue
        assert res["status"] == 0
        ordinal += n
        out += _oracle_text(res["mutations"], r.id, 0, cpu)
    return out


@pytest.mark.parametrize("rng_mode", ["philox", "mt"])
def test_worker_iterator_takes_the_device_route(rng_mode, tmp_path, monkeypatch):
    """worker_iterator with store_mutations never calls write_mutations on the device route; the .vcf is the oracle's text, and
    ISS_HOST_VCF=1 (the host route) writes the same bytes."""
    from insilicoseq_amd import generator as G

    dense, recs, counts = _worker_case(rng_mode)
    work = [(r, n, "default") for r, n in zip(recs, counts)]
    exp = _oracle_worker_vcf(dense, recs, counts, 5, 2, rng_mode)
    assert len(exp) > 2000

    def refuse(*a, **k):
        raise AssertionError("write_mutations called on the device route")

    monkeypatch.delenv("ISS_HOST_VCF", raising=False)
    monkeypatch.delenv("ISS_HOST_FASTQ", raising=False)
    with monkeypatch.context() as mp:
        mp.setattr(G, "write_mutations", refuse)
        G.worker_iterator(work, dense, 2, str(tmp_path / "dev"), 5, "metagenomics", False, device=0, rng=rng_mode)
    assert open(str(tmp_path / "dev.vcf"), "rb").read() == exp
    monkeypatch.setenv("ISS_HOST_VCF", "1")
    G.worker_iterator(work, dense, 2, str(tmp_path / "host"), 5, "metagenomics", False, device=0, rng=rng_mode)
    assert open(str(tmp_path / "host.vcf"), "rb").read() == exp
    for s in ("_R1.fastq", "_R2.fastq"):
        assert open(str(tmp_path / "dev") + s, "rb").read() == open(str(tmp_path / "host") + s, "rb").read()


@pytest.mark.parametrize("compress", [False, True])
def test_cli_equals_the_host_route(compress, tmp_path):
    """`generate --store_mutations --gpus 2` (Philox mode): the same files as under ISS_HOST_VCF=1."""
    from insilicoseq_amd.engine import ReadEngine

    ReadEngine(0).close()  # (no usable device: fail here, at once, and not in the workers of two commands)
    outs = {}
    for route in ("device", "host"):
        d = tmp_path / route
        d.mkdir()
        env = dict(os.environ)
        env.pop("ISS_HOST_VCF", None)
        if route == "host":
            env["ISS_HOST_VCF"] = "1"
        subprocess.check_call([sys.executable, "-m", "insilicoseq_amd", "generate", "--genomes", os.path.join(GOLDEN, "genomes.fasta"),
                               "--model", "hiseq", "-n", "3000", "--seed", "42", "--gpus", "2", "--devices", "1", "--store_mutations",
                               "-o", str(d / "run"), "--quiet"] + (["--compress"] if compress else []), cwd=ROOT, env=env,
                              timeout=90)  # (a run that hangs is a failure, not a wait)
        outs[route] = d
    rd = (lambda p: gzip.open(str(p) + ".gz", "rb").read()) if compress else (lambda p: open(str(p), "rb").read())
    for name in ("run.vcf", "run_R1.fastq", "run_R2.fastq"):
        a, b = rd(outs["device"] / name), rd(outs["host"] / name)
        assert a == b and len(a) > 1000, name
    assert open(str(outs["device"] / "run_abundance.txt"), "rb").read() == open(str(outs["host"] / "run_abundance.txt"), "rb").read()
    assert rd(outs["device"] / "run.vcf").startswith(b"##fileformat=VCFv4.1")
