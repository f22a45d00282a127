"""The mutation rows tallied on the device (ReadEngine.error_tally, k_errtally_rows / k_errtally_reads):
every word against the numpy twin applied to the rows of the same call (ReadEngine.mutations / mt_mutations), over the read
lengths, pair counts, windows, launch geometries and sources, the overflow of the row slots, the error paths,
ReadTensorStream(error_tally=True) and `generate --error_report`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (here, when the module is collected: torch's HIP runtime has to be the process's first)

from helpers import Guarded, dense_model, mixed_genome, random_genome
from insilicoseq_amd import errtally as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 4_000_000  # row slots of the engines below: far above what any case needs (the kernels take 256 per wavefront)
FIRST_ORDINAL = 11
SEED = 1
# model -> read length.  With SEED and FIRST_ORDINAL the oracle's rows of pairs [0, 333) of every model hold a substitution at
# position 0, one at position L - 1, one in mate 1, a pair with substitutions in both mates and a read with two rows (found on
# the CPU with the oracle; asserted again below).  151: five position tiles, the last of 23 positions; 32: exactly one tile.
MODELS = {"novaseq": 151, "miseq": 301, "basic125": 125, "basic32": 32, "basic33": 33}

_engines = {}


def _model(name):
    from insilicoseq_amd.model import DenseModel

    if name in ("basic32", "basic33"):  # (phreds around 20: a few hundred rows in 333 short pairs)
        return DenseModel.basic(MODELS[name], mean_quality=20)
    return dense_model("basic" if name == "basic125" else name)


def _genome(name):
    return random_genome(500 + MODELS[name], 50000)


def _engine(name):
    """One engine per model with rows reserved (made once)."""
    if name not in _engines:
        from insilicoseq_amd.engine import ReadEngine

        eng = ReadEngine(0)
        eng.load_model(_model(name))
        gid = eng.add_genome(_genome(name))
        eng.mutations_reserve(SLOTS)
        assert eng.read_length == MODELS[name] and eng.error_tally_words() == E.words(MODELS[name])
        _engines[name] = (eng, gid)
    return _engines[name]


def teardown_module(module):
    for eng, _ in _engines.values():
        eng.close()
    _engines.clear()


def _buffer(L, shift=0):
    """Guarded, zeroed words of a tally of read length L."""
    buf = Guarded(E.words(L) * 8, np.uint64, (E.words(L),), shift)
    buf.buf[buf.at:buf.at + buf.nbytes] = 0
    torch.cuda.synchronize()  # (filled on torch's stream, the engine works on its own)
    return buf


def _tally(eng, windows, source="philox", buf=None):
    buf = buf or _buffer(eng.read_length)
    for first, n in windows:
        eng.error_tally(first, n, buf.ptr, source=source)
    eng.synchronize()
    assert buf.guards_intact()
    return buf.value().copy()


def _assert_equal(got, exp, L):
    if not np.array_equal(got, exp):
        g, e = E.split(got, L), E.split(exp, L)
        bad = [name for name in E.FIELDS if not np.array_equal(g[name], e[name])]
        raise AssertionError("fields that differ: %s; first: got %r, expected %r" % (
            bad, g[bad[0]].reshape(-1)[:8] if bad else None, e[bad[0]].reshape(-1)[:8] if bad else None))


def _presences(rows, L):
    s = rows[rows["type"] == 0]
    both = set(s["pair"][s["mate"] == 0].tolist()) & set(s["pair"][s["mate"] == 1].tolist())
    reads = rows["pair"].astype(np.int64) * 2 + rows["mate"]
    return {"position 0": bool((s["position"] == 0).any()), "position L - 1": bool((s["position"] == L - 1).any()),
            "mate 1": bool((s["mate"] == 1).any()), "both mates of a pair": bool(both),
            "a read with two rows": bool(len(reads) and np.bincount(reads).max() >= 2)}


# ---------------------------------------------------------------------------------------------------- 1. whole calls, windows
@pytest.mark.parametrize("n_pairs", [1, 2, 63, 64, 65, 333])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_whole_call_equals_the_twin(name, n_pairs):
    eng, gid = _engine(name)
    L = eng.read_length
    eng.generate(gid, n_pairs, first_ordinal=FIRST_ORDINAL, seed=SEED)
    rows = eng.mutations()
    if n_pairs == 333:  # (not vacuous: the rows hold what the kernels can get wrong)
        have = _presences(rows, L)
        assert all(have.values()), have
    got = _tally(eng, [(0, n_pairs)])
    _assert_equal(got, E.errors_host(rows, 0, n_pairs, L), L)
    t = E.split(got, L)
    assert t["pairs"][0] == n_pairs and t["dropped"][0] == 0 and t["sub_q"].sum() == (rows["type"] == 0).sum()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_windows_inside_a_larger_call(name):
    """Windows of 1 to 257 pairs at rows 0 and 7 of a call of 333 pairs: the rows outside the window do not count."""
    eng, gid = _engine(name)
    L = eng.read_length
    eng.generate(gid, 333, first_ordinal=FIRST_ORDINAL, seed=SEED)
    rows = eng.mutations()
    whole = E.errors_host(rows, 0, 333, L)
    for first, n in ((0, 1), (7, 1), (0, 2), (7, 63), (0, 64), (7, 65), (0, 257), (7, 257)):
        exp = E.errors_host(rows, first, n, L)
        _assert_equal(_tally(eng, [(first, n)]), exp, L)
        if n == 257:
            assert 0 < E.split(exp, L)["sub_q"].sum() < E.split(whole, L)["sub_q"].sum()  # rows outside exist


# ---------------------------------------------------------------------------------------------------- 2. rebuilt reads, letters
@pytest.mark.parametrize("case", ["indel_heavy", "light_stale", "cut_templates", "letters"])
def test_rebuilt_reads_and_other_letters(case, monkeypatch):
    """indel_heavy: reads with insertions and deletions, rebuilt by the fix-up; light_stale: a light model with indels
    (ISS_LIGHT_INDELS=1), whose reads with an event are rebuilt after k_main wrote their rows -- stale rows exist and must not
    count; cut_templates: fragments of 300 +- 200 on 700 bases; letters: lower-case and IUPAC records (code 4).  The call stands
    at output row 5 and the window reaches over both of its ends."""
    from insilicoseq_amd.engine import ReadEngine

    if case == "light_stale":
        monkeypatch.setenv("ISS_LIGHT_INDELS", "1")
    dense = dense_model("novaseq", {"indel_heavy": (0.01, 0.03), "light_stale": (0.001, 0.003)}.get(case))
    L = dense.read_length
    genome = {"cut_templates": random_genome(521, 700), "letters": mixed_genome(530, 40000)}.get(case) or random_genome(520, 30000)
    n, row0 = 1500, 5
    total = row0 + n + 3
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        eng.generate(gid, total, seed=4)  # (every row holds something)
        eng.mutations_reserve(SLOTS)
        if case == "cut_templates":
            eng.set_fragment(300, 200)
        eng.generate(gid, n, first_ordinal=3, seed=21, out_first_pair=row0)
        rows = eng.mutations()
        if case in ("indel_heavy", "light_stale", "cut_templates"):
            assert eng.stats_read()["fixup_reads"] > 0, "no read was rebuilt: the case does not test what it claims"
        if case in ("indel_heavy", "light_stale"):
            assert (rows["type"] == 1).sum() > 20 and (rows["type"] == 2).sum() > 20
        if case == "letters":
            sub = rows[rows["type"] == 0]
            assert set(sub["ref"].tolist()) & set(b"acgt"), "no lower-case ref"
        assert len(rows) > 100
        exp = E.errors_host(rows, -row0, total, L)  # (the window starts five rows before the call's first pair)
        _assert_equal(_tally(eng, [(0, total)]), exp, L)
        assert E.split(exp, L)["pairs"][0] == total
        _assert_equal(_tally(eng, [(row0 + 100, 900)]), E.errors_host(rows, 100, 900, L), L)
        if case == "letters":
            t = E.split(exp, L)
            assert t["sub_mat"][:, :, :4, :4].sum() == t["sub_mat"].sum() > 0  # IUPAC positions take no substitution


# ---------------------------------------------------------------------------------------------------- 3. batches
def test_generate_batch_with_a_zero_pair_item():
    from insilicoseq_amd.engine import ReadEngine

    with ReadEngine(0) as eng:
        eng.load_model(dense_model("hiseq"))
        L = eng.read_length
        gids = [eng.add_genome(mixed_genome(81 + k, 3000 + 500 * k)) for k in range(3)]
        eng.reserve(200)
        eng.mutations_reserve(SLOTS)
        eng.generate_batch(gids, [65, 0, 130], first_ordinal=11, seed=5, out_first_pair=2)
        rows = eng.mutations()
        assert len(rows) > 50
        _assert_equal(_tally(eng, [(2, 195)]), E.errors_host(rows, 0, 195, L), L)
        _assert_equal(_tally(eng, [(0, 200)]), E.errors_host(rows, -2, 200, L), L)  # (over both ends of the call's rows)
        _assert_equal(_tally(eng, [(2 + 65, 130)]), E.errors_host(rows, 65, 130, L), L)  # the third item alone


# ---------------------------------------------------------------------------------------------------- 4. accumulation
def test_accumulation_over_windows_and_calls():
    eng, gid = _engine("novaseq")
    L = eng.read_length
    eng.generate(gid, 333, first_ordinal=FIRST_ORDINAL, seed=SEED)
    rows = eng.mutations()
    two = _tally(eng, [(0, 100), (100, 233)])
    _assert_equal(two, E.errors_host(rows, 0, 333, L), L)  # (the per-read work array is cleared for every call)
    buf, exp = _buffer(L, shift=8), []
    for seed, n in ((3, 200), (4, 65), (5, 333)):
        eng.generate(gid, n, first_ordinal=2, seed=seed)
        eng.error_tally(0, n, buf.ptr)
        exp.append(E.errors_host(eng.mutations(), 0, n, L))
    eng.synchronize()
    assert buf.guards_intact()
    _assert_equal(buf.value(), E.merge(exp), L)
    assert E.split(buf.value(), L)["pairs"][0] == 598


# ---------------------------------------------------------------------------------------------------- 5. launch geometry
@pytest.mark.parametrize("name", ["miseq", "basic33"])
def test_launch_geometry(name, monkeypatch):
    """ISS_ERRTALLY_WGS: the slot chunks per position tile -- one workgroup walks every slot, and many walk a few each."""
    eng, gid = _engine(name)
    L = eng.read_length
    eng.generate(gid, 333, first_ordinal=FIRST_ORDINAL, seed=SEED)
    exp = E.errors_host(eng.mutations(), 7, 300, L)
    monkeypatch.delenv("ISS_ERRTALLY_WGS", raising=False)
    _assert_equal(_tally(eng, [(7, 300)]), exp, L)
    for wgs in ("1", "2", "3", "64", "1000"):
        monkeypatch.setenv("ISS_ERRTALLY_WGS", wgs)
        _assert_equal(_tally(eng, [(7, 300)]), exp, L)


# ---------------------------------------------------------------------------------------------------- 6. overflow
def test_slot_buffer_overflow_is_counted_and_nothing_else():
    from insilicoseq_amd._native import E_NOMEM, EngineError
    from insilicoseq_amd.engine import ReadEngine

    n = 3000
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        L = eng.read_length
        gid = eng.add_genome(random_genome(560, 60000))
        eng.mutations_reserve(SLOTS)
        eng.generate(gid, n, seed=5)
        good = E.errors_host(eng.mutations(), 0, n, L)
        buf = _buffer(L)
        _assert_equal(_tally(eng, [(0, n)], buf=buf), good, L)
        eng.mutations_reserve(256)
        eng.generate(gid, n, seed=5)
        got = _tally(eng, [(0, n)], buf=buf)
        with pytest.raises(EngineError) as e:  # (the host route says the same, behind its wait)
            eng.mutations()
        assert e.value.code == E_NOMEM
        exp = good.copy()
        exp[0] = 1
        _assert_equal(got, exp, L)  # dropped == 1, every other word unchanged
        eng.mutations_reserve(SLOTS)
        eng.generate(gid, n, seed=5)
        exp = 2 * good
        exp[0] = 1
        _assert_equal(_tally(eng, [(0, n)], buf=buf), exp, L)  # a following good call still tallies


# ---------------------------------------------------------------------------------------------------- 7. MT rows
@pytest.mark.parametrize("indel", [None, (0.01, 0.03)], ids=["novaseq", "indel_heavy"])
def test_mt_rows(indel):
    from insilicoseq_amd.engine import ReadEngine

    n = 300
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq", indel))
        L = eng.read_length
        gid = eng.add_genome(random_genome(91, 20000))
        eng.reserve(n + 10)
        eng.seed_mt(17)
        eng.mt_mutations_reserve(64 * n)
        assert eng.generate_mt(gid, n, out_first_pair=4) == n
        rows = eng.mt_mutations()
        assert len(rows) > 50 and (indel is None or ((rows["type"] == 1).any() and (rows["type"] == 2).any()))
        _assert_equal(_tally(eng, [(4, n)], source="mt"), E.errors_host(rows, 0, n, L), L)
        _assert_equal(_tally(eng, [(0, n + 10)], source="mt"), E.errors_host(rows, -4, n + 10, L), L)
        _assert_equal(_tally(eng, [(4 + 50, 100)], source="mt"), E.errors_host(rows, 50, 100, L), L)


# ---------------------------------------------------------------------------------------------------- 8. stream order
def test_generation_into_the_same_rows_right_behind_the_call():
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import default_mutation_slots

    dense = dense_model("novaseq")
    n = 1 << 16
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        L = eng.read_length
        gid = eng.add_genome(random_genome(111, 200000))
        eng.mutations_reserve(default_mutation_slots(dense, n, torch.cuda.get_device_properties(0).multi_processor_count))
        eng.generate(gid, n, seed=1)
        exp = E.errors_host(eng.mutations(), 0, n, L)
        eng.generate(gid, n, seed=9)  # (other rows in between)
        buf = _buffer(L)
        eng.generate(gid, n, seed=1)
        eng.error_tally(0, n, buf.ptr)
        eng.generate(gid, n, seed=2)  # the rows and the row slots are written anew right behind the tally
        eng.synchronize()
        _assert_equal(buf.value(), exp, L)
        assert buf.guards_intact()


# ---------------------------------------------------------------------------------------------------- 9. errors
def test_errors_launch_nothing():
    from insilicoseq_amd._native import E_INVALID, EngineError
    from insilicoseq_amd.engine import ReadEngine

    with ReadEngine(0) as eng:
        with pytest.raises(EngineError) as e:  # no model
            eng.error_tally_words()
        assert e.value.code == E_INVALID
        eng.load_model(dense_model("basic"))
        L = eng.read_length
        buf = _buffer(L)
        zero = buf.buf.cpu().numpy().copy()
        gid = eng.add_genome(random_genome(590, 5000))

        def refused(first=0, n=4, ptr=buf.ptr, source="philox"):
            with pytest.raises(EngineError) as e:
                eng.error_tally(first, n, ptr, source=source)
            assert e.value.code == E_INVALID

        eng.generate(gid, 16, seed=1)
        refused()                      # no reservation
        refused(source="mt")
        eng.mutations_reserve(100000)
        refused()                      # no generate call under the reservation
        eng.generate(gid, 16, seed=1)
        refused(source="mt")           # rows of the other source only
        refused(first=15, n=2)         # a window outside the reserved rows
        refused(first=-1, n=2)
        refused(n=-1)
        refused(ptr=None)              # d_tally NULL with pairs
        with pytest.raises(EngineError) as e:
            eng._check(eng._lib.iss_mutations_tally(eng._ctx, 2, 0, 4, buf.ptr))  # an unknown source
        assert e.value.code == E_INVALID
        eng.error_tally(0, 0, buf.ptr)  # no pairs: fine, nothing added
        eng.error_tally(16, 0, None)
        eng.mt_mutations_reserve(4096)
        refused(source="mt")           # no generate_mt call under the reservation
        eng.synchronize()
        assert np.array_equal(buf.buf.cpu().numpy(), zero)
        eng.error_tally(0, 4, buf.ptr)  # (and the same call, complete, works)
        eng.synchronize()
        assert E.split(buf.value(), L)["pairs"][0] == 4
        eng.mutations_reserve(0)
        refused()                      # the reservation given up


# ---------------------------------------------------------------------------------------------------- 10. the tensor stream
WORK = [(0, 300), (1, 50), (2, 0), (0, 57), (2, 343)]  # record 1 is shorter than a read: skipped, 700 pairs remain


def test_stream_error_tally_does_not_depend_on_batch_pairs():
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import ReadTensorStream

    dense = dense_model("novaseq")
    L = dense.read_length
    recs = [mixed_genome(101, 6000), random_genome(102, 120), random_genome(103, 9000)]
    with ReadEngine(0) as eng:  # the whole list as one call
        eng.load_model(dense)
        gids = [eng.add_genome(recs[0]), eng.add_genome(recs[2])]
        eng.mutations_reserve(SLOTS)
        eng.generate_batch([gids[0], gids[0], gids[1]], [300, 57, 343], first_ordinal=0, seed=77)
        exp = E.errors_host(eng.mutations(), 0, 700, L)
    assert E.split(exp, L)["sub_q"].sum() > 100
    for batch_pairs, truth in ((1, False), (64, True), (333, False), (4096, True)):
        with ReadTensorStream(recs, dense, WORK, batch_pairs, seed=77, truth=truth, error_tally=True) as stream:
            assert stream.error_tally.dtype == torch.int64 and stream.error_tally.device == torch.device("cuda", 0)
            assert stream.engine.mutations_capacity == stream.mutation_slots > 0
            batches = list(stream)
            got = stream.error_tally.cpu().numpy().view(np.uint64)  # (the copy is ordered behind the tallies on the stream)
        assert all((b.truth is not None) == truth for b in batches)
        _assert_equal(got, exp, L)
    with ReadTensorStream(recs, dense, WORK, 400, seed=77) as plain:
        assert plain.error_tally is None and plain.mutation_slots == 0 and len(list(plain)) == 2


def test_stream_overflow_rule_covers_the_error_tally():
    from insilicoseq_amd._native import E_NOMEM, EngineError
    from insilicoseq_amd.tensors import ReadTensorStream

    with ReadTensorStream([random_genome(560, 60000)], dense_model("novaseq"), [(0, 3000)], 1000, seed=5, error_tally=True,
                          mutation_slots=256) as stream:
        with pytest.raises(EngineError) as e:
            for _ in stream:
                pass
        assert e.value.code == E_NOMEM and "mutation_slots=256" in str(e.value) and "batch 0" in str(e.value)
        t = E.split(stream.error_tally.cpu().numpy().view(np.uint64), 151)
        assert t["dropped"][0] >= 1 and t["pairs"][0] == 0 and t["sub_q"].sum() == 0


# ---------------------------------------------------------------------------------------------------- 11. the command line
def _vcf_rows(path):
    """The .vcf as iss_mutation rows: pairs numbered across records and workers (every read of the run its own pair), phred
    and position from the text."""
    from insilicoseq_amd.engine import MUT_DTYPE

    pairs, items = {}, []
    for line in open(path):
        if line.startswith("#"):
            continue
        name, pos, _dot, ref, alt, qual = line.rstrip("\n").split("\t")[:6]
        read, mate = name.rsplit("/", 1)
        pair = pairs.setdefault(read, len(pairs))
        typ = 2 if alt == "." else 1 if len(alt) == 2 else 0
        items.append((pair, int(mate) - 1, typ, int(pos) - 1, ord(ref), ord(alt[-1]), int(qual) if typ == 0 else -1))
    return np.array(items, dtype=MUT_DTYPE)


@pytest.mark.parametrize("rng", ["philox", "mt"])
@pytest.mark.parametrize("workers", [["--gpus", "1"], ["--gpus", "2", "--devices", "1"]], ids=["one_worker", "two_workers"])
def test_generate_error_report(tmp_path, workers, rng):
    from insilicoseq_amd.tally import split_tally

    fasta = str(tmp_path / "genomes.fasta")
    with open(fasta, "w") as fh:
        for k in range(3):
            fh.write(">rec%d\n%s\n" % (k, mixed_genome(121 + k, 5000 + 1000 * k)))
    outs = {}
    for tag, extra in (("errors", ["--error_report"]), ("plain", [])):
        out = str(tmp_path / tag)
        subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n",
                        "2000", "--seed", "5", "--rng", rng, "--store_mutations", "--report", "--output", out] + workers + extra,
                       cwd=ROOT, check=True, timeout=600)
        outs[tag] = out
    for suffix in ("_R1.fastq", "_R2.fastq", ".vcf", "_report.json"):  # byte for byte what the command writes without the flag
        assert open(outs["errors"] + suffix, "rb").read() == open(outs["plain"] + suffix, "rb").read(), suffix
    assert not os.path.exists(outs["plain"] + "_errtally.npy") and not os.path.exists(outs["plain"] + "_errors.json")
    assert not [f for f in os.listdir(str(tmp_path)) if ".iss.tmp." in f]
    words = np.load(outs["errors"] + "_errtally.npy")
    assert words.dtype == np.uint64
    rows = _vcf_rows(outs["errors"] + ".vcf")
    n_pairs = open(outs["errors"] + "_R1.fastq", "rb").read().count(b"\n") // 4
    assert len(rows) > 100 and n_pairs == 1000
    exp = E.split(E.errors_host(rows, 0, n_pairs, 151), 151)
    got = E.split(words, 151)
    assert got["pairs"][0] == n_pairs and got["dropped"][0] == 0
    for name in ("sub_q", "sub_mat", "ins", "del"):
        assert np.array_equal(got[name], exp[name]), name
    # (a read without a row has no line: the histograms of the text's reads agree from bin 1 on, bin 0 holds the rest)
    assert np.array_equal(got["per_read"][:, :, 1:], exp["per_read"][:, :, 1:])
    assert (got["per_read"].sum(axis=2) == n_pairs).all()
    report = json.load(open(outs["errors"] + "_errors.json"))
    assert report["pairs"] == n_pairs and report["read_length"] == 151 and report["dropped"] == 0
    qual = split_tally(np.load(outs["errors"] + "_tally.npy"), 151)["qual"]
    for m in range(2):
        bases = qual[m].sum(axis=0)
        assert [(e["phred"], e["bases"]) for e in report["calibration"][m]] == [(q, int(bases[q])) for q in range(94) if bases[q]]
        assert sum(e["substitutions"] for e in report["calibration"][m]) == int(got["sub_q"][m].sum())


def test_generate_error_report_needs_store_mutations(tmp_path):
    res = subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--genomes", str(tmp_path / "none.fasta"), "--model", "novaseq",
                          "--error_report", "--output", str(tmp_path / "out")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and len(res.stderr.strip().splitlines()) == 1 and "--store_mutations" in res.stderr
    assert os.listdir(str(tmp_path)) == []
