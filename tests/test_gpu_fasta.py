"""`generate --device_fasta` on the GPU (iss_fa_index, iss_genome_upload_fasta; k_fa_* of csrc/iss_fasta.hip.h).

The index: the device's table equals the numpy twin's row for row on the hand cases, on texts sized by the kernels' tile and the
scan's span, and on random files.  The upload: the resident letters equal the host parser's byte for byte, through the group route
and the owned route; a bad letter costs its record alone; a refused table launches nothing and leaves the context working.  Rows cut
from a device-FASTA genome equal rows cut from the host's letters.  The whole command writes the same files with and without the
flag, from plain, gzip and BGZF inputs.  A GenomeStore that has to drop brings its records back the same way."""
import gzip
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import fasta_cases as FC
from helpers import dense_model, mixed_genome, random_genome
from insilicoseq_amd import fasta as F
from insilicoseq_amd.generator import SMALL_RECORD, GenomeStore, body_letters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = set(b"ACGTYRWSKMNBVDHacgtyrwskmnbvdh")
KEYS = ("r1_base", "r1_qual", "r2_base", "r2_qual")


@pytest.fixture(scope="module")
def geometry():
    from insilicoseq_amd import _native

    lib = _native.lib()
    return lib.iss_fasta_tile(), lib.iss_fasta_scan_span()


@pytest.fixture(scope="module")
def sized(geometry):
    return FC.sized(*geometry)


@pytest.fixture(scope="module")
def indexer():
    with F.FastaIndexer(0) as fa:
        yield fa


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        yield eng


def rows_of(index):
    return [tuple(int(x) for x in row) for row in zip(*index)]


# ---------------------------------------------------------------------- 1. the index
def test_index_hand_cases(indexer):
    for name, data in sorted(FC.HAND.items()):
        assert rows_of(indexer.index(data)) == rows_of(F.index_host(data)), name


def test_index_sized_texts(indexer, sized, geometry):
    T, S = geometry
    assert {len(sized["scan_span_%d" % n]) for n in (S * T - 1, S * T, S * T + 1)} == {S * T - 1, S * T, S * T + 1}
    for name, data in sorted(sized.items()):
        want = F.index_host(data)
        assert rows_of(indexer.index(data)) == rows_of(want), name
        if name.startswith("scan_span"):  # the header in the last tile, behind the scan's first pass
            assert int(want.header_off[-1]) // T >= S - 1 and len(want.letters) == 3
    heads = {name: F.index_host(sized[name]).header_off.tolist() for name in ("header_at_%d" % (T - 1), "header_at_%d" % T)}
    assert heads["header_at_%d" % (T - 1)][1] == T - 1 and heads["header_at_%d" % T][1] == T


def test_index_random_files(indexer):
    for seed in range(1000, 1100):
        data = FC.random_file(seed)
        assert rows_of(indexer.index(data)) == rows_of(F.index_host(data)), seed


def test_index_more_records_than_the_first_call_has_room_for(indexer, monkeypatch):
    monkeypatch.setattr(F, "FIRST_CAPACITY", 3)
    data = FC.HAND["four_tiny_records_in_16_bytes"] * 3
    assert rows_of(indexer.index(data)) == rows_of(F.index_host(data)) and len(F.index_host(data).letters) == 12


# ---------------------------------------------------------------------- 2. the upload
def _source(data):
    return types.SimpleNamespace(array=np.frombuffer(data, dtype=np.uint8))


def _upload_and_compare(eng, data, name):
    """Every record of ``data`` that stays in the file, uploaded as it stands there: its resident letters are the host parser's,
    and it has no id exactly when it has no letters or one outside the alphabet."""
    eng.clear_genomes()
    index = F.index_host(data)
    seqs = [r.seq for r in F.records_of(_source(data), index) if not isinstance(r.seq, str)]
    gids = eng.add_genomes_fasta(seqs)
    assert len(gids) == len(seqs)
    for seq, gid in zip(seqs, gids):
        want = body_letters(bytes(seq.raw())).encode()
        assert len(want) == len(seq)
        if not want or not set(want) <= ALPHABET:
            assert gid == -1, name
        else:
            assert gid >= 0 and eng.genome_letters(gid).tobytes() == want, name
    return gids


def test_upload_hand_cases(engine):
    taken = 0
    for name, data in sorted(FC.HAND.items()):
        taken += sum(g >= 0 for g in _upload_and_compare(engine, data, name))
    assert taken >= 20


def test_upload_sized_texts(engine, sized):
    for name, data in sorted(sized.items()):
        gids = _upload_and_compare(engine, data, name)
        assert all(g >= 0 for g in gids), name  # (the sized texts hold plain letters only; the scan-span ones a record above SMALL_RECORD)


def _fasta_of(seqs, width=60, eol=b"\n"):
    return b"".join(b">s%d\n" % k + FC.wrapped(s.encode(), width + k % 7, b"\r\n" if k % 3 == 1 else eol) for k, s in enumerate(seqs))


def test_upload_group_of_50_and_a_record_above_small_record(engine):
    small = [mixed_genome(50 + k, 200 + 37 * k) if k % 5 == 2 else random_genome(50 + k, 200 + 37 * k) for k in range(50)]
    gids = _upload_and_compare(engine, _fasta_of(small), "group of 50")
    assert gids == list(range(50))
    big = random_genome(9, SMALL_RECORD + 1)
    gids = _upload_and_compare(engine, _fasta_of([big], 70), "owned")
    assert gids == [0] and engine.genome_length(0) == SMALL_RECORD + 1
    # a large record between small ones: it goes alone, the others in their groups, all in one call of the engine
    gids = _upload_and_compare(engine, _fasta_of(small[:3] + [big] + small[3:6]), "mixed")
    assert sorted(gids) == list(range(7))


def test_bad_letter_costs_its_record_alone(engine):
    seqs = [random_genome(70 + k, 500 + k) for k in range(6)]
    seqs[2] = seqs[2][:100] + "X" + seqs[2][101:]
    engine.clear_genomes()
    data = _fasta_of(seqs)
    got = engine.add_genomes_fasta([r.seq for r in F.records_of(_source(data), F.index_host(data))])
    assert got == [0, 1, -1, 2, 3, 4]
    for k, gid in enumerate(got):
        if gid >= 0:
            assert engine.genome_letters(gid).tobytes().decode() == seqs[k]


def _rows(eng, n):
    eng.synchronize()
    got = eng.download(0, n)
    return {k: got[k].copy() for k in KEYS}


def test_refused_tables_launch_nothing_and_the_context_goes_on(engine):
    from insilicoseq_amd._native import E_INVALID, EngineError

    engine.clear_genomes()
    genome = random_genome(3, 4000)
    data = _fasta_of([genome, genome[:900]])
    index = F.index_host(data)
    off, length, letters = index.body_off.tolist(), index.body_len.tolist(), index.letters.tolist()
    span = np.frombuffer(data, np.uint8)
    for what, table in (("a range past the span", ([off[0], off[1]], [length[0], length[1] + 1], letters)),
                        ("overlapping bodies", ([off[0], off[0] + 10], length, letters)),
                        ("letters too large", (off, length, [letters[0], length[1] + 1])),
                        ("a large record not alone", ([0, 10], [5, len(data) - 10], [5, SMALL_RECORD + 1]))):
        with pytest.raises(EngineError) as e:
            engine.add_genomes_fasta_table(span, *table)
        assert e.value.code == E_INVALID, what
    # a table that passes the check but counts the letters wrongly: nothing is written outside the records' places, the call fails
    with pytest.raises(EngineError) as e:
        engine.add_genomes_fasta_table(span, off, length, [letters[0] - 5, letters[1]])
    assert e.value.code == E_INVALID and "does not fit" in e.value.message
    gids = engine.add_genomes_fasta_table(span, off, length, letters)
    assert gids == [0, 1] and engine.genome_letters(0).tobytes().decode() == genome
    engine.generate(gids[0], 512, first_ordinal=0, seed=11)
    a = _rows(engine, 512)
    engine.generate(engine.add_genome(genome), 512, first_ordinal=0, seed=11)
    b = _rows(engine, 512)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------- 3. rows
@pytest.mark.parametrize("kind", ["philox_plain", "philox_iupac_lower", "mt"])
def test_rows_equal_those_of_the_host_letters(engine, kind):
    n = 2048
    genome = mixed_genome(21, 30011) if kind == "philox_iupac_lower" else random_genome(20, 30011)
    other = random_genome(22, 777)
    data = _fasta_of([other, genome], 61, b"\r\n")
    engine.clear_genomes()
    gid_device = engine.add_genomes_fasta([r.seq for r in F.records_of(_source(data), F.index_host(data))])[1]
    gid_host = engine.add_genome(genome)
    out = []
    for gid in (gid_device, gid_host):
        if kind == "mt":
            engine.seed_mt(77)
            assert engine.generate_mt(gid, n) == n
        else:
            engine.generate(gid, n, first_ordinal=5, seed=9)
        out.append(_rows(engine, n))
    for k in KEYS:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert len(set(out[0]["r1_base"].tobytes())) >= 4


# ---------------------------------------------------------------------- 4. the whole command
def _five_records():
    seqs = [random_genome(31, 4000), mixed_genome(32, 6500), random_genome(33, 3001), random_genome(34, 9000), mixed_genome(35, 5000)]
    parts = []
    for k, s in enumerate(seqs):
        eol = b"\r\n" if k % 2 else b"\n"
        parts.append(b">rec%d some text%s" % (k, eol) + (b"\n" if k == 1 else b"") + FC.wrapped(s.encode(), 60 + k, eol) + (eol if k == 3 else b""))
    return parts


def _generate(cwd, args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("ISS_DEVICE_FASTA", None)
    r = subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--model", "novaseq", "--seed", "5", "-n", "2000"] + args,
                       cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]


def _files(cwd, prefix):
    out = {name[len(prefix):]: (cwd / name).read_bytes() for name in sorted(os.listdir(str(cwd))) if name.startswith(prefix + "_")}
    assert "_R1.fastq" in out and len(out["_R1.fastq"]) > 100000 and not any(".iss.tmp" in name for name in out)
    return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_cmd")
    parts = _five_records()
    (d / "g.fa").write_bytes(b"".join(parts))
    (d / "g1.fa.gz").write_bytes(gzip.compress(b"".join(parts[:2])))  # two containers in one command: gzip, then BGZF
    (d / "g2.fa.gz").write_bytes(FC.bgzf(b"".join(parts[2:]), 3000))
    return d


@pytest.fixture(scope="module")
def philox_plain(inputs):
    _generate(inputs, ["--genomes", "g.fa", "-o", "plain"])
    return _files(inputs, "plain")


@pytest.mark.parametrize("name,args", [("philox", ["--genomes", "g.fa"]), ("mt", ["--genomes", "g.fa", "--rng", "mt"]),
                                       ("mt3", ["--genomes", "g.fa", "--rng", "mt", "--cpus", "3", "--devices", "1"]),
                                       ("draft", ["--draft", "g.fa"])])
def test_command_writes_the_same_files(inputs, philox_plain, name, args):
    if name == "philox":
        want = philox_plain
    else:
        _generate(inputs, args + ["-o", name + "_host"])
        want = _files(inputs, name + "_host")
    _generate(inputs, args + ["-o", name + "_dev", "--device_fasta"])
    assert _files(inputs, name + "_dev") == want


@pytest.mark.parametrize("flag", [[], ["--device_fasta"]])
def test_command_takes_gzip_and_bgzf_inputs(inputs, philox_plain, flag):
    prefix = "gz_dev" if flag else "gz_host"
    _generate(inputs, ["--genomes", "g1.fa.gz", "g2.fa.gz", "-o", prefix] + flag)
    assert _files(inputs, prefix) == philox_plain


def test_load_genomes_leaves_the_letters_in_the_file(tmp_path):
    """What the flag switches on in the command: the records of load_genomes are places in the concatenated file."""
    from insilicoseq_amd import drafts
    from insilicoseq_amd.generator import parse_fasta

    parts = _five_records()
    (tmp_path / "a.fa").write_bytes(b"".join(parts[:2]))
    (tmp_path / "b.fa.gz").write_bytes(FC.bgzf(b"".join(parts[2:]), 3000))  # (inflated on the device: the flag asks for it)
    genome_file, records = drafts.load_genomes([str(tmp_path / "a.fa"), str(tmp_path / "b.fa.gz")], None, str(tmp_path / "o"), None,
                                               device_fasta=True)
    assert open(genome_file, "rb").read() == b"".join(parts)
    assert len(records) == 5 and all(isinstance(r.seq, F.FastaSeq) for r in records)
    want = list(parse_fasta(genome_file))
    assert [(r.id, r.description, len(r.seq), str(r.seq)) for r in records] == [(r.id, r.description, len(r.seq), r.seq) for r in want]
    genome_file, kept = drafts.load_genomes([str(tmp_path / "a.fa"), str(tmp_path / "b.fa.gz")], None, str(tmp_path / "u"), 3, device_fasta=True)
    assert len(kept) == 3 and all(isinstance(r.seq, F.FastaSeq) for r in kept)  # (--n_genomes: the file written anew, read again)
    assert {(r.id, str(r.seq)) for r in kept} <= {(r.id, r.seq) for r in want}


# ---------------------------------------------------------------------- 5. drop, then the same way back
class _Limits(object):
    GROUP_BASES = 1 << 29

    def __init__(self, budget):
        self.GENOME_BUDGET = budget


def test_a_store_that_drops_uploads_its_records_again(engine, tmp_path):
    seqs = [random_genome(41, 5000), mixed_genome(42, 5200), random_genome(43, 4800)]
    path = str(tmp_path / "three.fa")
    with open(path, "wb") as fh:
        fh.write(_fasta_of(seqs, 50, b"\r\n"))
    records = F.read(path, device=0)
    assert all(isinstance(r.seq, F.FastaSeq) for r in records) and [len(r.seq) for r in records] == [len(s) for s in seqs]
    visits = [0, 1, 2, 0, 2, 1]
    out = {}
    for budget in (10500, 1 << 30):  # two records fit / all three do
        engine.clear_genomes()
        store = GenomeStore(engine, _Limits(budget), budget_divisor=1, drop_on_upload=True, skip_short=True)
        store.plan([records[v] for v in visits])
        rows, uploads = [], 0
        for step, v in enumerate(visits):
            before = store._hit(records[v]) is None
            gid = store.gid(records[v])
            uploads += before
            assert engine.genome_letters(gid).tobytes().decode() == seqs[v]
            engine.generate(gid, 300, first_ordinal=300 * step, seed=3)
            rows.append(_rows(engine, 300))
        out[budget] = rows, uploads
    assert out[10500][1] > out[1 << 30][1]  # (the small budget dropped and uploaded again)
    for a, b in zip(out[10500][0], out[1 << 30][0]):
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k
