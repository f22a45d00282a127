"""`generate --origins` on the device (iss_origins_emit_batch) against the twin insilicoseq_amd.origins.lines_host, byte for byte.

The bytes a call appends must be lines_host(coordinates of the same rows): the record of every pair, its two clamped template
intervals, the name, the insert size.  The twin itself is held to the definition without a GPU (tests/test_origins_host.py).  The
command line is checked against the reads: in perfect mode R1 is seq[s1:e1] and R2 the reverse complement of seq[s2:e2], and the
depth rebuilt from the file is the depth `--depth` reports."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import helpers as H
from insilicoseq_amd import depth as D
from insilicoseq_amd import origins as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {125: "basic", 301: "miseq"}
ROWS = 400  # rows generated per setting (the largest case takes 333)
FRONT = b"in front\n"


class Rows(object):
    """One engine with ``rows`` generated rows on one record and their coordinates (left unchanged: every case's reference)."""

    def __init__(self, model, length=20000, rows=ROWS, seed=77, mt=False, **kw):
        from insilicoseq_amd.engine import ReadEngine

        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(H.dense_model(model))
            self.RL, self.length, self.n, self.seed, self.kw = eng.read_length, length, rows, seed, dict(kw)
            self.genome = H.random_genome(700 + self.RL, length)
            self.gid = eng.add_genome(self.genome)
            fragment = self.kw.pop("fragment", None)
            eng.generate(self.gid, rows, first_ordinal=900, seed=99)  # (rows of another seed underneath)
            if fragment is not None:
                eng.set_fragment(*fragment)
            if mt:
                eng.seed_mt(17)
                assert eng.generate_mt(self.gid, rows) == rows
            else:
                self.generate(seed)
            eng.synchronize()
            self.coords = eng.coords(0, rows).copy()
        except Exception:
            eng.close()
            raise

    def generate(self, seed):
        self.eng.generate(self.gid, self.n, first_ordinal=3, seed=seed, **self.kw)


@pytest.fixture(scope="module")
def rows():
    made = {}

    def get(model, **kw):
        key = (model,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = Rows(model, **kw)
        return made[key]

    yield get
    for r in made.values():
        r.eng.close()


def emit_file(eng, calls, cpu, path, between=None):
    """Some bytes, every call's (items, record lengths) through ReadEngine.origins_emit_batch, one flush -> the appended bytes.
    between(k): called behind emit call k, before the flush."""
    with open(path, "wb") as fh:
        fh.write(FRONT)
        fh.flush()
        for k, (items, lengths) in enumerate(calls):
            eng.origins_emit_batch(fh.fileno(), items, lengths, cpu)
            if between:
                between(k)
        eng.origins_flush()
        assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(path)  # (the descriptor stands at the end)
    data = open(path, "rb").read()
    assert data[:len(FRONT)] == FRONT
    return data[len(FRONT):]


def twin(calls, cpu, coords, RL):
    """lines_host over the calls: coords[row] is the coordinate row of output row ``row``."""
    return b"".join(G.lines_host(items, lengths, cpu, np.concatenate([coords[row:row + n] for _r, _i, row, n in items] +
                                                                     [np.zeros((0, 4), dtype=np.int64)]), RL)
                    for items, lengths in calls)


def check(eng, calls, cpu, coords, RL, path, between=None):
    got = emit_file(eng, calls, cpu, path, between)
    want = twin(calls, cpu, coords, RL)
    print("RL %d, %d calls, %d pairs: device %d bytes, twin %d" % (RL, len(calls), sum(it[3] for c in calls for it in c[0]), len(got), len(want)))
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("the device's text is not the twin's: %d bytes against %d, first difference at byte %d (line %d): %r against %r"
                             % (len(got), len(want), k, want[:k].count(b"\n"), got[max(k - 20, 0):k + 40], want[max(k - 20, 0):k + 40]))
    return got


# ---------------------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize("RL", sorted(MODELS))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 333])
def test_shapes(rows, tmp_path, RL, n):
    """One item from row 5 on: one lane, a wavefront less one, a wavefront, one more, more than a workgroup's 256 lanes."""
    r = rows(MODELS[RL])
    assert r.RL == RL
    got = check(r.eng, [([("NZ_CP012345.1", 0, 5, n)], [r.length])], 2, r.coords, RL, tmp_path / "shape.bedpe")
    assert got.count(b"\n") == n
    f = got.split(b"\n")[0].split(b"\t")  # RL matters only through fs + RL
    assert int(f[2]) - int(f[1]) == RL and int(f[5]) - int(f[4]) == RL and f[6] == b"NZ_CP012345.1_0_2"


@pytest.mark.parametrize("cpu", [0, 123])
def test_items(tmp_path, cpu):
    """generate_batch over three records of different lengths (the descriptors carry arena coordinates, the later records' offsets
    are not zero): ids of 1, 17 and 200 characters, a zero-pair item between two others, pair numbers whose digit count changes
    inside an item, items that take only some of the call's rows, and a batch with an item of no pairs."""
    from insilicoseq_amd.engine import ReadEngine

    lengths = [3000, 1000, 2000]
    seqs = [H.random_genome(40 + k, n) for k, n in enumerate(lengths)]
    with ReadEngine(0) as eng:
        eng.load_model(H.dense_model("novaseq"))
        gids = eng.add_genomes(seqs)
        gids = [g if g >= 0 else eng.add_genome(s) for g, s in zip(gids, seqs)]
        eng.reserve(160)
        eng.generate(gids[0], 160, seed=3)  # (every row holds something)
        eng.generate_batch(gids, [40, 25, 60], first_ordinal=11, seed=5, out_first_pair=4)
        eng.synchronize()
        coords = np.zeros((160, 4), dtype=np.int64)
        coords[4:129] = eng.coords(4, 125)
        assert (coords[4:129, 0] >= 0).all() and (coords[44:69, 2] <= 1000).all() and (coords[69:129, 2] <= 2000).all()
        whole = ([("a", 7, 4, 40), ("zero", 3, 44, 0), ("b" * 17, 95, 44, 25), ("c" * 200, 0, 69, 60)], [3000, 1000, 1000, 2000])
        some = ([("a", 0, 10, 20), ("c" * 200, 99990, 100, 29)], [3000, 2000])
        check(eng, [whole, some], cpu, coords, 151, tmp_path / "items.bedpe")
        eng.generate_batch(gids, [40, 0, 60], first_ordinal=500, seed=6, out_first_pair=0)
        eng.synchronize()
        coords = eng.coords(0, 100)
        assert (coords[40:, 2] <= 2000).all()
        calls = [([("a", 0, 0, 40), ("zero", 0, 40, 0), ("c", 5, 40, 60)], [3000, 1000, 2000])]
        check(eng, calls, cpu, coords, 151, tmp_path / "items2.bedpe")


def test_tiles(rows, tmp_path, monkeypatch):
    """ISS_ORIGINS_TILE 1, 3 and 64 at 65 pairs: a tile's last line, a last tile of one or two lines, and spans that start at
    every alignment mod 16 (the text buffer is 256-byte aligned: a tile's first address mod 16 is its first line's offset mod 16)."""
    r = rows("basic")
    call = ([("x" * 17, 95, 7, 65)], [r.length])
    want = twin([call], 3, r.coords, r.RL)
    starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in want.split(b"\n")[:-1]])])
    seen = set()
    for tile in (1, 3, 64):
        monkeypatch.setenv("ISS_ORIGINS_TILE", str(tile))
        assert check(r.eng, [call], 3, r.coords, r.RL, tmp_path / ("tile%d.bedpe" % tile)) == want
        seen |= set(int(starts[t0]) % 16 for t0 in range(0, 65, tile))
    assert len(seen) >= 8 and len(set(int(s) % 16 for s in starts[:65])) >= 8, sorted(seen)
    monkeypatch.delenv("ISS_ORIGINS_TILE")
    assert check(r.eng, [call], 3, r.coords, r.RL, tmp_path / "default.bedpe") == want


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_scan_boundaries(rows, tmp_path, n):
    """VSCAN_TILE - 1, VSCAN_TILE, VSCAN_TILE + 1 and twice + 1 pairs on a 2 000-base record."""
    r = rows("novaseq", length=2000, rows=4097)
    got = check(r.eng, [([("rec", 0, 0, n)], [2000])], 0, r.coords, 151, tmp_path / "scan.bedpe")
    assert got.count(b"\n") == n


def test_mt_rows(rows, tmp_path):
    r = rows("hiseq", length=5000, rows=64, mt=True)
    check(r.eng, [([("mt", 0, 0, 64)], [5000])], 1, r.coords, r.RL, tmp_path / "mt.bedpe")


def test_amplicon_and_gc_bias(rows, tmp_path):
    """Amplicon: the template is the whole record -- s1 = 0 and e2 = len stand in the file.  gc_bias: redrawn pairs."""
    r = rows("novaseq", length=1000, sequence_type="amplicon")
    got = check(r.eng, [([("amp", 0, 0, 100)], [1000])], 0, r.coords, 151, tmp_path / "amp.bedpe")
    fields = [x.split(b"\t") for x in got.split(b"\n")[:-1]]
    assert any(f[1] == b"0" for f in fields) and any(f[5] == b"1000" for f in fields)
    r = rows("novaseq", gc_bias=True)
    check(r.eng, [([("gc", 0, 3, 200)], [r.length])], 0, r.coords, 151, tmp_path / "gc.bedpe")


def test_custom_fragments(rows, tmp_path):
    """Fragments of 300 +- 200 on 700 bases: the clamp bites.  First, with the oracle's coordinates and no GPU in the argument, the
    chosen seed gives a clamped start, an interval that is empty after the clamp and a negative insert size; then the engine's
    coordinates are the oracle's and the file is the twin's, with all three in it."""
    from oracle import oracle as O

    n, seed, length = 333, 1234, 700
    genome = H.random_genome(700 + 151, length)
    res = O.Oracle(H.dense_model("novaseq")).simulate(O.Rng().seed_philox(seed), genome, n, first_ordinal=3, fragment_length=300,
                                                     fragment_sd=200, want_coords=True)
    assert res["status"] == 0 and res["n_done"] == n
    fs, rs, re, isz = res["coords"].T
    assert (rs < 0).any() and (re <= 0).any() and (isz < 0).any() and (fs + 151 > length).any()
    r = rows("novaseq", length=length, rows=n, seed=seed, fragment=(300, 200))
    assert r.genome == genome and np.array_equal(r.coords, res["coords"])
    got = check(r.eng, [([("frag", 0, 0, n)], [length])], 0, r.coords, 151, tmp_path / "frag.bedpe")
    with open(tmp_path / "text.bedpe", "wb") as fh:  # (without the bytes in front)
        fh.write(got)
    p = G.parse(str(tmp_path / "text.bedpe"))
    assert len(p["s2"]) == n and got.startswith(b"frag\t")
    assert (p["s2"][rs < 0] == 0).all() and ((p["e2"] == p["s2"]) & (re <= 0)).any() and (p["isz"] < 0).any()
    assert (p["e1"][fs + 151 > length] == length).all()


def test_slot_reuse(rows, tmp_path):
    """Emit calls back to back (more than the two slots), then one flush; a call of no pairs appends nothing."""
    r = rows("miseq")
    ln = [r.length]
    calls = [([("first", 0, 0, 150)], ln), ([("second_of_four", 998, 150, 3)], ln), ([("none", 0, 0, 0)], ln), ([], []),
             ([("third", 50, 153, 120)], ln), ([("4", 0, 273, 40)], ln)]
    check(r.eng, calls, 2, r.coords, r.RL, tmp_path / "slots.bedpe")


def test_generation_behind_an_emit(rows, tmp_path):
    """The rows are generated anew right behind an emit, twice: the text holds the coordinates downloaded before."""
    r = rows("miseq")

    def regenerate(k):
        r.generate(78 + 2 * k)      # (other rows; no wait on the host: the other set of descriptors, then this one again)
        r.generate(79 + 2 * k)

    try:
        check(r.eng, [([("before", 0, 0, 200)], [r.length])], 1, r.coords, r.RL, tmp_path / "behind.bedpe", between=regenerate)
    finally:
        r.generate(r.seed)  # the module's rows again
        r.eng.synchronize()
        assert np.array_equal(r.eng.coords(0, r.n), r.coords)


def test_errors_launch_nothing(rows, tmp_path):
    from insilicoseq_amd._native import E_INVALID, EngineError

    r = rows("basic")
    ln = r.length
    bad = {
        "rows behind the reserved range": ([("a", 0, 10 ** 9, 5)], [ln]),
        "rows that end behind the reserved range": ([("a", 0, 0, 10 ** 9)], [ln]),
        "a record of no bases": ([("a", 0, 0, 5)], [0]),
        "a record of no bases, item of no pairs": ([("a", 0, 0, 5), ("b", 0, 5, 0)], [ln, 0]),
        "items out of order": ([("a", 0, 10, 5), ("b", 0, 0, 5)], [ln, ln]),
        "items that overlap": ([("a", 0, 0, 10), ("b", 0, 9, 10)], [ln, ln]),
        "a negative pair id": ([("a", -1, 0, 5)], [ln]),
    }
    path = tmp_path / "errors.bedpe"
    with open(path, "wb") as fh:
        fh.write(b"untouched")
        fh.flush()
        for what, (items, lengths) in bad.items():
            with pytest.raises(EngineError) as e:
                r.eng.origins_emit_batch(fh.fileno(), items, lengths, 0)
            assert e.value.code == E_INVALID, what
        with pytest.raises(ValueError):
            r.eng.origins_emit_batch(fh.fileno(), [("a", 0, 0, 5)], [], 0)
        r.eng.origins_flush()
    assert open(path, "rb").read() == b"untouched"
    check(r.eng, [([("fine", 0, 0, 5)], [ln])], 0, r.coords, r.RL, tmp_path / "fine.bedpe")  # (the context still works)


def _text_bound(call, cpu):
    """The bytes iss_origins_emit_batch reserves for a call's text: every pair at the longest line its item can have -- three ids,
    the worker's number, 16 fixed bytes, four coordinates within the record, the item's last pair number, 11 for the insert size."""
    items, lengths = call
    return sum(n * (3 * len(rid) + len(str(cpu)) + 16 + 4 * len(str(ln)) + len(str(first_i + n - 1)) + 11)
               for (rid, first_i, _row, n), ln in zip(items, lengths) if n)


def test_text_buffers_grow_mid_run(rows, tmp_path):
    """One pair, then a call whose bound is past what the first one allocated (bound + bound / 8 + 64 KiB: the id stands three
    times in a line), then a small one; no flush in between, the file stays attached while the buffers are replaced."""
    r = rows("miseq", seed=78)  # (an engine no other case has emitted from: its buffers are the first call's)
    ln = [r.length]
    calls = [([("one", 0, 0, 1)], ln), ([("L" * 300, 7, 1, 333)], ln), ([("small", 0, 334, 20)], ln)]
    first = _text_bound(calls[0], 2)
    allocated = first + first // 8 + (1 << 16)
    assert _text_bound(calls[1], 2) > allocated > _text_bound(calls[2], 2)
    got = check(r.eng, calls, 2, r.coords, r.RL, tmp_path / "grow.bedpe")
    assert len(got) > allocated


def test_a_new_descriptor_without_a_flush(rows, tmp_path):
    """File A, then file B, one flush: the emit to B lands A's text and leaves A's descriptor at A's end; B is appended to where B
    stood, whatever A's offset was."""
    r = rows("miseq")
    ln = [r.length]
    calls = {"a": ([("to_a", 0, 0, 150)], ln), "b": ([("to_b", 5, 150, 90)], ln)}
    front = {"a": b"A: in front\n", "b": b"B: other bytes, and more of them, in front\n"}
    with open(tmp_path / "a.bedpe", "wb") as fa, open(tmp_path / "b.bedpe", "wb") as fb:
        for k, fh in (("a", fa), ("b", fb)):
            fh.write(front[k])
            fh.flush()
            r.eng.origins_emit_batch(fh.fileno(), calls[k][0], calls[k][1], 2)
        r.eng.origins_flush()
        for k, fh in (("a", fa), ("b", fb)):
            assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(str(tmp_path / (k + ".bedpe"))), k
    for k in "ab":
        assert open(tmp_path / (k + ".bedpe"), "rb").read() == front[k] + twin([calls[k]], 2, r.coords, r.RL), k


def test_a_write_error_surfaces_once(rows, tmp_path):
    """A descriptor opened read-only (EBADF on the host, nothing on the device): the next flush raises E_IO "write failed ...",
    the one after returns, the file is as it was and the next emit appends the twin's bytes."""
    from insilicoseq_amd._native import E_IO, EngineError

    r = rows("miseq")
    call = ([("rec", 3, 10, 120)], [r.length])
    path = tmp_path / "readonly.bedpe"
    path.write_bytes(b"read only\n")
    with open(path, "rb") as fh:
        r.eng.origins_emit_batch(fh.fileno(), call[0], call[1], 0)
        with pytest.raises(EngineError) as e:
            r.eng.origins_flush()
        assert e.value.code == E_IO and e.value.message.startswith("write failed"), e.value.message
        r.eng.origins_flush()
    assert path.read_bytes() == b"read only\n"
    check(r.eng, [call], 0, r.coords, r.RL, tmp_path / "good.bedpe")


# ---------------------------------------------------------------------------------------------------- the command line
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
IDS = ["rec0", "rec1", "rec2"]


def _read(path):
    """A file's bytes; `path`.gz gunzipped where `--compress` left that instead."""
    return gzip.open(path + ".gz", "rb").read() if os.path.exists(path + ".gz") else open(path, "rb").read()


def _fastq(path):
    lines = _read(path).split(b"\n")
    return [(h[1:].decode(), s) for h, s in zip(lines[0::4], lines[1::4]) if h]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """`generate -n 2000` over three plain-ACGT records with the given flags -> (output prefix, the records' sequences); every
    command line runs once per module."""
    base = tmp_path_factory.mktemp("origins_cli")
    seqs = [H.random_genome(131 + k, 5000 + 1000 * k) for k in range(3)]
    fasta = str(base / "genomes.fasta")
    with open(fasta, "w") as fh:
        for rid, s in zip(IDS, seqs):
            fh.write(">%s\n%s\n" % (rid, s))
    made = {}

    def run(*flags):
        if flags not in made:
            where = base / ("run%d" % len(made))
            where.mkdir()
            out = str(where / "out")
            subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "-n", "2000", "--output", out]
                           + list(flags), cwd=ROOT, check=True, timeout=600)
            assert not [f for f in os.listdir(str(where)) if ".iss.tmp." in f]
            made[flags] = out
        return made[flags], seqs

    return run


@pytest.mark.parametrize("workers", [("--gpus", "1"), ("--gpus", "2", "--devices", "1")], ids=["one_worker", "two_workers_one_device"])
def test_generate_origins_perfect(cli, workers):
    """The file against the reads, no twin in between: every line's name is the FASTQ's name in order, R1 is seq[s1:e1] and R2 the
    reverse complement of seq[s2:e2]."""
    out, seqs = cli("--seed", "42", "--mode", "perfect", "--origins", *workers)
    p = G.parse(out + G.SUFFIX)
    r1, r2 = _fastq(out + "_R1.fastq"), _fastq(out + "_R2.fastq")
    assert len(r1) == len(r2) == len(p["name"]) == 1000
    assert [n + "/1" for n in p["name"]] == [h for h, _s in r1] and [n + "/2" for n in p["name"]] == [h for h, _s in r2]
    by_id = {rid: s.encode() for rid, s in zip(IDS, seqs)}
    for k in range(1000):
        seq = by_id[p["id"][k]]
        assert p["name"][k].rsplit("_", 2)[0] == p["id"][k]
        assert r1[k][1] == seq[p["s1"][k]:p["e1"][k]], p["name"][k]
        assert r2[k][1] == seq[p["s2"][k]:p["e2"][k]].translate(_COMPLEMENT)[::-1], p["name"][k]
        assert p["isz"][k] == p["s2"][k] - p["e1"][k]
    if len(workers) > 2:
        assert set(n.rsplit("_", 1)[1] for n in p["name"]) == {"0", "1"}


@pytest.mark.parametrize("rng_mode", [("--rng", "philox"), ("--rng", "mt")], ids=["philox", "mt"])
def test_generate_origins_depth(cli, tmp_path, rng_mode):
    """The depth table rebuilt from the BEDPE is the one `--depth` wrote."""
    out, seqs = cli("--seed", "42", "--model", "novaseq", "--origins", "--depth", "--depth_bin", "100", *rng_mode)
    p = G.parse(out + G.SUFFIX)
    assert len(p["name"]) == 1000
    table, n_words = D.depth_table([len(s) for s in seqs])
    coords, item, ids = G.intervals_for_depth(p, ids=IDS)
    diff = D.mark_host(np.zeros(n_words, dtype=np.int32), coords, item, table, 0)
    _depth, stats, bins = D.finish_host(diff, table, 100)
    assert int(stats[:, 0].sum()) == 2000 * 151
    D.write_depth_table(str(tmp_path / "exp.txt"), D.depth_rows(stats, table, IDS))
    D.write_bedgraph(str(tmp_path / "exp.bedgraph"), bins, table, IDS, 100)
    assert open(out + "_depth.txt").read() == open(str(tmp_path / "exp.txt")).read()
    assert open(out + "_depth.bedgraph").read() == open(str(tmp_path / "exp.bedgraph")).read()


def test_flag_neutrality(cli):
    """With and without --origins: the FASTQ and .vcf bytes are the same ones."""
    base = ("--seed", "42", "--model", "novaseq", "--store_mutations")
    plain, _ = cli(*base)
    with_flag, _ = cli(*(base + ("--origins",)))
    for suffix in ("_R1.fastq", "_R2.fastq", ".vcf"):
        assert open(with_flag + suffix, "rb").read() == open(plain + suffix, "rb").read(), suffix
    assert open(plain + ".vcf", "rb").read().count(b"\n") > 2
    assert not os.path.exists(plain + G.SUFFIX) and os.path.getsize(with_flag + G.SUFFIX) > 0
    assert [n + "/1" for n in G.parse(with_flag + G.SUFFIX)["name"]] == [h for h, _s in _fastq(with_flag + "_R1.fastq")]


def test_flag_neutrality_ubam_compress(cli):
    """Beside --ubam --store_mutations --compress --report: the .bam and the .vcf.gz are the same ones, and the .bedpe.gz
    gunzips to the text the run without --compress wrote."""
    base = ("--seed", "42", "--model", "novaseq", "--store_mutations")
    text, _ = cli(*(base + ("--origins",)))
    more = base + ("--ubam", "--compress", "--report")
    plain, _ = cli(*more)
    with_flag, _ = cli(*(more + ("--origins",)))
    assert open(with_flag + ".bam", "rb").read() == open(plain + ".bam", "rb").read()
    assert open(with_flag + ".vcf.gz", "rb").read() == open(plain + ".vcf.gz", "rb").read()
    assert open(with_flag + "_report.json", "rb").read() == open(plain + "_report.json", "rb").read()
    made = sorted(os.listdir(os.path.dirname(with_flag)))
    assert "out_origins.bedpe.gz" in made and "out_origins.bedpe" not in made
    assert gzip.open(with_flag + G.SUFFIX + ".gz", "rb").read() == open(text + G.SUFFIX, "rb").read()


def test_mt_workers_take_the_pool(cli):
    """--rng mt --cpus 2 --devices 1 --origins runs one process per worker: the FASTQ files are those of the side-by-side set
    without the flag, and of one process per worker (--report, which takes the pool too); the lines name the reads in order."""
    base = ("--seed", "42", "--mode", "perfect", "--rng", "mt", "--cpus", "2", "--devices", "1")
    side_by_side, _ = cli(*base)
    pool, _ = cli(*(base + ("--report",)))
    with_flag, seqs = cli(*(base + ("--origins",)))
    for suffix in ("_R1.fastq", "_R2.fastq"):
        assert open(with_flag + suffix, "rb").read() == open(side_by_side + suffix, "rb").read() == open(pool + suffix, "rb").read()
    p = G.parse(with_flag + G.SUFFIX)
    r1, r2 = _fastq(with_flag + "_R1.fastq"), _fastq(with_flag + "_R2.fastq")
    assert [n + "/1" for n in p["name"]] == [h for h, _s in r1] and len(r1) == 1000
    by_id = {rid: s.encode() for rid, s in zip(IDS, seqs)}
    for k in range(1000):
        seq = by_id[p["id"][k]]
        assert r1[k][1] == seq[p["s1"][k]:p["e1"][k]] and r2[k][1] == seq[p["s2"][k]:p["e2"][k]].translate(_COMPLEMENT)[::-1]
