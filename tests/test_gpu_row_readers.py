"""Every reader of the output rows across the read-length range.

A pair's row depends on the read length RL: pitch = 8 ceil(RL / 8), row = 128 ceil(pitch / 32) bytes, 16-byte pieces
[8 bases][8 phreds] behind xp(), a padded last line unless RL is a multiple of 32.  The writers are compared with the CPU
oracle at many read lengths elsewhere, always through download(); here the OTHER readers -- k_rows_export, k_fastq_format, the
k_deflate_* chain, the k_vcf_* chain, and k_perfect / k_mt_emit as writers in front of them -- run over
helpers.ROW_SWEEP: one partial piece (2, 5, 7), pitch == RL (8, 16, ...), no padding (32, 64, 128, 256, 1024), the engine's
limit (997, 1024).  Everything is byte-exact against the oracle's arrays (Philox mode) put into text by the few plain lines of
helpers.fastq_text / helpers.vcf_lines, which tests/test_row_readers_host.py pins to the host formatter without a GPU."""
import gzip

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import helpers as H
from helpers import Guarded

pytestmark = pytest.mark.gpu

N = H.ROW_SWEEP_PAIRS                   # 205 rows a case: 200 pairs from first pair 5
CPU = H.ROW_SWEEP_CPU
IDS = ("g", "NZ_" + "k" * 294 + ".17")  # record ids of 1 and of 300 letters
EMITS = ((4, 13), (17, 187))             # (first pair id, pairs) of the two emits, rows 5 .. 204: ids 4 .. 16 cross 9|10, 17 .. 203 cross 99|100
# read lengths whose export tiles start at different addresses mod 16 within ONE launch (tile * 2 RL is no multiple of 16).
# 1024 cannot be among them, nor 256: an output row of 2 RL bytes is a multiple of 16 there, so every tile of a launch starts at
# the buffer's own alignment and only the buffer's shift moves it.  Up to 191 positions a tile is 64 pairs and tile * 2 RL a
# multiple of 128: the same.  Asserted from the tile rule below, not assumed.
MIXED_TILE_STARTS = (250, 997)
CODES = np.full(256, 4, dtype=np.uint8)
for _k, _pair in enumerate(("Aa", "Cc", "Gg", "Tt")):
    CODES[[ord(c) for c in _pair]] = _k


class Case(object):
    """One engine with the sweep's model at RL and N generated rows, and the oracle's arrays for them (left unchanged)."""

    def __init__(self, RL, how="philox"):
        from insilicoseq_amd.engine import ReadEngine
        from insilicoseq_amd.model import DenseModel
        from oracle import oracle as O

        self.RL = RL
        dense = DenseModel.perfect(RL) if how == "perfect" else H.row_sweep_model(RL)
        # (perfect: insert size 200, so a longer record; the oracle runs its tables as quality mode 1, see test_gpu_perfect.py)
        genome = H.mixed_genome(60 * RL, 8 * RL + 400) if how == "perfect" else H.row_sweep_genome(RL)
        kw = dict(quality_mode=1, basic_insert_size=dense.basic_insert_size) if how == "perfect" else None
        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(dense)
            gid = eng.add_genome(genome)
            if how == "mt":
                eng.seed_mt(H.ROW_SWEEP_MT_SEED)
                assert eng.generate_mt(gid, N) == N
                rng, first = O.Rng().seed_mt(H.ROW_SWEEP_MT_SEED), 0
            else:
                eng.generate(gid, N, first_ordinal=H.ROW_SWEEP_FIRST_ORDINAL, seed=H.ROW_SWEEP_SEED)
                rng, first = O.Rng().seed_philox(H.ROW_SWEEP_SEED), H.ROW_SWEEP_FIRST_ORDINAL
            eng.synchronize()
            self.kernel = eng.main_kernel() if how != "mt" else None
            self.exp = H.row_sweep_oracle_rows(dense, rng, genome, N, first, kw)
        except Exception:
            eng.close()
            raise

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module", params=H.ROW_SWEEP)
def case(request):
    """(module scope and parametrised: pytest runs the checks read length by read length, one engine alive at a time)"""
    c = Case(request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ the checks, on any engine whose rows the oracle gave
def check_rows(c):
    """The writer's part: rows and coordinates as download() / coords() read them equal the oracle's."""
    d = c.eng.download(0, N)
    for k, (name, mate) in enumerate((("r1_base", 0), ("r1_qual", 0), ("r2_base", 1), ("r2_qual", 1))):
        want = c.exp["qual" if k % 2 else "bases"][:, mate]
        bad = np.argwhere(d[name] != want)
        assert bad.size == 0, "%s differs at (pair, pos) %s ... (%d cells)" % (name, bad[:5].tolist(), len(bad))
    assert np.array_equal(c.eng.coords(0, N), c.exp["coords"])


def check_export(c, first, n, shift, encoding, want=("bases", "qual", "coords", "item")):
    """export() of rows [first, +n) into guarded buffers whose payloads start at ``shift`` mod 16."""
    from insilicoseq_amd.tensors import recode

    RL, eng = c.RL, c.eng
    outs = {"bases": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), shift), "qual": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), shift),
            "coords": Guarded(n * 32, np.int64, (n, 4)), "item": Guarded(n * 4, np.int32, (n,))}
    torch.cuda.synchronize()  # (the buffers were filled on torch's stream, the engine works on its own)
    eng.export(first, n, *[outs[k].ptr if k in want else None for k in ("bases", "qual", "coords", "item")], encoding=encoding)
    eng.synchronize()
    sl = slice(first, first + n)
    ascii_ = c.exp["bases"][sl]
    expect = {"bases": ascii_ if encoding == "ascii" else CODES[ascii_], "qual": c.exp["qual"][sl], "coords": c.exp["coords"][sl],
              "item": np.zeros(n, dtype=np.int32)}
    if encoding == "codes":
        assert np.array_equal(expect["bases"], recode(ascii_))
    where = (RL, first, n, shift, encoding)
    for k, o in outs.items():
        assert o.guards_intact(), (k,) + where
        if k not in want:
            assert o.untouched(), ("%s was not asked for" % k,) + where
            continue
        got = o.value()
        if not np.array_equal(got, expect[k]):
            bad = np.argwhere(got != expect[k])
            raise AssertionError("export %s differs at %s ... (%d cells): RL %d, first pair %d, n %d, shift %d, %s" % (
                (k, bad[:5].tolist(), len(bad)) + where))


def expected_text(c, rid, mate):
    row, text = 5, []
    for first_i, n in EMITS:
        text.append(H.fastq_text(rid, first_i, CPU, mate, c.exp["bases"][row:row + n, mate - 1], c.exp["qual"][row:row + n, mate - 1]))
        row += n
    return b"".join(text)


def emit(c, tmp_path, rid, tag, compress=False):
    """The two emits of rows 5 .. 204 under record id ``rid``: the bytes of both files."""
    eng = c.eng
    head = b"" if compress else b"# a line the files already hold\n"  # (text is appended behind it)
    paths = [tmp_path / ("%s_%d.fq" % (tag, m)) for m in (1, 2)]
    fh = [open(p, "wb") for p in paths]
    try:
        for f in fh:
            f.write(head)
            f.flush()
        eng.fastq_compress(compress)
        row = 5
        for k, (first_i, n) in enumerate(EMITS):
            eng.fastq_emit(fh[0].fileno(), fh[1].fileno(), rid, first_i, CPU, row, n, n_threads=1 + k)
            row += n
        eng.fastq_flush()
    finally:
        for f in fh:
            f.close()
        eng.fastq_compress(False)
    out = [p.read_bytes() for p in paths]
    assert all(o.startswith(head) for o in out)
    return [o[len(head):] for o in out]


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d bytes against %d, first difference at byte %d: %r against %r" % (len(got), len(want), k, got[k:k + 40], want[k:k + 40])


def check_fastq_text(c, tmp_path, ids=IDS):
    for rid in ids:
        got = emit(c, tmp_path, rid, "t%d" % len(rid))
        for m in (1, 2):
            want = expected_text(c, rid, m)
            assert got[m - 1] == want, "RL %d, id of %d letters, mate %d: %s" % (c.RL, len(rid), m, first_difference(got[m - 1], want))


# ------------------------------------------------------------------ Philox rows over the whole sweep
def test_rows_match_oracle(case):
    check_rows(case)


def test_export(case):
    RL = case.RL
    for shift in (0, 1, 8, 15):
        starts = H.export_tile_alignments(RL, 200, shift)
        assert len(starts) >= 4  # (four tiles and more in 200 pairs)
        assert (len(set(starts)) > 1) == (RL in MIXED_TILE_STARTS), (RL, shift, starts)
        for first in (0, 1, 5):
            for n in (1, 13, 200):
                for encoding in ("ascii", "codes"):
                    check_export(case, first, n, shift, encoding)
    for want in (("bases",), ("qual",), ("coords",), ("item",), ()):  # outputs not asked for stay as they are
        check_export(case, 1, 13, 15, "ascii", want=want)
        check_export(case, 5, 200, 1, "codes", want=want)


def test_device_fastq_text(case, tmp_path):
    check_fastq_text(case, tmp_path)


def test_device_gzip(case, tmp_path, monkeypatch):
    RL = case.RL
    monkeypatch.delenv("ISS_DEFLATE_RUNS_ONLY", raising=False)  # (read by the library at every emit)
    for rid in IDS:
        want = [expected_text(case, rid, m) for m in (1, 2)]
        modes = ["matches"]
        if len(rid) == 1 and RL <= 8:
            # records shorter than the matcher's 32-byte chunk: a previous-record match overlaps its own source
            lines = want[0].split(b"\n")[:-1] + want[1].split(b"\n")[:-1]
            lengths = set(sum(len(x) + 1 for x in lines[k:k + 4]) for k in range(0, len(lines), 4))
            assert len(lines) == 1600 and all(17 <= x <= 31 for x in lengths), sorted(lengths)
            modes.append("runs only")
        packed = {}
        for mode in modes:
            if mode == "runs only":
                monkeypatch.setenv("ISS_DEFLATE_RUNS_ONLY", "1")
            packed[mode] = emit(case, tmp_path, rid, "z%d%s" % (len(rid), mode[0]), compress=True)
            monkeypatch.delenv("ISS_DEFLATE_RUNS_ONLY", raising=False)
            for m in (1, 2):
                z = packed[mode][m - 1]
                assert z[:4] == b"\x1f\x8b\x08\x00", (RL, mode, z[:4])
                text = gzip.decompress(z)  # (CRC-32 and ISIZE of every member are verified on the way)
                assert text == want[m - 1], "RL %d, id of %d letters, mate %d, %s: %s" % (RL, len(rid), m, mode,
                                                                                             first_difference(text, want[m - 1]))
        if len(modes) == 2:  # the switch reached the library: the streams with previous-record matches are other streams
            assert packed["matches"][0] != packed["runs only"][0]


def test_store_mutations_worker(case, tmp_path, monkeypatch):
    from insilicoseq_amd import generator as G

    RL = case.RL
    dense = H.row_sweep_model(RL)
    (ids, seqs, counts), r1, r2, vcf, types = H.row_sweep_worker_files(dense, RL)
    assert counts[1] == 0 and types.count(0) >= 1 and (RL < 16 or (types.count(1) >= 1 and types.count(2) >= 1))
    dense.store_mutations = True
    # 64 pairs a batch: the batches are cut across the items (64 | 6 + 58 | 64 | 8), and the row buffers stay small
    monkeypatch.setattr(G.Worker, "BATCH_PAIRS", 64)
    prefix = str(tmp_path / "w")
    work = [(G.Record(seq, id=rid), n, "default") for rid, seq, n in zip(ids, seqs, counts)]
    G.worker_iterator(work, dense, CPU, prefix, H.ROW_SWEEP_WORKER_SEED, "metagenomics", False, device=0, rng="philox")
    got = open(prefix + ".vcf").read()
    if got != vcf:
        a, b = got.split("\n"), vcf.split("\n")
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError("RL %d: %d VCF lines against %d, first difference at line %d: %r against %r" % (
            RL, len(a) - 1, len(b) - 1, k, a[k:k + 1], b[k:k + 1]))
    for name, want in (("_R1.fastq", r1), ("_R2.fastq", r2)):
        text = open(prefix + name, "rb").read()
        assert text == want, "RL %d, %s: %s" % (RL, name, first_difference(text, want))


# ------------------------------------------------------------------ k_perfect's rows, k_mt_emit's rows
@pytest.mark.parametrize("RL", H.ROW_SWEEP)
def test_perfect_rows_and_their_readers(RL, tmp_path):
    c = Case(RL, "perfect")
    try:
        assert c.kernel == "k_perfect", c.kernel
        assert (c.exp["qual"] == 40).all()
        check_rows(c)
        check_export(c, 5, 200, 5, "ascii")
        check_export(c, 5, 200, 5, "codes")
        check_fastq_text(c, tmp_path, ids=IDS[:1])
    finally:
        c.close()


@pytest.mark.parametrize("RL", [8, 32, 997])
def test_mt_rows_and_their_readers(RL, tmp_path):
    c = Case(RL, "mt")
    try:
        check_rows(c)
        check_export(c, 5, 200, 5, "ascii")
        check_export(c, 5, 200, 5, "codes")
        check_fastq_text(c, tmp_path, ids=IDS[:1])
    finally:
        c.close()
