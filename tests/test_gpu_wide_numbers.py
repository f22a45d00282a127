"""Everything that READS the output rows, at pair ids and coordinates that need more than 32 bits.

A. Pair ids (tests/wide_numbers.py: WIDE_ITEMS -- 9|10 digits, 2^31, 2^32, 10^10, 10^15, 10^18, the id x* at which the character
   count of all smaller ids passes 2^64, and 2^63 - 1) through every device formatter: FASTQ text and gzip, the scatter route,
   uBAM, VCF text from the Philox slots and from a worker set, BEDPE plain and as BGZF.  200 rows of a 5 000-base record; the
   expected bytes are the rows' own download formatted with "%d" in Python -- never a host formatter of the library.
B. Coordinates: one record of 2^32 + 70 000 003 bases with IUPAC and lower-case stretches and a prime period, uploaded once, alone
   and as the middle item of a batch whose last item then stands beyond 2^32 in the arena: k_rows_export's coordinates and item
   labels, the truth arrays against the record's own bytes, the BEDPE text, and k_perfect's mask / ASCII lookups up there."""
import gzip
import os
import struct
import time

import numpy as np
import pytest
import torch  # noqa: F401  (here, when the module is collected: torch's HIP runtime has to be the process's first)

import ubam_twin as U
import wide_numbers as W
from helpers import Guarded, dense_model, mixed_genome

pytestmark = pytest.mark.gpu

N_ROWS = 200
RECORD = 5000
READ_KEYS = ("r1_base", "r1_qual", "r2_base", "r2_qual")


def _first_difference(got, want):
    return next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))


def _same(got, want, what):
    assert len(got) == len(want) and got == want, "%s: %d bytes against %d, first difference at byte %d: %r against %r" % (
        what, len(got), len(want), _first_difference(got, want), got[max(0, _first_difference(got, want) - 30):][:60],
        want[max(0, _first_difference(got, want) - 30):][:60])


# ---------------------------------------------------------------------------------------------------- A. pair ids
class Rows(object):
    """An engine with N_ROWS rows of a 5 000-base record with lower-case and IUPAC letters, and their download (left unchanged)."""

    def __init__(self, model, indel=None, seed=77, slots=0):
        from insilicoseq_amd.engine import ReadEngine

        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(dense_model(model, indel))
            self.RL = eng.read_length
            self.gid = eng.add_genome(mixed_genome(900 + self.RL, RECORD))
            if slots:
                eng.mutations_reserve(slots)
            eng.generate(self.gid, N_ROWS, first_ordinal=3, seed=seed)
            eng.synchronize()
            d = eng.download(0, N_ROWS)
            self.rows = [d[k].copy() for k in READ_KEYS]
            self.coords = eng.coords(0, N_ROWS).copy()
            self.mutations = eng.mutations().copy() if slots else None
        except Exception:
            eng.close()
            raise


@pytest.fixture(scope="module")
def short():
    r = Rows("ecoli")
    assert r.RL == 20
    yield r
    r.eng.close()


@pytest.fixture(scope="module")
def mutated():
    r = Rows("novaseq", (0.01, 0.03), seed=21, slots=2_000_000)
    yield r
    r.eng.close()


def _fastq_want(r, items, cpu):
    return [W.fastq_items_text(items, cpu, r.rows[2 * m], r.rows[2 * m + 1], m + 1) for m in range(2)]


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("cpu", W.WIDE_CPUS)
def test_fastq_emit_batch(short, tmp_path, cpu, compress):
    """k_fastq_format (and with compress the k_deflate_* kernels behind it): all of WIDE_ITEMS as the items of ONE call -- the item
    offsets text_off and before_first behind a wide item -- then the same items one call each, appended to the same files."""
    eng, items = short.eng, W.wide_items()
    paths = [str(tmp_path / p) for p in ("d1.fq", "d2.fq")]
    fh = [open(p, "wb") for p in paths]
    eng.fastq_compress(compress)
    try:
        eng.fastq_emit_batch(fh[0].fileno(), fh[1].fileno(), items, cpu)
        for it in items:
            eng.fastq_emit_batch(fh[0].fileno(), fh[1].fileno(), [it], cpu)
        eng.fastq_flush()
        for f, p in zip(fh, paths):
            assert os.lseek(f.fileno(), 0, os.SEEK_CUR) == os.path.getsize(p)
    finally:
        eng.fastq_flush()
        eng.fastq_compress(False)
        for f in fh:
            f.close()
    for m, want in enumerate(_fastq_want(short, items, cpu)):
        got = open(paths[m], "rb").read()
        _same(gzip.decompress(got) if compress else got, want + want, "mate %d" % (m + 1))


def test_fastq_emit_scatter(short, tmp_path):
    """The worker-set route of k_fastq_format: three workers with the three worker numbers, each item written at its own byte
    offset of the final files (worker after worker), the offsets taken from the Python text's sizes."""
    eng = short.eng
    items = W.wide_items()
    by_worker = [[it for k, it in enumerate(items) if k % 3 == w] for w in range(3)]
    image, scatter = [b"", b""], []
    for w, its in enumerate(by_worker):
        for it in its:
            texts = _fastq_want(short, [it], W.WIDE_CPUS[w])
            assert len(texts[0]) == len(texts[1])
            scatter.append(it + (W.WIDE_CPUS[w], len(image[0])))
            image = [image[m] + texts[m] for m in range(2)]
    scatter = [scatter[k] for k in np.random.RandomState(3).permutation(len(scatter))]  # (not in file order)
    paths = [str(tmp_path / p) for p in ("s1.fq", "s2.fq")]
    fh = [open(p, "wb") for p in paths]
    try:
        eng.fastq_emit_scatter(fh[0].fileno(), fh[1].fileno(), scatter, n_threads=2)
        eng.fastq_flush()
    finally:
        for f in fh:
            f.close()
    for m in range(2):
        _same(open(paths[m], "rb").read(), image[m], "mate %d" % (m + 1))


@pytest.mark.parametrize("cpu", W.WIDE_CPUS)
def test_ubam_emit_batch(short, tmp_path, cpu):
    """k_ubam_format and the k_bgzf_* kernels: the members inflate to exactly the twin's records; block_size and l_read_name of the
    first and last record of every item, parsed here."""
    eng, items = short.eng, W.wide_items()
    path = str(tmp_path / "d.bam")
    with open(path, "wb") as fh:
        eng.ubam_emit_batch(fh.fileno(), items, cpu)
        for it in items[5:]:
            eng.ubam_emit_batch(fh.fileno(), [it], cpu)
        eng.ubam_flush()
    data = b"".join(U.inflate_member(m) for m in U.split_members(open(path, "rb").read()))
    _same(data, W.ubam_records(items, cpu, *short.rows) + W.ubam_records(items[5:], cpu, *short.rows), "records")
    at, pos = [], 0
    while pos < len(data):
        at.append(pos)
        pos += 4 + struct.unpack_from("<i", data, pos)[0]
    assert pos == len(data) and len(at) == 2 * (W.WIDE_ROWS + sum(it[3] for it in items[5:]))
    RL, rec = short.RL, 0
    for rid, first_i, _row, n in items + items[5:]:
        for j in (0, n - 1):
            for mate in range(2):
                p = at[2 * (rec + j) + mate]
                name = b"%s_%d_%d" % (rid.encode(), first_i + j, cpu)
                assert data[p + 12] == len(name) + 1 and data[p + 36:p + 36 + len(name) + 1] == name + b"\0", (first_i + j, mate)
                assert struct.unpack_from("<i", data, p)[0] == 32 + len(name) + 1 + (RL + 1) // 2 + RL, (first_i + j, mate)
        rec += n


def _rows_at_wide_ids(lines):
    """Lines of a VCF text whose pair id is at or beyond 2^32."""
    return sum(1 for ln in lines.split(b"\n")[:-1] if int(ln.split(b"\t")[0].rsplit(b"/", 1)[0].rsplit(b"_", 2)[1]) >= 2 ** 32)


@pytest.mark.parametrize("cpu", W.WIDE_CPUS)
def test_vcf_emit_philox(mutated, tmp_path, cpu):
    """k_vcf_len / k_vcf_format behind the Philox slots (k_vcf_count, k_vcf_scatter, k_vcf_rank): WIDE_ITEMS on consecutive pair
    ranges of the call, against the call's downloaded rows formatted in Python."""
    eng, items = mutated.eng, W.wide_items()
    want = W.vcf_items_text(items, cpu, mutated.mutations)
    assert _rows_at_wide_ids(want) >= 50 and b"\t.\t\t\n" in want  # (indel rows among them)
    path = str(tmp_path / "d.vcf")
    with open(path, "wb") as fh:
        eng.vcf_emit(fh.fileno(), items, cpu)
        eng.vcf_flush()
    _same(open(path, "rb").read(), want, "VCF text")


def test_vcf_emit_workers(tmp_path):
    """The worker-set route (VcfArgs::wbase): one worker per item of WIDE_ITEMS, its first pair id and pair count the item's, the
    worker numbers cycling through the three; every worker's file against its downloaded rows formatted in Python.  A negative
    first pair id in any worker's entry refuses the whole call."""
    from insilicoseq_amd._native import E_INVALID, EngineError
    from insilicoseq_amd.engine import ReadEngine

    n_w, stride = len(W.WIDE_ITEMS), 64
    cpus = [W.WIDE_CPUS[k % 3] for k in range(n_w)]
    rids = [W.WIDE_IDS[k % 2] for k in range(n_w)]
    files = [open(str(tmp_path / ("w%d.vcf" % k)), "wb") for k in range(n_w)]
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq", (0.01, 0.03)))
        gid = eng.add_genome(mixed_genome(903, RECORD))
        eng.seed_mt_workers([40 + k for k in range(n_w)])
        eng.mt_workers_mutations_reserve(20000)
        done, status = eng.generate_mt_workers([gid] * n_w, [n for _, n in W.WIDE_ITEMS], [k * stride for k in range(n_w)])
        assert list(done) == [n for _, n in W.WIDE_ITEMS] and not any(status)
        entries = [(files[k].fileno(), rids[k], W.WIDE_ITEMS[k][0], k * stride, W.WIDE_ITEMS[k][1], cpus[k]) for k in range(n_w)]
        with pytest.raises(EngineError) as e:
            eng.vcf_emit_workers(entries[:3] + [entries[3][:2] + (-1,) + entries[3][3:]] + entries[4:])
        assert e.value.code == E_INVALID
        eng.vcf_emit_workers(entries)
        eng.vcf_flush()
        want = ["".join(W.vcf_lines(rids[k], W.WIDE_ITEMS[k][0], cpus[k], eng.mt_workers_mutations(k))).encode() for k in range(n_w)]
    for f in files:
        f.close()
    assert sum(_rows_at_wide_ids(t) for t in want) >= 50
    for k in range(n_w):
        _same(open(str(tmp_path / ("w%d.vcf" % k)), "rb").read(), want[k], "worker %d" % k)


@pytest.mark.parametrize("bgzip", [False, True])
@pytest.mark.parametrize("cpu", W.WIDE_CPUS)
def test_origins_emit_batch(short, tmp_path, cpu, bgzip):
    """k_origins_len / k_origins_format (with bgzip the BGZF text kernels behind them): the ids across the 32-bit path switch of
    origins_digits / origins_put_u64, in one call and one call per item."""
    eng, items = short.eng, W.wide_items()
    want = W.bedpe_text(items, [RECORD] * len(items), cpu, short.coords[:W.WIDE_ROWS], short.RL)
    path = str(tmp_path / "o.bedpe")
    eng.origins_compress(bgzip)
    try:
        with open(path, "wb") as fh:
            eng.origins_emit_batch(fh.fileno(), items, [RECORD] * len(items), cpu)
            for it in items:
                eng.origins_emit_batch(fh.fileno(), [it], [RECORD], cpu)
            eng.origins_flush()
    finally:
        eng.origins_flush()
        eng.origins_compress(False)
    got = open(path, "rb").read()
    _same(gzip.decompress(got) if bgzip else got, want + want, "BEDPE text")
    assert b"_4294967296_" in want and b"_10000000000_" in want and b"_9223372036854775806_" in want


def test_negative_first_pair_id_is_refused(short, mutated, tmp_path):
    """Every entry that takes first pair ids: E_INVALID for a negative one (in the second item: the first is fine), and nothing is
    appended."""
    from insilicoseq_amd._native import E_INVALID, EngineError

    good, bad = ("g", 5, 0, 3), ("g", -1, 3, 3)
    paths = [str(tmp_path / p) for p in ("a", "b")]
    fh = [open(p, "wb") for p in paths]
    calls = [
        lambda: short.eng.fastq_emit_batch(fh[0].fileno(), fh[1].fileno(), [good, bad], 0),
        lambda: short.eng.fastq_emit(fh[0].fileno(), fh[1].fileno(), "g", -1, 0, 0, 3),
        lambda: short.eng.fastq_emit_scatter(fh[0].fileno(), fh[1].fileno(), [good + (0, 0), bad + (0, 4096)]),
        lambda: short.eng.ubam_emit_batch(fh[0].fileno(), [good, bad], 0),
        lambda: short.eng.origins_emit_batch(fh[0].fileno(), [good, bad], [RECORD, RECORD], 0),
        lambda: mutated.eng.vcf_emit(fh[0].fileno(), [good, bad], 0),
        lambda: short.eng.fastq_emit_batch(fh[0].fileno(), fh[1].fileno(), [good, ("g", -2 ** 63, 3, 3)], 0),
    ]
    try:
        for k, call in enumerate(calls):
            with pytest.raises(EngineError) as e:
                call()
            assert e.value.code == E_INVALID, (k, e.value)
        short.eng.fastq_flush()
        short.eng.ubam_flush()
        short.eng.origins_flush()
        mutated.eng.vcf_flush()
    finally:
        for f in fh:
            f.close()
    assert [os.path.getsize(p) for p in paths] == [0, 0]


# ---------------------------------------------------------------------------------------------------- B. coordinates
BIG = 2 ** 32 + 70_000_003
N_BIG = 150_000
SMALL = 3000
SIDE = 2000  # pairs of each small item of the batch
ORD0, SEED = 7, 13


class Big(object):
    def __init__(self):
        from insilicoseq_amd.engine import ReadEngine

        t0 = time.time()
        self.g = W.prime_period_record(BIG)
        self.small = [np.frombuffer(mixed_genome(910 + k, SMALL).encode(), dtype=np.uint8) for k in range(2)]
        self.eng = ReadEngine(0)
        try:
            self.eng.load_model(dense_model("hiseq"))
            self.gid = self.eng.add_genome(self.g)
            self.side = [self.eng.add_genome(s) for s in self.small]
        except Exception:
            self.eng.close()
            raise
        print("part B fixture: %.1f s" % (time.time() - t0))

    def picks(self, coords):
        """The pick list of test_records_of_2_31_bases_and_more: the 24 largest, the 8 smallest, 32 random pairs."""
        order = np.argsort(coords[:, 2])
        return [int(i) for i in list(order[-24:]) + list(order[:8]) + list(np.random.RandomState(2).randint(0, len(coords), 32))]


@pytest.fixture(scope="module")
def big():
    b = Big()
    yield b
    b.eng.close()


def _export(eng, first, n, RL, want=("bases", "qual", "coords", "item")):
    outs = {"bases": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), 3), "qual": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), 5),
            "coords": Guarded(n * 32, np.int64, (n, 4)), "item": Guarded(n * 4, np.int32, (n,))}
    torch.cuda.synchronize()  # (the buffers were filled on torch's stream, the engine works on its own)
    eng.export(first, n, *[outs[k].ptr if k in want else None for k in ("bases", "qual", "coords", "item")])
    eng.synchronize()
    assert all(o.guards_intact() for o in outs.values())
    return {k: outs[k].value() for k in want}


def _against_oracle(orc, g, seed, ordinal, coords_row, rows):
    """One pair at ``ordinal`` of the oracle's Philox stream: coordinates and, where given, the four rows (mate, RL)."""
    from oracle import oracle as O

    exp = orc.simulate(O.Rng().seed_philox(seed), g, 1, first_ordinal=ordinal, want_coords=True)
    assert exp["status"] == 0
    assert np.array_equal(coords_row, exp["coords"][0]), (ordinal, coords_row.tolist(), exp["coords"][0].tolist())
    if rows is not None:
        bases, qual = rows
        assert np.array_equal(bases[0], exp["r1_base"][0]) and np.array_equal(bases[1], exp["r2_base"][0]), ordinal
        assert np.array_equal(qual[0], exp["r1_qual"][0]) and np.array_equal(qual[1], exp["r2_qual"][0]), ordinal


def _origins_text(eng, path, items, lengths, cpu):
    with open(path, "wb") as fh:
        eng.origins_emit_batch(fh.fileno(), items, lengths, cpu)
        eng.origins_flush()
    return open(path, "rb").read()


def test_export_and_origins_of_a_record_beyond_2_32(big, tmp_path):
    """k_rows_export and k_origins_len / k_origins_format on the record alone: the exported coordinates are eng.coords and, at the
    pick list, the oracle's (with the exported rows); the BEDPE file of all rows is lines_host on eng.coords, ten-digit starts at or
    beyond 2^32 in it."""
    from oracle import oracle as O

    t0 = time.time()
    eng, dense = big.eng, dense_model("hiseq")
    eng.load_model(dense)
    RL = eng.read_length
    eng.generate(big.gid, N_BIG, first_ordinal=ORD0, seed=SEED)
    eng.synchronize()
    coords = eng.coords(0, N_BIG)
    assert int((coords[:, 0] >= 2 ** 32).sum()) > N_BIG // 100 and int(coords[:, 2].max()) <= BIG and int(coords[:, 0].min()) >= 0
    got = _export(eng, 0, N_BIG, RL)
    assert np.array_equal(got["coords"], coords) and not got["item"].any()
    orc = O.Oracle(dense)
    for i in big.picks(coords):
        _against_oracle(orc, big.g, SEED, ORD0 + i, got["coords"][i], (got["bases"][i], got["qual"][i]))
    first_i = 2 ** 32 - 1000  # (wide ids beside the wide coordinates)
    items = [("chrBig", first_i, 0, N_BIG)]
    text = _origins_text(eng, str(tmp_path / "o.bedpe"), items, [BIG], 7)
    _same(text, W.bedpe_text(items, [BIG], 7, coords, RL), "BEDPE text")
    s1 = [f.split(b"\t")[1] for f in text.split(b"\n")[:-1]]
    assert sum(1 for s in s1 if len(s) == 10 and int(s) >= 4294967296) > N_BIG // 100
    print("part B single: %.1f s" % (time.time() - t0))


def test_export_and_origins_of_a_batch_arena_beyond_2_32(big, tmp_path):
    """generate_batch([small, big, small]): the last item stands beyond 2^32 in the arena while its record coordinates are small.
    k_rows_export's and origins_pair's `descriptor - arena offset`: coordinates equal eng.coords, the third item's all lie in
    [0, 3000] under item label 2, the middle item's equal the oracle's at the pick list, and the BEDPE text is lines_host's."""
    from oracle import oracle as O

    t0 = time.time()
    eng, dense = big.eng, dense_model("hiseq")
    eng.load_model(dense)
    RL = eng.read_length
    counts = [SIDE, N_BIG, SIDE]
    total = sum(counts)
    eng.generate_batch([big.side[0], big.gid, big.side[1]], counts, first_ordinal=ORD0, seed=SEED)
    eng.synchronize()
    coords = eng.coords(0, total)
    got = _export(eng, 0, total, RL)
    assert np.array_equal(got["coords"], coords)
    assert np.array_equal(got["item"], np.repeat(np.arange(3, dtype=np.int32), counts))
    for lo, hi in ((0, SIDE), (SIDE + N_BIG, total)):
        c = got["coords"][lo:hi]
        assert int(c[:, :3].min()) >= 0 and int(c[:, :3].max()) <= SMALL and (c[:, 1] == c[:, 2] - RL).all(), (lo, hi)
    mid = got["coords"][SIDE:SIDE + N_BIG]
    assert int((mid[:, 0] >= 2 ** 32).sum()) > N_BIG // 100 and int(mid[:, 2].max()) <= BIG and int(mid[:, 0].min()) >= 0
    orc = O.Oracle(dense)
    for i in big.picks(mid):
        r = SIDE + i
        _against_oracle(orc, big.g, SEED, ORD0 + r, got["coords"][r], (got["bases"][r], got["qual"][r]))
    for k, r in ((0, 0), (0, SIDE - 1), (1, SIDE + N_BIG), (1, total - 1), (1, SIDE + N_BIG + 777)):  # the small items, too
        _against_oracle(orc, big.small[k], SEED, ORD0 + r, got["coords"][r], (got["bases"][r], got["qual"][r]))
    items = [("left", 2 ** 32 - 5, 0, SIDE), ("chrBig", 10 ** 10 - 70_000, SIDE, N_BIG), ("right", 2 ** 63 - 1 - SIDE, SIDE + N_BIG, SIDE)]
    text = _origins_text(eng, str(tmp_path / "o.bedpe"), items, [SMALL, BIG, SMALL], 2147483647)
    _same(text, W.bedpe_text(items, [SMALL, BIG, SMALL], 2147483647, coords, RL), "BEDPE text")
    print("part B batch: %.1f s" % (time.time() - t0))


def test_truth_of_a_record_beyond_2_32(big):
    """k_main<true, ...> (--store_mutations) and k_truth_scatter on a model without indels: for every pair that starts at or beyond
    2^31, and at or beyond 2^32, the truth of mate 1 is the record's own bytes g[fs : fs + RL] and the truth of mate 2 the reverse
    complement of g[re - RL : re] -- numpy on the host copy of the record, no library code in the expectation.  The shipped
    novaseq profile has insertion rates of its own (five reads of these 300 000 carry one, and a read behind an insertion is not
    its window): they are zeroed here."""
    from oracle import oracle as O

    t0 = time.time()
    eng = big.eng
    eng.load_model(dense_model("novaseq", (0.0, 0.0)))
    RL = eng.read_length
    eng.mutations_reserve(16_000_000)
    try:
        eng.generate(big.gid, N_BIG, first_ordinal=ORD0, seed=SEED)
        eng.synchronize()
        coords = eng.coords(0, N_BIG)
        bases = _export(eng, 0, N_BIG, RL, want=("bases",))["bases"]
        truth = Guarded(N_BIG * 2 * RL, np.uint8, (N_BIG, 2, RL), 7)
        events, n_events = Guarded(24, np.int32, (1, 6)), Guarded(8, np.int64, ())
        torch.cuda.synchronize()
        eng.export_mutations(0, N_BIG, truth_ptr=truth.ptr, events_ptr=events.ptr, capacity=1, n_events_ptr=n_events.ptr)
        eng.synchronize()
    finally:
        eng.mutations_reserve(0)
    assert truth.guards_intact() and events.guards_intact() and n_events.guards_intact()
    assert int(n_events.value()) > N_BIG // 10, "the row slots overflowed, or no rows: %d" % int(n_events.value())
    truth = truth.value()
    fs, re = coords[:, 0], coords[:, 2]
    assert (coords[:, 1] == re - RL).all()
    # the reverse complement of a window, letter by letter: the oracle's table of single letters
    comp = np.zeros(256, dtype=np.uint8)
    for c in b"ACGTNRYWSMKHBVDacgtnrywsmkhbvd":
        comp[c] = ord(O.rev_comp(bytes([c])))
    for bound in (2 ** 31, 2 ** 32):
        sel = np.flatnonzero(fs >= bound)
        assert len(sel) > N_BIG // 100, (bound, len(sel))
        w1 = big.g[fs[sel, None] + np.arange(RL)]
        w2 = comp[big.g[re[sel, None] - 1 - np.arange(RL)]]
        assert np.array_equal(truth[sel, 0], w1), (bound, "mate 1")
        assert np.array_equal(truth[sel, 1], w2), (bound, "mate 2")
        assert (bases[sel] != truth[sel]).sum() > len(sel) // 10  # (substitutions were put back up there)
    # rev_comp itself on a few whole windows (the table above is its letters)
    for i in np.flatnonzero(fs >= 2 ** 32)[:8]:
        want = np.frombuffer(O.rev_comp(big.g[re[i] - RL:re[i]].tobytes()).encode(), dtype=np.uint8)
        assert np.array_equal(truth[i, 1], want), int(i)
    print("part B truth: %.1f s" % (time.time() - t0))


def test_perfect_mode_of_a_record_beyond_2_32(big):
    """k_perfect's packed, mask and ASCII indexing (lo >> 4, lo >> 5, lo + c) beyond 2^32: rows and coordinates against the oracle
    at the pick list and at the first 16 pairs that start at or beyond 2^32 and hold a letter that is not A, C, G or T (the
    descriptor's exception bits: the mask and ASCII lookups)."""
    from insilicoseq_amd.model import DenseModel
    from oracle import oracle as O

    t0 = time.time()
    eng, dense = big.eng, DenseModel.perfect(125)
    eng.load_model(dense)
    RL = eng.read_length
    eng.generate(big.gid, N_BIG, first_ordinal=ORD0, seed=SEED)
    eng.synchronize()
    assert eng.main_kernel() == "k_perfect"
    coords = eng.coords(0, N_BIG)
    assert int((coords[:, 0] >= 2 ** 32).sum()) > N_BIG // 100
    plain = np.zeros(256, dtype=bool)
    plain[list(b"ACGT")] = True
    high = np.flatnonzero(coords[:, 0] >= 2 ** 32)
    exc = [int(i) for i in high if not plain[big.g[coords[i, 0]:coords[i, 0] + RL]].all() and not plain[big.g[coords[i, 2] - RL:coords[i, 2]]].all()][:16]
    assert len(exc) == 16
    orc = O.Oracle(dense, quality_mode=1, basic_insert_size=dense.basic_insert_size)
    for i in big.picks(coords) + exc:
        d = eng.download(i, 1)
        _against_oracle(orc, big.g, SEED, ORD0 + i, coords[i], ((d["r1_base"][0], d["r2_base"][0]), (d["r1_qual"][0], d["r2_qual"][0])))
    print("part B perfect: %.1f s" % (time.time() - t0))
