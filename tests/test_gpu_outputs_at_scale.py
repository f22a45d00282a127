"""Every device-built output of a noisy generate call at scale against the oracle (tests/scale_cases.py; DESIGN section 4, "What
holds the readers of a call at scale").

A case is ONE call on the device -- 2^14 pairs of the patterned tables on the mixed record (`fixup`: every read with an event is
k_indel_fixup's, and a wavefront of its grid records read after read), on the plain record (`scripted`: k_indel_script), three
items in one generate_batch (`batch`: seams inside a wavefront's 16 pairs, a record one fragment long, a mixed record), and 2^13
pairs of the MT path (`mt`) -- shared by one test function per reader.  Every expected value is built by scale_cases from the
oracle's arrays alone; nothing the device produced (mutations(), download(), coords()) stands on the expected side.  Each
case asserts the route it reached and that the readers saw what the ledger says."""
import gzip
import os

import numpy as np
import pytest
import torch  # noqa: F401  (here, when the module is collected: torch's HIP runtime has to be the process's first)

import scale_cases as S
from helpers import Guarded

pytestmark = pytest.mark.gpu

FRONT = b"# what the file already holds\n"
FIXUP_GRID_WAVEFRONTS = 8 * 4 * 256  # k_indel_fixup: at most 8 workgroups of 4 wavefronts on each of 256 compute units
MAIN = {"fixup": "k_main<true, false, true>", "scripted": "k_main<true, true, true>", "batch": "k_main<true, false, true>"}


class Run(object):
    """A case generated once on an engine of its own: ``call`` (the oracle's side), ``eng``, the route's counters."""

    def __init__(self, name):
        from insilicoseq_amd.engine import ReadEngine
        from insilicoseq_amd.tensors import default_mutation_slots

        self.call = call = S.expected(name)
        self.name, self.kind = name, call.case.kind
        self.source = "mt" if self.kind == "mt" else "philox"
        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(call.dense)
            gids = [eng.add_genome(seq) for _rid, seq in call.records]
            eng.reserve(call.n)
            if self.kind == "mt":
                eng.seed_mt(S.MT_SEED)
                eng.mt_mutations_reserve(int(call.n * (2 * call.dense.expected_mutation_rows_per_pair() + 4)))
                before = eng.mt_path_counts()
                assert eng.generate_mt(gids[0], call.n) == call.n
                self.mt_pairs = sum(eng.mt_path_counts()) - sum(before)
            else:
                eng.mutations_reserve(default_mutation_slots(call.dense, call.n))
                eng.stats_read()  # (the counters run on until they are read)
                if self.kind == "batch":
                    eng.generate_batch([gids[k] for k in call.record_of], [it[3] for it in call.items], first_ordinal=call.case.first_ordinal,
                                       seed=S.SEED)
                else:
                    eng.generate(gids[0], call.n, first_ordinal=call.case.first_ordinal, seed=S.SEED)
                eng.synchronize()
                self.kernel, self.stats = eng.main_kernel(), eng.stats_read()
                print("\n[outputs-at-scale] %s: %s, fix-up reads %d, scripted reads %d of %d reads" % (
                    name, self.kernel, self.stats["fixup_reads"], self.stats["scripted_reads"], 2 * call.n))
            eng.synchronize()
        except Exception:
            eng.close()
            raise

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def runs():
    """The cases' calls, each made when its first reader asks for it and shared by the rest (the engines live to the module's end)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Run(name)
        return made[name]

    yield get
    for r in made.values():
        r.close()


@pytest.fixture
def run(runs, request):
    return runs(request.param)


@pytest.fixture(autouse=True)
def _host_picks_the_kernel(monkeypatch):
    for k in ("ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_MAIN_WGS", "ISS_TILES", "ISS_CHUNK_PAIRS", "ISS_LIGHT_INDELS", "ISS_DEFLATE_RUNS_ONLY",
              "ISS_HOST_VCF"):
        monkeypatch.delenv(k, raising=False)


def readers(k):
    return pytest.mark.parametrize("run", S.cases_with(k), indirect=True)


def _guarded(nbytes, dtype, shape, shift=0, zero=False):
    g = Guarded(nbytes, dtype, shape, shift)
    if zero and nbytes:
        g.buf[g.at:g.at + nbytes] = 0
    return g


def _device(array):
    """A numpy array in a guarded device block."""
    a = np.ascontiguousarray(array)
    g = Guarded(a.nbytes, a.dtype, a.shape)
    g.buf[g.at:g.at + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to("cuda:0")
    return g


def _appended(path, emit, flush, stands_at_end=True, front=FRONT):
    """What ``emit(fd)`` and ``flush()`` append to a file that already holds ``front``."""
    with open(path, "wb") as fh:
        fh.write(front)
        fh.flush()
        emit(fh.fileno())
        flush()
        if stands_at_end:  # (as the tests of these writers hold them)
            assert os.lseek(fh.fileno(), 0, os.SEEK_CUR) == os.path.getsize(path)
    data = open(path, "rb").read()
    assert data[:len(front)] == front
    return data[len(front):]


def _same(got, want, what):
    assert got == want, "%s: %s" % (what, S.first_difference(got, want))


# ---------------------------------------------------------------------------------------------------- the route, reader 1
@readers(1)
def test_the_route_and_the_rows(run):
    """The case reached the kernels it is there for; rows, coordinates and mutation rows are the oracle's."""
    call, eng = run.call, run.eng
    reads = 2 * call.n
    if run.kind == "mt":
        assert run.mt_pairs == call.n
    else:
        assert run.kernel == MAIN[run.name]
        fixup, scripted = run.stats["fixup_reads"], run.stats["scripted_reads"]
        if run.name == "fixup":  # more fix-up reads than the fix-up grid has wavefronts: a wavefront records read after read
            assert fixup > 2 * FIXUP_GRID_WAVEFRONTS and scripted == 0, run.stats
        elif run.name == "scripted":
            assert scripted > 0.9 * reads and fixup > 0, run.stats
        else:
            # both routes and both of the fix-up's reasons in one call: the plain items' reads are scripted, every read of the
            # mixed item with an indel row is the fix-up's for its record's letters -- by themselves more than the grid has
            # wavefronts -- and reads of the plain items join them (a window that leaves the short record, a script too long)
            rows = call.rows_of_item(2)
            ind = rows[rows["type"] != 0]
            mixed_reads = np.unique(ind["pair"].astype(np.int64) * 2 + ind["mate"]).size
            assert fixup > mixed_reads > FIXUP_GRID_WAVEFRONTS and scripted > 0, (run.stats, mixed_reads)
    got = eng.download(0, call.n)
    for k, (name, mate) in enumerate((("r1_base", 0), ("r1_qual", 0), ("r2_base", 1), ("r2_qual", 1))):
        want = (call.qual if k % 2 else call.bases)[:, mate]
        bad = np.argwhere(got[name] != want)
        assert bad.size == 0, "%s differs at (pair, position) %s ... (%d cells)" % (name, bad[:5].tolist(), len(bad))
    assert np.array_equal(eng.coords(0, call.n), call.coords)
    rows = eng.mt_mutations() if run.kind == "mt" else eng.mutations()
    assert len(rows) == len(call.rows) == S.LEDGER[run.name]["rows"], (len(rows), len(call.rows))
    assert np.array_equal(rows, call.rows)


# ---------------------------------------------------------------------------------------------------- reader 2: VCF
def _vcf(run, path, compress):
    eng = run.eng
    eng.vcf_compress(compress)
    try:
        return _appended(path, lambda fd: eng.vcf_emit(fd, run.call.items, S.CPU, source=run.source), eng.vcf_flush)
    finally:
        eng.vcf_flush()
        eng.vcf_compress(False)


@readers(2)
def test_vcf_text(run, tmp_path):
    want = S.vcf_text(run.call)
    got = _vcf(run, str(tmp_path / "d.vcf"), False)
    assert got.count(b"\n") == S.LEDGER[run.name]["rows"]  # the reader saw every row
    _same(got, want, "VCF text")


@readers(2)
def test_vcf_bgzf(run, tmp_path):
    raw = _vcf(run, str(tmp_path / "d.vcf.gz"), True)
    members = S.bgzf_members(raw, S.vcf_text(run.call))
    assert members == S.LEDGER[run.name]["vcf members"]
    if run.name == "fixup":
        assert members >= 128


# ---------------------------------------------------------------------------------------------------- reader 3: truth, events
def _truth(run, first, n, encoding, shift):
    call, eng = run.call, run.eng
    truth, events = S.truth_and_events(call, first, n, encoding)
    outs = {"truth": Guarded(n * 2 * call.RL, np.uint8, (n, 2, call.RL), shift), "events": Guarded((len(events) + 3) * 24, np.int32, (len(events) + 3, 6)),
            "n_events": Guarded(8, np.int64, ())}
    torch.cuda.synchronize()  # (the buffers were filled on torch's stream, the engine works on its own)
    eng.export_mutations(first, n, truth_ptr=outs["truth"].ptr, events_ptr=outs["events"].ptr, capacity=len(events) + 3,
                         n_events_ptr=outs["n_events"].ptr, encoding=encoding)
    eng.synchronize()
    assert int(outs["n_events"].value()) == len(events)
    bad = np.argwhere(outs["truth"].value() != truth)
    assert bad.size == 0, "truth differs at (pair, mate, position) %s ... (%d cells)" % (bad[:5].tolist(), len(bad))
    assert np.array_equal(outs["events"].value()[:len(events)], events)
    assert (outs["events"].value()[len(events):].view(np.uint8) == 0xA5).all()  # (rows behind the last one are not written)
    assert all(o.guards_intact() for o in outs.values())
    return len(events)


@readers(3)
@pytest.mark.parametrize("encoding", ["ascii", "codes"])
def test_truth_and_events(run, encoding):
    assert _truth(run, 0, run.call.n, encoding, shift=3) == S.LEDGER[run.name]["rows"]


@readers(3)
def test_truth_and_events_of_a_window(run):
    """A window whose ends are no multiple of 64 (on the batch it reaches over both seams)."""
    first, n = S.windows(run.call)[1]
    assert 0 < _truth(run, first, n, "ascii", shift=9) < S.LEDGER[run.name]["rows"]


# ---------------------------------------------------------------------------------------------------- reader 4: error tally
def _error_tally(run, windows):
    from insilicoseq_amd import errtally as E

    L = run.call.RL
    assert run.eng.error_tally_words() == E.words(L)
    buf = _guarded(E.words(L) * 8, np.uint64, (E.words(L),), zero=True)
    torch.cuda.synchronize()
    for first, n in windows:
        run.eng.error_tally(first, n, buf.ptr, source=run.source)
    run.eng.synchronize()
    assert buf.guards_intact()
    return buf.value().copy()


def _assert_fields(got, want, split, fields):
    bad = [name for name in fields if not np.array_equal(split(got)[name], split(want)[name])]
    assert not bad and np.array_equal(got, want), "fields that differ: %s" % bad


@readers(4)
def test_error_tally(run):
    from insilicoseq_amd import errtally as E

    call = run.call
    got = _error_tally(run, [(0, call.n)])
    t = E.split(got, call.RL)
    assert t["dropped"][0] == 0 and t["pairs"][0] == call.n
    assert int(t["sub_q"].sum()) == S.LEDGER[run.name]["by type"][0]  # the reader saw every substitution row
    _assert_fields(got, S.error_tally(call, 0, call.n), lambda w: E.split(w, call.RL), E.FIELDS)


@readers(4)
def test_error_tally_over_three_windows(run):
    from insilicoseq_amd import errtally as E

    call, wins = run.call, S.windows(run.call)
    split = lambda w: E.split(w, call.RL)  # noqa: E731
    for first, n in wins:
        _assert_fields(_error_tally(run, [(first, n)]), S.error_tally(call, first, n), split, E.FIELDS)
    _assert_fields(_error_tally(run, wins), S.error_tally(call, 0, call.n), split, E.FIELDS)  # the windows sum to the whole


# ---------------------------------------------------------------------------------------------------- reader 5: read tally
@readers(5)
def test_read_tally(run):
    from insilicoseq_amd.tally import FIELDS, split_tally, tally_words

    call, eng = run.call, run.eng
    words = eng.tally_words()
    assert words == tally_words(call.RL)
    buf = _guarded(words * 8, np.uint64, (words,), zero=True)
    torch.cuda.synchronize()
    eng.tally(0, call.n, buf.ptr)
    eng.synchronize()
    assert buf.guards_intact()
    _assert_fields(buf.value(), S.read_tally(call), lambda w: split_tally(w, call.RL), FIELDS)


# ---------------------------------------------------------------------------------------------------- reader 6: depth
@readers(6)
def test_depth(run):
    call, eng = run.call, run.eng
    table, n_words, diff, depth, stats, bins = S.depth(call)
    d_table, d_diff = _device(table), _guarded(4 * n_words, np.int32, (n_words,), zero=True)
    d_depth, d_stats = Guarded(4 * n_words, np.uint32, (n_words,), shift=4), Guarded(32 * len(table), np.uint64, (len(table), 4))
    d_bins = Guarded(8 * len(bins), np.uint64, (len(bins),))
    torch.cuda.synchronize()
    eng.depth_mark(0, call.n, d_table.ptr, len(table), d_diff.ptr)
    eng.synchronize()
    assert np.array_equal(d_diff.value(), diff)
    eng.depth_finish(d_diff.ptr, n_words, d_depth.ptr, d_table.ptr, len(table), S.DEPTH_BIN, d_stats.ptr, d_bins.ptr)
    eng.synchronize()
    assert np.array_equal(d_depth.value(), depth) and np.array_equal(d_stats.value(), stats) and np.array_equal(d_bins.value(), bins)
    assert np.array_equal(d_diff.value(), diff) and np.array_equal(d_table.value(), table)
    assert all(g.guards_intact() for g in (d_table, d_diff, d_depth, d_stats, d_bins))


# ---------------------------------------------------------------------------------------------------- reader 7: origins
def _origins(run, path, compress):
    eng = run.eng
    eng.origins_compress(compress)
    try:
        return _appended(path, lambda fd: eng.origins_emit_batch(fd, run.call.items, run.call.lengths, S.CPU), eng.origins_flush)
    finally:
        eng.origins_flush()
        eng.origins_compress(False)


@readers(7)
def test_origins_text(run, tmp_path):
    _same(_origins(run, str(tmp_path / "o.bedpe"), False), S.origins_text(run.call), "origins text")


@readers(7)
def test_origins_bgzf(run, tmp_path):
    want = S.origins_text(run.call)
    assert S.bgzf_members(_origins(run, str(tmp_path / "o.bedpe.gz"), True), want) == -(-len(want) // S.BGZF_BLOCK)


# ---------------------------------------------------------------------------------------------------- reader 8: FASTQ
def _fastq(run, tmp_path, compress):
    eng, items = run.eng, run.call.items
    paths = [str(tmp_path / ("r%d.fq" % m)) for m in (1, 2)]
    front = b"" if compress else FRONT  # (text is appended behind what the files hold; gzip members start a file)
    eng.fastq_compress(compress)
    try:
        with open(paths[1], "wb") as f2:
            f2.write(front)
            f2.flush()

            def emit(fd):
                if run.kind == "batch":
                    eng.fastq_emit_batch(fd, f2.fileno(), items, S.CPU)
                else:
                    rid, first_i, row, n = items[0]
                    eng.fastq_emit(fd, f2.fileno(), rid, first_i, S.CPU, row, n, n_threads=2)

            first = _appended(paths[0], emit, eng.fastq_flush, stands_at_end=False, front=front)
    finally:
        eng.fastq_flush()
        eng.fastq_compress(False)
    second = open(paths[1], "rb").read()
    assert second[:len(front)] == front
    return [first, second[len(front):]]


@readers(8)
def test_fastq_text(run, tmp_path):
    want = S.fastq_texts(run.call)
    assert len(want[0]) == S.LEDGER[run.name]["fastq bytes of mate 1"]
    got = _fastq(run, tmp_path, False)
    for m in (0, 1):
        _same(got[m], want[m], "FASTQ text of mate %d" % (m + 1))


@readers(8)
def test_fastq_gzip(run, tmp_path):
    want = S.fastq_texts(run.call)
    got = _fastq(run, tmp_path, True)
    for m in (0, 1):
        assert got[m][:4] == b"\x1f\x8b\x08\x00" and len(got[m]) < len(want[m]) // 2
        _same(gzip.decompress(got[m]), want[m], "gunzipped FASTQ of mate %d" % (m + 1))  # (CRC-32 and ISIZE of every member verified)


# ---------------------------------------------------------------------------------------------------- reader 9: uBAM
@readers(9)
def test_ubam(run, tmp_path):
    import ubam_twin as U

    call, eng = run.call, run.eng
    raw = _appended(str(tmp_path / "u.bam"), lambda fd: eng.ubam_emit_batch(fd, call.items, S.CPU), eng.ubam_flush)
    want = S.ubam_records(call)
    data = b"".join(S.bgzf_inflate(raw))
    parsed = U.parse_records(data)  # (field by field, independent of records())
    assert len(parsed) == 2 * call.n
    names = [b"%s_%d_%d" % (rid.encode(), first_i + k, S.CPU) for rid, first_i, _row, n in call.items for k in range(n)]
    assert [p[0] for p in parsed[0::2]] == names and [p[0] for p in parsed[1::2]] == names
    assert {p[1] for p in parsed[0::2]} == {77} and {p[1] for p in parsed[1::2]} == {141}
    assert np.array_equal(np.stack([p[3] for p in parsed]).reshape(call.n, 2, call.RL), call.qual)
    expected = U.parse_records(want)
    assert [p[2] for p in parsed] == [p[2] for p in expected]
    _same(data, want, "uBAM records")


# ---------------------------------------------------------------------------------------------------- reader 10: dense tensors
@readers(10)
@pytest.mark.parametrize("encoding", ["ascii", "codes"])
def test_export(run, encoding):
    from insilicoseq_amd.tensors import recode

    call, eng = run.call, run.eng
    n, RL = call.n, call.RL
    outs = {"bases": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), 5), "qual": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), 11),
            "coords": Guarded(n * 32, np.int64, (n, 4)), "item": Guarded(n * 4, np.int32, (n,))}
    torch.cuda.synchronize()
    eng.export(0, n, *[outs[k].ptr for k in ("bases", "qual", "coords", "item")], encoding=encoding)
    eng.synchronize()
    want = {"bases": call.bases if encoding == "ascii" else recode(call.bases), "qual": call.qual, "coords": call.coords, "item": call.item}
    for k, o in outs.items():
        assert o.guards_intact(), k
        bad = np.argwhere(o.value() != want[k])
        assert bad.size == 0, "export %s differs at %s ... (%d cells)" % (k, bad[:5].tolist(), len(bad))
