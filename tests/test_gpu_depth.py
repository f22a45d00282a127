"""Per-base coverage depth built on the device (ReadEngine.depth_mark / depth_finish: the k_depth_* kernels) against the numpy
twins (insilicoseq_amd.depth.mark_host / finish_host) applied to export() / coords() of the same rows, word for word: windows,
models, contention, batch and MT rows, geometry-changing inputs, tile edges of the scan, its modes, launch geometries, error
paths, ReadTensorStream(depth=True) and `generate --depth`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

from helpers import Guarded, dense_model, mixed_genome, random_genome
from insilicoseq_amd import depth as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4096  # ISS_DEPTH_TILE_WORDS
N_ROWS = 7 + 257
RECORD = 40000


def test_tile_constant_is_the_header_s():
    text = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    assert "#define ISS_DEPTH_TILE_WORDS %d\n" % T in text


def _model(name):
    from insilicoseq_amd.model import DenseModel

    return DenseModel.basic(int(name[5:])) if name.startswith("basic") else dense_model(name)


def _device(array, shift=0):
    """A numpy array in a guarded device block."""
    a = np.ascontiguousarray(array)
    g = Guarded(a.nbytes, a.dtype, a.shape, shift=shift)
    if a.nbytes:
        g.buf[g.at:g.at + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()  # (filled on torch's stream, the engine works on its own)
    return g


def _zeros(n, dtype=np.int32, shift=0):
    return _device(np.zeros(n, dtype=dtype), shift)


_state = {}


def _rows(name, length=RECORD, fragment=None, gc_bias=False, sequence_type="metagenomics", n=N_ROWS):
    """One engine per setting with ``n`` generated rows on one record -- over rows of another seed -- and their coordinates."""
    key = (name, length, fragment, gc_bias, sequence_type, n)
    if key not in _state:
        from insilicoseq_amd.engine import ReadEngine

        eng = ReadEngine(0)
        eng.load_model(_model(name))
        gid = eng.add_genome(mixed_genome(71, length))
        eng.generate(gid, n, first_ordinal=900, seed=99)
        if fragment is not None:
            eng.set_fragment(*fragment)
        eng.generate(gid, n, first_ordinal=3, seed=1234, gc_bias=gc_bias, sequence_type=sequence_type)
        eng.synchronize()
        _state[key] = (eng, eng.coords(0, n), length)
    return _state[key]


def teardown_module(module):
    for eng, _c, _l in _state.values():
        eng.close()
    _state.clear()


def _mark(eng, windows, table, n_words, diff=None):
    """depth_mark of every window into one zeroed guarded accumulator -> its words."""
    d_table = _device(np.asarray(table, dtype=np.int64))
    diff = diff or _zeros(n_words)
    for first, n in windows:
        eng.depth_mark(first, n, d_table.ptr, len(table), diff.ptr)
    eng.synchronize()
    assert diff.guards_intact() and d_table.guards_intact()
    assert np.array_equal(d_table.value(), table)
    return diff.value().copy()


def _twin(coords, item, table, n_words, read_length):
    return D.mark_host(np.zeros(n_words, dtype=np.int32), coords, item, table, read_length)


@pytest.mark.parametrize("first_pair", [0, 7])
@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["novaseq", "miseq", "basic32"])
def test_mark_equals_twin(name, n_pairs, first_pair):
    eng, coords, length = _rows(name)
    assert eng.read_length == {"novaseq": 151, "miseq": 301, "basic32": 32}[name]
    table, n_words = D.depth_table([length])
    got = _mark(eng, [(first_pair, n_pairs)], table, n_words)
    exp = _twin(coords[first_pair:first_pair + n_pairs], 0, table, n_words, eng.read_length)
    assert np.array_equal(got, exp)
    assert got.sum() == 0 and (got > 0).sum() > 0
    # rows of the other seed under the window differ: the window is the one asked for
    assert first_pair == 0 or not np.array_equal(exp, _twin(coords[:n_pairs], 0, table, n_words, eng.read_length))


def test_content_is_present():
    eng, coords, length = _rows("novaseq", length=2000)
    table, n_words = D.depth_table([length])
    depth, stats, _ = D.finish_host(_mark(eng, [(0, N_ROWS)], table, n_words), table)
    assert depth.max() >= 2 and stats[0, 3] == depth.max()
    # amplicon: the template is the whole record -- its first and last read-length bases are covered
    eng, coords, length = _rows("novaseq", sequence_type="amplicon")
    table, n_words = D.depth_table([length])
    got = _mark(eng, [(0, 64)], table, n_words)
    assert np.array_equal(got, _twin(coords[:64], 0, table, n_words, 151))
    depth = D.finish_host(got, table)[0]
    assert depth[:151].any() and depth[length - 151:length].any() and not depth[151:length - 151].any()
    # a record of read length + 1 bases, amplicon: every reverse interval ends at len -- the sink takes a -1 per pair
    eng, coords, length = _rows("novaseq", length=152, sequence_type="amplicon", n=40)
    assert (coords[:, 2] == length).all()
    table, n_words = D.depth_table([length])
    got = _mark(eng, [(0, 40)], table, n_words)
    assert got[length] == -40 and np.array_equal(got, _twin(coords, 0, table, n_words, 151))


def test_contention():
    eng, coords, length = _rows("novaseq", length=2000, n=20000)
    table, n_words = D.depth_table([length])
    got = _mark(eng, [(0, 20000)], table, n_words)
    assert np.array_equal(got, _twin(coords, 0, table, n_words, 151))
    assert D.finish_host(got, table)[1][0, 3] >= 1000


def _export(eng, first, n):
    """(coords, item) of rows [first, +n) by the export kernel."""
    c, it = _zeros(4 * n, np.int64), _zeros(n, np.int32)
    eng.export(first, n, coords_ptr=c.ptr, item_ptr=it.ptr)
    eng.synchronize()
    assert c.guards_intact() and it.guards_intact()
    return c.value().reshape(n, 4).copy(), it.value().copy()


def test_batch_and_mt_rows():
    from insilicoseq_amd.engine import ReadEngine

    rng = np.random.RandomState(5)
    lengths = rng.randint(152, 401, size=300).tolist() + [3 * T + 5]
    seqs = [random_genome(1000 + k, n) for k, n in enumerate(lengths)]
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        gids = eng.add_genomes(seqs)
        gids = [g if g >= 0 else eng.add_genome(s) for g, s in zip(gids, seqs)]
        # the accumulator holds the records in ANOTHER order than the items name them
        order = rng.permutation(len(lengths))
        layout, n_words = D.depth_table([lengths[k] for k in order])
        row_of = np.empty(len(lengths), dtype=np.int64)
        row_of[order] = np.arange(len(lengths))
        counts = rng.randint(0, 6, size=len(lengths)).tolist()
        counts[-1], counts[0] = 400, 3
        n = sum(counts)
        eng.reserve(n + 9)
        eng.generate(gids[-1], n + 9, seed=3)  # (every row holds something)
        eng.generate_batch(gids, counts, first_ordinal=11, seed=5, out_first_pair=4)
        table = layout[row_of].copy()  # row k: the record of item k
        table[17, 0] = -1              # one item is not wanted
        assert counts[17] > 0
        coords, item = _export(eng, 4, n)
        assert set(item.tolist()) == set(k for k, c in enumerate(counts) if c) and (coords[:, 0] >= 0).all()
        diff = _zeros(n_words)
        got = _mark(eng, [(4, n)], table, n_words, diff)
        exp = _twin(coords, item, table, n_words, 151)
        assert np.array_equal(got, exp) and got.any()
        off17 = layout[row_of[17]]
        assert not got[off17[0]:off17[0] + off17[1] + 1].any()
        # a window that starts in front of the call's rows and ends inside them: the rows in front are item 0's of an older call
        with pytest.raises(Exception):
            eng.depth_mark(0, n, _device(table[:5]).ptr, 5, diff.ptr)  # fewer rows than the call has items
        # a second call naming other records, into the same accumulator
        pick = [300, 7, 250, 8]
        eng.generate_batch([gids[k] for k in pick], [50, 20, 0, 30], first_ordinal=2000, seed=6, out_first_pair=0)
        coords2, item2 = _export(eng, 0, 100)
        table2 = layout[row_of[pick]]
        got2 = _mark(eng, [(0, 60), (60, 40)], table2, n_words, diff)
        exp2 = D.mark_host(exp.copy(), coords2, item2, table2, 151)
        assert np.array_equal(got2, exp2)
        # generate_mt rows: item 0
        eng.seed_mt(17)
        assert eng.generate_mt(gids[-1], 64) == 64
        eng.synchronize()
        table3 = layout[row_of[[300]]]
        got3 = _mark(eng, [(0, 64)], table3, n_words, diff)
        assert np.array_equal(got3, D.mark_host(exp2.copy(), eng.coords(0, 64), 0, table3, 151))
        for off, ln in layout.tolist():
            assert got3[off:off + ln + 1].sum() == 0


def test_geometry_changing_inputs():
    eng, coords, length = _rows("novaseq", gc_bias=True)
    table, n_words = D.depth_table([length])
    assert np.array_equal(_mark(eng, [(3, 200)], table, n_words), _twin(coords[3:203], 0, table, n_words, 151))
    # custom fragments of 300 +- 200 on 700 bases: negative inserts (the reads overlap) and reverse reads redrawn at random
    eng, coords, length = _rows("novaseq", length=700, fragment=(300, 200))
    fs, rs, re, isz = coords.T
    assert (rs < fs + 151).any()
    assert (re != fs + 2 * 151 + isz).any()
    table, n_words = D.depth_table([length])
    got = _mark(eng, [(0, N_ROWS)], table, n_words)
    assert np.array_equal(got, _twin(coords, 0, table, n_words, 151)) and got.sum() == 0


# ---------------------------------------------------------------------------------------------------- depth_finish
def _layout(n_words, first=(), seed=0, skip=()):
    """A table that fills ``n_words`` exactly: records of ``first`` lengths, then records of 5 .. 15 bases (hundreds in a tile);
    its difference array from random intervals of 5-base reads, some outside the records, and a crowd on the first record."""
    rng = np.random.RandomState(seed)
    lengths = list(first)
    room = n_words - sum(x + 1 for x in lengths)
    assert room >= 0
    while room:
        x = int(rng.randint(5, 16))
        if room - (x + 1) < 7:
            x = room - 1
        lengths.append(x)
        room -= x + 1
    table, total = D.depth_table(lengths)
    assert total == n_words
    for k in skip:
        table[k, 0] = -1
    item = rng.randint(0, len(lengths), size=n_words // 2)
    item[:500] = 0  # a crowd on the first record
    ln = table[item, 1]
    fs = (rng.random_sample(item.shape) * (ln + 8)).astype(np.int64) - 4
    re = (rng.random_sample(item.shape) * (ln + 8)).astype(np.int64) - 4
    fs[:500], re[:500] = 1, 6  # (the crowd stands on one spot: bases 1 .. 4 of the first record are 1 000 deep)
    coords = np.stack([fs, re - 5, re, re - fs], axis=1)
    diff = D.mark_host(np.zeros(n_words, dtype=np.int32), coords, item, table, 5)
    return table, diff


LAYOUTS = {
    "T-1": dict(n_words=T - 1),
    "T": dict(n_words=T),
    "T+1": dict(n_words=T + 1, first=(T,)),              # one record; its sink is the first word of the second tile
    "2T+1": dict(n_words=2 * T + 1, first=(300, T - 301)),  # the second record's sink is the first word of the second tile
    "3T+100": dict(n_words=3 * T + 100, first=(100, 2 * T + 500), skip=(2,)),  # a record over three tiles; a skipped row
}


def _bare():
    if "bare" not in _state:
        from insilicoseq_amd.engine import ReadEngine

        _state["bare"] = (ReadEngine(0), None, None)  # no model, no genome
    return _state["bare"][0]


def _finish(table, diff, bin, in_place=False, want=("depth", "stats", "bins"), shift=0):
    eng = _bare()
    n_words, n_table = diff.shape[0], table.shape[0]
    exp_depth, exp_stats, exp_bins = D.finish_host(diff, table, bin)
    d_diff, d_table = _device(diff, shift), _device(table)
    d_depth = d_diff if in_place else Guarded(4 * n_words, np.uint32, (n_words,), shift=shift)
    d_stats = Guarded(32 * n_table, np.uint64, (n_table, 4))
    n_bins = int(D.n_windows(table, bin).sum())
    d_bins = Guarded(8 * n_bins, np.uint64, (n_bins,))
    eng.depth_finish(d_diff.ptr, n_words, d_depth.ptr if "depth" in want else None, d_table.ptr, n_table, bin,
                     d_stats.ptr if "stats" in want else None, d_bins.ptr if "bins" in want else None)
    eng.synchronize()
    for g in (d_diff, d_table, d_depth, d_stats, d_bins):
        assert g.guards_intact()
    assert np.array_equal(d_table.value(), table)
    if "depth" in want:
        assert np.array_equal(d_depth.value().view(np.uint32), exp_depth)
    else:
        assert in_place or d_depth.untouched()
    if not (in_place and "depth" in want):
        assert np.array_equal(d_diff.value(), diff)
    if "stats" in want:
        assert np.array_equal(d_stats.value(), exp_stats)
    else:
        assert d_stats.untouched()
    if "bins" in want and bin:
        assert np.array_equal(d_bins.value(), exp_bins)
        assert exp_bins.sum() == exp_stats[:, 0].sum()
    else:
        assert d_bins.untouched()
    return exp_depth, exp_stats


@pytest.mark.parametrize("bin", [0, 1, 7, 1024])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_finish_sizes(name, bin):
    table, diff = _layout(seed=len(name), **LAYOUTS[name])
    depth, stats = _finish(table, diff, bin)
    assert stats[0, 3] >= 1000 and depth.max() == stats[:, 3].max()
    if name == "T+1":
        assert table.shape[0] == 1 and table[0, 0] + table[0, 1] == T
    if name == "2T+1":
        assert table[1, 0] + table[1, 1] == T
    if name == "3T+100":
        assert table[1, 0] < T and table[1, 0] + table[1, 1] > 2 * T and (table[:, 0] < 0).sum() == 1
    if name == "T":
        assert table.shape[0] > 300


@pytest.mark.parametrize("bin", [0, 7])
def test_finish_modes(bin):
    table, diff = _layout(seed=9, **LAYOUTS["3T+100"])
    _finish(table, diff, bin, in_place=True)
    for leave_out in ("depth", "stats", "bins"):
        _finish(table, diff, bin, want=tuple(w for w in ("depth", "stats", "bins") if w != leave_out))
    _finish(table, diff, bin, in_place=True, want=("stats",))  # nothing written to the array
    _finish(table, diff, bin, shift=4)                         # not 16-byte aligned: the 4-byte path
    _finish(table, diff, bin, in_place=True, shift=8)


@pytest.mark.parametrize("wgs", ["1", "3", "7", "64", "100000"])
def test_launch_geometry(wgs, monkeypatch):
    monkeypatch.setenv("ISS_DEPTH_WGS", wgs)
    eng, coords, length = _rows("novaseq")
    table, n_words = D.depth_table([length])
    assert np.array_equal(_mark(eng, [(7, 257)], table, n_words), _twin(coords[7:264], 0, table, n_words, 151))
    table, diff = _layout(seed=9, **LAYOUTS["3T+100"])
    _finish(table, diff, 7)
    _finish(table, diff, 1)


def test_errors_launch_nothing():
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import EngineError

    eng, _coords, length = _rows("basic32")
    table, n_words = D.depth_table([length])
    d_table, diff = _device(table), _zeros(n_words)
    zero = diff.buf.cpu().numpy().copy()
    for first, n, tp, nt, dp in ((N_ROWS - 1, 2, d_table.ptr, 1, diff.ptr), (-1, 2, d_table.ptr, 1, diff.ptr), (0, -1, d_table.ptr, 1, diff.ptr),
                                 (N_ROWS, 1, d_table.ptr, 1, diff.ptr), (0, 4, None, 1, diff.ptr), (0, 4, d_table.ptr, 1, None),
                                 (0, 4, d_table.ptr, 0, diff.ptr)):
        with pytest.raises(EngineError) as e:
            eng.depth_mark(first, n, tp, nt, dp)
        assert e.value.code == _native.E_INVALID
    eng.depth_mark(0, 0, d_table.ptr, 1, diff.ptr)  # no pairs: fine, nothing added
    eng.depth_mark(N_ROWS, 0, None, 0, None)
    bare = _bare()
    with pytest.raises(EngineError) as e:
        bare.depth_mark(0, 1, d_table.ptr, 1, diff.ptr)  # no model, no rows
    assert e.value.code == _native.E_INVALID
    out, stats = Guarded(4 * n_words, np.uint32, (n_words,)), Guarded(32, np.uint64, (1, 4))
    for args in ((diff.ptr, -1, out.ptr, d_table.ptr, 1, 0, stats.ptr, None), (None, n_words, out.ptr, d_table.ptr, 1, 0, stats.ptr, None),
                 (diff.ptr, n_words, out.ptr, None, 1, 0, stats.ptr, None), (diff.ptr, n_words, out.ptr, d_table.ptr, -1, 0, stats.ptr, None),
                 (diff.ptr, n_words, out.ptr, d_table.ptr, 1, -2, stats.ptr, None)):
        with pytest.raises(EngineError) as e:
            bare.depth_finish(*args)
        assert e.value.code == _native.E_INVALID
    bare.depth_finish(diff.ptr, n_words, None, d_table.ptr, 1, 0, None, None)  # nothing wanted: fine
    eng.synchronize()
    bare.synchronize()
    assert np.array_equal(diff.buf.cpu().numpy(), zero) and out.untouched() and stats.untouched()


# ---------------------------------------------------------------------------------------------------- the stream
RECORDS = None
WORK = [(0, 300), (1, 50), (2, 0), (0, 57), (3, 643)]  # record 1 is shorter than a read: skipped; record 2 has no pairs


def _records():
    global RECORDS
    if RECORDS is None:
        RECORDS = [mixed_genome(101, 6000), random_genome(102, 120), random_genome(104, 700), random_genome(103, 9000)]
    return RECORDS


def test_stream_depth_does_not_depend_on_batch_pairs():
    from insilicoseq_amd.tensors import ReadTensorStream

    dense = dense_model("novaseq")
    recs = _records()
    seen = []
    for batch_pairs in (1, 64, 333, 4096):
        with ReadTensorStream(recs, dense, WORK, batch_pairs, seed=77, depth=True) as stream:
            assert stream.depth_diff.dtype == torch.int32 and stream.depth_table.dtype == torch.int64
            table = stream.depth_table.cpu().numpy()
            assert table[:, 1].tolist() == [6000, 120, 700, 9000] and table[1, 0] == -1 and (table[[0, 2, 3], 0] >= 0).all()
            assert stream.depth_diff.shape[0] == 6001 + 701 + 9001
            batches = list(stream)
            got = stream.depth_diff.cpu().numpy()  # (the copy is ordered behind the marks on the stream)
            coords, record = (torch.cat([getattr(b, f) for b in batches]).cpu().numpy() for f in ("coords", "record"))
            assert coords.shape == (1000, 4)
            exp = D.mark_host(np.zeros_like(got), coords, record, table, 151)
            assert np.array_equal(got, exp)
            if batch_pairs == 333:
                for bin in (0, 100):
                    out = stream.depth(bin)
                    e_depth, e_stats, e_bins = D.finish_host(exp, table, bin)
                    assert out[0].dtype == torch.uint32 and np.array_equal(out[0].cpu().numpy(), e_depth)
                    assert np.array_equal(out[1].cpu().numpy(), e_stats) and e_stats[2].tolist() == [0, 0, 0, 0]
                    assert len(out) == (3 if bin else 2) and (not bin or np.array_equal(out[2].cpu().numpy(), e_bins))
                assert np.array_equal(stream.depth_diff.cpu().numpy(), exp)  # not in place
        seen.append(got)
    assert all(np.array_equal(seen[0], s) for s in seen[1:])
    with ReadTensorStream(recs, dense, WORK, 400, seed=77) as plain:
        assert plain.depth_diff is None and plain.depth_table is None and len(list(plain)) == 3
        with pytest.raises(Exception):
            plain.depth()


def test_stream_order_without_synchronisation():
    """A mark followed at once by generation into the same rows, nothing waited for in between."""
    from insilicoseq_amd.engine import ReadEngine

    n = 1 << 16
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        gid = eng.add_genome(random_genome(111, 200000))
        table, n_words = D.depth_table([200000])
        eng.generate(gid, n, seed=1)
        eng.synchronize()
        exp = _twin(eng.coords(0, n), 0, table, n_words, 151)
        eng.generate(gid, n, seed=9)  # (other rows in between)
        d_table, diff = _device(table), _zeros(n_words)
        eng.generate(gid, n, seed=1)
        eng.depth_mark(0, n, d_table.ptr, 1, diff.ptr)
        eng.generate(gid, n, seed=2)  # the rows are written anew right behind the mark
        eng.synchronize()
        assert np.array_equal(diff.value(), exp) and diff.guards_intact()


# ---------------------------------------------------------------------------------------------------- the command line
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def _reads(path):
    lines = open(path, "rb").read().split(b"\n")
    return [(h[1:].decode(), s) for h, s in zip(lines[0::4], lines[1::4]) if h]


@pytest.mark.parametrize("rng_mode", [[], ["--rng", "mt"]])
@pytest.mark.parametrize("workers", [["--gpus", "1"], ["--gpus", "2", "--devices", "1"]])
def test_generate_depth(tmp_path, workers, rng_mode):
    ids = ["rec0", "rec1", "rec2"]
    seqs = [random_genome(131 + k, 5000 + 1000 * k).encode() for k in range(3)]
    fasta = str(tmp_path / "genomes.fasta")
    with open(fasta, "w") as fh:
        for rid, s in zip(ids, seqs):
            fh.write(">%s\n%s\n" % (rid, s.decode()))
    outs = {}
    for tag, extra in (("depth", ["--depth", "--depth_bin", "100"]), ("plain", [])):
        out = str(tmp_path / tag)
        subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--mode", "perfect", "-n", "2000",
                        "--seed", "5", "--output", out] + workers + rng_mode + extra, cwd=ROOT, check=True, timeout=600)
        outs[tag] = out
    for suffix in ("_R1.fastq", "_R2.fastq"):
        assert open(outs["depth"] + suffix, "rb").read() == open(outs["plain"] + suffix, "rb").read()
    assert not os.path.exists(outs["plain"] + "_depth.txt") and not os.path.exists(outs["plain"] + "_depth.bedgraph")
    assert not [f for f in os.listdir(str(tmp_path)) if ".iss.tmp." in f]
    # the expected depth, built without the engine's coordinates: every read is found in the record its id names, once
    table, n_words = D.depth_table([len(s) for s in seqs])
    diff = np.zeros(n_words, dtype=np.int32)
    n_reads, cpus = 0, {rid: set() for rid in ids}
    for mate, suffix in ((1, "_R1.fastq"), (2, "_R2.fastq")):
        for header, read in _reads(outs["depth"] + suffix):
            name, _i, tail = header.rsplit("_", 2)
            assert tail.endswith("/%d" % mate) and len(read) == 125
            cpus[name].add(int(tail.split("/")[0]))
            k = ids.index(name)
            want = read if mate == 1 else read.translate(_COMPLEMENT)[::-1]
            at = seqs[k].find(want)
            assert at >= 0 and seqs[k].find(want, at + 1) == -1, header
            diff[table[k, 0] + at] += 1
            diff[table[k, 0] + at + len(read)] -= 1
            n_reads += 1
    assert n_reads == 2000
    if len(workers) > 2:  # a record split across the two workers' chunks
        assert any(c == {0, 1} for c in cpus.values())
    _depth, stats, bins = D.finish_host(diff, table, 100)
    assert stats[:, 0].sum() == 2000 * 125
    D.write_depth_table(str(tmp_path / "exp.txt"), D.depth_rows(stats, table, ids))
    D.write_bedgraph(str(tmp_path / "exp.bedgraph"), bins, table, ids, 100)
    assert open(outs["depth"] + "_depth.txt").read() == open(str(tmp_path / "exp.txt")).read()
    assert open(outs["depth"] + "_depth.bedgraph").read() == open(str(tmp_path / "exp.bedgraph")).read()
    lines = open(outs["depth"] + "_depth.txt").read().split("\n")
    assert lines[0].split("\t")[0] == "id" and [x.split("\t")[0] for x in lines[1:4]] == ids
