"""Tallies of the output rows built on the device (ReadEngine.tally: k_tally_lines, k_tally_reads) against the numpy twin
(insilicoseq_amd.tally.tally_host) applied to download() + coords() of the same rows, word for word; accumulation, launch
geometry, the stream rule, ReadTensorStream(tally=True) and `generate --report`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

from helpers import Guarded, dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 7 + 257  # first_pair 7, 257 pairs: the largest window
READ_LENGTH = {"novaseq": 151, "miseq": 301, "basic125": 125, "basic32": 32, "basic33": 33, "perfect125": 125}


def _model(name):
    from insilicoseq_amd.model import DenseModel

    if name.startswith("basic"):
        return DenseModel.basic(int(name[5:]))
    if name.startswith("perfect"):
        return DenseModel.perfect(int(name[7:]))
    return dense_model(name)


def _reference(eng, n):
    eng.synchronize()
    d = eng.download(0, n)
    return {"bases": np.stack([d["r1_base"], d["r2_base"]], axis=1), "qual": np.stack([d["r1_qual"], d["r2_qual"]], axis=1),
            "coords": eng.coords(0, n)}


_state = {}


def _rows(name, fragment=None, gc_bias=False):
    """One engine per (model, fragment setting) with N_ROWS generated rows -- over rows of another seed, so that stale bytes
    differ -- and their download and coordinates (made once, left unchanged)."""
    key = (name, fragment, gc_bias)
    if key not in _state:
        from insilicoseq_amd.engine import ReadEngine

        eng = ReadEngine(0)
        eng.load_model(_model(name))
        gid = eng.add_genome(mixed_genome(71, 40000))
        eng.generate(gid, N_ROWS, first_ordinal=900, seed=99)
        if fragment is not None:
            eng.set_fragment(*fragment)
        eng.generate(gid, N_ROWS, first_ordinal=3, seed=1234, gc_bias=gc_bias)
        _state[key] = (eng, _reference(eng, N_ROWS))
    return _state[key]


def teardown_module(module):
    for eng, _ in _state.values():
        eng.close()
    _state.clear()


def _buffer(eng):
    """The tally words in a guarded block, zeroed."""
    words = eng.tally_words()
    g = Guarded(words * 8, np.uint64, (words,))
    g.buf[g.at:g.at + g.nbytes].zero_()
    torch.cuda.synchronize()  # (filled on torch's stream, the engine works on its own)
    return g


def _twin(eng, ref, first, n):
    from insilicoseq_amd.tally import tally_host

    sl = slice(first, first + n)
    return tally_host(ref["bases"][sl], ref["qual"][sl], ref["coords"][sl, 3], eng.read_length)


def _tally(eng, windows, buf=None):
    buf = buf or _buffer(eng)
    for first, n in windows:
        eng.tally(first, n, buf.ptr)
    eng.synchronize()
    assert buf.guards_intact()
    return buf.value().copy()


def _assert_equal(got, exp, L):
    from insilicoseq_amd.tally import split_tally

    a, b = split_tally(got, L), split_tally(exp, L)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("first_pair", [0, 7])
@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["novaseq", "miseq", "basic125", "basic32", "basic33", "perfect125"])
def test_tally_equals_twin(name, n_pairs, first_pair):
    from insilicoseq_amd.tally import split_tally, tally_words

    eng, ref = _rows(name)
    L = eng.read_length
    assert L == READ_LENGTH[name] and eng.tally_words() == tally_words(L)
    got = _tally(eng, [(first_pair, n_pairs)])
    exp = _twin(eng, ref, first_pair, n_pairs)
    assert int(exp[0]) == n_pairs
    _assert_equal(got, exp, L)
    t = split_tally(got, L)
    assert (t["qual"].sum(-1) == n_pairs).all() and (t["base"].sum(-1) == n_pairs).all()
    assert (t["gc"].sum(-1) == n_pairs).all() and (t["meanq"].sum(-1) == n_pairs).all() and t["insert"].sum() == n_pairs


def test_content_is_present():
    """What the comparisons above are meant to exercise is in the rows: letters of code 4 and lower-case ones, several phreds at
    one position, one mean-quality bin for the perfect model."""
    from insilicoseq_amd.tally import split_tally

    eng, ref = _rows("novaseq")
    letters = set(ref["bases"][7:].reshape(-1).tolist())
    assert letters & set(b"acgt") and letters & set(b"NRYWSMKHBVDnrywsmkhbvd")
    t = split_tally(_tally(eng, [(7, 257)]), eng.read_length)
    assert t["base"][:, :, 4].sum() > 0
    assert ((t["qual"] > 0).sum(-1) >= 2).any()
    # rows outside the window and the stale rows under them differ from the window's
    assert not np.array_equal(_twin(eng, ref, 0, 257)[1:], _twin(eng, ref, 7, 257)[1:])
    eng, ref = _rows("perfect125")
    t = split_tally(_tally(eng, [(0, 257)]), 125)
    assert t["meanq"][0, 40] == 257 and t["meanq"][1, 40] == 257 and t["qual"][:, :, 40].sum() == 2 * 125 * 257


def test_accumulation():
    eng, ref = _rows("novaseq")
    L = eng.read_length
    whole = _tally(eng, [(0, 257)])
    _assert_equal(whole, _twin(eng, ref, 0, 257), L)
    _assert_equal(_tally(eng, [(0, 100), (100, 157)]), whole, L)
    _assert_equal(_tally(eng, [(0, 257), (0, 257)]), 2 * whole, L)
    # a run over several calls and engines of one read length: the buffer carries on
    buf = _buffer(eng)
    _tally(eng, [(7, 64)], buf)
    _assert_equal(_tally(eng, [(71, 1)], buf), _twin(eng, ref, 7, 65), L)


@pytest.mark.parametrize("wgs", ["1", "3", "7", "64", "100000"])
def test_launch_geometry(wgs, monkeypatch):
    """ISS_TALLY_WGS: the workgroups a call aims at -- one chunk per line, chunks of 32 pairs, and in between."""
    for name in ("novaseq", "miseq"):
        eng, ref = _rows(name)
        monkeypatch.delenv("ISS_TALLY_WGS", raising=False)
        default = _tally(eng, [(7, 257)])
        monkeypatch.setenv("ISS_TALLY_WGS", wgs)
        _assert_equal(_tally(eng, [(7, 257)]), default, eng.read_length)
        _assert_equal(default, _twin(eng, ref, 7, 257), eng.read_length)


def test_insert_sizes_beyond_the_bins():
    from insilicoseq_amd.tally import split_tally

    eng, ref = _rows("novaseq", fragment=(3000, 10))
    assert (ref["coords"][:257, 3] >= 2048).any()
    got = _tally(eng, [(0, 257)])
    assert split_tally(got, 151)["insert"][2047] == (ref["coords"][:257, 3] >= 2047).sum() > 0
    _assert_equal(got, _twin(eng, ref, 0, 257), 151)
    eng, ref = _rows("novaseq", fragment=(200, 60))  # fragments shorter than two reads: negative inserts
    negative = int((ref["coords"][:257, 3] < 0).sum())
    assert negative > 0
    got = _tally(eng, [(0, 257)])
    assert split_tally(got, 151)["insert"][0] >= negative
    _assert_equal(got, _twin(eng, ref, 0, 257), 151)


def test_gc_bias():
    eng, ref = _rows("novaseq", gc_bias=True)
    _assert_equal(_tally(eng, [(3, 200)]), _twin(eng, ref, 3, 200), 151)


def test_batch_and_mt_rows():
    from insilicoseq_amd.engine import ReadEngine

    with ReadEngine(0) as eng:
        eng.load_model(dense_model("hiseq"))
        gids = [eng.add_genome(mixed_genome(81 + k, 3000 + 500 * k)) for k in range(3)]
        eng.reserve(200)
        eng.generate(gids[0], 200, seed=3)  # (every row holds something)
        eng.generate_batch(gids, [5, 60, 130], first_ordinal=11, seed=5, out_first_pair=2)
        ref = _reference(eng, 200)
        L = eng.read_length
        _assert_equal(_tally(eng, [(2, 195)]), _twin(eng, ref, 2, 195), L)
        _assert_equal(_tally(eng, [(0, 200)]), _twin(eng, ref, 0, 200), L)  # (over both ends of the call's rows)
        plain = eng.add_genome(random_genome(91, 5000))
        eng.seed_mt(17)
        assert eng.generate_mt(plain, 64) == 64
        ref = _reference(eng, 64)
        _assert_equal(_tally(eng, [(0, 64)]), _twin(eng, ref, 0, 64), L)


def test_errors_launch_nothing():
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import EngineError, ReadEngine

    eng, _ = _rows("basic125")
    buf = _buffer(eng)
    zero = buf.buf.cpu().numpy().copy()
    for first, n, ptr in ((N_ROWS - 1, 2, buf.ptr), (-1, 2, buf.ptr), (0, -1, buf.ptr), (N_ROWS, 1, buf.ptr), (0, 4, None)):
        with pytest.raises(EngineError) as e:
            eng.tally(first, n, ptr)
        assert e.value.code == _native.E_INVALID
    eng.tally(0, 0, buf.ptr)  # no pairs: fine, nothing added
    eng.tally(N_ROWS, 0, None)
    eng.synchronize()
    assert np.array_equal(buf.buf.cpu().numpy(), zero)
    with ReadEngine(0) as bare:  # no model
        with pytest.raises(EngineError) as e:
            bare.tally_words()
        assert e.value.code == _native.E_INVALID
        with pytest.raises(EngineError) as e:
            bare.tally(0, 1, buf.ptr)
        assert e.value.code == _native.E_INVALID
    assert np.array_equal(buf.buf.cpu().numpy(), zero)


RECORDS = None
WORK = [(0, 300), (1, 50), (2, 0), (0, 57), (2, 643)]  # record 1 is shorter than a read: skipped, 1 000 pairs remain


def _records():
    global RECORDS
    if RECORDS is None:
        RECORDS = [mixed_genome(101, 6000), random_genome(102, 120), random_genome(103, 9000)]
    return RECORDS


def test_stream_tally_does_not_depend_on_batch_pairs():
    from insilicoseq_amd.tally import tally_host
    from insilicoseq_amd.tensors import ReadTensorStream

    dense = dense_model("novaseq")
    recs = _records()
    seen = []
    for batch_pairs in (1, 64, 333, 4096):
        with ReadTensorStream(recs, dense, WORK, batch_pairs, seed=77, encoding="ascii", tally=True) as stream:
            assert stream.tally.dtype == torch.int64 and stream.tally.device == torch.device("cuda", 0)
            batches = list(stream)
            got = stream.tally.cpu().numpy().view(np.uint64)  # (the copy is ordered behind the tallies on the stream)
            bases, qual, coords = (torch.cat([getattr(b, f) for b in batches]).cpu().numpy() for f in ("bases", "qual", "coords"))
        assert bases.shape == (1000, 2, 151)
        _assert_equal(got, tally_host(bases, qual, coords[:, 3], 151), 151)
        seen.append(got)
    assert all(np.array_equal(seen[0], s) for s in seen[1:])
    with ReadTensorStream(recs, dense, WORK, 400, seed=77) as plain:
        assert plain.tally is None and len(list(plain)) == 3


def test_stream_order_without_synchronisation():
    """A tally followed at once by generation into the same rows, nothing waited for in between."""
    from insilicoseq_amd.engine import ReadEngine

    n = 1 << 16
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        gid = eng.add_genome(random_genome(111, 200000))
        eng.generate(gid, n, seed=1)
        ref = _reference(eng, n)
        exp = _twin(eng, ref, 0, n)
        eng.generate(gid, n, seed=9)  # (other rows in between)
        buf = _buffer(eng)
        eng.generate(gid, n, seed=1)
        eng.tally(0, n, buf.ptr)
        eng.generate(gid, n, seed=2)  # the rows are written anew right behind the tally
        eng.synchronize()
        _assert_equal(buf.value(), exp, 151)
        assert buf.guards_intact()


def _parse_fastq(path):
    lines = open(path, "rb").read().split(b"\n")
    seq = [np.frombuffer(x, dtype=np.uint8) for x in lines[1::4] if x]
    qual = [np.frombuffer(x, dtype=np.uint8) - 33 for x in lines[3::4] if x]
    return np.stack(seq), np.stack(qual)


@pytest.mark.parametrize("workers", [["--gpus", "1"], ["--gpus", "2", "--devices", "1"]])
def test_generate_report(tmp_path, workers):
    from insilicoseq_amd.tally import split_tally, tally_host

    fasta = str(tmp_path / "genomes.fasta")
    with open(fasta, "w") as fh:
        for k in range(3):
            fh.write(">rec%d\n%s\n" % (k, mixed_genome(121 + k, 5000 + 1000 * k)))
    outs = {}
    for tag, extra in (("report", ["--report"]), ("plain", [])):
        out = str(tmp_path / tag)
        subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", "2000",
                        "--seed", "5", "--output", out] + workers + extra, cwd=ROOT, check=True, timeout=600)
        outs[tag] = out
    for suffix in ("_R1.fastq", "_R2.fastq"):
        assert open(outs["report"] + suffix, "rb").read() == open(outs["plain"] + suffix, "rb").read()
    assert not os.path.exists(outs["plain"] + "_tally.npy") and not os.path.exists(outs["plain"] + "_report.json")
    assert not [f for f in os.listdir(str(tmp_path)) if ".iss.tmp." in f]
    words = np.load(outs["report"] + "_tally.npy")
    assert words.dtype == np.uint64
    (b1, q1), (b2, q2) = _parse_fastq(outs["report"] + "_R1.fastq"), _parse_fastq(outs["report"] + "_R2.fastq")
    n = b1.shape[0]
    assert n == 1000 and b1.shape == b2.shape == (n, 151)
    exp = split_tally(tally_host(np.stack([b1, b2], axis=1), np.stack([q1, q2], axis=1), np.zeros(n, dtype=np.int64), 151), 151)
    got = split_tally(words, 151)
    for name in ("qual", "base", "gc", "meanq", "pairs"):
        assert np.array_equal(got[name], exp[name]), name
    assert got["insert"].sum() == n and got["insert"][1:].any()
    report = json.load(open(outs["report"] + "_report.json"))
    assert report["pairs"] == n and report["read_length"] == 151 and sum(report["insert_size_histogram"]) == n
