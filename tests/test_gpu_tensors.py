"""Reads as device tensors: k_rows_export (ReadEngine.export) against the host copy route (download / coords), the item labels
of a batch call, export_tensors' stream order, and ReadTensorStream's contract -- the concatenated batches are one
generate_batch() of the whole work list whatever ``batch_pairs`` is."""
import numpy as np
import pytest
import torch  # noqa: F401  (here, when the module is collected: torch's HIP runtime has to be the process's first -- the engine's
              #  library then binds to it; torch imported behind a ReadEngine would start a second runtime that finds no GPU)

from helpers import Guarded, dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

N_ROWS = 7 + 257  # first_pair 7, 257 pairs: the largest case


def _model(name):
    from insilicoseq_amd.model import DenseModel

    return DenseModel.perfect(125) if name == "perfect" else dense_model(name)


_state = {}


def _rows(name):
    """One engine per model with N_ROWS generated rows, their download and coordinates (made once, left unchanged)."""
    if name not in _state:
        from insilicoseq_amd.engine import ReadEngine

        eng = ReadEngine(0)
        eng.load_model(_model(name))
        gid = eng.add_genome(mixed_genome(71, 40000))
        eng.generate(gid, N_ROWS, first_ordinal=3, seed=1234)
        eng.synchronize()
        d = eng.download(0, N_ROWS)
        ref = {"bases": np.stack([d["r1_base"], d["r2_base"]], axis=1), "qual": np.stack([d["r1_qual"], d["r2_qual"]], axis=1),
               "coords": eng.coords(0, N_ROWS)}
        _state[name] = (eng, ref)
    return _state[name]


def teardown_module(module):
    for eng, _ in _state.values():
        eng.close()
    _state.clear()


def _outputs(n, RL, shift=0):
    return {"bases": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), shift), "qual": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), (shift * 7) % 16),
            "coords": Guarded(n * 32, np.int64, (n, 4)), "item": Guarded(n * 4, np.int32, (n,))}


def _export(eng, first, n, outs, encoding="ascii", want=("bases", "qual", "coords", "item")):
    import torch

    torch.cuda.synchronize()  # (the buffers were filled on torch's stream, the engine works on its own)
    eng.export(first, n, *[outs[k].ptr if k in want else None for k in ("bases", "qual", "coords", "item")], encoding=encoding)
    eng.synchronize()


@pytest.mark.parametrize("first_pair", [0, 7])
@pytest.mark.parametrize("n_pairs", [1, 3, 4, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["novaseq", "basic", "miseq", "perfect"])
def test_export_equals_download(name, n_pairs, first_pair):
    eng, ref = _rows(name)
    RL = eng.read_length
    assert RL == {"novaseq": 151, "basic": 125, "miseq": 301, "perfect": 125}[name]
    outs = _outputs(n_pairs, RL, shift=(n_pairs + first_pair) % 16)
    _export(eng, first_pair, n_pairs, outs, "ascii")
    sl = slice(first_pair, first_pair + n_pairs)
    assert np.array_equal(outs["bases"].value(), ref["bases"][sl])
    assert np.array_equal(outs["qual"].value(), ref["qual"][sl])
    assert np.array_equal(outs["coords"].value(), ref["coords"][sl])
    assert not outs["item"].value().any()
    assert all(o.guards_intact() for o in outs.values())


@pytest.mark.parametrize("name", ["novaseq", "miseq"])
def test_codes(name):
    from insilicoseq_amd.tensors import recode

    eng, ref = _rows(name)  # (the record has lower-case, N and IUPAC letters)
    n = 257
    letters = set(ref["bases"][:n].reshape(-1).tolist())
    assert letters & set(b"acgt") and letters & set(b"Nn") and letters & set(b"RYWSMKHBVDrywsmkhbvd")
    outs = _outputs(n, eng.read_length, shift=5)
    _export(eng, 0, n, outs, "codes")
    codes = outs["bases"].value()
    expect = np.full(256, 4, dtype=np.uint8)
    for k, pair in enumerate(("Aa", "Cc", "Gg", "Tt")):
        expect[[ord(c) for c in pair]] = k
    assert np.array_equal(codes, expect[ref["bases"][:n]]) and np.array_equal(codes, recode(ref["bases"][:n]))
    assert codes.max() == 4 and codes.min() == 0
    assert np.array_equal(outs["qual"].value(), ref["qual"][:n])  # (the phreds are not recoded)
    assert all(o.guards_intact() for o in outs.values())


@pytest.mark.parametrize("shift", [0, 1, 8, 15])
@pytest.mark.parametrize("want", [("bases",), ("qual",), ("coords",), ("item",), (), ("bases", "qual", "coords", "item")])
def test_guard_bytes_and_null_outputs(want, shift):
    eng, ref = _rows("novaseq")
    n, first = 130, 2  # (three tiles, the last one short)
    outs = _outputs(n, eng.read_length, shift)
    _export(eng, first, n, outs, "ascii", want=want)
    for k, o in outs.items():
        assert o.guards_intact(), k
        if k not in want:
            assert (o.buf.cpu().numpy() == 0xA5).all(), "%s was not asked for" % k
        elif k != "item":
            assert np.array_equal(o.value(), ref[k][first:first + n]), k
        else:
            assert not o.value().any()


def test_labels_of_a_batch_call():
    from insilicoseq_amd.engine import ReadEngine

    counts = [5, 0, 130]
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        gids = [eng.add_genome(random_genome(81 + k, 3000 + 500 * k)) for k in range(3)]
        eng.reserve(160)
        eng.generate(gids[0], 160, seed=3)  # (every row holds something)
        eng.generate_batch(gids, counts, first_ordinal=11, seed=5, out_first_pair=3)
        eng.synchronize()
        outs = _outputs(135, eng.read_length)
        _export(eng, 3, 135, outs)
        assert outs["item"].value().tolist() == [0] * 5 + [2] * 130
        coords = eng.coords(3, 135)  # (record coordinates: the arena offsets are taken off)
        assert np.array_equal(outs["coords"].value(), coords)
        assert coords.min() >= 0 and (coords[:5, 2] <= 3000).all() and (coords[5:, 2] <= 4000).all()
        d = eng.download(3, 135)
        assert np.array_equal(outs["bases"].value(), np.stack([d["r1_base"], d["r2_base"]], axis=1))
        # a range that reaches over both ends of the call's rows: rows of the older call are item 0, their coordinates as they are
        outs = _outputs(160, eng.read_length)
        _export(eng, 0, 160, outs)
        assert outs["item"].value().tolist() == [0] * 3 + [0] * 5 + [2] * 130 + [0] * 22
        assert np.array_equal(outs["coords"].value(), eng.coords(0, 160))
        assert all(o.guards_intact() for o in outs.values())


def test_other_generators():
    from insilicoseq_amd.engine import ReadEngine

    n = 64
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("hiseq"))
        gids = [eng.add_genome(random_genome(91 + k, 5000)) for k in range(2)]
        eng.generate_batch(gids, [40, 24], seed=9)  # (a batch first: its item table must not label the later calls' rows)
        for how in ("generate", "generate_mt"):
            if how == "generate":
                eng.generate(gids[1], n, seed=2)
            else:
                eng.seed_mt(17)
                assert eng.generate_mt(gids[1], n) == n
            eng.synchronize()
            outs = _outputs(n, eng.read_length, shift=3)
            _export(eng, 0, n, outs)
            d = eng.download(0, n)
            assert np.array_equal(outs["bases"].value(), np.stack([d["r1_base"], d["r2_base"]], axis=1)), how
            assert np.array_equal(outs["qual"].value(), np.stack([d["r1_qual"], d["r2_qual"]], axis=1)), how
            assert np.array_equal(outs["coords"].value(), eng.coords(0, n)), how
            assert not outs["item"].value().any(), how
            assert all(o.guards_intact() for o in outs.values())


RECORDS = None
WORK = [(0, 300), (1, 50), (2, 0), (0, 57), (2, 643)]  # record 1 is shorter than a read: skipped, 1 000 pairs remain


def _records():
    global RECORDS
    if RECORDS is None:
        RECORDS = [mixed_genome(101, 6000), random_genome(102, 120), random_genome(103, 9000)]
    return RECORDS


@pytest.mark.parametrize("variant", ["plain", "gc_bias", "fragment"])
def test_stream_does_not_depend_on_batch_pairs(variant, caplog):
    import torch
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import ReadTensorStream

    dense = dense_model("novaseq")
    kw = {"gc_bias": variant == "gc_bias"}
    frag = (400.0, 35.0) if variant == "fragment" else (None, None)
    recs = _records()
    # one generate_batch() of the whole list (short record left out), through the host copy route
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gids = eng.add_genomes([recs[0], recs[2]])
        if variant == "fragment":
            eng.set_fragment(*frag)
        eng.generate_batch([gids[0], gids[1], gids[0], gids[1]], [300, 0, 57, 643], first_ordinal=0, seed=77, **kw)
        eng.synchronize()
        d = eng.download(0, 1000)
        ref_bases, ref_qual = np.stack([d["r1_base"], d["r2_base"]], axis=1), np.stack([d["r1_qual"], d["r2_qual"]], axis=1)
        ref_coords = eng.coords(0, 1000)
    ref_record = np.array([0] * 357 + [2] * 643, dtype=np.int32)
    for batch_pairs in (1, 64, 333, 1000, 4096):
        with ReadTensorStream(recs, dense, WORK, batch_pairs, seed=77, encoding="ascii", fragment_length=frag[0], fragment_sd=frag[1],
                              **kw) as stream:
            batches = list(stream)
            assert len(batches) == len(stream) == -(-1000 // batch_pairs)
            assert all(b.bases.shape[0] == batch_pairs for b in batches[:-1])
            got = [torch.cat([getattr(b, f) for b in batches]).cpu().numpy() for f in ("bases", "qual", "coords", "record")]
        assert batches[0].bases.dtype == torch.uint8 and batches[0].coords.dtype == torch.int64 and batches[0].record.dtype == torch.int32
        assert batches[0].bases.device == torch.device("cuda", 0) and tuple(batches[0].bases.shape[1:]) == (2, 151)
        assert np.array_equal(got[0], ref_bases), batch_pairs
        assert np.array_equal(got[1], ref_qual), batch_pairs
        assert np.array_equal(got[2], ref_coords), batch_pairs
        assert np.array_equal(got[3], ref_record), batch_pairs
    assert any("shorter than read length" in r.getMessage() for r in caplog.records)


def test_stream_codes_and_an_empty_work_list():
    import torch
    from insilicoseq_amd.tensors import ReadTensorStream, recode

    dense = dense_model("novaseq")
    recs = _records()
    with ReadTensorStream(recs, dense, WORK, 400, seed=77, encoding="ascii") as a, ReadTensorStream(recs, dense, WORK, 400, seed=77) as c:
        ascii_ = torch.cat([b.bases for b in a]).cpu().numpy()
        codes = torch.cat([b.bases for b in c]).cpu().numpy()
    assert np.array_equal(codes, recode(ascii_)) and codes.max() <= 4
    with ReadTensorStream(recs, dense, [(1, 10), (2, 0)], 8) as empty:
        assert list(empty) == [] and len(empty) == 0


def test_stream_order_without_synchronisation():
    import torch
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import export_tensors

    n = 1 << 16
    with ReadEngine(0) as eng:
        eng.load_model(dense_model("novaseq"))
        gid = eng.add_genome(random_genome(111, 200000))
        # the synchronous route: what the first batch holds
        eng.generate(gid, n, seed=1)
        eng.synchronize()
        d = eng.download(0, n)
        first = np.stack([d["r1_base"], d["r2_base"]], axis=1), np.stack([d["r1_qual"], d["r2_qual"]], axis=1)
        first_coords = eng.coords(0, n)
        expect_sum = int(first[0].astype(np.int64).sum() + first[1].astype(np.int64).sum())
        eng.generate(gid, n, seed=9)  # (other rows in between)
        for stream in (torch.cuda.Stream(device=0), torch.cuda.current_stream(0)):  # a stream of the caller's, torch's default stream
            eng.generate(gid, n, seed=1)
            with torch.cuda.stream(stream):
                batch = export_tensors(eng, 0, n, encoding="ascii")
                total = batch.bases.sum(dtype=torch.int64) + batch.qual.sum(dtype=torch.int64)  # queued behind the export, no wait
            eng.generate(gid, n, seed=2)  # the rows are written anew right behind the export
            torch.cuda.synchronize()
            assert int(total.item()) == expect_sum
            assert np.array_equal(batch.bases.cpu().numpy(), first[0]) and np.array_equal(batch.qual.cpu().numpy(), first[1])
            assert np.array_equal(batch.coords.cpu().numpy(), first_coords)
            assert not batch.record.any().item()
            assert eng.stream_ptr == 0  # (the engine is back on its own stream)
        # ``out``: the caller's tensors are written in place
        eng.generate(gid, 100, seed=1)
        out = export_tensors(eng, 0, 100, encoding="ascii")
        again = export_tensors(eng, 0, 100, encoding="ascii", out=out._replace(coords=None))
        torch.cuda.synchronize()
        assert again.bases.data_ptr() == out.bases.data_ptr() and again.coords is None
        assert np.array_equal(again.bases.cpu().numpy(), first[0][:100])


def test_errors_launch_nothing():
    from insilicoseq_amd.engine import EngineError
    from insilicoseq_amd.tensors import export_tensors

    eng, _ = _rows("basic")
    outs = _outputs(4, eng.read_length)
    cap = N_ROWS  # (the rows reserved by _rows)
    for first, n, enc in ((cap - 1, 2, "ascii"), (-1, 2, "ascii"), (0, -1, "ascii"), (cap, 1, "codes"), (0, 4, "2bit")):
        with pytest.raises(EngineError):
            _export(eng, first, n, outs, enc)
    with pytest.raises(EngineError):
        export_tensors(eng, 0, 4, encoding="2bit")
    with pytest.raises(EngineError):
        export_tensors(eng, cap - 1, 2)
    _export(eng, 0, 0, outs)  # no pairs: fine, nothing written
    for o in outs.values():
        assert (o.buf.cpu().numpy() == 0xA5).all()
