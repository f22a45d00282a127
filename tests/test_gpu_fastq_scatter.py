"""iss_fastq_emit_scatter -- the text job of one round of the worker set: items of several workers, each with its own worker
number and its own byte offset in both files -- against a plain Python formatter of the same rows.  Every file must equal
the image the Python text placed at the items' offsets, byte for byte, and the host formatter (iss_fastq_write) writing the
same items in file order must give the same bytes."""
import os

import numpy as np
import pytest

from helpers import dense_model, random_genome

pytestmark = pytest.mark.gpu

HEAD = b"# attached here\n"  # the files hold this when they are attached: scatter jobs write at absolute offsets after it
N_ROWS = 6000


def _engine(model="hiseq"):
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    eng.load_model(dense_model(model))
    gid = eng.add_genome(random_genome(11, 40000))
    eng.generate(gid, N_ROWS, first_ordinal=0, seed=3)
    eng.synchronize()
    return eng


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _rows(e):
    if not hasattr(e, "_test_rows"):
        d = e.download(0, N_ROWS)
        e._test_rows = (d, [np.ascontiguousarray(d[k]) for k in ("r1_base", "r1_qual", "r2_base", "r2_qual")])
    return e._test_rows


def _py_text(e, rid, first_i, first_pair, n, cpu):
    """The reference's records (iss/generator.py:64-65, 150, 181) of rows [first_pair, +n): one bytes object per mate."""
    _, (b1, q1, b2, q2) = _rows(e)
    out = []
    for mate, (b, q) in enumerate(((b1, q1), (b2, q2))):
        parts = []
        for j in range(n):
            r = first_pair + j
            parts.append(("@%s_%d_%d/%d\n" % (rid, first_i + j, cpu, mate + 1)).encode())
            parts.append(b[r].tobytes())
            parts.append(b"\n+\n")
            parts.append((q[r] + 33).astype(np.uint8).tobytes())
            parts.append(b"\n")
        out.append(b"".join(parts))
    return out


def _layout(e, items, order=None, at=len(HEAD)):
    """(rid, first_i, first_pair, n, cpu) -> scatter items with the offsets of a back-to-back layout in `order` (default:
    list order) starting at `at`, and the end of that layout.  The Python size (fastq_text_bytes) must be the text's."""
    from insilicoseq_amd.generator import fastq_text_bytes

    order = list(range(len(items))) if order is None else order
    off = [None] * len(items)
    for k in order:
        rid, first_i, first_pair, n, cpu = items[k]
        size = fastq_text_bytes(rid, first_i + n, cpu, e.read_length) - fastq_text_bytes(rid, first_i, cpu, e.read_length)
        assert size == len(_py_text(e, rid, first_i, first_pair, n, cpu)[0]), items[k]
        off[k] = at
        at += size
    return [it + (o,) for it, o in zip(items, off)], at


def _run(e, calls, tmp_path, n_threads=1):
    """Each call: one fastq_emit_scatter of its items.  Returns the two files' bytes after fastq_flush and checks the
    flush invariants: the descriptors stand where they were attached, and the files are exactly the expected size."""
    from insilicoseq_amd.engine import fastq_write

    paths = [str(tmp_path / p) for p in ("s1.fq", "s2.fq", "h1.fq", "h2.fq")]
    fh = [open(p, "wb") for p in paths]
    try:
        for f in fh:
            f.write(HEAD)
            f.flush()
        image = [bytearray(HEAD), bytearray(HEAD)]
        for items in calls:
            e.fastq_emit_scatter(fh[0].fileno(), fh[1].fileno(), items, n_threads=n_threads)
            for rid, first_i, first_pair, n, cpu, off in items:
                if n == 0:  # (nothing is written for it, at its offset or anywhere)
                    continue
                for m, t in enumerate(_py_text(e, rid, first_i, first_pair, n, cpu)):
                    if len(image[m]) < off + len(t):
                        image[m].extend(b"\0" * (off + len(t) - len(image[m])))
                    image[m][off:off + len(t)] = t
        e.fastq_flush()
        for m in range(2):  # scatter jobs do not move the file position
            assert os.lseek(fh[m].fileno(), 0, os.SEEK_CUR) == len(HEAD)
        # the host formatter on the same items, one after the other in file order
        d = _rows(e)[0]["_pitched"]
        at = len(HEAD)
        for rid, first_i, first_pair, n, cpu, off in sorted((it for c in calls for it in c if it[3] > 0), key=lambda it: it[5]):
            assert off == at, "the items do not tile the file"
            a, b = first_pair, first_pair + n
            fastq_write(fh[2].fileno(), fh[3].fileno(), rid, first_i, cpu, n, e.read_length, e.pitch, d[0][a:b], d[1][a:b], d[2][a:b],
                        d[3][a:b], n_threads=2)
            at += len(_py_text(e, rid, first_i, first_pair, n, cpu)[0])
    finally:
        for f in fh:
            f.close()
    got = [open(p, "rb").read() for p in paths]
    for m in range(2):
        assert len(got[m]) == len(image[m])
        assert got[m] == bytes(image[m]), "mate %d differs from the Python formatter at byte %d" % (
            m + 1, next(i for i, (x, y) in enumerate(zip(got[m], image[m])) if x != y))
        assert got[2 + m] == got[m], "the host formatter differs (mate %d)" % (m + 1)
    return got


MIXED = [  # (rid, first_i, first_pair, pairs, worker number): widths 1 .. 4, ids of 1 and 4096 bytes
    ("a", 0, 0, 37, 0),
    ("rec_7", 5, 40, 12, 7),            # 9|10 inside the item
    ("x" * 4096, 0, 60, 3, 10),
    ("NZ_CP0001.1", 95, 100, 10, 99),    # 99|100
    ("b", 995, 200, 9, 100),            # 999|1000
    ("c" * 300, 999990, 300, 25, 1023),  # 999999|1000000
    ("a", 0, 400, 1, 9),
    ("a", 0, 401, 2, 11),
]


@pytest.mark.parametrize("threads", [1, 3, 8, "pieces5"])
def test_scatter_mixed_widths(eng, threads, tmp_path, monkeypatch):
    """One call with items of worker numbers 0, 7, 9, 10, 11, 99, 100, 1023 (one to four digits), pair numbers that cross
    9|10, 99|100, 999|1000 and 999999|1000000 inside an item, ids of 1 and 4096 (FASTQ_ID_MAX) bytes."""
    if threads == "pieces5":
        monkeypatch.setenv("ISS_FASTQ_PIECES", "5")  # (overrides the argument)
        threads = 1
    items, _ = _layout(eng, MIXED)
    _run(eng, [items], tmp_path, n_threads=threads)


@pytest.mark.parametrize("order", ["reversed", "interleaved"])
def test_scatter_offsets_out_of_item_order(eng, order, tmp_path):
    """The file order is not the item order: reversed, or interleaved (even items first, then odd)."""
    n = len(MIXED)
    perm = list(range(n))[::-1] if order == "reversed" else list(range(0, n, 2)) + list(range(1, n, 2))
    items, _ = _layout(eng, MIXED, order=perm)
    _run(eng, [items], tmp_path, n_threads=3)


def test_scatter_gap_filled_by_a_later_call(eng, tmp_path):
    """The first call leaves a hole (items 2 and 5 of the layout), the second call fills it."""
    items, _ = _layout(eng, MIXED)
    first = [it for k, it in enumerate(items) if k not in (2, 5)]
    second = [items[5], items[2]]
    _run(eng, [first, second], tmp_path, n_threads=1)


@pytest.mark.parametrize("where", ["first", "middle", "last", "all_but_one"])
def test_scatter_zero_pair_items(eng, where, tmp_path):
    """A zero-pair item writes nothing and takes no offset: the other items still land at theirs.  Its own offset points
    far beyond the files (nothing may be written there: the files stay exactly their expected size)."""
    items, end = _layout(eng, MIXED[:4])
    zero = lambda k: ("zero%d" % k, 50, 1000 + k, 0, 10 + k, end + 4096 * (k + 1))  # noqa: E731
    if where == "first":
        items = [zero(0)] + items
    elif where == "middle":
        items = items[:2] + [zero(0), zero(1)] + items[2:]
    elif where == "last":
        items = items + [zero(0)]
    else:
        items = [zero(0), zero(1), _layout(eng, MIXED[3:4])[0][0], zero(2)]
    _run(eng, [items], tmp_path, n_threads=3)


def test_scatter_rounds_of_a_worker_set(eng, tmp_path):
    """Rounds as worker_set_iterator sends them: per call one piece per worker, a worker's pieces back to back in its own
    region of the files, items split across calls at 9|10 and 99|100."""
    workers = [(0, "g0"), (9, "g1"), (10, "g2"), (100, "g3")]
    per, rounds = [10, 45, 90, 7], 4
    from insilicoseq_amd.generator import fastq_text_bytes

    sizes = []
    for (cpu, rid), p in zip(workers, per):
        sizes.append(fastq_text_bytes(rid, rounds * p, cpu, eng.read_length))
    at = list(np.cumsum([len(HEAD)] + sizes[:-1]))
    calls, row = [], 0
    for r in range(rounds):
        items = []
        for k, ((cpu, rid), p) in enumerate(zip(workers, per)):
            items.append((rid, r * p, row, p, cpu, int(at[k])))
            at[k] += fastq_text_bytes(rid, (r + 1) * p, cpu, eng.read_length) - fastq_text_bytes(rid, r * p, cpu, eng.read_length)
            row += p
        calls.append(items)
    _run(eng, calls, tmp_path, n_threads=8)


def test_scatter_text_buffers_grow_mid_run(tmp_path):
    """A call whose text exceeds the capacity the first call sized (fastq_flush_keep with the first job still queued, free,
    reallocation while the files stay attached), then a smaller call, then a larger one again (a second reallocation)."""
    e = _engine()
    try:
        small, at = _layout(e, [("s", 0, 0, 20, 3), ("t", 20, 20, 20, 12)])
        big, at = _layout(e, [("big%d" % k, 1000 * k, 0, N_ROWS, 10 + k) for k in range(3)], at=at)  # ~5 MB per file
        small2, at = _layout(e, [("u", 7, 5, 30, 99)], at=at)
        bigger, _ = _layout(e, [("huge%d" % k, 0, 0, N_ROWS, 1000 + k) for k in range(7)], at=at)  # ~12 MB per file
        _run(e, [small, big, small2, bigger], tmp_path, n_threads=3)
    finally:
        e.close()


def test_scatter_refused_in_gzip_mode(tmp_path):
    """Scatter is text only (a gzip member's size is not known up front): refused with E_INVALID; after switching back the
    same context formats a text job correctly."""
    from insilicoseq_amd import _native

    e = _engine()
    try:
        items, _ = _layout(e, MIXED[:3])
        e.fastq_compress(True)
        with open(str(tmp_path / "g1"), "wb") as f1, open(str(tmp_path / "g2"), "wb") as f2:
            with pytest.raises(_native.EngineError) as ei:
                e.fastq_emit_scatter(f1.fileno(), f2.fileno(), items)
            assert ei.value.code == _native.E_INVALID
        e.fastq_compress(False)
        _run(e, [items], tmp_path, n_threads=3)
    finally:
        e.close()
