"""The device's gzip members bit for bit against the host twin (tests/deflate_twin.py).

gzip.decompress(device bytes) == text, which every other --compress test asserts, holds for any stream that still inflates: a
histogram that counts other tokens than the encoder emits (every symbol keeps a code), a code that depends on the number of
lanes that built it, matches that are not found.  Here the file must hold exactly the bytes the twin predicts -- the code of the
whole text's tokens built by iss_deflate_code_build on one host lane, the tokens of deflate_tokens' rule, block by block -- for
the cases of deflate_cases.cases(), whose shapes tests/test_deflate_twin_host.py asserts on the CPU."""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import deflate_cases as K
import deflate_twin as T
import helpers as H

pytestmark = pytest.mark.gpu

CASES = K.cases()


class Rows(object):
    """One engine with ROWS[RL] rows of the sweep's model at RL, and the oracle's arrays for them (left unchanged)."""

    def __init__(self, RL):
        from insilicoseq_amd.engine import ReadEngine

        self.RL, n = RL, K.ROWS[RL]
        self.exp = K.oracle_rows(RL)
        self.eng = eng = ReadEngine(0)
        try:
            eng.load_model(H.row_sweep_model(RL))
            gid = eng.add_genome(H.row_sweep_genome(RL))
            eng.generate(gid, n, first_ordinal=H.ROW_SWEEP_FIRST_ORDINAL, seed=H.ROW_SWEEP_SEED)
            eng.synchronize()
            d = eng.download(0, n)
            for k, (name, mate) in enumerate((("r1_base", 0), ("r1_qual", 0), ("r2_base", 1), ("r2_qual", 1))):
                assert np.array_equal(d[name], self.exp["qual" if k % 2 else "bases"][:, mate]), name
        except Exception:
            eng.close()
            raise


@pytest.fixture(scope="module")
def rows():
    """(one engine per read length, made when its first case runs, alive to the end of the module)"""
    made = {}

    def get(RL):
        if RL not in made:
            made[RL] = Rows(RL)
        return made[RL]

    yield get
    for r in made.values():
        r.eng.close()


@pytest.fixture(scope="module")
def native():
    from insilicoseq_amd import _native

    return _native


def emit_calls(r, calls, paths):
    """Every call's items through the C ABI with the ids as bytes (iss_fastq_emit for one item, iss_fastq_emit_batch for more),
    into the two files, then one flush: the files' bytes."""
    eng = r.eng
    fh = [open(p, "wb") for p in paths]
    try:
        eng.fastq_compress(True)
        for k, items in enumerate(calls):
            if len(items) == 1:
                rid, first_i, row, n = items[0]
                eng._check(eng._lib.iss_fastq_emit(eng._ctx, fh[0].fileno(), fh[1].fileno(), T.as_bytes(rid), first_i, K.CPU, row, n, 1 + k))
            else:
                ids = (C.c_char_p * len(items))(*[T.as_bytes(it[0]) for it in items])
                cols = [np.array([it[j] for it in items], dtype=np.int64) for j in (1, 2, 3)]
                eng._check(eng._lib.iss_fastq_emit_batch(eng._ctx, fh[0].fileno(), fh[1].fileno(), len(items), ids, cols[0].ctypes.data,
                                                         cols[1].ctypes.data, cols[2].ctypes.data, K.CPU))
        eng.fastq_flush()
    finally:
        for f in fh:
            f.close()
        eng.fastq_compress(False)
    return [open(p, "rb").read() for p in paths]


def check_case(name, mode, rows, native, tmp_path, monkeypatch):
    RL, calls, modes = CASES[name]
    assert mode in modes
    r = rows(RL)
    monkeypatch.delenv("ISS_DEFLATE_RUNS_ONLY", raising=False)  # (read by the library at every emit, and by record_distance)
    if mode == "runs only":
        monkeypatch.setenv("ISS_DEFLATE_RUNS_ONLY", "1")
    got = emit_calls(r, calls, [tmp_path / ("%s_%d.fq.gz" % (name, m)) for m in (1, 2)])
    failures = []
    for mate in (1, 2):
        texts = [K.call_text(items, r.exp, mate) for items in calls]
        members = [T.layout(native, t, T.record_distance(items, RL, K.CPU)) for items, t in zip(calls, texts)]
        want = b"".join(m["bytes"] for m in members)
        z = got[mate - 1]
        print("%s, %s, mate %d: %d text bytes in %d members, %d blocks; device %d bytes, twin %d" % (
            name, mode, mate, sum(map(len, texts)), len(members), sum(len(m["blocks"]) for m in members), len(z), len(want)))
        if z != want:
            try:
                inflated = "inflates to the text" if gzip.decompress(z) == b"".join(texts) else "inflates to OTHER text"
            except Exception as e:  # noqa: BLE001  (what zlib says belongs in the message)
                inflated = "does not inflate (%s)" % e
            failures.append("%s, %s, mate %d: the device's stream %s, but is not the twin's: %s" % (name, mode, mate, inflated,
                                                                                               T.describe_difference(z, members)))
    assert not failures, "\n".join(failures)
    return got


def test_one_record(rows, native, tmp_path, monkeypatch):
    check_case("one_record", "matches", rows, native, tmp_path, monkeypatch)


@pytest.mark.parametrize("RL", [5, 8])
def test_short_records(RL, rows, native, tmp_path, monkeypatch):
    a = check_case("short_records_%d" % RL, "matches", rows, native, tmp_path, monkeypatch)
    b = check_case("short_records_%d" % RL, "runs only", rows, native, tmp_path, monkeypatch)
    assert a[0] != b[0] and a[1] != b[1]


@pytest.mark.parametrize("name", ["block_multiple", "block_plus_sliver", "block_minus_sliver"])
def test_block_edges(name, rows, native, tmp_path, monkeypatch):
    check_case(name, "matches", rows, native, tmp_path, monkeypatch)


def test_run_at_block_edge(rows, native, tmp_path, monkeypatch):
    check_case("run_at_block_edge", "matches", rows, native, tmp_path, monkeypatch)


def test_shipped_shape(rows, native, tmp_path, monkeypatch):
    check_case("shipped_shape", "matches", rows, native, tmp_path, monkeypatch)


def test_deep_code(rows, native, tmp_path, monkeypatch):
    check_case("deep_code", "matches", rows, native, tmp_path, monkeypatch)


def test_many_symbols(rows, native, tmp_path, monkeypatch):
    check_case("many_symbols", "matches", rows, native, tmp_path, monkeypatch)


def test_most_pairs_not_first(rows, native, tmp_path, monkeypatch):
    check_case("most_pairs_not_first", "matches", rows, native, tmp_path, monkeypatch)


def test_slot_reuse(rows, native, tmp_path, monkeypatch):
    check_case("slot_reuse", "matches", rows, native, tmp_path, monkeypatch)
