"""errtally.py without a GPU: the layout, the numpy twin of iss_mutations_tally against a plain loop (hand-made rows, the
oracle's rows), the identities between the fields, the report, the CLI's flag, error, merge and file names, and where the work
loops place the call (the recording engine of test_work_loops_host.py)."""
import argparse
import ctypes
import json
import logging
import os

import numpy as np
import pytest

from helpers import dense_model, random_genome
from insilicoseq_amd import _native
from insilicoseq_amd import app as A
from insilicoseq_amd import errtally as E
from insilicoseq_amd import generator as G
from insilicoseq_amd.engine import MUT_DTYPE
from insilicoseq_amd.model import BasicErrorModel

CODE = {c: k for k, c in enumerate(b"ACGT")}
CODE.update({c | 0x20: k for c, k in list(CODE.items())})


def _rows(items):
    """(pair, mate, type, position, ref, alt, quality) tuples -> a structured iss_mutation array."""
    rows = np.zeros(len(items), dtype=MUT_DTYPE)
    for k, (pair, mate, typ, pos, ref, alt, q) in enumerate(items):
        rows[k] = (pair, mate, typ, pos, ord(ref), ord(alt), q)
    return rows


def _loop(rows, first_pair, n_pairs, L):
    """The definition of include/iss_mi355x.h, row by row."""
    flat = np.zeros(2 + 258 * L + 6 * 64, dtype=np.uint64)
    at = {"sub_q": 2, "sub_mat": 2 + 2 * L * 94, "ins": 2 + 2 * L * 119, "del": 2 + 2 * L * 124, "per_read": 2 + 2 * L * 129}
    flat[1] = n_pairs
    per_read = {}
    for r in rows:
        w = int(r["pair"]) - first_pair
        if int(r["pair"]) < 0 or not 0 <= w < n_pairs:
            continue
        m, t = int(r["mate"]) & 1, int(r["type"]) & 3
        pos = min(max(int(r["position"]), 0), L - 1)
        ref, alt = CODE.get(int(r["ref"]), 4), CODE.get(int(r["alt"]), 4)
        if t == 0:
            flat[at["sub_q"] + (m * L + pos) * 94 + min(max(int(r["quality"]), 0), 93)] += 1
            flat[at["sub_mat"] + ((m * L + pos) * 5 + ref) * 5 + alt] += 1
        elif t == 1:
            flat[at["ins"] + (m * L + pos) * 5 + alt] += 1
        elif t == 2:
            flat[at["del"] + (m * L + pos) * 5 + ref] += 1
        else:
            continue
        per_read[(w, m, t)] = per_read.get((w, m, t), 0) + 1
    for m in range(2):
        for t in range(3):
            flat[at["per_read"] + (m * 3 + t) * 64] = n_pairs
    for (w, m, t), k in per_read.items():
        flat[at["per_read"] + (m * 3 + t) * 64] -= 1
        flat[at["per_read"] + (m * 3 + t) * 64 + min(k, 63)] += 1
    return flat


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("L", [1, 32, 33, 125, 151, 301])
def test_layout(L):
    lay = E.layout(L)
    assert list(lay) == ["dropped", "pairs", "sub_q", "sub_mat", "ins", "del", "per_read", "words"]
    assert lay["words"] == E.words(L) == 2 + 258 * L + 6 * 64
    assert lay["dropped"] == (0, (1,)) and lay["pairs"] == (1, (1,))
    assert lay["sub_q"] == (2, (2, L, 94)) and lay["sub_mat"] == (2 + 188 * L, (2, L, 5, 5))
    assert lay["ins"] == (2 + 238 * L, (2, L, 5)) and lay["del"] == (2 + 248 * L, (2, L, 5))
    assert lay["per_read"] == (2 + 258 * L, (2, 3, 64))
    flat = np.arange(lay["words"], dtype=np.uint64)
    t = E.split(flat, L)
    at = 0
    for name in E.FIELDS:  # no padding, the fields in order, views of the words
        assert t[name].reshape(-1)[0] == at and t[name].base is not None
        at += t[name].size
    assert at == lay["words"]
    with pytest.raises(ValueError):
        E.split(flat[:-1], L)
    with pytest.raises(ValueError):
        E.layout(0)
    assert (E.PHREDS, E.READ_BINS) == (94, 64)


# ---------------------------------------------------------------------------------------------------- the twin, hand-made rows
def _hand_made(L):
    items = [
        (0, 0, 0, 0, "A", "C", 93), (0, 0, 0, L - 1, "c", "T", 94), (0, 1, 0, L // 2, "G", "a", 200),  # qualities 93, 94, 200
        (1, 0, 0, 3 % L, "N", "R", 7), (1, 1, 0, 2 % L, "t", "y", 0),                                   # IUPAC, lower case: code 4
        (2, 0, 0, -1, "A", "G", 11), (2, 1, 0, L, "C", "A", 12),                                         # the end bins
        (2, 0, 1, 0, "A", "T", -1), (2, 0, 1, L - 1, "A", "n", -1), (2, 1, 2, 0, "g", ".", -1), (2, 1, 2, L - 1, "K", ".", -1),
        (2, 1, 1, -1, "A", "C", -1), (2, 0, 2, L, "T", ".", -1),
        (-1, 0, 0, 0, "A", "C", 5),                                                                      # an unused slot
        (9, 0, 0, 1 % L, "A", "C", 5), (9, 1, 1, 1 % L, "A", "C", -1), (10, 0, 0, 0, "A", "C", 5),       # outside the window [0, 9)
    ]
    for pair, count in ((3, 63), (4, 64), (5, 70)):  # reads with 63, 64 and 70 substitutions: bins 63, 63, 63
        items += [(pair, 1, 0, k % L, "A", "G", 30 + k % 10) for k in range(count)]
    items += [(6, 0, 1, k % L, "C", "G", -1) for k in range(5)] + [(6, 0, 2, k % L, "C", ".", -1) for k in range(2)]
    return _rows(items)


@pytest.mark.parametrize("L", [1, 32, 33, 125, 151, 301])
def test_twin_equals_a_plain_loop_on_hand_made_rows(L):
    rows = _hand_made(L)
    rng = np.random.RandomState(L)
    rows = rows[rng.permutation(len(rows))]  # (any order)
    for first, n in ((0, 9), (0, 11), (2, 4), (3, 1), (9, 2), (20, 5), (0, 0)):
        got = E.errors_host(rows, first, n, L)
        assert got.dtype == np.uint64 and np.array_equal(got, _loop(rows, first, n, L)), (first, n)
    t = E.split(E.errors_host(rows, 0, 9, L), L)
    assert t["dropped"][0] == 0 and t["pairs"][0] == 9
    assert t["per_read"][1, 0, 63] == 3 and t["per_read"][1, 0, 1:63].sum() == 3  # pairs 0, 1, 2 have one each in mate 1
    assert t["per_read"][0, 1, 5] == 1 and t["per_read"][0, 2, 2] == 1
    if L > 2:
        assert t["sub_q"][0, 0, 93] == 1 and t["sub_q"][0, L - 1, 93] == 1 and t["sub_q"][1, L // 2, 93] == 1
        assert t["sub_q"][0, 0, 11] == 1 and t["sub_q"][1, L - 1, 12] == 1  # positions -1 and L
        assert t["sub_mat"][0, 3, 4, 4] == 1 and t["sub_mat"][1, 2, 3, 4] == 1 and t["sub_mat"][0, L - 1, 1, 3] == 1
        assert t["ins"][0, L - 1, 4] == 1 and t["ins"][1, 0, 1] == 1 and t["del"][1, L - 1, 4] == 1 and t["del"][0, L - 1, 3] == 1


def test_empty_rows():
    L = 33
    for rows in (np.zeros(0, dtype=MUT_DTYPE), _rows([(-1, 0, 0, 0, "A", "C", 1)])):
        t = E.split(E.errors_host(rows, 0, 17, L), L)
        assert t["pairs"][0] == 17 and (t["per_read"][:, :, 0] == 17).all() and t["per_read"].sum() == 6 * 17
        assert sum(int(t[f].sum()) for f in ("dropped", "sub_q", "sub_mat", "ins", "del")) == 0


def _oracle_rows(indel, n=400, seed=3):
    from oracle import oracle as O

    dense = dense_model("novaseq", indel)
    res = O.Oracle(dense).simulate(O.Rng().seed_philox(seed), random_genome(77, 30000), n, first_ordinal=5, store_mutations=True)
    assert res["status"] == 0 and res["n_done"] == n
    return res["mutations"], dense.read_length


@pytest.mark.parametrize("indel", [None, (0.01, 0.03)], ids=["novaseq", "indel_heavy"])
def test_twin_equals_the_loop_on_the_oracles_rows_and_the_identities_hold(indel):
    rows, L = _oracle_rows(indel)
    assert len(rows) > 100 and (indel is None or ((rows["type"] == 1).sum() > 20 and (rows["type"] == 2).sum() > 20))
    for first, n in ((0, 400), (7, 257), (399, 1), (350, 100)):
        assert np.array_equal(E.errors_host(rows, first, n, L), _loop(rows, first, n, L)), (first, n)
    t = E.split(E.errors_host(rows, 0, 400, L), L)
    k = np.arange(64, dtype=np.uint64)
    assert t["per_read"][:, :, 63].sum() == 0  # no read is clamped
    n_sub = int((rows["type"] == 0).sum())
    assert t["sub_q"].sum() == t["sub_mat"].sum() == (t["per_read"][:, 0] * k).sum() == n_sub
    assert t["ins"].sum() == (t["per_read"][:, 1] * k).sum() == (rows["type"] == 1).sum()
    assert t["del"].sum() == (t["per_read"][:, 2] * k).sum() == (rows["type"] == 2).sum()
    assert (t["per_read"].sum(axis=2) == t["pairs"][0]).all()
    assert np.array_equal(t["sub_q"].sum(axis=2), t["sub_mat"].sum(axis=(2, 3)))


# ---------------------------------------------------------------------------------------------------- merge, report
def test_merge_and_report():
    L = 5
    rows = _rows([(0, 0, 0, 0, "A", "C", 20), (0, 0, 0, 1, "A", "G", 20), (1, 0, 0, 0, "C", "T", 30), (1, 1, 0, 4, "g", "N", 10),
                  (2, 1, 1, 2, "A", "T", -1), (3, 1, 2, 3, "C", ".", -1), (3, 1, 2, 4, "C", ".", -1)])
    words = E.errors_host(rows, 0, 4, L)
    both = E.merge([words, words, words])
    assert both.dtype == np.uint64 and np.array_equal(both, 3 * words) and both is not words
    assert np.array_equal(E.merge([words]), words)
    with pytest.raises(ValueError):
        E.merge([words, words[:-1]])
    with pytest.raises(ValueError):
        E.merge([])
    rep = json.loads(json.dumps(E.report_dict(words, L)))  # (serialisable as it is)
    assert rep["pairs"] == 4 and rep["dropped"] == 0 and rep["read_length"] == L and "calibration" not in rep
    m0, m1 = rep["mates"]
    assert m0["rates"] == {"substitution": [0.5, 0.25, 0.0, 0.0, 0.0], "insertion": [0.0] * 5, "deletion": [0.0] * 5}
    assert m1["rates"] == {"substitution": [0.0, 0.0, 0.0, 0.0, 0.25], "insertion": [0.0, 0.0, 0.25, 0.0, 0.0],
                           "deletion": [0.0, 0.0, 0.0, 0.25, 0.25]}
    assert m0["substitution_matrix"]["A"] == {"A": 0, "C": 1, "G": 1, "T": 0, "other": 0} and m0["substitution_matrix"]["C"]["T"] == 1
    assert m1["substitution_matrix"]["G"]["other"] == 1
    assert m0["substitutions_by_phred"] == [0] * 20 + [2] + [0] * 9 + [1] and m1["substitutions_by_phred"] == [0] * 10 + [1]
    assert m0["per_read"] == {"substitution": [2, 1, 1], "insertion": [4], "deletion": [4]}
    assert m1["per_read"] == {"substitution": [3, 1], "insertion": [3, 1], "deletion": [3, 0, 1]}
    blank = E.report_dict(np.zeros(E.words(L), dtype=np.uint64), L)
    assert blank["pairs"] == 0 and blank["mates"][0]["rates"]["substitution"] == [None] * L and blank["mates"][1]["per_read"]["deletion"] == []
    # with the --report tally of the same run: bases per phred from its qual field; a phred without bases is left out
    from insilicoseq_amd import tally as T

    tally = np.zeros(T.tally_words(L), dtype=np.uint64)
    q = T.split_tally(tally, L)["qual"]
    q[0, :, 20] = [4, 4, 0, 0, 0]
    q[0, 0, 30] = 4
    q[0, 2:, 40] = 4
    q[1, :, 10] = 4
    rep = json.loads(json.dumps(E.report_dict(words, L, tally)))
    c0, c1 = rep["calibration"]
    assert [e["phred"] for e in c0] == [20, 30, 40] and [e["phred"] for e in c1] == [10]
    assert [e["bases"] for e in c0] == [8, 4, 12] and [e["substitutions"] for e in c0] == [2, 1, 0]
    assert [e["empirical"] for e in c0] == [2 / 8, 1 / 4, 0.0] and [e["nominal"] for e in c0] == [10.0 ** -2, 10.0 ** -3, 10.0 ** -4]
    assert c1 == [{"phred": 10, "bases": 20, "substitutions": 1, "nominal": 10.0 ** -1.0, "empirical": 1 / 20}]


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_names_are_exported():
    assert "iss_error_tally_words" in _native.EXPORTS and "iss_mutations_tally" in _native.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "iss_mi355x.h")).read()
    assert "int64_t iss_error_tally_words(const iss_ctx *ctx);" in header
    assert "int iss_mutations_tally(iss_ctx *ctx, int32_t source, int64_t first_pair, int64_t n_pairs, uint64_t *d_tally);" in header
    assert "#define ISS_ERRTALLY_PHREDS 94" in header and "#define ISS_ERRTALLY_READ_BINS 64" in header
    assert "#define ISS_ABI_VERSION 8" in header
    if os.path.exists(_native.LIB_PATH):  # (the library is built: it exports them, no GPU needed to look)
        lib = ctypes.CDLL(_native.LIB_PATH)
        assert hasattr(lib, "iss_error_tally_words") and hasattr(lib, "iss_mutations_tally")


def test_an_older_library_is_named():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine.__new__(ReadEngine)
    eng._lib = object()
    for call in (eng.error_tally_words, lambda: eng.error_tally(0, 1, 8)):
        with pytest.raises(_native.NativeLibraryError) as e:
            call()
        assert "iss_mutations_tally" in str(e.value)
    with pytest.raises(ValueError):
        eng.error_tally(0, 1, 8, source="workers")


# ---------------------------------------------------------------------------------------------------- the CLI
def test_parser_flag_and_the_error_without_store_mutations(tmp_path, caplog):
    p = A.build_parser()
    base = ["generate", "--genomes", str(tmp_path / "missing.fasta"), "--output", str(tmp_path / "out")]
    assert p.parse_args(base).error_report is False
    args = p.parse_args(base + ["--error_report"])
    assert args.error_report is True and not args.store_mutations
    with caplog.at_level(logging.ERROR):
        with pytest.raises(SystemExit) as e:
            A.generate_reads(args)  # (before anything is read: the genome file does not exist)
    assert e.value.code == 1
    errors = [r for r in caplog.records if r.levelno >= logging.ERROR]
    assert len(errors) == 1 and "--store_mutations" in errors[0].getMessage()
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(ValueError):  # the worker says the same
        G.worker_iterator([], BasicErrorModel(None, None, False), 0, str(tmp_path / "w"), 1, "metagenomics", False, error_report=True)


def test_worker_set_turns_off_with_the_flag():
    args = argparse.Namespace(gpus=4, rng="mt", devices=1, seed=3, origins=False)
    assert A._worker_set_wanted(args, False, False)
    args.error_report = False
    assert A._worker_set_wanted(args, False, False)
    args.error_report = True
    assert not A._worker_set_wanted(args, False, False)


def test_parent_merges_the_workers_files(tmp_path):
    from insilicoseq_amd import tally as T
    from insilicoseq_amd.distributed import temp_prefix

    L, out = 33, str(tmp_path / "run")
    rows = _hand_made(L)
    parts = [E.errors_host(rows, 0, 5, L), E.errors_host(rows, 5, 6, L), E.errors_host(rows[:0], 0, 3, L)]
    for rank, words in enumerate(parts):
        np.save("%s.errtally.npy" % temp_prefix(out, rank), words)
    assert A._write_errors(out, 3, L, False) == 0
    assert sorted(os.listdir(str(tmp_path))) == ["run_errors.json", "run_errtally.npy"]  # the workers' files are gone
    total = np.load(out + "_errtally.npy")
    assert total.dtype == np.uint64 and np.array_equal(total, parts[0] + parts[1] + parts[2])
    rep = json.load(open(out + "_errors.json"))
    assert rep == json.loads(json.dumps(E.report_dict(total, L))) and rep["pairs"] == 14 and "calibration" not in rep
    # with --report: <output>_tally.npy is there by then; and a dropped call is handed back
    tally = np.zeros(T.tally_words(L), dtype=np.uint64)
    T.split_tally(tally, L)["qual"][:, :, 30] = 14
    np.save(out + "_tally.npy", tally)
    parts[1][0] = 2
    for rank, words in enumerate(parts):
        np.save("%s.errtally.npy" % temp_prefix(out, rank), words)
    assert A._write_errors(out, 3, L, True) == 2
    rep = json.load(open(out + "_errors.json"))
    assert rep["dropped"] == 2 and [e["phred"] for e in rep["calibration"][0]] == [30] and rep["calibration"][1][0]["bases"] == 14 * L


# ---------------------------------------------------------------------------------------------------- the work loops
from test_work_loops_host import RecordingEngine, _work, rec  # noqa: E402,F401  (the recording stand-in for ReadEngine)


class _Words(object):
    def data_ptr(self):
        return 4096

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros(E.words(125), dtype=np.int64)


@pytest.fixture
def loops(rec):  # noqa: F811
    def error_tally(self, first_pair, n_pairs, ptr, source="philox"):
        self._log("errtally", first_pair, n_pairs, ptr, source)

    rec.setattr(RecordingEngine, "error_tally", error_tally, raising=False)
    rec.setattr(RecordingEngine, "synchronize", lambda self: None, raising=False)
    rec.setattr(RecordingEngine, "error_tally_words", lambda self: E.words(125), raising=False)
    rec.setattr(G, "_device_zeros", lambda engine, n_words, dtype: _Words())
    return rec


def _run(tmp_path, spec, rng, error_report=True):
    prefix = str(tmp_path / "w")
    kw = {"error_report": True} if error_report else {}
    G.worker_iterator(_work(spec), BasicErrorModel(None, None, True), 3, prefix, 5, "metagenomics", False, device=0, rng=rng, **kw)
    trace = [c for c in RecordingEngine.trace if c[0] != "mutations_reserve"]
    return trace, prefix


def test_batched_loop_tallies_once_per_batch_behind_the_settled_rows(loops, tmp_path):
    trace, prefix = _run(tmp_path, [("s1", 10), ("s2", 20), ("s3", 30)], "philox")
    kinds = [c[0] for c in trace if c[0] in ("batch", "vcf", "errtally", "emit_batch")]
    assert kinds == ["batch", "vcf", "errtally", "emit_batch"] * 2  # 32 pairs a batch: 10 + 20 + 2, then 28
    assert [c[1:] for c in trace if c[0] == "errtally"] == [(0, 32, 4096, "philox"), (0, 28, 4096, "philox")]
    assert os.path.exists(prefix + ".errtally.npy") and np.load(prefix + ".errtally.npy").shape == (E.words(125),)


def test_batched_loop_counts_a_repeated_call_once(loops, tmp_path):
    loops.setattr(RecordingEngine, "overflow", {"vcf"})
    trace, _ = _run(tmp_path, [("s1", 10), ("s2", 20)], "philox")
    kinds = [c[0] for c in trace if c[0] in ("batch", "vcf", "errtally", "emit_batch")]
    assert kinds == ["batch", "vcf", "batch", "vcf", "errtally", "emit_batch"]


def test_arena_fallback_tallies_every_item_as_a_call_of_its_own(loops, tmp_path):
    loops.setattr(RecordingEngine, "arena_ok", False)
    trace, _ = _run(tmp_path, [("s1", 10), ("s2", 20)], "philox")
    kinds = [c[0] for c in trace if c[0] in ("batch", "gen", "vcf", "errtally", "emit_batch")]
    assert kinds == ["batch", "gen", "vcf", "errtally", "gen", "vcf", "errtally", "emit_batch"]
    assert [c[1:3] for c in trace if c[0] == "errtally"] == [(0, 10), (10, 20)]  # the item's rows, where its call put them


def test_host_route_keeps_working(loops, tmp_path):
    loops.setenv("ISS_HOST_VCF", "1")
    trace, _ = _run(tmp_path, [("s1", 10), ("s2", 20)], "philox")
    kinds = [c[0] for c in trace if c[0] in ("batch", "rows", "vcf", "errtally", "emit_batch")]
    assert kinds == ["batch", "rows", "errtally", "emit_batch"]


@pytest.mark.parametrize("rng", ["mt", "philox"])
def test_itemwise_loop_tallies_every_call_with_its_source(loops, tmp_path, rng):
    if rng == "philox":
        loops.setenv("ISS_ITEMWISE", "1")
    trace, _ = _run(tmp_path, [("s1", 40), ("s2", 5)], rng)
    gen = "mt" if rng == "mt" else "gen"
    kinds = [c[0] for c in trace if c[0] in (gen, "vcf", "errtally", "emit")]
    assert kinds == [gen, "vcf", "errtally", "emit"] * 3  # 32 + 8 pairs of s1, 5 of s2
    assert [c[1:] for c in trace if c[0] == "errtally"] == [(0, 32, 4096, rng), (0, 8, 4096, rng), (0, 5, 4096, rng)]


@pytest.mark.parametrize("rng", ["mt", "philox"])
def test_no_call_and_no_file_without_the_flag(loops, tmp_path, rng):
    with_flag, _ = _run(tmp_path, [("s1", 40), ("s2", 5)], rng)
    os.remove(str(tmp_path / "w.errtally.npy"))
    loops.setattr(RecordingEngine, "trace", [])
    without, _ = _run(tmp_path, [("s1", 40), ("s2", 5)], rng, error_report=False)
    assert not [c for c in without if c[0] == "errtally"] and [c for c in with_flag if c[0] != "errtally"] == without
    assert not os.path.exists(str(tmp_path / "w.errtally.npy"))
