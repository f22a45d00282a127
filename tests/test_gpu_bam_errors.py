"""`report --bam --errors`: the alignments' errors tallied on the device (iss_br_errors_*: k_be_records, k_be_bases) against the
Python twin (insilicoseq_amd.bam_errors.bam_errors_host), word for word, and against the constructions of bam_error_cases.py;
the damaged records, the launch geometry, the feeds, the read tally beside it, the closed loop with the simulator and the round
trip through the command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import bam_error_cases as EC
import bam_synth
from helpers import random_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_contexts = {}
_twins = {}


def _context(max_len, errors=True):
    """One context per (max_len, errors) for the whole module, reset before every use."""
    from insilicoseq_amd.bam_report import BamReadTally

    if (max_len, errors) not in _contexts:
        _contexts[max_len, errors] = BamReadTally(0, max_len, errors=errors)
    _contexts[max_len, errors].reset()
    return _contexts[max_len, errors]


def teardown_module(module):
    for dev in _contexts.values():
        dev.close()
    _contexts.clear()


def _device(chunks, max_len):
    dev = _context(max_len)
    for chunk in chunks:
        dev.feed(chunk)
    return dev.download()


def _twin(key, records, max_len):
    """The twin's result for a record set, computed once per module (plain Python per record)."""
    from insilicoseq_amd.bam_errors import bam_errors_host

    if (key, max_len) not in _twins:
        _twins[key, max_len] = bam_errors_host(EC.chunk_of(records), max_len)
        _twins[key, max_len]["errors"].setflags(write=False)
    return _twins[key, max_len]


def _same(got, exp, max_len):
    from insilicoseq_amd.bam_errors import split

    assert got["error_counts"] == exp["error_counts"]
    assert (got["bad_alignment"], got["bad_alignment_code"]) == (exp["bad_alignment"], exp["bad_alignment_code"])
    g, e = split(got["errors"], max_len), split(exp["errors"], max_len)
    assert [k for k in g if not np.array_equal(g[k], e[k])] == []  # (the fields that differ)


# ---------------------------------------------------------------------------------------------------- lengths and ops
@pytest.mark.parametrize("max_len", [1024, 301])
def test_valid_cases_equal_the_twin_and_the_construction(max_len):
    from insilicoseq_amd.bam_errors import split

    records = [r for r in EC.valid_cases() if len(r["seq"]) <= max_len]
    assert {len(r["seq"]) for r in records} >= {n for n in EC.LENGTHS if n <= max_len}
    got = _device([EC.chunk_of(records)], max_len)
    _same(got, _twin("valid", records, max_len), max_len)
    _same(got, EC.expected(records, max_len), max_len)
    t = split(got["errors"], max_len)
    top = min(max_len, 1024)
    assert got["bad_alignment"] == -1 and not t["dropped"][0] and sum(got["error_counts"][:2]) == len(records)
    assert t["per_read"][:, :, 63].all() and t["sub_mat"][:, :, 4, 4].any() and t["bases"][:, top - 1].any() and t["sub_q"][:, top - 1].any()


def test_each_op_case_alone():
    """One record a feed, so that a difference names its record (the ops, the clamp at 63 rows, deletions at q = 0 and q = len)."""
    from insilicoseq_amd.bam_errors import bam_errors_host

    dev = _context(256)
    for r in EC.op_cases() + EC.length_cases((1, 2, 65)):
        dev.reset()
        dev.feed(EC.chunk_of([r]))
        got = dev.download()
        _same(got, EC.expected([r], 256), 256), r["name"]
        _same(got, bam_errors_host(EC.chunk_of([r]), 256), 256), r["name"]


# ---------------------------------------------------------------------------------------------------- damaged records
def test_damaged_records_between_good_ones():
    from insilicoseq_amd.bam_errors import bam_errors_host

    dev = _context(64)
    for r in EC.damaged_cases():
        what = r["_case"]["expect"]
        for k in range(3):
            three = EC.between_good(r, k)
            dev.reset()
            dev.feed(EC.chunk_of(three))
            got = dev.download()
            _same(got, EC.expected(three, 64), 64), (r["name"], k)
            _same(got, bam_errors_host(EC.chunk_of(three), 64), 64), (r["name"], k)
            assert (got["bad_alignment"], got["bad_alignment_code"]) == ((k, what) if isinstance(what, int) else (-1, 0)), r["name"]
            assert int(got["errors"][0]) == (1 if isinstance(what, int) else 0) and got["bad_record"] == -1
        dev.reset()
        dev.feed(EC.chunk_of([r]))  # alone: nothing but `dropped`
        got = dev.download()
        assert not got["errors"][1:].any() and int(got["errors"][0]) == (1 if isinstance(what, int) else 0), r["name"]


def test_all_damaged_records_in_one_chunk():
    records = []
    for k, r in enumerate(EC.damaged_cases()):
        records += EC.between_good(r, k % 3)
    got = _device([EC.chunk_of(records)], 64)
    _same(got, EC.expected(records, 64), 64)
    _same(got, _twin("damaged", records, 64), 64)
    assert int(got["errors"][0]) > 30 and got["error_counts"][2] >= 4 and got["error_counts"][3] >= 3


def test_first_bad_alignment_wins_across_feeds():
    bad = {r["name"]: r for r in EC.damaged_cases()}
    records = EC.between_good(bad["secondary"], 0) + EC.between_good(bad["md_too_long"], 2) + EC.between_good(bad["op9"], 1)
    exp = EC.expected(records, 64)
    assert (exp["bad_alignment"], exp["bad_alignment_code"]) == (5, 3)
    for per in (None, 4, 1):
        chunks = [EC.chunk_of(records)] if per is None else EC.split(EC.chunk_of(records), per)
        _same(_device(chunks, 64), exp, 64)
    swapped = records[6:] + records[:6]
    exp = EC.expected(swapped, 64)
    assert (exp["bad_alignment"], exp["bad_alignment_code"]) == (1, 1)
    _same(_device(EC.split(EC.chunk_of(swapped), 2), 64), exp, 64)


# ---------------------------------------------------------------------------------------------------- geometry and feeds
_records = {}


def _synthetic():
    if "synthetic" not in _records:
        _records["synthetic"] = EC.synth(bam_synth.records(71, n_pairs=2000))
    return list(_records["synthetic"])


def _edges():
    if "edges" not in _records:
        _records["edges"] = EC.synth(bam_synth.edge_table() + bam_synth.edge_fillers())
    return list(_records["edges"])


def test_synthetic_records():
    from insilicoseq_amd.bam_errors import split

    records = _synthetic()
    got = _device([EC.chunk_of(records)], 301)
    exp = _twin("synthetic", records, 301)
    _same(got, exp, 301)
    t = split(got["errors"], 301)
    assert got["bad_alignment"] == -1 and sum(got["error_counts"][:2]) > 3500 and got["error_counts"][2] > 0
    assert t["sub_q"].sum() > 3000 and t["ins"].sum() > 100 and t["del"].sum() > 100 and t["per_read"][:, 1:, 1:].any()


@pytest.mark.parametrize("max_len", [301, 1024])
def test_edge_table(max_len):
    records = _edges()
    got = _device([EC.chunk_of(records)], max_len)
    _same(got, _twin("edges", records, max_len), max_len)
    assert got["bad_alignment"] == -1 and got["error_counts"][2] >= 1 and sum(got["error_counts"][:2]) >= 100


@pytest.mark.parametrize("n_records", [1, 63, 64, 65, 1000])
def test_record_counts(n_records):
    records = _synthetic()[:n_records]
    _same(_device([EC.chunk_of(records)], 151), _twin("synthetic%d" % n_records, records, 151), 151)


@pytest.mark.parametrize("wgs", ["1", "3", "4096"])
def test_launch_geometry(wgs, monkeypatch):
    records = _synthetic()[:600] + _edges()
    exp = _twin("geometry", records, 301)
    monkeypatch.setenv("ISS_BR_WGS", wgs)
    _same(_device([EC.chunk_of(records)], 301), exp, 301)


def test_feeds_do_not_change_the_words():
    records = _edges() + _synthetic()[:40]
    exp = _twin("feeds", records, 301)
    whole = EC.chunk_of(records)
    third = (len(records) + 2) // 3
    for chunks in ([whole], EC.split(whole, third), EC.split(whole, 1)):
        got = _device(chunks, 301)
        _same(got, exp, 301)
        assert np.array_equal(got["errors"], exp["errors"])


def test_the_read_tally_does_not_depend_on_the_error_stage():
    records = _edges() + _synthetic()[:300]
    for k, r in enumerate(EC.damaged_cases()):
        records.insert(5 * k, r)
    chunks = EC.split(EC.chunk_of(records), 200)
    with_errors = _device(chunks, 301)
    plain = _context(301, errors=False)
    for chunk in chunks:
        plain.feed(chunk)
    without = plain.download()
    assert sorted(without) == ["bad_code", "bad_record", "records", "skipped", "tally"]  # exactly today's dict
    for key in without:
        assert np.array_equal(with_errors[key], without[key]), key
    assert sorted(set(with_errors) - set(without)) == ["bad_alignment", "bad_alignment_code", "error_counts", "errors"]
    res, res_plain = _context(301).result(), plain.result()
    assert sorted(set(res) - set(res_plain)) == ["bad_alignment", "bad_alignment_code", "error_counts", "errors"]


def test_result_is_relaid_to_the_longest_read():
    from insilicoseq_amd.bam_errors import relayout, words

    records = [r for r in EC.valid_cases() if len(r["seq"]) <= 129]
    dev = _context(1024)
    dev.feed(EC.chunk_of(records))
    raw, res = dev.download(), dev.result()
    assert res["read_length"] == 129 and res["errors"].size == words(129)
    assert np.array_equal(res["errors"], relayout(raw["errors"], 1024, 129)) and res["error_counts"] == raw["error_counts"]


def test_reset_and_kernel_time():
    records = EC.between_good({r["name"]: r for r in EC.damaged_cases()}["op9"], 0) + _synthetic()[:100]
    dev = _context(151)
    dev.feed(EC.chunk_of(records))
    dev.feed(EC.chunk_of(records))
    first = dev.download()
    assert (first["bad_alignment"], first["bad_alignment_code"]) == (0, 1) and int(first["errors"][0]) == 2 and dev.kernel_ms() > 0.0
    dev.reset()
    zero = dev.download()
    assert not zero["errors"].any() and zero["error_counts"] == [0, 0, 0, 0] and (zero["bad_alignment"], zero["bad_alignment_code"]) == (-1, 0)
    assert dev._lib.iss_br_error_words(dev._h) == zero["errors"].size  # still enabled
    dev.feed(EC.chunk_of(records))
    _same(dev.download(), _twin("reset", records, 151), 151)


def test_enable_rules_and_invalid_arguments():
    from insilicoseq_amd import _native
    from insilicoseq_amd.bam_errors import words
    from insilicoseq_amd.bam_report import BamReadTally

    lib = _native.lib()
    chunk = EC.chunk_of(_synthetic()[:10])
    counts, bad, code = (C.c_int64 * 4)(), C.c_int64(), C.c_int32()
    buf = np.zeros(words(151), dtype=np.uint64)
    with BamReadTally(0, 151) as dev:
        assert lib.iss_br_error_words(dev._h) == -1 and lib.iss_br_error_words(None) == -1
        assert lib.iss_br_errors_download(dev._h, buf.ctypes.data, C.addressof(counts), C.byref(bad), C.byref(code)) == _native.E_INVALID
        assert b"not enabled" in lib.iss_br_last_error(dev._h)
        dev.feed(chunk)
        before = dev.download()
        assert lib.iss_br_errors_enable(dev._h) == _native.E_INVALID and b"iss_br_errors_enable" in lib.iss_br_last_error(dev._h)
        assert lib.iss_br_error_words(dev._h) == -1  # the state stays as it was
        dev.feed(chunk)
        assert dev.download()["records"] == [2 * n for n in before["records"]]
        dev.reset()
        assert lib.iss_br_errors_enable(dev._h) == 0 and lib.iss_br_errors_enable(dev._h) == 0  # after a reset; twice is once
        assert lib.iss_br_error_words(dev._h) == 2 + 446 * 151 + 384 == buf.size
        dev.feed(chunk)
        args = [buf.ctypes.data, C.addressof(counts), C.byref(bad), C.byref(code)]
        for k in range(4):
            a = list(args)
            a[k] = None
            assert lib.iss_br_errors_download(dev._h, *a) == _native.E_INVALID
        assert lib.iss_br_errors_download(None, *args) == _native.E_INVALID and lib.iss_br_errors_enable(None) == _native.E_INVALID
        assert not buf.any()  # nothing was written
        assert lib.iss_br_errors_download(dev._h, *args) == 0 and sum(counts) == 10
        assert lib.iss_br_errors_enable(dev._h) == _native.E_INVALID  # fed again
        again = np.zeros_like(buf)
        assert lib.iss_br_errors_download(dev._h, again.ctypes.data, *args[1:]) == 0 and np.array_equal(again, buf)


# ---------------------------------------------------------------------------------------------------- the closed loop
def test_closed_loop_with_the_simulator():
    """2 048 pairs of the basic error model (no indels) on an A/C/G/T genome, written here as an aligned BAM -- {L}M, MD from the
    truth bases against the bases, mate 2 stored reversed (0x10) and every other mate 1 as well -- give the engine's own error
    tally back, and the --report tally's qual field as the aligned bases."""
    from insilicoseq_amd import errtally
    from insilicoseq_amd.bam_errors import errors_and_bases, split
    from insilicoseq_amd.bam_report import BamReadTally
    from insilicoseq_amd.model import DenseModel
    from insilicoseq_amd.tally import split_tally
    from insilicoseq_amd.tensors import ReadTensorStream

    L, n = 125, 2048
    dense = DenseModel.basic(L, mean_quality=20)
    genome = random_genome(901, 40000)
    assert set(genome) <= set("ACGT")
    with ReadTensorStream([genome], dense, [(0, n)], 1024, seed=9, encoding="codes", truth=True, error_tally=True, tally=True) as stream:
        batches = [(b.bases.cpu().numpy(), b.qual.cpu().numpy(), b.truth.cpu().numpy()) for b in stream]
        sim = stream.error_tally.cpu().numpy().view(np.uint64)
        report = stream.tally.cpu().numpy().view(np.uint64)
    bases, qual, truth = (np.concatenate([b[k] for b in batches]) for k in range(3))
    assert bases.shape == (n, 2, L) and bases.max() <= 3 and truth.max() <= 3
    records = []
    for p in range(n):
        for m in range(2):
            b, q, t = bases[p, m], qual[p, m], truth[p, m]
            reverse = m == 1 or p % 2 == 1
            if reverse:  # as stored: the reverse complement, the qualities reversed
                b, q, t = 3 - b[::-1], q[::-1], 3 - t[::-1]
            md, run = [], 0
            for k in np.flatnonzero(b != t):
                md.append("%d%s" % (k - run, "ACGT"[t[k]]))
                run = k + 1
            md.append(str(L - run))
            records.append(dict(name="p%d" % p, flag=(0x41, 0x81)[m] | (0x10 if reverse else 0), cigar=[(0, L)], seq="".join("ACGT"[c] for c in b),
                                qual=[int(x) for x in q], tags=[("MD", "Z", "".join(md))]))
    with BamReadTally(0, 301, errors=True) as dev:
        dev.feed(EC.chunk_of(records))
        res = dev.result()
    assert res["read_length"] == L and res["error_counts"] == [n, n, 0, 0] and res["bad_alignment"] == -1
    err, aligned = errors_and_bases(res["errors"], L)
    got, exp = errtally.split(err, L), errtally.split(sim, L)
    assert int(exp["sub_q"].sum()) > 1000 and int(exp["pairs"][0]) == n
    for name in ("sub_q", "sub_mat", "pairs"):
        assert np.array_equal(got[name], exp[name]), name
    assert np.array_equal(got["per_read"][:, 0], exp["per_read"][:, 0])
    assert not got["ins"].any() and not got["del"].any() and not got["dropped"][0]
    assert got["per_read"][:, 1:, 0].tolist() == [[n, n], [n, n]]
    assert np.array_equal(aligned, split_tally(report, L)["qual"]) and np.array_equal(aligned, split(res["errors"], L)["bases"])


# ---------------------------------------------------------------------------------------------------- the command line
def test_round_trip_both_inflate_routes(tmp_path):
    from insilicoseq_amd.bam_errors import errors_and_bases, relayout
    from insilicoseq_amd.bam_report import bam_reads_host, finish

    records = _synthetic()[:600]
    path = str(tmp_path / "a.bam")
    bam_synth.write_records(path, records)
    L = finish(bam_reads_host(EC.chunk_of(records), 1024), 1024)["read_length"]
    exp_err, exp_bases = errors_and_bases(relayout(_twin("cli", records, 1024)["errors"], 1024, L), L)
    other = str(tmp_path / "other_errtally.npy")
    np.save(other, exp_err)
    np.save(str(tmp_path / "other_errbases.npy"), exp_bases)
    env = {k: v for k, v in os.environ.items() if k not in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE")}
    outs = []
    suffixes = ("_errtally.npy", "_errbases.npy", "_errors.json", "_errors_compare.json")
    for tag, extra in (("host", []), ("device", ["--device_inflate"])):
        out = str(tmp_path / tag)
        subprocess.run([sys.executable, "-m", "insilicoseq_amd", "report", "--quiet", "--bam", path, "-o", out, "--errors", "--against_errors", other]
                       + extra, cwd=ROOT, check=True, timeout=600, env=env)
        outs.append([open(out + suffix, "rb").read() for suffix in suffixes])
    assert outs[0] == outs[1]
    assert np.array_equal(np.load(str(tmp_path / "host_errtally.npy")), exp_err)
    assert np.array_equal(np.load(str(tmp_path / "host_errbases.npy")), exp_bases)
    rep = json.load(open(str(tmp_path / "host_errors.json")))
    assert rep["dropped"] == 0 and sum(rep["counts"]["tallied"]) > 500 and rep["mates"][0]["rates"]["substitution"][0] is not None
    cmp = json.load(open(str(tmp_path / "host_errors_compare.json")))
    assert set(cmp["summary"].values()) == {0.0}
