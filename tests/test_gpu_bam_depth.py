"""`report --bam --depth`: the alignments' reference intervals marked on the device (iss_br_depth_*: k_bd_records) against the numpy
twin (insilicoseq_amd.bam_depth.mark_host) over the same chunks, word for word in a guarded array; the filters, the bad records,
the launch geometry, the feeds, the stages beside it, the entry rules, depth_result against depth.finish_host, the command line
and the closed loop with `generate --origins --depth`."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import bam_depth_cases as DC
import bam_report_cases as BC
import bam_synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, PATTERN = 64, 0x5A5A5A5A

_contexts = {}


def _context(errors=False):
    """One plain context per module and ``errors``, reset before every use; the stage is enabled on it through the C entries."""
    from insilicoseq_amd.bam_report import BamReadTally

    if errors not in _contexts:
        _contexts[errors] = BamReadTally(0, 1024, errors=errors)
    _contexts[errors].reset()
    return _contexts[errors]


def teardown_module(module):
    for dev in _contexts.values():
        dev.close()
    _contexts.clear()


def _table(skip=True):
    from insilicoseq_amd.depth import depth_table

    table, n_words = depth_table([ln for _name, ln in DC.REFS])
    if skip:
        table[DC.SKIPPED_ROW, 0] = -1
        n_words -= DC.REFS[DC.SKIPPED_ROW][1] + 1
    return table, n_words


class Accumulator(object):
    """The caller's side of the stage: the table and a zeroed difference array on the device between guard words; ``shift``: the
    array's address modulo 16."""

    def __init__(self, table, n_words, shift=0):
        dev = torch.device("cuda", 0)
        self.table, self.n_words = table, n_words
        self.d_table = torch.from_numpy(table).to(dev)
        self.buf = torch.full((GUARD + n_words + GUARD + 4,), PATTERN, dtype=torch.int32, device=dev)
        self.start = next(k for k in range(GUARD, GUARD + 4) if (self.buf.data_ptr() + 4 * k) % 16 == shift)
        self.buf[self.start:self.start + n_words] = 0
        torch.cuda.synchronize()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.start

    def enable(self, dev, flags=0, min_mapq=0):
        return dev._lib.iss_br_depth_enable(dev._h, C.c_void_p(self.d_table.data_ptr()), self.table.shape[0], C.c_void_p(self.ptr()), flags,
                                            min_mapq)

    def diff(self):
        """The array, the guards checked."""
        host = self.buf.cpu().numpy()
        assert (host[:self.start] == PATTERN).all() and (host[self.start + self.n_words:] == PATTERN).all()
        return host[self.start:self.start + self.n_words].copy()


def _download(dev):
    counts, bad, code = (C.c_int64 * 6)(), C.c_int64(), C.c_int32()
    dev._check(dev._lib.iss_br_depth_download(dev._h, C.addressof(counts), C.byref(bad), C.byref(code)))
    return {"depth_counts": list(counts), "bad_depth_record": bad.value, "bad_depth_code": code.value}


def _device(chunks, table, n_words, flags=0, min_mapq=0, errors=False, shift=0):
    """(the array, the stage's download, the context's download) of the chunks fed into a fresh accumulator."""
    dev = _context(errors)
    acc = Accumulator(table, n_words, shift)
    assert acc.enable(dev, flags, min_mapq) == 0
    for chunk in chunks:
        dev.feed(chunk)
    res = _download(dev)
    return acc.diff(), res, dev.download()


def _twin(chunks, table, n_words, flags=0, min_mapq=0):
    from insilicoseq_amd.bam_depth import mark_host

    diff = np.zeros(n_words, dtype=np.int32)
    return diff, mark_host(diff, chunks, table, flags, min_mapq)


def _same(chunks, table, n_words, flags=0, min_mapq=0, **kw):
    got, res, _tally = _device(chunks, table, n_words, flags, min_mapq, **kw)
    exp, exp_res = _twin(chunks, table, n_words, flags, min_mapq)
    assert res == exp_res
    assert np.flatnonzero(got != exp).tolist() == []  # (the words that differ)
    return got, res


# ---------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("min_mapq", [0, 20])
def test_case_table_equals_the_twin(flags, min_mapq):
    table, n_words = _table()
    records = DC.valid_cases()
    got, res = _same([DC.chunk_of(records)], table, n_words, flags, min_mapq)
    depth, counts, bad = DC.expected(records, table, bool(flags), min_mapq)
    assert np.array_equal(np.cumsum(got.astype(np.int64)), depth[:n_words]) and res["depth_counts"] == counts
    assert res["bad_depth_record"] == -1 and counts[0] >= 22 and counts[1] == 5 and counts[2] == 3 and counts[4] == 2
    assert got[int(table[0, 0]) + 50] < 0 and np.cumsum(got)[int(table[2, 0]) + 215] >= 2  # a sink that took -1s; depth 2


def test_each_case_alone():
    """One record a feed into an array of its own, so that a difference names its record."""
    table, n_words = _table()
    for r in DC.valid_cases():
        for flags in (0, 1):
            got, res = _same([DC.chunk_of([r])], table, n_words, flags, 20)
            depth, counts, _bad = DC.expected([r], table, bool(flags), 20)
            assert np.array_equal(np.cumsum(got.astype(np.int64)), depth[:n_words]) and res["depth_counts"] == counts, r["name"]


def test_bad_records_between_good_ones():
    table, n_words = _table()
    for bad, code in DC.bad_cases():
        for k in range(3):
            three = DC.between_good(bad, k)
            got, res = _same([DC.chunk_of(three)], table, n_words)
            assert (res["bad_depth_record"], res["bad_depth_code"]) == (k, code), bad["name"]
            assert res["depth_counts"][:5] == [2, 0, 0, 0, 0]
            assert np.array_equal(got, _twin([DC.chunk_of([r for r in three if r is not bad])], table, n_words)[0]), bad["name"]
        got, res = _same([DC.chunk_of([bad])], table, n_words, 1)
        assert not got.any() and res["depth_counts"] == [0] * 6, bad["name"]


def test_smallest_bad_record_wins_across_feeds_and_workgroups(monkeypatch):
    table, n_words = _table()
    records = []
    for k, (bad, _code) in enumerate(DC.bad_cases()):
        records += DC.between_good(bad, k % 3)
    records = records[6:] + records[:6]  # the third group comes first
    _depth, _counts, first = DC.expected(records, table)
    assert first == (2, 1)  # bad_op_and_ref at place 2 of its three
    chunk = DC.chunk_of(records)
    for wgs in (None, "1", "3"):
        if wgs:
            monkeypatch.setenv("ISS_BR_WGS", wgs)
        for per in (None, 1, 7):
            _got, res = _same([chunk] if per is None else DC.split(chunk, per), table, n_words)
            assert (res["bad_depth_record"], res["bad_depth_code"]) == first


# ---------------------------------------------------------------------------------------------------- independence
def _mixed_records():
    records = DC.valid_cases()
    for k, (bad, _code) in enumerate(DC.bad_cases()):
        records.insert(3 * k + 1, bad)
    return records * 3  # more than one workgroup of four records, and every base at depth 3 or more


def test_feeds_geometry_and_alignment_do_not_change_the_words(monkeypatch):
    table, n_words = _table()
    chunk = DC.chunk_of(_mixed_records())
    exp, exp_res = _twin([chunk], table, n_words, 1, 20)
    assert exp_res["bad_depth_record"] == 1 and exp_res["depth_counts"][0] > 60
    for per in (1, 7, None):
        got, res = _same([chunk] if per is None else DC.split(chunk, per), table, n_words, 1, 20)
        assert np.array_equal(got, exp) and res == exp_res
    for wgs in ("1", "3"):
        monkeypatch.setenv("ISS_BR_WGS", wgs)
        got, res = _same(DC.split(chunk, 50), table, n_words, 1, 20)
        assert np.array_equal(got, exp) and res == exp_res
    monkeypatch.delenv("ISS_BR_WGS")
    for shift in (4, 8, 12):  # an array that is only 4-byte aligned
        got, res = _same([chunk], table, n_words, 1, 20, shift=shift)
        assert np.array_equal(got, exp) and res == exp_res


def test_the_other_stages_do_not_depend_on_this_one():
    table, n_words = _table()
    records = _mixed_records()[:60]
    chunks = DC.split(DC.chunk_of(records), 25)
    exp, exp_res = _twin(chunks, table, n_words)
    for errors in (False, True):
        got, res, with_stage = _device(chunks, table, n_words, errors=errors)
        assert np.array_equal(got, exp) and res == exp_res
        from insilicoseq_amd.bam_report import BamReadTally

        with BamReadTally(0, 1024, errors=errors) as plain:
            for chunk in chunks:
                plain.feed(chunk)
            without = plain.download()
        assert sorted(with_stage) == sorted(without) and ("errors" in without) == errors
        for key in without:
            assert np.array_equal(with_stage[key], without[key]), key
        assert sum(without["records"]) > 40
        if errors:
            assert without["error_counts"][3] > 10  # (this module's records carry no MD tag: the error stage counts them)


def test_error_stage_beside_it_on_records_with_md():
    """bam_synth's records carry MD tags: the error words with the depth stage on equal those of a context without it."""
    from insilicoseq_amd.bam_report import BamReadTally
    from insilicoseq_amd.depth import depth_table

    records = bam_synth.records(5, n_pairs=60, var_lengths=(4, 301))
    chunks = BC.split(BC.chunk_of(records), 50)
    table, n_words = depth_table([1000000])
    _got, res, with_stage = _device(chunks, table, n_words, errors=True)
    assert res["depth_counts"][0] > 100
    with BamReadTally(0, 1024, errors=True) as plain:
        for chunk in chunks:
            plain.feed(chunk)
        without = plain.download()
    assert sum(without["error_counts"][:2]) > 100 and without["errors"].sum() > 1000
    for key in without:
        assert np.array_equal(with_stage[key], without[key]), key


# ---------------------------------------------------------------------------------------------------- the entries
def test_entry_rules():
    from insilicoseq_amd import _native
    from insilicoseq_amd.bam_report import BamReadTally

    lib = _native.lib()
    table, n_words = _table()
    chunk = DC.chunk_of(DC.valid_cases())
    exp, exp_res = _twin([chunk], table, n_words)
    counts, bad, code = (C.c_int64 * 6)(), C.c_int64(), C.c_int32()
    down = [C.addressof(counts), C.byref(bad), C.byref(code)]
    with BamReadTally(0, 1024) as dev:
        acc = Accumulator(table, n_words)
        assert lib.iss_br_depth_download(dev._h, *down) == _native.E_INVALID and b"not enabled" in lib.iss_br_last_error(dev._h)
        t, d = C.c_void_p(acc.d_table.data_ptr()), C.c_void_p(acc.ptr())
        for args in ((None, 4, d, 0, 0), (t, 4, None, 0, 0), (t, 0, d, 0, 0), (t, -1, d, 0, 0), (t, 4, d, 2, 0), (t, 4, d, 0x80000001, 0),
                     (t, 4, d, 0, -1), (t, 4, d, 0, 256), (t, 4, C.c_void_p(acc.ptr() + 2), 0, 0)):
            assert lib.iss_br_depth_enable(dev._h, *args) == _native.E_INVALID, args
            assert b"iss_br_depth_enable" in lib.iss_br_last_error(dev._h)
        assert lib.iss_br_depth_enable(None, t, 4, d, 0, 0) == _native.E_INVALID
        assert lib.iss_br_depth_download(dev._h, *down) == _native.E_INVALID  # still off
        dev.feed(chunk)
        before = dev.download()
        assert acc.enable(dev) == _native.E_INVALID and b"fed" in lib.iss_br_last_error(dev._h)  # after a feed
        assert lib.iss_br_depth_download(dev._h, *down) == _native.E_INVALID and not acc.diff().any()
        dev.reset()
        assert acc.enable(dev, 1, 30) == 0 and acc.enable(dev) == 0  # after a reset; again before a feed: the new arguments hold
        dev.feed(chunk)
        for k in range(3):
            a = list(down)
            a[k] = None
            assert lib.iss_br_depth_download(dev._h, *a) == _native.E_INVALID
        assert lib.iss_br_depth_download(None, *down) == _native.E_INVALID
        assert _download(dev) == exp_res and np.array_equal(acc.diff(), exp)
        assert acc.enable(dev) == _native.E_INVALID  # fed again
        for key in before:
            assert np.array_equal(dev.download()[key], before[key]), key
        # a reset zeroes the counts and the first-bad word, leaves the array alone and the stage on
        bad_chunk = DC.chunk_of([DC.bad_cases()[0][0]])
        dev.feed(bad_chunk)
        assert _download(dev)["bad_depth_record"] == len(chunk.offsets)
        dev.reset()
        assert _download(dev) == {"depth_counts": [0] * 6, "bad_depth_record": -1, "bad_depth_code": 0}
        assert np.array_equal(acc.diff(), exp)
        dev.feed(chunk)
        assert _download(dev) == exp_res and np.array_equal(acc.diff(), 2 * exp) and dev.kernel_ms() > 0.0


def test_python_class_rules():
    from insilicoseq_amd._native import EngineError
    from insilicoseq_amd.bam_report import BamReadTally

    chunk = DC.chunk_of(DC.valid_cases())
    with BamReadTally(0, 1024, depth=True, depth_flags=1, min_mapq=20) as dev:
        with pytest.raises(EngineError):
            dev.depth_result()  # no table yet
        with pytest.raises(EngineError):
            dev.set_depth_table([])
        dev.set_depth_table(DC.REFS)
        dev.set_depth_table([(name, ln) for name, ln in DC.REFS])  # the same again
        with pytest.raises(EngineError):
            dev.set_depth_table(DC.REFS[:3])
        dev.feed(chunk)
        table, n_words = _table(skip=False)
        exp, exp_res = _twin([chunk], table, n_words, 1, 20)
        res = dev.depth_result()
        assert {k: res[k] for k in exp_res} == exp_res and np.array_equal(dev.depth_diff(), exp)
        assert res["ids"] == [name for name, _ln in DC.REFS] and np.array_equal(res["table"], table) and res["bins"] is None
        assert sorted(dev.download()) == ["bad_code", "bad_record", "records", "skipped", "tally"]
        dev.reset()  # the class owns the array: its reset zeroes it
        assert not dev.depth_diff().any()
        dev.feed(chunk)
        assert np.array_equal(dev.depth_diff(), exp)
    with BamReadTally(0, 1024) as dev:
        with pytest.raises(EngineError):
            dev.set_depth_table(DC.REFS)


# ---------------------------------------------------------------------------------------------------- random records
def test_random_records_and_depth_result():
    from insilicoseq_amd.bam_report import BamReadTally
    from insilicoseq_amd.depth import finish_host

    records = bam_synth.records(5, n_pairs=300, var_lengths=(1, 301))  # (a seed whose short reads bam_synth can build)
    chunks = BC.split(BC.chunk_of(records), 256)
    refs = [("chr1", 1000000)]
    with BamReadTally(0, 1024, depth=True) as dev:
        dev.set_depth_table(refs)
        for chunk in chunks:
            dev.feed(chunk)
        results = {bin: dev.depth_result(bin) for bin in (0, 1, 7, 1024)}
        got = dev.depth_diff()
    table = results[0]["table"]
    exp, exp_res = _twin(chunks, table, 1000001)
    assert np.array_equal(got, exp) and exp_res["bad_depth_record"] == -1
    assert 500 < exp_res["depth_counts"][0] < 600 and exp_res["depth_counts"][5] > 50000  # (some of the 600 are secondary ...)
    for bin, res in results.items():
        _depth, stats, bins = finish_host(exp, table, bin)
        assert {k: res[k] for k in exp_res} == exp_res
        assert np.array_equal(res["stats"], stats), bin
        assert (res["bins"] is None and bins is None) if bin == 0 else np.array_equal(res["bins"], bins), bin
        assert int(res["stats"][0, 0]) == exp_res["depth_counts"][5]


# ---------------------------------------------------------------------------------------------------- the command line
def _report(argv):
    from insilicoseq_amd.app import main

    return main(["report", "--quiet"] + argv)


def test_command_line_both_inflate_routes(tmp_path, monkeypatch):
    from insilicoseq_amd import bam_depth
    from insilicoseq_amd import depth as D

    for name in ("ISS_DEVICE_INFLATE", "ISS_HOST_INFLATE"):
        monkeypatch.delenv(name, raising=False)
    records = _mixed_records()
    path = str(tmp_path / "cases.bam")
    DC.write_bam(path, DC.REFS, records)
    table, n_words = _table(skip=False)  # the header's references: row 3 is a row like any other
    exp, exp_res = _twin([DC.chunk_of(records)], table, n_words)
    _depth, stats, bins = D.finish_host(exp, table, 7)
    ids = [name for name, _ln in DC.REFS]
    twin = str(tmp_path / "twin")
    D.write_depth_table(twin + "_depth.txt", D.depth_rows(stats, table, ids))
    D.write_bedgraph(twin + "_depth.bedgraph", bins, table, ids, 7)
    bam_depth.write_coverage_file(twin + "_coverage.txt", bam_depth.coverage_rows(stats, table, ids))
    suffixes = ("_depth.txt", "_depth.bedgraph", "_coverage.txt")
    for tag, extra in (("host", []), ("device", ["--device_inflate", "--against_depth", twin + "_depth.txt"])):
        out = str(tmp_path / tag)
        assert _report(["--bam", path, "--depth_bin", "7", "-o", out] + extra) == 0
        for suffix in suffixes:
            assert open(out + suffix, "rb").read() == open(twin + suffix, "rb").read(), (tag, suffix)
        rep = json.load(open(out + "_report.json"))
        assert rep["depth"] == dict(bam_depth.counts_dict(exp_res["depth_counts"]),
                                    bad_record={"record": exp_res["bad_depth_record"], "code": exp_res["bad_depth_code"]})
        assert rep["depth"]["marked"] > 60 and rep["depth"]["bad_record"]["record"] == 1 and "records_skipped" in rep
    assert not os.path.exists(str(tmp_path / "host_depth_compare.json"))
    cmp = json.load(open(str(tmp_path / "device_depth_compare.json")))
    assert set(cmp["summary"].values()) == {0.0} and cmp["only_here"] == cmp["only_there"] == [] and sorted(cmp["records"]) == sorted(ids)
    # --depth_deletions and --min_mapq reach the stage; without a bin there is no bedgraph
    out = str(tmp_path / "flags")
    assert _report(["--bam", path, "--depth_deletions", "--min_mapq", "20", "-o", out]) == 0
    exp, exp_res = _twin([DC.chunk_of(records)], table, n_words, 1, 20)
    _depth, stats, _bins = D.finish_host(exp, table)
    D.write_depth_table(twin + "_flags_depth.txt", D.depth_rows(stats, table, ids))
    assert open(out + "_depth.txt", "rb").read() == open(twin + "_flags_depth.txt", "rb").read() and not os.path.exists(out + "_depth.bedgraph")
    assert json.load(open(out + "_report.json"))["depth"]["below_min_mapq"] == exp_res["depth_counts"][3] > 0


def test_command_line_errors(tmp_path, capsys):
    path = str(tmp_path / "norefs.bam")
    DC.write_bam(path, [], [DC.rec("r", -1, -1, [], flag=0x4D)])
    assert _report(["--bam", path, "--depth", "-o", str(tmp_path / "a")]) == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("ERROR: ") and "references" in err
    empty = str(tmp_path / "empty.bam")
    DC.write_bam(empty, DC.REFS, [])  # no records: the table is the header's all the same
    assert _report(["--bam", empty, "--depth", "-o", str(tmp_path / "e")]) == 0
    lines = open(str(tmp_path / "e_depth.txt")).read().splitlines()
    assert lines[1:] == ["%s\t%d\t0.0\t0.0\t0.0\t0" % (name, ln) for name, ln in DC.REFS]
    assert _report(["--bam", empty, "--against_depth", str(tmp_path / "missing.txt"), "-o", str(tmp_path / "m")]) == 1
    assert capsys.readouterr().err.count("\n") == 1
    assert _report(["--bam", empty, "--depth_bin", "0", "-o", str(tmp_path / "z")]) == 1
    assert _report(["--bam", empty, "--min_mapq", "256", "-o", str(tmp_path / "z")]) == 1
    assert capsys.readouterr().err.count("\n") == 2


# ---------------------------------------------------------------------------------------------------- the closed loop
def test_closed_loop_with_generate(tmp_path):
    """`generate --mode perfect --origins --depth` on two records of 2 000 bases; the BEDPE made an aligned BAM here, one {RL}M per
    mate at its interval; `report --bam --depth` of that BAM writes generate's _depth.txt byte for byte.  Condition: no interval
    of the run is clamped (asserted on the BEDPE: every interval has the read's length)."""
    from helpers import random_genome
    from insilicoseq_amd import origins

    ids, seqs = ["recA", "recB"], [random_genome(31, 2000), random_genome(32, 2000)]
    fasta = str(tmp_path / "g.fasta")
    with open(fasta, "w") as fh:
        for rid, seq in zip(ids, seqs):
            fh.write(">%s\n%s\n" % (rid, seq.decode() if isinstance(seq, bytes) else seq))
    gen = str(tmp_path / "gen")
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--mode", "perfect", "-n", "1000",
                    "--seed", "7", "--origins", "--depth", "--output", gen], cwd=ROOT, check=True, timeout=600)
    o = origins.parse(gen + origins.SUFFIX)
    assert len(o["id"]) == 500
    lengths = np.concatenate([o["e1"] - o["s1"], o["e2"] - o["s2"]])
    RL = int(lengths[0])
    assert 0 < RL <= 1024 and (lengths == RL).all()  # nothing clamped
    records = []
    for k in range(500):
        ref = ids.index(o["id"][k])
        records.append(DC.rec("p%d" % k, ref, int(o["s1"][k]), [(DC.M, RL)], flag=0x41))
        records.append(DC.rec("p%d" % k, ref, int(o["s2"][k]), [(DC.M, RL)], flag=0x91))
    path = str(tmp_path / "aligned.bam")
    DC.write_bam(path, [(rid, 2000) for rid in ids], records)
    out = str(tmp_path / "rep")
    assert _report(["--bam", path, "--depth", "-o", out]) == 0
    assert open(out + "_depth.txt", "rb").read() == open(gen + "_depth.txt", "rb").read()
    rep = json.load(open(out + "_report.json"))
    assert rep["depth"]["marked"] == 1000 and rep["depth"]["covered_bases"] == 1000 * RL and rep["depth"]["bad_record"]["record"] == -1
