"""BGZF members inflated on the MI355X (k_bgzf_inflate, iss_inflate_*) against the case table of tests/inflate_cases.py -- bytes and
statuses, no tolerance -- the feed/collect pipeline, the invalid arguments, and the round trips: the project's own BGZF outputs, `model`
and `report` through the device route against the host route.  The table itself is held against zlib, and the decoder's text runs
under the address sanitizer, without a GPU (tests/test_inflate_host.py, tests/test_inflate_core_host.py)."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import bam_synth
import fastq_cases as FC
import inflate_cases as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def Z():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import inflate

    return inflate


@pytest.fixture(scope="module")
def inf(Z):
    with Z.BgzfInflater(0) as d:
        yield d


@pytest.fixture()
def fresh(inf):
    inf.reset()
    return inf


def run_group(Z, inf, cases):
    blob = b"".join(c["member"] for c in cases)
    members, used = Z.scan(blob)
    assert used == len(blob) and members.offset.size == len(cases)
    inf.feed(blob, members)
    return members


def check_group(cases, members, data, status):
    assert status.tolist() == [c["status"] for c in cases], [(c["name"], IC.STATUS_NAMES[s]) for c, s in zip(cases, status) if c["status"] != s]
    assert data.size == int(members.isize.sum())
    at = 0
    for c, n in zip(cases, members.isize):
        if c["data"] is not None:
            assert data[at:at + int(n)].tobytes() == c["data"], c["name"]
        at += int(n)


@pytest.mark.parametrize("case", IC.all_cases(), ids=lambda c: c["name"])
def test_each_case_alone(Z, fresh, case):
    members = run_group(Z, fresh, [case])
    data, status = fresh.collect()
    check_group([case], members, data, status)
    assert fresh.first_bad() == ((0, case["status"]) if case["status"] else (-1, 0))


def test_all_cases_in_one_feed(Z, fresh):
    cases = IC.all_cases()
    members = run_group(Z, fresh, cases)
    data, status = fresh.collect()
    check_group(cases, members, data, status)
    first = next(k for k, c in enumerate(cases) if c["status"])
    assert fresh.first_bad() == (first, cases[first]["status"])
    # the first-bad word runs over all feeds: a second feed does not move it, a bad member in front of it would
    run_group(Z, fresh, cases)
    fresh.collect()
    assert fresh.first_bad() == (first, cases[first]["status"])


def small_members(n, seed):
    rnd = np.random.default_rng(seed)
    out = []
    for k in range(n):
        data = (b"member %d " % k) * int(rnd.integers(1, 40)) + rnd.integers(0, 256, int(rnd.integers(0, 300)), dtype=np.uint8).tobytes()
        out.append({"name": "m%d" % k, "member": IC.member(IC.deflate(data, level=int(rnd.integers(1, 10))), data), "data": data,
                    "status": IC.OK})
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("wgs", [None, 1, 3])
def test_member_counts(Z, fresh, n, wgs, monkeypatch):
    """The member-to-wave mapping wraps: more members than waves in flight, in launches of one workgroup, three and the default."""
    if wgs:
        monkeypatch.setenv("ISS_INFLATE_WGS", str(wgs))
    cases = small_members(n, n)
    if n >= 65:  # a bad member among them (with one workgroup: in a wave's eleventh round)
        cases[40] = dict(IC.bad_cases()[5], name="bad")
    members = run_group(Z, fresh, cases)
    data, status = fresh.collect()
    check_group(cases, members, data, status)
    assert fresh.first_bad() == ((40, cases[40]["status"]) if n >= 65 else (-1, 0))


@pytest.mark.parametrize("depth", [2, 3, 5])
def test_feeds_in_flight_before_the_first_collect(Z, fresh, depth):
    groups = [small_members(50 + 7 * k, 100 + k) + IC.good_cases()[3 + k:5 + k] for k in range(depth)]
    members = [run_group(Z, fresh, g) for g in groups]
    assert fresh.in_flight == depth
    for g, m in zip(groups, members):
        data, status = fresh.collect(copy=False)
        check_group(g, m, data, status)
    assert fresh.first_bad() == (-1, 0) and fresh.kernel_ms() > 0.0
    with pytest.raises(Exception) as e:
        fresh.collect()
    assert "no group in flight" in str(e.value)


def test_reset_and_reuse(Z, fresh):
    cases = IC.all_cases()
    run_group(Z, fresh, cases)
    run_group(Z, fresh, cases[:10])
    fresh.reset()  # drops both groups and the first-bad word
    assert fresh.in_flight == 0 and fresh.first_bad() == (-1, 0) and fresh.kernel_ms() == 0.0
    with pytest.raises(Exception):
        fresh.collect()
    good = IC.good_cases()
    members = run_group(Z, fresh, good)
    data, status = fresh.collect()
    check_group(good, members, data, status)
    assert fresh.first_bad() == (-1, 0)
    # a larger group than any before: the buffers grow
    big = [c for c in good if len(c["data"]) > 60000] * 6
    members = run_group(Z, fresh, big)
    data, status = fresh.collect()
    check_group(big, members, data, status)


def test_invalid_arguments_launch_nothing(Z, fresh):
    from insilicoseq_amd import _native

    lib, h = _native.lib(), fresh._h
    case = IC.good_cases()[2]
    blob = np.frombuffer(case["member"], dtype=np.uint8)
    m, _ = Z.scan(case["member"])
    po, pl, crc, isz = (np.ascontiguousarray(a) for a in (m.pay_off, m.pay_len, m.crc, m.isize))

    def feed(handle=h, data=blob.ctypes.data, n_bytes=blob.size, po=po, pl=pl, crc=crc, isz=isz, n=None):
        ptr = [a.ctypes.data if a is not None else None for a in (po, pl, crc, isz)]
        return lib.iss_inflate_feed(handle, data, n_bytes, ptr[0], ptr[1], ptr[2], ptr[3], po.size if n is None else n)

    E = _native.E_INVALID
    assert feed(handle=None) == E
    assert feed(data=None) == E and feed(po=None, n=1) == E and feed(pl=None) == E and feed(crc=None) == E and feed(isz=None) == E
    assert feed(n_bytes=-1) == E and feed(n=-1) == E
    assert feed(n_bytes=1 << 31) == E  # a group of 2^31 compressed bytes
    n = 32768  # 32768 members of 64 KiB each inflate to 2^31 bytes
    assert feed(po=np.zeros(n, np.int64), pl=np.zeros(n, np.uint32), crc=np.zeros(n, np.uint32), isz=np.full(n, 65536, np.uint32)) == E
    two = lambda a, b, t: np.array([a, b], dtype=t)  # noqa: E731
    ok_pl, ok_crc, ok_isz = two(pl[0], pl[0], np.uint32), two(crc[0], crc[0], np.uint32), two(isz[0], isz[0], np.uint32)
    assert feed(po=two(po[0], po[0], np.int64), pl=ok_pl, crc=ok_crc, isz=ok_isz) == E  # not ascending: the second starts inside the first
    assert feed(po=two(po[0], -1, np.int64), pl=ok_pl, crc=ok_crc, isz=ok_isz) == E
    assert feed(po=np.array([blob.size - 1], np.int64)) == E  # the payload leaves the buffer
    assert feed(po=np.array([blob.size + 1], np.int64), pl=np.zeros(1, np.uint32)) == E
    assert feed(isz=np.array([65537], np.uint32)) == E and feed(pl=np.array([65537], np.uint32), n_bytes=1 << 20) == E
    msg = lib.iss_inflate_last_error(h).decode()
    assert "member 0" in msg and "\n" not in msg
    data, st, nb, nm = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
    assert lib.iss_inflate_collect(h, C.byref(data), C.byref(nb), C.byref(st), C.byref(nm)) == E  # nothing was queued
    assert lib.iss_inflate_collect(None, C.byref(data), C.byref(nb), C.byref(st), C.byref(nm)) == E
    assert lib.iss_inflate_collect(h, None, C.byref(nb), C.byref(st), C.byref(nm)) == E
    assert lib.iss_inflate_first_bad(h, None, None) == E and lib.iss_inflate_kernel_ms(h, None) == E and lib.iss_inflate_reset(None) == E
    assert lib.iss_inflate_create(0, None) == E
    out = C.c_void_p()
    assert lib.iss_inflate_create(1 << 20, C.byref(out)) == E and not out
    assert feed(n=0) == 0 and fresh.first_bad() == (-1, 0) and fresh.kernel_ms() == 0.0  # nothing ran
    # and the context still works
    assert feed() == 0
    fresh.in_flight += 1
    got, status = fresh.collect()
    assert got.tobytes() == case["data"] and status.tolist() == [0]


# ---------------------------------------------------------------------------------------------------- round trips
@pytest.fixture(scope="module")
def run_outputs(tmp_path_factory):
    """One `generate` run with every BGZF output: .bam, .vcf.gz, _origins.bedpe.gz."""
    tmp = tmp_path_factory.mktemp("inflate_run")
    fasta = str(tmp / "genomes.fasta")
    with open(fasta, "w") as fh:
        for k in range(3):
            fh.write(">rec%d\n%s\n" % (k, "".join(np.random.default_rng(31 + k).choice(list("ACGT"), 6000 + 500 * k))))
    out = str(tmp / "run")
    subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate", "--quiet", "--genomes", fasta, "--model", "novaseq", "-n", "2000",
                    "--seed", "11", "--ubam", "--store_mutations", "--origins", "--bgzip", "--output", out], cwd=ROOT, check=True,
                   timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    return out


def test_own_bam_through_the_device(Z, inf, run_outputs):
    from insilicoseq_amd import bam

    path = run_outputs + ".bam"
    host, dev = bam.BamReader(path), bam.BamReader(path, inflater=inf)
    a, b = list(host.chunks()), list(dev.chunks())
    assert host.header == dev.header and host.references == dev.references and len(a) == len(b) >= 1
    assert sum(x.offsets.size for x in a) == 2000
    for x, y in zip(a, b):
        assert np.array_equal(x.data, y.data) and np.array_equal(x.offsets, y.offsets)


@pytest.mark.parametrize("suffix", [".vcf.gz", "_origins.bedpe.gz"])
def test_own_bgzf_text_through_the_device(Z, inf, run_outputs, suffix):
    from insilicoseq_amd import bgzf

    path = run_outputs + suffix
    want = bgzf.read(path)
    assert len(want) > 1000 and want == gzip.open(path, "rb").read()
    for group_bytes in (1 << 16, 32 << 20):
        got = b"".join(p.tobytes() for p in Z.inflate_file(path, inflater=inf, group_bytes=group_bytes, accept_trailing=False))
        assert got == want
    with Z.BgzfReader(path, 0, group_bytes=1 << 16) as fh:  # (a context of its own)
        assert fh.read() == want


def test_model_device_route_against_host_route(Z, tmp_path, monkeypatch):
    from insilicoseq_amd import modeller

    path = str(tmp_path / "m.bam")
    bam_synth.write_bam(path, 21, n_pairs=1500)
    timings = {}
    dev_npz = modeller.to_model(path, str(tmp_path / "dev"), device_inflate=True, timings=timings)
    monkeypatch.setenv("ISS_DEVICE_INFLATE", "1")
    with modeller.device_inflater(0) as d:
        assert isinstance(d, Z.BgzfInflater)
    monkeypatch.setenv("ISS_HOST_INFLATE", "1")
    with modeller.device_inflater(0, True) as d:
        assert d is None
    host_npz = modeller.to_model(path, str(tmp_path / "host"))
    a, b = np.load(dev_npz, allow_pickle=True), np.load(host_npz, allow_pickle=True)
    assert a.files == b.files
    import pickle

    for k in a.files:
        assert pickle.dumps(a[k]) == pickle.dumps(b[k]), k
    monkeypatch.delenv("ISS_HOST_INFLATE")
    monkeypatch.delenv("ISS_DEVICE_INFLATE")
    # a broken block on the device route: the prefix of the host route, the member's offset and the status name
    raw = bytearray(open(path, "rb").read())
    second = int(Z.scan(bytes(raw))[0].offset[1])
    raw[second + 18 + 200] ^= 0x20
    open(path, "wb").write(bytes(raw))
    with Z.BgzfInflater(0) as d:
        from insilicoseq_amd import bam

        with pytest.raises(bam.BamError) as e:
            list(bam.BamReader(path, inflater=d).chunks())
    assert str(e.value).startswith("corrupt BGZF block:") and "byte %d" % second in str(e.value)
    assert str(e.value).split(": ")[-1] in IC.STATUS_NAMES[1:]


def test_report_on_bgzf_fastq_against_the_plain_file(Z, tmp_path):
    from insilicoseq_amd import bgzf
    from insilicoseq_amd.fastq_report import FastqTally

    r1, r2 = FC.mixed(600, 41, (0, 30, 75, 151)), FC.mixed(600, 42, (75, 151))
    paths = {}
    for tag, text in (("R1", r1), ("R2", r2)):
        paths[tag] = str(tmp_path / ("x_%s.fastq" % tag))
        open(paths[tag], "wb").write(text)
        with open(paths[tag] + ".gz", "wb") as fh:
            for at in range(0, len(text), 20000):  # (members that cut records anywhere)
                bgzf.write_member(fh, text[at:at + 20000])
            fh.write(bgzf.EOF_BLOCK)
        assert Z.is_bgzf(paths[tag] + ".gz")
    res = []
    for suffix in ("", ".gz"):
        with FastqTally(0) as dev:
            dev.feed_file(paths["R1"] + suffix, 0, chunk_bytes=50000)
            dev.feed_file(paths["R2"] + suffix, 1, chunk_bytes=50000)
            res.append(dev.result())
    assert res[0]["records"] == res[1]["records"] == [600, 600] and res[1]["bad_record"] == [-1, -1]
    assert np.array_equal(res[0]["tally"], res[1]["tally"]) and np.array_equal(res[0]["lengths"], res[1]["lengths"])
    # a bad member: one error line, status 1
    raw = bytearray(open(paths["R2"] + ".gz", "rb").read())
    second = int(Z.scan(bytes(raw))[0].offset[1])
    raw[second + 18 + 50] ^= 0x01
    open(paths["R2"] + ".gz", "wb").write(bytes(raw))
    run = subprocess.run([sys.executable, "-m", "insilicoseq_amd", "report", "--quiet", "-1", paths["R1"] + ".gz", "-2", paths["R2"] + ".gz",
                          "-o", str(tmp_path / "y")], cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    lines = run.stderr.strip().splitlines()
    assert run.returncode == 1 and len(lines) == 1 and lines[0].startswith("ERROR") and "byte %d" % second in lines[0], run.stderr
    assert paths["R2"] + ".gz" in lines[0] and not os.path.exists(str(tmp_path / "y_tally.npy"))
