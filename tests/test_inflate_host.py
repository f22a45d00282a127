"""The BGZF inflate without a GPU: the case table held against zlib (a case zlib disagrees with is a wrong case, not a tolerance),
iss_bgzf_scan through the built library, is_bgzf, and the Python layers above the device context -- inflate_file, BgzfReader,
BamReader(inflater=...) -- on a stand-in inflater that answers with zlib."""
import gzip
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import bam_synth  # noqa: E402
import fastq_cases as FC  # noqa: E402
import inflate_cases as IC  # noqa: E402


@pytest.fixture(scope="module")
def Z():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import inflate

    return inflate


class ZlibInflater(object):
    """BgzfInflater's feed / collect / reset, answered by zlib on the host: status OK, CRC, SHORT, TRAILING or BAD_CODE."""

    def __init__(self):
        self.queue = []
        self.feeds = 0

    def reset(self):
        self.queue = []

    def close(self):
        pass

    def feed(self, data, members):
        data = bytes(data)
        out, status = [], []
        for po, pl, crc, isize in zip(members.pay_off, members.pay_len, members.crc, members.isize):
            d = zlib.decompressobj(-15)
            try:
                raw = d.decompress(data[int(po):int(po) + int(pl)])
                st = IC.SHORT if len(raw) != isize or not d.eof else IC.CRC if zlib.crc32(raw) & 0xFFFFFFFF != crc else \
                    IC.TRAILING if d.unused_data else IC.OK
            except zlib.error:
                raw, st = b"", IC.BAD_CODE
            out.append(raw if len(raw) == isize else bytes(int(isize)))
            status.append(st)
        self.feeds += 1
        if len(status):
            self.queue.append((np.frombuffer(b"".join(out), dtype=np.uint8), np.array(status, dtype=np.uint8)))

    def collect(self):
        return self.queue.pop(0)


# ---------------------------------------------------------------------------------------------------- the table against zlib
def test_table_covers_every_status():
    assert IC.EOF_BLOCK == __import__("insilicoseq_amd.bgzf", fromlist=["EOF_BLOCK"]).EOF_BLOCK
    assert sorted(set(c["status"] for c in IC.bad_cases())) == list(range(1, 11))
    names = [c["name"] for c in IC.all_cases()]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case", IC.good_cases(), ids=lambda c: c["name"])
def test_good_case_is_what_zlib_inflates(case):
    pay, crc, isize = IC.split_member(case["member"])
    d = zlib.decompressobj(-15)
    data = d.decompress(pay)
    assert data == case["data"] and d.eof and d.unused_data == b""
    assert crc == zlib.crc32(data) & 0xFFFFFFFF and isize == len(data) and len(case["member"]) <= 65536
    assert struct.unpack_from("<H", case["member"], case["member"].index(b"BC\x02\x00") + 4)[0] == len(case["member"]) - 1


@pytest.mark.parametrize("case", IC.bad_cases(), ids=lambda c: c["name"])
def test_bad_case_is_bad(case):
    pay, crc, isize = IC.split_member(case["member"])
    d = zlib.decompressobj(-15)
    if case["status"] not in IC.OWN_CHECK:
        try:
            d.decompress(pay)
        except zlib.error:
            return
        assert not d.eof, "zlib takes this stream"
        return
    data = d.decompress(pay)  # zlib takes the stream: the member's own fields, or the payload's end, say no
    assert d.eof
    if case["status"] == IC.CRC:
        assert isize == len(data) and crc != zlib.crc32(data) & 0xFFFFFFFF and d.unused_data == b""
    elif case["status"] == IC.SHORT:
        assert len(data) == isize - 1
    elif case["status"] == IC.OUT_OVERRUN:
        assert len(data) == isize + 1
    else:
        assert isize == len(data) and crc == zlib.crc32(data) & 0xFFFFFFFF and len(d.unused_data) > 0


# ---------------------------------------------------------------------------------------------------- iss_bgzf_scan
def _three():
    by = {c["name"]: c for c in IC.good_cases()}
    return [by["foreign_subfields"]["member"], by["isize_1"]["member"], IC.EOF_BLOCK]


def test_scan_of_buffers_cut_at_every_byte(Z):
    ms = _three()
    blob = b"".join(ms)
    ends = np.cumsum([len(m) for m in ms])
    for cut in range(len(blob) + 1):
        members, used = Z.scan(blob[:cut])
        n = int(np.searchsorted(ends, cut, side="right"))
        assert members.offset.size == n and used == (ends[n - 1] if n else 0), cut
    members, used = Z.scan(blob)
    assert members.offset.tolist() == [0, len(ms[0]), len(ms[0]) + len(ms[1])]
    at = 0
    for k, m in enumerate(ms):
        pay, crc, isize = IC.split_member(m)
        assert blob[members.pay_off[k]:members.pay_off[k] + members.pay_len[k]] == pay
        assert (members.crc[k], members.isize[k]) == (crc, isize)
        at += len(m)
    # the next call starts where this one stopped
    members, used = Z.scan(blob[:len(ms[0]) + 5])
    rest, used2 = Z.scan(blob[used:])
    assert used == len(ms[0]) and rest.offset.size == 2 and used + used2 == len(blob)
    # and a full capacity stops a scan like the buffer's end does
    members, used = Z.scan(blob, capacity=2)
    assert members.offset.size == 2 and used == len(ms[0]) + len(ms[1])


def test_scan_takes_foreign_subfields(Z):
    text = b"subfields\n" * 10
    pay = IC.deflate(text)
    for before, after in ((b"", b""), (b"AB\x00\x00", b""), (b"", b"AB\x04\x00wxyz"), (b"BC\x03\x00abc", b"CB\x02\x00\x01\x02")):
        m = IC.member(pay, text, before=before, after=after)
        members, used = Z.scan(m + IC.EOF_BLOCK)
        assert used == len(m) + 28 and members.pay_off[0] == 12 + len(before) + 6 + len(after) and members.pay_len[0] == len(pay)
        assert members.isize.tolist() == [len(text), 0]


def test_scan_rejections(Z):
    good = _three()[1]
    plain = gzip.compress(b"not blocked")
    no_bc = good[:10] + struct.pack("<H", 6) + b"XY\x02\x00\x00\x00" + good[18:]
    small = bytearray(good)
    struct.pack_into("<H", small, 16, 24)  # BSIZE + 1 = 25
    for blob, word in ((plain, "magic"), (good + b"junkjunkjunkjunk", "magic"), (no_bc, "BC"), (bytes(small), "BSIZE")):
        with pytest.raises(Z.InflateError) as e:
            Z.scan(blob)
        assert word in str(e.value) and "\n" not in str(e.value), str(e.value)
    # the members in front of the bad one are still handed out by the library
    import ctypes as C

    from insilicoseq_amd import _native

    lib = _native.lib()
    blob = np.frombuffer(good + b"junkjunkjunkjunk", dtype=np.uint8)
    off, po = np.zeros(4, np.int64), np.zeros(4, np.int64)
    pl, crc, isz = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    n, used = C.c_int64(), C.c_int64()
    rc = lib.iss_bgzf_scan(blob.ctypes.data, blob.size, off.ctypes.data, po.ctypes.data, pl.ctypes.data, crc.ctypes.data, isz.ctypes.data,
                           4, C.byref(n), C.byref(used))
    assert rc == _native.E_INVALID and n.value == 1 and used.value == len(good)
    assert lib.iss_bgzf_scan(None, 0, None, None, None, None, None, 0, C.byref(n), C.byref(used)) == _native.E_INVALID
    assert lib.iss_bgzf_scan(blob.ctypes.data, -1, off.ctypes.data, po.ctypes.data, pl.ctypes.data, crc.ctypes.data, isz.ctypes.data, 4,
                             C.byref(n), C.byref(used)) == _native.E_INVALID


def test_library_exports_the_inflate_symbols(Z):
    from insilicoseq_amd import _native

    lib = _native.lib()
    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    for name in ("iss_bgzf_scan", "iss_inflate_create", "iss_inflate_destroy", "iss_inflate_last_error", "iss_inflate_reset",
                 "iss_inflate_feed", "iss_inflate_collect", "iss_inflate_first_bad", "iss_inflate_kernel_ms"):
        assert name in _native.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    for code, name in enumerate(IC.STATUS_NAMES):
        assert "#define ISS_BGZF_%s %d" % (name, code) in header and _native.BGZF_STATUS[code] == name
    assert lib.iss_abi_version() == 8


def test_is_bgzf(Z, tmp_path):
    from insilicoseq_amd import bgzf

    def put(name, data):
        path = str(tmp_path / name)
        with open(path, "wb") as fh:
            fh.write(data)
        return path

    assert Z.is_bgzf(put("a.gz", bgzf.member(b"text") + bgzf.EOF_BLOCK))
    assert Z.is_bgzf(put("b.gz", IC.member(IC.deflate(b"x"), b"x", before=b"AB\x01\x00q")))
    assert not Z.is_bgzf(put("c.gz", gzip.compress(b"text")))
    assert not Z.is_bgzf(put("d.gz", b""))
    assert not Z.is_bgzf(put("e.gz", b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x04\x00XY\x00\x00"))
    assert not Z.is_bgzf(put("f.fastq", b"@r\nA\n+\n!\n"))


# ---------------------------------------------------------------------------------------------------- the layers above the context
def _bgzf_file(path, data, block):
    from insilicoseq_amd import bgzf

    with open(path, "wb") as fh:
        for at in range(0, len(data), block):
            fh.write(bgzf.member(data[at:at + block]))
        fh.write(bgzf.EOF_BLOCK)


def test_reader_readinto_against_gzip(Z, tmp_path):
    from insilicoseq_amd import fastq_report

    text = FC.mixed(400, 7, (0, 30, 75, 151))
    path, plain = str(tmp_path / "r.fastq.gz"), str(tmp_path / "r.fastq")
    _bgzf_file(path, text, 5000)
    open(plain, "wb").write(text)
    want = gzip.open(path, "rb").read()
    assert want == text
    for group_bytes, size in ((1 << 16, 1000), (1 << 16, 1 << 20), (1 << 20, 77)):
        got, buf = bytearray(), bytearray(size)
        with Z.BgzfReader(path, group_bytes=group_bytes, inflater=ZlibInflater()) as fh:
            while True:
                n = fh.readinto(buf)
                if not n:
                    break
                got += buf[:n]
            assert fh.readinto(buf) == 0
        assert bytes(got) == want
    with Z.BgzfReader(path, inflater=ZlibInflater()) as fh:
        assert fh.read(10) == want[:10] and fh.read() == want[10:] and fh.read() == b""
    # fastq_report's cutting runs unchanged on top of it
    for chunk_bytes in (777, 1 << 16):
        with Z.BgzfReader(path, group_bytes=1 << 16, inflater=ZlibInflater()) as a, open(plain, "rb") as b:
            assert list(fastq_report.split_chunks(a, chunk_bytes)) == list(fastq_report.split_chunks(b, chunk_bytes))


def test_inflate_file_groups_and_errors(Z, tmp_path):
    data = IC.noise(300000, 11)
    path = str(tmp_path / "n.gz")
    _bgzf_file(path, data, 60000)
    for kw in ({}, {"group_bytes": 1 << 16}, {"group_bytes": 1 << 16, "out_bytes": 1 << 16}, {"depth": 1}):
        inf = ZlibInflater()
        pieces = list(Z.inflate_file(path, inflater=inf, **kw))
        assert b"".join(p.tobytes() for p in pieces) == data and inf.queue == []
    assert len(list(Z.inflate_file(path, inflater=ZlibInflater(), group_bytes=1 << 16, out_bytes=1 << 16))) == 5  # (the EOF block rides along)
    raw = open(path, "rb").read()
    # a bad member: its file offset and its status name
    second = Z.scan(raw)[0].offset[1]
    broken = bytearray(raw)
    broken[second + 18 + 2000] ^= 0x55
    open(path, "wb").write(bytes(broken))
    with pytest.raises(Z.InflateError) as e:
        list(Z.inflate_file(path, inflater=ZlibInflater(), group_bytes=1 << 16))
    assert e.value.offset == second and e.value.status == "CRC" and "byte %d" % second in str(e.value) and path in str(e.value)
    # trailing bytes in a member: taken or not, as the caller says
    text = b"trailing\n" * 100
    open(path, "wb").write(IC.member(IC.deflate(text) + b"\0", text) + IC.EOF_BLOCK)
    assert b"".join(p.tobytes() for p in Z.inflate_file(path, inflater=ZlibInflater())) == text
    with pytest.raises(Z.InflateError) as e:
        list(Z.inflate_file(path, inflater=ZlibInflater(), accept_trailing=False))
    assert e.value.status == "TRAILING" and e.value.offset == 0
    # the container itself
    open(path, "wb").write(raw[:-40])
    with pytest.raises(Z.InflateError) as e:
        list(Z.inflate_file(path, inflater=ZlibInflater()))
    assert "truncated" in str(e.value) and e.value.status is None
    open(path, "wb").write(gzip.compress(b"plain gzip"))
    with pytest.raises(Z.InflateError) as e:
        list(Z.inflate_file(path, inflater=ZlibInflater()))
    assert "magic" in str(e.value) and e.value.status is None


def test_bam_reader_with_an_inflater_reads_what_the_pool_reads(Z, tmp_path):
    from insilicoseq_amd import bam

    path = str(tmp_path / "s.bam")
    bam_synth.write_bam(path, 3, n_pairs=300)
    host = bam.BamReader(path, chunk_bytes=1 << 15)
    dev = bam.BamReader(path, chunk_bytes=1 << 15, inflater=ZlibInflater())
    a, b = list(host.chunks()), list(dev.chunks())
    assert len(a) == len(b) >= 1 and host.header == dev.header and host.references == dev.references
    for x, y in zip(a, b):
        assert np.array_equal(x.data, y.data) and np.array_equal(x.offsets, y.offsets)
    raw = bytearray(open(path, "rb").read())
    second = Z.scan(bytes(raw))[0].offset[1]
    raw[second + 18 + 100] ^= 0x04
    open(path, "wb").write(bytes(raw))
    with pytest.raises(bam.BamError) as e:
        list(bam.BamReader(path, inflater=ZlibInflater()).chunks())
    assert str(e.value).startswith("corrupt BGZF block:") and "byte %d" % second in str(e.value)
    with pytest.raises(bam.BamError) as e2:
        list(bam.BamReader(path).chunks())
    assert str(e2.value).startswith("corrupt BGZF block:")
    open(path, "wb").write(b"no BAM at all, plain text of some length")
    with pytest.raises(bam.BamError) as e:
        list(bam.BamReader(path, inflater=ZlibInflater()).chunks())
    assert str(e.value).startswith("not a BAM file")


def test_host_switch(Z, monkeypatch, tmp_path):
    """ISS_HOST_INFLATE=1 keeps both commands on the host route; so does a gzip file that is no BGZF."""
    from insilicoseq_amd import fastq_report, modeller

    path, other = str(tmp_path / "a.fastq.gz"), str(tmp_path / "b.fastq.gz")
    _bgzf_file(path, b"@r\nA\n+\n!\n", 100)
    open(other, "wb").write(gzip.compress(b"@r\nA\n+\n!\n"))
    with fastq_report.open_fastq(other, 0) as fh:
        assert isinstance(fh, gzip.GzipFile)
    with fastq_report.open_fastq(path) as fh:
        assert isinstance(fh, gzip.GzipFile) and fh.read() == b"@r\nA\n+\n!\n"
    with modeller.device_inflater(0) as inf:  # `model` keeps the host pool unless it is asked
        assert inf is None
    monkeypatch.setenv("ISS_HOST_INFLATE", "1")
    with modeller.device_inflater(0, True) as inf:
        assert inf is None
    with fastq_report.open_fastq(path, 0) as fh:
        assert isinstance(fh, gzip.GzipFile)
