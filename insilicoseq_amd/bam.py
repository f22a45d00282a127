"""BAM input of `model` (the reference's `iss model`, iss/bam.py:14-46): BGZF inflate on the host or, given an inflater, on the device
(inflate.py), record boundaries in the HIP library's host code, the subsample.

A BAM file is a series of BGZF blocks (gzip members carrying a ``BC`` extra field with the block size, SAM/BAM specification
section 4.1).  ``BamReader`` inflates them with ``zlib`` in a pool of at most 16 threads (``zlib`` releases the GIL), parses the
header and hands out *chunks*: contiguous bytes holding whole alignment records, with the byte offset of every record's
``block_size`` field found by ``iss_bam_scan`` (the ``block_size`` chain, C++).  A chunk holds about ``chunk_bytes`` of records,
so a file of any size streams through in bounded memory.  Nothing here loops over records in Python.

Mapped records (``flag & 4 == 0``) are counted from the records themselves.  The reference reads that count from the ``.bai``
index (``pysam.idxstats``); the two agree for a consistent index, and this module does not need the index.
"""
import collections
import concurrent.futures as cf
import ctypes as C
import os
import struct
import time
import zlib

import numpy as np

from . import _native

MAX_THREADS = 16
BGZF_MAGIC = b"\x1f\x8b\x08\x04"
DEFAULT_N_READS = 1000000  # read_bam(bam_file, n_reads=1000000), iss/bam.py:14


class BamError(ValueError):
    """A file this module cannot read as BAM, or a record the reference would fail on: one line of text."""


Chunk = collections.namedtuple("Chunk", "data offsets")  # data: np.uint8 record bytes, offsets: np.int64 (block_size fields)


def _inflate_group(blocks):
    out = []
    for cdata, crc, isize in blocks:
        try:
            raw = zlib.decompress(cdata, -15)
        except zlib.error as e:
            raise BamError("corrupt BGZF block: %s" % e)
        if len(raw) != isize or (zlib.crc32(raw) & 0xFFFFFFFF) != crc:
            raise BamError("corrupt BGZF block: size or CRC32 mismatch")
        out.append(raw)
    return b"".join(out)


def _block_groups(fh, read_bytes, group_bytes):
    """Compressed BGZF blocks, in groups of about group_bytes of output, as (cdata, crc, isize) lists."""
    pending = b""
    group, size = [], 0
    first = True
    while True:
        piece = fh.read(read_bytes)
        buf = pending + piece
        pos = 0
        while pos + 18 <= len(buf):
            if buf[pos:pos + 4] != BGZF_MAGIC:
                raise BamError("not a BAM file (no BGZF block at byte %d)" % (fh.tell() - len(buf) + pos) if not first else
                               "not a BAM file (no BGZF header)")
            xlen = struct.unpack_from("<H", buf, pos + 10)[0]
            if pos + 12 + xlen > len(buf):
                break
            bsize, x = None, pos + 12
            while x + 4 <= pos + 12 + xlen:
                si1, si2, slen = buf[x], buf[x + 1], struct.unpack_from("<H", buf, x + 2)[0]
                if si1 == 66 and si2 == 67 and slen == 2:
                    bsize = struct.unpack_from("<H", buf, x + 4)[0] + 1
                x += 4 + slen
            if bsize is None:
                raise BamError("not a BAM file (gzip member without the BGZF BC field)")
            if pos + bsize > len(buf):
                break
            crc, isize = struct.unpack_from("<II", buf, pos + bsize - 8)
            group.append((buf[pos + 12 + xlen:pos + bsize - 8], crc, isize))
            size += isize
            first = False
            pos += bsize
            if size >= group_bytes:
                yield group
                group, size = [], 0
        pending = buf[pos:]
        if not piece:
            if pending:
                raise BamError("truncated BGZF block at the end of the file" if not first else "not a BAM file (too short)")
            if first:
                raise BamError("not a BAM file (empty)")
            break
    if group:
        yield group


def inflate(path, threads=None, read_bytes=16 << 20, group_bytes=4 << 20):
    """The decompressed bytes of a BGZF file, in order, as pieces of about group_bytes."""
    threads = max(1, min(MAX_THREADS, threads or os.cpu_count() or 1))
    with open(path, "rb") as fh, cf.ThreadPoolExecutor(threads) as pool:
        window = collections.deque()
        for group in _block_groups(fh, read_bytes, group_bytes):
            window.append(pool.submit(_inflate_group, group))
            if len(window) >= 2 * threads:
                yield window.popleft().result()
        while window:
            yield window.popleft().result()


def scan(data, base=0, capacity=None):
    """Record boundaries of inflated record bytes (``iss_bam_scan``): (offsets of the block_size fields, bytes covered)."""
    arr = np.frombuffer(data, dtype=np.uint8)
    n_bytes = arr.size - base
    cap = capacity if capacity is not None else n_bytes // 36 + 1
    offs = np.empty(cap, dtype=np.int64)
    n, used = C.c_int64(), C.c_int64()
    lib = _native.lib()
    rc = lib.iss_bam_scan(arr.ctypes.data + base, n_bytes, offs.ctypes.data, cap, C.byref(n), C.byref(used))
    if rc < 0:
        raise BamError(lib.iss_bam_last_error(None).decode())
    return offs[:n.value] + base, used.value


class BamReader(object):
    """Header and record chunks of a BAM file.  ``header`` is the SAM text, ``references`` the (name, length) list."""

    def __init__(self, path, chunk_bytes=64 << 20, threads=None, inflater=None):
        """``inflater``: an inflate.BgzfInflater -- the BGZF blocks are then inflated on its device; None: in the host pool."""
        self.path = path
        self.chunk_bytes = int(chunk_bytes)
        self.threads = threads
        self.inflater = inflater
        self.header = None
        self.references = None
        self.timings = collections.Counter()  # seconds: inflate (waiting for the pool), scan

    def _device_pieces(self):
        from . import inflate as device_inflate

        try:
            # (a member with bytes behind its final block is taken, as zlib.decompress takes it on the host route)
            for piece in device_inflate.inflate_file(self.path, inflater=self.inflater, accept_trailing=True):
                yield memoryview(piece)
        except device_inflate.InflateError as e:
            if e.status is not None:
                raise BamError("corrupt BGZF block: byte %d of the file: %s" % (e.offset, e.status))
            raise BamError("not a BAM file (%s)" % e)

    def _pieces(self):
        it = inflate(self.path, self.threads) if self.inflater is None else self._device_pieces()
        while True:
            t0 = time.perf_counter()
            try:
                piece = next(it)
            except StopIteration:
                self.timings["inflate"] += time.perf_counter() - t0
                return
            self.timings["inflate"] += time.perf_counter() - t0
            yield piece

    def chunks(self):
        """Yield Chunk(data, offsets) with whole records, in file order."""
        pieces = self._pieces()
        buf = bytearray()
        eof = False

        def need(n):
            nonlocal eof
            while len(buf) < n and not eof:
                try:
                    buf.extend(next(pieces))
                except StopIteration:
                    eof = True
            return len(buf) >= n

        if not need(12) or bytes(buf[:4]) != b"BAM\x01":
            raise BamError("not a BAM file (no BAM magic after inflating)")
        l_text = struct.unpack_from("<i", buf, 4)[0]
        if l_text < 0 or not need(12 + l_text):
            raise BamError("truncated BAM header")
        self.header = bytes(buf[8:8 + l_text]).split(b"\0", 1)[0].decode("utf-8", "replace")
        pos = 8 + l_text
        n_ref = struct.unpack_from("<i", buf, pos)[0]
        pos += 4
        refs = []
        for _ in range(max(0, n_ref)):
            if not need(pos + 4):
                raise BamError("truncated BAM header")
            ln = struct.unpack_from("<i", buf, pos)[0]
            if ln < 1 or not need(pos + 8 + ln):
                raise BamError("truncated BAM header")
            refs.append((bytes(buf[pos + 4:pos + 3 + ln]).decode("utf-8", "replace"), struct.unpack_from("<i", buf, pos + 4 + ln)[0]))
            pos += 8 + ln
        self.references = refs
        del buf[:pos]
        while True:
            need(self.chunk_bytes)
            if not buf:
                return
            data = bytes(buf)
            t0 = time.perf_counter()
            offs, used = scan(data)
            self.timings["scan"] += time.perf_counter() - t0
            if used == 0:
                if eof:
                    raise BamError("truncated BAM record at the end of the file")
                need(len(buf) + self.chunk_bytes)  # one record larger than a chunk
                continue
            yield Chunk(np.frombuffer(data, dtype=np.uint8, count=used), offs)
            del buf[:used]


def mapped_mask(chunk):
    """flag & 4 == 0 of every record of a chunk (``not read.is_unmapped``)."""
    o = chunk.offsets
    flag = chunk.data[o + 18].astype(np.uint16) | (chunk.data[o + 19].astype(np.uint16) << 8)
    return (flag & 4) == 0


class Subsample(object):
    """read_bam's selection (iss/bam.py:34-46) over the mapped records of a file, chunk by chunk.

    The fraction is n_reads / total (mapped records).  At a fraction of 1 or more every mapped record is taken, as in the reference.
    Below 1 the reference compares an unseeded ``random()`` with the fraction; here the uniform of the k-th mapped record is the k-th
    double of numpy's Philox generator keyed by ``seed`` -- the same selection law, not the same draws.  The stop rule is the
    reference's: once ``c >= n_reads`` records are taken, the first record that is not taken ends the read."""

    def __init__(self, total, n_reads=DEFAULT_N_READS, seed=0):
        if total <= 0:
            raise BamError("no mapped reads in the BAM file")
        self.fraction = n_reads / total
        self.n_reads = n_reads
        self.taken = 0
        self.stopped = False
        self._gen = None if self.fraction >= 1 else np.random.Generator(np.random.Philox(key=int(seed or 0)))

    def select(self, mapped):
        """uint8 selection of one chunk's records (mapped: bool per record)."""
        if self.stopped:
            return np.zeros(mapped.size, dtype=np.uint8)
        take = mapped.copy()
        if self._gen is not None:
            u = self._gen.random(int(mapped.sum()))
            take[mapped] = u < self.fraction
        before = self.taken + np.cumsum(take) - take
        stop = np.flatnonzero(~take & (before >= self.n_reads))
        if stop.size:
            take[stop[0]:] = False
            self.stopped = True
        self.taken += int(take.sum())
        return take.astype(np.uint8)
