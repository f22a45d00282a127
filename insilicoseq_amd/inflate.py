"""BGZF inflate on the device (include/iss_mi355x.h: iss_bgzf_scan, iss_inflate_*; k_bgzf_inflate of csrc/iss_inflate.hip.h): the
BAM input of `model` and BGZF-compressed FASTQ in `report`.

``scan`` walks the BSIZE chain of a buffer on the host (no GPU).  ``BgzfInflater`` is the device context: ``feed`` takes a buffer of
whole members with the scan's arrays and returns once the bytes are in a pinned staging buffer, ``collect`` hands back the oldest
group's inflated bytes and one status per member.  ``inflate_file`` streams a file through it, two groups in flight, and yields the
inflated pieces as ``bam.inflate`` does; ``BgzfReader`` puts a ``readinto`` on top, so that a reader written for plain files
(``fastq_report``'s chunk cutting) runs unchanged.  DESIGN.md section 27."""
import collections
import ctypes as C

import numpy as np

from . import _native

STATUS = _native.BGZF_STATUS
OK, TRAILING = _native.BGZF_OK, _native.BGZF_TRAILING
MAGIC = b"\x1f\x8b\x08\x04"

Members = collections.namedtuple("Members", "offset pay_off pay_len crc isize")  # int64, int64, uint32, uint32, uint32 arrays


class InflateError(ValueError):
    """A buffer that is no BGZF, or a member that does not inflate: one line.  ``offset``: the member's byte offset in the file (or
    buffer), ``status``: its ISS_BGZF_* name (None: the container itself is bad)."""

    def __init__(self, message, offset=None, status=None):
        ValueError.__init__(self, message)
        self.offset = offset
        self.status = status


def scan(data, capacity=None):
    """The whole members at the start of ``data`` (``iss_bgzf_scan``): (Members, bytes covered).  An incomplete member at the end is
    left out; a buffer that is no BGZF raises InflateError."""
    arr = np.frombuffer(data, dtype=np.uint8)
    cap = int(capacity) if capacity is not None else arr.size // 26 + 1
    m = Members(np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.uint32), np.empty(cap, np.uint32),
                np.empty(cap, np.uint32))
    n, used = C.c_int64(), C.c_int64()
    lib = _native.lib()
    rc = lib.iss_bgzf_scan(arr.ctypes.data if arr.size else m.offset.ctypes.data, arr.size, m.offset.ctypes.data, m.pay_off.ctypes.data,
                           m.pay_len.ctypes.data, m.crc.ctypes.data, m.isize.ctypes.data, cap, C.byref(n), C.byref(used))
    if rc < 0:
        raise InflateError(lib.iss_inflate_last_error(None).decode(), offset=used.value)
    return Members(*(a[:n.value] for a in m)), used.value


def is_bgzf(path):
    """True when the file starts with a gzip member that carries the BGZF ``BC`` subfield."""
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] != MAGIC:
            return False
        xlen = head[10] | head[11] << 8
        extra = fh.read(xlen)
    x = 0
    while x + 4 <= len(extra):
        slen = extra[x + 2] | extra[x + 3] << 8
        if extra[x:x + 2] == b"BC" and slen == 2 and x + 6 <= len(extra):
            return True
        x += 4 + slen
    return False


class BgzfInflater(_native.Session):
    """The device context (iss_inflate_*): feed groups of whole members, collect their inflated bytes in feed order."""

    PREFIX = "iss_inflate"

    def __init__(self, device=0):
        self.in_flight = 0
        _native.Session.__init__(self, device)

    def reset(self):
        """Drops what is in flight, the first-bad word and the kernel time."""
        _native.Session.reset(self)
        self.in_flight = 0

    def feed(self, data, members):
        """One group: ``data`` (bytes or any buffer) and the ``Members`` of ``scan`` (offsets relative to ``data``).  The bytes are
        free again when the call returns.  A group without members queues nothing."""
        a = np.frombuffer(data, dtype=np.uint8)
        pay_off = np.ascontiguousarray(members.pay_off, dtype=np.int64)
        pay_len = np.ascontiguousarray(members.pay_len, dtype=np.uint32)
        crc = np.ascontiguousarray(members.crc, dtype=np.uint32)
        isize = np.ascontiguousarray(members.isize, dtype=np.uint32)
        n = pay_off.size
        if not (pay_len.size == crc.size == isize.size == n):
            raise ValueError("the member arrays differ in length")
        self._check(self._lib.iss_inflate_feed(self._h, a.ctypes.data if a.size else None, a.size, pay_off.ctypes.data, pay_len.ctypes.data,
                                               crc.ctypes.data, isize.ctypes.data, n))
        if n:
            self.in_flight += 1

    def collect(self, copy=True):
        """The oldest group in flight: (inflated bytes as a uint8 array -- member m at the exclusive sum of ISIZE --, one ISS_BGZF_*
        status per member).  copy=False: views of the context's pinned memory, good until the next collect, reset or close."""
        data, status = C.c_void_p(), C.c_void_p()
        n_bytes, n_members = C.c_int64(), C.c_int64()
        self._check(self._lib.iss_inflate_collect(self._h, C.byref(data), C.byref(n_bytes), C.byref(status), C.byref(n_members)))
        self.in_flight -= 1
        out = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), (n_bytes.value,)) if n_bytes.value else np.empty(0, np.uint8)
        st = np.ctypeslib.as_array(C.cast(status, C.POINTER(C.c_uint8)), (n_members.value,))
        return (out.copy(), st.copy()) if copy else (out, st)

    def first_bad(self):
        """(member index over all feeds since the last reset, status) of the first bad member, or (-1, 0); waits for every kernel."""
        member, code = C.c_int64(), C.c_int32()
        self._check(self._lib.iss_inflate_first_bad(self._h, C.byref(member), C.byref(code)))
        return member.value, code.value


def check_status(status, members, base=0, accept_trailing=True):
    """Raises InflateError for the first member of a collected group that is not OK (or TRAILING, when that is accepted)."""
    bad = status != OK
    if accept_trailing:
        bad &= status != TRAILING
    if bad.any():
        m = int(np.flatnonzero(bad)[0])
        name = STATUS[status[m]] if status[m] < len(STATUS) else "status %d" % status[m]
        off = base + int(members.offset[m])
        raise InflateError("member at byte %d: %s" % (off, name), offset=off, status=name)


def inflate_file(path, device=0, group_bytes=32 << 20, inflater=None, accept_trailing=True, depth=2, out_bytes=1 << 30):
    """The inflated bytes of a BGZF file, in order, as one uint8 array per group of about ``group_bytes`` compressed bytes (and at most
    ``out_bytes`` inflated ones: text that compresses very well is cut into more groups).  ``depth`` groups are on the device while
    the next is read and scanned.  ``inflater``: a BgzfInflater to use (it is reset) instead of one made for ``device`` and closed at
    the end.  A bad member raises InflateError with its file offset and status name; an incomplete member at the end of the file,
    or a file that is no BGZF, raises it without a status."""
    own = inflater is None
    inf = BgzfInflater(device) if own else inflater
    group_bytes = max(1 << 16, int(group_bytes))
    out_bytes = max(1 << 16, min(int(out_bytes), (1 << 31) - 1))
    try:
        inf.reset()
        queue = collections.deque()  # (Members, file offset of the group's buffer) per group in flight

        def oldest():
            members, base = queue.popleft()
            data, status = inf.collect()
            try:
                check_status(status, members, base, accept_trailing)
            except InflateError as e:
                raise InflateError("%s: %s" % (path, e), e.offset, e.status)
            return data

        with open(path, "rb") as fh:
            tail, at, seen = b"", 0, False
            while True:
                piece = fh.read(group_bytes)
                buf = tail + piece if tail else piece
                if not buf:
                    break
                try:
                    members, used = scan(buf)
                except InflateError as e:
                    raise InflateError("%s: %s" % (path, e), offset=at + (e.offset or 0))
                n = members.offset.size
                seen = seen or n > 0
                lo = 0
                while lo < n:  # (one round, unless the group inflates to more than out_bytes)
                    total = np.cumsum(members.isize[lo:], dtype=np.int64)
                    hi = lo + max(1, int(np.searchsorted(total, out_bytes, side="right")))
                    first = int(members.offset[lo])
                    end = int(members.pay_off[hi - 1]) + int(members.pay_len[hi - 1]) + 8
                    part = Members(members.offset[lo:hi] - first, members.pay_off[lo:hi] - first, members.pay_len[lo:hi],
                                   members.crc[lo:hi], members.isize[lo:hi])
                    inf.feed(memoryview(buf)[first:end], part)
                    queue.append((part, at + first))
                    if len(queue) >= depth:
                        yield oldest()
                    lo = hi
                tail = buf[used:]
                at += used
                if not piece:
                    if tail:
                        raise InflateError("%s: truncated BGZF member at byte %d" % (path, at) if seen or len(tail) >= 4 else
                                           "%s: too short for a BGZF member" % path, offset=at)
                    break
        while queue:
            yield oldest()
    finally:
        if own:
            inf.close()
        else:
            inf.reset()


class BgzfReader(object):
    """A binary reader over the inflated bytes of a BGZF file: ``readinto`` / ``read`` / ``close``, a context manager.  ``pieces``: an
    iterator of buffers (``inflate_file`` by default)."""

    def __init__(self, path=None, device=0, group_bytes=32 << 20, inflater=None, pieces=None):
        self._pieces = pieces if pieces is not None else inflate_file(path, device, group_bytes, inflater, accept_trailing=False)
        self._cur = memoryview(b"")
        self._eof = False

    def readable(self):
        return True

    def _fill(self):
        while not len(self._cur) and not self._eof:
            try:
                self._cur = memoryview(next(self._pieces)).cast("B")
            except StopIteration:
                self._eof = True
        return len(self._cur)

    def readinto(self, b):
        view = memoryview(b).cast("B")
        if not len(view) or not self._fill():
            return 0
        n = min(len(view), len(self._cur))
        view[:n] = self._cur[:n]
        self._cur = self._cur[n:]
        return n

    def read(self, size=-1):
        out = bytearray()
        while (size < 0 or len(out) < size) and self._fill():
            n = len(self._cur) if size < 0 else min(len(self._cur), size - len(out))
            out += self._cur[:n]
            self._cur = self._cur[n:]
        return bytes(out)

    def close(self):
        self._eof = True
        self._cur = memoryview(b"")
        close = getattr(self._pieces, "close", None)
        if close:
            close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


__all__ = ["STATUS", "OK", "TRAILING", "Members", "InflateError", "scan", "is_bgzf", "BgzfInflater", "check_status", "inflate_file",
           "BgzfReader"]
