"""`generate --device_fasta`: the genome FASTA indexed, and its line ends removed, on the device (include/iss_mi355x.h: iss_fa_*,
iss_fasta_host_index, iss_genome_upload_fasta; kernels csrc/iss_fasta.hip.h, grammar csrc/iss_fasta_core.h).

The host never touches a body: ``read`` maps the file, has it indexed -- on the device (``index_device``) or by the numpy twin
(``index_host``) -- and returns ``generator.Record``s whose ``seq`` is a ``FastaSeq``: a length and a place in the file.
``GenomeStore`` hands runs of such records to ``ReadEngine.add_genomes_fasta``, which sends the file's bytes as they stand.

The grammar, the same as ``generator.parse_fasta(path)``'s:

* a header starts at a ``>`` that is byte 0 or directly follows ``\\n``; bytes in front of the first header are ignored;
* the header's text is the bytes between that ``>`` and the next ``\\n`` (or the end of the text);
* the body runs from behind that ``\\n`` to the next header or the end of the text; its letters are its bytes other than
  ``\\r`` and ``\\n``;
* a body with a byte outside 0x21 .. 0x7E other than those two is flagged ``ODD``: it takes the host parser, errors included.
"""
import collections
import ctypes as C
import mmap
import os

import numpy as np

from . import _native
from .generator import Record, body_letters, read_genome_bytes

ODD = 1  # ISS_FA_ODD
FIRST_CAPACITY = 1 << 16  # rows the first iss_fa_index call of a text has room for (more headers: one call more)

FastaIndex = collections.namedtuple("FastaIndex", "header_off header_len body_off body_len letters flags")
FastaIndex.__doc__ = "The table of a text, one row per record: five int64 arrays and ``flags`` (int32), offsets relative to the text."


def _empty(n):
    return FastaIndex(*([np.empty(n, np.int64) for _ in range(5)] + [np.empty(n, np.int32)]))


def _as_array(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)


def index_host(data):
    """The table of ``data`` (bytes or a uint8 array) with numpy alone: written from the grammar above, the twin every other
    indexer is held to."""
    a = _as_array(data)
    n = a.size
    if not n:
        return _empty(0)
    is_nl = a == 10
    is_eol = is_nl | (a == 13)
    starts = a == 62
    starts[1:] &= is_nl[:-1]
    header_off = np.flatnonzero(starts).astype(np.int64)
    end = np.append(header_off[1:], n).astype(np.int64)
    nl_at = np.flatnonzero(is_nl)
    k = np.searchsorted(nl_at, header_off)  # the first '\n' at or behind the '>'
    eol = np.where(k < nl_at.size, nl_at[np.minimum(k, nl_at.size - 1)], n) if nl_at.size else np.full(k.size, n)
    eol = np.minimum(eol, end).astype(np.int64)  # (a '\n' behind the next header is not this header's)
    body_off = np.where(eol < end, eol + 1, end)
    eol_before = np.concatenate(([0], np.cumsum(is_eol, dtype=np.int64)))
    odd_before = np.concatenate(([0], np.cumsum(~is_eol & ((a < 0x21) | (a > 0x7E)), dtype=np.int64)))
    body_len = end - body_off
    return FastaIndex(header_off, eol - header_off - 1, body_off, body_len, body_len - (eol_before[end] - eol_before[body_off]),
                      np.where(odd_before[end] > odd_before[body_off], ODD, 0).astype(np.int32))


def _index_call(call, data):
    """``call(text address, bytes, capacity, six row addresses, n_records)`` until the rows fit."""
    a = _as_array(data)
    n, cap = C.c_int64(0), FIRST_CAPACITY
    while True:
        rows = _empty(cap)
        call(a.ctypes.data if a.size else None, a.size, cap, *([r.ctypes.data for r in rows] + [C.byref(n)]))
        if n.value <= cap:
            return FastaIndex(*(r[:n.value].copy() for r in rows))
        cap = n.value


def index_native_host(data):
    """The table from the library's host entry (iss_fasta_host_index: the kernels' grammar source compiled for the host, no GPU)."""
    lib = _native.lib()
    _native.need(lib, "fasta")
    return _index_call(lambda *args: _native.check(None, lib.iss_fasta_host_index(*args)), data)


class FastaIndexer(_native.Session):
    """The device session (iss_fa_*): ``index(data)`` is the table of a text held in host memory."""

    PREFIX = "iss_fa"

    def index(self, data):
        return _index_call(lambda *args: self._check(self._lib.iss_fa_index(self._h, *args)), data)


class FastaSource(object):
    """The text of one FASTA file as the records' bodies are cut from it: the file mapped read-only, or -- a gzip file -- its
    inflated bytes.  ``array`` is the uint8 view the uploads take their spans from."""

    def __init__(self, path, device_inflate=None):
        self.path = os.fspath(path)
        self._map = None
        with open(self.path, "rb") as fh:
            magic = fh.read(2)
            size = os.fstat(fh.fileno()).st_size
            if magic == b"\x1f\x8b":
                self.array = np.frombuffer(read_genome_bytes(self.path, device_inflate), dtype=np.uint8)
            elif size:
                self._map = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
                self.array = np.frombuffer(self._map, dtype=np.uint8)
            else:
                self.array = np.empty(0, np.uint8)

    def __len__(self):
        return self.array.size


class FastaSeq(object):
    """A record's ``seq`` under --device_fasta: ``len()`` is its letters, ``raw()`` its body as it stands in the file, ``str()``
    the letters, stripped on the host when somebody asks (nothing is kept).  GenomeStore uploads it through
    ReadEngine.add_genomes_fasta: the body goes to the device with its line ends."""

    __slots__ = ("source", "body_off", "body_len", "letters")

    def __init__(self, source, body_off, body_len, letters):
        self.source, self.body_off, self.body_len, self.letters = source, int(body_off), int(body_len), int(letters)

    def __len__(self):
        return self.letters

    def raw(self):
        return self.source.array[self.body_off:self.body_off + self.body_len]

    def __str__(self):
        return self.raw().tobytes().translate(None, b"\r\n").decode()


def index_device(path_or_data, device=0):
    """The table of a file (mapped; a gzip file: inflated first) or of bytes, from an iss_fa session on ``device``."""
    data = FastaSource(path_or_data).array if isinstance(path_or_data, (str, os.PathLike)) else path_or_data
    with FastaIndexer(device) as fa:
        return fa.index(data)


def records_of(source, index):
    """The Records of an indexed source: ``seq`` a FastaSeq, or -- a record flagged ODD -- the str the host parser makes."""
    a, out = source.array, []
    for h, hl, b, bl, n, f in zip(*(col.tolist() for col in index)):
        header = a[h + 1:h + 1 + hl].tobytes().decode().rstrip("\r\n")
        seq = body_letters(a[b:b + bl].tobytes()) if f & ODD else FastaSeq(source, b, bl, n)
        out.append(Record(seq, id=(header.split(None, 1) or [""])[0], description=header))
    return out


def read(path, device=None, device_inflate=None):
    """The records of a FASTA file, equal to ``list(parse_fasta(path))`` in id, description, len and str, without a pass over the
    bodies on the host: indexed on ``device`` (None: by ``index_host``)."""
    source = FastaSource(path, device_inflate)
    if device is None:
        index = index_host(source.array)
    else:
        with FastaIndexer(device) as fa:
            index = fa.index(source.array)
    return records_of(source, index)


def upload_runs(seqs, gap=1 << 20):
    """How a list of FastaSeq is cut into add_genomes_fasta calls: [(first, last + 1)] over ``seqs``.  A run is records of one
    source in file order; it ends where the next record is of another file, stands in front of the one before, or lies more
    than ``gap`` bytes behind it -- the span of a call is one piece of the file, and what lies between two picked records
    travels with them."""
    runs, first = [], 0
    for k in range(1, len(seqs) + 1):
        if k == len(seqs) or seqs[k].source is not seqs[k - 1].source or seqs[k].body_off < seqs[k - 1].body_off + seqs[k - 1].body_len \
                or seqs[k].body_off - (seqs[k - 1].body_off + seqs[k - 1].body_len) > gap:
            runs.append((first, k))
            first = k
    return runs


__all__ = ["ODD", "FastaIndex", "index_host", "index_native_host", "FastaIndexer", "FastaSource", "FastaSeq", "index_device",
           "records_of", "read", "upload_runs"]
