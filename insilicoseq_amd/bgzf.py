"""BGZF on the host (SAM/BAM specification 4.1): the file frame of `generate --bgzip` and a small writer and reader.

A BGZF file is a series of gzip members, each with the ``BC`` extra field that holds its own size (BSIZE = size - 1), each
inflating on its own, ended by the 28-byte empty member ``EOF_BLOCK``.  The workers' ``.vcf`` and ``_origins.bedpe`` temp files
hold members compressed on the device (iss_bgzf_text.hip.h); the parent puts a header member built here in front (VCF), appends
the workers' members in worker order and ends the file with ``EOF_BLOCK`` (``assemble``).  ``compress_file`` is the host route of
the same container, for the one text that is not compressed on the device (the side-by-side worker set's VCF).  ``gzip.open``,
``zcat`` and htslib read all of it."""
import os
import struct
import zlib

BLOCK = 32768  # text bytes per member, like the device's (a member holds at most 65 536 bytes, BSIZE is a uint16)
EOF_BLOCK = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x1b, 0x00, 0x03, 0x00,
                   0, 0, 0, 0, 0, 0, 0, 0])
_HEAD = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00])  # ... BSIZE follows


class BgzfError(ValueError):
    pass


def member(data, level=6):
    """One BGZF member of ``data`` (at most 65 280 bytes, so that incompressible data still fits BSIZE)."""
    data = bytes(data)
    if len(data) > 65280:
        raise BgzfError("a BGZF member holds at most 65280 bytes of data here, not %d" % len(data))
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    size = len(_HEAD) + 2 + len(body) + 8
    if size > 65536:
        raise BgzfError("BGZF member of %d bytes" % size)
    return _HEAD + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def write_member(fh, data, level=6):
    """Append ``data`` to the binary file ``fh`` as BGZF members of at most ``BLOCK`` bytes each (none for no data)."""
    data = bytes(data)
    for at in range(0, len(data), BLOCK):
        fh.write(member(data[at:at + BLOCK], level))


def members(path):
    """The members of a BGZF file, the EOF block included: [(offset, size, inflated data)].  Every member must carry the ``BC``
    field, the BSIZE chain must end exactly at the file's end, every member must inflate ALONE (empty window) and match its
    CRC-32 and ISIZE; anything else raises BgzfError."""
    with open(path, "rb") as fh:
        raw = fh.read()
    return members_of(raw)


def members_of(raw):
    out, pos = [], 0
    while pos < len(raw):
        if pos + 18 > len(raw) or raw[pos:pos + 4] != b"\x1f\x8b\x08\x04" or raw[pos + 10:pos + 16] != b"\x06\x00BC\x02\x00":
            raise BgzfError("no BGZF member header at byte %d" % pos)
        size = struct.unpack_from("<H", raw, pos + 16)[0] + 1
        if size < 26 or pos + size > len(raw):
            raise BgzfError("BSIZE of the member at byte %d leads past the end of the file" % pos)
        d = zlib.decompressobj(-15)
        data = d.decompress(raw[pos + 18:pos + size - 8])
        if not d.eof or d.unused_data:
            raise BgzfError("the member at byte %d does not end where its BSIZE says" % pos)
        crc, isize = struct.unpack_from("<II", raw, pos + size - 8)
        if crc != (zlib.crc32(data) & 0xffffffff) or isize != len(data):
            raise BgzfError("CRC-32 or ISIZE of the member at byte %d" % pos)
        out.append((pos, size, data))
        pos += size
    return out


def read(path):
    """The content of a BGZF file (every member checked, see ``members``); the file must end with ``EOF_BLOCK``."""
    ms = members(path)
    with open(path, "rb") as fh:
        fh.seek(max(0, os.path.getsize(path) - len(EOF_BLOCK)))
        if fh.read() != EOF_BLOCK:
            raise BgzfError("%s does not end with the BGZF EOF block" % path)
    return b"".join(m[2] for m in ms)


def assemble(target, paths, header=None, cleanup=True):
    """``target`` = a member of ``header`` (bytes; None: none), the member streams in ``paths`` in order, ``EOF_BLOCK``.  A missing
    path is an error before anything is written (a worker without a chunk, like concatenate_rank_files); the paths are removed
    afterwards.  No members at all: the EOF block alone."""
    from .distributed import _append_file

    for path in paths:
        if not os.path.exists(path):
            raise FileNotFoundError(path)
    with open(target, "wb") as out:
        if header:
            write_member(out, header)
        for path in paths:
            _append_file(path, out)
        out.seek(0, os.SEEK_END)
        out.write(EOF_BLOCK)
    if cleanup:
        for path in paths:
            os.remove(path)
    return target


def compress_file(path, threads=None, level=6):
    """``path`` -> ``path + ".gz"`` as BGZF (members of ``BLOCK`` bytes compressed on host threads -- zlib releases the GIL --,
    then ``EOF_BLOCK``), the original removed: app.compress_file's counterpart in this container."""
    from concurrent.futures import ThreadPoolExecutor

    threads = threads or min(16, os.cpu_count() or 1)
    batch = 64 * BLOCK

    def piece(data):
        return b"".join(member(data[at:at + BLOCK], level) for at in range(0, len(data), BLOCK))

    with open(path, "rb") as fi, open(path + ".gz", "wb") as fo, ThreadPoolExecutor(threads) as pool:
        pending = []
        while True:
            data = fi.read(batch)
            if data:
                pending.append(pool.submit(piece, data))
            while pending and (not data or len(pending) >= 2 * threads):
                fo.write(pending.pop(0).result())
            if not data:
                break
        fo.write(EOF_BLOCK)
    os.remove(path)
    return path + ".gz"
