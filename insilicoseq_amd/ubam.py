"""The frame of `generate --ubam`'s file: what stands around the record blocks the device builds (ReadEngine.ubam_emit_batch).

An unaligned BAM is BGZF blocks (SAM/BAM specification 4.1): first the header -- magic, SAM text, no references -- as one member
built here with ``zlib``, then the workers' record blocks in worker order, then the standard 28-byte EOF block."""
import os
import struct
import zlib

HEADER_TEXT = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@PG\tID:insilicoseq_amd\tPN:insilicoseq_amd\n"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")  # a member's first 16 bytes; BSIZE - 1 (uint16) follows


def bgzf_member(data, level=6):
    """One BGZF member holding ``data`` (at most 65 280 bytes, so that the member stays within BSIZE whatever zlib makes of them)."""
    if len(data) > 65280:
        raise ValueError("a BGZF member holds at most 65280 bytes")
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    size = len(BGZF_HEAD) + 2 + len(body) + 8
    return BGZF_HEAD + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def header_block(text=HEADER_TEXT):
    """The BAM header (magic, l_text, text, n_ref = 0) as one BGZF member."""
    raw = text.encode()
    return bgzf_member(b"BAM\x01" + struct.pack("<i", len(raw)) + raw + struct.pack("<i", 0))


def assemble(target, block_paths):
    """``target`` = header, the record blocks of ``block_paths`` in order (the concatenation rule of the workers' FASTQ files,
    iss/app.py:123-127), the EOF block.  A missing file is an error before anything is written (iss/util.py:233); on any failure
    the partial target is removed.  The block files are removed once the target is whole."""
    from .distributed import _append_file

    for path in block_paths:
        if not os.path.exists(path):
            raise FileNotFoundError(path)
    try:
        with open(target, "wb", buffering=0) as out:
            out.write(header_block())
            for path in block_paths:
                _append_file(path, out)
            out.write(EOF_BLOCK)
    except BaseException:
        if os.path.exists(target):
            os.remove(target)
        raise
    for path in block_paths:
        os.remove(path)
