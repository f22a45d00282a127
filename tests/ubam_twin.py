"""A host twin of the device's unaligned BAM (iss_ubam.hip.h, iss_api_ubam.hip.h).

records() restates the record layout with numpy and struct (SAM/BAM specification 4.2, the fields `generate --ubam` fills).
members() is the BGZF stream the library has to write for a call's record bytes, bit for bit: deflate_twin's tokenizer run over
every 32 768-byte block ON ITS OWN -- the member rule: no predecessor byte at a block's start, no previous-record source before
it -- one code for the call (iss_deflate_code_build over the histogram of all blocks' tokens + one end-of-block per block), every
block packed as deflate_twin packs it but closed by a stored block with BFINAL = 1, and framed as one gzip member with the BC
field, the block's own CRC-32 and ISIZE."""
import os
import struct
import zlib

import numpy as np

import deflate_twin as T

BGZF_HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
BGZF_MAX = 65536
CODES = "=ACMGRSVTWYHKDBN"
IUPAC = "ACMGRSVTWYHKDBN"


def base_codes(bases):
    """4-bit codes of letters (uint8 array): lower case counts as upper case, anything that is not an IUPAC letter is N (15)."""
    lut = np.full(256, 15, dtype=np.uint8)
    for c in IUPAC:
        lut[ord(c)] = lut[ord(c.lower())] = CODES.index(c)
    return lut[np.asarray(bases, dtype=np.uint8)]


def record(name, flag, bases, quals):
    """One alignment record without reference, CIGAR or tags; name: bytes, bases / quals: uint8 [RL]."""
    RL = len(bases)
    codes = np.concatenate([base_codes(bases), np.zeros(RL & 1, dtype=np.uint8)])
    seq = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes()
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, 0, flag, RL, -1, -1, 0) + name + b"\0" + seq + \
        np.asarray(quals, dtype=np.uint8).tobytes()
    return struct.pack("<i", len(body)) + body


def records(items, cpu, r1_base, r1_qual, r2_base, r2_qual):
    """The record bytes of one emit call: items (record id, first pair number, first row, pairs) over rows [n, RL]."""
    out = []
    for rid, first_i, row, n in items:
        rid = T.as_bytes(rid)
        for k in range(n):
            name = b"%s_%d_%d" % (rid, first_i + k, cpu)
            out.append(record(name, 77, r1_base[row + k], r1_qual[row + k]))
            out.append(record(name, 141, r2_base[row + k], r2_qual[row + k]))
    return b"".join(out)


def record_length(rid, i, cpu, RL):
    return 36 + len(T.as_bytes(rid)) + len(str(cpu)) + 3 + (RL + 1) // 2 + RL + len(str(i))


def record_distance(items, RL, cpu):
    """iss_ubam_emit_batch's rule for the distance of the previous-record matches: the record length of the first item with the
    strictly largest pair count, at its LAST pair number; 0 (runs only) with ISS_DEFLATE_RUNS_ONLY set."""
    most, rec = 0, 0
    for rid, first_i, _, n in items:
        if n > most:
            most, rec = n, record_length(rid, first_i + n - 1, cpu, RL)
    if rec < 8 or rec > 32768 or os.environ.get("ISS_DEFLATE_RUNS_ONLY") is not None:
        return 0
    return rec


def layout(native, text, dist):
    """{"bytes": the BGZF stream of `text`, "members": each member's bytes, "hist", "hdr_bits"}; no bytes for an empty text."""
    text = bytes(text)
    blocks = [text[at:at + T.BLOCK] for at in range(0, len(text), T.BLOCK)]
    if not blocks:
        return {"bytes": b"", "members": [], "hist": None, "hdr_bits": 0}
    tables = [T.token_table(b, dist) for b in blocks]  # (every block tokenized as a text of its own: the member rule)
    hist = sum(T.histogram(t, 1).astype(np.int64) for t in tables).astype(np.uint32)
    entry, hdr_bits, hdr, dcode = T.code_tables(native, hist, dist)
    code, length = (entry & 0xffff).astype(np.uint64), (entry >> 16).astype(np.int64)
    hdr_fields = [(int(hdr[w]) & ((1 << min(32, hdr_bits - 32 * w)) - 1), min(32, hdr_bits - 32 * w)) for w in range((hdr_bits + 31) // 32)]
    members = []
    for block, table in zip(blocks, tables):
        sym, kind, xbits, xval, _at = table.T
        value = code[sym] | (xval.astype(np.uint64) << length[sym].astype(np.uint64))
        width = length[sym] + xbits
        rec = np.uint64(1 | (int(dcode[2]) << 1))
        value = np.where(kind == 2, value | (rec << width.astype(np.uint64)), value)
        width = width + np.where(kind == 1, 1, np.where(kind == 2, 1 + int(dcode[1]), 0))
        # header, tokens, end of block, then the stored block that ends the member: BFINAL 1, BTYPE 00
        v = np.concatenate([[f[0] for f in hdr_fields], value, [int(code[256])], [1]]).astype(np.uint64)
        w = np.concatenate([[f[1] for f in hdr_fields], width, [int(length[256])], [3]]).astype(np.int64)
        packed, _n = T._pack(v, w)
        packed += b"\x00\x00\xff\xff"  # LEN 0, NLEN 0xffff
        size = len(BGZF_HEAD) + 2 + len(packed) + 8
        assert size <= BGZF_MAX, size
        members.append(BGZF_HEAD + struct.pack("<H", size - 1) + packed + struct.pack("<II", zlib.crc32(block) & 0xffffffff, len(block)))
    return {"bytes": b"".join(members), "members": members, "hist": hist, "hdr_bits": hdr_bits}


def members(native, text, dist):
    return layout(native, text, dist)["bytes"]


def split_members(stream):
    """The members of a BGZF stream by their BSIZE chain."""
    out, pos = [], 0
    while pos < len(stream):
        assert stream[pos:pos + 16] == BGZF_HEAD, "no BGZF member at byte %d" % pos
        size = struct.unpack_from("<H", stream, pos + 16)[0] + 1
        out.append(stream[pos:pos + size])
        pos += size
    assert pos == len(stream)
    return out


def inflate_member(m):
    """A member's text, inflated ALONE with an empty window; CRC-32 and ISIZE checked."""
    d = zlib.decompressobj(-15)
    raw = d.decompress(m[18:-8]) + d.flush()
    assert d.eof and d.unused_data == b""
    crc, isize = struct.unpack("<II", m[-8:])
    assert len(raw) == isize and (zlib.crc32(raw) & 0xffffffff) == crc
    return raw


def parse_records(data):
    """Field by field, independent of records(): [(name, flag, bases as upper-case letters, phreds uint8)]; every constant field asserted."""
    out, pos = [], 0
    while pos < len(data):
        (size,) = struct.unpack_from("<i", data, pos)
        ref, p, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", data, pos + 4)
        assert (ref, p, mapq, bin_, n_cigar, nref, npos, tlen) == (-1, -1, 0, 4680, 0, -1, -1, 0)
        at = pos + 36
        name = data[at:at + l_name - 1]
        assert data[at + l_name - 1] == 0
        at += l_name
        packed = np.frombuffer(data, dtype=np.uint8, count=(l_seq + 1) // 2, offset=at)
        nib = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)
        assert l_seq % 2 == 0 or nib[-1] == 0
        bases = np.frombuffer(CODES.encode(), dtype=np.uint8)[nib[:l_seq]].tobytes()
        at += (l_seq + 1) // 2
        qual = np.frombuffer(data, dtype=np.uint8, count=l_seq, offset=at).copy()
        at += l_seq
        assert at == pos + 4 + size, "tags or a wrong block_size"
        out.append((name, flag, bases, qual))
        pos = at
    return out
