"""A host twin of the BGZF stage of the text pipes (iss_bgzf_text.hip.h): the exact bytes the device has to
append for a text and its line offsets.

Plain Python on top of tests/deflate_twin.py (the length code, the bit packer, the length-limited Huffman lengths), nothing of
the library: members(text, offsets) cuts the text into 32 768-byte blocks, gives every 32-byte chunk the length of the line in
front of the chunk's line as its copy distance (chunk_distances: the contract's three exceptions), tokenizes the chunks by
deflate_tokens' rule under the member rule (no predecessor byte at a block's start), builds ONE code for the call -- the
literal/length code over the smoothed histogram, the distance code over the 30 distance codes as they were counted -- and packs
every block as one BGZF member: header, dynamic block, an empty final stored block, CRC-32, ISIZE."""
import bisect
import struct
import zlib

import numpy as np

from deflate_twin import BLOCK, CHUNK, SYMS, _length_code, _pack, limited_lengths, smoothed

DSYMS = 30
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])  # ... BSIZE - 1 follows
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def line_offsets(text):
    """The byte offset of every line of ``text`` (lines end with a line feed; the formatters' offsets are these)."""
    out, at = [], 0
    while at < len(text):
        out.append(at)
        nl = text.find(b"\n", at)
        at = len(text) if nl < 0 else nl + 1
    return out


def dist_code(dist):
    """RFC 1951 3.2.5: (distance symbol, extra bits, their value)"""
    if dist <= 4:
        return dist - 1, 0, 0
    d = dist - 1
    hb = d.bit_length() - 1
    return 2 * hb + ((d >> (hb - 1)) & 1), hb - 1, d & ((1 << (hb - 1)) - 1)


def chunk_distances(n_bytes, offsets, runs_only=False):
    """The copy distance of every 32-byte chunk (0: no candidate): the byte length of the line in front of the line that holds
    the chunk's first byte.  None in the text's first line, past 32 768, or when the source would start before the chunk's
    block.  ``offsets`` may hold empty lines (equal offsets): they are no lines."""
    starts = sorted(set(int(o) for o in offsets if o < n_bytes))
    out = []
    for pos in range(0, n_bytes, CHUNK):
        d = 0
        k = bisect.bisect_right(starts, pos) - 1
        if not runs_only and k >= 1:
            length = starts[k] - starts[k - 1]
            if length <= BLOCK and pos % BLOCK >= length:
                d = length
        out.append(d)
    return out


def tokens(text, dists):
    """deflate_tokens over every chunk, at the chunk's own distance, under the member rule -> rows (symbol, kind 0 literal / 1 run /
    2 copy, extra bits of the length code, their value, distance symbol, its extra bits, their value, text offset)."""
    out = []
    for c, at in enumerate(range(0, len(text), CHUNK)):
        chunk = text[at:at + CHUNK]
        dist = dists[c]
        dsym, debits, deval = dist_code(dist) if dist else (0, 0, 0)
        first = at % BLOCK == 0  # no predecessor byte inside the member
        i = 0
        while i < len(chunk):
            r1 = rd = 0
            while i + r1 < len(chunk) and not (first and i + r1 == 0) and text[at + i + r1] == text[at + i + r1 - 1]:
                r1 += 1
            while dist and i + rd < len(chunk) and chunk[i + rd] == text[at + i + rd - dist]:
                rd += 1
            if r1 >= 3 and r1 >= rd:
                sym, xb, xv = _length_code(r1)
                out.append((sym, 1, xb, xv, 0, 0, 0, at + i))
                i += r1
            elif rd >= 4:
                sym, xb, xv = _length_code(rd)
                out.append((sym, 2, xb, xv, dsym, debits, deval, at + i))
                i += rd
            else:
                out.append((chunk[i], 0, 0, 0, 0, 0, 0, at + i))
                i += 1
    return np.array(out, dtype=np.int64).reshape(-1, 8)


def histogram(table, n_blocks):
    """[273 + 30]: token symbols (+ one end of block per block), then the distance codes of the matches (a run: code 0)."""
    h = np.zeros(SYMS + DSYMS, dtype=np.int64)
    np.add.at(h, table[:, 0], 1)
    h[256] += n_blocks
    np.add.at(h, SYMS + table[table[:, 1] > 0, 4], 1)
    return h.astype(np.uint32)


def lengths(counts, maxbits):
    """deflate_lengths: no symbol in use -> no code; one -> one bit, paired with symbol 1 (or 0) so that the code is complete."""
    counts = [int(c) for c in counts]
    used = [s for s, c in enumerate(counts) if c]
    if not used:
        return [0] * len(counts)
    if len(used) == 1:
        out = [0] * len(counts)
        out[used[0]] = 1
        out[1 if used[0] == 0 else 0] = 1
        return out
    return limited_lengths(counts, maxbits)[0]


def canonical(lens):
    """RFC 1951 3.2.2, bit-reversed for a least-significant-bit-first stream"""
    count = [0] * 16
    for x in lens:
        count[x] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    out = []
    for x in lens:
        v = 0
        if x:
            v = int(format(nxt[x], "0%db" % x)[::-1], 2)
            nxt[x] += 1
        out.append(v)
    return out


def build_code(hist):
    """bgzf_text_build_code: {"len", "code" [273], "dlen", "dcode" [30], "hdr": [(value, width)] of the dynamic-block header}."""
    hist = np.asarray(hist, dtype=np.int64)
    assert hist.size == SYMS + DSYMS
    lens = lengths(smoothed(hist[:SYMS]), 15)
    dlens = lengths(hist[SYMS:], 15)
    hdist = max([d + 1 for d in range(DSYMS) if dlens[d]] + [1])
    every = lens + dlens[:hdist]
    sym = []  # the code lengths run-length coded: the value, then "repeat the previous 3..6 times" (16) for a non-zero value
    i = 0
    while i < len(every):
        r = 1
        while i + r < len(every) and every[i + r] == every[i]:
            r += 1
        sym.append((every[i], 0))
        rem = r - 1
        if every[i]:
            while rem >= 3:
                t = min(rem, 6)
                sym.append((16, t - 3))
                rem -= t
        sym += [(every[i], 0)] * rem
        i += r
    ccnt = [0] * 19
    for s, _ in sym:
        ccnt[s] += 1
    clen = lengths(ccnt, 7)
    ccode = canonical(clen)
    hclen = 19
    while hclen > 4 and clen[ORDER[hclen - 1]] == 0:
        hclen -= 1
    hdr = [(0, 1), (2, 2), (SYMS - 257, 5), (hdist - 1, 5), (hclen - 4, 4)] + [(clen[ORDER[k]], 3) for k in range(hclen)]
    for s, x in sym:
        hdr.append((ccode[s], clen[s]))
        if s == 16:
            hdr.append((x, 2))
    return {"len": lens, "code": canonical(lens), "dlen": dlens, "dcode": canonical(dlens), "hdr": hdr, "hdist": hdist}


def layout(text, offsets=None, runs_only=False):
    """The BGZF members of ``text`` as the device appends them for one call: {"bytes", "members": [bytes], "hist", "code",
    "tokens", "dists"}.  An empty text: no member."""
    text = bytes(text)
    if not text:
        return {"bytes": b"", "members": [], "hist": None, "code": None, "tokens": None, "dists": []}
    offsets = line_offsets(text) if offsets is None else offsets
    n_blocks = (len(text) + BLOCK - 1) // BLOCK
    dists = chunk_distances(len(text), offsets, runs_only)
    table = tokens(text, dists)
    hist = histogram(table, n_blocks)
    code = build_code(hist)
    clen, ccode = np.array(code["len"], dtype=np.int64), np.array(code["code"], dtype=np.uint64)
    dlen, dcode = np.array(code["dlen"], dtype=np.int64), np.array(code["dcode"], dtype=np.uint64)
    sym, kind, xbits, xval, dsym, debits, deval, at = table.T
    # a token: its code and the extra bits of a length code; a match: then the distance code and its extra bits
    v1 = ccode[sym] | (xval.astype(np.uint64) << clen[sym].astype(np.uint64))
    w1 = clen[sym] + xbits
    v2 = dcode[dsym] | (deval.astype(np.uint64) << dlen[dsym].astype(np.uint64))
    w2 = np.where(kind > 0, dlen[dsym] + debits, 0)
    assert (dlen[dsym][kind > 0] > 0).all(), "a match whose distance code has no length"
    values = np.stack([v1, v2], axis=1).reshape(-1)
    widths = np.stack([w1, w2], axis=1).reshape(-1)
    block_of = np.repeat(at // BLOCK, 2)
    out = []
    for b in range(n_blocks):
        mine = (block_of == b) & (widths > 0)
        v = np.concatenate([[f[0] for f in code["hdr"]], values[mine], [code["code"][256]]]).astype(np.uint64)
        w = np.concatenate([[f[1] for f in code["hdr"]], widths[mine], [code["len"][256]]]).astype(np.int64)
        keep = w > 0
        packed, n = _pack(v[keep], w[keep])
        # the member's last block: BFINAL 1, BTYPE 00, padded to a byte, LEN 0, NLEN 0xffff
        bits = np.unpackbits(np.frombuffer(packed, dtype=np.uint8), bitorder="little")[:n]
        bits = np.concatenate([bits, [1, 0, 0]]).astype(np.uint8)
        body = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
        data = text[b * BLOCK:(b + 1) * BLOCK]
        size = len(HEAD) + 2 + len(body) + 8
        assert size <= 65536
        out.append(HEAD + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))
    return {"bytes": b"".join(out), "members": out, "hist": hist, "code": code, "tokens": table, "dists": dists}


def members(text, offsets=None, runs_only=False):
    return layout(text, offsets, runs_only)["bytes"]


def size(text, offsets=None, runs_only=False):
    return len(members(text, offsets, runs_only))
