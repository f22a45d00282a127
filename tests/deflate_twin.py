"""A host twin of the device's gzip members (iss_deflate.hip.h, fastq_emit_core, the writer thread of iss_host_fastq_pipe.hip.h).

The tokenizer and the one-block packer are plain Python, pinned by zlib in tests/test_host_cpu.py.  member() extends them to a
whole member: the bytes the library has to write for a text, bit for bit -- one code for the member (iss_deflate_code_build over
the histogram of ALL its tokens + one end-of-block per block), every 32 768-byte block with the dynamic-block header, its
tokens, the end-of-block code and an empty stored block, then the final empty block, CRC-32 and ISIZE.  The cases it is run
over are in tests/deflate_cases.py."""
import ctypes as C
import os
import zlib

import numpy as np

BLOCK = 32768   # DEFLATE_BLOCK: text bytes per block
CHUNK = 32      # DEFLATE_CHUNK: bytes a lane tokenizes on its own
SYMS = 273      # DEFLATE_SYMS
HEAD = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])  # the writer thread's member header: no flags, no time, no XFL, OS unknown


def _length_code(n):
    """RFC 1951 3.2.5 for match lengths 3..32: (symbol, extra bits, their value)"""
    if n <= 10:
        return 254 + n, 0, 0
    k = n - 11
    if k < 8:
        return 265 + (k >> 1), 1, k & 1
    return 269 + ((k - 8) >> 2), 2, (k - 8) & 3


def _tokens(data, dist=0):
    """The device's tokens (iss_deflate.hip.h, deflate_tokens): 32-byte chunks; at every position the run (the byte
    repeats its predecessor) and the previous record (the same bytes `dist` earlier) are tried, the longer one wins
    with >= 3 (run) / >= 4 (previous record) bytes inside the chunk, else a literal.
    -> (symbol, kind 0 literal / 1 run / 2 previous record, extra bits of the length code, their value)"""
    out = []
    for at in range(0, len(data), 32):
        chunk = data[at:at + 32]
        has_src = bool(dist) and at >= dist
        i = 0
        while i < len(chunk):
            c = chunk[i]
            r1 = rd = 0
            while i + r1 < len(chunk) and at + i + r1 > 0 and data[at + i + r1] == data[at + i + r1 - 1]:
                r1 += 1
            while has_src and i + rd < len(chunk) and chunk[i + rd] == data[at + i + rd - dist]:
                rd += 1
            if r1 >= 3 and r1 >= rd:
                out.append((*_length_code(r1)[:1], 1, *_length_code(r1)[1:]))
                i += r1
            elif rd >= 4:
                out.append((*_length_code(rd)[:1], 2, *_length_code(rd)[1:]))
                i += rd
            else:
                out.append((c, 0, 0, 0))
                i += 1
    return out


def _deflate_block(native, data, hist=None, dist=0):
    """One DEFLATE block of `data` built on the CPU with the code tables of iss_deflate_code_build (what the device
    kernels pack): header bits, the tokens' codes, end of block, then an empty stored block and a final empty block."""
    toks = _tokens(data, dist)
    if hist is None:
        hist = np.bincount(np.array([t[0] for t in toks] + [256], dtype=np.int64), minlength=273).astype(np.uint32)
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    assert hist.size == 273
    entry = np.zeros(273, dtype=np.uint32)
    hdr = np.zeros(64, dtype=np.uint32)
    dcode = np.zeros(3, dtype=np.uint32)
    nbits = C.c_uint32(0)
    assert native.lib().iss_deflate_code_build(hist.ctypes.data, dist, entry.ctypes.data, C.byref(nbits), hdr.ctypes.data,
                                               dcode.ctypes.data) == 0
    lens = (entry >> 16).astype(np.int64)
    assert lens.min() >= 1 and lens.max() <= 15
    assert sum(2.0 ** -int(x) for x in lens) == 1.0  # complete code (inflate rejects anything else)
    acc = 0
    for w in range((nbits.value + 31) // 32):
        acc |= int(hdr[w]) << (32 * w)
    acc &= (1 << nbits.value) - 1
    n = nbits.value
    for sym, kind, xbits, xval in toks:
        acc |= (int(entry[sym]) & 0xffff) << n
        n += int(lens[sym])
        acc |= xval << n           # extra bits of the length code
        n += xbits
        if kind == 1:              # distance 1: the bit 0
            n += 1
        elif kind == 2:            # the record distance: the bit 1, then its extra bits
            acc |= (1 | (int(dcode[2]) << 1)) << n
            n += 1 + int(dcode[1])
    acc |= (int(entry[256]) & 0xffff) << n
    n += int(lens[256])
    n += 3                      # empty stored block: BFINAL 0, BTYPE 00
    n = (n + 7) // 8 * 8
    acc |= 0xffff0000 << n      # LEN 0, NLEN 0xffff
    n += 32
    return acc.to_bytes(n // 8, "little") + b"\x03\x00", lens


# ------------------------------------------------------------------ one member
def token_table(text, dist):
    """_tokens(text, dist) as an int64 [n, 5] array: symbol, kind, extra bits, their value, text offset of the token."""
    t = np.array(_tokens(text, dist), dtype=np.int64).reshape(-1, 4)
    sym, xval = t[:, 0], t[:, 3]
    size = np.where(t[:, 1] == 0, 1, np.where(sym <= 264, sym - 254, np.where(sym <= 268, 11 + 2 * (sym - 265) + xval,
                                                                             19 + 4 * (sym - 269) + xval)))
    at = np.cumsum(size) - size
    assert int(size.sum()) == len(text)
    return np.concatenate([t, at[:, None]], axis=1)


def histogram(table, n_blocks):
    """What k_deflate_hist has to count: every token's symbol, and one end-of-block per block."""
    h = np.bincount(table[:, 0], minlength=SYMS)
    h[256] += n_blocks
    return h.astype(np.uint32)


def code_tables(native, hist, dist):
    """iss_deflate_code_build: (entry [273]: bit-reversed code | length << 16, header bits, header words, distance code)."""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    assert hist.size == SYMS
    entry, hdr, dcode, nbits = np.zeros(SYMS, dtype=np.uint32), np.zeros(64, dtype=np.uint32), np.zeros(3, dtype=np.uint32), C.c_uint32(0)
    assert native.lib().iss_deflate_code_build(hist.ctypes.data, int(dist), entry.ctypes.data, C.byref(nbits), hdr.ctypes.data,
                                               dcode.ctypes.data) == 0
    return entry, int(nbits.value), hdr, dcode


def _pack(values, widths):
    """Bit fields (value, width <= 32), least significant bit first, one after the other -> (bytes, bits)."""
    values, widths = np.asarray(values, dtype=np.uint64), np.asarray(widths, dtype=np.int64)
    at = np.cumsum(widths) - widths
    total = int(widths.sum())
    bits = np.zeros((total + 7) // 8 * 8, dtype=np.uint8)
    for j in range(int(widths.max()) if len(widths) else 0):
        sel = widths > j
        bits[at[sel] + j] = (values[sel] >> np.uint64(j)) & np.uint64(1)
    return np.packbits(bits, bitorder="little").tobytes(), total


def layout(native, text, dist):
    """One gzip member of `text` as the library writes it: {"bytes", "blocks": byte offset of every block's first bit in the
    member, "hdr_bits": bits of a block's dynamic header (the code), "hist", "tokens": token_table()}."""
    text = bytes(text)
    assert text, "an emit of no records writes no member"
    n_blocks = (len(text) + BLOCK - 1) // BLOCK
    table = token_table(text, dist)
    hist = histogram(table, n_blocks)
    entry, hdr_bits, hdr, dcode = code_tables(native, hist, dist)
    code, length = (entry & 0xffff).astype(np.uint64), (entry >> 16).astype(np.int64)
    hdr_fields = [(int(hdr[w]) & ((1 << min(32, hdr_bits - 32 * w)) - 1), min(32, hdr_bits - 32 * w)) for w in range((hdr_bits + 31) // 32)]
    sym, kind, xbits, xval, at = table.T
    # a token: its code, the extra bits of a length code, then the distance code -- "0" for a run, "1" + extra bits for the record
    value = code[sym] | (xval.astype(np.uint64) << length[sym].astype(np.uint64))
    width = length[sym] + xbits
    rec = np.uint64(1 | (int(dcode[2]) << 1))
    value = np.where(kind == 2, value | (rec << width.astype(np.uint64)), value)
    width = width + np.where(kind == 1, 1, np.where(kind == 2, 1 + int(dcode[1]), 0))
    block_of = at // BLOCK
    out, starts = [HEAD], []
    size = len(HEAD)
    for b in range(n_blocks):
        mine = block_of == b
        v = np.concatenate([[f[0] for f in hdr_fields], value[mine], [int(code[256])]]).astype(np.uint64)
        w = np.concatenate([[f[1] for f in hdr_fields], width[mine], [int(length[256])]]).astype(np.int64)
        packed, n = _pack(v, w)
        packed = packed[:(n + 3 + 7) // 8]  # + the empty stored block's BFINAL 0, BTYPE 00, padded to a byte
        packed += b"\0" * ((n + 3 + 7) // 8 - len(packed)) + b"\x00\x00\xff\xff"  # LEN 0, NLEN 0xffff
        starts.append(size)
        size += len(packed)
        out.append(packed)
    out.append(b"\x03\x00" + (zlib.crc32(text) & 0xffffffff).to_bytes(4, "little") + (len(text) & 0xffffffff).to_bytes(4, "little"))
    return {"bytes": b"".join(out), "blocks": starts, "hdr_bits": hdr_bits, "hist": hist, "tokens": table}


def member(native, text, dist):
    return layout(native, text, dist)["bytes"]


def record_distance(items, RL, cpu):
    """fastq_emit_core's rule for the distance of the previous-record matches: the record length of the first item with the
    strictly largest pair count, at its LAST pair number; 0 (runs only) outside 8 .. 32 768 or with ISS_DEFLATE_RUNS_ONLY set.
    items: (record id, first pair number, first row, pairs)."""
    most, rec = 0, 0
    for rid, first_i, _, n in items:
        if n > most:
            most = n
            rec = len(as_bytes(rid)) + len(str(cpu)) + 2 * RL + 10 + len(str(first_i + n - 1))
    if rec < 8 or rec > 32768 or os.environ.get("ISS_DEFLATE_RUNS_ONLY") is not None:
        return 0
    return rec


def as_bytes(rid):
    return rid if isinstance(rid, bytes) else str(rid).encode()


def describe_difference(got, members):
    """Where the file's bytes leave the twin's: the member, its first block that differs, header bits (the code) or tokens."""
    want = b"".join(m["bytes"] for m in members)
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    head = "%d bytes against the twin's %d, first difference at byte %d" % (len(got), len(want), k)
    base = 0
    for j, m in enumerate(members):
        if k < base + len(m["bytes"]) or j + 1 == len(members):
            r = k - base
            where = "the member header"
            for b, start in enumerate(m["blocks"]):
                if r >= start:
                    part = "header bits (the code)" if (r - start) * 8 < m["hdr_bits"] else "the tokens behind the header, bit %d of the block" % ((r - start) * 8)
                    where = "block %d of %d (starts at byte %d of the member): %s" % (b, len(m["blocks"]), start, part)
            if r >= len(m["bytes"]) - 10:
                where = "the final empty block, CRC-32, ISIZE"
            head += "; member %d of %d, %s" % (j, len(members), where)
            break
        base += len(m["bytes"])
    return "%s: %r against %r" % (head, got[k:k + 40], want[k:k + 40])


def huffman_depths(counts):
    """Leaf depths of a plain Huffman tree (heapq, no length limit) over the symbols with a count."""
    import heapq

    heap = [(int(c), s, (s,)) for s, c in enumerate(counts) if c]
    depth = dict((s, 0) for _, s, _ in heap)
    heapq.heapify(heap)
    tick = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def smoothed(hist):
    """The counts deflate_build_code builds the tree from: every symbol keeps a code (count + 1, at least 2^-15 of the total)."""
    h = np.asarray(hist, dtype=np.int64)
    return np.maximum(h + 1, int(h.sum()) >> 15)


def limited_lengths(counts, maxbits=15, lanes=1):
    """deflate_lengths in plain Python: the unlimited tree's depths clamped to maxbits, then the Kraft sum repaired one step at a
    time -- lengthen the longest code below maxbits (the rarer symbol first), then shorten the longest code that fits (the more
    frequent first), ties to the lower symbol.  lanes > 1 is NOT the device's rule: it is what `lanes` lanes would give if the
    merge of their proposals broke ties by lane order (symbol s is lane s % lanes's) instead of by symbol -- the mistake the
    deep_code case has to be able to see.  -> (lengths, steps taken as (symbol, candidates tied with it))"""
    counts = [int(c) for c in counts]
    depth = huffman_depths(counts)
    length = [min(depth.get(s, 0), maxbits) for s in range(len(counts))]
    one = 1 << maxbits
    kraft = sum(one >> x for x in length if x)
    steps = []

    def pick(lengthen, room):
        ok = [s for s, x in enumerate(length) if ((x and x < maxbits) if lengthen else (x > 1 and (one >> x) <= room))]
        if not ok:
            return -1
        order = lambda s: (-length[s], counts[s] if lengthen else -counts[s])  # noqa: E731
        tied = [s for s in ok if order(s) == min(map(order, ok))]
        steps.append((min(tied, key=lambda s: (s % lanes, s)), len(tied)))
        return steps[-1][0]

    while kraft > one:
        s = pick(True, 0)
        kraft -= one >> (length[s] + 1)
        length[s] += 1
    while kraft < one:
        s = pick(False, one - kraft)
        if s < 0:
            break
        kraft += one >> length[s]
        length[s] -= 1
    return length, steps
