"""The case table of the BGZF inflate (insilicoseq_amd/csrc/iss_inflate_core.h on the host, k_bgzf_inflate on the device): members
that must inflate to stated bytes and members that must end with a stated ISS_BGZF_* status.  A small bit writer builds the DEFLATE
streams by hand where the stream's shape is the point; zlib builds the ordinary ones.  tests/test_inflate_host.py holds every case
against zlib itself, so a case zlib disagrees with is a wrong case."""
import heapq
import os
import random
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OK, BAD_BTYPE, STORED_LEN, BAD_CODE, BAD_SYMBOL, BAD_DISTANCE, IN_OVERRUN, OUT_OVERRUN, SHORT, TRAILING, CRC = range(11)
STATUS_NAMES = ("OK", "BAD_BTYPE", "STORED_LEN", "BAD_CODE", "BAD_SYMBOL", "BAD_DISTANCE", "IN_OVERRUN", "OUT_OVERRUN", "SHORT", "TRAILING",
                "CRC")
OWN_CHECK = (CRC, SHORT, OUT_OVERRUN, TRAILING)  # zlib's raw inflate takes these streams: the footer or the payload's end says no

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
EOF_BLOCK = bytes(bytearray([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x1b, 0x00, 0x03, 0x00,
                             0, 0, 0, 0, 0, 0, 0, 0]))  # insilicoseq_amd.bgzf.EOF_BLOCK


class BitWriter(object):
    """DEFLATE's bit order: values from the low bit up, Huffman codes from their first bit."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def pos(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        self.bits(int(format(code, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2); no check of the set."""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


def huffman_lengths(weights):
    """Code lengths of a Huffman code for the weights (all positive)."""
    heap = [(w, i, (i,)) for i, w in enumerate(weights)]
    heapq.heapify(heap)
    lens = [0] * len(weights)
    tick = len(weights)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return lens


def length_symbol(length):
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length and (s == 28 or length < LEN_BASE[s] + (1 << LEN_EXTRA[s])):
            if s == 28 and length != 258:
                continue
            return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]
    raise ValueError(length)


def distance_symbol(dist):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= dist:
            return s, DIST_EXTRA[s], dist - DIST_BASE[s]
    raise ValueError(dist)


def put_tokens(w, tokens, lit_lens, dist_lens):
    """Tokens: ("lit", byte) | ("match", length, distance) | ("end",) | ("lsym", symbol) | ("dsym", symbol) | ("bits", value, n)."""
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if t[0] == "lit":
            w.code(*lc[t[1]])
        elif t[0] == "match":
            s, eb, ev = length_symbol(t[1])
            w.code(*lc[s])
            w.bits(ev, eb)
            d, deb, dev = distance_symbol(t[2])
            w.code(*dc[d])
            w.bits(dev, deb)
        elif t[0] == "end":
            w.code(*lc[256])
        elif t[0] == "lsym":
            w.code(*lc[t[1]])
        elif t[0] == "dsym":
            w.code(*dc[t[1]])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        else:
            raise ValueError(t)


def fixed_block(w, tokens, final=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(w, data, final=True, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen))
    w.raw(data)


DEFAULT_CL = [4] * 13 + [5] * 6  # a complete code over all 19 code-length symbols


def plain_ops(lens):
    return [("len", l) for l in lens]


def dynamic_header(w, hlit, hdist, ops, cl_lens=DEFAULT_CL, final=True, hclen=19):
    """ops: ("len", 0 .. 15) | ("rep16", 3 .. 6) | ("z17", 3 .. 10) | ("z18", 11 .. 138), written with the code-length code cl_lens."""
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    cc = canonical(cl_lens)
    for op in ops:
        if op[0] == "len":
            w.code(*cc[op[1]])
        elif op[0] == "rep16":
            w.code(*cc[16])
            w.bits(op[1] - 3, 2)
        elif op[0] == "z17":
            w.code(*cc[17])
            w.bits(op[1] - 3, 3)
        elif op[0] == "z18":
            w.code(*cc[18])
            w.bits(op[1] - 11, 7)
        else:
            raise ValueError(op)


def dynamic_block(w, lit_lens, dist_lens, tokens, final=True, ops=None, cl_lens=DEFAULT_CL):
    dynamic_header(w, len(lit_lens), len(dist_lens), ops if ops is not None else plain_ops(list(lit_lens) + list(dist_lens)), cl_lens, final)
    put_tokens(w, tokens, lit_lens, dist_lens)


def play(tokens, before=b""):
    """The bytes the literal and match tokens produce behind `before`."""
    out = bytearray(before)
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            n, start = t[1], len(out) - t[2]
            assert start >= 0, t
            if t[2] >= n:
                out += out[start:start + n]
            else:  # the period t[2] repeats
                out += (bytes(out[start:]) * (n // t[2] + 1))[:n]
    return bytes(out[len(before):])


def lits(data):
    return [("lit", c) for c in bytearray(data)]


def member(payload, data=None, crc=None, isize=None, before=b"", after=b""):
    """A BGZF member around the DEFLATE payload; before / after: foreign subfields around BC."""
    crc = (zlib.crc32(data) & 0xFFFFFFFF) if crc is None else crc
    isize = len(data) if isize is None else isize
    xlen = len(before) + 6 + len(after)
    size = 12 + xlen + len(payload) + 8
    assert size <= 65536, size
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + before + b"BC\x02\x00" + struct.pack("<H", size - 1) + after +
            payload + struct.pack("<II", crc, isize))


def split_member(m):
    """(payload, crc, isize) of one member."""
    xlen = struct.unpack_from("<H", m, 10)[0]
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    return m[12 + xlen:len(m) - 8], crc, isize


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(flush_mode) + c.compress(data[flush_at:]) + c.flush()


def fastq_text(n_bytes, seed=1):
    rnd = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n_bytes:
        seq = "".join(rnd.choice("ACGT") for _ in range(100))
        qual = "".join(chr(33 + min(40, max(2, int(rnd.gauss(34, 6))))) for _ in range(100))
        out += ("@read_%d/1\n%s\n+\n%s\n" % (i, seq, qual)).encode()
        i += 1
    return bytes(out[:n_bytes])


def bam_bytes(n_bytes):
    import bam_synth

    recs = bam_synth.records(7, n_pairs=200)
    raw = bam_synth.header_bytes() + b"".join(bam_synth.encode_record(r) for r in recs)
    assert len(raw) >= n_bytes
    return raw[:n_bytes]


def noise(n, seed):
    rnd = random.Random(seed)
    return bytes(bytearray(rnd.getrandbits(8) for _ in range(n)))


def _good():
    cases = []

    def add(name, m, data):
        cases.append({"name": name, "member": m, "data": bytes(data), "status": OK})

    add("eof_block", EOF_BLOCK, b"")
    w = BitWriter()
    stored_block(w, b"")
    add("empty_stored", member(w.done(), b""), b"")
    add("isize_1", member(deflate(b"A"), b"A"), b"A")
    text = fastq_text(65536)
    for n in (65280, 65535, 65536):
        add("isize_%d" % n, member(deflate(text[:n]), text[:n]), text[:n])
    big = noise(65505, 2)
    w = BitWriter()
    stored_block(w, big)
    m = member(w.done(), big)
    assert len(m) == 65536
    add("stored_bsize_65535", m, big)
    parts = [noise(1, 3), noise(20000, 4), b"", noise(16384, 5), noise(257, 6)]
    w = BitWriter()
    for i, p in enumerate(parts):
        stored_block(w, p, final=i == len(parts) - 1)
    add("stored_blocks", member(w.done(), b"".join(parts)), b"".join(parts))
    add("fixed_zlib", member(deflate(text[:3000], 6, zlib.Z_FIXED), text[:3000]), text[:3000])
    add("dynamic_fastq_l6", member(deflate(text[:65280], 6), text[:65280]), text[:65280])
    bam = bam_bytes(65280)
    for level in (6, 1, 9):
        add("dynamic_bam_l%d" % level, member(deflate(bam, level), bam), bam)
    add("dynamic_fastq_l1", member(deflate(text[:40000], 1), text[:40000]), text[:40000])
    add("dynamic_fastq_l9", member(deflate(text[:40000], 9), text[:40000]), text[:40000])
    add("sync_flush", member(deflate(text[:30000], 6, flush_at=12345), text[:30000]), text[:30000])
    add("full_flush", member(deflate(text[:30000], 6, flush_at=20001, flush_mode=zlib.Z_FULL_FLUSH), text[:30000]), text[:30000])

    def fixed(name, tokens, before=b""):
        w = BitWriter()
        if before:
            stored_block(w, before, final=False)
        fixed_block(w, tokens + [("end",)])
        data = before + play(tokens, before)
        add(name, member(w.done(), data), data)

    seed = lits(b"The quick brown fox jumps over the lazy dog, twice. " * 6)  # 312 bytes
    for length in (3, 10, 11, 257, 258):
        fixed("match_len_%d" % length, seed + [("match", length, 300), ("lit", 33)])
    for dist in (1, 2, 3, 4, 63, 64, 65, 256, 257):
        for length in sorted(set(l for l in (3, dist - 1, dist, dist + 1, 258) if l >= 3)):
            fixed("dist_%d_len_%d" % (dist, length), seed + [("match", length, dist), ("lit", 10), ("match", 3, 5)])
    far = noise(32768, 8)
    for dist in (32767, 32768):
        for length in (3, 258):
            fixed("dist_%d_len_%d" % (dist, length), [("match", length, dist), ("lit", 7), ("match", length, dist)], before=far)
    fixed("dist_equals_produced", lits(b"hello") + [("match", 5, 5), ("match", 20, 10)])
    # far matches that straddle the pieces in which the ring leaves for the output, the window full
    fixed("ring_wrap", [("match", 258, 32768)] * 100 + [("match", 258, 32767)] * 20 + [("match", 100, 1)], before=far)

    # a 15-bit literal code (Huffman lengths of Fibonacci weights) and a 7-bit code-length code
    fib = [1, 1]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    hl = huffman_lengths(fib)
    assert max(hl) == 15 and kraft(hl) == 1.0
    syms = list(range(97, 112)) + [256]  # 'a' .. 'o' and the end of the block: the rarest two carry 15 bits
    lit_lens = [0] * 257
    for s, l in zip(syms, [hl[0], hl[2]] + hl[3:] + [hl[1]]):
        lit_lens[s] = l
    assert lit_lens[256] == 15 and sorted(l for l in lit_lens if l) == sorted(hl)
    cl7 = [0] * 19
    cl7[0] = 1
    for s, l in zip([18, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [4] * 5 + [5] * 3 + [6] * 4 + [7] * 4):
        cl7[s] = l
    assert kraft(cl7) == 1.0 and max(cl7) == 7
    ops = [("z18", 97)] + [("len", lit_lens[s]) for s in range(97, 112)] + [("z18", 138)] + [("len", 0)] * 6 + [("len", 15), ("len", 0)]
    rnd = random.Random(9)
    data = bytes(bytearray(rnd.choice(range(97, 112)) for _ in range(500))) + b"abcdefghijklmno"
    w = BitWriter()
    dynamic_block(w, lit_lens, [0], lits(data) + [("end",)], ops=ops, cl_lens=cl7)
    add("lit_code_15_bits_cl_7_bits", member(w.done(), data), data)

    # no distance code in use: HLIT = 257, HDIST = 1, the one distance length zero
    ll = [0] * 257
    ll[ord("x")] = ll[ord("y")] = 2
    ll[ord("z")] = 2
    ll[256] = 2
    w = BitWriter()
    dynamic_block(w, ll, [0], lits(b"xyzzyx" * 20) + [("end",)])
    add("no_distance_code_hlit_257_hdist_1", member(w.done(), b"xyzzyx" * 20), b"xyzzyx" * 20)

    # exactly one distance code, of length 1 (an incomplete code zlib takes)
    ll = [0] * 258
    ll[ord("x")] = 2
    ll[ord("y")] = 2
    ll[256] = 2
    ll[257] = 2
    tokens = lits(b"xy") + [("match", 3, 1), ("lit", ord("x")), ("match", 3, 1)]
    w = BitWriter()
    dynamic_block(w, ll, [1], tokens + [("end",)])
    add("one_distance_code_of_length_1", member(w.done(), play(tokens)), play(tokens))

    # a repeat-16 that runs from the literal lengths into the distance lengths
    ll = [0] * 257
    ll[97] = 1
    ll[253] = ll[254] = ll[255] = ll[256] = 3
    ops = [("z18", 97), ("len", 1), ("z18", 138), ("z18", 17), ("len", 3), ("rep16", 6), ("rep16", 5)]
    tokens = lits(b"a\xfda\xfe\xffaaa")
    w = BitWriter()
    dynamic_block(w, ll, [3] * 8, tokens + [("end",)], ops=ops)
    add("repeat_16_across_the_boundary", member(w.done(), play(tokens)), play(tokens))

    # HLIT = 286 and HDIST = 30
    ll = [8] * 226 + [9] * 60
    dl = [4, 4] + [5] * 28
    assert kraft(ll) == 1.0 and kraft(dl) == 1.0
    tokens = lits(noise(700, 10)) + [("match", 258, 700), ("match", 31, 1), ("match", 4, 513), ("lit", 0), ("lit", 255)]
    w = BitWriter()
    dynamic_block(w, ll, dl, tokens + [("end",)])
    add("hlit_286_hdist_30", member(w.done(), play(tokens)), play(tokens))

    # XLEN > 6: a foreign subfield before BC and one after it
    pay = deflate(text[:5000])
    add("foreign_subfields", member(pay, text[:5000], before=b"XY\x03\x00abc", after=b"ZZ\x00\x00Q1\x02\x00\x01\x02"), text[:5000])
    return cases


def _bad():
    cases = []
    text = fastq_text(4000, 3)

    def add(name, status, payload, data=b"", crc=None, isize=None):
        cases.append({"name": name, "member": member(payload, data, crc, isize), "data": None, "status": status})

    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    add("btype_3", BAD_BTYPE, w.done() + b"\0\0\0\0")
    w = BitWriter()
    stored_block(w, b"abcdef", nlen=(6 ^ 0xFFFF) ^ 0x0100)
    add("stored_len_nlen", STORED_LEN, w.done(), b"abcdef")

    def header_only(name, status, lit_lens, dist_lens, ops=None, tail=b"\0" * 8):
        w = BitWriter()
        dynamic_header(w, len(lit_lens), len(dist_lens), ops if ops is not None else plain_ops(list(lit_lens) + list(dist_lens)))
        add(name, status, w.done() + tail, b"")

    ll = [0] * 257
    ll[97] = ll[98] = ll[256] = 1
    header_only("oversubscribed_literal_code", BAD_CODE, ll, [1, 1])
    ll = [0] * 257
    ll[97] = ll[256] = 2
    header_only("incomplete_literal_code", BAD_CODE, ll, [1, 1])
    ll = [0] * 257
    ll[97] = ll[98] = 1
    header_only("no_end_of_block_code", BAD_CODE, ll, [1, 1])
    header_only("repeat_16_first", BAD_CODE, [0] * 257, [1, 1], ops=[("rep16", 3)] + [("len", 1)] * 10)
    ll = [0] * 257
    ll[97] = ll[256] = 1
    header_only("repeat_past_the_lengths", BAD_CODE, ll, [1, 1],
                ops=[("z18", 97), ("len", 1), ("z18", 138), ("z18", 20), ("len", 1), ("len", 1), ("rep16", 3)])
    w = BitWriter()
    fixed_block(w, lits(b"ab") + [("lsym", 286), ("end",)])
    add("literal_symbol_286", BAD_SYMBOL, w.done(), b"ab")
    w = BitWriter()
    fixed_block(w, lits(b"ab") + [("lsym", 257), ("dsym", 30), ("end",)])
    add("distance_symbol_30", BAD_SYMBOL, w.done(), b"ab")
    w = BitWriter()
    fixed_block(w, lits(b"abc") + [("match", 3, 4), ("end",)])
    add("distance_past_the_start", BAD_DISTANCE, w.done(), b"abc")

    # the payload cut inside a symbol, inside a length's extra bits, inside the dynamic header
    w = BitWriter()
    fixed_block(w, lits(b"\xff\xff") + [("end",)])
    add("cut_mid_symbol", IN_OVERRUN, w.done()[:1], b"")
    w = BitWriter()
    fixed_block(w, lits(b"\xff"))
    s, eb, ev = length_symbol(250)
    w.code(*canonical(FIXED_LIT)[s])
    sym_end = w.pos()
    w.bits(ev, eb)
    extra_end = w.pos()
    cut = (sym_end + 7) // 8
    assert sym_end <= 8 * cut < extra_end
    add("cut_mid_extra_bits", IN_OVERRUN, w.done()[:cut], b"", isize=251)  # (room for the literal and the match)
    dyn = deflate(text)
    assert (bytearray(dyn)[0] >> 1) & 3 == 2
    add("cut_in_dynamic_header", IN_OVERRUN, dyn[:6], b"")

    add("one_byte_more_than_isize", OUT_OVERRUN, dyn, text, isize=len(text) - 1)
    add("one_byte_fewer_than_isize", SHORT, dyn, text, isize=len(text) + 1)
    add("crc_bit_flipped", CRC, dyn, text, crc=(zlib.crc32(text) & 0xFFFFFFFF) ^ 0x00400000)
    w = BitWriter()
    flipped = bytearray(text)
    flipped[1234] ^= 0x10
    stored_block(w, bytes(flipped))
    add("data_bit_flipped", CRC, w.done(), text)
    add("trailing_bytes", TRAILING, dyn + b"\0\0", text)

    # A code-length code without a code (every HCLEN length 0).  zlib reads each of the HLIT + HDIST lengths as 0 from one bit: the
    # stream misses its end-of-block code if it holds those 258 bits and runs out of input if it does not (found by
    # tests/inflate_gen.py's damaged streams: the decoder said BAD_CODE for both).
    w = BitWriter()
    dynamic_header(w, 257, 1, [], cl_lens=[0] * 19, hclen=4)
    add("no_code_length_code", BAD_CODE, w.done() + b"\0" * 33)
    add("no_code_length_code_input_ends", IN_OVERRUN, w.done() + b"\0\0")
    return cases


_CACHE = {}


def good_cases():
    if "good" not in _CACHE:
        _CACHE["good"] = _good()
    return _CACHE["good"]


def bad_cases():
    if "bad" not in _CACHE:
        _CACHE["bad"] = _bad()
    return _CACHE["bad"]


def all_cases():
    """Good and bad interleaved."""
    g, b = good_cases(), bad_cases()
    out = []
    for i in range(max(len(g), len(b))):
        out += g[i:i + 1] + b[i:i + 1]
    return out
