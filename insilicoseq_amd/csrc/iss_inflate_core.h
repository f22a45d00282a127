// iss_inflate_core.h -- the DEFLATE decoder of one BGZF member (RFC 1951, RFC 1952, SAM/BAM specification 4.1): ONE implementation of
// every decision that makes a stream good or bad, for the host (plain C++17: tests/inflate_core_main.cpp runs it under the address
// sanitizer with buffers of exact size) and for the device (k_bgzf_inflate of iss_inflate.hip.h), in the manner of deflate_lengths.
//
// inflate_member is written for `nl` cooperating lanes that all walk the same control flow: every lane holds the same bit reader,
// the same position and the same status in its own registers, so every branch below is uniform.  What is shared lives in `Work`
// (LDS on the device): the 32 KiB ring of the bytes produced last, the code tables, the per-slice CRCs.  The serial pieces of a
// table's construction are lane 0's; table fills, match copies, stored copies, the ring's way to the output and the CRC slices are
// strided over the lanes; sync() stands between a piece that writes `Work` and a piece that reads it.  With nl == 1 and an empty
// sync the same text is the host's sequential decoder: the accept/reject result and the bytes do not depend on nl.
//
// Bounds.  The bit reader never touches a byte at or behind pay + pay_len; the output is written only by flush(), only inside
// [out, out + isize) -- a symbol that would produce byte isize ends the member with ST_OUT_OVERRUN before anything of it is
// stored.  Every loop consumes input bits or produces bytes in each round, or ends with a status: DESIGN.md section 27.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ISS_INF_HD __host__ __device__ __forceinline__
#else
#define ISS_INF_HD inline
#endif

namespace iss_inf {

// include/iss_mi355x.h: ISS_BGZF_*
enum : int {
    ST_OK = 0, ST_BAD_BTYPE = 1, ST_STORED_LEN = 2, ST_BAD_CODE = 3, ST_BAD_SYMBOL = 4, ST_BAD_DISTANCE = 5, ST_IN_OVERRUN = 6,
    ST_OUT_OVERRUN = 7, ST_SHORT = 8, ST_TRAILING = 9, ST_CRC = 10
};

constexpr uint32_t RING = 32768;              // the window: a distance reaches at most this far back
constexpr uint32_t RING_MASK = RING - 1;
constexpr uint32_t FLUSH = 16384;             // the ring goes to the output in pieces of this size, so the bytes a piece holds
                                              // and the window behind the position never overlap what is written next
constexpr uint32_t SLICE = 256;               // bytes per CRC slice of a piece
constexpr uint32_t N_SLICES = FLUSH / SLICE;
constexpr int FAST_L = 10, FAST_D = 8, FAST_C = 7;  // index bits of the direct tables: literal/length, distance, code lengths
constexpr int N_OPS = 17;                     // CRC operators "append 2^k zero bytes", k = 0 .. 16
constexpr int KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2;

// What one member's decoder shares between its lanes.
struct Work {
    uint8_t ring[RING];
    uint16_t fast_l[1 << FAST_L];  // (symbol << 4) | code length, 0: no code of at most FAST_L bits starts like this
    uint16_t fast_d[1 << FAST_D];  // (the code-length code uses the distance code's tables until the distance code is built)
    uint16_t sym_l[288], sym_d[32];  // symbols by (code length, symbol)
    uint16_t cnt_l[16], cnt_d[16];   // symbols per code length
    uint16_t offs[16];
    uint8_t lens[320];               // HLIT + HDIST code lengths (at most 286 + 30; the fixed code: 288 + 32)
    uint8_t cl_lens[32];             // the 19 lengths of the code-length code
    uint32_t crcs[N_SLICES];
};

// ---------------------------------------------------------------- CRC-32 (reflected 0xEDB88320)
ISS_INF_HD uint32_t crc_byte_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
ISS_INF_HD uint32_t gf2_apply(const uint32_t *mat, uint32_t vec) {
    uint32_t sum = 0;
    for (int i = 0; vec; vec >>= 1, ++i)
        if (vec & 1u) sum ^= mat[i];
    return sum;
}
// the register after n more zero bytes: ops[k] appends 2^k of them (n < 2^17)
ISS_INF_HD uint32_t crc_shift(const uint32_t *ops, uint32_t crc, uint32_t n) {
    for (int k = 0; n; n >>= 1, ++k)
        if (n & 1u) crc = gf2_apply(ops + 32 * k, crc);
    return crc;
}
// host: the byte table [256] and the operators [N_OPS][32] (zlib's crc32_combine construction)
inline void crc_tables(uint32_t *tab, uint32_t *ops) {
    for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_byte_entry(i);
    uint32_t a[32], b[32];
    a[0] = 0xEDB88320u;  // one zero bit
    for (int n = 1; n < 32; ++n) a[n] = 1u << (n - 1);
    for (int s = 0; s < 3; ++s) {  // two, four, eight bits
        for (int n = 0; n < 32; ++n) b[n] = gf2_apply(a, a[n]);
        memcpy(a, b, sizeof a);
    }
    for (int k = 0; k < N_OPS; ++k) {
        memcpy(ops + 32 * k, a, sizeof a);
        for (int n = 0; n < 32; ++n) b[n] = gf2_apply(a, a[n]);
        memcpy(a, b, sizeof a);
    }
}

// ---------------------------------------------------------------- the bit reader, bounded by the member's payload
struct Bits {
    const uint8_t *pay;
    uint32_t len;  // bytes of the payload
    uint32_t ip;   // the next byte to load
    uint64_t bb;   // bits not yet consumed, the next one lowest
    uint32_t bc;   // how many
    uint32_t pre;  // the four bytes at ip, loaded ahead (valid when ip + 4 <= len): a refill does not wait for memory
};

// the four bytes at ip if the payload holds them
ISS_INF_HD void preload(Bits &b) {
    b.pre = 0;
    if (b.ip + 4 <= b.len) memcpy(&b.pre, b.pay + b.ip, 4);
}

// At least 33 bits afterwards, or all the payload has left.
ISS_INF_HD void refill(Bits &b) {
    while (b.bc <= 32 && b.ip < b.len) {
        if (b.ip + 4 <= b.len) {
            b.bb |= (uint64_t)b.pre << b.bc;
            b.bc += 32;
            b.ip += 4;
            preload(b);
        } else {
            b.bb |= (uint64_t)b.pay[b.ip] << b.bc;
            b.bc += 8;
            b.ip += 1;
        }
    }
}
ISS_INF_HD void drop(Bits &b, uint32_t n) {
    b.bb >>= n;
    b.bc -= n;
}
// n <= 16 bits into *v; false: the payload ends first
ISS_INF_HD bool take(Bits &b, uint32_t n, uint32_t *v) {
    refill(b);
    if (n > b.bc) return false;
    *v = (uint32_t)b.bb & ((1u << n) - 1u);
    drop(b, n);
    return true;
}

ISS_INF_HD uint32_t bit_reverse(uint32_t v, int n) {  // the low n <= 16 bits, mirrored
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}

// ---------------------------------------------------------------- canonical codes
// The tables of the code whose n lengths are lens[]: cnt / sym (sorted symbols) for every code, `fast` for the codes of at most fb
// bits.  zlib's acceptance rule (inflate_table): an over-subscribed set is bad; an incomplete one is bad unless it is a literal/length
// or distance code whose longest code has one bit; no code at all is accepted (every use of it is then bad).
template <class Sync>
ISS_INF_HD int build_code(const uint8_t *lens, int n, uint16_t *cnt, uint16_t *sym, uint16_t *fast, int fb, int kind, uint16_t *offs,
                          int lane, int nl, Sync sync) {
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) cnt[l] = 0;
        for (int s = 0; s < n; ++s) cnt[lens[s]] = (uint16_t)(cnt[lens[s]] + 1);
    }
    for (int j = lane; j < (1 << fb); j += nl) fast[j] = 0;
    sync();
    int left = 1, longest = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return ST_BAD_CODE;
        if (cnt[l]) longest = l;
    }
    if (longest == 0) return ST_OK;
    if (left > 0 && (kind == KIND_CODES || longest != 1)) return ST_BAD_CODE;
    if (lane == 0) {
        offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
        for (int s = 0; s < n; ++s)
            if (lens[s]) {
                sym[offs[lens[s]]] = (uint16_t)s;
                offs[lens[s]] = (uint16_t)(offs[lens[s]] + 1);
            }
    }
    sync();
    uint32_t code = 0, idx = 0;
    for (int l = 1; l <= fb; ++l) {
        const uint32_t c = cnt[l];
        for (uint32_t k = 0; k < c; ++k) {
            const uint32_t rev = bit_reverse(code + k, l);
            const uint16_t e = (uint16_t)((sym[idx + k] << 4) | l);
            for (int j = lane; j < (1 << (fb - l)); j += nl) fast[rev | ((uint32_t)j << l)] = e;
        }
        idx += c;
        code = (code + c) << 1;
    }
    sync();
    return ST_OK;
}

// One symbol of the code into *s.  The bits behind the payload's end read as zeros; a code that needs one of them is ST_IN_OVERRUN.
ISS_INF_HD int decode_symbol(Bits &b, const uint16_t *cnt, const uint16_t *sym, const uint16_t *fast, int fb, uint32_t *s) {
    refill(b);
    const uint32_t v = (uint32_t)b.bb;
    const uint32_t e = fast[v & ((1u << fb) - 1u)];
    uint32_t l = e & 15u;
    *s = e >> 4;
    if (!e) {
        uint32_t code = 0, first = 0, idx = 0;
        for (l = 1; l < 16; ++l) {
            code |= (v >> (l - 1)) & 1u;
            const uint32_t c = cnt[l];
            if (code < first + c) {
                *s = sym[idx + (code - first)];
                break;
            }
            idx += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (l == 16) return b.bc >= 15 ? ST_BAD_CODE : ST_IN_OVERRUN;
    }
    if (l > b.bc) return ST_IN_OVERRUN;
    drop(b, l);
    return ST_OK;
}

// ---------------------------------------------------------------- the ring's way out
struct Out {
    uint8_t *out;      // the member's output, isize bytes
    uint32_t isize;
    uint32_t pos;      // bytes produced
    uint32_t flushed;  // of them stored to out and in the CRC: a multiple of FLUSH until the member's end
    uint32_t crc;      // the CRC register over out[0 .. flushed)
};

// The n <= FLUSH bytes behind `flushed` (flushed + n <= pos <= isize): into the CRC register, and to the output as aligned words
// with single bytes at both ends.  (flushed is a multiple of FLUSH, so the piece does not wrap in the ring.)
template <class Sync>
ISS_INF_HD void flush(Work &W, Out &o, uint32_t n, const uint32_t *crc_tab, const uint32_t *ops, int lane, int nl, Sync sync) {
    sync();
    const uint8_t *src = W.ring + (o.flushed & RING_MASK);
    const uint32_t n_slices = (n + SLICE - 1) / SLICE;
    for (uint32_t s = (uint32_t)lane; s < n_slices; s += (uint32_t)nl) {
        const uint32_t end = (s + 1) * SLICE < n ? (s + 1) * SLICE : n;
        uint32_t c = 0;
        for (uint32_t i = s * SLICE; i < end; ++i) c = crc_tab[(c ^ src[i]) & 0xffu] ^ (c >> 8);
        W.crcs[s] = c;
    }
    sync();
    for (uint32_t s = 0; s < n_slices; ++s) {
        const uint32_t m = (s + 1) * SLICE < n ? SLICE : n - s * SLICE;
        o.crc = crc_shift(ops, o.crc, m) ^ W.crcs[s];
    }
    uint8_t *dst = o.out + o.flushed;
    uint32_t head = (uint32_t)(-(intptr_t)dst) & 3u;
    if (head > n) head = n;
    const uint32_t words = (n - head) / 4;
    const uint32_t tail = head + 4 * words;
    for (uint32_t i = (uint32_t)lane; i < head; i += (uint32_t)nl) dst[i] = src[i];
    for (uint32_t w = (uint32_t)lane; w < words; w += (uint32_t)nl) {
        const uint8_t *p = src + head + 4 * w;
        const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = v;
    }
    for (uint32_t i = tail + (uint32_t)lane; i < n; i += (uint32_t)nl) dst[i] = src[i];
    o.flushed += n;
    sync();
}

// the code-length code's order (RFC 1951 3.2.7), five bits each
ISS_INF_HD uint32_t cl_order(int i) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// ---------------------------------------------------------------- one member
// pay[0 .. pay_len): the member's DEFLATE payload; out[0 .. isize): where its bytes go; crc_expect: the footer's CRC-32.
// Returns ST_*; *crc_got is the CRC-32 of the bytes stored (of all of them when the status is OK, TRAILING or CRC).
template <class Sync>
ISS_INF_HD int inflate_member(const uint8_t *pay, uint32_t pay_len, uint8_t *out, uint32_t isize, uint32_t crc_expect, Work &W,
                              const uint32_t *crc_tab, const uint32_t *ops, int lane, int nl, Sync sync, uint32_t *crc_got) {
    Bits b{pay, pay_len, 0, 0, 0, 0};
    preload(b);
    Out o{out, isize, 0, 0, 0xFFFFFFFFu};
    *crc_got = 0;
    uint32_t last = 0;
    while (!last) {
        uint32_t btype = 0, v = 0;
        if (!take(b, 1, &last) || !take(b, 2, &btype)) return ST_IN_OVERRUN;
        if (btype == 3) return ST_BAD_BTYPE;
        if (btype == 0) {
            drop(b, b.bc & 7u);
            uint32_t len = 0, nlen = 0;
            if (!take(b, 16, &len) || !take(b, 16, &nlen)) return ST_IN_OVERRUN;
            if ((len ^ 0xFFFFu) != nlen) return ST_STORED_LEN;
            b.ip -= b.bc / 8;  // (whole bytes: the reader stands on a byte boundary)
            b.bb = 0;
            b.bc = 0;
            if (len > b.len - b.ip) return ST_IN_OVERRUN;
            if (len > o.isize - o.pos) return ST_OUT_OVERRUN;
            while (len) {
                const uint32_t room = FLUSH - (o.pos - o.flushed);
                const uint32_t m = len < room ? len : room;
                for (uint32_t i = (uint32_t)lane; i < m; i += (uint32_t)nl) W.ring[(o.pos + i) & RING_MASK] = b.pay[b.ip + i];
                b.ip += m;
                o.pos += m;
                len -= m;
                if (o.pos - o.flushed >= FLUSH) flush(W, o, FLUSH, crc_tab, ops, lane, nl, sync);
            }
            preload(b);
            continue;
        }
        int nl_codes, nd_codes;
        if (btype == 1) {
            nl_codes = 288;
            nd_codes = 32;
            for (int s = lane; s < 320; s += nl) W.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
            sync();
        } else {
            uint32_t hlit = 0, hdist = 0, hclen = 0;
            if (!take(b, 5, &hlit) || !take(b, 5, &hdist) || !take(b, 4, &hclen)) return ST_IN_OVERRUN;
            nl_codes = (int)hlit + 257;
            nd_codes = (int)hdist + 1;
            if (nl_codes > 286 || nd_codes > 30) return ST_BAD_CODE;
            for (int i = lane; i < 19; i += nl) W.cl_lens[i] = 0;
            sync();
            uint32_t any = 0;
            for (int i = 0; i < (int)hclen + 4; ++i) {
                if (!take(b, 3, &v)) return ST_IN_OVERRUN;
                any |= v;
                if (lane == 0) W.cl_lens[cl_order(i)] = (uint8_t)v;
            }
            sync();
            // A code-length code without a code: zlib reads every length as 0 from one bit each and then misses the end-of-block
            // code -- or runs out of input before it has read them all.
            if (!any) return (uint64_t)b.bc + 8ull * (b.len - b.ip) >= (uint64_t)(nl_codes + nd_codes) ? ST_BAD_CODE : ST_IN_OVERRUN;
            if (int st = build_code(W.cl_lens, 19, W.cnt_d, W.sym_d, W.fast_d, FAST_C, KIND_CODES, W.offs, lane, nl, sync)) return st;
            const int total = nl_codes + nd_codes;
            int idx = 0;
            uint32_t prev = 0;
            while (idx < total) {
                uint32_t s = 0;
                if (int st = decode_symbol(b, W.cnt_d, W.sym_d, W.fast_d, FAST_C, &s)) return st;
                if (s < 16) {
                    if (lane == 0) W.lens[idx] = (uint8_t)s;
                    prev = s;
                    ++idx;
                    continue;
                }
                uint32_t rep = 0;
                if (s == 16) {
                    if (idx == 0) return ST_BAD_CODE;
                    if (!take(b, 2, &rep)) return ST_IN_OVERRUN;
                    rep += 3;
                } else if (s == 17) {
                    if (!take(b, 3, &rep)) return ST_IN_OVERRUN;
                    rep += 3;
                    prev = 0;
                } else {
                    if (!take(b, 7, &rep)) return ST_IN_OVERRUN;
                    rep += 11;
                    prev = 0;
                }
                if (idx + (int)rep > total) return ST_BAD_CODE;
                for (int i = lane; i < (int)rep; i += nl) W.lens[idx + i] = (uint8_t)prev;
                idx += (int)rep;
            }
            sync();
            if (W.lens[256] == 0) return ST_BAD_CODE;
        }
        if (int st = build_code(W.lens, nl_codes, W.cnt_l, W.sym_l, W.fast_l, FAST_L, KIND_LENS, W.offs, lane, nl, sync)) return st;
        if (int st = build_code(W.lens + nl_codes, nd_codes, W.cnt_d, W.sym_d, W.fast_d, FAST_D, KIND_DISTS, W.offs, lane, nl, sync)) return st;
        for (;;) {
            uint32_t s = 0;
            if (int st = decode_symbol(b, W.cnt_l, W.sym_l, W.fast_l, FAST_L, &s)) return st;
            if (s < 256) {
                if (o.pos >= o.isize) return ST_OUT_OVERRUN;
                if (lane == 0) W.ring[o.pos & RING_MASK] = (uint8_t)s;
                o.pos += 1;
            } else if (s == 256) {
                break;
            } else {
                if (s >= 286) return ST_BAD_SYMBOL;
                uint32_t eb = 0, base = 3 + (s - 257);
                if (s == 285) {
                    base = 258;
                } else if (s >= 265) {
                    eb = (s - 261) >> 2;
                    base = 3 + ((4 + ((s - 261) & 3u)) << eb);
                }
                if (!take(b, eb, &v)) return ST_IN_OVERRUN;
                const uint32_t len = base + v;
                uint32_t d = 0;
                if (int st = decode_symbol(b, W.cnt_d, W.sym_d, W.fast_d, FAST_D, &d)) return st;
                if (d >= 30) return ST_BAD_SYMBOL;
                uint32_t deb = 0, dbase = 1 + d;
                if (d >= 4) {
                    deb = (d >> 1) - 1;
                    dbase = 1 + ((2 + (d & 1u)) << deb);
                }
                if (!take(b, deb, &v)) return ST_IN_OVERRUN;
                const uint32_t dist = dbase + v;
                if (dist > o.pos) return ST_BAD_DISTANCE;
                if (len > o.isize - o.pos) return ST_OUT_OVERRUN;
                // The bytes [pos - dist, pos) repeat with period dist.  Every round reads before pos and writes at or behind it; a
                // round's loads stand before its stores, because with dist + len > RING a slot read late in the copy is one the
                // copy itself writes later -- never earlier.
                const uint32_t from = o.pos - dist;
                sync();
                for (uint32_t i0 = 0; i0 < len; i0 += (uint32_t)nl) {
                    const uint32_t i = i0 + (uint32_t)lane;
                    uint8_t byte = 0;
                    if (i < len) byte = W.ring[(from + (dist >= len ? i : i % dist)) & RING_MASK];
                    sync();
                    if (i < len) W.ring[(o.pos + i) & RING_MASK] = byte;
                }
                sync();
                o.pos += len;
            }
            if (o.pos - o.flushed >= FLUSH) flush(W, o, FLUSH, crc_tab, ops, lane, nl, sync);
        }
    }
    if (o.pos > o.flushed) flush(W, o, o.pos - o.flushed, crc_tab, ops, lane, nl, sync);
    *crc_got = o.crc ^ 0xFFFFFFFFu;
    if (o.pos != o.isize) return ST_SHORT;
    if (*crc_got != crc_expect) return ST_CRC;
    if (b.len - b.ip + b.bc / 8 > 0) return ST_TRAILING;
    return ST_OK;
}

struct NoSync {
    ISS_INF_HD void operator()() const {}
};

}  // namespace iss_inf
