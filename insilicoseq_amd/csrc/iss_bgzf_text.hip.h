// iss_bgzf_text.hip.h -- line-oriented text (the --origins BEDPE, the --store_mutations VCF rows) as BGZF members built on the
// device (`generate --bgzip`).
//
// The chunk size, the block size, the member's framing, the CRC tree and the bit packer are those of k_bgzf_* (iss_ubam.hip.h).
// What differs is where a chunk's copy distance comes from, and the distance alphabet.  The records of FASTQ and BAM have ONE
// length per call; lines of text have not, so here the distance of a chunk is the byte length of the line in front of the line
// that holds the chunk's first byte -- known per line from the offsets the formatters computed (k_bgzt_dist writes it per chunk).
// With it `{id}`, the leading digits of the coordinates and the fixed columns copy from the line above.  Distances differ from
// chunk to chunk, so the code has a real distance alphabet: a histogram over the 30 distance codes, lengths from deflate_lengths,
// both tables in the dynamic header, extra distance bits per RFC 1951.
//
// The text's size is known on the device only (the scan's grand total), so every kernel reads it there; grids are sized for the
// host's bound of it, and the workgroups of blocks the text does not have leave a member size of 0 and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iss_ubam.hip.h"  // BGZF_FRAME, BGZF_MAX; iss_deflate.hip.h

namespace iss {

constexpr int BGZT_DSYMS = 30;      // DEFLATE's distance codes
constexpr int BGZT_HDR_WORDS = 80;  // 14 + 19 * 3 bits, then at most 7 bits for each of the 273 + 30 code lengths
constexpr int BGZT_HIST = DEFLATE_SYMS + BGZT_DSYMS;  // the histogram: literal/length counts, then the distance codes'
static_assert(14 + 57 + (DEFLATE_SYMS + BGZT_DSYMS) * 7 <= BGZT_HDR_WORDS * 32, "the dynamic header fits its words");
static_assert(DEFLATE_BLOCK * 15 / 8 + BGZT_HDR_WORDS * 4 + 8 + BGZF_FRAME <= BGZF_MAX, "a BGZF member of one block fits BSIZE");

struct BgzfTextCode {
    uint32_t entry[DEFLATE_SYMS];     // bit-reversed code | length << 16
    uint32_t dentry[BGZT_DSYMS];      // the same for the distance codes (length 0: not in use)
    uint32_t hdr_bits;                // BFINAL, BTYPE, HLIT, HDIST, HCLEN, both code tables
    uint32_t hdr[BGZT_HDR_WORDS];
    uint32_t crc_shift[8][32];        // DeflateCode's operators
};

struct BgzfTextWork {  // the builder's scratch: LDS on the device
    DeflateWork w;
    uint32_t dcnt[BGZT_DSYMS];
    uint8_t dlen[32];
    uint16_t dcode[BGZT_DSYMS];
    uint32_t dentry[BGZT_DSYMS];
    uint32_t hdr[BGZT_HDR_WORDS];
    uint32_t hdr_bits;
    uint32_t bl_count[16], next_code[16];  // of bgzf_text_codes
};

// deflate_codes with its two small tables in the work area (private arrays indexed by a code length live in scratch memory)
__host__ __device__ inline void bgzf_text_codes(const uint8_t *len, int n, uint16_t *code, uint32_t *bl_count, uint32_t *next_code) {
    for (int b = 0; b < 16; ++b) bl_count[b] = next_code[b] = 0;
    for (int s = 0; s < n; ++s) ++bl_count[len[s]];
    bl_count[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + bl_count[b - 1]) << 1; next_code[b] = c; }
    for (int s = 0; s < n; ++s) {
        uint32_t v = 0;
        if (len[s]) {
            const uint32_t x = next_code[len[s]]++;
            for (int b = 0; b < len[s]; ++b) v |= ((x >> b) & 1u) << (len[s] - 1 - b);
        }
        code[s] = (uint16_t)v;
    }
}

// hist[0 .. 272]: token counts as deflate_build_code takes them ([256] = number of blocks); hist[273 + d]: matches whose distance
// has code d (a run is a match at distance 1: code 0).  The literal/length code is deflate_build_code's (every symbol keeps a
// code); the distance code is built from the counts as they are -- a code that no chunk uses gets no length, HDIST is the highest
// code in use + 1 (one code of length 0 when there is no match at all, RFC 1951 3.2.7).  Called by all nl lanes; deterministic
// and independent of nl (every choice of deflate_lengths is made on a total order).
template <typename Sync>
__host__ __device__ inline void bgzf_text_build_code(const uint32_t *hist, BgzfTextWork *ws, int lane, int nl, Sync sync) {
    DeflateWork *w = &ws->w;
    uint32_t *cnt = w->cnt;
    uint64_t total = 0;
    for (int s = 0; s < DEFLATE_SYMS; ++s) total += hist[s];
    const uint32_t floor_cnt = (uint32_t)(total >> 15);
    for (int s = lane; s < DEFLATE_SYMS; s += nl) cnt[s] = hist[s] + 1u > floor_cnt ? hist[s] + 1u : floor_cnt;
    for (int d = lane; d < BGZT_DSYMS; d += nl) ws->dcnt[d] = hist[DEFLATE_SYMS + d];
    sync();
    uint8_t *len = w->len;
    deflate_lengths(cnt, DEFLATE_SYMS, 15, len, w, lane, nl, sync);
    sync();
    deflate_lengths(ws->dcnt, BGZT_DSYMS, 15, ws->dlen, w, lane, nl, sync);
    sync();
    if (lane == 0) {
        bgzf_text_codes(len, DEFLATE_SYMS, w->code, ws->bl_count, ws->next_code);
        for (int s = 0; s < DEFLATE_SYMS; ++s) w->entry[s] = (uint32_t)w->code[s] | ((uint32_t)len[s] << 16);
        bgzf_text_codes(ws->dlen, BGZT_DSYMS, ws->dcode, ws->bl_count, ws->next_code);
        int hdist = 1;
        for (int d = 0; d < BGZT_DSYMS; ++d) {
            ws->dentry[d] = (uint32_t)ws->dcode[d] | ((uint32_t)ws->dlen[d] << 16);
            if (ws->dlen[d]) hdist = d + 1;
        }
        // ---- header: the literal/length code lengths, then the distance code lengths, run-length coded together (3.2.7)
        const int n_all = DEFLATE_SYMS + hdist;
        for (int d = 0; d < hdist; ++d) len[DEFLATE_SYMS + d] = ws->dlen[d];
        uint8_t *sym = w->sym, *extra = w->extra;
        int ns = 0;
        for (int i = 0; i < n_all;) {
            int r = 1;
            while (i + r < n_all && len[i + r] == len[i]) ++r;
            sym[ns] = len[i]; extra[ns] = 0; ++ns;  // the value itself
            int rem = r - 1;
            if (len[i] != 0)
                while (rem >= 3) { const int t = rem > 6 ? 6 : rem; sym[ns] = 16; extra[ns] = (uint8_t)(t - 3); ++ns; rem -= t; }
            for (; rem > 0; --rem) { sym[ns] = len[i]; extra[ns] = 0; ++ns; }
            i += r;
        }
        w->ns = (uint32_t)ns;
        for (int i = 0; i < 19; ++i) w->ccnt[i] = 0;
        for (int i = 0; i < ns; ++i) ++w->ccnt[sym[i]];
    }
    sync();
    deflate_lengths(w->ccnt, 19, 7, w->clen, w, lane, nl, sync);
    sync();
    if (lane == 0) {
        const uint8_t *clen = w->clen, *sym = w->sym, *extra = w->extra;
        uint16_t *ccode = w->ccode;
        bgzf_text_codes(clen, 19, ccode, ws->bl_count, ws->next_code);
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && clen[order[hclen - 1]] == 0) --hclen;
        uint32_t hdist = 1;
        for (int d = 0; d < BGZT_DSYMS; ++d) if (ws->dlen[d]) hdist = (uint32_t)d + 1u;
        for (int i = 0; i < BGZT_HDR_WORDS; ++i) ws->hdr[i] = 0;
        BitSink bs{ws->hdr, 0, 0};
        bs.put(0, 1);  // BFINAL = 0 (the member is closed by an empty final block)
        bs.put(2, 2);  // BTYPE = 10: dynamic Huffman codes
        bs.put(DEFLATE_SYMS - 257, 5);  // HLIT
        bs.put(hdist - 1u, 5);          // HDIST
        bs.put((uint32_t)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) bs.put(clen[order[i]], 3);
        const int ns = (int)w->ns;
        for (int i = 0; i < ns; ++i) {
            bs.put(ccode[sym[i]], clen[sym[i]]);
            if (sym[i] == 16) bs.put(extra[i], 2);
        }
        bs.finish();
        ws->hdr_bits = bs.n;
    }
    sync();
}

__host__ __device__ inline void bgzf_text_store_code(const BgzfTextWork *ws, BgzfTextCode *out, int lane, int n_lanes) {
    for (int s = lane; s < DEFLATE_SYMS; s += n_lanes) out->entry[s] = ws->w.entry[s];
    for (int d = lane; d < BGZT_DSYMS; d += n_lanes) out->dentry[d] = ws->dentry[d];
    for (int i = lane; i < BGZT_HDR_WORDS; i += n_lanes) out->hdr[i] = ws->hdr[i];
    if (lane == 0) out->hdr_bits = ws->hdr_bits;
}

// ---------------------------------------------------------------- kernels
struct BgzfTextArgs {
    const uint8_t *text;        // 16-byte aligned, with room behind the text (deflate_source reads whole words)
    const uint64_t *n_bytes;    // device: bytes of the text
    uint64_t text_cap;          // the host's bound of it: the grids, dist, block_* and out are sized for it
    const uint64_t *off;        // [n_lines] byte offset of every line, ascending; a line may be empty (two equal offsets)
    uint64_t n_lines;
    uint32_t *dist;             // [ceil(text_cap / 32)] copy distance of every chunk, 0: none
    uint32_t *hist;             // [BGZT_HIST]
    BgzfTextCode *code;
    uint32_t *block_bytes;      // [n_blocks] member sizes (0: the text has no such block)
    uint32_t *block_crc;        // [n_blocks] CRC-32 of each block's text
    uint64_t *block_off;        // [n_blocks + 1] the members' offsets in `out`, [n_blocks] = their total (k_deflate_scan)
    uint32_t n_blocks;          // ceil(text_cap / DEFLATE_BLOCK)
    uint8_t *out;
    uint64_t out_cap;
    int32_t runs_only;          // no line copies (the yardstick of tools/bgzf_text_bench.py)
};

__device__ __forceinline__ uint64_t bgzt_bytes(const BgzfTextArgs &A) {
    const uint64_t n = *A.n_bytes;
    return n <= A.text_cap ? n : 0;  // (a text that overran its bound is the host's to report: it reads the size too)
}

// The distance of chunk c.  The line that holds byte c * 32: the last offset <= it (a line that is empty shares its offset with
// the next one, so the last such line is not empty).  The line in front: the last offset below that line's.  No candidate in the
// text's first line, past 32 768, or when the chunk's first source byte would lie before the chunk's BGZF block.
__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzt_dist(BgzfTextArgs A) {
    const uint64_t n = bgzt_bytes(A);
    const uint64_t n_chunks = (n + DEFLATE_CHUNK - 1) / DEFLATE_CHUNK;
    for (uint64_t c = (uint64_t)blockIdx.x * DEFLATE_THREADS + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * DEFLATE_THREADS) {
        const uint64_t pos = c * DEFLATE_CHUNK;
        uint32_t d = 0;
        if (!A.runs_only && A.n_lines) {
            uint64_t lo = 0, hi = A.n_lines;  // off[lo] <= pos < off[hi] (off[0] = 0)
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (A.off[mid] <= pos) lo = mid; else hi = mid;
            }
            const uint64_t start = A.off[lo];
            if (start) {
                uint64_t a = 0, b = lo;  // off[a] < start <= off[b]
                while (b - a > 1) {
                    const uint64_t mid = (a + b) >> 1;
                    if (A.off[mid] < start) a = mid; else b = mid;
                }
                const uint64_t len = start - A.off[a];
                if (len <= (uint64_t)DEFLATE_BLOCK && (pos % DEFLATE_BLOCK) >= len) d = (uint32_t)len;
            }
        }
        A.dist[c] = d;
    }
}

// chunk `c` under the member rule, at its own distance.  deflate_chunk's loads with every index of `raw` a constant (the short
// last chunk of a text is filled byte by byte under an unrolled loop), so that the chunk stays in registers.
__device__ __forceinline__ void bgzt_chunk(const BgzfTextArgs &A, uint64_t n, uint64_t c, DeflateChunk &C, uint32_t *dist) {
    const uint8_t *t = A.text;
    const uint64_t at = c * DEFLATE_CHUNK;
    const uint32_t d = A.dist[c];
    *dist = d;
    C.m = (uint32_t)min((uint64_t)DEFLATE_CHUNK, n - at);
    C.prev = at % DEFLATE_BLOCK ? (int)t[at - 1] : -1;  // (a member is inflated with an empty window)
    C.has_src = d != 0;                                 // (k_bgzt_dist: the source lies inside the block)
#pragma unroll
    for (int q = 0; q < DEFLATE_NQ; ++q) C.src[q] = d ? deflate_source(t, at + 8u * q, d) : 0;
    if (C.m == (uint32_t)DEFLATE_CHUNK) {  // (the text buffer is 16-byte aligned)
#pragma unroll
        for (int q = 0; q < DEFLATE_NQ; q += 2) {
            const uint4 v = *reinterpret_cast<const uint4 *>(t + at + 8 * q);
            C.raw[q] = (uint64_t)v.x | ((uint64_t)v.y << 32);
            C.raw[q + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
        }
    } else {
#pragma unroll
        for (int q = 0; q < DEFLATE_NQ; ++q) {
            uint64_t w = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if ((uint32_t)(8 * q + k) < C.m) w |= (uint64_t)t[at + 8 * q + k] << (8 * k);
            C.raw[q] = w;
        }
    }
}

// deflate_tokens, rule for rule (runs, copies at the chunk's distance, its priorities and minimum lengths); a literal's byte is
// picked from the four words by selects, not by an index into them, which would put the chunk into scratch memory.  The twin
// (tests/bgzf_text_twin.py) and the GPU tests hold the two to the same tokens.
template <typename F>
__device__ __forceinline__ void bgzt_tokens(const DeflateChunk &C, F &&f) {
    uint64_t diff_run = 0, diff_rec = 0;
#pragma unroll
    for (int q = 0; q < DEFLATE_NQ; ++q) {
        const uint64_t before = (C.raw[q] << 8) | (q ? C.raw[q - 1] >> 56 : (uint64_t)(C.prev & 0xff));
        diff_run |= (uint64_t)deflate_nonzero_bytes(C.raw[q] ^ before) << (8 * q);
        diff_rec |= (uint64_t)(C.has_src ? deflate_nonzero_bytes(C.raw[q] ^ C.src[q]) : 0xffu) << (8 * q);
    }
    if (C.prev < 0) diff_run |= 1u;
    diff_run |= 1ull << C.m;
    diff_rec |= 1ull << C.m;
    uint32_t i = 0;
    while (i < C.m) {
        const uint32_t r1 = (uint32_t)__builtin_ctzll(diff_run >> i), rd = (uint32_t)__builtin_ctzll(diff_rec >> i);
        const uint32_t q = i >> 3;
        const uint64_t word = q == 0 ? C.raw[0] : q == 1 ? C.raw[1] : q == 2 ? C.raw[2] : C.raw[3];
        uint32_t step = 1, sym = (uint32_t)((word >> (8 * (i & 7u))) & 0xffu), xbits = 0, xval = 0;
        int kind = 0;
        if (r1 >= 3u && r1 >= rd) { step = r1; kind = 1; }   // (a run is the cheaper match)
        else if (rd >= 4u) { step = rd; kind = 2; }          // (its distance costs bits: three bytes are not worth it)
        if (kind) deflate_length_code(step, &sym, &xbits, &xval);
        f(sym, kind, xbits, xval);
        i += step;
    }
}
static_assert(DEFLATE_NQ == 4, "bgzt_tokens selects among four words");

__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzt_hist(BgzfTextArgs A) {
    __shared__ uint32_t h[BGZT_HIST];
    for (int s = threadIdx.x; s < BGZT_HIST; s += DEFLATE_THREADS) h[s] = 0;
    __syncthreads();
    const uint64_t n = bgzt_bytes(A);
    const uint64_t n_chunks = (n + DEFLATE_CHUNK - 1) / DEFLATE_CHUNK;
    for (uint64_t c = (uint64_t)blockIdx.x * DEFLATE_THREADS + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * DEFLATE_THREADS) {
        DeflateChunk C;
        uint32_t dist, dsym = 0, debits, deval;
        bgzt_chunk(A, n, c, C, &dist);
        if (dist) deflate_dist_code(dist, &dsym, &debits, &deval);
        bgzt_tokens(C, [&](uint32_t sym, int kind, uint32_t, uint32_t) {
            atomicAdd(&h[sym], 1u);
            if (kind) atomicAdd(&h[DEFLATE_SYMS + (kind == 2 ? dsym : 0u)], 1u);
        });
    }
    __syncthreads();
    for (int s = threadIdx.x; s < BGZT_HIST; s += DEFLATE_THREADS)
        if (h[s]) atomicAdd(&A.hist[s], h[s]);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&A.hist[256], (uint32_t)((n + DEFLATE_BLOCK - 1) / DEFLATE_BLOCK));
}

// one wavefront
__global__ __launch_bounds__(64) void k_bgzt_build(BgzfTextArgs A) {
    __shared__ BgzfTextWork ws;
    __shared__ uint32_t hist[BGZT_HIST];
    for (int s = threadIdx.x; s < BGZT_HIST; s += blockDim.x) hist[s] = A.hist[s];
    __syncthreads();
    bgzf_text_build_code(hist, &ws, (int)threadIdx.x, (int)blockDim.x, DeflateBlockSync());
    bgzf_text_store_code(&ws, A.code, (int)threadIdx.x, (int)blockDim.x);
}

// bits behind a token's length code: the distance code and its extra bits
__device__ __forceinline__ uint32_t bgzt_dist_bits(const uint32_t *dlens, int kind, uint32_t dsym, uint32_t debits) {
    return kind == 1 ? dlens[0] : kind == 2 ? dlens[dsym] + debits : 0u;
}

// k_bgzf_len with the text's own size and per-chunk distances
__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzt_len(BgzfTextArgs A) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t lens[DEFLATE_SYMS];
    __shared__ uint32_t dlens[32];
    __shared__ uint32_t red[DEFLATE_THREADS];
    __shared__ uint32_t crcs[DEFLATE_THREADS];
    __shared__ uint32_t shift[8][32];
    const uint32_t b = blockIdx.x;
    const uint64_t n_bytes = bgzt_bytes(A);
    if ((uint64_t)b * DEFLATE_BLOCK >= n_bytes) {  // (uniform: the whole workgroup leaves)
        if (threadIdx.x == 0) { A.block_bytes[b] = 0; A.block_crc[b] = 0; }
        return;
    }
    const BgzfTextCode *C = A.code;
    shift[threadIdx.x >> 5][threadIdx.x & 31] = C->crc_shift[threadIdx.x >> 5][threadIdx.x & 31];
    tab[threadIdx.x] = crc_table_entry(threadIdx.x);
    for (int s = threadIdx.x; s < DEFLATE_SYMS; s += DEFLATE_THREADS) lens[s] = C->entry[s] >> 16;
    if (threadIdx.x < BGZT_DSYMS) dlens[threadIdx.x] = C->dentry[threadIdx.x] >> 16;
    __syncthreads();
    const uint64_t start = (uint64_t)b * DEFLATE_BLOCK;
    const uint32_t n = deflate_block_len(n_bytes, b);
    const uint8_t *t = A.text + start;
    uint32_t bits = 0, crc = 0;
    for (uint32_t c = threadIdx.x; c * DEFLATE_CHUNK < n; c += DEFLATE_THREADS) {
        DeflateChunk K;
        uint32_t dist, dsym = 0, debits = 0, deval;
        bgzt_chunk(A, n_bytes, start / DEFLATE_CHUNK + c, K, &dist);
        if (dist) deflate_dist_code(dist, &dsym, &debits, &deval);
        bgzt_tokens(K, [&](uint32_t sym, int kind, uint32_t xbits, uint32_t) { bits += lens[sym] + xbits + bgzt_dist_bits(dlens, kind, dsym, debits); });
    }
    const int64_t lo = (int64_t)n - (int64_t)(DEFLATE_THREADS - threadIdx.x) * 128;  // may be negative: zeros in front
    for (int64_t i = lo < 0 ? 0 : lo; i < lo + 128; ++i) {
        if (i == 0) crc = 0xffffffffu;
        crc = tab[(crc ^ t[i]) & 0xffu] ^ (crc >> 8);
    }
    red[threadIdx.x] = bits;
    crcs[threadIdx.x] = crc;
    __syncthreads();
    for (int k = 0, s = 1; s < DEFLATE_THREADS; s <<= 1, ++k) {
        if ((threadIdx.x & (2 * s - 1)) == 0) {
            red[threadIdx.x] += red[threadIdx.x + s];
            crcs[threadIdx.x] = gf2_times(shift[k], crcs[threadIdx.x]) ^ crcs[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t total = C->hdr_bits + red[0] + lens[256] + 3u;  // + end of block + header of the empty stored block
        A.block_bytes[b] = (total + 7u) / 8u + 4u + BGZF_FRAME;        // + LEN = 0, NLEN = 0xffff, + the member's frame
        A.block_crc[b] = crcs[0] ^ 0xffffffffu;
    }
}

// k_bgzf_encode with the text's own size, per-chunk distances and the distance code: a match's length code (<= 17 bits with its
// extra bits) and its distance code (<= 28) go into the lane's accumulator one after the other -- together they may pass 32 bits.
__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzt_encode(BgzfTextArgs A) {
    __shared__ uint32_t ent[DEFLATE_SYMS];
    __shared__ uint32_t dent[32];
    __shared__ uint32_t win[DEFLATE_WIN_WORDS];
    __shared__ uint32_t wsum[DEFLATE_THREADS / 64];
    const uint32_t b = blockIdx.x;
    const uint64_t n_bytes = bgzt_bytes(A);
    if ((uint64_t)b * DEFLATE_BLOCK >= n_bytes) return;  // (uniform)
    const BgzfTextCode *C = A.code;
    for (int s = threadIdx.x; s < DEFLATE_SYMS; s += DEFLATE_THREADS) ent[s] = C->entry[s];
    if (threadIdx.x < BGZT_DSYMS) dent[threadIdx.x] = C->dentry[threadIdx.x];
    for (int i = threadIdx.x; i < DEFLATE_WIN_WORDS; i += DEFLATE_THREADS) win[i] = 0;
    __syncthreads();
    const uint64_t start = (uint64_t)b * DEFLATE_BLOCK;
    const uint32_t n = deflate_block_len(n_bytes, b);
    const uint64_t off = A.block_off[b];
    const uint32_t member = A.block_bytes[b];
    if (member > BGZF_MAX || off + member > A.out_cap) return;  // (the host finds the hole: it walks the BSIZE chain)
    uint32_t *outw = reinterpret_cast<uint32_t *>(A.out + (off & ~3ull));
    uint32_t wpos = 0;                            // words of this member already written
    uint32_t fill = (uint32_t)(off & 3ull) * 8u;  // bits in the window so far (the first tile starts misaligned)
    auto or_bits = [&](uint32_t at, uint64_t v) {  // OR <= 64 bits at bit `at` of the window
        if (!v) return;
        const uint32_t w = at >> 5, sh = at & 31u;
        atomicOr(&win[w], (uint32_t)(v << sh));
        const uint64_t hi = sh ? v >> (32 - sh) : v >> 32;
        if (hi) {
            atomicOr(&win[w + 1], (uint32_t)hi);
            if (hi >> 32) atomicOr(&win[w + 2], (uint32_t)(hi >> 32));
        }
    };
    auto flush = [&](bool last) {  // whole words of the window -> out; the partial last word moves to the front
        __syncthreads();
        const uint32_t nw = last ? (fill + 31u) >> 5 : fill >> 5;
        for (uint32_t i = threadIdx.x; i < nw; i += DEFLATE_THREADS) {
            const uint32_t v = win[i];
            if ((wpos + i == 0) || (last && i == nw - 1)) { if (v) atomicOr(&outw[wpos + i], v); }
            else outw[wpos + i] = v;
        }
        __syncthreads();
        const uint32_t keep = last ? 0u : win[nw];
        __syncthreads();
        for (uint32_t i = threadIdx.x; i <= nw + 4 && i < DEFLATE_WIN_WORDS; i += DEFLATE_THREADS) win[i] = 0;
        __syncthreads();
        if (threadIdx.x == 0) win[0] = keep;
        wpos += nw;
        fill &= last ? 0u : 31u;
        __syncthreads();
    };
    // ---- member header: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C', SLEN 2, BSIZE - 1
    if (threadIdx.x == 0) {
        or_bits(fill, 0x0000000004088b1full);
        or_bits(fill + 64u, 0x000243420006ff00ull);
        or_bits(fill + 128u, (uint64_t)(member - 1u));
    }
    fill += 144u;
    // ---- block header
    for (uint32_t i = threadIdx.x; i * 32u < C->hdr_bits; i += DEFLATE_THREADS) {
        const uint32_t left = C->hdr_bits - i * 32u;
        const uint32_t v = left >= 32u ? C->hdr[i] : (C->hdr[i] & ((1u << left) - 1u));
        or_bits(fill + i * 32u, v);
    }
    fill += C->hdr_bits;
    flush(false);
    // ---- tokens
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n; base += DEFLATE_THREADS * DEFLATE_CHUNK) {
        const uint32_t at = base + threadIdx.x * DEFLATE_CHUNK;
        DeflateChunk K;
        uint32_t nb = 0, dist, dsym = 0, debits = 0, deval = 0;
        if (at < n) {
            bgzt_chunk(A, n_bytes, (start + at) / DEFLATE_CHUNK, K, &dist);
            if (dist) deflate_dist_code(dist, &dsym, &debits, &deval);
            bgzt_tokens(K, [&](uint32_t sym, int kind, uint32_t xbits, uint32_t) {
                nb += (ent[sym] >> 16) + xbits + (kind == 1 ? dent[0] >> 16 : kind == 2 ? (dent[dsym] >> 16) + debits : 0u);
            });
        }
        uint32_t x = nb;  // exclusive scan of nb over the workgroup
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t pre = x - nb, tile_bits = 0;
        for (int w = 0; w < DEFLATE_THREADS / 64; ++w) {
            if (w < wave) pre += wsum[w];
            tile_bits += wsum[w];
        }
        if (at < n) {
            uint32_t pos = fill + pre, have = 0;
            uint64_t acc = 0;  // bits not yet in the window (< 32 of them between pushes)
            auto push = [&](uint32_t v, uint32_t l) {  // l <= 28
                acc |= (uint64_t)v << have;
                have += l;
                if (have >= 32u) { or_bits(pos, acc & 0xffffffffull); pos += 32u; acc >>= 32; have -= 32u; }
            };
            bgzt_tokens(K, [&](uint32_t sym, int kind, uint32_t xbits, uint32_t xval) {
                const uint32_t e = ent[sym];
                const uint32_t l = e >> 16;
                push((e & 0xffffu) | (xval << l), l + xbits);  // the code, the extra bits of a length code
                if (kind) {                                    // the distance code, its extra bits
                    const uint32_t de = dent[kind == 2 ? dsym : 0u], dl = de >> 16;
                    push((de & 0xffffu) | ((kind == 2 ? deval : 0u) << dl), dl + (kind == 2 ? debits : 0u));
                }
            });
            or_bits(pos, acc);
        }
        fill += tile_bits;
        flush(false);
    }
    // ---- end of block; the empty stored block that ends the member: BFINAL 1, BTYPE 00, padding, LEN = 0, NLEN = 0xffff;
    // CRC-32 and ISIZE
    if (threadIdx.x == 0) or_bits(fill, ent[256] & 0xffffu);
    fill += ent[256] >> 16;
    if (threadIdx.x == 0) or_bits(fill, 1ull);
    fill += 3u;
    fill = (fill + 7u) & ~7u;
    if (threadIdx.x == 0) {
        or_bits(fill + 16u, 0xffffull);
        or_bits(fill + 32u, (uint64_t)A.block_crc[b] | ((uint64_t)n << 32));
    }
    fill += 96u;
    flush(true);
}

}  // namespace iss
