// iss_ubam.hip.h -- unaligned BAM built on the device (`generate --ubam`): the rows as BAM alignment records
// (SAM/BAM specification 4.2: no reference, no CIGAR, no tags) in ONE byte stream, R1 then R2 of every pair, and that stream as
// BGZF blocks (specification 4.1) -- every 32 768 bytes of it one complete gzip member with the `BC` field.
//
// k_ubam_format is k_fastq_format for another layout: a record's length is C + digits(i), so the offset of (pair i, mate) is a
// closed form of i and one wavefront writes one record without a scan.  The members reuse the scheme of iss_deflate.hip.h -- one
// dynamic Huffman code per emit call (k_deflate_build), run and previous-record matches found inside 32-byte chunks
// (deflate_tokens), sizes, a scan (k_deflate_scan), bit packing through LDS -- under the MEMBER rule: a member is inflated with an
// empty window, so a chunk at a block's start has no predecessor byte, and a previous-record source counts only if it lies inside
// the block.  The kernels of iss_deflate.hip.h are not touched: k_bgzf_hist / k_bgzf_len / k_bgzf_encode are their siblings here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iss_fastq.hip.h"    // FastqItem, digits_before
#include "iss_deflate.hip.h"

namespace iss {

constexpr int UBAM_FIXED = 36;        // block_size and the 32 fixed bytes behind it
constexpr int UBAM_NAME_MAX = 254;    // characters of a read name: l_read_name (uint8) counts the NUL too
constexpr uint32_t BGZF_FRAME = 26;   // 18 bytes of member header, CRC-32, ISIZE
constexpr uint32_t BGZF_MAX = 65536;  // a member's size: BSIZE - 1 is a uint16
// 32 768 literals at the 15-bit code limit (a match spends at most 31 bits on three bytes or more), the dynamic header's words,
// end of block + the stored block's header and padding (< 4 bytes) + LEN / NLEN, the frame
static_assert(DEFLATE_BLOCK * 15 / 8 + DEFLATE_HDR_WORDS * 4 + 8 + BGZF_FRAME <= BGZF_MAX, "a BGZF member of one block fits BSIZE");

// 4-bit code of a base ("=ACMGRSVTWYHKDBN"): BAM has no case, so lower-case letters count as their capitals; any byte that is not
// an IUPAC letter ('=' included: the rows never hold it) is N
__host__ __device__ inline uint32_t ubam_code(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    switch (c) {
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
        case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
        case 'D': return 13; case 'B': return 14; default: return 15;
    }
}

// byte k < UBAM_FIXED of a record: block_size, refID -1, pos -1, l_read_name, mapq 0, bin 4680 (reg2bin(-1, 0)), n_cigar_op 0,
// flag, l_seq, next_refID -1, next_pos -1, tlen 0 -- nine little-endian words
__host__ __device__ inline uint8_t ubam_fixed_byte(int k, uint32_t block_size, uint32_t l_read_name, uint32_t flag, uint32_t l_seq) {
    uint32_t w;
    switch (k >> 2) {
        case 0: w = block_size; break;
        case 3: w = l_read_name | (4680u << 16); break;
        case 4: w = flag << 16; break;
        case 5: w = l_seq; break;
        case 8: w = 0; break;
        default: w = 0xffffffffu; break;
    }
    return (uint8_t)(w >> (8 * (k & 3)));
}
__host__ __device__ inline uint32_t ubam_flag(int mate) { return mate ? 141u : 77u; }  // paired, both unmapped, first / last

// bytes of a record but for the digits of its pair number
__host__ __device__ inline uint64_t ubam_record_const(uint64_t id_len, uint64_t cpu_len, uint64_t RL) {
    return (uint64_t)UBAM_FIXED + id_len + cpu_len + 3ull + (RL + 1ull) / 2ull + RL;
}

// The item table is iss_fastq_emit_batch's (rec_first counts PAIRS; text_off: the item's first record in the one stream).
struct UbamArgs {
    const uint8_t *base[2], *qual[2];  // output rows (row 0): [mate]
    uint8_t *text;
    const FastqItem *items;
    const char *ids;
    int32_t n_items, row, RL;
    int64_t n_pairs;                   // of all items
};

// grid = ceil(2 n_pairs / FASTQ_WAVES), block = 64 * FASTQ_WAVES: one wavefront per record.  Records are not aligned: bytes.
__global__ __launch_bounds__(64 * FASTQ_WAVES) void k_ubam_format(UbamArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * FASTQ_WAVES + (threadIdx.x >> 6);
    if (r >= 2 * A.n_pairs) return;
    const int64_t pair = r >> 1;
    const int mate = (int)(r & 1);
    int lo = 0, hi = A.n_items;  // the item of the pair: largest k with rec_first[k] <= pair
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.items[mid].rec_first <= pair) lo = mid; else hi = mid;
    }
    const FastqItem it = A.items[lo];
    const int64_t i = pair - it.rec_first;
    const uint64_t g = it.first_i + (uint64_t)i;
    int dg = 1;
    for (uint64_t p = 10; dg < 20 && g >= p; p *= 10) ++dg;
    const int half = (A.RL + 1) >> 1;
    const uint64_t C = ubam_record_const((uint64_t)it.id_len, (uint64_t)it.cpu_len, (uint64_t)A.RL);
    uint8_t *w = A.text + it.text_off + 2ull * ((uint64_t)i * C + (digits_before(g) - it.before_first)) + (mate ? C + (uint64_t)dg : 0ull);
    const int n1 = it.id_len;           // id
    const int n2 = n1 + 1 + dg;         // '_' digits
    const int nlen = n2 + 1 + it.cpu_len;  // '_' cpu
    if (lane < UBAM_FIXED) w[lane] = ubam_fixed_byte(lane, (uint32_t)(C + (uint64_t)dg) - 4u, (uint32_t)nlen + 1u, ubam_flag(mate), (uint32_t)A.RL);
    w += UBAM_FIXED;
    const char *id = A.ids + it.id_off;
    for (int k = lane; k <= nlen; k += 64) {
        char c;
        if (k < n1) c = id[k];
        else if (k == n1) c = '_';
        else if (k < n2) {
            uint64_t v = g;
            for (int z = n2 - 1 - k; z > 0; --z) v /= 10;  // digit (n2 - 1 - k) from the right
            c = (char)('0' + (int)(v % 10));
        } else if (k == n2) c = '_';
        else if (k < nlen) c = it.cpu[k - n2 - 1];
        else c = 0;
        w[k] = (uint8_t)c;
    }
    w += nlen + 1;
    const uint8_t *b = A.base[mate] + (size_t)(it.first_pair + i) * A.row;
    const uint8_t *q = A.qual[mate] + (size_t)(it.first_pair + i) * A.row;
    for (int k = lane; k < half; k += 64) {  // first base in the high nibble; the low nibble past an odd length is 0
        const uint32_t h = ubam_code(b[xp(2 * k)]), l = 2 * k + 1 < A.RL ? ubam_code(b[xp(2 * k + 1)]) : 0u;
        w[k] = (uint8_t)((h << 4) | l);
    }
    w += half;
    for (int k = lane; k < A.RL; k += 64) w[k] = q[xp(k)];  // the raw phred
}

// ---------------------------------------------------------------- BGZF: one member per block
// The kernels take a DeflateArgs with the arrays of mate 0 only; block_bytes holds MEMBER sizes (deflate bytes + BGZF_FRAME),
// block_crc the standard CRC-32 of each block's text (initial value and final xor applied), block_off the members' offsets.

// chunk `c` of the text under the member rule
__device__ __forceinline__ void bgzf_chunk(const uint8_t *t, uint64_t n_bytes, uint64_t c, uint32_t dist, DeflateChunk &C) {
    deflate_chunk(t, n_bytes, c, dist, C);
    const uint32_t in_block = (uint32_t)((c * DEFLATE_CHUNK) % DEFLATE_BLOCK);
    if (in_block == 0) C.prev = -1;
    if (in_block < dist) C.has_src = false;  // (the chunk's first source byte would lie before the block's start)
}

__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzf_hist(DeflateArgs A) {
    __shared__ uint32_t h[DEFLATE_SYMS];
    for (int s = threadIdx.x; s < DEFLATE_SYMS; s += DEFLATE_THREADS) h[s] = 0;
    __syncthreads();
    const uint64_t n_chunks = (A.n_bytes + DEFLATE_CHUNK - 1) / DEFLATE_CHUNK;
    for (uint64_t c = (uint64_t)blockIdx.x * DEFLATE_THREADS + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * DEFLATE_THREADS) {
        DeflateChunk C;
        bgzf_chunk(A.text[0], A.n_bytes, c, A.dist, C);
        deflate_tokens(C, [&](uint32_t sym, int, uint32_t, uint32_t) { atomicAdd(&h[sym], 1u); });
    }
    __syncthreads();
    for (int s = threadIdx.x; s < DEFLATE_SYMS; s += DEFLATE_THREADS)
        if (h[s]) atomicAdd(&A.hist[0][s], h[s]);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&A.hist[0][256], A.n_blocks);
}

// One workgroup per block: member size and CRC-32.  The CRC tree is k_deflate_len's (lane t owns the 128 bytes that end
// (256 - t) * 128 bytes before the block's end, zeros in front of a short block); the lane that owns the block's first byte
// starts it from 0xffffffff there -- the state in front of it is 0, so this is the standard CRC's initial value -- and the
// final xor is applied to the root.  Every block takes k_deflate_len's plain path (no LDS staging).
__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzf_len(DeflateArgs A) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t lens[DEFLATE_SYMS];
    __shared__ uint32_t red[DEFLATE_THREADS];
    __shared__ uint32_t crcs[DEFLATE_THREADS];
    __shared__ uint32_t shift[8][32];
    const uint32_t b = blockIdx.x;
    const DeflateCode *C = A.code[0];
    shift[threadIdx.x >> 5][threadIdx.x & 31] = C->crc_shift[threadIdx.x >> 5][threadIdx.x & 31];
    tab[threadIdx.x] = crc_table_entry(threadIdx.x);
    for (int s = threadIdx.x; s < DEFLATE_SYMS; s += DEFLATE_THREADS) lens[s] = C->entry[s] >> 16;
    __syncthreads();
    const uint64_t start = (uint64_t)b * DEFLATE_BLOCK;
    const uint32_t n = deflate_block_len(A.n_bytes, b);
    const uint8_t *t = A.text[0] + start;
    uint32_t bits = 0, crc = 0;
    const uint32_t kind_bits[3] = {0u, 1u, 1u + A.dist_ebits};
    for (uint32_t c = threadIdx.x; c * DEFLATE_CHUNK < n; c += DEFLATE_THREADS) {
        DeflateChunk K;
        bgzf_chunk(A.text[0], A.n_bytes, start / DEFLATE_CHUNK + c, A.dist, K);
        deflate_tokens(K, [&](uint32_t sym, int kind, uint32_t xbits, uint32_t) { bits += lens[sym] + xbits + kind_bits[kind]; });
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
        A.block_bytes[0][b] = (total + 7u) / 8u + 4u + BGZF_FRAME;      // + LEN = 0, NLEN = 0xffff, + the member's frame
        A.block_crc[0][b] = crcs[0] ^ 0xffffffffu;
    }
}

// One workgroup per block, k_deflate_encode's tiles and window; the member's header goes through the window in front of the
// block's bits and CRC-32 + ISIZE behind them, so the member is written like a block was: whole words, the first and the
// last merged with atomicOr (the buffer is zeroed).  The empty stored block is the member's last: BFINAL = 1.
__global__ __launch_bounds__(DEFLATE_THREADS) void k_bgzf_encode(DeflateArgs A) {
    __shared__ uint32_t ent[DEFLATE_SYMS];
    __shared__ uint32_t win[DEFLATE_WIN_WORDS];
    __shared__ uint32_t wsum[DEFLATE_THREADS / 64];
    const uint32_t b = blockIdx.x;
    const DeflateCode *C = A.code[0];
    for (int s = threadIdx.x; s < DEFLATE_SYMS; s += DEFLATE_THREADS) ent[s] = C->entry[s];
    for (int i = threadIdx.x; i < DEFLATE_WIN_WORDS; i += DEFLATE_THREADS) win[i] = 0;
    __syncthreads();
    const uint64_t start = (uint64_t)b * DEFLATE_BLOCK;
    const uint32_t n = deflate_block_len(A.n_bytes, b);
    const uint64_t off = A.block_off[0][b];
    const uint32_t member = A.block_bytes[0][b];
    if (member > BGZF_MAX || off + member > A.out_cap) return;  // (the host finds the hole: it walks the BSIZE chain)
    uint32_t *outw = reinterpret_cast<uint32_t *>(A.out[0] + (off & ~3ull));
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
    const uint32_t kind_bits[3] = {0u, 1u, 1u + A.dist_ebits};
    for (uint32_t base = 0; base < n; base += DEFLATE_THREADS * DEFLATE_CHUNK) {
        const uint32_t at = base + threadIdx.x * DEFLATE_CHUNK;
        DeflateChunk K;
        uint32_t nb = 0;
        if (at < n) {
            bgzf_chunk(A.text[0], A.n_bytes, (start + at) / DEFLATE_CHUNK, A.dist, K);
            deflate_tokens(K, [&](uint32_t sym, int kind, uint32_t xbits, uint32_t) { nb += (ent[sym] >> 16) + xbits + kind_bits[kind]; });
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
            uint64_t acc = 0;  // bits not yet in the window (< 32 of them between tokens)
            deflate_tokens(K, [&](uint32_t sym, int kind, uint32_t xbits, uint32_t xval) {
                const uint32_t e = ent[sym];
                uint32_t v = e & 0xffffu, l = e >> 16;
                v |= xval << l; l += xbits;
                if (kind == 1) l += 1u;
                if (kind == 2) { v |= (1u | (A.dist_eval << 1)) << l; l += 1u + A.dist_ebits; }
                acc |= (uint64_t)v << have;
                have += l;
                if (have >= 32u) { or_bits(pos, acc & 0xffffffffull); pos += 32u; acc >>= 32; have -= 32u; }
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
        or_bits(fill + 32u, (uint64_t)A.block_crc[0][b] | ((uint64_t)n << 32));
    }
    fill += 96u;
    flush(true);
}

}  // namespace iss
