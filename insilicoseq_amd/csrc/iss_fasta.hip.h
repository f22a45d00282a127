// iss_fasta.hip.h -- `generate --device_fasta`: a FASTA text indexed and its line ends removed on the device (the grammar:
// iss_fasta_core.h).  Plain vector code: 256 lanes, one uint4 -- 16 bytes -- per lane, a tile of 4 096 bytes per
// workgroup, every byte offset 64-bit.
//
//   the index (iss_fa_index)
//   a  k_fa_count   per tile: header starts, line-end bytes ('\r', '\n') and odd bytes; a header start looks one byte back, across the
//                   tile's edge too
//   b  k_fa_scan    exclusive scan of the three counts over the tiles (one workgroup, FA_SCAN_SPAN tiles per pass); [n_tiles]: the totals
//   c  k_fa_heads   header number r of the text, at byte p, makes header_off[r] = p (r: the tile's prefix plus a scan inside the tile)
//   d  k_fa_rows    one lane per record: it walks the header line to its '\n' (a megabyte header: correct and slow), then fa_row();
//                   letters = body_len - line-end bytes of the body, flags = odd bytes of the body > 0, both from fa_prefix_at():
//                   the tile's prefix plus a count inside the tile
//   the upload (iss_genome_upload_fasta), behind a and b over the span it was given
//   e  k_fa_bases   per record: line-end bytes in front of its body
//   f  k_fa_strip   input-centric: a lane owns 16 bytes of the span, finds the record whose body holds its first byte by binary
//                   search over the bodies' offsets (bounded by the two searches its tile made) and walks on from there -- 16 bytes can
//                   hold several tiny records.  A letter's rank in its record is its offset in the body minus the line-end bytes of
//                   the body in front of it; it is stored at dest[record] + rank only if 0 <= rank < letters[record], and counted in
//                   *bad otherwise: a table that does not fit the text cannot write outside the records' places.
#pragma once

#include "iss_fasta_core.h"

namespace iss {
namespace fa {

constexpr int FA_THREADS = 256;
constexpr int FA_TILE = FA_THREADS * 16;               // bytes of a tile: one uint4 per lane
constexpr int FA_SCAN_PER = 4;                         // tile counts per lane and pass of k_fa_scan
constexpr int FA_SCAN_SPAN = FA_THREADS * FA_SCAN_PER;  // tiles per pass of k_fa_scan

struct FaText {
    const uint8_t *text;      // 16-byte aligned; readable up to the next multiple of FA_TILE
    int64_t n_bytes;          // >= 1
    int64_t n_tiles;          // ceil(n_bytes / FA_TILE)
    unsigned long long *pre;  // [3][n_tiles + 1]: header starts, line-end bytes, odd bytes -- per tile (a), then of the tiles before (b)
};
__device__ __forceinline__ unsigned long long *fa_pre(const FaText &A, int which) { return A.pre + (size_t)which * (size_t)(A.n_tiles + 1); }

struct FaRows {  // the index's table on the device, [n_rec] each
    int64_t n_rec;
    int64_t *header_off, *header_len, *body_off, *body_len, *letters;
    int32_t *flags;
};

struct FaStrip {  // the upload's table on the device, [n_rec] each
    int64_t n_rec;
    const int64_t *body_off, *body_len, *letters, *dest;  // dest: where the record's first letter goes in `out`
    unsigned long long *e0;                               // (e) line-end bytes of the span in front of body_off
    uint8_t *out;
    unsigned long long *bad;  // letters that would have fallen outside their record's place
};

// the lane's 16 bytes at `at` (a multiple of 16) and their masks; bytes at or past the text's end are no bytes
__device__ __forceinline__ Masks16 fa_lane(const FaText &A, int64_t at, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (at >= A.n_bytes) return Masks16{0u, 0u, 0u};
    const uint4 v = *reinterpret_cast<const uint4 *>(A.text + at);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    const int64_t left = A.n_bytes - at;
    return fa_masks16(w, left >= 16 ? 16 : (int)left, at > 0 ? (uint32_t)A.text[at - 1] : 0x0Au);
}

// exclusive scan over the workgroup's FA_THREADS values; *total: their sum.  `sh`: one word per wavefront
__device__ __forceinline__ unsigned long long fa_block_scan(unsigned long long v, unsigned long long *sh, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long x = __shfl_up(incl, (unsigned)d, 64);
        if (lane >= d) incl += x;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    unsigned long long base = 0ull, sum = 0ull;
#pragma unroll
    for (int k = 0; k < FA_THREADS / 64; ++k) {
        const unsigned long long s = sh[k];
        base += k < wave ? s : 0ull;
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return base + incl - v;
}

// a  grid = n_tiles.  The three counts of a lane, each at most 16, of a tile at most 4 096: packed 20 bits apart for one scan
__global__ __launch_bounds__(FA_THREADS) void k_fa_count(const FaText A) {
    __shared__ unsigned long long sh[FA_THREADS / 64];
    uint32_t w[4];
    const Masks16 m = fa_lane(A, (int64_t)blockIdx.x * FA_TILE + (int64_t)threadIdx.x * 16, w);
    unsigned long long total;
    (void)fa_block_scan((unsigned long long)__popc(m.head) << 40 | (unsigned long long)__popc(m.eol) << 20 | (unsigned long long)__popc(m.odd),
                        sh, &total);
    if (threadIdx.x == 0) {
        fa_pre(A, 0)[blockIdx.x] = total >> 40;
        fa_pre(A, 1)[blockIdx.x] = (total >> 20) & 0xFFFFFull;
        fa_pre(A, 2)[blockIdx.x] = total & 0xFFFFFull;
    }
}

// b  one workgroup: pre[which][t] -> the count of the tiles before t; pre[which][n_tiles]: the total
__global__ __launch_bounds__(FA_THREADS) void k_fa_scan(const FaText A) {
    __shared__ unsigned long long sh[FA_THREADS / 64];
    for (int which = 0; which < 3; ++which) {
        unsigned long long *p = fa_pre(A, which), carry = 0ull;
        for (int64_t base = 0; base < A.n_tiles; base += FA_SCAN_SPAN) {
            const int64_t at = base + (int64_t)threadIdx.x * FA_SCAN_PER;
            unsigned long long v[FA_SCAN_PER], s = 0ull;
#pragma unroll
            for (int k = 0; k < FA_SCAN_PER; ++k) {
                v[k] = at + k < A.n_tiles ? p[at + k] : 0ull;
                s += v[k];
            }
            unsigned long long total;
            unsigned long long run = carry + fa_block_scan(s, sh, &total);
#pragma unroll
            for (int k = 0; k < FA_SCAN_PER; ++k) {
                if (at + k < A.n_tiles) p[at + k] = run;
                run += v[k];
            }
            carry += total;
        }
        if (threadIdx.x == 0) p[A.n_tiles] = carry;
    }
}

// c  grid = n_tiles
__global__ __launch_bounds__(FA_THREADS) void k_fa_heads(const FaText A, const FaRows R) {
    __shared__ unsigned long long sh[FA_THREADS / 64];
    uint32_t w[4];
    const int64_t at = (int64_t)blockIdx.x * FA_TILE + (int64_t)threadIdx.x * 16;
    const Masks16 m = fa_lane(A, at, w);
    unsigned long long total;
    int64_t r = (int64_t)(fa_pre(A, 0)[blockIdx.x] + fa_block_scan((unsigned long long)__popc(m.head), sh, &total));
    for (uint32_t left = m.head; left; left &= left - 1u, ++r)
        if (r < R.n_rec) R.header_off[r] = at + (__ffs((int)left) - 1);
}

// line-end bytes and odd bytes of text[0, p), 0 <= p <= n_bytes: the prefix of p's tile, then the tile's bytes in front of p
__device__ __forceinline__ void fa_prefix_at(const FaText &A, int64_t p, unsigned long long *eol, unsigned long long *odd) {
    const int64_t tile = p / FA_TILE;
    unsigned long long e = fa_pre(A, 1)[tile], o = fa_pre(A, 2)[tile];
    for (int64_t q = tile * FA_TILE; q < p; q += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(A.text + q);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const Masks16 m = fa_masks16(w, p - q >= 16 ? 16 : (int)(p - q), 0u);
        e += (unsigned long long)__popc(m.eol);
        o += (unsigned long long)__popc(m.odd);
    }
    *eol = e;
    *odd = o;
}

// d  one lane per record, behind c
__global__ __launch_bounds__(FA_THREADS) void k_fa_rows(const FaText A, const FaRows R) {
    const int64_t r = (int64_t)blockIdx.x * FA_THREADS + threadIdx.x;
    if (r >= R.n_rec) return;
    const int64_t h = R.header_off[r], end = r + 1 < R.n_rec ? R.header_off[r + 1] : A.n_bytes;
    int64_t eol = h;
    while (eol < end && A.text[eol] != 0x0Au) ++eol;
    int64_t header_len, body_off, body_len;
    fa_row(h, eol, end, &header_len, &body_off, &body_len);
    unsigned long long e0, o0, e1, o1;
    fa_prefix_at(A, body_off, &e0, &o0);
    fa_prefix_at(A, end, &e1, &o1);
    R.header_len[r] = header_len;
    R.body_off[r] = body_off;
    R.body_len[r] = body_len;
    R.letters[r] = body_len - (int64_t)(e1 - e0);
    R.flags[r] = o1 != o0 ? FA_ODD : 0;
}

// e  one lane per record of the upload's table
__global__ __launch_bounds__(FA_THREADS) void k_fa_bases(const FaText A, const FaStrip S) {
    const int64_t k = (int64_t)blockIdx.x * FA_THREADS + threadIdx.x;
    if (k >= S.n_rec) return;
    unsigned long long e, o;
    fa_prefix_at(A, S.body_off[k], &e, &o);
    S.e0[k] = e;
}

// f  grid = n_tiles, behind e.  The table has passed fa_table_check over [0, n_bytes): bodies inside the text, ascending, disjoint.
__global__ __launch_bounds__(FA_THREADS) void k_fa_strip(const FaText A, const FaStrip S) {
    __shared__ unsigned long long sh[FA_THREADS / 64];
    __shared__ int64_t k_range[2];
    uint32_t w[4];
    const int64_t tile0 = (int64_t)blockIdx.x * FA_TILE, at = tile0 + (int64_t)threadIdx.x * 16;
    const Masks16 m = fa_lane(A, at, w);
    unsigned long long total;
    const unsigned long long e_at = fa_pre(A, 1)[blockIdx.x] + fa_block_scan((unsigned long long)__popc(m.eol), sh, &total);
    // the records a byte of this tile can belong to: from the last body that starts at or before the tile to the last one that starts inside it
    if (threadIdx.x == 0) {
        const int64_t k = fa_find(S.body_off, S.n_rec, tile0);
        k_range[0] = k < 0 ? 0 : k;
    }
    if (threadIdx.x == 64) {
        const int64_t last = tile0 + FA_TILE < A.n_bytes ? tile0 + FA_TILE : A.n_bytes;
        k_range[1] = fa_find(S.body_off, S.n_rec, last - 1);
    }
    __syncthreads();
    if (at >= A.n_bytes) return;
    const int64_t k_lo = k_range[0], k_hi = k_range[1];
    if (k_hi < k_lo) return;
    const int64_t first = fa_find(S.body_off + k_lo, k_hi - k_lo + 1, at);
    const int64_t stop = at + 16 < A.n_bytes ? at + 16 : A.n_bytes;
    unsigned long long n_bad = 0ull;
    for (int64_t k = k_lo + (first < 0 ? 0 : first); k <= k_hi; ++k) {
        const int64_t b0 = S.body_off[k];
        if (b0 >= stop) break;
        const int64_t b1 = b0 + S.body_len[k];
        const int j0 = (int)((at > b0 ? at : b0) - at), j1 = (int)((stop < b1 ? stop : b1) - at);
        if (j0 >= j1) continue;
        const int64_t L = S.letters[k], d = S.dest[k];
        // offset in the body minus the body's line-end bytes in front: of byte j, minus those among the lane's bytes below j
        const int64_t rank0 = (at - b0) - (int64_t)(e_at - S.e0[k]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < j0 || j >= j1 || ((m.eol >> j) & 1u)) continue;
            const int64_t rank = rank0 + j - (int64_t)__popc(m.eol & ((1u << j) - 1u));
            if (rank >= 0 && rank < L) S.out[d + rank] = (uint8_t)fa_byte16(w, j);
            else ++n_bad;
        }
    }
    if (n_bad) atomicAdd(S.bad, n_bad);
}

}  // namespace fa
}  // namespace iss
