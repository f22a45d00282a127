// iss_vcf.hip.h -- the --store_mutations VCF text built on the device.
//
// The reference writes one row per mutation (write_mutations, iss/generator.py:598-620):
//     "{record.id}_{i}_{cpu}/{mate + 1}\t{position + 1}\t.\t{ref}\t{alt}\t{qual}\t\t\n"
// alt = ref + alt for an insertion, qual = the phred of a substitution and '.' otherwise.  The rows stand in HBM as MutRecord
// (iss_kernels.hip.h).  MT mode leaves them in the reference's order; the Philox kernels append them unordered, with unused
// slots and with stale rows of the reads the indel fix-up rebuilt.  The stages:
//   a  k_vcf_count     Philox: which slots stay (the filter of iss_mutations_download), counted per pair
//      scan            exclusive scan of the counts: a pair's rows are one segment
//   b  k_vcf_scatter   the slots that stay -> their pair's segment, with the 32 key bits that order them inside it
//      k_vcf_rank      a row's place in its segment = the keys of the segment below its own (keys are unique)
//   c  k_vcf_len       length of every row's text;  scan: byte offset of every row
//   d  k_vcf_format    one lane per row writes its text
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iss_kernels.hip.h"  // MutRecord

namespace iss {

// ------------------------------------------------------------------ exclusive scan of uint32 counts into uint64 offsets
// out[i] = in[0] + .. + in[i - 1] for i in [0, n]; three launches: sums of tiles, scan of the sums (one workgroup), the tiles
constexpr int VSCAN_THREADS = 256, VSCAN_PER = 8, VSCAN_TILE = VSCAN_THREADS * VSCAN_PER;

// exclusive scan over the workgroup's VSCAN_THREADS values; *total: their sum.  `sh`: VSCAN_THREADS words of LDS
__device__ __forceinline__ uint64_t vcf_block_scan(uint64_t v, uint64_t *sh, uint64_t *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < VSCAN_THREADS; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[VSCAN_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// grid = ceil(n / VSCAN_TILE): tile_sum[b] = sum of tile b
__global__ __launch_bounds__(VSCAN_THREADS) void k_vcf_scan_sums(const uint32_t *in, uint64_t n, uint64_t *tile_sum) {
    __shared__ uint64_t sh[VSCAN_THREADS];
    const uint64_t at = (uint64_t)blockIdx.x * VSCAN_TILE + (uint64_t)threadIdx.x * VSCAN_PER;
    uint64_t s = 0;
    for (int k = 0; k < VSCAN_PER; ++k)
        if (at + k < n) s += in[at + k];
    uint64_t total;
    (void)vcf_block_scan(s, sh, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum[b] -> sum of the tiles before b; *grand = sum of all
__global__ __launch_bounds__(VSCAN_THREADS) void k_vcf_scan_tiles(uint64_t *tile_sum, uint64_t n_tiles, uint64_t *grand) {
    __shared__ uint64_t sh[VSCAN_THREADS];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += VSCAN_THREADS) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? tile_sum[i] : 0;
        uint64_t total;
        const uint64_t ex = vcf_block_scan(v, sh, &total);
        if (i < n_tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *grand = carry;
}

// grid = ceil(n / VSCAN_TILE): out[i] for the tile's elements (out[n] is k_vcf_scan_tiles' *grand)
__global__ __launch_bounds__(VSCAN_THREADS) void k_vcf_scan_apply(const uint32_t *in, uint64_t n, const uint64_t *tile_sum, uint64_t *out) {
    __shared__ uint64_t sh[VSCAN_THREADS];
    const uint64_t at = (uint64_t)blockIdx.x * VSCAN_TILE + (uint64_t)threadIdx.x * VSCAN_PER;
    uint32_t v[VSCAN_PER];
    uint64_t s = 0;
    for (int k = 0; k < VSCAN_PER; ++k) {
        v[k] = at + k < n ? in[at + k] : 0;
        s += v[k];
    }
    uint64_t total;
    uint64_t run = tile_sum[blockIdx.x] + vcf_block_scan(s, sh, &total);
    for (int k = 0; k < VSCAN_PER; ++k) {
        if (at + k < n) out[at + k] = run;
        run += v[k];
    }
}

// ------------------------------------------------------------------ rows -> text
// One emit call formats the rows of several work items: item k = pairs [pair0, pair0 + n_pairs) of the generate call, under
// "{id_k}_{first_i + (pair - pair0)}_{cpu_k}".  Items stand in ascending pair order and do not overlap.
// The rows of a worker set (VcfArgs::wbase): item k is worker k's piece, the rows of the text are the
// workers' rows one worker after the other, and a row's item is its worker -- pair numbers start at 0 in every worker.
struct VcfItem {
    uint64_t first_i;   // pair id of the item's first pair
    int64_t pair0;      // the item's first pair, counted from the call's first pair
    int64_t n_pairs;
    uint32_t id_off;    // of the record id in `ids`
    int32_t id_len;
    int32_t cpu_len;
    char cpu[12];       // the worker's number in decimal
};

struct VcfArgs {
    const MutRecord *mut;     // Philox: the reserved slots; MT mode: the rows, in order
    uint32_t n_slots;         // slots to look at (an upper bound of the rows)
    int64_t n_pairs;          // pairs of the generate call
    const uint32_t *flags;    // Philox: the call's flag words (which mates the fix-up rebuilt)
    uint32_t *cnt;            // [n_pairs] rows that stay per pair (k_vcf_scatter counts them down again)
    uint64_t *seg;            // [n_pairs + 1] first row of every pair's segment; seg[n_pairs] = rows that stay
    uint32_t *key, *slot;     // [n_slots] scattered by segment: low key bits and slot of a row
    uint32_t *order;          // [n_slots] row j of the text -> its slot (NULL: slot j, MT mode)
    const uint64_t *n_rows;   // rows of the text (Philox: &seg[n_pairs]; NULL: n_slots)
    uint32_t *len;            // [n_slots] bytes of row j (0 behind the last row, and for rows of no item)
    uint64_t *off;            // [n_slots + 1] byte offset of row j; off[n_slots] = bytes of the text
    uint8_t *text;
    uint64_t text_cap;
    const VcfItem *items;
    const char *ids;
    int32_t n_items;
    // a worker set: row j of the text is row j - wbase[k] of worker k = the last k with wbase[k] <= j, whose rows start at
    // mut + k * wstride ([n_items + 1], wbase[n_items] = n_slots; NULL: one worker, or the Philox slots)
    const uint64_t *wbase;
    uint64_t wstride;
    uint64_t *wbytes;         // out [n_items + 1]: byte offset of worker k's first row in the text (k_vcf_worker_bytes)
    uint32_t *stats;          // ISS_VCF_DEBUG (else NULL): [0] slots that hold a row, [1] rows that stay
};

// does the row in this slot stay?  (iss_mutations_download: used slots; k_main's rows only for mates the fix-up did not rebuild)
// `n_pairs`, `flags`: the pairs of the generate call and its flag words.  The one statement of the filter on the device: the VCF
// text and the truth arrays (iss_truth.hip.h) both go through it.
__device__ __forceinline__ bool mut_row_stays(const MutRecord &r, int64_t n_pairs, const uint32_t *flags) {
    if (r.pair < 0 || (int64_t)r.pair >= n_pairs) return false;
    if ((uint8_t)r.type & 32) return true;
    const uint32_t f = flags[r.pair];
    const int mate = r.mate & 1;
    return (((f >> mate) | (f >> (2 + mate))) & 1u) == 0;
}
__device__ __forceinline__ bool vcf_keep(const VcfArgs &A, const MutRecord &r) { return mut_row_stays(r, A.n_pairs, A.flags); }

// the low half of iss_mutations_download's key: mate, indel rows (loop order) before substitution rows, position, slot of the step
__device__ __forceinline__ uint32_t vcf_key(const MutRecord &r) {
    const uint32_t t = (uint8_t)r.type;
    const uint32_t phase = (t & 3) == 0 ? 1u : 0u;
    return ((uint32_t)(r.mate & 1) << 31) | (phase << 30) | ((uint32_t)(uint16_t)r.position << 8) | ((t >> 2) & 7u);
}

constexpr int VCF_THREADS = 256;

// a. grid-stride over the slots
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_count(VcfArgs A) {
    for (uint64_t i = (uint64_t)blockIdx.x * VCF_THREADS + threadIdx.x; i < A.n_slots; i += (uint64_t)gridDim.x * VCF_THREADS) {
        const MutRecord r = A.mut[i];
        const bool keep = vcf_keep(A, r);
        if (keep) atomicAdd(&A.cnt[r.pair], 1u);
        if (A.stats) {
            if (r.pair >= 0) atomicAdd(&A.stats[0], 1u);
            if (keep) atomicAdd(&A.stats[1], 1u);
        }
    }
}

// b. the rows that stay, into their pair's segment (in any order: k_vcf_rank orders them)
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_scatter(VcfArgs A) {
    for (uint64_t i = (uint64_t)blockIdx.x * VCF_THREADS + threadIdx.x; i < A.n_slots; i += (uint64_t)gridDim.x * VCF_THREADS) {
        const MutRecord r = A.mut[i];
        if (!vcf_keep(A, r)) continue;
        const uint64_t p = A.seg[r.pair] + (uint64_t)(atomicSub(&A.cnt[r.pair], 1u) - 1u);
        if (p >= A.n_slots) continue;  // (cannot happen: the segments hold what k_vcf_count counted)
        A.key[p] = vcf_key(r);
        A.slot[p] = (uint32_t)i;
    }
}

// b. one lane per scattered row: its place inside the segment is the number of keys below its own
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_rank(VcfArgs A) {
    const uint64_t n_rows = *A.n_rows < A.n_slots ? *A.n_rows : A.n_slots;
    for (uint64_t p = (uint64_t)blockIdx.x * VCF_THREADS + threadIdx.x; p < n_rows; p += (uint64_t)gridDim.x * VCF_THREADS) {
        const uint32_t s = A.slot[p];
        const int32_t pair = A.mut[s].pair;
        const uint64_t lo = A.seg[pair], hi = A.seg[pair + 1];
        const uint32_t k = A.key[p];
        uint64_t below = 0;
        for (uint64_t q = lo; q < hi; ++q) below += A.key[q] < k ? 1 : 0;
        A.order[lo + below] = s;
    }
}

__device__ __forceinline__ int vcf_digits(uint64_t v) {
    int dg = 1;
    for (uint64_t p = 10; dg < 20 && v >= p; p *= 10) ++dg;
    return dg;
}
__device__ __forceinline__ int vcf_signed_len(int32_t v) { return v < 0 ? 1 + vcf_digits((uint64_t)(-(int64_t)v)) : vcf_digits((uint64_t)v); }
// decimal of v, `n` characters (vcf_digits / vcf_signed_len), at w
__device__ __forceinline__ void vcf_put_u64(uint8_t *w, uint64_t v, int n) {
    for (int k = n - 1; k >= 0; --k) { w[k] = (uint8_t)('0' + (int)(v % 10)); v /= 10; }
}
__device__ __forceinline__ void vcf_put_signed(uint8_t *w, int32_t v, int n) {
    if (v < 0) { w[0] = '-'; vcf_put_u64(w + 1, (uint64_t)(-(int64_t)v), n - 1); }
    else vcf_put_u64(w, (uint64_t)v, n);
}

// the item of pair p: the last one that starts at or before p, if p lies inside it (else -1)
__device__ __forceinline__ int vcf_item_of(const VcfArgs &A, int64_t p) {
    if (A.n_items <= 0) return -1;
    int lo = 0, hi = A.n_items;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.items[mid].pair0 <= p) lo = mid; else hi = mid;
    }
    const VcfItem &it = A.items[lo];
    return p >= it.pair0 && p < it.pair0 + it.n_pairs ? lo : -1;
}

// row j of the text and its item (-1: none)
__device__ __forceinline__ MutRecord vcf_row(const VcfArgs &A, uint64_t j, int *item) {
    if (A.wbase) {
        int lo = 0, hi = A.n_items;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (A.wbase[mid] <= j) lo = mid; else hi = mid;
        }
        const MutRecord r = A.mut[(uint64_t)lo * A.wstride + (j - A.wbase[lo])];
        *item = r.pair >= 0 && (int64_t)r.pair < A.items[lo].n_pairs ? lo : -1;
        return r;
    }
    const MutRecord r = A.mut[A.order ? A.order[j] : (uint32_t)j];
    *item = vcf_item_of(A, r.pair);
    return r;
}

__device__ __forceinline__ uint64_t vcf_rows(const VcfArgs &A) {
    if (!A.n_rows) return A.n_slots;
    return *A.n_rows < A.n_slots ? *A.n_rows : A.n_slots;
}

// c. one lane per row j of the text (every j < n_slots gets a length: the scan runs over all of them)
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_len(VcfArgs A) {
    const uint64_t n_rows = vcf_rows(A);
    for (uint64_t j = (uint64_t)blockIdx.x * VCF_THREADS + threadIdx.x; j < A.n_slots; j += (uint64_t)gridDim.x * VCF_THREADS) {
        uint32_t len = 0;
        if (j < n_rows) {
            int k;
            const MutRecord r = vcf_row(A, j, &k);
            if (k >= 0) {
                const VcfItem &it = A.items[k];
                const int type = r.type & 3;
                len = (uint32_t)it.id_len + (uint32_t)it.cpu_len + 14u + (uint32_t)vcf_digits(it.first_i + (uint64_t)(r.pair - it.pair0)) +
                      (uint32_t)vcf_signed_len((int32_t)r.position + 1) + (type == 1 ? 2u : 1u) +
                      (type == 0 ? (uint32_t)vcf_signed_len(r.quality) : 1u);
            }
        }
        A.len[j] = len;
    }
}

// d. one lane per row: "{id}_{i}_{cpu}/{mate + 1}\t{position + 1}\t.\t{ref}\t{alt}\t{qual}\t\t\n" at its offset
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_format(VcfArgs A) {
    const uint64_t n_rows = vcf_rows(A);
    for (uint64_t j = (uint64_t)blockIdx.x * VCF_THREADS + threadIdx.x; j < n_rows; j += (uint64_t)gridDim.x * VCF_THREADS) {
        const uint32_t len = A.len[j];
        const uint64_t at = A.off[j];
        if (!len || at + len > A.text_cap) continue;  // (a row of no item; the second test cannot fail: the host sized the text)
        int ki;
        const MutRecord r = vcf_row(A, j, &ki);
        const VcfItem it = A.items[ki];
        uint8_t *w = A.text + at;
        const char *id = A.ids + it.id_off;
        for (int k = 0; k < it.id_len; ++k) w[k] = (uint8_t)id[k];
        w += it.id_len;
        *w++ = '_';
        const uint64_t g = it.first_i + (uint64_t)(r.pair - it.pair0);
        int n = vcf_digits(g);
        vcf_put_u64(w, g, n);
        w += n;
        *w++ = '_';
        for (int k = 0; k < it.cpu_len; ++k) w[k] = (uint8_t)it.cpu[k];
        w += it.cpu_len;
        *w++ = '/';
        *w++ = (uint8_t)('1' + (r.mate & 1));
        *w++ = '\t';
        n = vcf_signed_len((int32_t)r.position + 1);
        vcf_put_signed(w, (int32_t)r.position + 1, n);
        w += n;
        *w++ = '\t'; *w++ = '.'; *w++ = '\t';
        *w++ = r.ref;
        *w++ = '\t';
        const int type = r.type & 3;
        if (type == 1) *w++ = r.ref;  // insertion: alt = ref + the inserted letter
        *w++ = r.alt;
        *w++ = '\t';
        if (type == 0) {
            n = vcf_signed_len(r.quality);
            vcf_put_signed(w, r.quality, n);
            w += n;
        } else {
            *w++ = '.';
        }
        *w++ = '\t'; *w++ = '\t'; *w++ = '\n';
    }
}

// a worker set: where every worker's rows start in the text (the writer thread appends each range to its worker's file)
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_worker_bytes(VcfArgs A) {
    for (int k = blockIdx.x * VCF_THREADS + threadIdx.x; k <= A.n_items; k += gridDim.x * VCF_THREADS) A.wbytes[k] = A.off[A.wbase[k]];
}

}  // namespace iss
