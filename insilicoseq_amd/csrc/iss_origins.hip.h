// iss_origins.hip.h -- `generate --origins`: where every pair came from, as BEDPE text built on the device.
//
// One line per pair, tab separated, no header:
//     {id} s1 e1 {id} s2 e2 {id}_{i}_{cpu} . + - isz \n
// With (fs, rs, re, isz) what iss_output_download_coords returns for the row, RL the read length and len the record's length,
// [s1, e1) is [fs, fs + RL) -- the template interval read 1 was cut from, iss/generator.py:135-147 -- and [s2, e2) is [rs, re)
// -- read 2's, generator.py:165-177 --, each clamped by the rule of section 19: s' = min(max(s, 0), len),
// e' = max(min(max(e, 0), len), s'), so that an interval that is empty after the clamp is written as "s' s'" (the clamp bites
// only with custom fragment lengths).  Read 1 is always '+' and read 2 always '-' (generator.py:149, 180), the score is '.', the
// name is the FASTQ read name without /1, /2, and the eleventh column is isz as drawn, a signed decimal.  Nothing is read from the
// mutation rows: these are the nominal intervals `--depth` counts.
//
//   k_origins_len     one lane per pair: descriptor -> record coordinates (the search of k_rows_export / k_depth_mark), clamp,
//                     bytes of the pair's line
//   scan              k_vcf_scan_sums / k_vcf_scan_tiles / k_vcf_scan_apply as they are: byte offset of every line
//   k_origins_format  one workgroup per tile of consecutive pairs: the lines composed in LDS, the tile's span stored in aligned
//                     16-byte pieces (k_rows_export's way out)
// Line length, clamp and the decimal writers are __host__ __device__: iss_origins_host_text formats with the same functions.
// Included by iss_mi355x.hip behind iss_ubam.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iss_kernels.hip.h"  // PairDesc, BatchItem

namespace iss {

constexpr int ORIGINS_THREADS = 256;
constexpr int ORIGINS_MAX_TILE = 256;             // pairs of a workgroup unless ISS_ORIGINS_TILE says otherwise: one per lane
constexpr size_t ORIGINS_LDS_BUDGET = 16 * 1024;  // of the 160 KB of a CU: ten workgroups per CU by LDS, no launch attribute
constexpr size_t ORIGINS_LDS_MAX = 48 * 1024;     // what ISS_ORIGINS_TILE may ask for
constexpr int ORIGINS_TARGET_WGS = 2048;          // k_origins_len: workgroups of a launch, about
// characters of a line beside the ids, the worker's number and the six numbers: ten tabs, '_' '_', '.', '+', '-', '\n'
constexpr uint32_t ORIGINS_FIXED = 16;

// One emit call formats the rows of several work items: iss_fastq_emit_batch's table plus the record lengths.
struct OriginsItem {
    uint64_t first_i;    // pair id of the item's first row
    int64_t first_pair;  // first output row
    int64_t rec_first;   // pairs of the items before this one
    int64_t rec_len;     // bases of the item's record
    uint32_t id_off;     // of the record id in `ids`
    int32_t id_len;
    int32_t cpu_len;
    char cpu[12];        // the worker's number in decimal
};

// the four numbers of a line's two intervals
struct OriginsSpan {
    int64_t s1, e1, s2, e2;
};

__host__ __device__ __forceinline__ int64_t origins_clamp(int64_t x, int64_t len) { return x < 0 ? 0 : (x > len ? len : x); }

// (fs, rs, re) in record coordinates -> the clamped intervals
__host__ __device__ __forceinline__ OriginsSpan origins_span(int64_t fs, int64_t rs, int64_t re, int64_t RL, int64_t len) {
    OriginsSpan o;
    o.s1 = origins_clamp(fs, len);
    o.e1 = origins_clamp((fs > len ? len : fs) + RL, len);  // (a start behind the record ends at len whatever RL adds: no overflow)
    if (o.e1 < o.s1) o.e1 = o.s1;
    o.s2 = origins_clamp(rs, len);
    o.e2 = origins_clamp(re, len);
    if (o.e2 < o.s2) o.e2 = o.s2;
    return o;
}

// decimal digits of v.  Coordinates and pair ids nearly always fit 32 bits: that path has no 64-bit division
__host__ __device__ __forceinline__ uint32_t origins_digits(uint64_t v) {
    if ((v >> 32) == 0) {
        const uint32_t x = (uint32_t)v;
        return x < 10u ? 1u : x < 100u ? 2u : x < 1000u ? 3u : x < 10000u ? 4u : x < 100000u ? 5u : x < 1000000u ? 6u :
               x < 10000000u ? 7u : x < 100000000u ? 8u : x < 1000000000u ? 9u : 10u;
    }
    uint32_t dg = 10;
    for (uint64_t p = 10000000000ull; dg < 20 && v >= p; p *= 10) ++dg;
    return dg;
}
__host__ __device__ __forceinline__ uint64_t origins_abs(int64_t v) { return v < 0 ? 0ull - (uint64_t)v : (uint64_t)v; }
__host__ __device__ __forceinline__ uint32_t origins_signed_len(int64_t v) { return (v < 0 ? 1u : 0u) + origins_digits(origins_abs(v)); }

// n = origins_digits(v) characters at w; returns w + n
__host__ __device__ __forceinline__ uint8_t *origins_put_u64(uint8_t *w, uint64_t v, uint32_t n) {
    uint32_t k = n;
    for (; (v >> 32) != 0 && k > 0; v /= 10) w[--k] = (uint8_t)('0' + (uint32_t)(v % 10));
    for (uint32_t x = (uint32_t)v; k > 0; x /= 10) w[--k] = (uint8_t)('0' + x % 10u);
    return w + n;
}
__host__ __device__ __forceinline__ uint8_t *origins_put_i64(uint8_t *w, int64_t v) {
    if (v < 0) *w++ = '-';
    const uint64_t a = origins_abs(v);
    return origins_put_u64(w, a, origins_digits(a));
}

// bytes of the line of pair id `g` of an item with these id and worker-number lengths
__host__ __device__ __forceinline__ uint32_t origins_line_len(uint32_t id_len, uint32_t cpu_len, uint64_t g, const OriginsSpan &o, int64_t isz) {
    return 3u * id_len + cpu_len + ORIGINS_FIXED + origins_digits((uint64_t)o.s1) + origins_digits((uint64_t)o.e1) +
           origins_digits((uint64_t)o.s2) + origins_digits((uint64_t)o.e2) + origins_digits(g) + origins_signed_len(isz);
}

// the line at w (origins_line_len bytes); returns the byte behind it.  `id`, `cpu`: id_len and cpu_len characters
__host__ __device__ __forceinline__ uint8_t *origins_put_line(uint8_t *w, const char *id, uint32_t id_len, const char *cpu, uint32_t cpu_len,
                                                              uint64_t g, const OriginsSpan &o, int64_t isz) {
    for (uint32_t k = 0; k < id_len; ++k) w[k] = (uint8_t)id[k];
    w += id_len;
    *w++ = '\t';
    w = origins_put_u64(w, (uint64_t)o.s1, origins_digits((uint64_t)o.s1));
    *w++ = '\t';
    w = origins_put_u64(w, (uint64_t)o.e1, origins_digits((uint64_t)o.e1));
    *w++ = '\t';
    for (uint32_t k = 0; k < id_len; ++k) w[k] = (uint8_t)id[k];
    w += id_len;
    *w++ = '\t';
    w = origins_put_u64(w, (uint64_t)o.s2, origins_digits((uint64_t)o.s2));
    *w++ = '\t';
    w = origins_put_u64(w, (uint64_t)o.e2, origins_digits((uint64_t)o.e2));
    *w++ = '\t';
    for (uint32_t k = 0; k < id_len; ++k) w[k] = (uint8_t)id[k];
    w += id_len;
    *w++ = '_';
    w = origins_put_u64(w, g, origins_digits(g));
    *w++ = '_';
    for (uint32_t k = 0; k < cpu_len; ++k) w[k] = (uint8_t)cpu[k];
    w += cpu_len;
    *w++ = '\t';
    *w++ = '.';
    *w++ = '\t';
    *w++ = '+';
    *w++ = '\t';
    *w++ = '-';
    *w++ = '\t';
    w = origins_put_i64(w, isz);
    *w++ = '\n';
    return w;
}

// the most bytes a line of an item can have: coordinates within [0, rec_len], the item's last pair id, isz an int32
inline uint64_t origins_line_bound(uint64_t id_len, uint64_t cpu_len, int64_t rec_len, uint64_t last_i) {
    return 3 * id_len + cpu_len + ORIGINS_FIXED + 4ull * origins_digits((uint64_t)rec_len) + origins_digits(last_i) + 11ull;
}
// bytes of LDS of a tile: its span at any alignment mod 16
inline uint32_t origins_region_bytes(uint64_t tile, uint64_t max_line) { return (uint32_t)(((tile * max_line + 15u) / 16u + 1u) * 16u); }
// pairs per workgroup for lines of at most max_line bytes (at least one: the caller bounds max_line)
inline int origins_tile_pairs(uint64_t max_line, int asked) {
    const size_t budget = asked > 0 ? ORIGINS_LDS_MAX : ORIGINS_LDS_BUDGET;
    int64_t t = asked > 0 ? asked : ORIGINS_MAX_TILE;
    t = std::min<int64_t>(t, (int64_t)((budget - 16) / max_line));
    return (int)std::max<int64_t>(t, 1);
}

struct OriginsArgs {
    const PairDesc *desc;      // descriptor of output row 0
    int64_t n_pairs;           // of all items
    int32_t RL, n_items;
    const OriginsItem *items;
    const char *ids;
    uint32_t *len;             // [n_pairs] bytes of every pair's line
    const uint64_t *off;       // [n_pairs] byte offset of every pair's line
    const uint64_t *total;     // bytes of the text
    uint8_t *text;
    uint64_t text_cap;
    int32_t tile;              // pairs per workgroup of k_origins_format
    uint32_t region;           // its bytes of LDS: origins_region_bytes(tile, the call's longest line)
    // rows of the last iss_generate_batch call, as in ExportArgs (iss_export.hip.h): output row row0 + r, 0 <= r < call_pairs, is
    // of the batch item k with item_first[k] <= r < item_first[k + 1]; its descriptor carries arena coordinates (batch[k].off)
    const BatchItem *batch;    // NULL: no such rows
    const int64_t *item_first;
    int32_t n_batch;
    int64_t row0, call_pairs;
};

// what both kernels know of a pair: its item, its pair id, the intervals, isz
struct OriginsPair {
    const OriginsItem *it;
    uint64_t g;
    OriginsSpan o;
    int64_t isz;
};

__device__ __forceinline__ OriginsPair origins_pair(const OriginsArgs &A, int64_t pair) {
    int lo = 0, hi = A.n_items;  // the item of the pair: largest k with rec_first[k] <= pair
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.items[mid].rec_first <= pair) lo = mid; else hi = mid;
    }
    OriginsPair P;
    P.it = A.items + lo;
    const int64_t i = pair - P.it->rec_first, row = P.it->first_pair + i;
    P.g = P.it->first_i + (uint64_t)i;
    int64_t off = 0;
    const int64_t r = row - A.row0;
    if (A.batch && r >= 0 && r < A.call_pairs) {
        int l2 = 0, h2 = A.n_batch;  // largest k with item_first[k] <= r (k_rows_export's search)
        while (h2 - l2 > 1) {
            const int mid = (l2 + h2) >> 1;
            if (A.item_first[mid] <= r) l2 = mid; else h2 = mid;
        }
        off = A.batch[l2].off;
    }
    const PairDesc d = A.desc[row];
    const int64_t fs = desc_fs(d) - off, re = desc_re(d) - off;
    P.o = origins_span(fs, re - (int64_t)A.RL, re, (int64_t)A.RL, P.it->rec_len);
    P.isz = d.isz;
    return P;
}

__global__ __launch_bounds__(ORIGINS_THREADS) void k_origins_len(const OriginsArgs A) {
    const int64_t stride = (int64_t)gridDim.x * ORIGINS_THREADS;
    for (int64_t pair = (int64_t)blockIdx.x * ORIGINS_THREADS + threadIdx.x; pair < A.n_pairs; pair += stride) {
        const OriginsPair P = origins_pair(A, pair);
        A.len[pair] = origins_line_len((uint32_t)P.it->id_len, (uint32_t)P.it->cpu_len, P.g, P.o, P.isz);
    }
}

// One workgroup per tile of `tile` consecutive pairs.  Their lines are one span [off[t0], off[t1]) of the text.  A lane composes
// the whole line of a pair at its place of the span's image in LDS; the image stands at the offset (the span's first address mod
// 16), so that the 16-byte chunks of LDS are the aligned 16-byte chunks of the text: the span goes out in aligned 16-byte stores,
// the bytes in front of the first and behind the last whole chunk one by one (a line has any length: a tile starts at every
// alignment, and the neighbour tile owns the other bytes of those two chunks).  Dynamic LDS: A.region bytes.
__global__ __launch_bounds__(ORIGINS_THREADS) void k_origins_format(const OriginsArgs A) {
    extern __shared__ uint4 origins_lds[];
    uint8_t *const lds = reinterpret_cast<uint8_t *>(origins_lds);
    const uint32_t tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * A.tile;
    if (t0 >= A.n_pairs) return;
    const int64_t t1 = min(t0 + (int64_t)A.tile, A.n_pairs);
    const uint32_t np = (uint32_t)(t1 - t0);
    const uint64_t first = A.off[t0], last = t1 < A.n_pairs ? A.off[t1] : *A.total;
    if (last > A.text_cap || last < first) return;  // (the host sized the text from a bound of every line: never)
    const uint32_t span = (uint32_t)(last - first);
    uint8_t *const g = A.text + first;
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u);
    if (a + span > A.region) return;  // (likewise: a line is never longer than its bound)
    uint8_t *const l = lds + a;
    for (uint32_t p = tid; p < np; p += ORIGINS_THREADS) {
        const int64_t pair = t0 + p;
        const OriginsPair P = origins_pair(A, pair);
        (void)origins_put_line(l + (uint32_t)(A.off[pair] - first), A.ids + P.it->id_off, (uint32_t)P.it->id_len, P.it->cpu,
                               (uint32_t)P.it->cpu_len, P.g, P.o, P.isz);
    }
    __syncthreads();
    const uint32_t head = min(span, (16u - a) & 15u);
    const uint32_t n16 = (span - head) >> 4;
    const uint32_t tail0 = head + (n16 << 4);
    for (uint32_t c = tid; c < n16; c += ORIGINS_THREADS)
        *reinterpret_cast<uint4 *>(g + head + (c << 4)) = *reinterpret_cast<const uint4 *>(l + head + (c << 4));
    if (tid < head) g[tid] = l[tid];
    if (tid >= 16u && tail0 + (tid - 16u) < span) g[tail0 + (tid - 16u)] = l[tail0 + (tid - 16u)];
}

}  // namespace iss
