// iss_depth.hip.h -- per-base coverage depth of the generated reads on the device (iss_depth_mark, iss_depth_finish).
//   k_depth_mark        one lane per pair: +1 / -1 at the ends of the pair's two template intervals in the caller's int32
//                       difference array (global atomic adds without return)
//   k_depth_table_prep  one workgroup over the record table: the rows in use (offset >= 0) compacted, every row's first window
//   k_depth_clear       zeroes the statistics and the window sums (their number is known on the device only)
//   k_depth_tile_sums   the sum of every tile of DEPTH_TILE words         \  reduce-then-scan inclusive prefix sum of the
//   k_depth_scan_tiles  one workgroup: exclusive scan of the tile sums     > difference array = the depth of every base of
//   k_depth_apply       the prefix of a tile's words + statistics + bins  /  every record at once (the sinks make it unsegmented)
// All arithmetic is exact integers: the results depend neither on the launch geometry nor on the order of arrival.  The prefix
// is computed in wrapping u32 arithmetic; it is exact because every prefix lies in [0, 2^31) (the caller's bound).
// DESIGN.md section 19.  Included by iss_mi355x.hip.
#pragma once

namespace iss {

constexpr int DEPTH_THREADS = 256;
constexpr int DEPTH_TILE = 4096;            // words of a tile (= ISS_DEPTH_TILE_WORDS): 16 per lane, four 16-byte pieces
constexpr int DEPTH_PASS = 4 * DEPTH_THREADS;  // words of one pass of the workgroup over its tile: lane t holds words 4 t .. 4 t + 3
constexpr int DEPTH_TARGET_WGS = 2048;      // workgroups of a launch, about: 8 per compute unit
constexpr uint32_t DEPTH_BINS_LDS_SMALL = 1024, DEPTH_BINS_LDS_LARGE = DEPTH_TILE + 1;  // window sums of a tile kept in LDS

// ---------------------------------------------------------------------------------------------------- mark
struct DepthMarkArgs {
    const PairDesc *desc;    // the window's first descriptor
    int64_t n_pairs;
    int32_t RL;
    const int64_t *table;    // [n_table][2]: (offset, length) of the record of item k
    int32_t n_table;
    int32_t *diff;
    // rows of the last iss_generate_batch call, as in ExportArgs (iss_export.hip.h)
    const BatchItem *items;  // NULL: no such rows
    const int64_t *item_first;
    int32_t n_items;
    int64_t rel0, call_pairs;
};

__host__ __device__ __forceinline__ int64_t depth_clamp(int64_t x, int64_t len) { return x < 0 ? 0 : (x > len ? len : x); }

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_mark(const DepthMarkArgs A) {
    const int64_t stride = (int64_t)gridDim.x * DEPTH_THREADS;
    for (int64_t pair = (int64_t)blockIdx.x * DEPTH_THREADS + threadIdx.x; pair < A.n_pairs; pair += stride) {
        int64_t off = 0;
        int32_t k = 0;
        const int64_t r = A.rel0 + pair;
        if (A.items && r >= 0 && r < A.call_pairs) {
            int lo = 0, hi = A.n_items;  // largest k with item_first[k] <= r (k_rows_export's search)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (A.item_first[mid] <= r) lo = mid; else hi = mid;
            }
            k = lo;
            off = A.items[k].off;
        }
        if (k >= A.n_table) continue;  // (the host has refused such a call)
        const int64_t t_off = A.table[2 * (int64_t)k], len = A.table[2 * (int64_t)k + 1];
        if (t_off < 0 || len < 1) continue;
        const PairDesc d = A.desc[pair];
        const int64_t fs = desc_fs(d) - off, re = desc_re(d) - off;
        const int64_t s0 = depth_clamp(fs, len), e0 = depth_clamp(fs + A.RL, len);
        const int64_t s1 = depth_clamp(re - A.RL, len), e1 = depth_clamp(re, len);
        int32_t *const w = A.diff + t_off;
        if (s0 < e0) {
            (void)__hip_atomic_fetch_add(w + s0, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(w + e0, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (s1 < e1) {
            (void)__hip_atomic_fetch_add(w + s1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(w + e1, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- finish
// The launch geometry and the work array of a finish call (host).  The work array, in this order: tile sums u32 [n_tiles + 1]
// (padded to 8 bytes), info i64 [2] (rows in use, windows of all rows), first i64 [n_table + 1] (a row's first window), idx i32
// [n_table] (the rows in use, in table order).
struct DepthPlan {
    int64_t n_tiles;
    uint32_t grid;           // workgroups of k_depth_tile_sums and k_depth_apply
    uint32_t bins_lds;       // window sums a workgroup keeps in LDS (0: no windows)
    size_t off_info, off_first, off_idx, bytes;
};
inline bool depth_plan(int64_t n_words, int32_t n_table, int32_t bin, int wgs, DepthPlan *out) {
    if (n_words < 1 || n_table < 0 || bin < 0) return false;
    DepthPlan p;
    p.n_tiles = (n_words + DEPTH_TILE - 1) / DEPTH_TILE;
    if (p.n_tiles > ((int64_t)1 << 40)) return false;
    const int64_t target = wgs > 0 ? wgs : DEPTH_TARGET_WGS;
    p.grid = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p.n_tiles, target), 0x7fffffff));
    p.bins_lds = bin == 0 ? 0u : (bin >= 8 ? DEPTH_BINS_LDS_SMALL : DEPTH_BINS_LDS_LARGE);
    p.off_info = (((size_t)p.n_tiles + 1) * 4 + 7) / 8 * 8;
    p.off_first = p.off_info + 16;
    p.off_idx = p.off_first + ((size_t)n_table + 1) * 8;
    p.bytes = p.off_idx + ((size_t)n_table + 1) * 4;
    *out = p;
    return true;
}

struct DepthFinishArgs {
    const int32_t *diff;
    int64_t n_words;
    uint32_t *depth;           // NULL: statistics only; may be `diff` itself
    const int64_t *table;
    int32_t n_table, bin;
    unsigned long long *stats;  // [n_table][4] or NULL
    unsigned long long *bins;   // or NULL (always NULL when bin == 0)
    uint32_t *tiles;            // work array: see DepthPlan
    int64_t n_tiles;
    int64_t *info, *first;
    int32_t *idx;
    uint32_t bins_lds;
    int32_t vec;                // diff (and depth, if any) are 16-byte aligned: 16-byte loads and stores
};

// inclusive scan over the workgroup's 256 values (Hillis-Steele in LDS; the cold kernels)
template <typename T>
__device__ __forceinline__ T depth_wg_scan(T x, T *lds) {
    const uint32_t tid = threadIdx.x;
    lds[tid] = x;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < (uint32_t)DEPTH_THREADS; d <<= 1) {
        const T y = tid >= d ? lds[tid - d] : (T)0;
        __syncthreads();
        lds[tid] += y;
        __syncthreads();
    }
    const T r = lds[tid];
    __syncthreads();
    return r;
}

// a / b for 0 <= a < 2^52 (depth_plan's limit on n_words), 0 < b < 2^31, without a 64-bit integer division: the quotient of the
// two as doubles (both exact) is the true one or a neighbour of it, and one step either way settles it.  (hipcc expands a 64-bit
// division with a workgroup-uniform operand into scalar code that materialises carries with s_cselect, which tools/scan_isa.py
// cannot tell from the stale-SCC select it guards against.)
__device__ __forceinline__ int64_t depth_div(int64_t a, int32_t b) {
    int64_t q = (int64_t)((double)a / (double)b);
    const int64_t r = a - q * (int64_t)b;
    if (r < 0) --q; else if (r >= (int64_t)b) ++q;
    return q;
}

// A row is in use with offset >= 0 and length >= 1.  Row k owns ceil(length_k / bin) windows whether in use or not (the layout
// of d_bins is a function of the lengths alone); first[k] = the windows of the rows before it.
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_table_prep(const DepthFinishArgs A) {
    __shared__ int64_t s_w[DEPTH_THREADS];
    __shared__ int32_t s_v[DEPTH_THREADS];
    __shared__ int64_t s_tw;
    __shared__ int32_t s_tv;
    const uint32_t tid = threadIdx.x;
    int64_t windows = 0;
    int32_t used = 0;
    for (int64_t k0 = 0; k0 < A.n_table; k0 += DEPTH_THREADS) {
        const int64_t k = k0 + tid;
        int64_t nw = 0;
        int32_t v = 0;
        if (k < A.n_table) {
            const int64_t off = A.table[2 * k], len = A.table[2 * k + 1];
            v = off >= 0 && len >= 1;
            if (A.bin > 0 && len >= 1) nw = depth_div(len + A.bin - 1, A.bin);
        }
        const int64_t iw = depth_wg_scan<int64_t>(nw, s_w);
        const int32_t iv = depth_wg_scan<int32_t>(v, s_v);
        if (k < A.n_table) {
            A.first[k] = windows + iw - nw;
            if (v) A.idx[used + iv - 1] = (int32_t)k;
        }
        if (tid == DEPTH_THREADS - 1) { s_tw = iw; s_tv = iv; }
        __syncthreads();
        windows += s_tw;
        used += s_tv;
        __syncthreads();
    }
    if (tid == 0) {
        A.first[A.n_table] = windows;
        A.info[0] = used;
        A.info[1] = windows;
    }
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_clear(const DepthFinishArgs A) {
    const int64_t stride = (int64_t)gridDim.x * DEPTH_THREADS, t0 = (int64_t)blockIdx.x * DEPTH_THREADS + threadIdx.x;
    if (A.stats) for (int64_t i = t0; i < 4 * (int64_t)A.n_table; i += stride) A.stats[i] = 0ull;
    if (A.bins) { const int64_t n = A.info[1]; for (int64_t i = t0; i < n; i += stride) A.bins[i] = 0ull; }
}

// the four words from word w0 on (those at or past n_words: 0)
__device__ __forceinline__ void depth_load4(const DepthFinishArgs &A, int64_t w0, uint32_t v[4]) {
    if (A.vec && w0 + 4 <= A.n_words) {
        const uint4 q = *reinterpret_cast<const uint4 *>(A.diff + w0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = w0 + i < A.n_words ? (uint32_t)A.diff[w0 + i] : 0u;
    }
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_tile_sums(const DepthFinishArgs A) {
    __shared__ uint32_t s_sum[DEPTH_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < A.n_tiles; t += gridDim.x) {
        const int64_t tile0 = t * DEPTH_TILE;
        uint32_t s = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t v[4];
            depth_load4(A, tile0 + j * DEPTH_PASS + 4 * (int64_t)tid, v);
            s += v[0] + v[1] + v[2] + v[3];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if ((tid & 63u) == 0u) s_sum[tid >> 6] = s;
        __syncthreads();
        if (tid == 0u) A.tiles[t] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        __syncthreads();
    }
}

// tiles[t] <- the sum of the tiles before t, in place; one workgroup, a chunk of 256 tiles a turn
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_scan_tiles(const DepthFinishArgs A) {
    __shared__ uint32_t s_x[DEPTH_THREADS];
    __shared__ uint32_t s_total;
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0u;
    for (int64_t t0 = 0; t0 < A.n_tiles; t0 += DEPTH_THREADS) {
        const int64_t t = t0 + tid;
        const uint32_t x = t < A.n_tiles ? A.tiles[t] : 0u;
        const uint32_t incl = depth_wg_scan<uint32_t>(x, s_x);
        if (t < A.n_tiles) A.tiles[t] = carry + incl - x;
        if (tid == DEPTH_THREADS - 1) s_total = incl;
        __syncthreads();
        carry += s_total;
        __syncthreads();
    }
    if (tid == 0u) A.tiles[A.n_tiles] = carry;
}

// the record cursor of a lane: row idx[j] of the table, the j-th row in use (j == -1: in front of the first)
struct DepthCursor {
    int64_t j, off, len, first, next_off;  // next_off: offset of row idx[j + 1] (INT64_MAX: none)
    int32_t k;
};
__device__ __forceinline__ void depth_cursor_load(const DepthFinishArgs &A, int64_t n_used, int64_t j, DepthCursor &c) {
    c.j = j;
    if (j >= 0) {
        c.k = A.idx[j];
        c.off = A.table[2 * (int64_t)c.k];
        c.len = A.table[2 * (int64_t)c.k + 1];
        c.first = A.first[c.k];
    } else {
        c.k = -1; c.off = 0; c.len = 0; c.first = 0;
    }
    c.next_off = j + 1 < n_used ? A.table[2 * (int64_t)A.idx[j + 1]] : INT64_MAX;
}
// largest j in [lo, hi] with offset(idx[j]) <= w; lo may be -1 (none); offsets of the rows in use ascend
__device__ __forceinline__ int64_t depth_find(const DepthFinishArgs &A, int64_t w, int64_t lo, int64_t hi) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (A.table[2 * (int64_t)A.idx[mid]] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void depth_add_window(const DepthFinishArgs &A, unsigned long long *s_bins, int64_t g0, int64_t g, unsigned long long x) {
    if (!x) return;
    const int64_t gi = g - g0;
    if (gi >= 0 && gi < (int64_t)A.bins_lds) atomicAdd(&s_bins[gi], x);
    else atomicAdd(&A.bins[g], x);
}
__device__ __forceinline__ void depth_add_stats(unsigned long long *st, unsigned long long sum, unsigned long long sq, unsigned long long cov, unsigned long long mx) {
    if (!cov) return;  // (no base with depth > 0: nothing to add)
    atomicAdd(&st[0], sum);
    atomicAdd(&st[1], sq);
    atomicAdd(&st[2], cov);
    atomicMax(&st[3], mx);
}

// One tile a turn.  Lane t holds words 4 t .. 4 t + 3 of each of the tile's four passes (16-byte loads and stores, a wave
// instruction = 1 KB in a row); the scan runs over (pass, lane) in that order: a wave scan per pass by shuffles, the 16 wave totals
// through LDS, in front of them the tile's prefix from k_depth_scan_tiles.  Statistics: a lane finds the record of each of its four
// 4-word pieces by bisection among the rows the tile touches and walks on.  What falls to the record of the tile's first word is
// summed in registers and over the workgroup (one set of atomics per tile); what falls to another record leaves the lane as
// atomics per run.  Window sums gather in LDS (u64, indexed from the tile's first window) and leave once per tile, one atomic per
// non-zero window; a window outside the LDS range goes straight to memory.
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_apply(const DepthFinishArgs A) {
    extern __shared__ unsigned long long depth_lds_[];
    unsigned long long *const s_bins = depth_lds_;
    __shared__ uint32_t s_w[16];
    __shared__ unsigned long long s_red[4][DEPTH_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool want_stats = A.stats != nullptr, want_bins = A.bins != nullptr;
    const int64_t n_used = (want_stats || want_bins) ? A.info[0] : 0;
    for (uint32_t i = tid; i < A.bins_lds; i += DEPTH_THREADS) s_bins[i] = 0ull;
    __syncthreads();
    for (int64_t t = blockIdx.x; t < A.n_tiles; t += gridDim.x) {
        const int64_t tile0 = t * DEPTH_TILE;
        uint32_t v[4][4], s[4], incl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            depth_load4(A, tile0 + j * DEPTH_PASS + 4 * (int64_t)tid, v[j]);
            s[j] = v[j][0] + v[j][1] + v[j][2] + v[j][3];
            uint32_t x = s[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d);
                if (lane >= (uint32_t)d) x += y;
            }
            incl[j] = x;
            if (lane == 63u) s_w[j * 4 + (int)wave] = x;
        }
        __syncthreads();
        const uint32_t base = A.tiles[t];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t run = base + incl[j] - s[j];
            for (uint32_t i = 0; i < (uint32_t)j * 4u + wave; ++i) run += s_w[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) { run += v[j][i]; v[j][i] = run; }
            if (A.depth) {
                const int64_t w0 = tile0 + j * DEPTH_PASS + 4 * (int64_t)tid;
                if (A.vec && w0 + 4 <= A.n_words) {
                    *reinterpret_cast<uint4 *>(A.depth + w0) = make_uint4(v[j][0], v[j][1], v[j][2], v[j][3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (w0 + i < A.n_words) A.depth[w0 + i] = v[j][i];
                }
            }
        }
        if (want_stats || want_bins) {
            // the rows the tile touches: [jlo, jhi] (uniform over the workgroup), the tile's first window g0 and its last
            // (an equality on the tile number, not a 64-bit min: deflate_block_len() in iss_deflate.hip.h says why)
            const int64_t tile_last = tile0 + (t == A.n_tiles - 1 ? (int64_t)(uint32_t)(A.n_words - tile0) : (int64_t)DEPTH_TILE) - 1;
            const int64_t jlo = depth_find(A, tile0, -1, n_used - 1), jhi = depth_find(A, tile_last, jlo, n_used - 1);
            DepthCursor c0;
            depth_cursor_load(A, n_used, jlo >= 0 ? jlo : (n_used > 0 ? 0 : -1), c0);
            const int32_t k0 = c0.k;
            int64_t g0 = 0, g_last = -1;
            if (want_bins) {
                g0 = c0.first + (jlo >= 0 ? depth_div(min(tile0 - c0.off, c0.len), A.bin) : 0);
                if (jhi >= 0) {
                    DepthCursor c1;
                    depth_cursor_load(A, n_used, jhi, c1);
                    g_last = c1.first + depth_div(min(tile_last - c1.off, c1.len), A.bin);
                }
            }
            unsigned long long a_sum = 0ull, a_sq = 0ull;  // the share of row k0
            uint32_t a_cov = 0u, a_max = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // (unrolled: v[][] stays in registers)
                const int64_t w0 = tile0 + j * DEPTH_PASS + 4 * (int64_t)tid;
                if (w0 >= A.n_words) break;
                DepthCursor c;
                depth_cursor_load(A, n_used, depth_find(A, w0, jlo, jhi), c);
                unsigned long long r_sum = 0ull, r_sq = 0ull, b_sum = 0ull;  // the run of a row other than k0; of a window
                uint32_t r_cov = 0u, r_max = 0u;
                int64_t win = -1;  // window of the row the run stands in (-1: not worked out)
                int32_t rem = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t w = w0 + i;
                    if (w >= A.n_words) break;
                    if (w >= c.next_off) {  // the next row in use begins (the rows ascend: one step, then whatever the table says)
                        if (want_stats && c.k >= 0) depth_add_stats(A.stats + 4 * (int64_t)c.k, r_sum, r_sq, r_cov, r_max);
                        if (want_bins && win >= 0) depth_add_window(A, s_bins, g0, c.first + win, b_sum);
                        r_sum = r_sq = b_sum = 0ull; r_cov = r_max = 0u; win = -1;
                        int64_t jn = c.j + 1;
                        while (jn + 1 < n_used && A.table[2 * (int64_t)A.idx[jn + 1]] <= w) ++jn;
                        depth_cursor_load(A, n_used, jn, c);
                    }
                    const int64_t pos = w - c.off;
                    if (c.k < 0 || pos < 0 || pos >= c.len) continue;  // a sink, a gap between records, words in front of the first
                    const uint32_t d = v[j][i];
                    if (want_stats) {
                        if (c.k == k0) {
                            a_sum += d; a_sq += (unsigned long long)d * d; a_cov += d > 0u; a_max = max(a_max, d);
                        } else {
                            r_sum += d; r_sq += (unsigned long long)d * d; r_cov += d > 0u; r_max = max(r_max, d);
                        }
                    }
                    if (want_bins) {
                        if (win < 0) {
                            win = pos ? depth_div(pos, A.bin) : 0;
                            rem = (int32_t)(pos - win * A.bin);
                        }
                        b_sum += d;
                        if (++rem == A.bin) {
                            depth_add_window(A, s_bins, g0, c.first + win, b_sum);
                            b_sum = 0ull; rem = 0; ++win;
                        }
                    }
                }
                if (want_stats && c.k >= 0 && c.k != k0) depth_add_stats(A.stats + 4 * (int64_t)c.k, r_sum, r_sq, r_cov, r_max);
                if (want_bins && win >= 0) depth_add_window(A, s_bins, g0, c.first + win, b_sum);
            }
            if (want_stats) {
                unsigned long long cov = a_cov, mx = a_max;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    a_sum += __shfl_xor(a_sum, d);
                    a_sq += __shfl_xor(a_sq, d);
                    cov += __shfl_xor(cov, d);
                    const unsigned long long o = __shfl_xor(mx, d);
                    mx = o > mx ? o : mx;
                }
                if (lane == 0u) { s_red[0][wave] = a_sum; s_red[1][wave] = a_sq; s_red[2][wave] = cov; s_red[3][wave] = mx; }
            }
            __syncthreads();
            if (want_stats && tid == 0u && k0 >= 0) {
                unsigned long long mx = 0ull;
                for (int i = 0; i < DEPTH_THREADS / 64; ++i) mx = s_red[3][i] > mx ? s_red[3][i] : mx;
                depth_add_stats(A.stats + 4 * (int64_t)k0, s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3],
                                s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3], s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3], mx);
            }
            if (want_bins) {
                const int64_t n_lds = min((int64_t)A.bins_lds, g_last - g0 + 1);
                for (int64_t i = tid; i < n_lds; i += DEPTH_THREADS) {
                    const unsigned long long x = s_bins[i];
                    if (x) { atomicAdd(&A.bins[g0 + i], x); s_bins[i] = 0ull; }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace iss
