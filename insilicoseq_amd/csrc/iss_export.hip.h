// iss_export.hip.h -- k_rows_export: output rows as dense arrays in the caller's device memory (iss_output_export): bases and
// phreds uint8 [n_pairs][2][read_length] (mate 1, then mate 2, no pitch padding), record coordinates int64 [n_pairs][4] and the
// work item of every pair.  Included by iss_mi355x.hip.
#pragma once

namespace iss {

constexpr int EXPORT_THREADS = 256;
constexpr int EXPORT_MAX_TILE = 64;               // pairs of a workgroup at most
constexpr size_t EXPORT_LDS_BUDGET = 48 * 1024;   // of the 160 KB of a CU: three workgroups and more per CU, no launch attribute
constexpr int32_t EXPORT_ASCII = 0, EXPORT_CODES = 1;  // (= ISS_EXPORT_* of the header)

struct ExportArgs {
    const uint8_t *rows;     // byte 0 of the first row
    const PairDesc *desc;    // the first row's descriptor
    int64_t n_pairs;
    int32_t RL, row;         // read length, bytes of a device row (DevModel::row)
    int32_t tile;            // pairs per workgroup
    uint32_t region;         // bytes of LDS per output array: export_region_bytes(tile, RL)
    int32_t encoding;
    uint8_t *bases, *qual;   // outputs; any of the four may be NULL
    int64_t *coords;
    int32_t *item;
    // rows of the last iss_generate_batch call: pair r of that call (r = rel0 + pair of this launch, 0 <= r < call_pairs) is of
    // the item k with item_first[k] <= r < item_first[k + 1], its descriptor carries arena coordinates (items[k].off)
    const BatchItem *items;  // NULL: no such rows
    const int64_t *item_first;
    int32_t n_items;
    int64_t rel0, call_pairs;
};

// ISS_EXPORT_CODES: A, C, G, T -> 0, 1, 2, 3 (alphabetical), either case; every other letter 4
__host__ __device__ __forceinline__ uint32_t export_code(uint32_t c) {
    const uint32_t u = c & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// pairs per workgroup: both output arrays of a tile in LDS within the budget (0: the read length is beyond this kernel)
__host__ __device__ inline uint32_t export_region_bytes(int tile, int RL) { return (((uint32_t)tile * 2u * (uint32_t)RL + 15u) / 16u + 1u) * 16u; }
inline int export_tile_pairs(int RL) {
    int t = (int)std::min<size_t>(EXPORT_MAX_TILE, (EXPORT_LDS_BUDGET - 64) / ((size_t)4 * (size_t)RL));
    while (t > 0 && 2 * (size_t)export_region_bytes(t, RL) > EXPORT_LDS_BUDGET) --t;
    return t;
}

// One workgroup per tile of `tile` pairs.  The tile's rows are one span of whole 128-byte lines: a lane loads 16-byte pieces
// [8 bases][8 phreds] (xp()), recodes the bases and puts both halves at their places of the tile's two dense images in LDS.  An
// image stands at the offset (its first global byte's address mod 16), so that the 16-byte chunks of LDS are the aligned 16-byte
// chunks of the output: the span goes out in aligned 16-byte stores, the bytes in front of the first and behind the last whole
// chunk one by one (an output row is 2 RL bytes: a tile starts at every alignment, and a neighbour tile owns the other bytes of
// those two chunks).
__global__ __launch_bounds__(EXPORT_THREADS) void k_rows_export(const ExportArgs E) {
    extern __shared__ uint4 export_lds[];
    uint8_t *const lds = reinterpret_cast<uint8_t *>(export_lds);
    const uint32_t tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * E.tile;
    if (tile0 >= E.n_pairs) return;
    const uint32_t np = (uint32_t)min((int64_t)E.tile, E.n_pairs - tile0);
    const uint32_t RL = (uint32_t)E.RL, out_row = 2u * RL, span = np * out_row;
    uint8_t *const gb = E.bases ? E.bases + tile0 * (int64_t)out_row : nullptr;
    uint8_t *const gq = E.qual ? E.qual + tile0 * (int64_t)out_row : nullptr;
    const uint32_t ab = (uint32_t)(reinterpret_cast<uintptr_t>(gb) & 15u), aq = (uint32_t)(reinterpret_cast<uintptr_t>(gq) & 15u);
    uint8_t *const lb = lds + ab, *const lq = lds + E.region + aq;
    if (gb || gq) {
        const uint32_t ppr = (uint32_t)E.row >> 4;  // pieces per row
        const uint32_t n_pieces = np * ppr;
        const uint4 *const src = reinterpret_cast<const uint4 *>(E.rows + tile0 * (int64_t)E.row);
        const bool codes = E.encoding == EXPORT_CODES;
        for (uint32_t i0 = tid; i0 < n_pieces; i0 += 4u * EXPORT_THREADS) {
            uint4 v[4];
            uint32_t dst[4], nv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // (the loads of four pieces in flight)
                const uint32_t idx = i0 + (uint32_t)u * EXPORT_THREADS;
                nv[u] = 0u;
                dst[u] = 0u;
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                if (idx < n_pieces) {
                    const uint32_t p = idx / ppr, q = idx - p * ppr;          // piece q of the row: line q / 8, mate (q / 4) % 2
                    const uint32_t pos = (((q >> 3) << 2) | (q & 3u)) << 3;  // its first read position
                    if (pos < RL) {  // (else: padding of the last line)
                        v[u] = src[idx];
                        dst[u] = p * out_row + ((q >> 2) & 1u) * RL + pos;
                        nv[u] = min(8u, RL - pos);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!nv[u]) continue;
                const uint64_t bw = (uint64_t)v[u].x | ((uint64_t)v[u].y << 32), qw = (uint64_t)v[u].z | ((uint64_t)v[u].w << 32);
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    if (j >= nv[u]) break;
                    const uint32_t b = (uint32_t)(bw >> (8u * j)) & 0xffu;
                    if (gb) lb[dst[u] + j] = (uint8_t)(codes ? export_code(b) : b);
                    if (gq) lq[dst[u] + j] = (uint8_t)(qw >> (8u * j));
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint8_t *const g = k ? gq : gb;
            if (!g) continue;
            const uint8_t *const l = k ? lq : lb;
            const uint32_t a = k ? aq : ab;
            const uint32_t head = min(span, (16u - a) & 15u);
            const uint32_t n16 = (span - head) >> 4;
            const uint32_t tail0 = head + (n16 << 4);
            for (uint32_t c = tid; c < n16; c += EXPORT_THREADS)
                *reinterpret_cast<uint4 *>(g + head + (c << 4)) = *reinterpret_cast<const uint4 *>(l + head + (c << 4));
            if (tid < head) g[tid] = l[tid];
            if (tid >= 16u && tail0 + (tid - 16u) < span) g[tail0 + (tid - 16u)] = l[tail0 + (tid - 16u)];
        }
    }
    if ((E.coords || E.item) && tid < np) {
        const int64_t pair = tile0 + tid;
        int64_t off = 0;
        int32_t k = 0;
        const int64_t r = E.rel0 + pair;
        if (E.items && r >= 0 && r < E.call_pairs) {
            int lo = 0, hi = E.n_items;  // largest k with item_first[k] <= r (items of no pairs are passed over)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (E.item_first[mid] <= r) lo = mid; else hi = mid;
            }
            k = lo;
            off = E.items[k].off;
        }
        if (E.item) E.item[pair] = k;
        if (E.coords) {  // (iss_output_download_coords)
            const PairDesc d = E.desc[pair];
            int64_t *const c = E.coords + 4 * pair;
            c[0] = desc_fs(d) - off;
            c[1] = desc_re(d) - off - (int64_t)RL;
            c[2] = desc_re(d) - off;
            c[3] = d.isz;
        }
    }
}

}  // namespace iss
