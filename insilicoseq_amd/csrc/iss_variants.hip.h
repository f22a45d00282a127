// iss_variants.hip.h -- `generate --variants`: a record's haplotype spliced together on the device, in front of k_pack_genome, and
// the coordinates of what was cut from it carried back to the record.  The mapping itself is
// iss_variants_core.h; the host restatement of these kernels is insilicoseq_amd/variants.py (VariantTable.apply_host, lift_host).
//   k_variant_check   one lane per variant: its REF letters against the record, case ignored
//   k_variant_apply   one workgroup per APPLY_TILE output bytes, 16 per lane, one 16-byte store each
//   k_variant_lift    one lane per coordinate
// None of them uses LDS.  256 lanes: four wavefronts, the block size of k_pack_genome behind them; 16 bytes per lane is the widest
// store there is, so a tile is 256 x 16 = 4096 output bytes.
#pragma once
#include "iss_variants_core.h"

namespace iss {

constexpr int VAR_THREADS = 256;
constexpr int VAR_LANE_BYTES = 16;
constexpr int64_t VAR_APPLY_TILE = (int64_t)VAR_THREADS * VAR_LANE_BYTES;

struct VarTables {  // device views of one record's tables (iss_variants_core.h); alt_off / alt: the apply alone
    int64_t n;
    const int64_t *pos0;
    const int32_t *ref_len, *alt_len;
    const int64_t *out_pos;  // [n + 1]
    const int64_t *alt_off;
    const uint8_t *alt;
};

__device__ __forceinline__ uint32_t var_upper(uint32_t c) { return c - (uint32_t)'a' < 26u ? c - 32u : c; }

// status[0] += variants whose REF letters differ from the record's (case ignored), status[1] = min(index of such a variant).
__global__ __launch_bounds__(VAR_THREADS) void k_variant_check(const uint8_t *__restrict__ src, int64_t n,
                                                               const int64_t *__restrict__ pos0, const int32_t *__restrict__ ref_len,
                                                               const int64_t *__restrict__ ref_off, const uint8_t *__restrict__ ref,
                                                               unsigned long long *status) {
    const int64_t i = (int64_t)blockIdx.x * VAR_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = src + pos0[i], *r = ref + ref_off[i];
    const int64_t len = (int64_t)ref_len[i];
    bool differ = false;
    for (int64_t k = 0; k < len && !differ; ++k) differ = var_upper(s[k]) != var_upper(r[k]);
    if (differ) {
        atomicAdd(&status[0], 1ull);
        atomicMin(&status[1], (unsigned long long)i);
    }
}

// dst[0 .. L') = the record `src` with the variants of T put in.  dst is 16-byte aligned (an allocation's start); the bytes of
// the last, partial 16 are stored one by one.  The reads of src and of the ALT blob are byte loads: their addresses have no
// alignment in common with the output's.
__global__ __launch_bounds__(VAR_THREADS) void k_variant_apply(const uint8_t *__restrict__ src, VarTables T, int64_t out_len,
                                                               uint8_t *__restrict__ dst) {
    const int64_t tile0 = (int64_t)blockIdx.x * VAR_APPLY_TILE;
    const int64_t o0 = tile0 + (int64_t)threadIdx.x * VAR_LANE_BYTES;
    if (o0 >= out_len) return;
    // the tile's variant (the same search in every lane: uniform), then on to the lane's own start
    int64_t i = var::var_find(T.out_pos, T.n, tile0);
    while (i + 1 < T.n && T.out_pos[i + 1] <= o0) ++i;
    const int64_t INF = (int64_t)1 << 62;
    int64_t next = i + 1 < T.n ? T.out_pos[i + 1] : INF;  // where the variant behind i takes over
    // the current piece: ALT letters for o in [alt_lo, alt_hi), source letters at o + src_shift behind them
    int64_t alt_lo = 0, alt_hi = 0, alt_at = 0, src_shift = 0;
    auto enter = [&](int64_t v) {
        const int64_t op = T.out_pos[v], a = (int64_t)T.alt_len[v];
        alt_lo = op;
        alt_hi = op + a;
        alt_at = T.alt_off[v];
        src_shift = T.pos0[v] + (int64_t)T.ref_len[v] - alt_hi;
    };
    if (i >= 0) enter(i);
    const int nb = (int)(out_len - o0 < VAR_LANE_BYTES ? out_len - o0 : VAR_LANE_BYTES);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int b = 0; b < nb; ++b) {
        const int64_t o = o0 + b;
        while (o >= next) {  // (variants that put nothing in may share an out_pos: the last one decides)
            ++i;
            next = i + 1 < T.n ? T.out_pos[i + 1] : INF;
            enter(i);
        }
        const uint32_t c = (o >= alt_lo && o < alt_hi) ? T.alt[alt_at + (o - alt_lo)] : src[o + src_shift];
        w[b >> 2] |= c << ((b & 3) * 8);
    }
    if (nb == VAR_LANE_BYTES) {
        *reinterpret_cast<uint4 *>(dst + o0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int b = 0; b < nb; ++b) dst[o0 + b] = (uint8_t)(w[b >> 2] >> ((b & 3) * 8));
    }
}

// out[t] = the record coordinate of haplotype coordinate in[t] of genome gids[t] (gids NULL: `gid` for all).  tabs[g].n == 0 (a
// genome without a table) and a genome id outside [0, n_tabs) are the identity.
struct VarLiftTab {
    int64_t n;
    const int64_t *pos0;
    const int32_t *ref_len, *alt_len;
    const int64_t *out_pos;
};
__global__ __launch_bounds__(VAR_THREADS) void k_variant_lift(const VarLiftTab *__restrict__ tabs, int32_t n_tabs,
                                                              const int32_t *__restrict__ gids, int32_t gid,
                                                              const int64_t *__restrict__ in, int64_t n, int64_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * VAR_THREADS + threadIdx.x;
    if (t >= n) return;
    const int32_t g = gids ? gids[t] : gid;
    const int64_t h = in[t];
    int64_t r = h;
    if (g >= 0 && g < n_tabs) {
        const VarLiftTab T = tabs[g];
        if (T.n > 0) r = var::var_lift(h, T.n, T.pos0, T.ref_len, T.alt_len, T.out_pos);
    }
    out[t] = r;
}

}  // namespace iss
