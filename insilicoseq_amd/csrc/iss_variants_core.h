// iss_variants_core.h -- `generate --variants`: the one mapping of a spliced record, "output offset o -> source offset | ALT offset",
// and its inverse for coordinates (the lift).  Plain C++ that compiles for the device (iss_variants.hip.h: k_variant_apply,
// k_variant_lift) and for the host (iss_variants_host_apply / iss_variants_host_lift, tools/variants_core_check.cpp drives them
// under a sanitizer).  DESIGN.md section 30.
//
// The tables of one record of L letters with n variants, sorted, disjoint (pos0[i + 1] >= pos0[i] + ref_len[i]; two pure insertions
// never share a pos0):
//     pos0[n]     first replaced letter of the record, 0-based           ref_len[n], alt_len[n]   letters replaced / put in
//     out_pos[n + 1]   where variant i's ALT run starts in the output: pos0[i] + sum over j < i of (alt_len[j] - ref_len[j]);
//                      out_pos[n] = L', the output's length
// Output offset o with i the LAST variant whose out_pos[i] <= o (none: the letter is src[o]) and k = o - out_pos[i]:
//     k <  alt_len[i]:  ALT letter alt_off[i] + k
//     k >= alt_len[i]:  src[pos0[i] + ref_len[i] + (k - alt_len[i])]
// (variants that put nothing in -- deletions -- may share an out_pos with the variant behind them: the last one decides.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISS_VAR_HD __host__ __device__ __forceinline__
#else
#define ISS_VAR_HD inline
#endif

namespace iss {
namespace var {

// The last i in [lo, n) with out_pos[i] <= o, or lo - 1 when there is none (lo = 0: -1).
ISS_VAR_HD int64_t var_find(const int64_t *out_pos, int64_t n, int64_t o, int64_t lo = 0) {
    int64_t hi = n;  // the answer + 1 lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (out_pos[mid] <= o) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// Where output offset o comes from, given i = var_find(out_pos, n, o): *from_alt says which blob the returned offset is into.
ISS_VAR_HD int64_t var_source(int64_t o, int64_t i, const int64_t *pos0, const int32_t *ref_len, const int32_t *alt_len,
                              const int64_t *alt_off, const int64_t *out_pos, bool *from_alt) {
    *from_alt = false;
    if (i < 0) return o;
    const int64_t k = o - out_pos[i], a = (int64_t)alt_len[i];
    if (k < a) {
        *from_alt = true;
        return alt_off[i] + k;
    }
    return pos0[i] + (int64_t)ref_len[i] + (k - a);
}

// Output coordinate h (0 .. L' inclusive: half-open interval ends) -> source coordinate.  Non-decreasing, lift(0) = 0 unless the
// record starts with an insertion's run (then its insertion point, 0 as well), lift(L') = L.  A coordinate inside an ALT run maps
// to pos0 + min(k, ref_len): an insertion's letters all map to the insertion point.
ISS_VAR_HD int64_t var_lift(int64_t h, int64_t n, const int64_t *pos0, const int32_t *ref_len, const int32_t *alt_len,
                            const int64_t *out_pos) {
    const int64_t i = var_find(out_pos, n, h);
    if (i < 0) return h;
    const int64_t k = h - out_pos[i], a = (int64_t)alt_len[i], r = (int64_t)ref_len[i];
    if (k < a) return pos0[i] + (k < r ? k : r);
    return pos0[i] + r + (k - a);
}

// Do the tables describe a splice of a record of L letters that reads nothing outside it and the two blobs?  0, or which rule
// fails: 1 a negative field, 2 a variant past the record's end, 3 order / overlap, 4 out_pos is not the running sum, 5 a blob
// range outside its blob.  *bad_at: the variant.  (alt_off / ref_off NULL: the lift's tables alone are checked.)
ISS_VAR_HD int var_tables_check(int64_t L, int64_t n, const int64_t *pos0, const int32_t *ref_len, const int32_t *alt_len,
                                const int64_t *alt_off, int64_t n_alt, const int64_t *ref_off, int64_t n_ref, const int64_t *out_pos,
                                int64_t *bad_at) {
    int64_t delta = 0, prev_end = 0;
    for (int64_t i = 0; i < n; ++i) {
        *bad_at = i;
        const int64_t p = pos0[i], r = (int64_t)ref_len[i], a = (int64_t)alt_len[i];
        if (p < 0 || r < 0 || a < 0 || (r == 0 && a == 0)) return 1;
        if (p > L || r > L - p) return 2;
        if (p < prev_end) return 3;
        if (i > 0 && r == 0 && ref_len[i - 1] == 0 && p == pos0[i - 1]) return 3;
        if (out_pos[i] != p + delta) return 4;
        if (alt_off && (alt_off[i] < 0 || alt_off[i] > n_alt || a > n_alt - alt_off[i])) return 5;
        if (ref_off && (ref_off[i] < 0 || ref_off[i] > n_ref || r > n_ref - ref_off[i])) return 5;
        delta += a - r;
        prev_end = p + r;
    }
    *bad_at = n;
    if (out_pos[n] != L + delta) return 4;
    return 0;
}

}  // namespace var
}  // namespace iss
