// iss_truth.hip.h -- the mutation rows of the last Philox generate call as dense arrays in the caller's device memory
// (iss_mutations_export): per-base truth for a consumer that stays on the GPU.
//   truth   uint8 [n_pairs][2][read_length]: the exported bases (k_rows_export, a second time), then k_truth_scatter puts the
//           `ref` letter of every substitution row that stays at its place
//   events  int32 [capacity][6] (pair - first_pair, mate, type, position, ref, alt) in the order of iss_mutations_download:
//           stages a and b of iss_vcf.hip.h order the rows per pair, k_truth_events writes the window's segments out
// Both kernels read the call's slot counter themselves: a call that asked for more slots than were reserved has no row that
// can be trusted, and that is decided here, on the device (no kernel of this file is launched behind a wait on the host).
// Included by iss_mi355x.hip.
#pragma once
#include "iss_vcf.hip.h"     // mut_row_stays
#include "iss_export.hip.h"  // export_code

namespace iss {

struct TruthArgs {
    const MutRecord *mut;     // the reserved slots
    const uint32_t *count;    // slots the call asked for (more than `cap`: the buffer overflowed)
    uint32_t cap;             // slots reserved
    const uint32_t *flags;    // the call's flag words (which mates the fix-up rebuilt)
    int64_t call_pairs;       // pairs of the generate call
    int64_t rel0, n_pairs;    // the window: pairs [rel0, rel0 + n_pairs) of the call (it may reach over either end)
    int32_t RL, encoding;
    uint8_t *truth;           // k_truth_scatter
    // k_truth_events: the window's rows are the rows [seg[w0], seg[w1]) of `order` (w0 <= w1: the window cut to the call's pairs)
    const uint64_t *seg;      // NULL: the window holds no pair of the call
    const uint32_t *order;
    int64_t w0, w1;
    int32_t *events;
    int64_t capacity;
    int64_t *n_events;
};

constexpr int TRUTH_THREADS = 256;

// Grid-stride over the slots the call used, one lane per slot: a substitution row that stays and lies in the window writes its
// `ref` letter over the base k_rows_export put there.  No order and no atomics: the rows that stay are those of ONE pass of
// mut_sequence over the read as it came out (k_main's, or the fix-up's where it rebuilt the mate -- never both, that is the
// filter), and mut_sequence visits each position once (iss/error_models/__init__.py:93-110): a byte of `truth` has one writer
// at most.
__global__ __launch_bounds__(TRUTH_THREADS) void k_truth_scatter(const TruthArgs T) {
    const uint32_t used = *T.count;
    if (used > T.cap) return;  // overflow: `truth` stays the plain bases
    const bool codes = T.encoding == EXPORT_CODES;
    for (uint64_t i = (uint64_t)blockIdx.x * TRUTH_THREADS + threadIdx.x; i < used; i += (uint64_t)gridDim.x * TRUTH_THREADS) {
        const MutRecord r = T.mut[i];
        if (!mut_row_stays(r, T.call_pairs, T.flags) || ((uint8_t)r.type & 3) != 0) continue;
        const int64_t w = (int64_t)r.pair - T.rel0;
        if (w < 0 || w >= T.n_pairs || (uint32_t)(int32_t)r.position >= (uint32_t)T.RL) continue;
        const uint32_t c = r.ref;
        T.truth[(2 * w + (r.mate & 1)) * (int64_t)T.RL + r.position] = (uint8_t)(codes ? export_code(c) : c);
    }
}

// One lane per row of the window, in the order stages a and b left in `order`; lane 0 of the grid writes the count.
__global__ __launch_bounds__(TRUTH_THREADS) void k_truth_events(const TruthArgs T) {
    const bool overflow = *T.count > T.cap;
    const uint64_t lo = T.seg ? T.seg[T.w0] : 0, hi = T.seg ? T.seg[T.w1] : 0;
    const uint64_t g = (uint64_t)blockIdx.x * TRUTH_THREADS + threadIdx.x;
    if (g == 0) *T.n_events = overflow ? (int64_t)-1 : (int64_t)(hi - lo);
    if (overflow) return;
    const uint64_t n = min(hi - lo, (uint64_t)T.capacity);
    for (uint64_t j = g; j < n; j += (uint64_t)gridDim.x * TRUTH_THREADS) {
        const uint32_t s = T.order[lo + j];
        if (s >= T.cap) continue;  // (cannot happen: k_vcf_rank filled every place of the segments)
        const MutRecord r = T.mut[s];
        int32_t *const e = T.events + 6 * j;
        e[0] = (int32_t)((int64_t)r.pair - T.rel0);
        e[1] = r.mate & 1;
        e[2] = (uint8_t)r.type & 3;
        e[3] = r.position;
        e[4] = r.ref;
        e[5] = r.alt;
    }
}

}  // namespace iss
