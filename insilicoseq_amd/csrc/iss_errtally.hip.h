// iss_errtally.hip.h -- k_errtally_rows, k_errtally_reads: integer tallies over the mutation rows of the last generate call
// (iss_mutations_tally): what the run did to the reads.  One flat u64 array in the caller's device memory, added to
// (include/iss_mi355x.h has the layout):
//   dropped [1] | pairs [1] | sub_q [2][L][94] | sub_mat [2][L][5][5] | ins [2][L][5] | del [2][L][5] | per_read [2][3][64]
// Every count is an exact integer sum: the result depends neither on the launch geometry nor on the order of arrival.
// Counts are gathered in LDS (u32) and added to the u64 words once per workgroup, one global atomic per non-zero counter (the
// pattern of iss_tally.hip.h).  Both kernels read the call's slot counter themselves, like k_truth_scatter: a call that asked
// for more slots than were reserved has no row that can be trusted -- it adds 1 to `dropped` and nothing else.
// DESIGN.md section 23.  Included by iss_mi355x.hip.
#pragma once
#include "iss_vcf.hip.h"     // mut_row_stays
#include "iss_export.hip.h"  // export_code

namespace iss {

constexpr int ERRTALLY_THREADS = 256;
constexpr int ERRTALLY_NQ = 94;             // phred 0 .. 93 (= ISS_ERRTALLY_PHREDS); a larger quality counts in bin 93
constexpr int ERRTALLY_NK = 64;             // (= ISS_ERRTALLY_READ_BINS)
constexpr int ERRTALLY_TILE = 32;           // positions of a workgroup's tables
constexpr int ERRTALLY_QPITCH = 95;         // LDS words per (mate, position) of the sub_q table: odd, like TALLY_QPITCH -- lanes that
                                            // stand at different (mate, position) with the same phred fall into different banks
constexpr int ERRTALLY_SLOT_WORDS = ERRTALLY_QPITCH + 25 + 5 + 5;  // 130: the counters of one (mate, position)
constexpr int ERRTALLY_LDS_WORDS = 2 * ERRTALLY_TILE * ERRTALLY_SLOT_WORDS;  // 8 320 words, 33 280 bytes
constexpr int ERRTALLY_TARGET_WGS = 2048;   // workgroups of a launch, about: 8 per compute unit
constexpr int ERRTALLY_WG_SLOTS = 8192;     // slots a workgroup of k_errtally_rows should at least have to walk (32 per lane)
constexpr int64_t ERRTALLY_MAX_SLOTS = 0x7fffffff;          // slots of a call at most: what a u32 LDS counter holds, see below
constexpr int64_t ERRTALLY_MAX_WG_PAIRS = (int64_t)1 << 30;  // pairs of a k_errtally_reads workgroup at most, likewise
// the work array: one u64 per read (pair - first_pair, mate), three 21-bit counters (substitution, insertion, deletion rows).
// A read has at most one substitution, four insertion and one deletion row per loop step (iss/error_models/__init__.py:93-110,
// 187-222; the four insertion slots of MutRecord::type) and at most 1 024 steps (FIX_MAX_RL): 4 096 < 2^21, no counter reaches
// its neighbour.
constexpr int ERRTALLY_CNT_BITS = 21;

struct ErrTallyLayout {  // word offsets of the fields for read length L
    int64_t dropped, pairs, sub_q, sub_mat, ins, del, per_read, words;
};
__host__ __device__ inline ErrTallyLayout errtally_layout(int L) {
    ErrTallyLayout t;
    t.dropped = 0;
    t.pairs = 1;
    t.sub_q = 2;
    t.sub_mat = t.sub_q + 2 * (int64_t)L * ERRTALLY_NQ;
    t.ins = t.sub_mat + 2 * (int64_t)L * 25;
    t.del = t.ins + 2 * (int64_t)L * 5;
    t.per_read = t.del + 2 * (int64_t)L * 5;
    t.words = t.per_read + 2 * 3 * ERRTALLY_NK;
    return t;
}

struct ErrTallyArgs {
    const MutRecord *mut;     // source 0: the reserved slots; source 1: the rows
    const uint32_t *count;    // source 0: slots the call asked for (more than `cap`: the buffer overflowed); NULL: `used`
    uint32_t cap;             // slots reserved
    uint32_t used;            // source 1: rows of the call (the host has checked them against the reservation)
    const uint32_t *flags;    // source 0: the call's flag words (which mates the fix-up rebuilt); NULL: every used row stays
    int64_t call_pairs;       // pairs of the generate call (source 0)
    int64_t rel0, n_pairs;    // the window: pairs [rel0, rel0 + n_pairs) of the call (it may reach over either end)
    int32_t RL;
    int64_t read_per;         // k_errtally_reads: pairs of a workgroup
    unsigned long long *reads;  // the work array [n_pairs][2]
    unsigned long long *tally;
};

__device__ __forceinline__ uint32_t errtally_used(const ErrTallyArgs &T) { return T.count ? *T.count : T.used; }

// The per-position tables.  Workgroup (t, c) owns the positions 32 t .. 32 t + 31 of both mates and walks the used slots
// grid-stride with the workgroups (t, *) of its column: slot i belongs to lane i % 256 of workgroup (i / 256) % gridDim.y.  A row
// is read as one 12-byte record (k_vcf_count); it counts when it stays (mut_row_stays), lies in the window and has its position
// -- clamped to [0, L - 1] -- in the tile.  LDS holds 64 (mate, position) x 130 u32 counters; a workgroup adds to a counter at
// most once per slot it walks, and a call has fewer than 2^31 slots (ERRTALLY_MAX_SLOTS, checked on the host): no counter wraps.
// Lanes of one wave that meet at a word: a wave holds 64 consecutive slots, of which one tile keeps about a fifth, spread over
// 64 (mate, position); the odd pitch keeps equal phreds of different positions in different banks, and what still meets at one
// word is serialised by the LDS atomic unit -- a few adds per wave instruction at most, next to the 768 bytes the wave loaded.
// The workgroups of column 0 also count every kept row of the window for its read: one u64 global add to the work array.
__global__ __launch_bounds__(ERRTALLY_THREADS) void k_errtally_rows(const ErrTallyArgs T) {
    __shared__ uint32_t s_cnt[ERRTALLY_LDS_WORDS];
    const uint32_t tid = threadIdx.x;
    const uint32_t used = errtally_used(T);
    if (used > T.cap) return;  // overflow: k_errtally_reads says so
    for (uint32_t i = tid; i < (uint32_t)ERRTALLY_LDS_WORDS; i += ERRTALLY_THREADS) s_cnt[i] = 0u;
    __syncthreads();
    const int32_t RL = T.RL, tile = (int32_t)blockIdx.x;
    const bool reads_too = blockIdx.x == 0;
    for (uint64_t i = (uint64_t)blockIdx.y * ERRTALLY_THREADS + tid; i < used; i += (uint64_t)gridDim.y * ERRTALLY_THREADS) {
        const MutRecord r = T.mut[i];
        if (T.flags ? !mut_row_stays(r, T.call_pairs, T.flags) : r.pair < 0) continue;
        const int64_t w = (int64_t)r.pair - T.rel0;
        if (w < 0 || w >= T.n_pairs) continue;
        const uint32_t mate = (uint32_t)r.mate & 1u, type = (uint8_t)r.type & 3u;
        if (type > 2u) continue;  // (no such row is written)
        if (reads_too) atomicAdd(&T.reads[2 * w + mate], 1ull << (ERRTALLY_CNT_BITS * type));
        const int32_t pos = min(max((int32_t)r.position, 0), RL - 1);
        if ((pos >> 5) != tile) continue;
        uint32_t *const s = s_cnt + (mate * ERRTALLY_TILE + (uint32_t)(pos & 31)) * ERRTALLY_SLOT_WORDS;
        if (type == 0u) {
            const uint32_t q = (uint32_t)min(max((int32_t)r.quality, 0), ERRTALLY_NQ - 1);
            atomicAdd(&s[q], 1u);
            atomicAdd(&s[ERRTALLY_QPITCH + export_code(r.ref) * 5u + export_code(r.alt)], 1u);
        } else if (type == 1u) {
            atomicAdd(&s[ERRTALLY_QPITCH + 25 + export_code(r.alt)], 1u);
        } else {
            atomicAdd(&s[ERRTALLY_QPITCH + 30 + export_code(r.ref)], 1u);
        }
    }
    __syncthreads();
    const ErrTallyLayout lay = errtally_layout(RL);
    for (uint32_t i = tid; i < (uint32_t)ERRTALLY_LDS_WORDS; i += ERRTALLY_THREADS) {
        const uint32_t n = s_cnt[i];
        if (!n) continue;
        const uint32_t slot = i / ERRTALLY_SLOT_WORDS, k = i - slot * ERRTALLY_SLOT_WORDS;
        const int64_t mp = (int64_t)(slot >> 5) * RL + (tile * ERRTALLY_TILE + (int32_t)(slot & 31u));  // (mate, position): < 2 L, or n is 0
        int64_t word;
        if (k < (uint32_t)ERRTALLY_NQ) word = lay.sub_q + mp * ERRTALLY_NQ + k;
        else if (k < (uint32_t)ERRTALLY_QPITCH) continue;  // (the pitch's spare word: never added to)
        else if (k < (uint32_t)ERRTALLY_QPITCH + 25u) word = lay.sub_mat + mp * 25 + (k - ERRTALLY_QPITCH);
        else if (k < (uint32_t)ERRTALLY_QPITCH + 30u) word = lay.ins + mp * 5 + (k - ERRTALLY_QPITCH - 25);
        else word = lay.del + mp * 5 + (k - ERRTALLY_QPITCH - 30);
        atomicAdd(&T.tally[word], (unsigned long long)n);
    }
}

// The per-read histograms, behind k_errtally_rows: one lane per pair of the window reads the two words of its reads (16 bytes),
// and adds every count above 0, clamped to K - 1, to a [2][3][K] LDS table; the reads with none -- nearly all of them, one word
// for the whole wave -- are counted by arithmetic at the flush: the workgroup's pairs less the table's other bins.  A workgroup
// has at most 2^30 pairs (ERRTALLY_MAX_WG_PAIRS, the host's plan): no counter wraps.  Lane 0 of the grid adds n_pairs to `pairs`
// -- or, when the call overflowed its reservation, 1 to `dropped`, and nothing else is added by anyone.
__global__ __launch_bounds__(ERRTALLY_THREADS) void k_errtally_reads(const ErrTallyArgs T) {
    __shared__ uint32_t s_hist[2 * 3 * ERRTALLY_NK];
    const uint32_t tid = threadIdx.x;
    const ErrTallyLayout lay = errtally_layout(T.RL);
    if (errtally_used(T) > T.cap) {
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&T.tally[lay.dropped], 1ull);
        return;
    }
    for (uint32_t i = tid; i < 2u * 3u * ERRTALLY_NK; i += ERRTALLY_THREADS) s_hist[i] = 0u;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * T.read_per, c1 = min(T.n_pairs, c0 + T.read_per);
    constexpr unsigned long long mask = (1ull << ERRTALLY_CNT_BITS) - 1ull;
    for (int64_t p = c0 + tid; p < c1; p += ERRTALLY_THREADS) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(T.reads + 2 * p);
        if (!(v.x | v.y)) continue;
#pragma unroll
        for (uint32_t m = 0; m < 2u; ++m) {
            const unsigned long long c = m ? v.y : v.x;
#pragma unroll
            for (uint32_t t = 0; t < 3u; ++t) {
                const uint32_t n = (uint32_t)((c >> (ERRTALLY_CNT_BITS * t)) & mask);
                if (n) atomicAdd(&s_hist[(m * 3u + t) * ERRTALLY_NK + min(n, (uint32_t)ERRTALLY_NK - 1u)], 1u);
            }
        }
    }
    __syncthreads();
    if (c1 <= c0) return;
    for (uint32_t i = tid; i < 2u * 3u * ERRTALLY_NK; i += ERRTALLY_THREADS) {
        uint32_t n = s_hist[i];
        if ((i & (ERRTALLY_NK - 1u)) == 0u) {  // bin 0: the reads of the workgroup that are in no other bin
            uint32_t some = 0u;
            for (uint32_t k = 1; k < (uint32_t)ERRTALLY_NK; ++k) some += s_hist[i + k];
            n = (uint32_t)(c1 - c0) - some;
        }
        if (n) atomicAdd(&T.tally[lay.per_read + i], (unsigned long long)n);
    }
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&T.tally[lay.pairs], (unsigned long long)T.n_pairs);
}

}  // namespace iss
