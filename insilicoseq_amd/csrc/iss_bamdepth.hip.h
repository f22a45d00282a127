// iss_bamdepth.hip.h -- k_bd_records: where an aligned BAM's reads fall on the references, as their CIGARs tell it (`report --bam
// --depth`, iss_br_depth_enable): the fourth, optional stage of iss_br_feed, behind k_br_records and k_br_positions (and behind
// the error stage when both are on) on the same staged chunk and the same descriptors.  It adds to the CALLER's int32 difference
// array in iss_depth_*'s layout (iss_depth.hip.h): row refID of the table is (offset, length), a covered run [s, e) of the
// reference adds +1 at offset + s and -1 at offset + e, and iss_depth_finish makes depths, statistics and window sums of it.
// Which records: those the read tally took (descriptor not BR_D_OUT), then, the first that applies --
//   not aligned (0x4, n_cigar_op == 0 or refID < 0)  counts[1]   |   0x200 or 0x400  counts[2]   |   mapq < min_mapq  counts[3]
// -- then validated completely before any word is touched, the first code deciding: BD_CIGAR (an op code above 8), BD_REF (refID >=
// n_table), [a row with offset < 0: counts[4], nothing marked, its length not looked at], BD_SPAN (pos < 0 or pos + the lengths of M,
// D, N, =, X, summed in 64 bits, past the row's length).  A bad record adds nothing anywhere; the smallest (record << 8 | code) over
// all feeds is kept.  A valid one: counts[0], its M / = / X runs (D too with BD_COUNT_DEL; N never) marked, their lengths to counts[5].
//   k_bd_records   a wavefront per record; the lanes stride over the ops in turns of 64.  Pass 1: bad-op ballot and the 64-bit sum
//                  of the reference-consuming lengths by shuffles.  Pass 2: a wave-wide scan of those lengths gives every lane its
//                  op's reference cursor, a carry goes from turn to turn, and every lane with a covering op issues its two int32
//                  atomic adds without return (relaxed, agent scope, as k_depth_mark does).  The counts gather in LDS and are
//                  added once per workgroup.
// Every result is an exact integer sum: neither the launch geometry nor the cut into feeds shows.  Plain vector code, no scratch.
// DESIGN.md section 32.  Included by iss_mi355x.hip behind iss_bamerrors.hip.h.
#pragma once

namespace iss {
namespace bd {

constexpr int BD_CIGAR = 1, BD_REF = 2, BD_SPAN = 3;  // (= ISS_BR_DEPTH_*)
constexpr uint32_t BD_COUNT_DEL = 1u;                 // (= ISS_BR_DEPTH_COUNT_DEL)

struct BdState {  // of the context
    unsigned long long counts[6];  // marked, not aligned, filtered (0x200 | 0x400), below min_mapq, on a skipped row, covered bases
    unsigned long long bad;        // ((record << 8) | code) of the first bad record, the smallest wins; ~0: none
};

struct BdArgs {
    br::BrArgs R;          // the feed: chunk, offsets, descriptors (k_br_records wrote them), first_rec
    const int64_t *table;  // [n_table][2]: (offset, length) of reference refID; offset < 0: a skipped row
    int32_t *diff;         // the caller's difference array (4-byte aligned)
    BdState *state;
    int32_t n_table;
    uint32_t flags, min_mapq;
};

// Wave w of workgroup b takes records b * 4 + w, then every gridDim.x * 4 further: the record is the same for all lanes of a wave,
// so the shuffles and ballots below run with every lane in step.  The CIGAR of a record the read tally took lies inside the record
// (k_br_records checked 32 + l_read_name + 4 n_cigar_op + ... <= block_size), so inside the chunk.
__global__ __launch_bounds__(br::BR_THREADS) void k_bd_records(const BdArgs E) {
    __shared__ unsigned long long s_counts[6];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (tid < 6u) s_counts[tid] = 0ull;
    __syncthreads();
    const bool count_del = (E.flags & BD_COUNT_DEL) != 0u;
    for (uint64_t r64 = (uint64_t)blockIdx.x * br::BR_WAVES + w; r64 < E.R.n_rec; r64 += (uint64_t)gridDim.x * br::BR_WAVES) {
        const uint32_t r = (uint32_t)r64;
        if (E.R.desc[r].z & br::BR_D_OUT) continue;
        const uint8_t *const rec = E.R.data + E.R.offs[r];
        const brec::RecHead h = brec::rec_head(rec);
        const int32_t ref_id = h.ref_id, pos = h.pos;
        const uint32_t n_cigar = h.n_cigar;
        int slot = -1;  // the count of a record that marks nothing
        if ((h.flag & 4u) || !n_cigar || ref_id < 0) slot = 1;
        else if (h.flag & 0x600u) slot = 2;
        else if (h.mapq < E.min_mapq) slot = 3;
        if (slot >= 0) {
            if (lane == 0u) atomicAdd(&s_counts[slot], 1ull);
            continue;
        }
        const uint8_t *const cig = rec + h.cigar_at();
        // ---- pass 1: the ops and the reference span
        bool bad_op = false;
        unsigned long long span = 0ull;
        for (uint32_t i = lane; i < n_cigar; i += 64u) {
            const uint32_t c = brec::u32(cig + 4u * i), op = c & 15u;
            bad_op |= op > brec::OP_LAST;
            if (brec::in(op, brec::OPS_REF)) span += c >> 4;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) span += __shfl_xor(span, o);  // (at most 65 535 ops below 2^28 each: below 2^44)
        int code = 0;
        int64_t off = -1, length = 0;
        if (__any(bad_op)) {
            code = BD_CIGAR;
        } else if (ref_id >= E.n_table) {
            code = BD_REF;
        } else {
            off = E.table[2 * (int64_t)ref_id];
            length = E.table[2 * (int64_t)ref_id + 1];
            if (off < 0) {
                if (lane == 0u) atomicAdd(&s_counts[4], 1ull);
                continue;
            }
            if (pos < 0 || (int64_t)pos + (int64_t)span > length) code = BD_SPAN;
        }
        if (code) {
            if (lane == 0u) atomicMin(&E.state->bad, ((E.R.first_rec + r64) << 8) | (unsigned long long)code);
            continue;
        }
        // ---- pass 2: every word index below lies in [off, off + length]: cursor + ln <= pos + span <= length
        int32_t *const words = E.diff + off;
        unsigned long long carry = (unsigned long long)pos, covered = 0ull;
        for (uint32_t i0 = 0; i0 < n_cigar; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const uint32_t c = i < n_cigar ? brec::u32(cig + 4u * i) : 0u, op = c & 15u, ln = i < n_cigar ? c >> 4 : 0u;
            const bool column = op == brec::OP_M || op == brec::OP_EQ || op == brec::OP_X;  // (OPS_COLUMN, OPS_REF: in() costs registers here)
            const unsigned long long step = (column || op == brec::OP_D || op == brec::OP_N) ? ln : 0u;
            unsigned long long incl = step;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long y = __shfl_up(incl, d);
                if (lane >= (uint32_t)d) incl += y;
            }
            if (ln && (column || (count_del && op == brec::OP_D))) {
                const unsigned long long start = carry + incl - step;
                (void)__hip_atomic_fetch_add(words + start, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(words + start + ln, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                covered += ln;
            }
            carry += __shfl(incl, 63);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) covered += __shfl_xor(covered, o);
        if (lane == 0u) {
            atomicAdd(&s_counts[0], 1ull);
            if (covered) atomicAdd(&s_counts[5], covered);
        }
    }
    __syncthreads();
    if (tid < 6u && s_counts[tid]) atomicAdd(&E.state->counts[tid], s_counts[tid]);
}

}  // namespace bd
}  // namespace iss
