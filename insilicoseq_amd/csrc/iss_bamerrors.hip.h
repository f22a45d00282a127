// iss_bamerrors.hip.h -- k_be_*: the errors of an aligned BAM's reads against the reference they were aligned to, told by CIGAR and
// MD (`report --bam --errors`, iss_br_errors_enable): the third stage of iss_br_feed, behind k_br_records and k_br_positions on the
// same staged chunk and the same descriptors.  One flat u64 array of the context, added to -- iss_errtally.hip.h's words at
// L = max_len, then the aligned bases:
//   dropped [1] | pairs [1] | sub_q [2][L][94] | sub_mat [2][L][5][5] | ins [2][L][5] | del [2][L][5] | per_read [2][3][64]
//   | bases [2][L][94]
// Positions and letters are those of the read as sequenced (k_br_positions): SEQ index q of a reverse record counts at len - 1 - q
// with its letters complemented (0 <-> 3, 1 <-> 2, 4 fixed).
//   c  k_be_records   a wavefront per record the read tally took: aligned or not; validated completely -- BE_ALN_CIGAR, _TAGS, _MD,
//                     the first that applies; the smallest (record << 8 | code) over all feeds kept -- before any of its counts is
//                     added; then its rows (substitutions, insertions, deletions: global u64 atomics, they are sparse), its
//                     rows-per-read bins and the record counts (LDS, added once per workgroup), and one bit per position as
//                     sequenced, "an M, = or X column", for stage d
//   d  k_be_bases     the dense field: bases [2][L][94] of the marked positions, one tile of 64 positions per workgroup, gathered
//                     in LDS and added to the words once per workgroup (k_br_positions' tables without the base codes)
// Every count is an exact integer sum: the words depend neither on the launch geometry nor on how the records were cut into feeds.
// Plain vector code.  DESIGN.md section 29.  Included by iss_mi355x.hip behind iss_bamreads.hip.h and iss_errtally.hip.h.
#pragma once
#include "iss_bam_record.h"

namespace iss {
namespace be {
using brec::RecHead, brec::rec_head, brec::be_tag_walk, brec::BE_TAGS_MD, brec::BE_TAGS_NO_MD, brec::nib_code, brec::seq_nibble;
using brec::OP_M, brec::OP_I, brec::OP_S, brec::OP_EQ, brec::OP_X;

constexpr int BE_MAP = br::BR_MAX_LEN;  // bytes of a wave's map: one per SEQ index
constexpr int BE_NK = ERRTALLY_NK;      // rows-per-read bins
// a wave's map, per SEQ index: 0 soft-clipped, BE_COL an M / = / X column that matches, BE_INS an inserted base,
// BE_MISMATCH | code of the MD letter a column that does not
constexpr uint32_t BE_COL = 1u, BE_INS = 2u, BE_MISMATCH = 0x80u;

struct BeState {  // of the context, behind the error words
    unsigned long long counts[4];  // aligned and tallied per mate [2], taken but not aligned, aligned without an MD tag
    unsigned long long bad;        // ((record << 8) | code) of the first bad alignment, the smallest wins; ~0: none
};

struct BeArgs {
    br::BrArgs R;                // the feed: chunk, offsets, descriptors (k_br_records wrote them), head, first_rec, L
    unsigned long long *err;     // the error words
    BeState *state;
    unsigned long long *mask;    // [n_rec][tiles]: bit p % 64 of word p / 64 -- position p as sequenced is an aligned column
    uint32_t tiles;              // ceil(L / 64)
    uint32_t rounds;             // of k_be_records: ceil(n_rec / (its workgroups * 4)), from the host
};

__host__ __device__ inline int64_t be_words(int L) { return errtally_layout(L).words + 2 * (int64_t)L * ERRTALLY_NQ; }

// Stage c.  Wave w of workgroup b takes record (i * gridDim.x + b) * 4 + w in round i; every wave of a workgroup runs the same
// number of rounds (BeArgs::rounds), so that workgroup barriers separate the phases (lane 0 writes the map that all lanes read).
// The CIGAR's sum is checked before the map is written and the MD walk stays inside the CIGAR's columns: no map index reaches
// len <= 1 024.
__global__ __launch_bounds__(br::BR_THREADS) void k_be_records(const BeArgs E) {
    __shared__ uint8_t s_map[br::BR_WAVES][BE_MAP];
    __shared__ uint32_t s_pr[2 * 3 * BE_NK];
    __shared__ uint32_t s_misc[8];  // tallied per mate [2], unaligned, no_md, dropped
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, L = (uint32_t)E.R.L;
    for (uint32_t i = tid; i < 2u * 3u * BE_NK; i += br::BR_THREADS) s_pr[i] = 0u;
    if (tid < 8u) s_misc[tid] = 0u;
    uint8_t *const map = s_map[w];
    __syncthreads();
    const uint8_t *const data = E.R.data;
    const ErrTallyLayout lay = errtally_layout((int)L);
    const uint64_t per_round = (uint64_t)gridDim.x * br::BR_WAVES;
    for (uint64_t it = 0; it < E.rounds; ++it) {
        const uint64_t r64 = it * per_round + (uint64_t)blockIdx.x * br::BR_WAVES + w;
        // ---- phase A: taken or not, aligned or not, the CIGAR's ops and sum, the optional fields up to MD:Z
        enum { NONE, UNALIGNED, NO_MD, BAD, LIVE } kind = NONE;
        uint32_t code = 0u, len = 0u, n_cigar = 0u, md_len = 0u, mate = 0u, seq_at = 0u, qual_at = 0u;
        bool reverse = false, has_del = false;
        const uint8_t *cig = nullptr, *md = nullptr;
        if (r64 < E.R.n_rec) {
            const uint4 d = E.R.desc[(uint32_t)r64];
            if (!(d.z & br::BR_D_OUT)) {
                const uint8_t *const rec = data + E.R.offs[(uint32_t)r64];
                const RecHead h = rec_head(rec);  // (the record is good: its fields fit block_size)
                n_cigar = h.n_cigar;
                len = d.z & br::BR_D_LEN;
                mate = (d.z & br::BR_D_MATE) ? 1u : 0u;
                reverse = (d.z & br::BR_D_REVERSE) != 0u;
                seq_at = d.x;
                qual_at = d.y;
                cig = rec + h.cigar_at();
                if ((h.flag & 4u) || !n_cigar || !len) {
                    kind = UNALIGNED;
                } else {
                    bool bad_op = false, del = false;
                    unsigned long long qsum = 0ull;
                    for (uint32_t i = lane; i < n_cigar; i += 64u) {
                        const uint32_t c = u32(cig + 4u * i), op = c & 15u;
                        bad_op |= op > OP_LAST;
                        del |= op == OP_D;  // (OPS_QUERY spelled out, and the sum shuffled in halves: in() or a 64-bit shuffle
                        if (op == OP_M || op == OP_I || op == OP_S || op == OP_EQ || op == OP_X) qsum += c >> 4;  // costs registers)
                    }
                    uint32_t lo = (uint32_t)qsum, hi = (uint32_t)(qsum >> 32);  // (at most 65 535 ops below 2^28 each)
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const uint32_t lo2 = __shfl_xor(lo, o), hi2 = __shfl_xor(hi, o);
                        const unsigned long long s = (((unsigned long long)hi << 32) | lo) + (((unsigned long long)hi2 << 32) | lo2);
                        lo = (uint32_t)s;
                        hi = (uint32_t)(s >> 32);
                    }
                    has_del = __any(del);
                    if (__any(bad_op) || hi != 0u || lo != len) {
                        kind = BAD;
                        code = BE_ALN_CIGAR;
                    } else {
                        int st = 0;
                        uint32_t at = 0u, n = 0u;
                        if (lane == 0u) {
                            const uint8_t *const aux = data + qual_at + len;
                            int64_t md_at = 0;
                            st = be_tag_walk(aux, (rec + h.end()) - aux, &md_at, &n);
                            at = (uint32_t)md_at;  // (inside the record, so below 2^31)
                        }
                        st = __shfl(st, 0);
                        at = __shfl(at, 0);
                        md_len = __shfl(n, 0);
                        md = data + qual_at + len + at;
                        kind = st == BE_TAGS_MD ? LIVE : st == BE_TAGS_NO_MD ? NO_MD : BAD;
                        code = BE_ALN_TAGS;
                    }
                }
            }
        }
        if (kind == LIVE)
            for (uint32_t i = lane; i < len; i += 64u) map[i] = 0u;
        __syncthreads();
        // ---- phase B: which SEQ indices are aligned columns, which inserted bases
        if (kind == LIVE) {
            uint32_t q = 0u;
            for (uint32_t k = 0; k < n_cigar; ++k) {
                const uint32_t c = u32(cig + 4u * k), op = c & 15u, ln = c >> 4;
                if (in(op, OPS_COLUMN | 1u << OP_I))
                    for (uint32_t i = lane; i < ln; i += 64u) map[q + i] = (uint8_t)(op == OP_I ? BE_INS : BE_COL);
                if (in(op, OPS_QUERY)) q += ln;
            }
        }
        __syncthreads();
        // ---- phase C: the MD string against the CIGAR, its mismatches placed (lane 0)
        if (kind == LIVE) {
            int ok = 1;
            if (lane == 0u)
                ok = be_md_walk(cig, n_cigar, md, md_len, [&](uint32_t q, uint32_t ch) { map[q] = (uint8_t)(BE_MISMATCH | be_letter_code(ch)); },
                                [](uint32_t, uint32_t) {}) ? 1 : 0;
            if (!__shfl(ok, 0)) {
                kind = BAD;
                code = BE_ALN_MD;
            }
        }
        __syncthreads();
        // ---- phase D: the counts of a valid record; the marks of every taken one
        const uint64_t mp0 = (uint64_t)mate * L;
        if (kind == LIVE) {
            uint32_t n_sub = 0u, n_ins = 0u, n_del = 0u;
            for (uint32_t q0 = 0; q0 < len; q0 += 64u) {
                const uint32_t q = q0 + lane, c = q < len ? map[q] : 0u;
                const bool sub = (c & BE_MISMATCH) != 0u, ins = c == BE_INS;
                if (sub || ins) {
                    const uint64_t mp = mp0 + (reverse ? len - 1u - q : q);
                    uint32_t alt = nib_code(seq_nibble(data, seq_at, q));
                    if (reverse) alt = be_complement(alt);
                    if (sub) {
                        const uint32_t ref = reverse ? be_complement(c & 7u) : (c & 7u), ph = data[qual_at + q];  // (k_br_records saw ph <= 93)
                        atomicAdd(&E.err[lay.sub_q + mp * ERRTALLY_NQ + ph], 1ull);
                        atomicAdd(&E.err[lay.sub_mat + (mp * 5u + ref) * 5u + alt], 1ull);
                    } else {
                        atomicAdd(&E.err[lay.ins + mp * 5u + alt], 1ull);
                    }
                }
                n_sub += (uint32_t)__popcll(__ballot(sub));
                n_ins += (uint32_t)__popcll(__ballot(ins));
            }
            if (lane == 0u) {
                if (has_del)  // (the walk again, it is known to fit: each deleted letter at the base behind the gap in sequencing order)
                    be_md_walk(cig, n_cigar, md, md_len, [](uint32_t, uint32_t) {}, [&](uint32_t q, uint32_t ch) {
                        const uint32_t pos = min(reverse ? len - q : q, len - 1u), ref = be_letter_code(ch);
                        atomicAdd(&E.err[lay.del + (mp0 + pos) * 5u + (reverse ? be_complement(ref) : ref)], 1ull);
                        ++n_del;
                    });
                atomicAdd(&s_pr[(mate * 3u + 0u) * BE_NK + min(n_sub, (uint32_t)BE_NK - 1u)], 1u);
                atomicAdd(&s_pr[(mate * 3u + 1u) * BE_NK + min(n_ins, (uint32_t)BE_NK - 1u)], 1u);
                atomicAdd(&s_pr[(mate * 3u + 2u) * BE_NK + min(n_del, (uint32_t)BE_NK - 1u)], 1u);
                atomicAdd(&s_misc[mate], 1u);
            }
        } else if (lane == 0u && kind != NONE) {
            atomicAdd(&s_misc[kind == UNALIGNED ? 2 : kind == NO_MD ? 3 : 4], 1u);
            if (kind == BAD) atomicMin(&E.state->bad, ((E.R.first_rec + r64) << 8) | (unsigned long long)code);
        }
        if (kind != NONE) {  // (a record the read tally left out has a descriptor that says so: stage d does not look at its marks)
            for (uint32_t p0 = 0; p0 < len; p0 += 64u) {
                const uint32_t p = p0 + lane;
                bool col = false;
                if (kind == LIVE && p < len) {
                    const uint32_t c = map[reverse ? len - 1u - p : p];
                    col = c == BE_COL || (c & BE_MISMATCH) != 0u;
                }
                const unsigned long long bits = __ballot(col);
                if (lane == 0u) E.mask[r64 * E.tiles + (p0 >> 6)] = bits;
            }
        }
        __syncthreads();  // (the map is zeroed again in the next round)
    }
    for (uint32_t i = tid; i < 2u * 3u * BE_NK; i += br::BR_THREADS)
        if (s_pr[i]) atomicAdd(&E.err[lay.per_read + i], (unsigned long long)s_pr[i]);
    if (tid < 4u && s_misc[tid]) atomicAdd(&E.state->counts[tid], (unsigned long long)s_misc[tid]);
    if (tid == 4u && s_misc[4]) atomicAdd(&E.err[lay.dropped], (unsigned long long)s_misc[4]);
    if (tid == 5u && s_misc[0]) atomicAdd(&E.err[lay.pairs], (unsigned long long)s_misc[0]);  // pairs: the tallied records of mate 0
}

// Stage d.  k_br_positions' geometry and phred tables: workgroup (t, c) holds positions [64 t, 64 t + 64) of both mates, a wave takes
// a record, a lane a position, and counts its phred where the record's word t of marks has the lane's bit.
__global__ __launch_bounds__(br::BR_THREADS) void k_be_bases(const BeArgs E) {
    __shared__ uint32_t s_qual[2 * br::BR_POS_TILE * TALLY_QPITCH];
    const uint32_t tid = threadIdx.x, pos0 = blockIdx.x * (uint32_t)br::BR_POS_TILE;
    if (pos0 >= E.R.head->longest) return;  // (the same word for every lane of the workgroup: nobody waits at a barrier below)
    tile_qual_zero<2>(s_qual, tid);
    __syncthreads();
    const uint32_t lane = tid & 63u, L = (uint32_t)E.R.L, pos = pos0 + lane;
    for (uint64_t r64 = (uint64_t)blockIdx.y * br::BR_WAVES + (tid >> 6); r64 < E.R.n_rec; r64 += (uint64_t)gridDim.y * br::BR_WAVES) {
        const uint4 d = E.R.desc[(uint32_t)r64];
        const uint32_t len = d.z & br::BR_D_LEN;
        if ((d.z & br::BR_D_OUT) || pos >= len) continue;  // (len <= L: the word read below was written, blockIdx.x < tiles)
        if (!((E.mask[r64 * E.tiles + blockIdx.x] >> lane) & 1ull)) continue;
        const uint32_t q = E.R.data[d.y + ((d.z & br::BR_D_REVERSE) ? len - 1u - pos : pos)];  // (k_br_records saw q <= 93)
        atomicAdd(&s_qual[(((d.z & br::BR_D_MATE) ? (uint32_t)br::BR_POS_TILE : 0u) + lane) * TALLY_QPITCH + q], 1u);
    }
    __syncthreads();
    tile_qual_flush<2>(s_qual, tid, pos0, L, E.err + errtally_layout((int)L).words);
}

// The launch geometry (host): k_be_records runs br::wave_record_wgs workgroups and this many rounds; k_be_bases takes
// k_br_positions' grid.
inline uint32_t be_record_rounds(int64_t n_rec, uint32_t wgs) { return (uint32_t)((n_rec + (int64_t)wgs * br::BR_WAVES - 1) / ((int64_t)wgs * br::BR_WAVES)); }

}  // namespace be
}  // namespace iss
