// iss_bamreads.hip.h -- k_br_*: the tallies of iss_fqtally.hip.h over BAM RECORDS instead of FASTQ text (iss_br_feed): `report --bam`,
// the reads of an aligned BAM or of `generate --ubam` as the sequencer gave them, the insert sizes a FASTQ file does not say included.
// Input: a chunk of inflated BAM bytes in device memory that holds whole alignment records, and the byte offset of every record's
// block_size field (u32: a chunk is below 2^31 bytes; the host has checked that every record lies inside the chunk).  One flat u64
// array of the context, added to -- iss_fqtally.hip.h's words at L = max_len:
//   pairs [1] | qual [2][L][94] | base [2][L][5] | gc [2][L + 1] | meanq [2][94] | insert [2048] | length [2][L + 1]
// A record as read: base p is "=ACMGRSVTWYHKDBN"[nibble p of SEQ], phred p the quality byte p as stored; with flag 0x10 the read as
// sequenced is the reverse complement -- nibble len - 1 - p with its four bits in reverse order (A 1 <-> T 8, C 2 <-> G 4, N 15 and
// '=' 0 fixed) -- and quality len - 1 - p.  A, C, G, T count as base codes 0 .. 3, every other letter as 4; G and C as GC.
//   a  k_br_records     per record: validated (BR_REC_*, the first code that applies; the smallest (record << 8 | code) over all
//                       feeds kept by an atomic minimum), then skipped (secondary / supplementary; mate flags that name no mate) or
//                       taken: the per-read fields (gc, meanq, length, pairs, insert); every record's descriptor for stage b
//   b  k_br_positions   the per-position fields (qual, base) of the taken records, one tile of 64 positions per workgroup
// Every count is an exact integer sum: the words depend neither on the launch geometry nor on the order of arrival.  Counts are
// gathered in LDS (u32) and added to the u64 words once per workgroup, one global atomic per non-zero counter (iss_tally.hip.h).
// Plain vector code.  DESIGN.md section 28.  Included by iss_mi355x.hip.
#pragma once
#include "iss_bam_record.h"

namespace iss {
namespace br {

constexpr int BR_THREADS = 256;
constexpr int BR_WAVES = BR_THREADS / 64;  // records of a workgroup and turn in the wave-per-record kernels (k_br_positions, k_be_*, k_bd_records)
constexpr int BR_MAX_LEN = 1024;         // (= ISS_BR_MAX_LEN = ISS_FQ_MAX_LEN)
constexpr int BR_GROUP = 16;             // lanes of a record in k_br_records: 8 bases a lane, 128 bases a step
constexpr int BR_LANE_BASES = 8;         // 4 bytes of SEQ and 8 of QUAL
constexpr int BR_POS_TILE = 64;          // positions of a workgroup's tables in k_br_positions: a wave's lanes
static_assert(BR_THREADS == TALLY_THREADS && BR_POS_TILE == TALLY_TILE, "k_br_positions and k_be_bases use iss_tally.hip.h's phred tile");
constexpr int BR_TARGET_WGS = 2048;      // workgroups of a launch, about: 8 per compute unit
constexpr int BR_PAD = 16;               // bytes readable behind the chunk: k_br_records reads up to 7 past a record's qualities

constexpr int BR_REC_SHORT = 1, BR_REC_TOO_LONG = 2, BR_REC_NO_QUAL = 3, BR_REC_QUAL_RANGE = 4;

// the descriptor's third word: length (0 .. 1024) | mate << 11 | reverse << 12 | not tallied << 13
constexpr uint32_t BR_D_LEN = 0x7FFu, BR_D_MATE = 1u << 11, BR_D_REVERSE = 1u << 12, BR_D_OUT = 1u << 13;

struct BrHead {  // of the feed in flight (zeroed in front of k_br_records)
    uint32_t longest;  // longest taken read of the chunk (atomic maximum)
    uint32_t pad_;
};

struct BrState {  // of the context, behind the tally words
    unsigned long long records[2];  // good records taken per mate
    unsigned long long skipped[2];  // secondary or supplementary | paired with both or neither of 0x40 / 0x80
    unsigned long long bad;         // ((record << 8) | code) of the first bad record, the smallest wins; ~0: none
};

struct BrArgs {
    const uint8_t *data;     // the chunk; readable BR_PAD bytes past n_bytes
    const uint32_t *offs;    // [n_rec]: the record's block_size field; offs + 36 <= n_bytes and offs + 4 + block_size <= n_bytes
    uint4 *desc;             // [n_rec]: SEQ offset, QUAL offset, BR_D_* word, 0
    BrHead *head;
    BrState *state;
    unsigned long long *tally;
    uint64_t first_rec;      // index of the chunk's record 0 over all records fed
    uint32_t n_bytes, n_rec;
    int32_t L;               // the context's max_len
};

// words of k_br_records' LDS: length and gc [2][L + 1] each, meanq [2][94], insert [2048], then good records [2], skipped [2], longest
inline size_t br_records_lds(int L) { return sizeof(uint32_t) * (size_t)(4 * (L + 1) + 2 * TALLY_NQ + TALLY_NINS + 5); }

// Stage a.  BR_GROUP lanes a record, 16 records a workgroup and pass, record r of pass i = (i * gridDim.x + blockIdx.x) * 16 + group.
// Lane 0 parses the fixed header; the lanes then walk SEQ and QUAL together, 8 bases a lane: 4 bytes of packed bases and 8 quality
// bytes (unaligned: SEQ starts anywhere behind the name and the CIGAR; bytes past the read's end, 7 at most, are read -- the buffer
// reaches BR_PAD bytes past the chunk -- and not counted), and sum over the group by shuffles.
__global__ __launch_bounds__(BR_THREADS) void k_br_records(const BrArgs A) {
    extern __shared__ uint32_t br_records_lds_[];
    const uint32_t tid = threadIdx.x, L = (uint32_t)A.L;
    uint32_t *const s_len = br_records_lds_, *const s_gc = s_len + 2u * (L + 1u), *const s_mq = s_gc + 2u * (L + 1u),
                    *const s_ins = s_mq + 2 * TALLY_NQ, *const s_misc = s_ins + TALLY_NINS;
    const uint32_t n_lds = 4u * (L + 1u) + 2u * TALLY_NQ + TALLY_NINS + 5u;
    for (uint32_t i = tid; i < n_lds; i += BR_THREADS) s_len[i] = 0u;
    __syncthreads();
    const uint32_t lane = tid & (BR_GROUP - 1), per_pass = BR_THREADS / BR_GROUP;
    const uint8_t *const data = A.data;
    // (the trip count is the same for all lanes of a group, and the shuffles stay inside it)
    for (uint64_t r64 = (uint64_t)blockIdx.x * per_pass + (tid / BR_GROUP); r64 < A.n_rec; r64 += (uint64_t)gridDim.x * per_pass) {
        const uint32_t r = (uint32_t)r64;
        uint32_t code = 0u, len = 0u, seq_at = 0u, flag = 0u;
        int32_t ref_id = 0, next_ref = 0, tlen = 0;
        if (lane == 0u) {
            const uint8_t *const rec = data + A.offs[r];
            const brec::RecHead h = brec::rec_head(rec);
            flag = h.flag;
            ref_id = h.ref_id;
            next_ref = h.next_ref;
            tlen = h.tlen;
            if (h.l_name == 0u || !h.fits()) code = BR_REC_SHORT;
            else if ((uint32_t)h.l_seq > L) code = BR_REC_TOO_LONG;
            else {
                len = (uint32_t)h.l_seq;
                seq_at = A.offs[r] + (uint32_t)h.seq_at();  // (inside the record, so inside the chunk)
                if (len && data[seq_at + (len + 1u) / 2u] == 0xFFu) code = BR_REC_NO_QUAL;
            }
        }
        code = __shfl(code, 0, BR_GROUP);
        len = __shfl(len, 0, BR_GROUP);
        seq_at = __shfl(seq_at, 0, BR_GROUP);
        const uint32_t qual_at = seq_at + (len + 1u) / 2u;
        uint32_t gc = 0u, qs = 0u, out_of_range = 0u;
        if (!code) {
            for (uint32_t at = lane * BR_LANE_BASES; at < len; at += BR_GROUP * BR_LANE_BASES) {
                const uint32_t bw = brec::u32(data + seq_at + at / 2u);  // bases at .. at + 7: byte k holds at + 2k (high nibble), at + 2k + 1
                const uint32_t q0 = brec::u32(data + qual_at + at), q1 = brec::u32(data + qual_at + at + 4u);
                const uint32_t nv = min((uint32_t)BR_LANE_BASES, len - at);
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)BR_LANE_BASES; ++j) {
                    if (j < nv) {
                        const uint32_t nib = (bw >> (8u * (j >> 1) + ((j & 1u) ? 0u : 4u))) & 15u;
                        const uint32_t q = ((j < 4u ? q0 : q1) >> (8u * (j & 3u))) & 0xFFu;
                        gc += (nib == 2u || nib == 4u) ? 1u : 0u;  // C, G (their complements are each other: the strand does not matter)
                        out_of_range |= q > 93u ? 1u : 0u;
                        qs += q;
                    }
                }
            }
#pragma unroll
            for (int d = 1; d < BR_GROUP; d <<= 1) {
                gc += __shfl_xor(gc, d);
                qs += __shfl_xor(qs, d);
                out_of_range |= __shfl_xor(out_of_range, d);
            }
            if (out_of_range) code = BR_REC_QUAL_RANGE;
        }
        if (lane == 0u) {
            uint32_t d = BR_D_OUT;
            if (code) {
                atomicMin(&A.state->bad, ((A.first_rec + r) << 8) | (unsigned long long)code);
            } else if (flag & 0x900u) {
                atomicAdd(&s_misc[2], 1u);
            } else if ((flag & 1u) && ((flag & 0xC0u) == 0u || (flag & 0xC0u) == 0xC0u)) {
                atomicAdd(&s_misc[3], 1u);
            } else {
                const uint32_t mate = ((flag & 1u) && (flag & 0x80u)) ? 1u : 0u;
                d = len | (mate ? BR_D_MATE : 0u) | ((flag & 0x10u) ? BR_D_REVERSE : 0u);
                atomicAdd(&s_len[mate * (L + 1u) + len], 1u);
                atomicAdd(&s_gc[mate * (L + 1u) + gc], 1u);
                if (len) atomicAdd(&s_mq[mate * TALLY_NQ + min(qs / len, (uint32_t)TALLY_NQ - 1u)], 1u);  // (a read of length 0 has no mean)
                atomicAdd(&s_misc[mate], 1u);
                atomicMax(&s_misc[4], len);
                if (mate == 0u && (flag & 1u) && !(flag & 0xCu) && ref_id == next_ref && ref_id >= 0 && tlen != 0) {
                    const int64_t t = tlen, gap = (t < 0 ? -t : t) - 2ll * (int64_t)len;  // (64 bits: INT32_MIN does not wrap)
                    atomicAdd(&s_ins[gap < 0 ? 0u : gap > TALLY_NINS - 1 ? (uint32_t)TALLY_NINS - 1u : (uint32_t)gap], 1u);
                }
            }
            A.desc[r] = make_uint4(seq_at, qual_at, d, 0u);
        }
    }
    __syncthreads();
    const fq::FqLayout lay = fq::fq_layout((int)L);
    for (uint32_t i = tid; i < 2u * (L + 1u); i += BR_THREADS) {  // ([2][L + 1] in LDS as in the words)
        if (s_len[i]) atomicAdd(&A.tally[lay.length + i], (unsigned long long)s_len[i]);
        if (s_gc[i]) atomicAdd(&A.tally[lay.t.gc + i], (unsigned long long)s_gc[i]);
    }
    for (uint32_t i = tid; i < 2u * (uint32_t)TALLY_NQ; i += BR_THREADS)
        if (s_mq[i]) atomicAdd(&A.tally[lay.t.meanq + i], (unsigned long long)s_mq[i]);
    for (uint32_t i = tid; i < (uint32_t)TALLY_NINS; i += BR_THREADS)
        if (s_ins[i]) atomicAdd(&A.tally[lay.t.insert + i], (unsigned long long)s_ins[i]);
    if (tid < 4u && s_misc[tid]) {
        if (tid == 0u) atomicAdd(&A.tally[0], (unsigned long long)s_misc[0]);  // pairs: the good records of mate 0
        atomicAdd(tid < 2u ? &A.state->records[tid] : &A.state->skipped[tid - 2u], (unsigned long long)s_misc[tid]);
    }
    if (tid == 4u && s_misc[4]) atomicMax(&A.head->longest, s_misc[4]);
}

// Stage b.  Workgroup (t, c): positions [64 t, 64 t + 64) of the records c * 4 + wave, then every gridDim.y * 4 further; its tables
// are those of one tile for both mates, 2 x 64 positions x (94 phreds + 5 base codes), the phred rows at an odd pitch
// (k_fq_positions).  A wave takes a record, a lane a position: lane p of a forward read takes nibble p and quality p, lane p of a
// reverse read nibble len - 1 - p with its bits reversed and quality len - 1 - p.  Nibble k is the high half of byte k / 2 for even
// k, the low half for odd k -- so the last base of an odd-length read is a high half whose low half is padding, on either strand.
// A tile past the chunk's longest read has nothing to count and leaves at once.
__global__ __launch_bounds__(BR_THREADS) void k_br_positions(const BrArgs A) {
    __shared__ uint32_t s_qual[2 * BR_POS_TILE * TALLY_QPITCH];
    __shared__ uint32_t s_base[2 * BR_POS_TILE * 5];
    const uint32_t tid = threadIdx.x, pos0 = blockIdx.x * (uint32_t)BR_POS_TILE;
    if (pos0 >= A.head->longest) return;  // (the same word for every lane of the workgroup: nobody waits at a barrier below)
    tile_qual_zero<2>(s_qual, tid);
    for (uint32_t i = tid; i < 2u * BR_POS_TILE * 5u; i += BR_THREADS) s_base[i] = 0u;
    __syncthreads();
    const uint32_t lane = tid & 63u, L = (uint32_t)A.L;
    const uint32_t pos = pos0 + lane;
    for (uint64_t r64 = (uint64_t)blockIdx.y * BR_WAVES + (tid >> 6); r64 < A.n_rec; r64 += (uint64_t)gridDim.y * BR_WAVES) {
        const uint4 d = A.desc[(uint32_t)r64];
        const uint32_t len = d.z & BR_D_LEN;
        if ((d.z & BR_D_OUT) || pos >= len) continue;  // (len <= L)
        const uint32_t src = (d.z & BR_D_REVERSE) ? len - 1u - pos : pos;
        uint32_t nib = brec::seq_nibble(A.data, d.x, src);
        if (d.z & BR_D_REVERSE) nib = __brev(nib) >> 28;  // the complement: the four bits in reverse order
        const uint32_t q = A.data[d.y + src];             // (k_br_records saw q <= 93)
        const uint32_t c = brec::nib_code(nib);           // (in front of the adds: both loads are in flight together)
        const uint32_t slot = ((d.z & BR_D_MATE) ? (uint32_t)BR_POS_TILE : 0u) + lane;
        atomicAdd(&s_qual[slot * TALLY_QPITCH + q], 1u);
        atomicAdd(&s_base[slot * 5u + c], 1u);
    }
    __syncthreads();
    const fq::FqLayout lay = fq::fq_layout((int)L);
    tile_qual_flush<2>(s_qual, tid, pos0, L, A.tally + lay.t.qual);
    tile_base_flush<2>(s_base, tid, pos0, L, A.tally + lay.t.base);
}

// The launch geometry (host): wgs workgroups aimed at (0: BR_TARGET_WGS) by k_br_records and by every tile column of
// k_br_positions, no more than the records can keep busy.
struct BrPlan {
    uint32_t rec_wgs, pos_tiles, pos_chunks;
};
// workgroups of a wave-per-record kernel (k_be_records, k_bd_records, a tile column of k_br_positions): no more than have records
inline uint32_t wave_record_wgs(int64_t n_rec, int wgs) {
    const int64_t target = wgs > 0 ? wgs : BR_TARGET_WGS;
    return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(target, (n_rec + BR_WAVES - 1) / BR_WAVES));
}
inline BrPlan br_plan(int64_t n_rec, int L, int wgs) {
    const int64_t target = wgs > 0 ? wgs : BR_TARGET_WGS;
    BrPlan p;
    p.rec_wgs = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(target, (n_rec + BR_THREADS / BR_GROUP - 1) / (BR_THREADS / BR_GROUP)));
    p.pos_tiles = (uint32_t)((L + BR_POS_TILE - 1) / BR_POS_TILE);
    // (per tile column: the host does not know the longest read, and the columns beyond it leave at their first instruction)
    p.pos_chunks = std::min<uint32_t>(wave_record_wgs(n_rec, wgs), 65535u);
    return p;
}

}  // namespace br
}  // namespace iss
