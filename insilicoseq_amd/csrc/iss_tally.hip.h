// iss_tally.hip.h -- k_tally_lines, k_tally_reads: integer tallies over the output rows (iss_output_tally): what a run produced,
// without a byte of FASTQ.  One flat u64 array in the caller's device memory, added to (include/iss_mi355x.h has the layout):
//   pairs [1] | qual [2][L][94] | base [2][L][5] | gc [2][L + 1] | meanq [2][94] | insert [2048]
// Every count is an exact integer sum: the result depends neither on the launch geometry nor on the order of arrival.
// Counts are gathered in LDS (u32) and added to the u64 words once per workgroup, one global atomic per non-zero counter (the
// pattern of k_bam_* in iss_bam.hip.h).  DESIGN.md section 18.  Included by iss_mi355x.hip.
#pragma once

namespace iss {

constexpr int TALLY_THREADS = 256;
constexpr int TALLY_NQ = 94;            // phred 0 .. 93 (= ISS_TALLY_PHREDS); a larger byte counts in bin 93
constexpr int TALLY_NINS = 2048;        // (= ISS_TALLY_INSERT_BINS)
constexpr int TALLY_QPITCH = 95;        // LDS words per (mate, position) of the phred table: odd, so that the 64 lanes of a wave
                                        // instruction -- 64 different (mate, position) -- fall into different banks at equal phreds
constexpr int TALLY_TARGET_WGS = 2048;  // workgroups of a launch, about: 8 per compute unit
constexpr int64_t TALLY_MAX_WG_PAIRS = (int64_t)1 << 30;  // pairs of one workgroup at most: a u32 LDS counter cannot wrap

constexpr int TALLY_TILE = 64;          // positions of a phred tile: a wave's lanes

struct TallyLayout {  // word offsets of the fields for read length L
    int64_t qual, base, gc, meanq, insert, words;
};
__host__ __device__ inline TallyLayout tally_layout(int L) {
    TallyLayout t;
    t.qual = 1;
    t.base = t.qual + 2 * (int64_t)L * TALLY_NQ;
    t.gc = t.base + 2 * (int64_t)L * 5;
    t.meanq = t.gc + 2 * ((int64_t)L + 1);
    t.insert = t.meanq + 2 * TALLY_NQ;
    t.words = t.insert + TALLY_NINS;
    return t;
}

// The launch geometry (host): k_tally_lines runs (lines of a row) x n_chunks workgroups, workgroup (l, c) owning line l of the
// pairs [c * chunk, (c + 1) * chunk); k_tally_reads runs read_wgs workgroups of read_per pairs each.  wgs: the workgroups aimed at
// (0: TALLY_TARGET_WGS).  false: more pairs than a launch takes (no geometry keeps a workgroup under TALLY_MAX_WG_PAIRS).
struct TallyPlan {
    int64_t chunk, read_per;
    uint32_t n_lines, n_chunks, read_wgs;
};
inline bool tally_plan(int64_t n_pairs, int row, int wgs, TallyPlan *out) {
    if (n_pairs < 1 || row < 128 || (row & 127)) return false;
    const int64_t target = wgs > 0 ? wgs : TALLY_TARGET_WGS;
    TallyPlan p;
    p.n_lines = (uint32_t)(row >> 7);
    const int64_t per_line = std::max<int64_t>(1, target / p.n_lines);
    p.chunk = std::min<int64_t>((n_pairs + per_line - 1) / per_line, TALLY_MAX_WG_PAIRS);  // (rather more workgroups than a counter that wraps)
    p.chunk = std::max<int64_t>(p.chunk, (n_pairs + 65534) / 65535);  // (gridDim.y)
    p.chunk = (p.chunk + 31) / 32 * 32;                               // whole passes of a workgroup's 32 pair slots
    const int64_t n_chunks = (n_pairs + p.chunk - 1) / p.chunk;
    p.read_per = std::min<int64_t>((n_pairs + target - 1) / target, TALLY_MAX_WG_PAIRS);
    p.read_per = (p.read_per + 31) / 32 * 32;
    const int64_t read_wgs = (n_pairs + p.read_per - 1) / p.read_per;
    if (p.chunk > TALLY_MAX_WG_PAIRS || p.read_per > TALLY_MAX_WG_PAIRS || n_chunks > 65535 || read_wgs > (int64_t)0x7fffffff) return false;
    p.n_chunks = (uint32_t)n_chunks;
    p.read_wgs = (uint32_t)read_wgs;
    *out = p;
    return true;
}

struct TallyArgs {
    const uint8_t *rows;     // byte 0 of the window's first row
    const PairDesc *desc;    // its descriptor
    int64_t n_pairs;
    int32_t RL, row;         // read length, bytes of a device row
    int64_t chunk;           // k_tally_lines: pairs of a workgroup
    int64_t read_per;        // k_tally_reads: pairs of a workgroup
    unsigned long long *tally;
};

constexpr size_t TALLY_LINES_LDS = sizeof(uint32_t) * (64 * TALLY_QPITCH + 64 * 5);
inline size_t tally_reads_lds(int RL) { return sizeof(uint32_t) * (size_t)(TALLY_NINS + 2 * TALLY_NQ + 2 * (RL + 1)); }

// The phred tile of k_fq_positions, k_br_positions and k_be_bases: u32 [MATES x 64][TALLY_QPITCH] in LDS, slot = mate * 64 + position
// in the tile; beside it [MATES x 64][5] base codes.  A flush adds the non-zero counters of positions pos0 .. pos0 + 63 below L to a
// field [..][L][94] (or [..][L][5]) of u64 words, `field` its word 0 for the tile's mate 0.  All TALLY_THREADS threads call.
template <int MATES>
__device__ __forceinline__ void tile_qual_zero(uint32_t *s_qual, uint32_t tid) {
    for (uint32_t i = tid; i < (uint32_t)(MATES * TALLY_TILE * TALLY_QPITCH); i += TALLY_THREADS) s_qual[i] = 0u;
}
template <int MATES>
__device__ __forceinline__ void tile_qual_flush(const uint32_t *s_qual, uint32_t tid, uint32_t pos0, uint32_t L, unsigned long long *field) {
    for (uint32_t i = tid; i < (uint32_t)(MATES * TALLY_TILE * TALLY_NQ); i += TALLY_THREADS) {
        const uint32_t slot = i / TALLY_NQ, ph = i - slot * TALLY_NQ;
        const uint32_t n = s_qual[slot * TALLY_QPITCH + ph], p = pos0 + (slot & 63u);
        const int64_t m = slot >> 6;
        if (n && p < L) atomicAdd(&field[(m * L + p) * TALLY_NQ + ph], (unsigned long long)n);
    }
}
template <int MATES>
__device__ __forceinline__ void tile_base_flush(const uint32_t *s_base, uint32_t tid, uint32_t pos0, uint32_t L, unsigned long long *field) {
    for (uint32_t i = tid; i < (uint32_t)(MATES * TALLY_TILE * 5); i += TALLY_THREADS) {
        const uint32_t slot = i / 5u, p = pos0 + (slot & 63u);
        const int64_t m = slot >> 6;
        if (s_base[i] && p < L) atomicAdd(&field[(m * L + p) * 5 + (i - slot * 5u)], (unsigned long long)s_base[i]);
    }
}

// The per-position tables.  Workgroup (l, c) reads line l -- 128 bytes: the 32 positions 32 l .. 32 l + 31 of both mates -- of
// every pair of its chunk, at stride `row`; its tables are those of one line: 64 (mate, position) x (94 phreds + 5 base codes).
// A lane owns one 16-byte piece [8 bases][8 phreds] of a pair: 8 lanes a pair, a wave 8 pairs, the workgroup 32 pairs a pass.
// Lanes that hold the same piece of different pairs would add to the same counter whenever the phreds agree, and they mostly do
// (a model has a few phreds per position).  So the 8 lanes of a piece walk its 8 positions in ROTATED order -- the lane of pair
// slot g takes position (j + g) % 8 at step j: in every wave instruction the 64 lanes stand at 64 different (mate, position),
// hence at 64 different LDS words, and no add of one instruction waits for another lane's.
__global__ __launch_bounds__(TALLY_THREADS) void k_tally_lines(const TallyArgs T) {
    __shared__ uint32_t s_qual[64 * TALLY_QPITCH];
    __shared__ uint32_t s_base[64 * 5];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 64u * TALLY_QPITCH; i += TALLY_THREADS) s_qual[i] = 0u;
    for (uint32_t i = tid; i < 64u * 5u; i += TALLY_THREADS) s_base[i] = 0u;
    __syncthreads();
    const uint32_t line = blockIdx.x, RL = (uint32_t)T.RL;
    const uint32_t q = tid & 7u, g = (tid >> 3) & 7u;          // piece of the line; pair slot within the wave
    const uint32_t slot0 = (q >> 2) * 32u + (q & 3u) * 8u;     // (mate, position in the line) of the piece's first byte
    const uint32_t pos0 = line * 32u + (q & 3u) * 8u;
    const uint32_t nv = pos0 < RL ? min(8u, RL - pos0) : 0u;   // positions of the piece inside the read (the rest: padding)
    const int64_t c0 = (int64_t)blockIdx.y * T.chunk, c1 = min(T.n_pairs, c0 + T.chunk);
    if (nv) {
        const uint8_t *const src = T.rows + (size_t)line * 128u + (size_t)q * 16u;
        for (int64_t p0 = c0 + (tid >> 3); p0 < c1; p0 += 4 * 32) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // (the loads of four passes in flight)
                const int64_t p = p0 + 32 * u;
                v[u] = p < c1 ? *reinterpret_cast<const uint4 *>(src + (size_t)p * (size_t)T.row) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (p0 + 32 * u >= c1) break;
                const uint64_t bw = (uint64_t)v[u].x | ((uint64_t)v[u].y << 32), qw = (uint64_t)v[u].z | ((uint64_t)v[u].w << 32);
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    const uint32_t jj = (j + g) & 7u;
                    if (jj < nv) {
                        const uint32_t b = (uint32_t)(bw >> (8u * jj)) & 0xffu, ph = (uint32_t)(qw >> (8u * jj)) & 0xffu;
                        atomicAdd(&s_qual[(slot0 + jj) * TALLY_QPITCH + min(ph, (uint32_t)TALLY_NQ - 1u)], 1u);
                        atomicAdd(&s_base[(slot0 + jj) * 5u + export_code(b)], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    const TallyLayout lay = tally_layout((int)RL);
    for (uint32_t i = tid; i < 64u * TALLY_NQ; i += TALLY_THREADS) {
        const uint32_t slot = i / TALLY_NQ, ph = i - slot * TALLY_NQ;
        const uint32_t n = s_qual[slot * TALLY_QPITCH + ph], pos = line * 32u + (slot & 31u);
        if (n && pos < RL) atomicAdd(&T.tally[lay.qual + ((int64_t)(slot >> 5) * RL + pos) * TALLY_NQ + ph], (unsigned long long)n);
    }
    for (uint32_t i = tid; i < 64u * 5u; i += TALLY_THREADS) {
        const uint32_t slot = i / 5u, code = i - slot * 5u;
        const uint32_t n = s_base[i], pos = line * 32u + (slot & 31u);
        if (n && pos < RL) atomicAdd(&T.tally[lay.base + ((int64_t)(slot >> 5) * RL + pos) * 5 + code], (unsigned long long)n);
    }
}

// The per-read quantities need a read's whole length, and a read's lines belong to different workgroups of k_tally_lines: a
// second kernel over pairs.  8 lanes a pair again, lane q on piece q of every line; G / C letters and phred sums are counted 8
// bytes at a time, summed over the four lanes of a mate, and one lane per mate adds to the LDS tables (gc, meanq), one per pair
// to insert.  A workgroup's pairs are counted by arithmetic.
__global__ __launch_bounds__(TALLY_THREADS) void k_tally_reads(const TallyArgs T) {
    extern __shared__ uint32_t tally_reads_lds_[];
    const uint32_t tid = threadIdx.x, RL = (uint32_t)T.RL;
    uint32_t *const s_ins = tally_reads_lds_, *const s_mq = s_ins + TALLY_NINS, *const s_gc = s_mq + 2 * TALLY_NQ;
    const uint32_t n_lds = TALLY_NINS + 2u * TALLY_NQ + 2u * (RL + 1u);
    for (uint32_t i = tid; i < n_lds; i += TALLY_THREADS) s_ins[i] = 0u;
    __syncthreads();
    const uint32_t q = tid & 7u, mate = q >> 2, n_lines = (uint32_t)T.row >> 7;
    const int64_t c0 = (int64_t)blockIdx.x * T.read_per, c1 = min(T.n_pairs, c0 + T.read_per);
    for (int64_t p = c0 + (tid >> 3); p < c1; p += 32) {  // (c0 and the stride are multiples of 32: the 8 lanes of a pair stay together)
        const uint8_t *const src = T.rows + (size_t)p * (size_t)T.row + (size_t)q * 16u;
        uint32_t gc = 0u, qs = 0u;
#pragma unroll 4
        for (uint32_t l = 0; l < n_lines; ++l) {
            const uint32_t pos0 = l * 32u + (q & 3u) * 8u;
            if (pos0 >= RL) break;  // (padding of the last line)
            const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)l * 128u);
            const uint32_t nv = min(8u, RL - pos0);
            const uint64_t valid = nv >= 8u ? ~0ull : ((1ull << (8u * nv)) - 1ull);
            const uint64_t bw = (uint64_t)v.x | ((uint64_t)v.y << 32), qw = ((uint64_t)v.z | ((uint64_t)v.w << 32)) & valid;
            // 'C' 0x43, 'G' 0x47, 'c' 0x63, 'g' 0x67: the letters that are 0x43 with bits 2 and 5 cleared -> a zero byte of t
            const uint64_t t = (bw & 0xDBDBDBDBDBDBDBDBull) ^ 0x4343434343434343ull;
            const uint64_t nonzero = (((t & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | t) & 0x8080808080808080ull;
            gc += (uint32_t)__popcll(~nonzero & 0x8080808080808080ull & valid);
            const uint64_t s2 = (qw & 0x00FF00FF00FF00FFull) + ((qw >> 8) & 0x00FF00FF00FF00FFull);  // four 16-bit sums
            const uint64_t s4 = (s2 & 0x0000FFFF0000FFFFull) + ((s2 >> 16) & 0x0000FFFF0000FFFFull);
            qs += (uint32_t)s4 + (uint32_t)(s4 >> 32);
        }
        gc += __shfl_xor(gc, 1);
        qs += __shfl_xor(qs, 1);
        gc += __shfl_xor(gc, 2);
        qs += __shfl_xor(qs, 2);
        if ((q & 3u) == 0u) {
            atomicAdd(&s_gc[mate * (RL + 1u) + gc], 1u);
            atomicAdd(&s_mq[mate * TALLY_NQ + min(qs / RL, (uint32_t)TALLY_NQ - 1u)], 1u);
        }
        if (q == 0u) {
            const int32_t isz = T.desc[p].isz;
            atomicAdd(&s_ins[(uint32_t)min(max(isz, 0), TALLY_NINS - 1)], 1u);
        }
    }
    __syncthreads();
    const TallyLayout lay = tally_layout((int)RL);
    for (uint32_t i = tid; i < (uint32_t)TALLY_NINS; i += TALLY_THREADS)
        if (s_ins[i]) atomicAdd(&T.tally[lay.insert + i], (unsigned long long)s_ins[i]);
    for (uint32_t i = tid; i < 2u * TALLY_NQ; i += TALLY_THREADS)
        if (s_mq[i]) atomicAdd(&T.tally[lay.meanq + i], (unsigned long long)s_mq[i]);
    for (uint32_t i = tid; i < 2u * (RL + 1u); i += TALLY_THREADS)
        if (s_gc[i]) atomicAdd(&T.tally[lay.gc + i], (unsigned long long)s_gc[i]);
    if (tid == 0u && c1 > c0) atomicAdd(&T.tally[0], (unsigned long long)(c1 - c0));
}

}  // namespace iss
