// iss_perfect.hip.h -- k_perfect: the Philox path of quality mode 2 (PerfectErrorModel, iss/error_models/perfect.py).
//
// A perfect read is its genome window (R1) or the window's reverse complement (R2), every phred 40, no indel (all-zero
// tables): nothing of k_main's sampling is left but mut_sequence's error test, and that test can only change a byte where
// the letter is a lower-case a/c/g/t (the substitution "alternatives" are the upper-case base itself; ambiguous letters are
// skipped; an upper-case base stays what it is).  So k_perfect is a copy of the genome into the output rows:
//   * one lane per 16-byte piece of a pair's row ([8 letters][8 phreds] of one mate, iss::xp): the 64 lanes of a wavefront
//     store 1 KB of consecutive rows, whole 128-byte lines, nothing written twice;
//   * letters from the packed 2-bit genome (one 64-bit window per piece), exceptions (IUPAC, lower case) from the mask and the
//     ASCII copy -- read only for pairs whose window holds one (k_setup's descriptor bits 4 / 5);
//   * per lower-case a/c/g/t: the error-test draw at exactly the address k_main uses (K_QM block (p >> 3, sub 1), byte of
//     word half * 2 + mate; the K_SUB block (p, mate) only when the 8-bit digit ties the threshold's), an event upper-cases
//     the letter.  No other Philox block is computed.
// Irregular pairs (custom fragment lengths: a template cut by the genome end) get their phreds here and their letters from
// k_indel_fixup, which runs behind this kernel as it runs behind k_main.
#pragma once

namespace iss {

constexpr int PERFECT_PHRED = 40;       // PerfectErrorModel.gen_phred_scores (perfect.py:36-43)
constexpr int PERFECT_THREADS = 256;

constexpr int PERFECT_UNROLL = 8;  // passes a lane keeps in flight: their descriptor and window loads are issued together

// lowest genome position of read positions p0 .. p0 + 7 of mate o of a regular pair: forward fs + p0 (ascending), reverse
// re - 8 - p0 (read position p0 + k is genome position re - 1 - p0 - k).  Its packed word and the next are readable: word -1
// and the two words behind a record are padding.
__device__ __forceinline__ int64_t perfect_lo(int o, const PairDesc &d, int p0) { return o == 0 ? desc_fs(d) + p0 : desc_re(d) - 8 - p0; }

// letters (ASCII) of those 8 positions from the 64-bit window `win` of packed words lo >> 4 and (lo >> 4) + 1: bytes 0-3 in .x,
// 4-7 in .y.  `valid`: the positions below the read length (bit k: position p0 + k) -- only theirs are looked up in the ASCII copy
__device__ __forceinline__ uint2 perfect_letters(const DevGenome &g, int o, int64_t lo, uint64_t win, bool exc, uint32_t valid) {
    uint32_t codes = (uint32_t)(win >> (2 * (uint32_t)(lo & 15))) & 0xffffu;  // code of genome position lo + c at bits 2c
    if (o) {  // reverse the 8 codes and complement them (code ^ 1)
        codes = ((codes & 0x3333u) << 2) | ((codes >> 2) & 0x3333u);
        codes = ((codes & 0x0f0fu) << 4) | ((codes >> 4) & 0x0f0fu);
        codes = (((codes & 0x00ffu) << 8) | (codes >> 8)) ^ 0x5555u;
    }
    uint2 r = make_uint2(codes_to_ascii4(codes & 0xffu), codes_to_ascii4(codes >> 8));
    if (exc) {  // IUPAC / lower-case letters of the window: from the ASCII copy
        const int64_t mi = lo >> 5;
        const uint64_t mw = ((uint64_t)g.mask[mi + 1] << 32) | g.mask[mi];
        uint32_t m8 = (uint32_t)(mw >> (uint32_t)(lo & 31)) & 0xffu;  // bit c: genome position lo + c
        if (o) m8 &= valid << (8 - __popc(valid)); else m8 &= valid;  // (reverse: position p0 + k is bit 7 - k)
        if (m8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int c = o ? 7 - k : k;
                if ((m8 >> c) & 1u) {
                    const int ch = o ? complement_ascii(g.ascii[lo + c]) : (int)g.ascii[lo + c];
                    uint32_t &w = k < 4 ? r.x : r.y;
                    const uint32_t sh = 8u * (uint32_t)(k & 3);
                    w = (w & ~(0xffu << sh)) | ((uint32_t)ch << sh);
                }
            }
        }
    }
    return r;
}

// bytes of the 8 letters that are lower-case a/c/g/t (bit k: letter k)
__device__ __forceinline__ uint32_t perfect_lower_mask(uint2 r) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int ch = (int)(((k < 4 ? r.x : r.y) >> (8 * (k & 3))) & 0xffu);
        m |= (ch == 'a' || ch == 'c' || ch == 'g' || ch == 't') ? 1u << k : 0u;
    }
    return m;
}

// pairs a workgroup writes per pass: as many whole rows as its lanes cover (pieces = M.row / 16 <= 8 * 32 -- RL <= 1024)
__host__ __device__ inline uint32_t perfect_pairs_per_pass(int row) { return (uint32_t)PERFECT_THREADS / ((uint32_t)row >> 4); }

// Persistent grid.  Lane i of a workgroup keeps piece i % pieces of pair i / pieces of every pass (lanes past the last whole
// row idle); a pass is perfect_pairs_per_pass consecutive pairs, the workgroups take every gridDim-th pass, PERFECT_UNROLL of
// them at a time (descriptors, then windows, then letters, then stores).
__global__ __launch_bounds__(PERFECT_THREADS) void k_perfect(DevModel M, DevGenome g, RunArgs A, const PairDesc *__restrict__ desc) {
    const uint32_t pieces = (uint32_t)M.row >> 4;
    const uint32_t ppp = perfect_pairs_per_pass(M.row);
    const uint32_t pp = threadIdx.x / pieces, k = threadIdx.x - pp * pieces;
    if (pp >= ppp) return;
    const int RL = M.RL;
    // mut_sequence's test at phred 40: error iff m > thr; its leading 8 bits decide unless the draw's digit ties them
    const uint64_t thr = M.mut_thr[PERFECT_PHRED];
    const uint32_t t8 = (uint32_t)(thr >> 45) < 255u ? (uint32_t)(thr >> 45) : 255u;
    const uint32_t q4 = 0x01010101u * PERFECT_PHRED;
    // piece k = bytes 16k .. 16k + 15 of the row: line k >> 3, mate (k >> 2) & 1, read positions 32 (k >> 3) + 8 (k & 3) + 0 .. 7
    const int o = (int)((k >> 2) & 1u);
    const int p0 = (int)(((k >> 3) << 5) + ((k & 3u) << 3));
    const bool live = p0 < RL;  // (pieces past the read length: zeros)
    const uint32_t valid = RL - p0 < 8 ? (1u << (RL - p0)) - 1u : 0xffu;
    const int64_t step = (int64_t)gridDim.x * ppp;
    for (int64_t pair0 = (int64_t)blockIdx.x * ppp + pp; pair0 < A.n_pairs; pair0 += PERFECT_UNROLL * step) {
        PairDesc d[PERFECT_UNROLL];
        uint64_t win[PERFECT_UNROLL];
        int64_t lo[PERFECT_UNROLL];
#pragma unroll
        for (int j = 0; j < PERFECT_UNROLL; ++j) {
            const int64_t pair = pair0 + j * step;
            d[j] = pair < A.n_pairs ? desc[pair] : PairDesc{0, 0, 64u, 0};  // (past the end: "irregular", nothing read)
        }
#pragma unroll
        for (int j = 0; j < PERFECT_UNROLL; ++j) {  // (irregular pairs: k_indel_fixup writes the letters)
            const bool regular = live && !((d[j].meta >> 6) & 1u);
            lo[j] = regular ? perfect_lo(o, d[j], p0) : 0;
            win[j] = regular ? ((uint64_t)g.packed[(lo[j] >> 4) + 1] << 32) | g.packed[lo[j] >> 4] : 0;
        }
#pragma unroll
        for (int j = 0; j < PERFECT_UNROLL; ++j) {
            const int64_t pair = pair0 + j * step;
            if (pair >= A.n_pairs) break;
            if (k == 0) A.desc_out[pair] = d[j];  // (the call's coordinates: iss_output_download_coords)
            uint2 let = make_uint2(0u, 0u);
            if (live && !((d[j].meta >> 6) & 1u)) {
                const bool exc = (d[j].meta >> (4 + o)) & 1u;
                let = perfect_letters(g, o, lo[j], win[j], exc, valid);
                const uint32_t low = exc ? perfect_lower_mask(let) & valid : 0u;
                if (low) {
                    const Addr a = make_addr(A.seed, A.first_ordinal + (uint64_t)pair, d[j].meta >> 16);
                    const u32x4 blk = draw_block(a, K_QM, (uint32_t)(p0 >> 3), 1u);
                    for (uint32_t m = low; m; m &= m - 1u) {
                        const int c = __ffs((int)m) - 1;  // position p0 + c: half c >> 2, byte c & 3
                        const uint32_t e8 = hot_e8(blk, c >> 2, o, c & 3);
                        bool err = e8 > t8;
                        if (e8 == t8) err = error_test_draw(e8, draw_block(a, K_SUB, (uint32_t)(p0 + c), (uint32_t)o)) > thr;
                        if (err) {  // np.random.choice over the identity distribution: the upper-case letter
                            uint32_t &w = c < 4 ? let.x : let.y;
                            w &= ~(0x20u << (8u * (uint32_t)(c & 3)));
                        }
                    }
                }
            }
            uint4 *dst = reinterpret_cast<uint4 *>(A.out[0] + (size_t)pair * (size_t)M.row) + k;
            *dst = make_uint4(let.x, let.y, live ? q4 : 0u, live ? q4 : 0u);
        }
    }
}

}  // namespace iss
