// iss_pack_group.hip.h -- k_pack_group: a group of records (draft contigs) packed in one launch (iss_genome_upload_group).
//
// The host stages the group's letters in iss_generate_batch's arena layout: the first record at coordinate 64, every record
// at a multiple of 32 bases, at least 64 bases of 'A' between records and behind the last one.  One copy brings the letters
// and the records' start coordinates to the device; this kernel then writes the arena's packed words and mask words:
//   * one lane per 32 arena bases: two 16-byte loads, two packed words (one 8-byte store), one mask word;
//   * 'A' padding packs to code 0 with no mask bit, so a lane of padding writes zeros and looks nothing up;
//   * a lane with mask bits (IUPAC / lower case / letters outside util.rev_comp's alphabet, iss/util.py:57-88) finds its
//     record by binary search over the start coordinates -- a 32-base span holds letters of at most one record, records
//     being 32-aligned with padding between them -- and adds its counts to the record's row of the status table:
//     status[2 r] letters outside the alphabet, status[2 r + 1] exception letters (all mask bits).
#pragma once

namespace iss {

constexpr int PACK_GROUP_THREADS = 256;

// letter -> 2-bit code (A,T,C,G = 0..3); every other byte sets the mask bit; *bad counts those outside the alphabet
__device__ __forceinline__ void pack_group_byte(uint32_t c, int i, uint32_t &pk, uint32_t &mk, uint32_t &bad) {
    uint32_t code = 0;
    switch (c) {
        case 'A': code = 0; break; case 'T': code = 1; break; case 'C': code = 2; break; case 'G': code = 3; break;
        default: {
            mk |= 1u << i;
            const uint32_t u = c & ~0x20u;
            const bool letter = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
            const bool ok = letter && (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'Y' || u == 'R' || u == 'W' ||
                                       u == 'S' || u == 'K' || u == 'M' || u == 'N' || u == 'B' || u == 'V' || u == 'D' ||
                                       u == 'H');
            bad += ok ? 0u : 1u;
        }
    }
    pk |= code << ((i & 15) * 2);
}

// ascii: the staged arena (16-byte aligned), n_words = arena bases / 32; starts[0 .. n - 1]: ascending start coordinates;
// packed / mask: the arena's word 0 (coordinate 0); status: 2 x n counters, zeroed before the launch
__global__ __launch_bounds__(PACK_GROUP_THREADS) void k_pack_group(const uint8_t *__restrict__ ascii, int64_t n_words,
                                                                   const int64_t *__restrict__ starts, int32_t n,
                                                                   uint32_t *__restrict__ packed, uint32_t *__restrict__ mask,
                                                                   unsigned long long *__restrict__ status) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(ascii + w * 32);
    const uint4 v[2] = {src[0], src[1]};
    uint32_t pk[2] = {0, 0}, mk = 0, bad = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t q[4] = {v[h].x, v[h].y, v[h].z, v[h].w};
#pragma unroll
        for (int j = 0; j < 16; ++j) pack_group_byte((q[j >> 2] >> (8 * (j & 3))) & 0xffu, h * 16 + j, pk[h], mk, bad);
    }
    *reinterpret_cast<uint2 *>(packed + 2 * w) = make_uint2(pk[0], pk[1]);
    mask[w] = mk;
    if (!mk) return;
    const int64_t base = w * 32;
    int lo = 0, hi = n - 1;  // the last record starting at or before `base`
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= base) lo = mid; else hi = mid - 1;
    }
    atomicAdd(&status[2 * lo + 1], (unsigned long long)__popc(mk));
    if (bad) atomicAdd(&status[2 * lo], (unsigned long long)bad);
}

}  // namespace iss
