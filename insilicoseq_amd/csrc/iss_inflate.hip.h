// iss_inflate.hip.h -- k_bgzf_inflate: BGZF members inflated on the device (the BAM input of `model`, BGZF FASTQ in `report`).  The
// decoder is iss_inflate_core.h, the text the host twin runs; this file gives it 64 lanes, LDS and a launch geometry.
//
// One wavefront per member, INF_WAVES of them per workgroup, members dealt to the waves round robin.  A member's symbol stream is
// serial, so all 64 lanes decode it side by side from the same bits (uniform branches, broadcast loads) and part only where there is
// width: table fills, match and stored copies, the CRC slices, the stores of the ring to the output.  The window is a 32 KiB ring in
// LDS per wave -- a back-reference never reads the output in global memory, so there is no question of when a wave's own stores
// become visible to its loads -- and with the tables a wave holds sizeof(Work) = 36.7 KiB: four waves and the shared CRC tables fill
// 147 KiB of a CU's 160 KiB, one workgroup per CU, one wave per SIMD.  DESIGN.md section 27.
#pragma once

#include "iss_inflate_core.h"

namespace iss {
namespace inf {

constexpr int INF_WAVES = 4;
constexpr int INF_THREADS = 64 * INF_WAVES;

struct InflateShared {
    uint32_t crc_tab[256];
    uint32_t ops[iss_inf::N_OPS * 32];
    iss_inf::Work w[INF_WAVES];
};
constexpr size_t INF_LDS = sizeof(InflateShared);
static_assert(INF_LDS <= 160 * 1024, "k_bgzf_inflate: a workgroup's LDS");

struct InflateArgs {
    const uint8_t *in;        // the group's compressed bytes
    uint8_t *out;             // the group's inflated bytes: member m at out_off[m], isize[m] of them
    const uint32_t *pay_off;  // per member: its DEFLATE payload in `in`,
    const uint32_t *pay_len;
    const uint32_t *out_off;  // the exclusive sum of isize,
    const uint32_t *isize;
    const uint32_t *crc;      // the footer's CRC-32
    uint8_t *status;          // ISS_BGZF_* per member
    const uint32_t *ops;      // iss_inf::crc_tables
    unsigned long long *bad;  // min over the bad members of all feeds: (member << 8) | status
    uint32_t n_members;
    unsigned long long member_base;  // members fed before this group
};

// Between a piece that writes a wave's LDS and a piece that reads it.  LDS operations of one wave complete in the order they were
// issued; the fence keeps the compiler from moving them across.
struct WaveSync {
    __device__ __forceinline__ void operator()() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

__global__ __launch_bounds__(INF_THREADS) void k_bgzf_inflate(InflateArgs A) {
    extern __shared__ __align__(16) uint8_t inflate_lds[];
    InflateShared &S = *reinterpret_cast<InflateShared *>(inflate_lds);
    for (uint32_t i = threadIdx.x; i < 256; i += INF_THREADS) S.crc_tab[i] = iss_inf::crc_byte_entry(i);
    for (uint32_t i = threadIdx.x; i < iss_inf::N_OPS * 32; i += INF_THREADS) S.ops[i] = A.ops[i];
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    for (uint32_t m = blockIdx.x * INF_WAVES + (uint32_t)wave; m < A.n_members; m += gridDim.x * INF_WAVES) {
        uint32_t crc_got = 0;
        const int st = iss_inf::inflate_member(A.in + A.pay_off[m], A.pay_len[m], A.out + A.out_off[m], A.isize[m], A.crc[m], S.w[wave],
                                                   S.crc_tab, S.ops, lane, 64, WaveSync{}, &crc_got);
        if (lane == 0) {
            A.status[m] = (uint8_t)st;
            if (st) atomicMin(A.bad, ((A.member_base + m) << 8) | (unsigned long long)st);
        }
    }
}

}  // namespace inf
}  // namespace iss
