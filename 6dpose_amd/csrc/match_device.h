// Device helpers that both matching units use (match_bytes.hip, match_bits.hip): the score, the buffer loads of the arenas and
// the wave's exclusive scan.  What one unit alone uses stays in that unit.  gfx950 only.
#pragma once
#include "lm_kernels.h"

namespace lm {

// score = (raw * 100.f) / (4 * num_features)  — LL.cpp:1842, 1918; IEEE single, no contraction
static __device__ __forceinline__ float score_of(int raw, int nfeat) {
    return __fdiv_rn(__fmul_rn((float)raw, 100.f), (float)(4 * nfeat));
}

// The gathers of the three fast paths go through buffer loads: `buffer_load_dwordx4 v, v_off, s[rsrc], s_off offen` takes the
// arena as a resource in SGPRs, ONE 32-bit per-lane offset (constant for the whole item) and the feature's wave-uniform byte
// offset in an SGPR.  As global loads the compiler kept a 64-bit VGPR address per load in flight — 16 VGPRs for a batch of 8 and
// two VALU adds per load — which is what put k_local at 67 and k_coarse at 96 VGPRs (occupancy 7 / 5 waves per SIMD); the
// kernels' speed follows their occupancy (profiles/r02_local_experiments.txt).
using BufRsrc = __amdgpu_buffer_rsrc_t;
static __device__ __forceinline__ BufRsrc make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1 /* no range check: 2^32 - 1 bytes */, 0x00020000 /* gfx9: raw dwords */);
}
static __device__ __forceinline__ uint4 ld_buf16(BufRsrc r, uint32_t lane_off, uint32_t uniform_off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)lane_off, (int)uniform_off, 0);
    uint4 u;
    __builtin_memcpy(&u, &v, 16);
    return u;
}

// exclusive prefix of `mine` over the lanes of the wave; total = the wave's sum
static __device__ __forceinline__ int wave_excl_scan(int mine, int lane, int& total) {
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    total = __shfl(incl, 63, 64);
    return incl - mine;
}

}  // namespace lm
