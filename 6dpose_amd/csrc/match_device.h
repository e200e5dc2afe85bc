// Device helpers that the matching units share (match_bytes.hip, match_bits.hip, match_wide.hip): the score, the buffer loads of the arenas,
// the wave's exclusive scan and the bit-sliced counters of the bit-plane kernels.  The STAGES that the bit-plane kernels share (template head,
// hit test and emission of the coarse pass; window, arg-max and epilogue of the refinement; the packers' indexing) are in match_planes.h, which
// match_bits.hip and match_wide.hip include instead of this file.  What one unit alone uses stays in that unit.  gfx950 only.
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

// ---- bit-sliced counters of the bit-plane kernels (match_bits.hip, match_wide.hip) ----
// carry-save adder: two v_bitop3_b32 (gfx950's ternary logic op; truth tables with a = 0xF0, b = 0xCC, c = 0xAA: parity 0x96, majority 0xE8)
static __device__ __forceinline__ void csa(uint32_t& sum, uint32_t& carry, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t s = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
    carry = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
    sum = s;
}
// eight 1-bit inputs into {ones, twos, fours}; returns the carry of weight 8 (7 carry-save adders = 14 v_bitop3)
static __device__ __forceinline__ uint32_t add8(const uint32_t (&x)[8], uint32_t& ones, uint32_t& twos, uint32_t& fours) {
    uint32_t ta, tb, fa, fb, e;
    csa(ones, ta, ones, x[0], x[1]);
    csa(ones, tb, ones, x[2], x[3]);
    csa(twos, fa, twos, ta, tb);
    csa(ones, ta, ones, x[4], x[5]);
    csa(ones, tb, ones, x[6], x[7]);
    csa(twos, fb, twos, ta, tb);
    csa(fours, e, fours, fa, fb);
    return e;
}
// Counter of kN bits per position: c[0..3] = ones, twos, fours, eights, c[4..] = 16s and up.  Two carries of weight 8 (16 features) enter
// through one more adder and ONE ripple of the sixteens (Harley-Seal: 2.5 operations per input instead of 3.25 with a ripple per 8).
template <int kN>
static __device__ __forceinline__ void add_eights2(uint32_t (&c)[kN], uint32_t e1, uint32_t e2) {
    uint32_t k16;
    csa(c[3], k16, c[3], e1, e2);
#pragma unroll
    for (int k = 4; k < kN; ++k) { const uint32_t t = c[k] & k16; c[k] ^= k16; k16 = t; }
}
template <int kN>
static __device__ __forceinline__ void add_eights1(uint32_t (&c)[kN], uint32_t e1) {
    uint32_t k16 = c[3] & e1;
    c[3] ^= e1;
#pragma unroll
    for (int k = 4; k < kN; ++k) { const uint32_t t = c[k] & k16; c[k] ^= k16; k16 = t; }
}

// The bit-sliced sum S = a n_a + 4 n_4 of two bit-sliced counts (kA = a: the weight of the low plane, lm_kernels.h resp_pack; 1 for the
// default table 4 1 0 0 0, whose instantiation is the code it always was).  n_a + n_4 <= features, so kN + 3 bits hold any of them.
template <int kA, int kN>
static __device__ __forceinline__ void weighted_sum(uint32_t (&S)[kN + 3], const uint32_t (&na)[kN], const uint32_t (&n4)[kN]) {
    constexpr int kS = kN + 3;
    uint32_t carry = 0;
    if (kA == 1) {
        S[0] = na[0]; S[1] = na[1];
#pragma unroll
        for (int k = 2; k < kS; ++k) csa(S[k], carry, k < kN ? na[k] : 0u, k - 2 < kN ? n4[k - 2] : 0u, carry);
    } else if (kA == 2) {
        S[0] = 0u; S[1] = na[0];
#pragma unroll
        for (int k = 2; k < kS; ++k) csa(S[k], carry, k - 1 < kN ? na[k - 1] : 0u, k - 2 < kN ? n4[k - 2] : 0u, carry);
    } else {                                                        // 3 n_a = n_a + 2 n_a first (kN + 2 bits), then + 4 n_4
        uint32_t t[kN + 2];
        t[0] = na[0];
#pragma unroll
        for (int k = 1; k < kN + 2; ++k) csa(t[k], carry, k < kN ? na[k] : 0u, k - 1 < kN ? na[k - 1] : 0u, carry);
        carry = 0;
        S[0] = t[0]; S[1] = t[1];
#pragma unroll
        for (int k = 2; k < kS; ++k) csa(S[k], carry, k < kN + 2 ? t[k] : 0u, k - 2 < kN ? n4[k - 2] : 0u, carry);
    }
}

// ---- what the part kernels add (match_parts.hip): sums of sums, comparisons against a per-lane bound, a small counter of passes ----
// S += A, both bit-sliced (a ripple of carry-save adders; the caller knows that kS bits hold the sum)
template <int kS>
static __device__ __forceinline__ void sliced_add(uint32_t (&S)[kS], const uint32_t (&A)[kS]) {
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < kS; ++k) csa(S[k], carry, S[k], A[k], carry);
}
// the positions whose bit-sliced value is >= r, r per lane (coarse_hit_mask, match_planes.h, does it for a wave-uniform r); r >= 2^kS: none
template <int kS>
static __device__ __forceinline__ uint32_t sliced_ge(const uint32_t (&S)[kS], int r) {
    uint32_t gt = 0, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int k = kS - 1; k >= 0; --k) {
        const uint32_t b = 0u - (((uint32_t)r >> k) & 1u);          // all ones where bit k of r is set
        gt |= eq & S[k] & ~b;
        eq &= ~(S[k] ^ b);
    }
    return r < (1 << kS) ? (gt | eq) : 0u;
}
// a bit-sliced counter 0..4 of one-bit inputs {q0, q1, q2}: += x; and the positions whose count is >= m (m = 1..4)
static __device__ __forceinline__ void count3_add(uint32_t& q0, uint32_t& q1, uint32_t& q2, uint32_t x) {
    const uint32_t t = q0 & x;
    q0 ^= x;
    q2 ^= q1 & t;
    q1 ^= t;
}
static __device__ __forceinline__ uint32_t count3_ge(uint32_t q0, uint32_t q1, uint32_t q2, int m) {
    return m <= 1 ? (q0 | q1 | q2) : m == 2 ? (q1 | q2) : m == 3 ? (q2 | (q1 & q0)) : q2;
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
