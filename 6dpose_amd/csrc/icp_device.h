// Device helpers and constants that two or more of the ICP translation units use (icp_clouds.hip, icp.hip, icp_eval.hip,
// icp_team.hip), and the launch helper of icp_clouds.hip that launch_icp_prepare (icp.hip) calls.  What one unit
// alone uses stays in that unit.  gfx950 only.
#pragma once
#include "icp_kernels.h"

namespace lm {

// RegistrationICP, shared by the sliced evaluation (icp_eval.hip) and the team kernel (icp_team.hip)
constexpr double kFarMargin = 1.2;  // search radius (x max_dist) of a source point that has no correspondence (1.5: 49 columns per search instead of 36; profiles/r02_icp_experiments.txt)
constexpr int kClasses = 8;         // search-cost classes of the queue (by overlapped grid columns)

static __device__ __forceinline__ double sqdist(double ax, double ay, double az, double bx, double by, double bz) {
    double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

static __device__ __forceinline__ double shfl_xor_d(double v, int m) { return __shfl_xor(v, m, 64); }

// Exclusive prefix of a per-thread flag in thread order; `total` = number of flags set in the workgroup.
static __device__ __forceinline__ int block_scan_flag(bool flag, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int within = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const int c = s_wave[w];
        if (w < wave) base += c;
        tot += c;
    }
    total = tot;
    return base + within;
}

static __device__ __forceinline__ int grid_coord(double v, double mn, double inv, int g) {
    const double f = floor((v - mn) * inv);
    return f >= 0.0 ? (f < (double)g ? (int)f : g - 1) : 0;      // NaN -> 0, never UB
}

// quantised depth of a target point: the z step of the search grid's sort key (k_icp_grid), found again by the searches
static __device__ __forceinline__ int zq_of(double z, double minz, double inv_z, int zq_max) {
    const double f = floor((z - minz) * inv_z);
    return f >= 0.0 ? (f < (double)zq_max ? (int)f : zq_max) : 0;      // NaN -> 0
}

// DPP moves inside a row of lanes (0xB1: xor 1, 0x4E: xor 2, 0x141: mirror within the half row) and the 64-bit xor shuffle
template <int CTRL> static __device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL> static __device__ __forceinline__ double dpp_mov(double v) {
    return __hiloint2double(dpp_mov<CTRL>(__double2hiint(v)), dpp_mov<CTRL>(__double2loint(v)));
}
template <int CTRL> static __device__ __forceinline__ unsigned long long dpp_mov64(unsigned long long v);
template <int CTRL> static __device__ __forceinline__ unsigned long long dpp_mov(unsigned long long v) { return dpp_mov64<CTRL>(v); }
template <int CTRL> static __device__ __forceinline__ unsigned long long dpp_mov64(unsigned long long v) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)v, CTRL, 0xF, 0xF, false);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)hi << 32) | lo;
}
static __device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, m, 64), hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// Sum of 32 per-lane values over the wave with 32 shuffles instead of 6 x 32: every step halves the
// number of values a lane carries (lanes whose bit `off` is set keep the upper half).  Afterwards lane l
// holds the wave total of value (l >> 1).
template <int N, int OFF, int M>
static __device__ __forceinline__ void reduce_halve(double (&v)[M], int lane) {
    const bool hi = (lane & OFF) != 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double send = hi ? v[k] : v[k + N];
        const double keep = hi ? v[k + N] : v[k];
        v[k] = keep + shfl_xor_d(send, OFF);
    }
}
static __device__ __forceinline__ double wave_reduce32(double (&v)[32], int lane) {
    reduce_halve<16, 32>(v, lane);
    reduce_halve<8, 16>(v, lane);
    reduce_halve<4, 8>(v, lane);
    reduce_halve<2, 4>(v, lane);
    reduce_halve<1, 2>(v, lane);
    return v[0] + shfl_xor_d(v[0], 1);
}

// The first launches of launch_icp_prepare: box, dilated mask and back-projection of every hypothesis (icp_clouds.hip)
[[nodiscard]] hipError_t launch_icp_clouds(const IcpBuffers& B, int count, int W, int H, int flags, hipStream_t s);

}  // namespace lm
