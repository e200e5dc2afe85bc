// Depth slabs (depth_modes.h): k_depth_hist + k_depth_nms find the scene's primary depths — the modes of the depth
// histogram of the resident frame —, k_slab_mask writes the mask of the pixels within slab_mm of one of them.  Integers only: the
// counts, and so the modes, do not depend on the order the workgroups arrive in.
#include <algorithm>

#include "launch.h"
#include "depth_modes.h"

namespace lm {

// The image in units of 8 pixels of a row, one per thread and step: a unit that lies inside its row and starts 16-byte aligned is one
// dwordx4 load, the others (the last of a row whose width is no multiple of 8, every unit of a row that starts unaligned) go pixel by
// pixel.  Neighbouring pixels mostly share a bin, so a thread adds a run of equal bins to the workgroup's LDS table at once; the table
// goes to the global one with one atomic add per non-empty bin.
__global__ __launch_bounds__(256) void k_depth_hist(const DepthHistArgs a, uint32_t units, uint32_t units_per_row) {
    __shared__ uint32_t s_h[kDepthMaxBins];
    for (int b = threadIdx.x; b < a.nbins; b += 256) s_h[b] = 0u;
    __syncthreads();
    uint32_t run_bin = 0u, run_n = 0u;
    auto count = [&](uint32_t d) {
        if (d < (uint32_t)a.near_mm || d >= (uint32_t)a.far_mm) return;        // (near_mm >= 1: depth 0 counts nowhere)
        const uint32_t n = d - (uint32_t)a.near_mm;
        const uint32_t b = a.m_bin ? __umulhi(n, a.m_bin) : n;
        if (b >= (uint32_t)a.nbins) return;
        if (run_n && b == run_bin) { ++run_n; return; }
        if (run_n) atomicAdd(&s_h[run_bin], run_n);
        run_bin = b; run_n = 1u;
    };
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const uint32_t y = u / units_per_row;
        const uint32_t x0 = (u - y * units_per_row) * 8u;
        const uint16_t* p = a.depth + (size_t)y * a.pitch + x0;
        if (x0 + 8u <= (uint32_t)a.W && ((uintptr_t)p & 15u) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            count(v.x & 0xFFFFu); count(v.x >> 16); count(v.y & 0xFFFFu); count(v.y >> 16);
            count(v.z & 0xFFFFu); count(v.z >> 16); count(v.w & 0xFFFFu); count(v.w >> 16);
        } else {
            const int n = min(8, a.W - (int)x0);
            for (int k = 0; k < n; ++k) count(p[k]);
        }
    }
    if (run_n) atomicAdd(&s_h[run_bin], run_n);
    __syncthreads();
    for (int b = threadIdx.x; b < a.nbins; b += 256) {
        const uint32_t c = s_h[b];
        if (c) atomicAdd(&a.hist[b], c);
    }
}

hipError_t launch_depth_hist(const DepthHistArgs& a, hipStream_t s) {
    if (a.W < 1 || a.H < 1 || a.nbins < 1 || a.nbins > kDepthMaxBins) return hipErrorInvalidValue;
    DepthHistArgs k = a;
    if (k.pitch == k.W && (long long)k.W * k.H < (1ll << 30)) { k.W = k.W * k.H; k.H = 1; k.pitch = k.W; }   // contiguous rows: one long row
    const uint32_t upr = ((uint32_t)k.W + 7u) / 8u;
    const uint32_t units = upr * (uint32_t)k.H;
    const uint32_t blocks = std::min<uint32_t>((units + 255u) / 256u, 512u);
    return lm_launch(k_depth_hist, dim3(blocks), dim3(256), 0, s, k, units, upr);
}

// Thread t owns bins t, t + 256, ...: a bit per owned bin says "a mode, not selected yet"; a selection round is a maximum over the
// keys pixels << 32 | (kDepthMaxBins - bin) — most pixels, then the smaller bin — of the bins still marked.
__global__ __launch_bounds__(256) void k_depth_nms(const uint32_t* hist, int nbins, int near_mm, int bin_mm, int window, uint32_t min_pixels,
                                                   int max_modes, uint32_t* out) {
    __shared__ uint32_t s_h[kDepthMaxBins];
    __shared__ unsigned long long s_key[256];
    const int t = threadIdx.x;
    for (int b = t; b < nbins; b += 256) s_h[b] = hist[b];
    __syncthreads();
    uint32_t marked = 0u;
    for (int i = 0; t + 256 * i < nbins; ++i) {
        const int b = t + 256 * i;
        const uint32_t h = s_h[b];
        bool ok = h >= min_pixels;
        for (int j = max(0, b - window); ok && j < b; ++j) ok = h > s_h[j];
        const int last = min(nbins - 1, b + window);
        for (int j = b + 1; ok && j <= last; ++j) ok = h >= s_h[j];
        if (ok) marked |= 1u << i;
    }
    int n = 0;
    for (int k = 0; k < max_modes; ++k) {
        unsigned long long best = 0ull;
        for (int i = 0; i < kDepthMaxBins / 256; ++i)
            if (marked >> i & 1u) {
                const int b = t + 256 * i;
                const unsigned long long key = ((unsigned long long)s_h[b] << 32) | (uint32_t)(kDepthMaxBins - b);
                best = key > best ? key : best;
            }
        s_key[t] = best;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) { const unsigned long long o = s_key[t + s]; if (o > s_key[t]) s_key[t] = o; }
            __syncthreads();
        }
        const unsigned long long w = s_key[0];
        __syncthreads();
        if (!w) break;                                         // (a mode has min_pixels >= 1 pixels: its key is not 0)
        const int b = kDepthMaxBins - (int)(uint32_t)w;
        if ((b & 255) == t) marked &= ~(1u << (b >> 8));
        if (t == 0) {
            out[4 + 3 * k] = (uint32_t)b;
            out[5 + 3 * k] = (uint32_t)(near_mm + b * bin_mm + bin_mm / 2);
            out[6 + 3 * k] = (uint32_t)(w >> 32);
        }
        ++n;
    }
    if (t == 0) out[0] = (uint32_t)n;
}

hipError_t launch_depth_nms(const uint32_t* hist, int nbins, int near_mm, int bin_mm, int window, uint32_t min_pixels, int max_modes,
                            uint32_t* out, hipStream_t s) {
    if (nbins < 1 || nbins > kDepthMaxBins || max_modes < 1 || max_modes > kDepthMaxModes || window < 0 || min_pixels < 1u) return hipErrorInvalidValue;
    return lm_launch(k_depth_nms, dim3(1), dim3(256), 0, s, hist, nbins, near_mm, bin_mm, std::min(window, nbins), min_pixels, max_modes, out);
}

// Eight pixels per thread: one dwordx4 of depths in, one dwordx2 per output mask out.
__global__ __launch_bounds__(256) void k_slab_mask(const SlabMaskArgs a) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= a.n / 8u) return;
    const uint4 v = reinterpret_cast<const uint4*>(a.depth)[u];
    const uint32_t d[8] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16, v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16};
    uint32_t in[2] = {0u, 0u};                                 // 0xFF per pixel inside the slab
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (d[k] != 0u && (int)d[k] >= a.lo && (int)d[k] <= a.hi) in[k >> 2] |= 0xFFu << (8 * (k & 3));
    auto keep = [](uint32_t m) -> uint32_t { return (((((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u) >> 7) * 0xFFu; };   // 0xFF per non-zero mask byte
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        if (o >= a.n_out) break;
        uint2 m = make_uint2(in[0], in[1]);
        if (a.user[o]) {
            const uint2 um = reinterpret_cast<const uint2*>(a.user[o])[u];
            m.x &= keep(um.x); m.y &= keep(um.y);
        }
        reinterpret_cast<uint2*>(a.out[o])[u] = m;
    }
}

hipError_t launch_slab_mask(const SlabMaskArgs& a, hipStream_t s) {
    if (a.n == 0 || a.n % 8u || a.n_out < 1 || a.n_out > 3 || ((uintptr_t)a.depth & 15u)) return hipErrorInvalidValue;
    for (int o = 0; o < a.n_out; ++o)
        if (!a.out[o] || ((uintptr_t)a.out[o] & 7u) || ((uintptr_t)a.user[o] & 7u)) return hipErrorInvalidValue;
    return lm_launch(k_slab_mask, dim3((a.n / 8u + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace lm
