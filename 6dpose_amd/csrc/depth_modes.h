// Depth slabs: the depth histogram of the resident frame and its 1-D NMS (the scene's primary depths), and the slab
// mask — the pixels within slab_mm of a primary depth — written on the device at the frame's aligned size.  Kernels: depth_modes.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lm {

constexpr int kDepthMaxBins = 4096;           // bins of the histogram: one workgroup's LDS table (16 KB)
constexpr int kDepthMaxModes = 16;
constexpr int kDepthModeWords = 4 + 3 * kDepthMaxModes;   // the record block: [0] = number of modes, [4 + 3 k ..] = {bin, depth_mm, pixels} of mode k

struct DepthHistArgs {
    const uint16_t* depth;                    // H rows of `pitch` elements, the first W of a row are the image
    int W, H, pitch;
    int near_mm, far_mm, bin_mm, nbins;       // near_mm <= d < far_mm counts in bin (d - near_mm) / bin_mm  (< nbins)
    uint32_t m_bin;                           // ceil(2^32 / bin_mm), 0 for bin_mm = 1: n / bin_mm = umulhi(n, m_bin), exact for n, bin_mm <= 65536
    uint32_t* hist;                           // [nbins], zero before the launch
};
// hist[b] += pixels of bin b: per-workgroup counts in LDS, one atomic add per non-empty bin and workgroup.  Any W, H, pitch and alignment.
[[nodiscard]] hipError_t launch_depth_hist(const DepthHistArgs& a, hipStream_t s);

// One workgroup: bin b is a mode iff hist[b] >= min_pixels, hist[b] > hist[j] for j in [b - window, b) and hist[b] >= hist[j] for j in
// (b, b + window] (bins outside [0, nbins) do not exist); out = the max_modes modes with the most pixels, ties towards the smaller bin,
// in that order, as kDepthModeWords words.
[[nodiscard]] hipError_t launch_depth_nms(const uint32_t* hist, int nbins, int near_mm, int bin_mm, int window, uint32_t min_pixels, int max_modes,
                                          uint32_t* out, hipStream_t s);

// out[k][i] = (depth[i] != 0 && lo <= depth[i] <= hi && (!user[k] || user[k][i])) ? 255 : 0 for the n_out outputs; n pixels, a multiple of 8,
// every pointer 16-byte (depth) / 8-byte (masks) aligned.
struct SlabMaskArgs {
    const uint16_t* depth;
    uint32_t n;
    int lo, hi;
    int n_out;
    const uint8_t* user[3];
    uint8_t* out[3];
};
[[nodiscard]] hipError_t launch_slab_mask(const SlabMaskArgs& a, hipStream_t s);

}  // namespace lm
