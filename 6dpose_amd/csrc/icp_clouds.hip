// The clouds of poseRefine::process (reference LL.cpp:43-104) and the glue in front of them.
//   k_icp_bind          pipeline glue: the detections kept by the on-device NMS become ICP hypotheses
//   k_icp_bbox          bounding box of modelDepth > 0                                                      (LL.cpp:43-50)
//   k_icp_model_boxes   the same box, once per resident model image at upload (launch_icp_model_boxes)
//   k_icp_points<>      dilated mask, back-projection, raster-order compaction, centroids: a counting and a
//                       writing launch                                                                      (LL.cpp:52-104)
//   k_icp_points_fused  the same in one launch: the strips publish their counts to each other
// launch_icp_prepare (icp.hip) starts with launch_icp_clouds.
// Part of poseRefine::process on gfx950 (reference LL.cpp:27-155; the stages and their files: icp_kernels.h).  The cloud arithmetic is
// Open3D's (un-vendored), restated per SURVEY Appendix B with the deterministic rules of DESIGN.md §5 (shared with
// oracle/linemod_oracle.py).  All arithmetic is double like Open3D's (f64 VALU; nothing here is a dense contraction, so no MFMA).
#include <limits.h>

#include "launch.h"
#include "icp_device.h"
#include "icp_kernels.h"
#include "knobs.h"
#include "lm_kernels.h"

namespace lm {

constexpr int kDilate = 4;         // LL.cpp:45 (9x9 dilation)

static __device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------
// k_icp_bbox: bounding rectangle of modelDepth > 0 (the 9x9 dilation only grows it by 4, LL.cpp:43-50)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_icp_bbox(IcpBuffers B, int W, int H) {
    const int h = blockIdx.y;
    const int status = B.st[h].status, slot = B.in[h].model_slot;   // (both loads leave together)
    if (status != 0) return;                                       // slot without a detection (pipeline)
    // the box of a resident image is worked out once: a later run finds it in model_bbox (k_icp_points<false> of the first run put it there
    // once this kernel was through; the host clears the state word when the image changes)
    if (blockIdx.x == 0 && threadIdx.x < kIcpStrips) B.strip_pub[(size_t)h * kIcpStrips + threadIdx.x] = 0;   // (k_icp_points_fused: the strips' counts, not yet known)
    const int* known = B.model_bbox + (size_t)slot * 8;
    if (known[4] == 1) {
        if (blockIdx.x == 0 && threadIdx.x < 4) B.st[h].bbox[threadIdx.x] = threadIdx.x < 2 ? INT_MAX - known[threadIdx.x] : known[threadIdx.x] - 1;
        return;
    }
    const uint16_t* img = B.models + (size_t)slot * W * H;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    const bool vec = (W & 7) == 0;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const uint16_t* row = img + (size_t)y * W;
        for (int x = threadIdx.x * 8; x < W; x += blockDim.x * 8) {
            uint16_t px[8];
            if (vec) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + x);
                px[0] = v.x & 0xFFFF; px[1] = v.x >> 16; px[2] = v.y & 0xFFFF; px[3] = v.y >> 16;
                px[4] = v.z & 0xFFFF; px[5] = v.z >> 16; px[6] = v.w & 0xFFFF; px[7] = v.w >> 16;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) px[k] = x + k < W ? row[x + k] : 0;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (px[k]) {
                    x0 = min(x0, x + k); x1 = max(x1, x + k);
                    y0 = min(y0, y); y1 = max(y1, y);
                }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && x1 >= 0) {
        int* bb = B.st[h].bbox;
        atomicMin(&bb[0], x0); atomicMin(&bb[1], y0); atomicMax(&bb[2], x1); atomicMax(&bb[3], y1);
    }
}

// k_icp_model_boxes: the same rectangle for resident model images AT UPLOAD (lm_icp_set_models, the pipeline's view upload): 32 workgroups
// per image, model_bbox[slot] = INT_MAX - x0, INT_MAX - y0, x1 + 1, y1 + 1 (so that a cleared record is the empty box and every word
// only grows: atomicMax), state 1.  A run whose slots all came that way does not launch k_icp_bbox at all: reading a 614 KB image per
// hypothesis and run was 12 us of every run for a fact that changes when the image does.
__global__ void __launch_bounds__(256)
k_icp_model_boxes(const uint16_t* __restrict__ models, int* __restrict__ model_bbox, int first_slot, int W, int H) {
    const int slot = first_slot + (int)blockIdx.y;
    const uint16_t* img = models + (size_t)slot * W * H;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    const bool vec = (W & 7) == 0;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const uint16_t* row = img + (size_t)y * W;
        for (int x = threadIdx.x * 8; x < W; x += 256 * 8) {
            uint16_t px[8];
            if (vec) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + x);
                px[0] = v.x & 0xFFFF; px[1] = v.x >> 16; px[2] = v.y & 0xFFFF; px[3] = v.y >> 16;
                px[4] = v.z & 0xFFFF; px[5] = v.z >> 16; px[6] = v.w & 0xFFFF; px[7] = v.w >> 16;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) px[k] = x + k < W ? row[x + k] : 0;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (px[k]) {
                    x0 = min(x0, x + k); x1 = max(x1, x + k);
                    y0 = min(y0, y); y1 = max(y1, y);
                }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    int* known = model_bbox + (size_t)slot * 8;
    if ((threadIdx.x & 63) == 0 && x1 >= 0) {
        atomicMax(&known[0], INT_MAX - x0); atomicMax(&known[1], INT_MAX - y0); atomicMax(&known[2], x1 + 1); atomicMax(&known[3], y1 + 1);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) known[4] = 1;        // (read by the kernels of a later launch)
}

hipError_t launch_icp_model_boxes(const uint16_t* models, int* model_bbox, int first_slot, int count, int W, int H, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    LAUNCH_TRY(hipMemsetAsync(model_bbox + (size_t)first_slot * 8, 0, (size_t)count * 8 * sizeof(int), s));
    return lm_launch(k_icp_model_boxes, dim3(32, count), dim3(256), 0, s, models, model_bbox, first_slot, W, H);
}

// ---------------------------------------------------------------------------------------------
// k_icp_points (LL.cpp:52-104): raster scan of the dilated bounding box; model point where
// modelDepth > 0, scene point where the dilated mask is set and sceneDepth (window shifted by
// detect - 4, clamped at 0) > 0; compaction keeps raster order; centroid difference = init_guess.
// The box is cut into kIcpStrips row strips, one workgroup each: pass 0 counts the points of every
// strip, pass 1 starts each strip at the sum of the counts before it and writes points + centroid sums
// (k_icp_grid adds the strips' sums in order -> init_guess).
// ---------------------------------------------------------------------------------------------
constexpr int kPtsWG = 256;

template <bool kWrite>
__global__ void __launch_bounds__(kPtsWG)
k_icp_points(IcpBuffers B, int W, int H, int flags) {
    __shared__ int s_wave[8];
    __shared__ double s_red[kPtsWG / 64][7];
    __shared__ double s_ext[kPtsWG / 64][12];
    __shared__ int s_tot[2];
    const int h = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x;
    IcpState& S = B.st[h];
    if (S.status != 0) return;
    const IcpIn I = B.in[h];
    const int x0 = S.bbox[0], y0 = S.bbox[1], x1 = S.bbox[2], y1 = S.bbox[3];
    if (!kWrite && strip == 0 && tid == 0) {                       // k_icp_bbox is through: the box of this image is known from now on
        int* known = B.model_bbox + (size_t)B.in[h].model_slot * 8;
        if (known[4] == 0) { known[0] = INT_MAX - x0; known[1] = INT_MAX - y0; known[2] = x1 + 1; known[3] = y1 + 1; __threadfence(); known[4] = 1; }
    }
    if (x1 < 0) {                                                  // pass 1 never gets here: pass 0 set the status
        if (strip == 0 && tid == 0) { S.status = 2; S.n_model = 0; S.n_scene = 0; }
        return;
    }
    const int bx0 = max(x0 - kDilate, 0), by0 = max(y0 - kDilate, 0);
    const int bx1 = min(x1 + kDilate, W - 1), by1 = min(y1 + kDilate, H - 1);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    if (I.dx + bw >= W || I.dy + bh >= H) {                       // LL.cpp:52-55
        if (strip == 0 && tid == 0) { S.status = 1; S.n_model = 0; S.n_scene = 0; }
        return;
    }
    const uint16_t* model = B.models + (size_t)I.model_slot * W * H;
    const uint16_t* scene = B.scene;
    int* cnt = B.strip_cnt + ((size_t)h * kIcpStrips) * 2;
    const int r_lo = (int)((long long)bh * strip / kIcpStrips), r_hi = (int)((long long)bh * (strip + 1) / kIcpStrips);
    const int p_lo = r_lo * bw, p_hi = r_hi * bw;
    const bool keep_scene = (flags & 1) != 0;

    if (!kWrite) {
        int cm = 0, cs = 0;
        for (int p = p_lo + tid; p < p_hi; p += kPtsWG) {
            const int r = p / bw, c = p - r * bw;
            const int mr = r + by0, mc = c + bx0;
            const int sr = max(r + I.dy - kDilate, 0), sc = max(c + I.dx - kDilate, 0);
            const uint16_t md = model[(size_t)mr * W + mc];
            const uint16_t sd = scene[(size_t)sr * W + sc];
            cm += md > 0;
            if (sd > 0 && keep_scene) {
                bool in_mask = md > 0;
                if (!in_mask) {                                   // dilate(modelDepth > 0, 9x9) at (mr, mc)
                    const int ya = max(mr - kDilate, 0), yb = min(mr + kDilate, H - 1);
                    const int xa = max(mc - kDilate, 0), xb = min(mc + kDilate, W - 1);
                    for (int yy = ya; yy <= yb && !in_mask; ++yy)
                        for (int xx = xa; xx <= xb; ++xx)
                            if (model[(size_t)yy * W + xx]) { in_mask = true; break; }
                }
                cs += in_mask;
            }
        }
        if (tid < 2) s_tot[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cm += __shfl_xor(cm, o, 64); cs += __shfl_xor(cs, o, 64); }
        if ((tid & 63) == 0) { atomicAdd(&s_tot[0], cm); atomicAdd(&s_tot[1], cs); }
        __syncthreads();
        if (tid < 2) cnt[strip * 2 + tid] = s_tot[tid];
        return;
    }

    if (strip == 0 && tid < 2 * kIcpSortGroups) B.sort_look[(size_t)h * 2 * kIcpSortGroups + tid] = 0;   // (k_icp_voxel_wide: voxel counts of the groups, not yet known)
    const double anchor = model[(size_t)(H / 2) * W + W / 2] / 1000.0;   // LL.cpp:62
    double* mp = B.model_pts + (size_t)h * B.cap * 3;
    double* sp = B.scene_pts + (size_t)h * B.cap * 3;
    int nm = 0, nsn = 0, tot_m = 0, tot_s = 0;
    for (int k = 0; k < kIcpStrips; ++k) {
        const int a = cnt[k * 2], b2 = cnt[k * 2 + 1];
        if (k < strip) { nm += a; nsn += b2; }
        tot_m += a; tot_s += b2;
    }
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};     // model xyz, scene-near-anchor xyz, its count
    double ext[12] = {1e300, 1e300, 1e300, -1e300, -1e300, -1e300, 1e300, 1e300, 1e300, -1e300, -1e300, -1e300};   // min, max of the strip's model points, of its scene points
    for (int base = p_lo; base < p_hi; base += kPtsWG) {
        const int p = base + tid;
        bool is_m = false, is_s = false;
        double mx = 0, my = 0, mz = 0, sx = 0, sy = 0, sz = 0;
        if (p < p_hi) {
            const int r = p / bw, c = p - r * bw;
            const int mr = r + by0, mc = c + bx0;
            const int sr = max(r + I.dy - kDilate, 0), sc = max(c + I.dx - kDilate, 0);
            const uint16_t md = model[(size_t)mr * W + mc];
            const uint16_t sd = scene[(size_t)sr * W + sc];
            if (md > 0) {
                is_m = true;
                mz = md / 1000.0;
                // (int - float) / float evaluated in float, then * double (LL.cpp:79-80)
                mx = (double)__fdiv_rn(__fsub_rn((float)mc, I.mK[2]), I.mK[0]) * mz;
                my = (double)__fdiv_rn(__fsub_rn((float)mr, I.mK[5]), I.mK[4]) * mz;
                acc[0] += mx; acc[1] += my; acc[2] += mz;
                ext[0] = fmin(ext[0], mx); ext[1] = fmin(ext[1], my); ext[2] = fmin(ext[2], mz);
                ext[3] = fmax(ext[3], mx); ext[4] = fmax(ext[4], my); ext[5] = fmax(ext[5], mz);
            }
            if (sd > 0) {
                bool in_mask = md > 0;
                if (!in_mask) {                                   // dilate(modelDepth > 0, 9x9) at (mr, mc)
                    const int ya = max(mr - kDilate, 0), yb = min(mr + kDilate, H - 1);
                    const int xa = max(mc - kDilate, 0), xb = min(mc + kDilate, W - 1);
                    for (int yy = ya; yy <= yb && !in_mask; ++yy)
                        for (int xx = xa; xx <= xb; ++xx)
                            if (model[(size_t)yy * W + xx]) { in_mask = true; break; }
                }
                if (in_mask) {
                    is_s = true;
                    sz = sd / 1000.0;
                    sx = (double)__fdiv_rn(__fsub_rn((float)sc, B.sK[2]), B.sK[0]) * sz;
                    sy = (double)__fdiv_rn(__fsub_rn((float)sr, B.sK[5]), B.sK[4]) * sz;
                    if (fabs(sz - anchor) < 0.4 && md > 0) { acc[3] += sx; acc[4] += sy; acc[5] += sz; acc[6] += 1.0; }
                    ext[6] = fmin(ext[6], sx); ext[7] = fmin(ext[7], sy); ext[8] = fmin(ext[8], sz);
                    ext[9] = fmax(ext[9], sx); ext[10] = fmax(ext[10], sy); ext[11] = fmax(ext[11], sz);
                }
            }
        }
        int tot;
        const int pm = nm + block_scan_flag(is_m, s_wave, tot);
        nm += tot;
        if (is_m) { mp[3 * (size_t)pm] = mx; mp[3 * (size_t)pm + 1] = my; mp[3 * (size_t)pm + 2] = mz; }
        if (keep_scene) {
            const int ps = nsn + block_scan_flag(is_s, s_wave, tot);
            nsn += tot;
            if (is_s) { sp[3 * (size_t)ps] = sx; sp[3 * (size_t)ps + 1] = sy; sp[3 * (size_t)ps + 2] = sz; }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double v = wave_sum(acc[k]);
        if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        double v = ext[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = (k % 6) < 3 ? fmin(v, shfl_xor_d(v, o)) : fmax(v, shfl_xor_d(v, o));
        if ((tid & 63) == 0) s_ext[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 7) {
        double v = 0;
        for (int w = 0; w < kPtsWG / 64; ++w) v += s_red[w][tid];
        B.strip_sum[((size_t)h * kIcpStrips + strip) * 8 + tid] = v;
    }
    if (tid >= 64 && tid < 76) {                                   // the strip's extents: what k_icp_voxel_keys takes the voxel origin from (min / max are exact in any order)
        const int k = tid - 64;
        double v = s_ext[0][k];
        for (int w = 1; w < kPtsWG / 64; ++w) v = (k % 6) < 3 ? fmin(v, s_ext[w][k]) : fmax(v, s_ext[w][k]);
        B.strip_mm[((size_t)h * kIcpStrips + strip) * 12 + k] = v;
    }
    if (strip == 0 && tid == 0) { S.n_model = tot_m; S.n_scene = keep_scene ? tot_s : 0; }
}

// ---------------------------------------------------------------------------------------------
// k_icp_points_fused: both passes of k_icp_points in one launch.  A strip classifies its pixels once (two bits per pixel and thread in
// registers: the 9x9 dilation test is the expensive part), publishes its two counts as one agent-scope word and waits for the strips
// before it (lower block indices, dispatched before it) — their sum is where its points start — then writes.  The last strip, which has
// seen every count, sets n_model / n_scene.  k_icp_bbox clears the words (B.strip_pub) for the next run.
// ---------------------------------------------------------------------------------------------
constexpr long long kStripTimeout = 1000ll * 100000;            // wall_clock64 ticks: 1 s (then: status kIcpStalled)

__global__ void __launch_bounds__(kPtsWG)
k_icp_points_fused(IcpBuffers B, int W, int H, int flags) {
    __shared__ int s_wave[8];
    __shared__ double s_red[kPtsWG / 64][7];
    __shared__ double s_ext[kPtsWG / 64][12];
    __shared__ int s_tot[2];
    __shared__ long long s_before[2];
    const int h = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x;
    IcpState& S = B.st[h];
    if (S.status != 0) return;
    const IcpIn I = B.in[h];
    // the box of the model image: worked out when the image was uploaded (k_icp_model_boxes), else by k_icp_bbox of this run
    const int* known = B.model_bbox + (size_t)I.model_slot * 8;
    const bool boxed = known[4] == 1;
    const int x0 = boxed ? INT_MAX - known[0] : S.bbox[0], y0 = boxed ? INT_MAX - known[1] : S.bbox[1], x1 = boxed ? known[2] - 1 : S.bbox[2],
              y1 = boxed ? known[3] - 1 : S.bbox[3];
    if (strip == 0 && tid == 0 && !boxed) {                        // (k_icp_bbox is through: known from now on)
        int* kn = B.model_bbox + (size_t)I.model_slot * 8;
        kn[0] = INT_MAX - x0; kn[1] = INT_MAX - y0; kn[2] = x1 + 1; kn[3] = y1 + 1; __threadfence(); kn[4] = 1;
    }
    if (strip == 0 && tid < 2 * kIcpSortGroups) B.sort_look[(size_t)h * 2 * kIcpSortGroups + tid] = 0;   // (k_icp_voxel_wide: voxel counts of the groups, not yet known)
    if (x1 < 0) {
        if (strip == 0 && tid == 0) { S.status = kIcpEmptyModel; S.n_model = 0; S.n_scene = 0; }
        return;
    }
    const int bx0 = max(x0 - kDilate, 0), by0 = max(y0 - kDilate, 0);
    const int bx1 = min(x1 + kDilate, W - 1), by1 = min(y1 + kDilate, H - 1);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    if (I.dx + bw >= W || I.dy + bh >= H) {                       // LL.cpp:52-55
        if (strip == 0 && tid == 0) { S.status = kIcpOutOfFrame; S.n_model = 0; S.n_scene = 0; }
        return;
    }
    const uint16_t* model = B.models + (size_t)I.model_slot * W * H;
    const uint16_t* scene = B.scene;
    const int r_lo = (int)((long long)bh * strip / kIcpStrips), r_hi = (int)((long long)bh * (strip + 1) / kIcpStrips);
    const int p_lo = r_lo * bw, p_hi = r_hi * bw;
    const bool keep_scene = (flags & 1) != 0;
    // model point where modelDepth > 0; scene point where sceneDepth > 0 under the dilated mask (LL.cpp:43-50, 66-90)
    auto classify = [&](const int p, bool& is_m, bool& is_s) {
        const int r = p / bw, c = p - r * bw;
        const int mr = r + by0, mc = c + bx0;
        const int sr = max(r + I.dy - kDilate, 0), sc = max(c + I.dx - kDilate, 0);
        const uint16_t md = model[(size_t)mr * W + mc];
        const uint16_t sd = scene[(size_t)sr * W + sc];
        is_m = md > 0;
        is_s = false;
        if (sd > 0) {
            bool in_mask = md > 0;
            if (!in_mask) {                                       // dilate(modelDepth > 0, 9x9) at (mr, mc)
                const int ya = max(mr - kDilate, 0), yb = min(mr + kDilate, H - 1);
                const int xa = max(mc - kDilate, 0), xb = min(mc + kDilate, W - 1);
                for (int yy = ya; yy <= yb && !in_mask; ++yy)
                    for (int xx = xa; xx <= xb; ++xx)
                        if (model[(size_t)yy * W + xx]) { in_mask = true; break; }
            }
            is_s = in_mask;
        }
    };
    unsigned long long fm = 0, fs = 0;                             // the classes of this thread's first 64 pixels
    int cm = 0, cs = 0;
    {
        int it = 0;
        for (int p = p_lo + tid; p < p_hi; p += kPtsWG, ++it) {
            bool is_m, is_s;
            classify(p, is_m, is_s);
            cm += is_m ? 1 : 0; cs += (is_s && keep_scene) ? 1 : 0;
            if (it < 64) { fm |= (unsigned long long)is_m << it; fs |= (unsigned long long)is_s << it; }
        }
    }
    if (tid < 2) s_tot[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cm += __shfl_xor(cm, o, 64); cs += __shfl_xor(cs, o, 64); }
    if ((tid & 63) == 0) { atomicAdd(&s_tot[0], cm); atomicAdd(&s_tot[1], cs); }
    __syncthreads();
    unsigned long long* pub = B.strip_pub + (size_t)h * kIcpStrips;
    if (tid == 0) __hip_atomic_store(pub + strip, (1ull << 63) | ((unsigned long long)s_tot[1] << 32) | (unsigned long long)s_tot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
        unsigned long long v = 1ull << 63;
        if (tid < strip) {
            const long long t0 = wall_clock64();
            do { v = __hip_atomic_load(pub + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (!(v >> 63) && wall_clock64() - t0 < kStripTimeout);
        }
        const bool lost = __ballot(!(v >> 63)) != 0ull;
        long long bm = (long long)(v & 0xFFFFFFFFull), bs = (long long)((v >> 32) & 0x7FFFFFFFull);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { bm += __shfl_xor(bm, o, 64); bs += __shfl_xor(bs, o, 64); }
        if (tid == 0) { s_before[0] = lost ? -1 : bm; s_before[1] = bs; }
    }
    __syncthreads();
    if (s_before[0] < 0) {                                         // a strip before this one never came
        if (tid == 0) S.status = kIcpStalled;
        return;
    }
    int nm = (int)s_before[0], nsn = (int)s_before[1];

    const double anchor = model[(size_t)(H / 2) * W + W / 2] / 1000.0;   // LL.cpp:62
    double* mp = B.model_pts + (size_t)h * B.cap * 3;
    double* sp = B.scene_pts + (size_t)h * B.cap * 3;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};     // model xyz, scene-near-anchor xyz, its count
    double ext[12] = {1e300, 1e300, 1e300, -1e300, -1e300, -1e300, 1e300, 1e300, 1e300, -1e300, -1e300, -1e300};   // min, max of the strip's model points, of its scene points
    int it = 0;
    for (int base = p_lo; base < p_hi; base += kPtsWG, ++it) {
        const int p = base + tid;
        bool is_m = false, is_s = false;
        double mx = 0, my = 0, mz = 0, sx = 0, sy = 0, sz = 0;
        if (p < p_hi) {
            if (it < 64) { is_m = (fm >> it) & 1ull; is_s = (fs >> it) & 1ull; }
            else classify(p, is_m, is_s);
            const int r = p / bw, c = p - r * bw;
            const int mr = r + by0, mc = c + bx0;
            const int sr = max(r + I.dy - kDilate, 0), sc = max(c + I.dx - kDilate, 0);
            if (is_m) {
                const uint16_t md = model[(size_t)mr * W + mc];
                mz = md / 1000.0;
                // (int - float) / float evaluated in float, then * double (LL.cpp:79-80)
                mx = (double)__fdiv_rn(__fsub_rn((float)mc, I.mK[2]), I.mK[0]) * mz;
                my = (double)__fdiv_rn(__fsub_rn((float)mr, I.mK[5]), I.mK[4]) * mz;
                acc[0] += mx; acc[1] += my; acc[2] += mz;
                ext[0] = fmin(ext[0], mx); ext[1] = fmin(ext[1], my); ext[2] = fmin(ext[2], mz);
                ext[3] = fmax(ext[3], mx); ext[4] = fmax(ext[4], my); ext[5] = fmax(ext[5], mz);
            }
            if (is_s) {
                const uint16_t sd = scene[(size_t)sr * W + sc];
                sz = sd / 1000.0;
                sx = (double)__fdiv_rn(__fsub_rn((float)sc, B.sK[2]), B.sK[0]) * sz;
                sy = (double)__fdiv_rn(__fsub_rn((float)sr, B.sK[5]), B.sK[4]) * sz;
                if (fabs(sz - anchor) < 0.4 && is_m) { acc[3] += sx; acc[4] += sy; acc[5] += sz; acc[6] += 1.0; }
                ext[6] = fmin(ext[6], sx); ext[7] = fmin(ext[7], sy); ext[8] = fmin(ext[8], sz);
                ext[9] = fmax(ext[9], sx); ext[10] = fmax(ext[10], sy); ext[11] = fmax(ext[11], sz);
            }
        }
        int tot;
        const int pm = nm + block_scan_flag(is_m, s_wave, tot);
        nm += tot;
        if (is_m) { mp[3 * (size_t)pm] = mx; mp[3 * (size_t)pm + 1] = my; mp[3 * (size_t)pm + 2] = mz; }
        if (keep_scene) {
            const int ps = nsn + block_scan_flag(is_s, s_wave, tot);
            nsn += tot;
            if (is_s) { sp[3 * (size_t)ps] = sx; sp[3 * (size_t)ps + 1] = sy; sp[3 * (size_t)ps + 2] = sz; }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double v = wave_sum(acc[k]);
        if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        double v = ext[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = (k % 6) < 3 ? fmin(v, shfl_xor_d(v, o)) : fmax(v, shfl_xor_d(v, o));
        if ((tid & 63) == 0) s_ext[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 7) {
        double v = 0;
        for (int w = 0; w < kPtsWG / 64; ++w) v += s_red[w][tid];
        B.strip_sum[((size_t)h * kIcpStrips + strip) * 8 + tid] = v;
    }
    if (tid >= 64 && tid < 76) {
        const int k = tid - 64;
        double v = s_ext[0][k];
        for (int w = 1; w < kPtsWG / 64; ++w) v = (k % 6) < 3 ? fmin(v, s_ext[w][k]) : fmax(v, s_ext[w][k]);
        B.strip_mm[((size_t)h * kIcpStrips + strip) * 12 + k] = v;
    }
    if (strip == kIcpStrips - 1 && tid == 0) { S.n_model = nm; S.n_scene = keep_scene ? nsn : 0; }
}

// Pipeline glue (pipeline.cpp): turns the detections kept by the on-device NMS into ICP hypotheses without a
// host round trip.  One thread per hypothesis slot: the view (rendered depth slot + camera matrix) of the
// matched template, detect = match position (linemod_and_levelup_test.py:354-367).
__global__ void k_icp_bind(const TopkSel* __restrict__ sel, const int32_t* __restrict__ nsel_status, const int32_t* __restrict__ class_base,
                           const float* __restrict__ view_K, const int32_t* __restrict__ view_valid, int num_views, IcpIn* __restrict__ in,
                           IcpState* __restrict__ st, int top_k) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= top_k) return;
    IcpIn I;
    for (int k = 0; k < 9; ++k) I.mK[k] = 0.f;
    I.dx = 0; I.dy = 0; I.model_slot = 0; I.pad = 0;
    int status = kIcpNoDetection;                                // no detection for this slot
    if (nsel_status[1] == 0 && h < nsel_status[0]) {
        const TopkSel s = sel[h];
        const int base = class_base[s.class_index];
        const int v = base + s.template_id;
        status = kIcpNoView;                                     // the matched template has no rendered view
        if (base >= 0 && v >= 0 && v < num_views && view_valid[v]) {
            status = 0;
            for (int k = 0; k < 9; ++k) I.mK[k] = view_K[(size_t)v * 9 + k];
            I.dx = s.x; I.dy = s.y; I.model_slot = v;
        }
    }
    in[h] = I;
    IcpState& S = st[h];
    S = IcpState{};                                              // (a memset launch of its own cost 5 us + a gap)
    S.bbox[0] = INT_MAX; S.bbox[1] = INT_MAX; S.bbox[2] = -1; S.bbox[3] = -1;
    S.status = status;
}

hipError_t launch_icp_bind(const TopkSel* sel, const int32_t* nsel_status, const int32_t* class_base, const float* view_K,
                     const int32_t* view_valid, int num_views, IcpIn* in, IcpState* st, int top_k, hipStream_t s) {
    if (top_k <= 0) return hipSuccess;
    return lm_launch(k_icp_bind, dim3((top_k + 63) / 64), dim3(64), 0, s, sel, nsel_status, class_base, view_K, view_valid, num_views, in, st, top_k);
}

hipError_t launch_icp_clouds(const IcpBuffers& B, int count, int W, int H, int flags, hipStream_t s) {
    const Knobs& kn = knobs();
    if (!(flags & 0x100) || !kn.icp_wide_sort) LAUNCH_TRY(lm_launch(k_icp_bbox, dim3(32, count), dim3(256), 0, s, B, W, H));   // (0x100: every slot's box is in model_bbox)
    if (kn.icp_wide_sort) return lm_launch(k_icp_points_fused, dim3(kIcpStrips, count), dim3(kPtsWG), 0, s, B, W, H, flags);
    LAUNCH_TRY(lm_launch(k_icp_points<false>, dim3(kIcpStrips, count), dim3(kPtsWG), 0, s, B, W, H, flags));
    return lm_launch(k_icp_points<true>, dim3(kIcpStrips, count), dim3(kPtsWG), 0, s, B, W, H, flags);
}

}  // namespace lm
