// Pose errors on the device (pysixd/pose_error.py, visibility.py, misc.py; tools/calc_gt_stats.py:103-155):
//   * k_pose_pts — ADD, ADI and the mesh diameter.  One block per (pose pair, chunk of kPtsChunk GT-frame vertices);
//     each lane keeps kPtsPer GT-frame vertices in registers and sweeps tiles of kPtsTile estimate vertices staged in
//     LDS, already moved into the GT model frame (q = M v + c, f32, coordinates object-sized).  The search is f32 and
//     keeps the index of the nearest (ADI) / farthest (diameter) vertex; that one distance is re-evaluated in f64 in
//     the camera frame, so the result differs from an exact f64 search only where two candidates lie within f32
//     resolution (~1e-5 mm) of each other.  ADD needs no search: f64 per vertex.
//   * k_pose_sym, k_pose_sym_min — MSSD and MSPD: the largest surface / projection distance over the vertices, the smallest
//     over an explicit set of symmetry transformations.  f64 throughout, no search; max and min only, no sums.
//   * k_vsd — one pass per (estimate, GT) pair over the pixels: rendered depths from the rasteriser's z-buffer keys
//     (float32 eye depth, high 32 bits), scene depth resident, distance images built on the fly in f64 with numpy's
//     operation order, visibility with both distances cast to f32 (visibility.py:18), integer counts and the tlinear
//     cost sum in f64.
//   * k_gt_stats — one pass per GT: px_count_all / valid / visib and the box of the visible pixels.
// Every partial is reduced inside the block by a fixed LDS tree and written per block; the host sums the blocks in
// order, so repeated calls are bit-identical (no floating-point atomics).  -ffp-contract=off (Makefile) keeps the f64
// pixel expressions unfused; the f32 distance of the search uses explicit fmaf.
#include "launch.h"
#include "pose_error_kernels.h"

namespace lm {

static __device__ __forceinline__ double norm3(double x, double y, double z) {
    return __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
}
// p = R v + t in f64, misc.transform_pts_Rt
static __device__ __forceinline__ void xform(const double* R, const double* t, double x, double y, double z, double* p) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        p[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(R[3 * r], x), __dmul_rn(R[3 * r + 1], y)), __dmul_rn(R[3 * r + 2], z)), t[r]);
}

template <int MODE>
__global__ __launch_bounds__(kPtsThreads) void k_pose_pts(const float* __restrict__ v, int nv, const PtsPair* __restrict__ pairs,
                                                         PtsPartial* __restrict__ partial) {
    __shared__ float4 tile[kPtsTile];
    __shared__ double red_a[kPtsThreads], red_b[kPtsThreads];
    const int tid = threadIdx.x, chunk = blockIdx.x, pair = blockIdx.y;
    const PtsPair& P = pairs[pair];
    float px[kPtsPer], py[kPtsPer], pz[kPtsPer], best[kPtsPer];
    int bi[kPtsPer];
#pragma unroll
    for (int k = 0; k < kPtsPer; ++k) {
        const int i = chunk * kPtsChunk + k * kPtsThreads + tid;
        const bool ok = i < nv;
        px[k] = ok ? v[3 * (size_t)i] : 0.f;
        py[k] = ok ? v[3 * (size_t)i + 1] : 0.f;
        pz[k] = ok ? v[3 * (size_t)i + 2] : 0.f;
        best[k] = MODE == kPtsDiameter ? -1.f : __builtin_huge_valf();
        bi[k] = 0;
    }
    if (MODE != kPtsAddOnly) {
        float M[9], c[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = P.M[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = P.c[k];
        for (int base = 0; base < nv; base += kPtsTile) {
            const int n = min(kPtsTile, nv - base);
            __syncthreads();                                            // the previous tile has been swept by every lane
            for (int j = tid; j < n; j += kPtsThreads) {
                const size_t g = (size_t)(base + j);
                const float x = v[3 * g], y = v[3 * g + 1], z = v[3 * g + 2];
                tile[j] = make_float4(((M[0] * x + M[1] * y) + M[2] * z) + c[0], ((M[3] * x + M[4] * y) + M[5] * z) + c[1],
                                      ((M[6] * x + M[7] * y) + M[8] * z) + c[2], 0.f);
            }
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const float4 q = tile[j];                               // one address for the whole wave: broadcast
#pragma unroll
                for (int k = 0; k < kPtsPer; ++k) {
                    const float dx = px[k] - q.x, dy = py[k] - q.y, dz = pz[k] - q.z;
                    const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    const bool better = MODE == kPtsDiameter ? d2 > best[k] : d2 < best[k];   // strict: the first index wins ties
                    best[k] = better ? d2 : best[k];
                    bi[k] = better ? base + j : bi[k];
                }
            }
        }
    }
    double sa = 0.0, sb = 0.0;                                           // ADD / ADI sums, or (diameter) the max in sb
#pragma unroll
    for (int k = 0; k < kPtsPer; ++k) {
        const int i = chunk * kPtsChunk + k * kPtsThreads + tid;
        if (i >= nv) continue;
        const double x = px[k], y = py[k], z = pz[k];
        if (MODE == kPtsDiameter) {
            const size_t j = (size_t)bi[k];
            const double d = norm3(__dsub_rn(x, (double)v[3 * j]), __dsub_rn(y, (double)v[3 * j + 1]), __dsub_rn(z, (double)v[3 * j + 2]));
            sb = fmax(sb, d);
            continue;
        }
        double pg[3], pe[3];
        xform(P.Rg, P.tg, x, y, z, pg);
        xform(P.Re, P.te, x, y, z, pe);
        sa = __dadd_rn(sa, norm3(__dsub_rn(pe[0], pg[0]), __dsub_rn(pe[1], pg[1]), __dsub_rn(pe[2], pg[2])));
        if (MODE == kPtsAdi) {
            const size_t j = (size_t)bi[k];
            xform(P.Re, P.te, (double)v[3 * j], (double)v[3 * j + 1], (double)v[3 * j + 2], pe);
            sb = __dadd_rn(sb, norm3(__dsub_rn(pe[0], pg[0]), __dsub_rn(pe[1], pg[1]), __dsub_rn(pe[2], pg[2])));
        }
    }
    red_a[tid] = sa; red_b[tid] = sb;
    __syncthreads();
    for (int s = kPtsThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red_a[tid] = __dadd_rn(red_a[tid], red_a[tid + s]);
            red_b[tid] = MODE == kPtsDiameter ? fmax(red_b[tid], red_b[tid + s]) : __dadd_rn(red_b[tid], red_b[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)pair * gridDim.x + chunk] = PtsPartial{red_a[0], red_b[0]};
}

hipError_t launch_pose_pts(const float* v, int nv, const PtsPair* pairs, int npairs, int mode, PtsPartial* partial, hipStream_t s) {
    if (nv <= 0 || npairs <= 0) return hipSuccess;
    const dim3 grid((nv + kPtsChunk - 1) / kPtsChunk, npairs);
    if (mode == kPtsAddOnly) return lm_launch(k_pose_pts<kPtsAddOnly>, grid, dim3(kPtsThreads), 0, s, v, nv, pairs, partial);
    if (mode == kPtsAdi) return lm_launch(k_pose_pts<kPtsAdi>, grid, dim3(kPtsThreads), 0, s, v, nv, pairs, partial);
    return lm_launch(k_pose_pts<kPtsDiameter>, grid, dim3(kPtsThreads), 0, s, v, nv, pairs, partial);
}

// ---- symmetry-aware maxima (MSSD, MSPD) -------------------------------------------------------------------------
// max and min are exact, so the kernels carry SQUARED distances and take one square root at the very end
// (sqrt is monotonic and correctly rounded: sqrt(max d^2) == max sqrt(d^2) bit for bit).
template <int CTRL>
static __device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// The maximum over the 64 lanes, wave-uniform.  Every lane of the wave must be active.
static __device__ __forceinline__ double wave_max(double x) {
    x = fmax(x, dpp_f64<0xB1>(x));                                      // quad_perm [1,0,3,2]
    x = fmax(x, dpp_f64<0x4E>(x));                                      // quad_perm [2,3,0,1]
    x = fmax(x, dpp_f64<0x141>(x));                                     // row_half_mirror
    x = fmax(x, dpp_f64<0x140>(x));                                     // row_mirror: every lane holds its row's maximum
    const int lo = __double2loint(x), hi = __double2hiint(x);
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * k), __builtin_amdgcn_readlane(lo, 16 * k));
    return fmax(fmax(r[0], r[1]), fmax(r[2], r[3]));
}
// proj(p) = ((K p)[0] / (K p)[2], (K p)[1] / (K p)[2])
static __device__ __forceinline__ void project(const SymCam& c, const double* p, double& u, double& v) {
    double w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = (c.K[3 * r] * p[0] + c.K[3 * r + 1] * p[1]) + c.K[3 * r + 2] * p[2];
    u = w[0] / w[2];
    v = w[1] / w[2];
}

// One block per (pair, chunk of kSymThreads vertices).  A lane keeps its vertex, the estimate-side point and pixel in
// registers and sweeps the GT's composed transforms, staged in LDS kSymTile at a time and read at one address per wave.
// kSymFlight independent symmetries are evaluated before their maxima are reduced, so no lane waits on one f64 chain.
template <bool SSD, bool SPD>
__global__ __launch_bounds__(kSymThreads) void k_pose_sym(const float* __restrict__ v, int nv, const SymPair* __restrict__ pairs,
                                                         const SymXf* __restrict__ xf, int n_sym, SymCam cam, double* __restrict__ partial) {
    constexpr int NM = (SSD ? 1 : 0) + (SPD ? 1 : 0);
    __shared__ double tile[kSymTile * 12];
    __shared__ double red[NM][kSymWaves][kSymTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x, pair = blockIdx.y;
    const SymPair& P = pairs[pair];
    const size_t i = (size_t)chunk * kSymThreads + tid;
    const bool ok = i < (size_t)nv;
    const double x = ok ? (double)v[3 * i] : 0.0, y = ok ? (double)v[3 * i + 1] : 0.0, z = ok ? (double)v[3 * i + 2] : 0.0;
    double pe[3], ue = 0.0, ve = 0.0;
    xform(P.Re, P.te, x, y, z, pe);
    if (SPD) project(cam, pe, ue, ve);
    const double* src = (const double*)(xf + (size_t)P.g * n_sym);
    double* dst = partial + ((size_t)pair * gridDim.x + chunk) * NM * n_sym;
    for (int s0 = 0; s0 < n_sym; s0 += kSymTile) {
        const int n = min(kSymTile, n_sym - s0);
        __syncthreads();                                                // the previous tile and its maxima have been read
        for (int j = tid; j < 12 * n; j += kSymThreads) tile[j] = src[12 * (size_t)s0 + j];
        __syncthreads();
        for (int j0 = 0; j0 < n; j0 += kSymFlight) {
            double d3[kSymFlight], d2[kSymFlight];
#pragma unroll
            for (int k = 0; k < kSymFlight; ++k) {
                const double* T = tile + 12 * min(j0 + k, n - 1);       // the tail repeats the last transform
                double q[3];
                xform(T, T + 9, x, y, z, q);
                if (SSD) {
                    const double dx = pe[0] - q[0], dy = pe[1] - q[1], dz = pe[2] - q[2];
                    d3[k] = ok ? (dx * dx + dy * dy) + dz * dz : 0.0;   // 0 is neutral: distances are >= 0
                }
                if (SPD) {
                    double ug, vg;                                      // two divisions, as the definition: a pose against itself is 0
                    project(cam, q, ug, vg);
                    const double du = ue - ug, dv = ve - vg;
                    d2[k] = ok ? du * du + dv * dv : 0.0;
                }
            }
#pragma unroll
            for (int k = 0; k < kSymFlight; ++k) {
                if (SSD) d3[k] = wave_max(d3[k]);
                if (SPD) d2[k] = wave_max(d2[k]);
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < kSymFlight; ++k)
                    if (j0 + k < n) {
                        if (SSD) red[0][wave][j0 + k] = d3[k];
                        if (SPD) red[NM - 1][wave][j0 + k] = d2[k];
                    }
            }
        }
        __syncthreads();
        if (tid < NM * n) {
            const int mi = tid / n, j = tid % n;
            double r = red[mi][0][j];
#pragma unroll
            for (int w = 1; w < kSymWaves; ++w) r = fmax(r, red[mi][w][j]);
            dst[(size_t)mi * n_sym + s0 + j] = r;
        }
    }
}

// One block per (pair, metric): the maximum over the chunks for each symmetry (a wave per symmetry, a lane per chunk), the
// minimum over the symmetries, one sqrt.
__global__ __launch_bounds__(kSymThreads) void k_pose_sym_min(const double* __restrict__ partial, int chunks, int nm, int n_sym,
                                                             double* __restrict__ out) {
    __shared__ double red[kSymWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x / nm, mi = blockIdx.x % nm;
    const double* src = partial + ((size_t)pair * chunks * nm + mi) * n_sym;
    double best = __builtin_huge_val();
    for (int s = wave; s < n_sym; s += kSymWaves) {                     // wave-uniform: every lane reaches wave_max
        double mx = 0.0;
        for (int c = lane; c < chunks; c += 64) mx = fmax(mx, src[(size_t)c * nm * n_sym + s]);
        best = fmin(best, wave_max(mx));
    }
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (tid == 0) {
        double r = red[0];
#pragma unroll
        for (int w = 1; w < kSymWaves; ++w) r = fmin(r, red[w]);
        out[blockIdx.x] = __dsqrt_rn(r);
    }
}

hipError_t launch_pose_sym(const float* v, int nv, const SymPair* pairs, int npairs, const SymXf* xf, int n_sym, SymCam cam, bool mssd, bool mspd,
                     double* partial, double* out, hipStream_t s) {
    if (nv <= 0 || npairs <= 0 || n_sym <= 0 || !(mssd || mspd)) return hipSuccess;
    const int chunks = sym_chunks(nv);
    const dim3 grid(chunks, npairs), block(kSymThreads);
    if (mssd && mspd) LAUNCH_TRY(lm_launch(k_pose_sym<true, true>, grid, block, 0, s, v, nv, pairs, xf, n_sym, cam, partial));
    else if (mssd) LAUNCH_TRY(lm_launch(k_pose_sym<true, false>, grid, block, 0, s, v, nv, pairs, xf, n_sym, cam, partial));
    else LAUNCH_TRY(lm_launch(k_pose_sym<false, true>, grid, block, 0, s, v, nv, pairs, xf, n_sym, cam, partial));
    const int nm = (mssd ? 1 : 0) + (mspd ? 1 : 0);
    return lm_launch(k_pose_sym_min, dim3(npairs * nm), block, 0, s, (const double*)partial, chunks, nm, n_sym, out);
}

// ---- pixel passes -----------------------------------------------------------------------------------------------
// misc.depth_im_to_dist_im: X = ((u - cx) * d) * (1/fx), Y likewise, dist = sqrt((X^2 + Y^2) + d^2), all f64
static __device__ __forceinline__ double dist_px(double d, int u, int v, const PixCam& c) {
    const double X = __dmul_rn(__dmul_rn(__dsub_rn((double)u, c.cx), d), c.ifx);
    const double Y = __dmul_rn(__dmul_rn(__dsub_rn((double)v, c.cy), d), c.ify);
    return norm3(X, Y, d);
}
static __device__ __forceinline__ double key_depth(unsigned long long k) {
    return k == ~0ull ? 0.0 : (double)__uint_as_float((unsigned int)(k >> 32));
}
// visibility.estimate_visib_mask: both distance images cast to f32 before the difference
static __device__ __forceinline__ bool visible(double d_test, double d_model, float delta) {
    return d_test > 0.0 && d_model > 0.0 && __fsub_rn((float)d_model, (float)d_test) <= delta;
}

int pix_blocks(int npx) {
    const int b = (npx + 4 * kPixThreads - 1) / (4 * kPixThreads);
    return b < 1 ? 1 : (b > 128 ? 128 : b);
}

__global__ __launch_bounds__(kPixThreads) void k_vsd(const unsigned long long* __restrict__ zbuf, int gt_view0, int est_view0, int n_est,
                                                     const float* __restrict__ scene, int W, int npx, PixCam cam, float delta,
                                                     double tau_inv, double tau, VsdPartial* __restrict__ partial) {
    __shared__ double red_d[kPixThreads];
    __shared__ unsigned int red_u[5][kPixThreads];
    const int tid = threadIdx.x, pair = blockIdx.y;
    const int gi = pair / n_est, ei = pair % n_est;
    const unsigned long long* Zg = zbuf + (size_t)(gt_view0 + gi) * npx;
    const unsigned long long* Ze = zbuf + (size_t)(est_view0 + ei) * npx;
    double tl = 0.0;
    unsigned int vu = 0, vi = 0, st = 0, ci = 0, cu = 0;
    for (int i = blockIdx.x * kPixThreads + tid; i < npx; i += gridDim.x * kPixThreads) {
        const double dg = key_depth(Zg[i]), de = key_depth(Ze[i]);
        ci += (dg > 0.0 && de > 0.0);                                   // pose_error.cou: masks depth > 0
        cu += (dg > 0.0 || de > 0.0);
        if (!scene) continue;
        const int u = i % W, v = i / W;
        const double Dt = dist_px((double)scene[i], u, v, cam), Dg = dist_px(dg, u, v, cam), De = dist_px(de, u, v, cam);
        const bool vis_g = visible(Dt, Dg, delta);
        const bool vis_e = visible(Dt, De, delta) || (vis_g && De > 0.0);   // visibility.estimate_visib_mask_est
        vu += (vis_g || vis_e);
        if (vis_g && vis_e) {
            ++vi;
            const double cost = fabs(__dsub_rn(Dg, De));
            st += cost >= tau;
            tl = __dadd_rn(tl, fmin(__dmul_rn(cost, tau_inv), 1.0));
        }
    }
    red_d[tid] = tl;
    red_u[0][tid] = vu; red_u[1][tid] = vi; red_u[2][tid] = st; red_u[3][tid] = ci; red_u[4][tid] = cu;
    __syncthreads();
    for (int s = kPixThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red_d[tid] = __dadd_rn(red_d[tid], red_d[tid + s]);
#pragma unroll
            for (int k = 0; k < 5; ++k) red_u[k][tid] += red_u[k][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)pair * gridDim.x + blockIdx.x] = VsdPartial{red_d[0], red_u[0][0], red_u[1][0], red_u[2][0], red_u[3][0], red_u[4][0], 0};
}

__global__ __launch_bounds__(kPixThreads) void k_gt_stats(const unsigned long long* __restrict__ zbuf, const float* __restrict__ scene, int W,
                                                          int npx, PixCam cam, float delta, GtPartial* __restrict__ partial) {
    __shared__ int red[7][kPixThreads];
    const int tid = threadIdx.x, g = blockIdx.y;
    const unsigned long long* Zg = zbuf + (size_t)g * npx;
    int all = 0, valid = 0, visib = 0, minx = 0x7fffffff, miny = 0x7fffffff, maxx = -1, maxy = -1;
    for (int i = blockIdx.x * kPixThreads + tid; i < npx; i += gridDim.x * kPixThreads) {
        const int u = i % W, v = i / W;
        const double Dg = dist_px(key_depth(Zg[i]), u, v, cam);
        if (!(Dg > 0.0)) continue;                                      // obj_mask_gt = dist_gt > 0
        const double Dt = dist_px((double)scene[i], u, v, cam);
        ++all;
        valid += Dt > 0.0;
        if (visible(Dt, Dg, delta)) {
            ++visib;
            minx = min(minx, u); maxx = max(maxx, u);
            miny = min(miny, v); maxy = max(maxy, v);
        }
    }
    red[0][tid] = all; red[1][tid] = valid; red[2][tid] = visib;
    red[3][tid] = minx; red[4][tid] = miny; red[5][tid] = maxx; red[6][tid] = maxy;
    __syncthreads();
    for (int s = kPixThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + s];
            red[3][tid] = min(red[3][tid], red[3][tid + s]);
            red[4][tid] = min(red[4][tid], red[4][tid + s]);
            red[5][tid] = max(red[5][tid], red[5][tid + s]);
            red[6][tid] = max(red[6][tid], red[6][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0)
        partial[(size_t)g * gridDim.x + blockIdx.x] =
            GtPartial{(unsigned)red[0][0], (unsigned)red[1][0], (unsigned)red[2][0], 0u, red[3][0], red[4][0], red[5][0], red[6][0]};
}

hipError_t launch_vsd(const unsigned long long* zbuf, int gt_view0, int n_gt, int est_view0, int n_est, const float* scene, int W, int H,
                PixCam cam, float delta, double tau_inv, double tau, VsdPartial* partial, hipStream_t s) {
    if (n_gt <= 0 || n_est <= 0) return hipSuccess;
    const int npx = W * H;
    return lm_launch(k_vsd, dim3(pix_blocks(npx), n_gt * n_est), dim3(kPixThreads), 0, s, zbuf, gt_view0, est_view0, n_est, scene, W, npx, cam,
                     delta, tau_inv, tau, partial);
}
hipError_t launch_gt_stats(const unsigned long long* zbuf, int n_gt, const float* scene, int W, int H, PixCam cam, float delta, GtPartial* partial,
                     hipStream_t s) {
    if (n_gt <= 0) return hipSuccess;
    const int npx = W * H;
    return lm_launch(k_gt_stats, dim3(pix_blocks(npx), n_gt), dim3(kPixThreads), 0, s, zbuf, scene, W, npx, cam, delta, partial);
}

}  // namespace lm
