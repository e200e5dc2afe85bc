// Internal interface between pose_error.cpp (host) and pose_error.hip (kernels).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lm {

// One (estimate, GT) pair of the point metrics.  M, c move estimate-frame model points into the GT model frame
// (M = R_g^-1 R_e, c = R_g^-1 (t_e - t_g), computed in f64 on the host, rounded to f32 for the search); the f64
// camera-frame poses re-evaluate the distance of the nearest point the search found.
struct PtsPair {
    float M[9], c[3];
    double Re[9], te[3], Rg[9], tg[3];
};
// Per (pair, chunk of 1024 GT-frame vertices): sums of the ADD and ADI distances of the chunk, or (diameter) the
// largest distance of the chunk.
struct PtsPartial {
    double add, adi;
};

enum PtsMode { kPtsAddOnly = 0, kPtsAdi = 1, kPtsDiameter = 2 };
constexpr int kPtsThreads = 256, kPtsPer = 1, kPtsChunk = kPtsThreads * kPtsPer, kPtsTile = 1024;

[[nodiscard]] hipError_t launch_pose_pts(const float* v, int nv, const PtsPair* pairs, int npairs, int mode, PtsPartial* partial, hipStream_t s);

// Symmetry-aware maxima (MSSD, MSPD).  One composed GT-side transform per (GT, symmetry): A = R_g R_s, b = R_g t_s + t_g
// (f64, host), stored [g][s]; a pair names its GT and carries the estimate's pose.
struct SymXf {
    double A[9], b[3];
};
struct SymPair {
    double Re[9], te[3];
    int g, pad;
};
struct SymCam {           // K, row-major f64
    double K[9];
};
constexpr int kSymThreads = 256, kSymWaves = kSymThreads / 64;
constexpr int kSymTile = 64;    // transforms staged in LDS at once (lm_pose_sym_tile)
constexpr int kSymFlight = 4;   // symmetries evaluated per lane before the wave reduces them
// metrics: LM_POSE_MSSD | LM_POSE_MSPD (nm = number of bits set, MSSD first).
// partial: f64 [npairs][chunks][nm][n_sym], the largest SQUARED distance of the chunk's vertices, chunks = sym_chunks(nv).
// out: f64 [npairs][nm] = sqrt(min over s of max over chunks).
inline int sym_chunks(int nv) { return (nv + kSymThreads - 1) / kSymThreads; }
[[nodiscard]] hipError_t launch_pose_sym(const float* v, int nv, const SymPair* pairs, int npairs, const SymXf* xf, int n_sym, SymCam cam, bool mssd, bool mspd,
                                         double* partial, double* out, hipStream_t s);

// Per (pair, block) counts of the pixel pass.  VSD: union / inter of the visibility masks and the step cost count;
// COU: inter / union of the rendered masks.  tl: the block's tlinear cost sum (f64, fixed order).
struct VsdPartial {
    double tl;
    unsigned int vis_union, vis_inter, step, cou_inter, cou_union, pad;
};
// Per (GT, block): px_count_all / valid / visib and the bounding box of the visible pixels.
struct GtPartial {
    unsigned int all, valid, visib, pad;
    int minx, miny, maxx, maxy;
};
struct PixCam {           // what depth_im_to_dist_im reads of K (f64): 1/fx, 1/fy (computed on the host), cx, cy
    double ifx, ify, cx, cy;
};
constexpr int kPixThreads = 256;
int pix_blocks(int npx);  // blocks per pair / GT of the pixel passes (a function of the image size only)

// zbuf: [views][H][W] keys of the rasteriser (float32 eye depth in the high 32 bits, ~0 = background).
// Pair p = (gi, ei) reads view gt_view0 + gi and est_view0 + ei, gi = p / n_est, ei = p % n_est.
// scene == nullptr: COU counts only.
[[nodiscard]] hipError_t launch_vsd(const unsigned long long* zbuf, int gt_view0, int n_gt, int est_view0, int n_est, const float* scene, int W, int H,
                                    PixCam cam, float delta, double tau_inv, double tau, VsdPartial* partial, hipStream_t s);
[[nodiscard]] hipError_t launch_gt_stats(const unsigned long long* zbuf, int n_gt, const float* scene, int W, int H, PixCam cam, float delta, GtPartial* partial,
                                         hipStream_t s);

}  // namespace lm
