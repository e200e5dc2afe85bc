// RegistrationICP + TransformationEstimationPointToPlane (reference LL.cpp:128-130), one launch per evaluation: the last stage of
// the ICP ladder (pose_refine.cpp), which takes what k_icp_team (icp_team.hip) left, and the whole loop under LM_ICP_SLICED=1, for
// TransformationEstimationPointToPoint (k_icp_eval<true>; LL.cpp:132-134) and for criteria other than the defaults.
//   k_icp_eval  once per ICP evaluation (<= 31 + 1): exact nearest neighbours through the grid (search radius = distance to the
//               previous correspondence), 29 double sums by a halving wave reduction, then 6x6 LU, Rz*Ry*Rx update and the
//               convergence test.
// The grid only prunes: candidate distances are the same expression the oracle evaluates and ties go to the lower original index, so
// correspondences equal a brute-force search.
// Part of poseRefine::process on gfx950 (reference LL.cpp:27-155; the stages and their files: icp_kernels.h).  The cloud arithmetic is
// Open3D's (un-vendored), restated per SURVEY Appendix B with the deterministic rules of DESIGN.md §5 (shared with
// oracle/linemod_oracle.py).  All arithmetic is double like Open3D's (f64 VALU; nothing here is a dense contraction, so no MFMA).
#include <limits.h>

#include "launch.h"
#include "icp_device.h"
#include "icp_kabsch.h"
#include "icp_kernels.h"
#include "knobs.h"

namespace lm {

// ---- RegistrationICP ------------------------------------------------------------------------------
// One launch (k_icp_eval) per ICP evaluation, grid (G, hypotheses): workgroup g owns a slice of the
// source points.  Splitting a hypothesis over G workgroups is what fills the chip at the batch sizes of
// the pipeline (16 hypotheses x 16 slices = 256 workgroups = one per CU); the stream order of the
// launches is the only synchronisation, converged hypotheses return at once.
constexpr int kSearchWG = 256;      // workgroup of k_icp_eval
constexpr int kIcpFineFrom = 6;     // evaluations from this one on run on kIcpMaxSplit slices per hypothesis
constexpr int kLoopQueue = 1024;    // source points per round whose correspondence needs a grid search
constexpr int kSlabPts = 1024;      // target points of a slice's x slab staged in LDS (32-byte records)
constexpr int kSlabCells = 4096;    // cells of that slab (16-bit starts)

// Gaussian elimination with partial pivoting, [A | b] (6 x 7), in registers: every loop is unrolled, a row exchange is a chain of
// conditional swaps (no dynamic indexing, so nothing goes to scratch), one reciprocal per pivot.  Returns false if singular /
// non-finite.  (On LDS arrays — the first version — the ~250 dependent LDS accesses of the elimination were most of the
// evaluation's 6 us prologue, which every slice of every hypothesis pays before it can transform a point.)
static __device__ __forceinline__ bool solve6(double (&M)[6][7], double (&x)[6]) {
    double inv[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        double best = fabs(M[c][c]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r)
            if (fabs(M[r][c]) > best) { best = fabs(M[r][c]); piv = r; }
        if (!(best > 0.0)) return false;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int q = c; q < 7; ++q) { const double a = M[c][q], b = M[r][q]; M[c][q] = sw ? b : a; M[r][q] = sw ? a : b; }
        }
        inv[c] = 1.0 / M[c][c];
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const double f = M[r][c] * inv[c];
#pragma unroll
            for (int q = c + 1; q < 7; ++q) M[r][q] -= f * M[c][q];
        }
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = M[r][6];
#pragma unroll
        for (int q = r + 1; q < 6; ++q) s -= M[r][q] * x[q];
        x[r] = s * inv[r];
    }
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) ok = ok && isfinite(x[r]);
    return ok;
}

// One ICP evaluation of one source slice.  Prologue (evaluations >= 1, every workgroup of the hypothesis
// redundantly, so that no second launch or inter-workgroup barrier is needed): add the G partials of
// the previous evaluation in fixed order, Open3D's relative-change convergence test,
// TransformationEstimationPointToPlane::ComputeTransformation (6x6 LU with partial pivoting),
// transformation = update * transformation (workgroup 0 records it).  Then pcd.Transform on the slice and
// the correspondences (GetRegistrationResultAndCorrespondences):
//   A1  every source point first re-measures its previous correspondence j: with d = |p - t_j|^2 and
//       sep2(j) = squared distance from t_j to its nearest other target (from k_icp_knn), 4 d < sep2(j)
//       proves by the triangle inequality that t_j is still the unique nearest neighbour — no search.
//       A point without correspondence carries a lower bound on its nearest-target distance (what its
//       last search saw, minus its motion since); while that exceeds max_dist it needs no search either.
//       The other points are queued in LDS, ordered by the number of grid columns their search cube
//       overlaps, so that the searches a wave runs in lock-step cost about the same;
//   A2  queued points search the cells overlapping the cube of half-width sqrt(min(d_prev, r^2)):
//       exact lexicographic minimum of (d, original index); a point of class c (<= 2^c columns) has 2^c lanes, one column
//       each, and all classes are walked in one sweep of the workgroup's lanes;
// and the slice's 32 partial sums (21 JtJ upper + 6 Jtr + sum d^2 + count, padded) for the next prologue.
// Returns true when the hypothesis is finished (converged, or evaluation max_iter done).
// P2P: TransformationEstimationPointToPoint instead (the #else branch of LL.cpp:122-135).  Correspondences, fitness and inlier RMSE are
// the same; the slice publishes n, sum d^2, sum p, sum q and sum q p^T (p = transformed source, q = target) in the same 32 slots (0-2,
// 3-5, 6-14; 27 and 28 as before), and the prologue solves for [R | t] with kabsch_update (icp_kabsch.h) instead of the 6x6.  The
// normals are not read.
template <bool P2P>
static __device__ __forceinline__ bool icp_eval_body(const IcpBuffers& B, IcpState& S, const int h, const int it, const int Gprev, const int max_shift, TgtRec* s_tgt,
                                                     unsigned short* s_cs, int* s_q, unsigned char* s_cls, const double max_dist,
                                                     const int max_iter, const double rel_fit, const double rel_rmse, double* fit_hist, double* rmse_hist) {
    __shared__ double s_part[kSearchWG / 64][32];
    __shared__ double s_sum[32];
    __shared__ double s_U[12];
    __shared__ int s_stop;
    __shared__ int s_cnt[kClasses], s_cur[kClasses];
    __shared__ double s_xmm[kSearchWG / 64][2];
    __shared__ double s_red8[8][32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = gridDim.x, g = blockIdx.x;
    const int ns = S.n_src, nt = S.n_tgt;
    const long long t0 = (long long)__builtin_amdgcn_s_memtime();

    const double* Src = B.src + (size_t)h * B.cap * 3;
    const double* T = B.tgt_sorted + (size_t)h * B.cap * 3;
    const double* N = B.normals + (size_t)h * B.cap * 3;
    const double* cov = B.cov + (size_t)h * B.cap * kIcpCovStride;
    const int* orig = B.tgt_orig + (size_t)h * B.cap;
    const int* cs = B.cell_start + (size_t)h * kIcpCells;
    double* P = B.work + (size_t)h * B.cap * 3;
    int* prev = B.prev_nn + (size_t)h * B.cap;
    double* lb = B.nn_lb + (size_t)h * B.cap;
    const int gx = S.gx, gy = S.gy, zq_max = S.zq_max;
    const double minx = S.gminx, miny = S.gminy, minz = S.gminz, inv = S.inv_cell, inv_z = S.inv_z;
    const TgtRec* rec = B.tgt_rec + (size_t)h * B.cap;
    const double r2 = max_dist * max_dist;
    const double far = max_dist * kFarMargin, far2 = far * far, lb_need = max_dist * (1.0 + 1e-9);
    const int i_lo = (int)((long long)ns * g / G), i_hi = (int)((long long)ns * (g + 1) / G);

    // this thread's (first) point and what the transform needs of its correspondence, requested before the prologue waits for
    // the slices' partial sums and the solve: the loads ride out that wait instead of starting after it
    const int i_pf = i_lo + tid;
    const bool pf = it > 0 && i_pf < i_hi;
    double pfx = 0, pfy = 0, pfz = 0, pflb = 0, pftx = 0, pfty = 0, pftz = 0, pfsep = 0;
    int pfj = -1;
    if (pf) {
        pfx = P[3 * (size_t)i_pf]; pfy = P[3 * (size_t)i_pf + 1]; pfz = P[3 * (size_t)i_pf + 2];
        pfj = prev[i_pf]; pflb = lb[i_pf];
        if (pfj >= 0) { pftx = T[3 * (size_t)pfj]; pfty = T[3 * (size_t)pfj + 1]; pftz = T[3 * (size_t)pfj + 2]; pfsep = cov[(size_t)pfj * kIcpCovStride + 10]; }
    }

    // ---- prologue: finish evaluation it - 1 ----
    if (it > 0) {
        const double* part = B.partial + (((size_t)((it - 1) & 1) * B.count + h) * kIcpMaxSplit) * 32;
        {   // fixed association: 8 interleaved groups of <= 8 slices each, loads issued together
            const int k = tid & 31, grp = tid >> 5;
            double a8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int gg = grp + 8 * u;
                a8[u] = 0.0;
                if (gg < Gprev) a8[u] = part[(size_t)gg * 32 + k];
            }
            double v = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) v += a8[u];
            s_red8[grp][k] = v;
        }
        __syncthreads();
        if (tid < 32) {
            double v = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) v += s_red8[w][tid];
            s_sum[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {
            const int ncorr = (int)s_sum[28];
            const double fit = ncorr ? (double)ncorr / (double)ns : 0.0;
            const double rmse = ncorr ? sqrt(s_sum[27] / (double)ncorr) : 0.0;
            bool stop = false;
            if (it > 1 && fabs(fit_hist[it & 1] - fit) < rel_fit && fabs(rmse_hist[it & 1] - rmse) < rel_rmse) stop = true;
            if (it - 1 == max_iter) stop = true;
            if (g == 0) { fit_hist[(it - 1) & 1] = fit; rmse_hist[(it - 1) & 1] = rmse; }
            if (g == 0) {
                S.fitness = fit; S.rmse = rmse; S.n_corr = ncorr;
                if (stop) { S.stop = 1; S.build = 0; }
            }
            s_stop = stop ? 1 : 0;
            if (!stop) {
                double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
                if constexpr (P2P) {                        // (through LDS: a local array handed to the non-inlined solve would live in scratch)
                    for (int a = 0; a < 12; ++a) s_U[a] = U[a];
                    (void)kabsch_update(s_sum, ncorr, s_U);     // left as it is (the identity) when n < 3 or the result is not finite
                    for (int a = 0; a < 12; ++a) U[a] = s_U[a];
                } else {
                    double M[6][7], x[6];
                    {
                        double up[21];
#pragma unroll
                        for (int q = 0; q < 21; ++q) up[q] = s_sum[q];
                        int k = 0;
#pragma unroll
                        for (int a = 0; a < 6; ++a)
#pragma unroll
                            for (int c = a; c < 6; ++c) { M[a][c] = up[k]; M[c][a] = up[k]; ++k; }
#pragma unroll
                        for (int a = 0; a < 6; ++a) M[a][6] = -s_sum[21 + a];
                    }
                    if (ncorr >= 6 && solve6(M, x)) {
                        double sx, cx, sy, cy, sz, cz;
                        sincos(x[0], &sx, &cx); sincos(x[1], &sy, &cy); sincos(x[2], &sz, &cz);
                        // Rz(x2) * Ry(x1) * Rx(x0)
                        U[0] = cz * cy; U[1] = cz * sy * sx - sz * cx; U[2] = cz * sy * cx + sz * sx; U[3] = x[3];
                        U[4] = sz * cy; U[5] = sz * sy * sx + cz * cx; U[6] = sz * sy * cx - cz * sx; U[7] = x[4];
                        U[8] = -sy;     U[9] = cy * sx;                U[10] = cy * cx;               U[11] = x[5];
                    }
                }
                for (int a = 0; a < 12; ++a) s_U[a] = U[a];
                if (g == 0) {                               // transformation = update * transformation
                    double Tn[12];
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 4; ++c)
                            Tn[4 * r + c] = U[4 * r] * S.T[c] + U[4 * r + 1] * S.T[4 + c] + U[4 * r + 2] * S.T[8 + c] + (c == 3 ? U[4 * r + 3] : 0.0);
                    for (int a = 0; a < 12; ++a) S.T[a] = Tn[a];
                    S.iterations = it;
                }
            }
        }
        __syncthreads();
        if (s_stop) return true;
    } else if (g == 0 && tid == 0) {
        for (int a = 0; a < 16; ++a) S.T[a] = (a % 5 == 0) ? 1.0 : 0.0;
        S.T[3] = S.init[0]; S.T[7] = S.init[1]; S.T[11] = S.init[2];
        S.iterations = 0;
    }
    if (it > max_iter) return true;                         // the last round only finishes evaluation max_iter
    const long long t1 = (long long)__builtin_amdgcn_s_memtime();

    // pcd.Transform: the initial guess at evaluation 0, the update afterwards
    double xmn = 1e300, xmx = -1e300;
    if (it == 0) {
        const double t0 = S.init[0], t1 = S.init[1], t2 = S.init[2];
        for (int i = i_lo + tid; i < i_hi; i += kSearchWG) {
            const double x = Src[3 * (size_t)i], y = Src[3 * (size_t)i + 1], z = Src[3 * (size_t)i + 2];
            const double nx = 1.0 * x + 0.0 * y + 0.0 * z + t0;
            P[3 * (size_t)i] = nx;
            P[3 * (size_t)i + 1] = 0.0 * x + 1.0 * y + 0.0 * z + t1;
            P[3 * (size_t)i + 2] = 0.0 * x + 0.0 * y + 1.0 * z + t2;
            prev[i] = -1;
            lb[i] = 0.0;
            xmn = fmin(xmn, nx - far * 1.001); xmx = fmax(xmx, nx + far * 1.001);
        }
    } else {
        double U[12];
#pragma unroll
        for (int a = 0; a < 12; ++a) U[a] = s_U[a];
        auto move_point = [&](const int i, const double x, const double y, const double z, const int pj, const double lbi, const double tx,
                              const double ty, const double tz, const double sep) {
            const double nx = U[0] * x + U[1] * y + U[2] * z + U[3];
            const double ny = U[4] * x + U[5] * y + U[6] * z + U[7];
            const double nz = U[8] * x + U[9] * y + U[10] * z + U[11];
            P[3 * (size_t)i] = nx; P[3 * (size_t)i + 1] = ny; P[3 * (size_t)i + 2] = nz;
            // how far this point's search will reach (the same tests as the queue below): nothing when its previous
            // correspondence is certified or it is provably out of range, the distance to the previous correspondence, or
            // kFarMargin x max_dist for a point without one
            double reach = 0.0;
            if (pj < 0) {
                const double nlb = lbi - (sqrt(sqdist(nx, ny, nz, x, y, z)) * (1.0 + 1e-9) + 1e-12);
                lb[i] = nlb;
                if (!(nlb > lb_need)) reach = far;
            } else {
                const double d = sqdist(nx, ny, nz, tx, ty, tz);
                if (!(d < r2 && 4.0 * d * (1.0 + 1e-9) < sep)) reach = sqrt(d < r2 ? d : r2);
            }
            reach = reach * (1.0 + 1e-6) + 1e-9;
            xmn = fmin(xmn, nx - reach); xmx = fmax(xmx, nx + reach);
        };
        if (pf) move_point(i_pf, pfx, pfy, pfz, pfj, pflb, pftx, pfty, pftz, pfsep);
        for (int i = i_pf + kSearchWG; i < i_hi; i += kSearchWG) {
            const int pj = prev[i];
            double tx = 0, ty = 0, tz = 0, sep = 0;
            if (pj >= 0) { tx = T[3 * (size_t)pj]; ty = T[3 * (size_t)pj + 1]; tz = T[3 * (size_t)pj + 2]; sep = cov[(size_t)pj * kIcpCovStride + 10]; }
            move_point(i, P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], pj, lb[i], tx, ty, tz, sep);
        }
    }
    // the x slab of the grid this slice's searches can reach: a contiguous range of cells [c0, c1] and of sorted target
    // points [p0, p1), staged in LDS when it fits (sized by the actual search radii: once most points keep their
    // correspondence the slab is a few columns, not the kFarMargin x max_dist margin on either side)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { xmn = fmin(xmn, shfl_xor_d(xmn, o)); xmx = fmax(xmx, shfl_xor_d(xmx, o)); }
    if (lane == 0) { s_xmm[wave][0] = xmn; s_xmm[wave][1] = xmx; }
    __syncthreads();
    for (int w = 0; w < kSearchWG / 64; ++w) { xmn = fmin(xmn, s_xmm[w][0]); xmx = fmax(xmx, s_xmm[w][1]); }
    const int xlo = grid_coord(xmn, minx, inv, gx), xhi = grid_coord(xmx, minx, inv, gx);
    const int c0 = xlo * gy, c1 = (xhi + 1) * gy;
    const int c0a = c0 & ~7;                                  // 16-byte aligned start of the table copy
    const int p0 = cs[c0], p1 = cs[c1];
    const int np = p1 - p0;
    const bool kLds = np <= kSlabPts && c1 - c0a + 1 <= kSlabCells && nt < 65536;
    if (tid == 0) {                                          // diagnostics: slices whose slab did not fit LDS, largest slab seen
        if (!kLds) atomicAdd((unsigned long long*)&S.clk[6], 1ull);
        atomicMax((unsigned long long*)&S.clk[7], (unsigned long long)np);
    }
    if (kLds) {                                              // 16-byte copies of the prepared records / 16-bit cell table
        const uint4* src = reinterpret_cast<const uint4*>(B.tgt_rec + (size_t)h * B.cap + p0);
        uint4* dst = reinterpret_cast<uint4*>(s_tgt);
        for (int j = tid; j < np * 2; j += kSearchWG) dst[j] = src[j];
        const uint4* csrc = reinterpret_cast<const uint4*>(B.cell_start16 + (size_t)h * kIcpCells16 + c0a);
        uint4* cdst = reinterpret_cast<uint4*>(s_cs);
        for (int j = tid; j < (c1 - c0a + 8) / 8; j += kSearchWG) cdst[j] = csrc[j];
    }
    __syncthreads();
    const long long t2 = (long long)__builtin_amdgcn_s_memtime();
    long long t_a2 = 0;

    // target point j (sorted position): from the staged slab when it is inside (always, for the candidates of a search;
    // a previous correspondence may have been left behind by a large update)
    auto tgt_xyz = [&](int j, double& x, double& y, double& z) {
        if (kLds && (unsigned)(j - p0) < (unsigned)np) { const TgtRec& r = s_tgt[j - p0]; x = r.x; y = r.y; z = r.z; }
        else { x = T[3 * (size_t)j]; y = T[3 * (size_t)j + 1]; z = T[3 * (size_t)j + 2]; }
    };
    auto tgt_orig = [&](int j) { return (kLds && (unsigned)(j - p0) < (unsigned)np) ? s_tgt[j - p0].orig : orig[j]; };
    auto tgt_zq = [&](int j) { return (kLds && (unsigned)(j - p0) < (unsigned)np) ? s_tgt[j - p0].zq : rec[j].zq; };
    auto cell_at = [&](int c) { return kLds ? (int)s_cs[c - c0a] : cs[c]; };

    for (int base = i_lo; base < i_hi; base += kLoopQueue) {
        const int end = base + kLoopQueue < i_hi ? base + kLoopQueue : i_hi;
        if (tid < kClasses) s_cnt[tid] = 0;
        __syncthreads();
        for (int i0 = base; i0 < end; i0 += kSearchWG) {
            const int i = i0 + tid;
            const int pj = i < end ? prev[i] : -2;
            bool need = i < end;
            int cls = kClasses;
            if (need) {
                const double px = P[3 * (size_t)i], py = P[3 * (size_t)i + 1], pz = P[3 * (size_t)i + 2];
                double bd0 = far2;
                if (pj >= 0) {
                    double qx, qy, qz;
                    tgt_xyz(pj, qx, qy, qz);
                    const double d = sqdist(px, py, pz, qx, qy, qz);
                    need = !(d < r2 && 4.0 * d * (1.0 + 1e-9) < cov[(size_t)pj * kIcpCovStride + 10]);
                    bd0 = d < r2 ? d : r2;
                } else {
                    need = !(lb[i] > lb_need);          // nearest target provably beyond max_dist: still no correspondence
                }
                if (need) {
                    const double rad = sqrt(bd0) * (1.0 + 1e-9) + 1e-12;
                    const int nxc = grid_coord(px + rad, minx, inv, gx) - grid_coord(px - rad, minx, inv, gx) + 1;
                    const int nyc = grid_coord(py + rad, miny, inv, gy) - grid_coord(py - rad, miny, inv, gy) + 1;
                    const int ncol = nxc * nyc;
                    cls = ncol <= 1 ? 0 : ncol <= 2 ? 1 : ncol <= 4 ? 2 : ncol <= 8 ? 3 : ncol <= 16 ? 4 : ncol <= 32 ? 5 : 6;   // lanes = 2^cls, one column each
                }
            }
            if (i < end) s_cls[i - base] = (unsigned char)cls;
#pragma unroll
            for (int c = 0; c < kClasses; ++c) {
                const unsigned long long m = __ballot(cls == c);
                if (m && lane == 0) atomicAdd(&s_cnt[c], __popcll(m));
            }
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int c = 0; c < kClasses; ++c) { s_cur[c] = run; run += s_cnt[c]; }
        }
        __syncthreads();
        for (int i0 = base; i0 < end; i0 += kSearchWG) {
            const int i = i0 + tid;
            const int cls = i < end ? (int)s_cls[i - base] : kClasses;
#pragma unroll
            for (int c = 0; c < kClasses; ++c) {
                const unsigned long long m = __ballot(cls == c);
                if (m) {                                      // one LDS atomic per wave and class reserves the slots
                    int qb = 0;
                    if (lane == 0) qb = atomicAdd(&s_cur[c], __popcll(m));
                    qb = __shfl(qb, 0, 64);
                    if (cls == c) s_q[qb + __popcll(m & ((1ull << lane) - 1ull))] = i;
                }
            }
        }
        __syncthreads();
        const long long ta = (long long)__builtin_amdgcn_s_memtime();
        // The queue is ordered by cost class; a point of class c gets 2^c lanes, one grid column each, so that the lanes of a
        // wave finish together — a search of kFarMargin x max_dist for a point without correspondence overlaps dozens of columns and
        // would otherwise hold 63 lanes up.  All classes in one sweep of the workgroup's lanes: the points are laid out over the lanes widest class first (so that a
        // point's 2^shift lanes are aligned and never straddle a wave), lane t finds its class in the table of lane offsets.
        // Walking the classes one after the other cost a latency-bound pass per non-empty class (five or six per evaluation).
        int lane_end[kClasses], q_start[kClasses], total_lanes = 0;
#pragma unroll
        for (int c = kClasses - 1; c >= 0; --c) {
            const int cnt = s_cnt[c];
            q_start[c] = s_cur[c] - cnt;                       // s_cur[c] = end of the class in the queue, after the scatter
            total_lanes += cnt << (c < max_shift ? c : max_shift);
            lane_end[c] = total_lanes;
        }
        for (int t0 = 0; t0 < total_lanes; t0 += kSearchWG) {
            const int t = t0 + tid;
            const bool active = t < total_lanes;
            int cq = 0, lane0 = lane_end[1], qs = q_start[0];
#pragma unroll
            for (int c = kClasses - 1; c >= 1; --c) {
                const int first = c == kClasses - 1 ? 0 : lane_end[c + 1];
                if (t >= first && t < lane_end[c]) { cq = c; lane0 = first; qs = q_start[c]; }
            }
            const int lpp_shift = cq < max_shift ? cq : max_shift, lpp = 1 << lpp_shift;
            const int sub = (t - lane0) & (lpp - 1);
            const int i = active ? s_q[qs + ((t - lane0) >> lpp_shift)] : i_lo;
            const double px = P[3 * (size_t)i], py = P[3 * (size_t)i + 1], pz = P[3 * (size_t)i + 2];
            const int pj = prev[i];
            // a point without correspondence searches kFarMargin x max_dist once: the distance it finds (or the search
            // radius) minus its later motion is the lower bound that keeps it out of the queue (A1)
            const double bound2 = pj >= 0 ? r2 : far2;
            double bd = bound2;
            int bo = INT_MAX, bp = -1;
            if (pj >= 0) {
                double qx, qy, qz;
                tgt_xyz(pj, qx, qy, qz);
                const double d = sqdist(px, py, pz, qx, qy, qz);
                if (d < bd) { bd = d; bo = tgt_orig(pj); bp = pj; }
            }
            if (active && nt > 0 && px == px && py == py && pz == pz) {
                // every target with d <= bd lies in the cube of half-width sqrt(bd) around p: the columns overlapping it,
                // cut to its depth range, suffice
                const double rad = sqrt(bd) * (1.0 + 1e-9) + 1e-12;
                const int xa = grid_coord(px - rad, minx, inv, gx), xb = grid_coord(px + rad, minx, inv, gx);
                const int ya = grid_coord(py - rad, miny, inv, gy), yb = grid_coord(py + rad, miny, inv, gy);
                const int zlo = zq_of(pz - rad, minz, inv_z, zq_max), zhi = zq_of(pz + rad, minz, inv_z, zq_max);
                const int nxc = xb - xa + 1, ncol = nxc * (yb - ya + 1);
                const float inv_nxc = 1.0f / (float)nxc;
                for (int r = sub; r < ncol; r += lpp) {            // one column per lane and trip
                    const int yy = (int)(((float)r + 0.5f) * inv_nxc);       // r / nxc, exact for these small integers
                    const int c = (xa + (r - yy * nxc)) * gy + ya + yy;
                    int a = cell_at(c);
                    const int b = cell_at(c + 1);
                    if (b - a > 8) {                              // long run: first point at depth step >= zlo by bisection (the run is depth-ordered)
                        int hi = b;
                        while (a < hi) { const int mid = (a + hi) >> 1; if (tgt_zq(mid) < zlo) a = mid + 1; else hi = mid; }
                    }
                    // four candidates per trip (independent LDS reads in flight); indices past the run are
                    // clamped to its last point, which only re-tests a candidate; past depth step zhi the run is done
                    for (int j0 = a; j0 < b; j0 += 4) {
                        double d4[4];
                        int j4[4];
                        bool more = true;
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            j4[v] = j0 + v < b ? j0 + v : b - 1;
                            double qx, qy, qz;
                            tgt_xyz(j4[v], qx, qy, qz);
                            d4[v] = sqdist(px, py, pz, qx, qy, qz);
                            if (tgt_zq(j4[v]) > zhi) more = false;
                        }
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int j = j4[v];
                            const double d = d4[v];
                            if (d < bd) { bd = d; bo = tgt_orig(j); bp = j; }
                            else if (d == bd && bp >= 0 && bp != j) { const int o = tgt_orig(j); if (o < bo) { bo = o; bp = j; } }
                        }
                        if (!more) break;
                    }
                }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {          // combine the lanes that shared the point (every lane makes every exchange)
                const double od = shfl_xor_d(bd, off);
                const int oo = __shfl_xor(bo, off, 64), op = __shfl_xor(bp, off, 64);
                if (off < lpp && op >= 0 && (od < bd || (od == bd && oo < bo))) { bd = od; bo = oo; bp = op; }
            }
            if (active && sub == 0) {
                if (bp >= 0 && !(bd < r2)) bp = -1;          // seen, but not a correspondence (d^2 < max_dist^2 required)
                prev[i] = bp;
                if (bp < 0) lb[i] = sqrt(bd);                 // every target closer than sqrt(bound2) was visited
            }
        }
        __syncthreads();
        t_a2 += (long long)__builtin_amdgcn_s_memtime() - ta;
    }
    const long long t3 = (long long)__builtin_amdgcn_s_memtime();
    // --- JtJ / Jtr of TransformationEstimationPointToPlane over the correspondences of the slice ---
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    for (int i = i_lo + tid; i < i_hi; i += kSearchWG) {
        const int bp = prev[i];
        if (bp < 0) continue;
        const double px = P[3 * (size_t)i], py = P[3 * (size_t)i + 1], pz = P[3 * (size_t)i + 2];
        double qx, qy, qz;
        tgt_xyz(bp, qx, qy, qz);
        const double bd = sqdist(px, py, pz, qx, qy, qz);
        if constexpr (P2P) {
            acc[0] += px; acc[1] += py; acc[2] += pz;
            acc[3] += qx; acc[4] += qy; acc[5] += qz;
            acc[6] += qx * px; acc[7] += qx * py; acc[8] += qx * pz;
            acc[9] += qy * px; acc[10] += qy * py; acc[11] += qy * pz;
            acc[12] += qz * px; acc[13] += qz * py; acc[14] += qz * pz;
            acc[27] += bd;
            acc[28] += 1.0;
        } else {
            const double nx = N[3 * (size_t)bp], ny = N[3 * (size_t)bp + 1], nz = N[3 * (size_t)bp + 2];
            const double r = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;
            const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) acc[k++] += J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
            acc[27] += bd;
            acc[28] += 1.0;
        }
    }
    {
        const double v = wave_reduce32(acc, lane);
        if ((lane & 1) == 0) s_part[wave][lane >> 1] = v;
    }
    __syncthreads();
    if (tid < 32) {
        double v = 0;
        for (int w = 0; w < kSearchWG / 64; ++w) v += s_part[w][tid];
        double* dst = B.partial + ((((size_t)(it & 1) * B.count + h) * kIcpMaxSplit) + g) * 32 + tid;
        if (tid >= 29) {   // diagnostics in the padding: shader cycles of this slice's evaluation (total, search, prologue)
            const long long tn = (long long)__builtin_amdgcn_s_memtime();
            v = tid == 29 ? (double)(tn - t0) : tid == 30 ? (double)t_a2 : (double)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3] + s_cnt[4] + s_cnt[5] + s_cnt[6] + s_cnt[7]);
        }
        *dst = v;
    }
    if (g == 0 && tid == 0) {      // shader-cycle split of workgroup 0 (diagnostics): prologue, staging+transform, queue, search, sums
        const long long t4 = (long long)__builtin_amdgcn_s_memtime();
        S.clk[0] += t1 - t0; S.clk[1] += t2 - t1; S.clk[2] += (t3 - t2) - t_a2; S.clk[3] += t_a2; S.clk[4] += t4 - t3; S.clk[5] += 1;
    }
    return false;
}

template <bool P2P>
__global__ void __launch_bounds__(kSearchWG, 3)
k_icp_eval(IcpBuffers B, int it, int prev_slices, int max_shift, double max_dist, int max_iter, double rel_fit, double rel_rmse) {
    __shared__ TgtRec s_tgt[kSlabPts];
    __shared__ __attribute__((aligned(16))) unsigned short s_cs[kSlabCells + 8];
    __shared__ int s_q[kLoopQueue];
    __shared__ unsigned char s_cls[kLoopQueue];
    const int h = blockIdx.y;
    IcpState& S = B.st[h];
    if (S.status != 0 || S.stop != 0) return;
    (void)icp_eval_body<P2P>(B, S, h, it, prev_slices, max_shift, s_tgt, s_cs, s_q, s_cls, max_dist, max_iter, rel_fit, rel_rmse, S.fit_hist, S.rmse_hist);
}

// the sliced launches of evaluations [it_from, max_iter + 1]: evaluation `it` is finished (convergence test, solve, update) by the prologue
// of launch it + 1.  The first evaluations have every hypothesis at work (768 workgroups = three per CU); by the sixth most have
// converged and the ones that go on for all 30 are cut finer (their latency is what is left): 64 slices each
static int icp_slices(int count, int it) {
    const Knobs& kn = knobs();
    int splits = 768 / count;                                        // enough workgroups to cover the chip, at least ~128 source points each at typical sizes
    if (kn.icp_splits > 0) splits = kn.icp_splits;                     // tuning knob (profiles/)
    if (splits > kIcpMaxSplit) splits = kIcpMaxSplit;
    if (splits < 1) splits = 1;
    return it < kIcpFineFrom || kn.icp_splits > 0 ? splits : kIcpMaxSplit;
}

hipError_t launch_icp_evals(const IcpBuffers& B, int count, int it_from, int it_to, bool p2p, double max_dist, int max_iter, double rel_fit, double rel_rmse,
                      hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const Knobs& kn = knobs();
#ifdef LM_DIAG
    if (kn.icp_maxiter_diag >= 0) max_iter = kn.icp_maxiter_diag;            // diagnostics only (profiles/): stop after a few evaluations
#endif
    if (it_to > max_iter + 1) it_to = max_iter + 1;
    for (int it = it_from; it <= it_to; ++it) {
        // lanes per searching point: at most 8 while every point searches (the first evaluations: more lanes only multiply the
        // set-up), 16 afterwards (few searches left: their latency is what counts) — measured, profiles/r02_icp_experiments.txt
        LAUNCH_TRY(lm_launch(p2p ? k_icp_eval<true> : k_icp_eval<false>, dim3(icp_slices(count, it), count), dim3(kSearchWG), 0, s, B, it,
                             it > 0 ? icp_slices(count, it - 1) : 1, it < kIcpFineFrom ? kn.icp_maxshift : kn.icp_maxshift_late, max_dist, max_iter,
                             rel_fit, rel_rmse));
    }
    return hipSuccess;
}

}  // namespace lm
