// Pose errors of a batch of estimates against a batch of ground truths (pysixd/pose_error.py vsd / cou / add / adi /
// re / te, the loop of tools/eval_calc_errors.py:142-172) and the GT statistics of tools/calc_gt_stats.py:103-155.
//
// VSD and COU: the E + G views are rendered by lm_mesh_render_device (R, t, K cast to float32, as the renderer of
// lm_mesh_render) and read as float32 eye depth from the z-buffer keys; then one k_vsd pass per (estimate, GT) pair.
// ADD / ADI / diameter: k_pose_pts.  RE / TE: here, f64.  MSSD / MSPD (lm_mesh_pose_errors_sym): the composed GT-side
// transforms here in f64, then k_pose_sym and k_pose_sym_min.
//
// Deliberate differences from pysixd (also DESIGN.md, "Pose errors"):
//   * the renders are this project's rasteriser, not OpenGL: its fill rule, no near-plane clipping (a triangle with a
//     vertex behind the camera is dropped), depth interpolated in f64 and stored as float32;
//   * ADI searches the nearest point in f32 in the GT model frame and re-evaluates that one distance in f64: within
//     ~1e-5 mm of scipy's cKDTree where two candidates are that close;
//   * sums run in a fixed order different from numpy's pairwise sum (tlinear VSD, ADD, ADI: last-ulp differences);
//   * inv(R_g) is the f64 adjugate inverse, not LAPACK's LU (RE: ~1e-16 in the cosine);
//   * bbox_obj projects the vertices with ((P0 x + P1 y) + P2 z) + P3, not numpy's dot (differs only on a .5 tie).
// Scratch buffers (scene, pairs, partials, and the render buffers of lm_mesh_render_device) live in lm_mesh; every
// render call re-renders what it returns, so lm_mesh_render and the detector / pipeline paths see no difference.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pose_error_kernels.h"
#include "render_internal.h"

using namespace lm;

namespace {

constexpr size_t kZbufBudget = (size_t)512 << 20;   // bytes of z-buffer (8 B per pixel) per render call
constexpr int kMaxViewsPerRender = 256;              // keeps the pair grid (views^2 / 4) below the launch limit
constexpr int kMaxPtsPairs = 16384;                  // pairs per k_pose_pts / k_pose_sym launch
constexpr size_t kSymPartialBudget = (size_t)256 << 20;   // bytes of k_pose_sym partials per launch (one pair may exceed it)

bool inv3(const double* A, double* B) {
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return false;
    B[0] = c00 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
    B[3] = c01 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
    B[6] = c02 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
    return true;
}
void matmul3(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

int views_per_render(int W, int H) {
    const size_t per = (size_t)W * H * sizeof(unsigned long long);
    return (int)std::max<size_t>(2, std::min<size_t>(kMaxViewsPerRender, kZbufBudget / per));
}

// renders views [R_a(i0..i0+na), R_b(j0..j0+nb)] into m->d_zbuf (depth only, float32 poses)
int render_views(lm_mesh* m, int W, int H, const double* K, const double* Ra, const double* ta, int na, const double* Rb,
                 const double* tb, int nb, double clip_near, double clip_far) {
    const int n = na + nb;
    std::vector<float> Ks((size_t)9 * n), Rs((size_t)9 * n), ts((size_t)3 * n);
    for (int i = 0; i < n; ++i) {
        const double* R = i < na ? Ra + 9 * (size_t)i : Rb + 9 * (size_t)(i - na);
        const double* t = i < na ? ta + 3 * (size_t)i : tb + 3 * (size_t)(i - na);
        for (int k = 0; k < 9; ++k) { Ks[9 * (size_t)i + k] = (float)K[k]; Rs[9 * (size_t)i + k] = (float)R[k]; }
        for (int k = 0; k < 3; ++k) ts[3 * (size_t)i + k] = (float)t[k];
    }
    return lm_mesh_render_device(m, n, W, H, Ks.data(), Rs.data(), ts.data(), (float)clip_near, (float)clip_far, 0.f, 1, true, false);
}

bool finite_all(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!isfinite(p[i])) return false;
    return true;
}

PixCam pix_cam(const double* K) { return PixCam{1.0 / K[0], 1.0 / K[4], K[2], K[5]}; }

int check_image(const double* K, int W, int H) {
    if (!K) return lm_set_error(LM_ERR_INVALID, "K is required for rendered metrics");
    if (W <= 0 || H <= 0 || (long long)W * H >= (1ll << 31)) return lm_set_error(LM_ERR_INVALID, "bad image size %dx%d", W, H);
    if (!finite_all(K, 9) || K[0] == 0.0 || K[4] == 0.0) return lm_set_error(LM_ERR_INVALID, "K must be finite with fx, fy != 0");
    return LM_OK;
}

int upload_scene(lm_mesh* m, const float* scene, int W, int H) {
    const size_t n = (size_t)W * H;
    int rc = m->d_scene.ensure(n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m->d_scene.p, scene, n * sizeof(float), hipMemcpyHostToDevice, m->s));
    return LM_OK;
}

// ADD / ADI sums (or the diameter) of `pairs`: out_add[p], out_adi[p] = sums over the vertices (max for the diameter)
int run_pts(lm_mesh* m, const std::vector<PtsPair>& pairs, int mode, std::vector<double>& out_add, std::vector<double>& out_b) {
    const int chunks = (m->nv + kPtsChunk - 1) / kPtsChunk;
    const int npairs = (int)pairs.size();
    out_add.assign(npairs, 0.0); out_b.assign(npairs, 0.0);
    std::vector<PtsPartial> part;
    for (int p0 = 0; p0 < npairs; p0 += kMaxPtsPairs) {
        const int np = std::min(kMaxPtsPairs, npairs - p0);
        int rc;
        if ((rc = m->d_pe_pairs.ensure((size_t)np * sizeof(PtsPair)))) return rc;
        if ((rc = m->d_pe_partial.ensure((size_t)np * chunks * sizeof(PtsPartial)))) return rc;
        HIP_TRY(hipMemcpyAsync(m->d_pe_pairs.p, pairs.data() + p0, (size_t)np * sizeof(PtsPair), hipMemcpyHostToDevice, m->s));
        HIP_TRY(launch_pose_pts(m->d_v.p, m->nv, (const PtsPair*)m->d_pe_pairs.p, np, mode, (PtsPartial*)m->d_pe_partial.p, m->s));
        part.resize((size_t)np * chunks);
        HIP_TRY(hipMemcpyAsync(part.data(), m->d_pe_partial.p, part.size() * sizeof(PtsPartial), hipMemcpyDeviceToHost, m->s));
        HIP_TRY(hipStreamSynchronize(m->s));
        for (int p = 0; p < np; ++p) {
            double a = 0.0, b = 0.0;
            for (int c = 0; c < chunks; ++c) {                          // chunk order: fixed
                const PtsPartial& q = part[(size_t)p * chunks + c];
                a += q.add;
                b = mode == kPtsDiameter ? std::max(b, q.adi) : b + q.adi;
            }
            out_add[p0 + p] = a; out_b[p0 + p] = b;
        }
    }
    return LM_OK;
}

}  // namespace

extern "C" int lm_mesh_pose_errors(lm_mesh* m, int n_est, const double* R_est, const double* t_est, int n_gt, const double* R_gt,
                                   const double* t_gt, const double* K, int width, int height, const float* scene_depth, int metrics,
                                   double delta, double tau, int cost, double clip_near, double clip_far, double* out) {
    if (!m) return lm_set_error(LM_ERR_INVALID, "null mesh");
    if (n_est < 0 || n_gt < 0) return lm_set_error(LM_ERR_INVALID, "negative pose count");
    const int all = LM_POSE_VSD | LM_POSE_COU | LM_POSE_ADD | LM_POSE_ADI | LM_POSE_RE | LM_POSE_TE;
    if (metrics & (LM_POSE_MSSD | LM_POSE_MSPD))
        return lm_set_error(LM_ERR_INVALID, "LM_POSE_MSSD / LM_POSE_MSPD take a symmetry set: call lm_mesh_pose_errors_sym");
    if (metrics == 0 || (metrics & ~all)) return lm_set_error(LM_ERR_INVALID, "bad metrics mask 0x%x", metrics);
    const bool rendered = metrics & (LM_POSE_VSD | LM_POSE_COU);
    if (metrics & LM_POSE_VSD) {
        if (!scene_depth) return lm_set_error(LM_ERR_INVALID, "vsd needs the scene depth (scene_depth is NULL)");
        if (cost != LM_POSE_COST_STEP && cost != LM_POSE_COST_TLINEAR) return lm_set_error(LM_ERR_INVALID, "unknown vsd cost %d", cost);
        if (!(tau > 0.0) || !isfinite(tau) || !isfinite(delta)) return lm_set_error(LM_ERR_INVALID, "vsd needs tau > 0 and a finite delta");
    }
    if (rendered) {
        int rc = check_image(K, width, height);
        if (rc) return rc;
        if (!(clip_near > 0.0) || !(clip_far > clip_near)) return lm_set_error(LM_ERR_INVALID, "need 0 < clip_near < clip_far");
    }
    if (n_est == 0 || n_gt == 0) return LM_OK;
    if (!R_est || !t_est || !R_gt || !t_gt || !out) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!finite_all(R_est, 9 * (size_t)n_est) || !finite_all(t_est, 3 * (size_t)n_est) || !finite_all(R_gt, 9 * (size_t)n_gt) ||
        !finite_all(t_gt, 3 * (size_t)n_gt))
        return lm_set_error(LM_ERR_INVALID, "non-finite pose");
    HIP_TRY(hipSetDevice(m->device));

    const size_t EG = (size_t)n_est * n_gt;
    int slot[6], nm = 0;
    for (int b = 0; b < 6; ++b) slot[b] = (metrics >> b) & 1 ? nm++ : -1;
    auto at = [&](int bit, int e, int g) -> double& { return out[(size_t)slot[bit] * EG + (size_t)e * n_gt + g]; };

    // RE / TE (pose_error.py:154-180), host f64
    std::vector<double> Rg_inv((size_t)9 * n_gt);
    for (int g = 0; g < n_gt; ++g)
        if (!inv3(R_gt + 9 * (size_t)g, &Rg_inv[9 * (size_t)g])) return lm_set_error(LM_ERR_INVALID, "GT rotation %d is singular", g);
    for (int e = 0; e < n_est; ++e)
        for (int g = 0; g < n_gt; ++g) {
            const double* Re = R_est + 9 * (size_t)e;
            const double* Gi = &Rg_inv[9 * (size_t)g];
            if (slot[4] >= 0) {
                double C[9];
                matmul3(Re, Gi, C);
                double c = 0.5 * (((C[0] + C[4]) + C[8]) - 1.0);
                c = std::min(1.0, std::max(-1.0, c));
                at(4, e, g) = 180.0 * acos(c) / M_PI;
            }
            if (slot[5] >= 0) {
                const double* te = t_est + 3 * (size_t)e;
                const double* tg = t_gt + 3 * (size_t)g;
                const double dx = tg[0] - te[0], dy = tg[1] - te[1], dz = tg[2] - te[2];
                at(5, e, g) = sqrt((dx * dx + dy * dy) + dz * dz);
            }
        }

    // ADD / ADI (pose_error.py:117-152): k_pose_pts
    if (metrics & (LM_POSE_ADD | LM_POSE_ADI)) {
        std::vector<PtsPair> pairs(EG);
        for (int e = 0; e < n_est; ++e)
            for (int g = 0; g < n_gt; ++g) {
                PtsPair& P = pairs[(size_t)e * n_gt + g];
                const double* Re = R_est + 9 * (size_t)e;
                const double* te = t_est + 3 * (size_t)e;
                const double* Rg = R_gt + 9 * (size_t)g;
                const double* tg = t_gt + 3 * (size_t)g;
                const double* Gi = &Rg_inv[9 * (size_t)g];
                double M[9];
                matmul3(Gi, Re, M);
                const double d[3] = {te[0] - tg[0], te[1] - tg[1], te[2] - tg[2]};
                for (int k = 0; k < 9; ++k) { P.M[k] = (float)M[k]; P.Re[k] = Re[k]; P.Rg[k] = Rg[k]; }
                for (int k = 0; k < 3; ++k) {
                    P.c[k] = (float)((Gi[3 * k] * d[0] + Gi[3 * k + 1] * d[1]) + Gi[3 * k + 2] * d[2]);
                    P.te[k] = te[k]; P.tg[k] = tg[k];
                }
            }
        std::vector<double> s_add, s_adi;
        int rc = run_pts(m, pairs, (metrics & LM_POSE_ADI) ? kPtsAdi : kPtsAddOnly, s_add, s_adi);
        if (rc) return rc;
        for (size_t p = 0; p < EG; ++p) {
            const int e = (int)(p / n_gt), g = (int)(p % n_gt);
            if (slot[2] >= 0) at(2, e, g) = s_add[p] / m->nv;
            if (slot[3] >= 0) at(3, e, g) = s_adi[p] / m->nv;
        }
    }

    // VSD / COU (pose_error.py:12-115): renders of G + E views, then one k_vsd pass per pair
    if (rendered) {
        const bool want_vsd = metrics & LM_POSE_VSD;
        int rc;
        if (want_vsd && (rc = upload_scene(m, scene_depth, width, height))) return rc;
        const int cap = views_per_render(width, height);
        int gch = n_gt, ech = n_est;
        if (n_gt + n_est > cap) { gch = std::min(n_gt, std::max(1, cap / 2)); ech = std::min(n_est, cap - gch); }
        const int nblk = pix_blocks(width * height);
        const PixCam cam = pix_cam(K);
        std::vector<VsdPartial> part;
        for (int g0 = 0; g0 < n_gt; g0 += gch) {
            const int ng = std::min(gch, n_gt - g0);
            for (int e0 = 0; e0 < n_est; e0 += ech) {
                const int ne = std::min(ech, n_est - e0);
                if ((rc = render_views(m, width, height, K, R_gt + 9 * (size_t)g0, t_gt + 3 * (size_t)g0, ng, R_est + 9 * (size_t)e0,
                                       t_est + 3 * (size_t)e0, ne, clip_near, clip_far)))
                    return rc;
                const size_t np = (size_t)ng * ne;
                if ((rc = m->d_pe_partial.ensure(np * nblk * sizeof(VsdPartial)))) return rc;
                HIP_TRY(launch_vsd(m->d_zbuf.p, 0, ng, ng, ne, want_vsd ? m->d_scene.p : nullptr, width, height, cam, (float)delta, 1.0 / tau, tau,
                                   (VsdPartial*)m->d_pe_partial.p, m->s));
                part.resize(np * nblk);
                HIP_TRY(hipMemcpyAsync(part.data(), m->d_pe_partial.p, part.size() * sizeof(VsdPartial), hipMemcpyDeviceToHost, m->s));
                HIP_TRY(hipStreamSynchronize(m->s));
                for (size_t p = 0; p < np; ++p) {
                    const int g = g0 + (int)(p / ne), e = e0 + (int)(p % ne);
                    double tl = 0.0;
                    long long vu = 0, vi = 0, st = 0, ci = 0, cu = 0;
                    for (int b = 0; b < nblk; ++b) {                    // block order: fixed
                        const VsdPartial& q = part[p * nblk + b];
                        tl += q.tl;
                        vu += q.vis_union; vi += q.vis_inter; st += q.step; ci += q.cou_inter; cu += q.cou_union;
                    }
                    if (want_vsd) {
                        const double costs = cost == LM_POSE_COST_STEP ? (double)st : tl;
                        at(0, e, g) = vu > 0 ? (costs + (double)(vu - vi)) / (double)vu : 1.0;
                    }
                    if (slot[1] >= 0) at(1, e, g) = cu > 0 ? 1.0 - (double)ci / (double)cu : 1.0;
                }
            }
        }
    }
    return LM_OK;
}

extern "C" int lm_pose_sym_tile(void) { return kSymTile; }

extern "C" int lm_mesh_pose_errors_sym(lm_mesh* m, int n_est, const double* R_est, const double* t_est, int n_gt, const double* R_gt,
                                       const double* t_gt, int n_sym, const double* R_sym, const double* t_sym, const double* K, int metrics,
                                       double* out) {
    if (!m) return lm_set_error(LM_ERR_INVALID, "null mesh");
    if (n_est < 0 || n_gt < 0) return lm_set_error(LM_ERR_INVALID, "negative pose count");
    if (metrics == 0 || (metrics & ~(LM_POSE_MSSD | LM_POSE_MSPD)))
        return lm_set_error(LM_ERR_INVALID, "bad metrics mask 0x%x (LM_POSE_MSSD | LM_POSE_MSPD)", metrics);
    if (n_sym < 1) return lm_set_error(LM_ERR_INVALID, "n_sym = %d: the symmetry set holds at least the identity", n_sym);
    const bool mssd = metrics & LM_POSE_MSSD, mspd = metrics & LM_POSE_MSPD;
    if (mspd && !K) return lm_set_error(LM_ERR_INVALID, "mspd needs K (K is NULL)");
    if (mspd && !finite_all(K, 9)) return lm_set_error(LM_ERR_INVALID, "K must be finite");
    if (!R_sym || !t_sym) return lm_set_error(LM_ERR_INVALID, "null symmetry set");
    if (!finite_all(R_sym, 9 * (size_t)n_sym) || !finite_all(t_sym, 3 * (size_t)n_sym)) return lm_set_error(LM_ERR_INVALID, "non-finite symmetry");
    if (n_est == 0 || n_gt == 0) return LM_OK;
    if (!R_est || !t_est || !R_gt || !t_gt || !out) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!finite_all(R_est, 9 * (size_t)n_est) || !finite_all(t_est, 3 * (size_t)n_est) || !finite_all(R_gt, 9 * (size_t)n_gt) ||
        !finite_all(t_gt, 3 * (size_t)n_gt))
        return lm_set_error(LM_ERR_INVALID, "non-finite pose");
    if ((size_t)n_gt * n_sym > ((size_t)1 << 24)) return lm_set_error(LM_ERR_INVALID, "n_gt * n_sym = %zu is too large", (size_t)n_gt * n_sym);
    HIP_TRY(hipSetDevice(m->device));

    // A[g][s] = R_g R_s, b[g][s] = R_g t_s + t_g, once per call
    const size_t nxf = (size_t)n_gt * n_sym;
    std::vector<SymXf> xf(nxf);
    for (int g = 0; g < n_gt; ++g)
        for (int s = 0; s < n_sym; ++s) {
            SymXf& X = xf[(size_t)g * n_sym + s];
            const double* Rg = R_gt + 9 * (size_t)g;
            const double* ts = t_sym + 3 * (size_t)s;
            matmul3(Rg, R_sym + 9 * (size_t)s, X.A);
            for (int r = 0; r < 3; ++r) X.b[r] = ((Rg[3 * r] * ts[0] + Rg[3 * r + 1] * ts[1]) + Rg[3 * r + 2] * ts[2]) + t_gt[3 * (size_t)g + r];
        }
    SymCam cam;
    for (int k = 0; k < 9; ++k) cam.K[k] = K ? K[k] : 0.0;

    const size_t EG = (size_t)n_est * n_gt;
    const int nm = (mssd ? 1 : 0) + (mspd ? 1 : 0), chunks = sym_chunks(m->nv);
    const size_t per_pair = (size_t)chunks * nm * n_sym;                // partial doubles of one pair
    const size_t batch = std::max<size_t>(1, std::min<size_t>(kMaxPtsPairs, (kSymPartialBudget / sizeof(double)) / per_pair));
    const size_t xf_bytes = nxf * sizeof(SymXf);
    std::vector<SymPair> pairs;
    std::vector<double> res;
    for (size_t p0 = 0; p0 < EG; p0 += batch) {
        const size_t np = std::min(batch, EG - p0);
        pairs.resize(np);
        for (size_t p = 0; p < np; ++p) {
            const size_t e = (p0 + p) / n_gt;
            memcpy(pairs[p].Re, R_est + 9 * e, sizeof(pairs[p].Re));
            memcpy(pairs[p].te, t_est + 3 * e, sizeof(pairs[p].te));
            pairs[p].g = (int)((p0 + p) % n_gt);
            pairs[p].pad = 0;
        }
        // one buffer holds the transforms and then the pairs; one holds the partials and then the results
        int rc;
        if ((rc = m->d_pe_pairs.ensure(xf_bytes + np * sizeof(SymPair)))) return rc;
        if ((rc = m->d_pe_partial.ensure((np * per_pair + np * nm) * sizeof(double)))) return rc;
        SymXf* d_xf = (SymXf*)m->d_pe_pairs.p;
        SymPair* d_pairs = (SymPair*)(m->d_pe_pairs.p + xf_bytes);
        double* d_partial = (double*)m->d_pe_partial.p;
        double* d_out = d_partial + np * per_pair;
        HIP_TRY(hipMemcpyAsync(d_xf, xf.data(), xf_bytes, hipMemcpyHostToDevice, m->s));   // again after ensure() may have moved the buffer
        HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), np * sizeof(SymPair), hipMemcpyHostToDevice, m->s));
        HIP_TRY(launch_pose_sym(m->d_v.p, m->nv, d_pairs, (int)np, d_xf, n_sym, cam, mssd, mspd, d_partial, d_out, m->s));
        res.resize(np * nm);
        HIP_TRY(hipMemcpyAsync(res.data(), d_out, res.size() * sizeof(double), hipMemcpyDeviceToHost, m->s));
        HIP_TRY(hipStreamSynchronize(m->s));
        for (size_t p = 0; p < np; ++p)
            for (int k = 0; k < nm; ++k) out[(size_t)k * EG + p0 + p] = res[p * nm + k];
    }
    return LM_OK;
}

extern "C" int lm_mesh_gt_stats(lm_mesh* m, int n_gt, const double* R_gt, const double* t_gt, const double* K, int width, int height,
                                const float* scene_depth, double delta, double clip_near, double clip_far, int64_t* counts,
                                double* visib_fract, int32_t* bbox_obj, int32_t* bbox_visib) {
    if (!m) return lm_set_error(LM_ERR_INVALID, "null mesh");
    if (n_gt < 0) return lm_set_error(LM_ERR_INVALID, "negative pose count");
    if (!scene_depth) return lm_set_error(LM_ERR_INVALID, "gt stats need the scene depth (scene_depth is NULL)");
    int rc = check_image(K, width, height);
    if (rc) return rc;
    if (!(clip_near > 0.0) || !(clip_far > clip_near)) return lm_set_error(LM_ERR_INVALID, "need 0 < clip_near < clip_far");
    if (!isfinite(delta)) return lm_set_error(LM_ERR_INVALID, "delta must be finite");
    if (n_gt == 0) return LM_OK;
    if (!R_gt || !t_gt || !counts || !visib_fract || !bbox_obj || !bbox_visib) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!finite_all(R_gt, 9 * (size_t)n_gt) || !finite_all(t_gt, 3 * (size_t)n_gt)) return lm_set_error(LM_ERR_INVALID, "non-finite pose");
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = upload_scene(m, scene_depth, width, height))) return rc;
    const int cap = views_per_render(width, height), nblk = pix_blocks(width * height);
    const PixCam cam = pix_cam(K);
    std::vector<GtPartial> part;
    for (int g0 = 0; g0 < n_gt; g0 += cap) {
        const int ng = std::min(cap, n_gt - g0);
        if ((rc = render_views(m, width, height, K, R_gt + 9 * (size_t)g0, t_gt + 3 * (size_t)g0, ng, nullptr, nullptr, 0, clip_near, clip_far)))
            return rc;
        if ((rc = m->d_pe_partial.ensure((size_t)ng * nblk * sizeof(GtPartial)))) return rc;
        HIP_TRY(launch_gt_stats(m->d_zbuf.p, ng, m->d_scene.p, width, height, cam, (float)delta, (GtPartial*)m->d_pe_partial.p, m->s));
        part.resize((size_t)ng * nblk);
        HIP_TRY(hipMemcpyAsync(part.data(), m->d_pe_partial.p, part.size() * sizeof(GtPartial), hipMemcpyDeviceToHost, m->s));
        HIP_TRY(hipStreamSynchronize(m->s));
        for (int i = 0; i < ng; ++i) {
            const int g = g0 + i;
            long long all = 0, valid = 0, visib = 0;
            int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
            for (int b = 0; b < nblk; ++b) {
                const GtPartial& q = part[(size_t)i * nblk + b];
                all += q.all; valid += q.valid; visib += q.visib;
                x0 = std::min(x0, q.minx); y0 = std::min(y0, q.miny); x1 = std::max(x1, q.maxx); y1 = std::max(y1, q.maxy);
            }
            counts[3 * (size_t)g] = all; counts[3 * (size_t)g + 1] = valid; counts[3 * (size_t)g + 2] = visib;
            visib_fract[g] = all > 0 ? (double)visib / (double)all : 0.0;
            int32_t* bv = bbox_visib + 4 * (size_t)g;
            if (visib > 0) { bv[0] = x0; bv[1] = y0; bv[2] = x1 - x0; bv[3] = y1 - y0; }
            else bv[0] = bv[1] = bv[2] = bv[3] = -1;
        }
    }
    // bbox_obj: misc.calc_pose_2d_bbox (projection of the model points, np.round, no clipping)
    std::vector<float> V((size_t)m->nv * 3);
    HIP_TRY(hipMemcpy(V.data(), m->d_v.p, V.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int g = 0; g < n_gt; ++g) {
        const double* R = R_gt + 9 * (size_t)g;
        const double* t = t_gt + 3 * (size_t)g;
        double P[12];                                                   // K [R | t]
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                const double b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
                P[4 * r + c] = (K[3 * r] * b0 + K[3 * r + 1] * b1) + K[3 * r + 2] * b2;
            }
        long long x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        for (int i = 0; i < m->nv; ++i) {
            const double x = V[3 * (size_t)i], y = V[3 * (size_t)i + 1], z = V[3 * (size_t)i + 2];
            double p[3];
            for (int r = 0; r < 3; ++r) p[r] = ((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3];
            const long long u = (long long)nearbyint(p[0] / p[2]), v = (long long)nearbyint(p[1] / p[2]);   // np.round: half to even
            if (i == 0 || u < x0) x0 = u;
            if (i == 0 || u > x1) x1 = u;
            if (i == 0 || v < y0) y0 = v;
            if (i == 0 || v > y1) y1 = v;
        }
        int32_t* bo = bbox_obj + 4 * (size_t)g;
        bo[0] = (int32_t)x0; bo[1] = (int32_t)y0; bo[2] = (int32_t)(x1 - x0); bo[3] = (int32_t)(y1 - y0);
    }
    return LM_OK;
}

extern "C" int lm_mesh_diameter(lm_mesh* m, double* diameter) {
    if (!m || !diameter) return lm_set_error(LM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    PtsPair P;
    memset(&P, 0, sizeof(P));
    P.M[0] = P.M[4] = P.M[8] = 1.f;
    P.Re[0] = P.Re[4] = P.Re[8] = P.Rg[0] = P.Rg[4] = P.Rg[8] = 1.0;
    std::vector<double> a, b;
    int rc = run_pts(m, std::vector<PtsPair>(1, P), kPtsDiameter, a, b);
    if (rc) return rc;
    *diameter = b[0];
    return LM_OK;
}
