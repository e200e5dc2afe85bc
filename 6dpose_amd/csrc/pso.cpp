// lm_pso — pose refinement by particle swarm over rendered depth (kernels and the rule: pso.hip), and over the
// scene's edges for cameras without depth (§5.3.1; pso_edges.hip): the same swarm with k_pso_edge_cost in k_pso_cost's place, or with
// k_pso_orient_cost against the scene's quantised orientations (§5.3.2; pso_orient.hip).
// A call enqueues, on the context's own stream, k_pso_init and then per generation k_pso_views, k_project, k_raster,
// k_pso_cost and k_pso_step; nothing is read back before the copy of the results.  The swarm renders into scratch of its
// own (projected vertices, z-buffer): the mesh is only read, so lm_mesh_render returns what it did before.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "detector_internal.h"
#include "pso_kernels.h"
#include "render_internal.h"

using namespace lm;

struct lm_pso {
    int device = 0;
    DevStream s;                          // first: every event and buffer below dies before it (dev_buf.h)
    DevEvent ev0, ev1;
    // the scene
    DevBuf<uint16_t> d_scene;
    int W = 0, H = 0;
    double K[9] = {0};
    // the edge scene (lm_pso_set_scene_edges): the map, its row distances g and the truncated squared distance D2; a frame and K of its own
    DevBuf<uint8_t> d_edges, d_g;
    DevBuf<uint16_t> d_d2;
    int eW = 0, eH = 0, eM = 0;
    double eK[9] = {0};
    // the oriented scene (lm_pso_set_scene_orientations, lm_pso_set_scene_from_detector): the map Q, per channel its row distances and D2_j,
    // and the nine planes DD2; a frame and K of its own
    DevBuf<uint8_t> d_q, d_og;
    DevBuf<uint16_t> d_od2, d_dd2;
    int oW = 0, oH = 0, oM = 0, oP = 0;
    double oK[9] = {0};
    // swarm state, render scratch and the record of the last run
    DevBuf<PsoHyp> d_hyp;
    DevBuf<ViewParams> d_views;
    DevBuf<ProjVtx> d_pv;
    DevBuf<unsigned long long> d_zbuf;
    DevBuf<double> x, v, pbest_x, pbest_cost, rec_x, rec_cost;   // what PsoState points to (pso_kernels.h: the sizes)
    DevBuf<unsigned long long> sum, rec_sum;
    DevBuf<unsigned int> n_r, rec_nr;
    DevBuf<PsoBest> best;
    DevBuf<int> rec_best;
    DevBuf<PsoResultDev> result;
    PsoState state() const {                 // the kernels' view of the buffers: taken after the run's ensure() calls
        return PsoState{x.p, v.p, pbest_x.p, pbest_cost.p, sum.p, n_r.p, best.p, rec_x.p, rec_cost.p, rec_sum.p, rec_nr.p, rec_best.p, result.p};
    }
    std::vector<PsoHyp> h_hyp;            // live until the call's synchronisation
    std::vector<PsoResultDev> h_res;
    int last_H = 0, last_P = 0, last_G = -1;
};

extern "C" void lm_pso_options_init(lm_pso_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->size = (uint32_t)sizeof(*o);
    o->particles = 64; o->generations = 30; o->tau = 20; o->cover_pixels = 0; o->seed = 0;
    o->trans_range_mm = 20.0; o->rot_range = tan(10.0 * M_PI / 180.0 / 2.0);
    o->inertia = 0.7298; o->c1 = 1.49618; o->c2 = 1.49618;
    o->clip_near = 10.0; o->clip_far = 10000.0;
}

extern "C" int lm_pso_create(int device, lm_pso** out) {
    if (!out) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = lm_open_device(device)) return rc;
    lm_pso* c = new lm_pso();
    c->device = device;
    if (c->s.ensure(hipStreamNonBlocking) || c->ev0.ensure() || c->ev1.ensure()) {
        lm_pso_destroy(c);
        return lm_set_error(LM_ERR_HIP, "stream / event creation failed");
    }
    *out = c;
    return LM_OK;
}

extern "C" void lm_pso_destroy(lm_pso* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->s) (void)hipStreamSynchronize(c->s);
    delete c;                                                             // every buffer, the events, then the stream: device selected, stream idle
}

extern "C" int lm_pso_set_scene(lm_pso* c, const uint16_t* scene_depth, int width, int height, const double* K) {
    if (!c || !scene_depth || !K) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    for (int k = 0; k < 9; ++k)
        if (!isfinite(K[k])) return lm_set_error(LM_ERR_INVALID, "K is not finite");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->s));
    const size_t n = (size_t)width * height;
    int rc = c->d_scene.ensure(n);
    if (rc) { c->W = c->H = 0; return rc; }
    HIP_TRY(hipMemcpy(c->d_scene.p, scene_depth, n * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->W = width; c->H = height;
    memcpy(c->K, K, sizeof(c->K));
    return LM_OK;
}

extern "C" int lm_pso_set_scene_edges(lm_pso* c, const uint8_t* edges, int width, int height, const double* K, int max_dist) {
    if (!c || !edges || !K) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    if (max_dist < 1 || max_dist > 255) return lm_set_error(LM_ERR_INVALID, "max_dist must be in 1..255 (got %d)", max_dist);
    for (int k = 0; k < 9; ++k)
        if (!isfinite(K[k])) return lm_set_error(LM_ERR_INVALID, "K is not finite");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->s));
    const size_t n = (size_t)width * height;
    c->eW = c->eH = 0;                                                    // until D2 stands
    int rc;
    if ((rc = c->d_edges.ensure(n))) return rc;
    if ((rc = c->d_g.ensure(n))) return rc;
    if ((rc = c->d_d2.ensure(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_edges.p, edges, n, hipMemcpyHostToDevice, c->s));
    HIP_TRY(launch_edt(c->d_edges.p, width, height, max_dist, c->d_g.p, c->d_d2.p, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));                                  // `edges` is the caller's again
    c->eW = width; c->eH = height; c->eM = max_dist;
    memcpy(c->eK, K, sizeof(c->eK));
    return LM_OK;
}

extern "C" int64_t lm_pso_read_edge_distance(lm_pso* c, uint16_t* dst, int64_t capacity) {
    if (!c) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (c->eW <= 0) return lm_set_error(LM_ERR_INVALID, "no scene edges set (lm_pso_set_scene_edges)");
    const int64_t size = (int64_t)c->eW * c->eH;
    if (!dst || capacity <= 0) return size;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(dst, c->d_d2.p, (size_t)std::min<int64_t>(capacity, size) * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return size;
}

// What lm_pso_set_scene_orientations and lm_pso_set_scene_from_detector share: the arguments' checks, and the transforms of the map in d_q.
static int check_orient_args(const double* K, int max_dist, int orient_penalty) {
    if (max_dist < 1 || max_dist > 255) return lm_set_error(LM_ERR_INVALID, "max_dist must be in 1..255 (got %d)", max_dist);
    if (orient_penalty < 0 || orient_penalty > 4096) return lm_set_error(LM_ERR_INVALID, "orient_penalty must be in 0..4096 (got %d)", orient_penalty);
    for (int k = 0; k < 9; ++k)
        if (!isfinite(K[k])) return lm_set_error(LM_ERR_INVALID, "K is not finite");
    return LM_OK;
}
static int ensure_orient(lm_pso* c, size_t n) {
    int rc;
    if ((rc = c->d_q.ensure(n))) return rc;
    if ((rc = c->d_og.ensure(8 * n))) return rc;
    if ((rc = c->d_od2.ensure(8 * n))) return rc;
    return c->d_dd2.ensure(9 * n);
}
static int orient_transforms(lm_pso* c, int width, int height, const double* K, int max_dist, int orient_penalty) {
    HIP_TRY(launch_edt_orient(c->d_q.p, width, height, max_dist, orient_penalty, c->d_og.p, c->d_od2.p, c->d_dd2.p, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    c->oW = width; c->oH = height; c->oM = max_dist; c->oP = orient_penalty;
    memcpy(c->oK, K, sizeof(c->oK));
    return LM_OK;
}

extern "C" int lm_pso_set_scene_orientations(lm_pso* c, const uint8_t* Q, int width, int height, const double* K, int max_dist, int orient_penalty) {
    if (!c || !Q || !K) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    if (int rc = check_orient_args(K, max_dist, orient_penalty)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->s));
    const size_t n = (size_t)width * height;
    c->oW = c->oH = 0;                                                    // until DD2 stands
    if (int rc = ensure_orient(c, n)) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_q.p, Q, n, hipMemcpyHostToDevice, c->s));
    return orient_transforms(c, width, height, K, max_dist, orient_penalty);      // synchronises: `Q` is the caller's again
}

// The device hand-over: the detector's quantised colour map of `level` (lvl[level].ang, what lm_detector_read_stage(level, 0) reads) is
// copied device to device on the context's stream once the detector's streams are idle; no byte of it crosses PCIe.
extern "C" int lm_pso_set_scene_from_detector(lm_pso* c, lm_detector* det, int level, const double* K, int max_dist, int orient_penalty) {
    if (!c || !det || !K) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (int rc = check_orient_args(K, max_dist, orient_penalty)) return rc;
    if (det->device != c->device) return lm_set_error(LM_ERR_INVALID, "the detector lives on device %d, the context on %d", det->device, c->device);
    if (!det->use[0]) return lm_set_error(LM_ERR_INVALID, "the detector's modality set has no ColorGradient: it quantises no orientations");
    if (level < 0 || level >= det->pyramid_levels) return lm_set_error(LM_ERR_INVALID, "level %d out of range (the detector has %d)", level, det->pyramid_levels);
    if (det->n_submitted != det->n_collected) return lm_set_error(LM_ERR_INVALID, "the detector has frames in flight: collect them first");
    if (!det->quantised) return lm_set_error(LM_ERR_INVALID, "no front end has run on the detector: match a frame first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->s));
    HIP_TRY(hipStreamSynchronize(det->stream));                           // the front end that wrote the map, on either stream
    HIP_TRY(hipStreamSynchronize(det->mstream));
    const LevelBufs& b = det->lvl[level];
    if (b.W <= 0 || b.H <= 0 || b.W > 16384 || b.H > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", b.W, b.H);
    const size_t n = (size_t)b.W * b.H;
    c->oW = c->oH = 0;
    if (int rc = ensure_orient(c, n)) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_q.p, b.ang.p, n, hipMemcpyDeviceToDevice, c->s));
    return orient_transforms(c, b.W, b.H, K, max_dist, orient_penalty);
}

extern "C" int64_t lm_pso_read_orient_distance(lm_pso* c, int plane, uint16_t* dst, int64_t capacity) {
    if (!c) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (c->oW <= 0) return lm_set_error(LM_ERR_INVALID, "no scene orientations set (lm_pso_set_scene_orientations)");
    if (plane < 0 || plane > 8) return lm_set_error(LM_ERR_INVALID, "plane must be in 0..8 (got %d)", plane);
    const int64_t size = (int64_t)c->oW * c->oH;
    if (!dst || capacity <= 0) return size;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(dst, c->d_dd2.p + (size_t)plane * size, (size_t)std::min<int64_t>(capacity, size) * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return size;
}

// The body of lm_pso_run, lm_pso_run_edges and lm_pso_run_oriented.  kCostDepth: the depth cost against the scene depth; kCostEdges: the
// edge cost against D2 with edge_step (mm), tau in pixels, the frame and K of the edge scene; kCostOriented: the same against the nine
// planes DD2 of the oriented scene.
enum { kCostDepth = 0, kCostEdges = 1, kCostOriented = 2 };
static int run_swarm(lm_pso* c, lm_mesh* mesh, int count, const double* Rs, const double* ts, const int32_t* windows_xy, int w, int h,
                     const lm_pso_options* options, int mode, int edge_step, lm_pso_result* results, float* device_ms) {
    const bool edges = mode == kCostEdges, oriented = mode == kCostOriented;
    if (!c || !mesh || !Rs || !ts || !windows_xy || !results) return lm_set_error(LM_ERR_INVALID, "null argument");
    lm_pso_options o;
    if (options) {
        if (options->size != sizeof(lm_pso_options))
            return lm_set_error(LM_ERR_INVALID, "lm_pso_options.size is %u, this library expects %u", options->size, (unsigned)sizeof(lm_pso_options));
        o = *options;
    } else lm_pso_options_init(&o);
    if (o.particles < 1 || o.particles > 256) return lm_set_error(LM_ERR_INVALID, "particles must be in 1..256 (got %d)", o.particles);
    if (count < 1 || (long long)count * o.particles > 4096)
        return lm_set_error(LM_ERR_INVALID, "hypotheses x particles must be in 1..4096 (got %d x %d)", count, o.particles);
    if (w < 8 || w > 256 || h < 8 || h > 256) return lm_set_error(LM_ERR_INVALID, "the window must be 8..256 on each side (got %dx%d)", w, h);
    if (o.generations < 0 || o.generations > 256) return lm_set_error(LM_ERR_INVALID, "generations must be in 0..256 (got %d)", o.generations);
    if (o.tau < 1 || o.tau > 65535) return lm_set_error(LM_ERR_INVALID, "tau must be in 1..65535 (got %d)", o.tau);
    if (o.cover_pixels < 0) return lm_set_error(LM_ERR_INVALID, "cover_pixels must be >= 0 (got %d)", o.cover_pixels);
    if (!(isfinite(o.trans_range_mm) && o.trans_range_mm > 0.0)) return lm_set_error(LM_ERR_INVALID, "trans_range_mm must be finite and > 0");
    if (!(isfinite(o.rot_range) && o.rot_range > 0.0)) return lm_set_error(LM_ERR_INVALID, "rot_range must be finite and > 0");
    if (!isfinite(o.inertia) || !isfinite(o.c1) || !isfinite(o.c2)) return lm_set_error(LM_ERR_INVALID, "inertia, c1 and c2 must be finite");
    if (!isfinite(o.clip_near) || !isfinite(o.clip_far)) return lm_set_error(LM_ERR_INVALID, "the clip planes must be finite");
    if (mesh->nf <= 0 || mesh->nv <= 0) return lm_set_error(LM_ERR_INVALID, "the mesh has no faces");
    if (mesh->device != c->device) return lm_set_error(LM_ERR_INVALID, "the mesh lives on device %d, the context on %d", mesh->device, c->device);
    if (mode == kCostDepth && (!c->d_scene.p || c->W <= 0)) return lm_set_error(LM_ERR_INVALID, "no scene depth set (lm_pso_set_scene)");
    if (edges && c->eW <= 0) return lm_set_error(LM_ERR_INVALID, "no scene edges set (lm_pso_set_scene_edges)");
    if (edges && o.tau > c->eM) return lm_set_error(LM_ERR_INVALID, "tau must be <= max_dist for the edge cost (got %d > %d)", o.tau, c->eM);
    if (oriented && c->oW <= 0) return lm_set_error(LM_ERR_INVALID, "no scene orientations set (lm_pso_set_scene_orientations)");
    if (oriented && o.tau > c->oM) return lm_set_error(LM_ERR_INVALID, "tau must be <= max_dist for the oriented cost (got %d > %d)", o.tau, c->oM);
    for (size_t k = 0; k < (size_t)count * 9; ++k)
        if (!isfinite(Rs[k])) return lm_set_error(LM_ERR_INVALID, "a hypothesis' R is not finite");
    for (size_t k = 0; k < (size_t)count * 3; ++k)
        if (!isfinite(ts[k])) return lm_set_error(LM_ERR_INVALID, "a hypothesis' t is not finite");
    for (int i = 0; i < 2 * count; ++i)
        if (windows_xy[i] < -(1 << 20) || windows_xy[i] > (1 << 20)) return lm_set_error(LM_ERR_INVALID, "window origin %d out of range", windows_xy[i]);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->s));                                  // h_hyp / h_res of an earlier call that failed half way

    PsoParams prm{};
    memcpy(prm.K, oriented ? c->oK : edges ? c->eK : c->K, sizeof(prm.K));
    for (int d = 0; d < 3; ++d) { prm.range[d] = o.trans_range_mm; prm.range[3 + d] = o.rot_range; }
    prm.inertia = o.inertia; prm.c1 = o.c1; prm.c2 = o.c2; prm.seed = o.seed;
    prm.G = o.generations;
    prm.P = prm.G == 0 ? 1 : o.particles;                                 // evaluate-only: the given pose alone
    prm.w = w; prm.h = h; prm.W = oriented ? c->oW : edges ? c->eW : c->W; prm.H = oriented ? c->oH : edges ? c->eH : c->H; prm.tau = o.tau; prm.cover_pixels = o.cover_pixels;
    const int H = count, P = prm.P, G = prm.G;
    const size_t HP = (size_t)H * P, npx = (size_t)w * h, gen = (size_t)G + 1;

    int rc;
    if ((rc = c->d_hyp.ensure(H))) return rc;
    if ((rc = c->d_views.ensure(HP))) return rc;
    if ((rc = c->d_pv.ensure(HP * mesh->nv))) return rc;
    if ((rc = c->d_zbuf.ensure(HP * npx))) return rc;
    if ((rc = c->x.ensure(HP * 6))) return rc;
    if ((rc = c->v.ensure(HP * 6))) return rc;
    if ((rc = c->pbest_x.ensure(HP * 6))) return rc;
    if ((rc = c->pbest_cost.ensure(HP))) return rc;
    if ((rc = c->sum.ensure(HP))) return rc;
    if ((rc = c->n_r.ensure(HP))) return rc;
    if ((rc = c->best.ensure(H))) return rc;
    if ((rc = c->rec_x.ensure(gen * HP * 6))) return rc;
    if ((rc = c->rec_cost.ensure(gen * HP))) return rc;
    if ((rc = c->rec_sum.ensure(gen * HP))) return rc;
    if ((rc = c->rec_nr.ensure(gen * HP))) return rc;
    if ((rc = c->rec_best.ensure(gen * H * 2))) return rc;
    if ((rc = c->result.ensure(H))) return rc;
    const PsoState st = c->state();
    c->last_G = -1;

    c->h_hyp.resize(H);
    c->h_res.resize(H);
    for (int i = 0; i < H; ++i) {
        memcpy(c->h_hyp[i].R0, Rs + 9 * (size_t)i, 9 * sizeof(double));
        memcpy(c->h_hyp[i].t0, ts + 3 * (size_t)i, 3 * sizeof(double));
        c->h_hyp[i].x0 = windows_xy[2 * i]; c->h_hyp[i].y0 = windows_xy[2 * i + 1];
    }
    MeshDev M{mesh->d_v.p, mesh->d_n.p, mesh->d_c.p, mesh->d_f.p, mesh->nv, mesh->nf};
    HIP_TRY(hipEventRecord(c->ev0, c->s));
    HIP_TRY(hipMemcpyAsync(c->d_hyp.p, c->h_hyp.data(), H * sizeof(PsoHyp), hipMemcpyHostToDevice, c->s));
    HIP_TRY(launch_pso_init(prm, H, st, c->s));
    for (int g = 0; g <= G; ++g) {
        HIP_TRY(launch_pso_views(prm, H, c->d_hyp.p, st.x, c->d_views.p, c->s));
        HIP_TRY(launch_project(M, c->d_views.p, (int)HP, 1, c->d_pv.p, c->s));
        HIP_TRY(launch_raster(M, c->d_pv.p, (int)HP, w, h, o.clip_near, o.clip_far, c->d_zbuf.p, c->s));
        if (oriented) HIP_TRY(launch_pso_orient_cost(prm, H, edge_step, c->d_hyp.p, c->d_zbuf.p, c->d_dd2.p, st.sum, st.n_r, c->s));
        else if (edges) HIP_TRY(launch_pso_edge_cost(prm, H, edge_step, c->d_hyp.p, c->d_zbuf.p, c->d_d2.p, st.sum, st.n_r, c->s));
        else HIP_TRY(launch_pso_cost(prm, H, c->d_hyp.p, c->d_zbuf.p, c->d_scene.p, st.sum, st.n_r, c->s));
        HIP_TRY(launch_pso_step(prm, H, g, c->d_hyp.p, st, c->s));
    }
    HIP_TRY(hipMemcpyAsync(c->h_res.data(), st.result, H * sizeof(PsoResultDev), hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipEventRecord(c->ev1, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    if (device_ms) HIP_TRY(hipEventElapsedTime(device_ms, c->ev0, c->ev1));
    for (int i = 0; i < H; ++i) {
        const PsoResultDev& r = c->h_res[i];
        memcpy(results[i].R, r.R, sizeof(r.R));
        memcpy(results[i].t, r.t, sizeof(r.t));
        results[i].cost = r.cost; results[i].initial_cost = r.initial_cost;
        results[i].n_rendered = r.n_rendered; results[i].n_initial = r.n_initial;
        results[i].best_particle = r.best_particle; results[i].best_generation = r.best_generation;
    }
    c->last_H = H; c->last_P = P; c->last_G = G;
    return LM_OK;
}

extern "C" int lm_pso_run(lm_pso* c, lm_mesh* mesh, int count, const double* Rs, const double* ts, const int32_t* windows_xy, int w, int h,
                          const lm_pso_options* options, lm_pso_result* results, float* device_ms) {
    return run_swarm(c, mesh, count, Rs, ts, windows_xy, w, h, options, kCostDepth, 0, results, device_ms);
}

extern "C" int lm_pso_run_edges(lm_pso* c, lm_mesh* mesh, int count, const double* Rs, const double* ts, const int32_t* windows_xy, int w, int h,
                                const lm_pso_options* options, int edge_step_mm, lm_pso_result* results, float* device_ms) {
    if (edge_step_mm < 0 || edge_step_mm > 65535) return lm_set_error(LM_ERR_INVALID, "edge_step_mm must be in 0..65535 (got %d)", edge_step_mm);
    return run_swarm(c, mesh, count, Rs, ts, windows_xy, w, h, options, kCostEdges, edge_step_mm, results, device_ms);
}

extern "C" int lm_pso_run_oriented(lm_pso* c, lm_mesh* mesh, int count, const double* Rs, const double* ts, const int32_t* windows_xy, int w, int h,
                                   const lm_pso_options* options, int edge_step_mm, lm_pso_result* results, float* device_ms) {
    if (edge_step_mm < 0 || edge_step_mm > 65535) return lm_set_error(LM_ERR_INVALID, "edge_step_mm must be in 0..65535 (got %d)", edge_step_mm);
    return run_swarm(c, mesh, count, Rs, ts, windows_xy, w, h, options, kCostOriented, edge_step_mm, results, device_ms);
}

extern "C" int64_t lm_pso_read_debug(lm_pso* c, int hypothesis, int kind, double* dst, int64_t capacity) {
    if (!c) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (c->last_G < 0) return lm_set_error(LM_ERR_INVALID, "no run to read back");
    if (hypothesis < 0 || hypothesis >= c->last_H) return lm_set_error(LM_ERR_INVALID, "hypothesis %d out of range", hypothesis);
    if (kind < 0 || kind > 3) return lm_set_error(LM_ERR_INVALID, "unknown kind %d", kind);
    const size_t H = c->last_H, P = c->last_P, gen = (size_t)c->last_G + 1, HP = H * P;
    const size_t per = kind == 0 ? P * 6 : kind == 1 ? P : 2 * (kind == 2 ? P : 1);
    const int64_t size = (int64_t)(gen * per);
    if (!dst || capacity <= 0) return size;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<double> out(gen * per);
    const PsoState st = c->state();
    if (kind == 0 || kind == 1) {                                         // doubles, bit for bit
        const double* src = kind == 0 ? st.rec_x : st.rec_cost;
        HIP_TRY(hipMemcpy2D(out.data(), per * sizeof(double), src + (size_t)hypothesis * per, HP * (per / P) * sizeof(double), per * sizeof(double), gen,
                            hipMemcpyDeviceToHost));
    } else if (kind == 2) {
        std::vector<unsigned long long> sum(gen * P);
        std::vector<unsigned int> nr(gen * P);
        HIP_TRY(hipMemcpy2D(sum.data(), P * sizeof(unsigned long long), st.rec_sum + (size_t)hypothesis * P, HP * sizeof(unsigned long long),
                            P * sizeof(unsigned long long), gen, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(nr.data(), P * sizeof(unsigned int), st.rec_nr + (size_t)hypothesis * P, HP * sizeof(unsigned int), P * sizeof(unsigned int), gen,
                            hipMemcpyDeviceToHost));
        for (size_t k = 0; k < gen * P; ++k) { out[2 * k] = (double)sum[k]; out[2 * k + 1] = (double)nr[k]; }
    } else {
        std::vector<int> best(gen * 2);
        HIP_TRY(hipMemcpy2D(best.data(), 2 * sizeof(int), st.rec_best + (size_t)hypothesis * 2, H * 2 * sizeof(int), 2 * sizeof(int), gen, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < gen * 2; ++k) out[k] = (double)best[k];
    }
    memcpy(dst, out.data(), (size_t)std::min<int64_t>(capacity, size) * sizeof(double));
    return size;
}
