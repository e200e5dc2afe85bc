// poseRefine::process (LL.cpp:27-155) behind the C ABI.  The host only validates arguments, stages
// the depth images through pinned memory and composes the final [R|t] from the device result
// (LL.cpp:146-154); everything between — bounding box, dilated mask, back-projection, centroid
// init, both VoxelDownSample calls, EstimateNormals and the whole ICP loop — runs in the icp*.hip units (icp_kernels.h) with
// no host round trip.  An `lm_icp` context owns one HIP stream, the resident depth images and the
// worst-case-sized arenas (W*H points per hypothesis and cloud: 288 GB of HBM make that free).
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/amd_linemod.h"
#include "icp_internal.h"
#include "lm_error.h"

using namespace lm;

namespace {
constexpr double kVoxel = 0.0025;     // LL.cpp:106
constexpr double kMaxDist = 0.01;     // LL.cpp:31
constexpr int kMaxIter = 30;          // open3d ICPConvergenceCriteria defaults (lm_icp_options_init)
constexpr double kRelTol = 1e-6;
constexpr int kKnn = 30;              // open3d KDTreeSearchParamKNN default
constexpr int kEvalChunk = 64;        // evaluations the sliced launches are enqueued for at a time (the defaults need 32: one chunk)

size_t pow2_at_least(size_t n) {
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
}  // namespace

IcpBuffers lm_icp::buffers() const {
    IcpBuffers B{};
    B.models = d_models.p; B.model_bbox = d_model_bbox.p; B.in = ar.in.p; B.st = ar.st.p;
    B.cap = (size_t)W * H; B.cap2 = pow2_at_least(B.cap);
    B.model_pts = ar.model_pts.p; B.scene_pts = ar.scene_pts.p; B.src = ar.src.p; B.tgt = ar.tgt.p; B.tgt_sorted = ar.tgt_sorted.p;
    B.tgt_orig = ar.tgt_orig.p; B.tgt_rec = ar.tgt_rec.p; B.cell_start = ar.cell_start.p; B.cell_start16 = ar.cell_start16.p;
    B.cov = ar.cov.p; B.normals = ar.normals.p; B.work = ar.work.p; B.prev_nn = ar.prev_nn.p; B.nn_lb = ar.nn_lb.p;
    B.strip_cnt = ar.strip_cnt.p; B.strip_sum = ar.strip_sum.p; B.strip_pub = ar.strip_pub.p; B.strip_mm = ar.strip_mm.p;
    B.sort_look = ar.sort_look.p; B.partial = ar.partial.p; B.keys = ar.keys.p; B.xchg = ar.xchg.p;
    return B;
}

int lm_icp_ensure_arenas(lm_icp* c, int count) {
    if (count <= c->max_count) return LM_OK;
    HIP_TRY(hipStreamSynchronize(c->s));
    c->ar = lm_icp::Arenas{};                                        // all of them go before the first grows; a failure below leaves max_count 0
    c->max_count = 0;
    const size_t n = (size_t)std::max(count, 16), cap = (size_t)c->W * c->H, pts = n * cap * 3;
    lm_icp::Arenas& a = c->ar;
    int rc;
    for (DevBuf<double>* b : {&a.model_pts, &a.scene_pts, &a.src, &a.tgt, &a.tgt_sorted, &a.normals, &a.work})
        if ((rc = b->ensure(pts))) return rc;
    if ((rc = a.cov.ensure(n * cap * kIcpCovStride)) || (rc = a.tgt_orig.ensure(n * cap)) || (rc = a.prev_nn.ensure(n * cap)) ||
        (rc = a.nn_lb.ensure(n * cap)) || (rc = a.partial.ensure(2 * n * kIcpMaxSplit * 32)) || (rc = a.strip_cnt.ensure(n * kIcpStrips * 2)) ||
        (rc = a.strip_sum.ensure(n * kIcpStrips * 8)) || (rc = a.strip_pub.ensure(n * kIcpStrips)) || (rc = a.strip_mm.ensure(n * kIcpStrips * 12)) ||
        (rc = a.sort_look.ensure(n * 2 * kIcpSortGroups)) || (rc = a.tgt_rec.ensure(n * cap)) || (rc = a.cell_start16.ensure(n * kIcpCells16)) ||
        (rc = a.cell_start.ensure(n * kIcpCells)) || (rc = a.keys.ensure(n * 2 * pow2_at_least(cap))) || (rc = a.xchg.ensure(2 * n * kIcpMaxSplit * 64)))
        return rc;
    HIP_TRY(hipMemset(a.strip_pub.p, 0, a.strip_pub.cap * sizeof(unsigned long long)));   // (0 = not counted yet; every run leaves them cleared for the next)
    HIP_TRY(hipMemset(a.xchg.p, 0, a.xchg.cap * sizeof(unsigned long long)));             // tag 0 = never published (runs count from 1)
    HIP_TRY(hipDeviceSynchronize());                                 // (the ICP stream does not wait for the null stream)
    if ((rc = a.in.ensure(n)) || (rc = a.st.ensure(n)) || (rc = a.h_in.ensure(n)) || (rc = a.h_st.ensure(n)) || (rc = a.h_st2.ensure(n))) return rc;
    c->max_count = (int)n;
    return LM_OK;
}

int lm_icp_set_geometry(lm_icp* c, int W, int H) {
    if (W == c->W && H == c->H) return LM_OK;
    HIP_TRY(hipStreamSynchronize(c->s));
    c->ar = lm_icp::Arenas{};
    c->max_count = 0;
    c->d_scene.release(); c->d_models.release(); c->d_model_bbox.release();
    c->slots = 0; c->have_scene = false;
    c->slot_boxed.clear();
    c->W = W; c->H = H;
    return c->d_scene.ensure((size_t)W * H);
}

// Grows the slot arrays and keeps what they hold (DevBuf::ensure would not): into buffers of its own, which a failing step frees.
int lm_icp_ensure_slots(lm_icp* c, int slots) {
    if (slots <= c->slots) return LM_OK;
    const size_t px = (size_t)c->W * c->H;
    const int n = std::max(slots, std::max(16, c->slots * 2));
    DevBuf<uint16_t> models;
    DevBuf<int> boxes;
    int rc;
    if ((rc = models.ensure((size_t)n * px))) return rc;
    if (c->d_models.p) {
        HIP_TRY(hipMemcpyAsync(models.p, c->d_models.p, (size_t)c->slots * px * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->s));
        HIP_TRY(hipStreamSynchronize(c->s));
    }
    c->d_models = std::move(models);
    if ((rc = boxes.ensure((size_t)n * 8))) return rc;
    HIP_TRY(hipMemset(boxes.p, 0, (size_t)n * 8 * sizeof(int)));
    if (c->d_model_bbox.p) HIP_TRY(hipMemcpy(boxes.p, c->d_model_bbox.p, (size_t)c->slots * 8 * sizeof(int), hipMemcpyDeviceToDevice));
    HIP_TRY(hipDeviceSynchronize());
    c->d_model_bbox = std::move(boxes);
    c->slot_boxed.resize((size_t)n, 0);
    c->slots = n;
    return LM_OK;
}


void lm_icp_compose_result(const IcpState& st, const float* model_R, const float* model_t, lm_pose_result* op) {
    lm_pose_result& o = *op;
    // init_base (float): [R|t], only t.z / 1000 (LL.cpp:34-39)
    float base[16];
    for (int k = 0; k < 16; ++k) base[k] = 0.f;
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) base[4 * r + q] = model_R[3 * r + q];
        base[4 * r + 3] = model_t[r];
    }
    base[11] = base[11] / 1000.0f;
    base[15] = 1.f;
    // result = transformation_ * init_base.cast<double>() (LL.cpp:146); t * 1000 (LL.cpp:154)
    double M[16];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            double v = 0;
            for (int k = 0; k < 4; ++k) v += st.T[4 * a + k] * (double)base[4 * k + b];
            M[4 * a + b] = v;
        }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) o.R[3 * a + b] = M[4 * a + b];
        o.t[a] = M[4 * a + 3] * 1000.0;
    }
    o.residual = (float)st.fitness;       // residual = fitness_ (LL.cpp:148)
    o.inlier_rmse = (float)st.rmse;
    o.iterations = st.iterations;
    o.n_source = st.n_src;
    o.n_target = st.n_tgt;
}

namespace {
// k_icp_team is point-to-plane and is handed the default criteria only (it takes one tolerance for both tests, and its cut after
// evaluation 3 and its resume path are exercised at max_iteration 30 alone): every other hypothesis goes straight to the sliced launches
bool sliced_first(const lm_icp* c) {
    return c->sliced_only || c->run_p2p || c->opt.max_iteration != kMaxIter || c->opt.relative_fitness != kRelTol || c->opt.relative_rmse != kRelTol;
}

// the next evaluations of the sliced launches, at most kEvalChunk of them, up to the prologue that finishes evaluation max_iteration
int enqueue_evals(lm_icp* c, const IcpBuffers& B, hipStream_t s) {
    const int last = c->opt.max_iteration + 1;
    const int to = last - c->next_it < kEvalChunk ? last : c->next_it + kEvalChunk - 1;
    HIP_TRY(launch_icp_evals(B, B.count, c->next_it, to, c->run_p2p, kMaxDist, c->opt.max_iteration, c->opt.relative_fitness, c->opt.relative_rmse, s));
    c->next_it = to + 1;
    return LM_OK;
}
}  // namespace

int lm_icp_enqueue(lm_icp* c, const IcpBuffers& B, int flags, IcpState* h_st, hipStream_t s) {
    c->run_p2p = (flags & LM_ICP_POINT_TO_POINT) != 0;
    c->next_it = 0;
    HIP_TRY(launch_icp_prepare(B, B.count, c->W, c->H, flags, kVoxel, kKnn, s));
    if (sliced_first(c)) { if (int rc = enqueue_evals(c, B, s)) return rc; }
    else HIP_TRY(launch_icp_team(B, B.count, kIcpStageTeam, c->cus, kMaxDist, kMaxIter, kRelTol, s));
    HIP_TRY(hipEventRecord(c->e1, s));
    HIP_TRY(hipMemcpyAsync(h_st, B.st, (size_t)B.count * sizeof(IcpState), hipMemcpyDeviceToHost, s));
    return LM_OK;
}

int lm_icp_finish(lm_icp* c, const IcpBuffers& B, IcpState* h_st, hipStream_t s) {
    c->stage.assign((size_t)B.count, kIcpStageNone);
    for (int stage = sliced_first(c) ? kIcpStageSliced : kIcpStageTeam;;) {
        bool unfinished = false;                                     // (status 0, stop 0)
        for (int i = 0; i < B.count; ++i) {
            if (h_st[i].status != 0) continue;
            if (h_st[i].stop == 0) unfinished = true;
            else if (c->stage[i] == kIcpStageNone) c->stage[i] = stage;
        }
        if (!unfinished) return LM_OK;
        // clouds the first team builds do not hold (more than 704 source points per workgroup): the builds with more points per thread;
        // what those leave too, or a team that timed out: the sliced launches
        // (more than kEvalChunk evaluations asked for: the next chunk)
        if (stage == kIcpStageSliced && c->next_it > c->opt.max_iteration + 1) return lm_set_error(LM_ERR_HIP, "ICP: a hypothesis was left unfinished");
        if (stage == kIcpStageTeam) {
            HIP_TRY(launch_icp_team(B, B.count, kIcpStageLarge, c->cus, kMaxDist, kMaxIter, kRelTol, s));
            stage = kIcpStageLarge;
        } else {
            stage = kIcpStageSliced;
            if (int rc = enqueue_evals(c, B, s)) return rc;
        }
        HIP_TRY(hipEventRecord(c->e1, s));
        HIP_TRY(hipMemcpyAsync(h_st, B.st, (size_t)B.count * sizeof(IcpState), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
}

extern "C" int lm_icp_create(int device, lm_icp** out) {
    if (!out) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = lm_open_device(device)) return rc;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    lm_icp* c = new lm_icp();
    c->device = device;
    c->cus = cus;
    if (const char* e = getenv("LM_ICP_SLICED")) c->sliced_only = e[0] && e[0] != '0';
    if (c->s.ensure(hipStreamNonBlocking) || c->e0.ensure() || c->e1.ensure()) {
        delete c;                                                         // (releases what was created)
        return lm_set_error(LM_ERR_HIP, "could not create the ICP stream / events");
    }
    *out = c;
    return LM_OK;
}

extern "C" void lm_icp_options_init(lm_icp_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->max_iteration = kMaxIter;
    o->relative_fitness = kRelTol;
    o->relative_rmse = kRelTol;
}

extern "C" int lm_icp_set_options(lm_icp* c, const lm_icp_options* options) {
    if (!c) return lm_set_error(LM_ERR_INVALID, "null argument");
    lm_icp_options o;
    lm_icp_options_init(&o);
    if (options) o = *options;
    if (o.max_iteration < 0) return lm_set_error(LM_ERR_INVALID, "max_iteration %d is negative", o.max_iteration);
    if (o.max_iteration > INT_MAX - 2) return lm_set_error(LM_ERR_INVALID, "max_iteration %d is too large", o.max_iteration);
    if (!(o.relative_fitness > 0.0) || !isfinite(o.relative_fitness))
        return lm_set_error(LM_ERR_INVALID, "relative_fitness %g is not a positive finite number", o.relative_fitness);
    if (!(o.relative_rmse > 0.0) || !isfinite(o.relative_rmse))
        return lm_set_error(LM_ERR_INVALID, "relative_rmse %g is not a positive finite number", o.relative_rmse);
    o.reserved = 0;
    c->opt = o;
    return LM_OK;
}

extern "C" void lm_icp_destroy(lm_icp* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->s) (void)hipStreamSynchronize(c->s);
    delete c;                                                         // every buffer, the events, then the stream: device selected, stream idle
}

extern "C" int lm_icp_set_scene(lm_icp* c, const uint16_t* scene_depth, int width, int height, const float* scene_K) {
    if (!c || !scene_depth || !scene_K || width <= 0 || height <= 0) return lm_set_error(LM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = lm_icp_set_geometry(c, width, height);
    if (rc) return rc;
    const size_t img = (size_t)width * height * sizeof(uint16_t);
    HIP_TRY(hipStreamSynchronize(c->s));                            // the staging buffer may still be in flight
    if ((rc = c->pinned.ensure(img))) return rc;
    memcpy(c->pinned.p, scene_depth, img);
    HIP_TRY(hipMemcpyAsync(c->d_scene.p, c->pinned.p, img, hipMemcpyHostToDevice, c->s));
    memcpy(c->sK, scene_K, sizeof(c->sK));
    c->have_scene = true;
    return LM_OK;
}

extern "C" int lm_icp_set_models(lm_icp* c, int first_slot, int count, const uint16_t* const* model_depths) {
    if (!c || first_slot < 0 || count < 0 || (count && !model_depths)) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (c->W <= 0) return lm_set_error(LM_ERR_INVALID, "lm_icp_set_scene must define the frame geometry first");
    if (count == 0) return LM_OK;
    for (int i = 0; i < count; ++i)
        if (!model_depths[i]) return lm_set_error(LM_ERR_INVALID, "model depth %d is null", i);
    HIP_TRY(hipSetDevice(c->device));
    int rc = lm_icp_ensure_slots(c, first_slot + count);
    if (rc) return rc;
    const size_t img = (size_t)c->W * c->H * sizeof(uint16_t);
    HIP_TRY(hipStreamSynchronize(c->s));
    // the scene image may sit at the start of the staging buffer and still be copying: keep it, append after it
    if ((rc = c->pinned.ensure(img * (size_t)(count + 1)))) return rc;
    uint8_t* stage = c->pinned.p + img;
    for (int i = 0; i < count; ++i) memcpy(stage + (size_t)i * img, model_depths[i], img);
    HIP_TRY(hipMemcpyAsync(c->d_models.p + (size_t)first_slot * c->W * c->H, stage, img * (size_t)count, hipMemcpyHostToDevice, c->s));
    HIP_TRY(lm::launch_icp_model_boxes(c->d_models.p, c->d_model_bbox.p, first_slot, count, c->W, c->H, c->s));   // the boxes of the new images, once (LL.cpp:43-50)
    for (int i = 0; i < count; ++i) c->slot_boxed[(size_t)first_slot + i] = 1;
    return LM_OK;
}

extern "C" int lm_icp_run(lm_icp* c, int count, const int32_t* model_slots, const float* model_Ks, const float* model_Rs,
                          const float* model_ts, const int32_t* detect_xy, int flags, lm_pose_result* results, float* device_ms) {
    if (!c || count < 0 || (count && (!model_Ks || !model_Rs || !model_ts || !detect_xy || !results)))
        return lm_set_error(LM_ERR_INVALID, "null argument");
    if (device_ms) *device_ms = 0.f;
    if (count == 0) return LM_OK;
    if (!c->have_scene) return lm_set_error(LM_ERR_INVALID, "no scene depth resident (lm_icp_set_scene)");
    for (int i = 0; i < count; ++i) {
        const int slot = model_slots ? model_slots[i] : i;
        if (slot < 0 || slot >= c->slots) return lm_set_error(LM_ERR_INVALID, "model slot %d of hypothesis %d is not resident", slot, i);
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc = lm_icp_ensure_arenas(c, count);
    if (rc) return rc;
    for (int i = 0; i < count; ++i) {
        IcpIn& in = c->ar.h_in.p[i];
        memcpy(in.mK, model_Ks + 9 * i, sizeof(in.mK));
        in.dx = detect_xy[2 * i]; in.dy = detect_xy[2 * i + 1];
        in.model_slot = model_slots ? model_slots[i] : i;
        in.pad = 0;
        IcpState& st = c->ar.h_st.p[i];
        memset(&st, 0, sizeof(st));
        st.bbox[0] = INT_MAX; st.bbox[1] = INT_MAX; st.bbox[2] = -1; st.bbox[3] = -1;
    }
    IcpBuffers B = c->buffers();
    B.scene = c->d_scene.p;
    B.count = count;
    memcpy(B.sK, c->sK, sizeof(B.sK));
    HIP_TRY(hipMemcpyAsync(c->ar.in.p, c->ar.h_in.p, (size_t)count * sizeof(IcpIn), hipMemcpyHostToDevice, c->s));
    HIP_TRY(hipMemcpyAsync(c->ar.st.p, c->ar.h_st.p, (size_t)count * sizeof(IcpState), hipMemcpyHostToDevice, c->s));
    HIP_TRY(hipEventRecord(c->e0, c->s));
    bool boxed = true;                                               // every slot's box was worked out when its image was uploaded: no k_icp_bbox
    for (int i = 0; i < count; ++i) boxed = boxed && c->slot_boxed[(size_t)(model_slots ? model_slots[i] : i)] != 0;
    if ((rc = lm_icp_enqueue(c, B, (flags & 0xFF) | (boxed ? 0x100 : 0), c->ar.h_st2.p, c->s))) return rc;
    HIP_TRY(hipStreamSynchronize(c->s));
    if ((rc = lm_icp_finish(c, B, c->ar.h_st2.p, c->s))) return rc;
    memcpy(c->ar.h_st.p, c->ar.h_st2.p, (size_t)count * sizeof(IcpState));
    c->last_count = count; c->last_flags = flags;
    if (device_ms) (void)hipEventElapsedTime(device_ms, c->e0, c->e1);
    for (int i = 0; i < count; ++i) {
        const IcpState& st = c->ar.h_st.p[i];
        if (st.status == 2) return lm_set_error(LM_ERR_INVALID, "model depth image is empty");
        if (st.status == lm::kIcpStalled) return lm_set_error(LM_ERR_HIP, "hypothesis %d: the point kernels stalled (strips waited a second for each other)", i);
        if (st.status == 3)
            return lm_set_error(LM_ERR_INVALID, "hypothesis %d: point cloud too large for 64-bit voxel keys (depth spans tens of metres?)", i);
    }
    for (int i = 0; i < count; ++i) {
        const IcpState& st = c->ar.h_st.p[i];
        lm_pose_result& o = results[i];
        memset(&o, 0, sizeof(o));
        if (st.status == 1) { o.residual = -1.f; continue; }        // LL.cpp:52-55
        lm_icp_compose_result(st, model_Rs + 9 * i, model_ts + 3 * i, &o);
        o.stage = c->stage[(size_t)i];
    }
    return LM_OK;
}

extern "C" int64_t lm_icp_read_debug(lm_icp* c, int hypothesis, int kind, double* dst, int64_t capacity) {
    if (!c || hypothesis < 0 || hypothesis >= c->last_count) return lm_set_error(LM_ERR_INVALID, "no such hypothesis in the last run");
    if (hipSetDevice(c->device) != hipSuccess) return lm_set_error(LM_ERR_HIP, "hipSetDevice failed");
    const IcpState& st = c->ar.h_st.p[hypothesis];
    const size_t off = (size_t)hypothesis * c->W * c->H;
    const bool scene_mode = (c->last_flags & LM_ICP_SCENE_FROM_SCENE) != 0;
    std::vector<double> tmp;
    int64_t n = 0;
    switch (kind) {
        case 0: {   // source cloud
            n = (int64_t)st.n_src * 3; tmp.resize((size_t)n);
            if (n && hipMemcpy(tmp.data(), c->ar.src.p + off * 3, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return lm_set_error(LM_ERR_HIP, "read-back failed");
            break;
        }
        case 1: {   // target cloud, original (voxel) order
            n = (int64_t)st.n_tgt * 3; tmp.resize((size_t)n);
            if (n && hipMemcpy(tmp.data(), (scene_mode ? c->ar.tgt.p : c->ar.src.p) + off * 3, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return lm_set_error(LM_ERR_HIP, "read-back failed");
            break;
        }
        case 2: {   // target normals, original order
            n = (int64_t)st.n_tgt * 3; tmp.resize((size_t)n);
            std::vector<double> sorted((size_t)n);
            std::vector<int> orig((size_t)st.n_tgt);
            if (n && (hipMemcpy(sorted.data(), c->ar.normals.p + off * 3, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(orig.data(), c->ar.tgt_orig.p + off, (size_t)st.n_tgt * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
                return lm_set_error(LM_ERR_HIP, "read-back failed");
            for (int p = 0; p < st.n_tgt; ++p)
                for (int k = 0; k < 3; ++k) tmp[(size_t)orig[p] * 3 + k] = sorted[(size_t)p * 3 + k];
            break;
        }
        case 3: {   // init_guess translation, final T (16), counters
            tmp = {st.init[0], st.init[1], st.init[2]};
            for (int k = 0; k < 16; ++k) tmp.push_back(st.T[k]);
            tmp.push_back((double)st.n_model); tmp.push_back((double)st.n_scene);
            tmp.push_back((double)st.gx); tmp.push_back((double)st.gy); tmp.push_back(st.cell);
            tmp.push_back((double)st.iterations);
            for (int k = 0; k < 8; ++k) tmp.push_back((double)st.clk[k]);
            for (int k = 0; k < 4; ++k) tmp.push_back((double)st.team_note[k]);
            tmp.push_back((double)st.n_src); tmp.push_back((double)st.n_tgt);
            for (int k = 0; k < 4; ++k) tmp.push_back((double)st.knn_clk[k]);
            for (int k = 0; k < 4; ++k) tmp.push_back((double)st.vox_clk[k]);
            tmp.push_back((double)st.n_model); tmp.push_back((double)st.n_scene);
            for (int k = 0; k < 16; ++k) tmp.push_back((double)st.sort_clk[k]);
            tmp.push_back((double)st.team_size); tmp.push_back((double)st.resume_it); tmp.push_back((double)st.build);
            // which kernels prepared the clouds: groups of the wide sorts that finished (kIcpSortGroups = the one-workgroup kernel had nothing
            // to do), points k_icp_knn handed to k_icp_knn_far and points that list had no room for (none: it holds every target)
            tmp.push_back((double)st.vox_done[0]); tmp.push_back((double)st.vox_done[1]); tmp.push_back((double)st.grid_done);
            tmp.push_back((double)std::min(st.n_far, st.n_tgt)); tmp.push_back((double)std::max(st.n_far - st.n_tgt, 0));
            n = (int64_t)tmp.size();
            break;
        }
        case 5: {   // cumulants of the k nearest neighbours per sorted target position [n_tgt][kIcpCovStride]
            n = (int64_t)st.n_tgt * kIcpCovStride; tmp.resize((size_t)n);
            if (n && hipMemcpy(tmp.data(), c->ar.cov.p + off * kIcpCovStride, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return lm_set_error(LM_ERR_HIP, "read-back failed");
            break;
        }
        case 6: {   // original (voxel-order) index of the target point at every sorted position [n_tgt]: the row order of kind 5
            n = (int64_t)st.n_tgt; tmp.resize((size_t)n);
            std::vector<int> orig((size_t)n);
            if (n && hipMemcpy(orig.data(), c->ar.tgt_orig.p + off, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
                return lm_set_error(LM_ERR_HIP, "read-back failed");
            for (int64_t p = 0; p < n; ++p) tmp[(size_t)p] = (double)orig[(size_t)p];
            break;
        }
        case 4: {   // the slices' partial sums of the last two evaluations, [2][kIcpMaxSplit][32] (slots 29..31: shader cycles of the slice)
            n = 2 * kIcpMaxSplit * 32; tmp.resize((size_t)n);
            for (int par = 0; par < 2; ++par)
                if (hipMemcpy(tmp.data() + (size_t)par * kIcpMaxSplit * 32, c->ar.partial.p + (((size_t)par * c->last_count + hypothesis) * kIcpMaxSplit) * 32,
                              (size_t)kIcpMaxSplit * 32 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                    return lm_set_error(LM_ERR_HIP, "read-back failed");
            break;
        }
        default: return lm_set_error(LM_ERR_INVALID, "unknown debug kind %d", kind);
    }
    if (dst && capacity > 0) memcpy(dst, tmp.data(), (size_t)std::min<int64_t>(n, capacity) * sizeof(double));
    return n;
}

// ---- the reference-shaped entry points: one shared context per device -----------------------------
namespace {
std::mutex g_mu;
std::vector<lm_icp*> g_ctx;

int shared_context(int device, lm_icp** out) {
    if (device < 0) return lm_set_error(LM_ERR_INVALID, "device %d out of range", device);
    if ((size_t)device >= g_ctx.size()) g_ctx.resize((size_t)device + 1, nullptr);
    if (!g_ctx[device]) {
        int rc = lm_icp_create(device, &g_ctx[device]);
        if (rc) return rc;
    }
    *out = g_ctx[device];
    return LM_OK;
}
}  // namespace

extern "C" int lm_pose_refine_batch(int device, const uint16_t* scene_depth, int width, int height, const float* scene_K,
                                    int count, const uint16_t* const* model_depths, const float* model_Ks, const float* model_Rs,
                                    const float* model_ts, const int32_t* detect_xy, int flags, lm_pose_result* results,
                                    float* device_ms) {
    if (!scene_depth || !scene_K || count < 0 || (count && (!model_depths || !model_Ks || !model_Rs || !model_ts || !detect_xy || !results)))
        return lm_set_error(LM_ERR_INVALID, "null argument");
    if (device_ms) *device_ms = 0.f;
    if (count == 0) return LM_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    lm_icp* c = nullptr;
    int rc = shared_context(device, &c);
    if (rc) return rc;
    if ((rc = lm_icp_set_scene(c, scene_depth, width, height, scene_K))) return rc;
    if ((rc = lm_icp_set_models(c, 0, count, model_depths))) return rc;
    return lm_icp_run(c, count, nullptr, model_Ks, model_Rs, model_ts, detect_xy, flags, results, device_ms);
}

extern "C" int lm_pose_refine(int device, const uint16_t* scene_depth, const uint16_t* model_depth, int width, int height,
                              const float* scene_K, const float* model_K, const float* model_R, const float* model_t, int detect_x,
                              int detect_y, int flags, lm_pose_result* result) {
    const uint16_t* models[1] = {model_depth};
    int32_t xy[2] = {detect_x, detect_y};
    return lm_pose_refine_batch(device, scene_depth, width, height, scene_K, 1, models, model_K, model_R, model_t, xy, flags, result,
                                nullptr);
}
