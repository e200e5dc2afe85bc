// lm_pipeline — the per-frame loop of the reference driver (linemod_and_levelup_test.py:324-372) as ONE
// stream of device work: Detector::match (front end, coarse, refinement) -> boxes of the matched
// templates -> greedy NMS -> the first top_k kept detections -> poseRefine on each, with the rendered
// depth of every template view resident in HBM.  The host enqueues everything, waits once, and composes
// [R|t] = T_icp * [R_view | t_view] (LL.cpp:146-154).  SURVEY §8f N1.
//
// Equals, on the same frame: lm_detector_match -> lm_nms_boxes on (x, y, x+width, y+height, similarity)
// -> lm_pose_refine_batch on the first top_k kept matches (tests/test_gpu_parity.py checks exactly that).
#include <string.h>

#include <algorithm>
#include <map>

#include "detector_internal.h"
#include "icp_internal.h"
#include "render_internal.h"

struct lm_pipeline {
    lm_detector* det = nullptr;
    lm_icp* icp = nullptr;
    int W = 0, H = 0;                             // the aligned geometry: the detector's frame buffers, the ICP context, the model slots
    int srcW = 0, srcH = 0;                       // what the caller named: the size of the frames and depth renderings it hands over (== W x H unless the detector pads or crops)
    DevBuf<uint8_t> border_src;                   // depth renderings of the source size on their way into the model slots (k_frame_border)
    struct ClassViews { int base = 0, count = 0; };
    std::map<std::string, ClassViews> views;      // class id -> range of view slots
    int num_views = 0;                            // slots handed out
    std::vector<float> view_K, view_R, view_t;    // per slot: 9, 9, 3
    std::vector<int32_t> view_valid;
    std::vector<int32_t> view_wh;                 // per slot: NMS box width, height (-1: the template's size)
    bool views_dirty = true;
    DevBuf<float> d_view_K;                       // the view tables on the device: replaced and uploaded together (ensure_run_buffers)
    DevBuf<int32_t> d_view_valid, d_view_wh;
    DevBuf<int32_t> d_class_base;
    DevBuf<TopkSel> d_sel;
    DevBuf<int32_t> d_nsel;                       // kept, refused, distinct records, (pad)
    DevBuf<uint8_t> d_scratch;                    // of launch_topk_nms
    PinBuf<TopkSel> h_sel;
    PinBuf<int32_t> h_nsel, h_class_base;
    std::vector<int32_t> class_base_on_device;    // what d_class_base holds (re-uploaded only when it changes)
    DevEvent e0, e1, e2;                          // (no stream of its own: the pipeline runs on the detector's and the ICP context's, which both outlive it)
};

extern "C" int lm_pipeline_create(lm_detector* det, int width, int height, lm_pipeline** out) {
    if (!det || !out || width <= 0 || height <= 0) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = lm_need_both(det, "lm_pipeline_create")) return rc;   // the ICP stage reads the scene depth of the detector's frame
    if (int rc = lm_parts_refused(det, "lm_pipeline_create")) return rc; // (a part-mode record's similarity may lie below the threshold: the NMS chain has not been held to that)
    HIP_TRY(hipSetDevice(det->device));
    lm_pipeline* p = new lm_pipeline();
    p->det = det; p->srcW = width; p->srcH = height;
    int rc = border_resolve(det, width, height, &p->W, &p->H);   // under the detector's border policy as it is now
    if (rc) { delete p; return rc; }
    rc = lm_icp_create(det->device, &p->icp);
    if (!rc) rc = lm_icp_set_geometry(p->icp, p->W, p->H);
    if (rc) { if (p->icp) lm_icp_destroy(p->icp); delete p; return rc; }
    if (p->e0.ensure() || p->e1.ensure() || p->e2.ensure()) {
        lm_icp_destroy(p->icp); delete p;
        return lm_set_error(LM_ERR_HIP, "could not create the pipeline events");
    }
    ++det->pipelines;                                            // (depth-scaled matching refuses a detector that serves a pipeline)
    *out = p;
    return LM_OK;
}

extern "C" void lm_pipeline_destroy(lm_pipeline* p) {
    if (!p) return;
    --p->det->pipelines;
    (void)hipSetDevice(p->det->device);
    (void)hipStreamSynchronize(p->det->stream);
    (void)hipStreamSynchronize(p->det->mstream);
    lm_icp* icp = p->icp;
    delete p;                                                     // the events and every buffer: device selected, the detector's streams idle
    lm_icp_destroy(icp);
}

extern "C" int lm_pipeline_set_icp_options(lm_pipeline* p, const lm_icp_options* options) {
    if (!p) return lm_set_error(LM_ERR_INVALID, "null argument");
    return lm_icp_set_options(p->icp, options);
}

// The view slots of a class of nt templates: a new range behind those handed out (tables grown, slots not valid yet), or the one it has.
static int claim_views(lm_pipeline* p, const char* class_id, int nt, int* base) {
    auto it = p->views.find(class_id);
    if (it == p->views.end()) {
        lm_pipeline::ClassViews cv;
        cv.base = p->num_views; cv.count = nt;
        p->num_views += nt;
        p->view_K.resize((size_t)p->num_views * 9, 0.f); p->view_R.resize((size_t)p->num_views * 9, 0.f);
        p->view_t.resize((size_t)p->num_views * 3, 0.f); p->view_valid.resize((size_t)p->num_views, 0);
        p->view_wh.resize((size_t)p->num_views * 2, -1);
        it = p->views.emplace(class_id, cv).first;
    } else if (it->second.count != nt) {
        return lm_set_error(LM_ERR_INVALID, "class '%s' changed its template count after views were set", class_id);
    }
    *base = it->second.base;
    return LM_OK;
}

// K, R, t and the NMS box of `count` slots from slot0 on, now valid; the next run uploads the tables.
static void record_views(lm_pipeline* p, int slot0, int count, const float* Ks, const float* Rs, const float* ts, const int32_t* box_wh) {
    memcpy(&p->view_K[(size_t)slot0 * 9], Ks, (size_t)count * 9 * sizeof(float));
    memcpy(&p->view_R[(size_t)slot0 * 9], Rs, (size_t)count * 9 * sizeof(float));
    memcpy(&p->view_t[(size_t)slot0 * 3], ts, (size_t)count * 3 * sizeof(float));
    for (int i = 0; i < count; ++i) {
        p->view_valid[(size_t)slot0 + i] = 1;
        p->view_wh[2 * ((size_t)slot0 + i)] = box_wh ? box_wh[2 * i] : -1;
        p->view_wh[2 * ((size_t)slot0 + i) + 1] = box_wh ? box_wh[2 * i + 1] : -1;
    }
    p->views_dirty = true;
}

extern "C" int lm_pipeline_set_views(lm_pipeline* p, const char* class_id, int first_template, int count, const uint16_t* const* depth_ren,
                                     const float* Ks, const float* Rs, const float* ts, const int32_t* box_wh) {
    if (!p || !class_id || first_template < 0 || count < 0 || (count && (!depth_ren || !Ks || !Rs || !ts)))
        return lm_set_error(LM_ERR_INVALID, "null argument");
    const int nt = lm_detector_num_templates(p->det, class_id);
    if (nt <= 0) return lm_set_error(LM_ERR_NOT_FOUND, "class '%s' has no templates in the detector", class_id);
    if (first_template + count > nt) return lm_set_error(LM_ERR_INVALID, "views [%d, %d) exceed the %d templates of class '%s'", first_template, first_template + count, nt, class_id);
    int base = 0;
    if (int rc = claim_views(p, class_id, nt, &base)) return rc;
    if (count == 0) return LM_OK;
    HIP_TRY(hipSetDevice(p->det->device));
    HIP_TRY(hipStreamSynchronize(p->det->stream));                 // the slot array may be reallocated: no frame may be in flight
    HIP_TRY(hipStreamSynchronize(p->det->mstream));
    const int slot0 = base + first_template;
    int rc;
    if (p->srcW == p->W && p->srcH == p->H) {
        if ((rc = lm_icp_set_models(p->icp, slot0, count, depth_ren))) return rc;
    } else {
        // depth renderings of the source size: padded with 0 or cropped into the model slots like the scene depth (k_frame_border), eight per launch
        for (int i = 0; i < count; ++i)
            if (!depth_ren[i]) return lm_set_error(LM_ERR_INVALID, "model depth %d is null", i);
        if ((rc = lm_icp_ensure_slots(p->icp, slot0 + count))) return rc;
        const size_t src_img = (size_t)p->srcW * p->srcH * sizeof(uint16_t), npx = (size_t)p->W * p->H;
        const int chunk = 8;
        if ((rc = p->border_src.ensure(src_img * chunk + 16))) return rc;
        for (int c0 = 0; c0 < count; c0 += chunk) {
            const int n = std::min(chunk, count - c0);
            BorderStage bs{};
            for (int i = 0; i < n; ++i) {
                HIP_TRY(hipMemcpyAsync(p->border_src.p + (size_t)i * src_img, depth_ren[c0 + i], src_img, hipMemcpyHostToDevice, p->icp->s));
                border_job(bs.job[bs.njobs++], p->border_src.p + (size_t)i * src_img, p->icp->d_models.p + ((size_t)slot0 + c0 + i) * npx, p->srcW, p->srcH, p->W, p->H, 2, false);
            }
            HIP_TRY(launch_frame_border(bs, p->icp->s));
            HIP_TRY(hipStreamSynchronize(p->icp->s));              // the staging buffer serves the next eight
        }
        HIP_TRY(lm::launch_icp_model_boxes(p->icp->d_models.p, p->icp->d_model_bbox.p, slot0, count, p->W, p->H, p->icp->s));   // the boxes of the new images, once (LL.cpp:43-50)
        for (int i = 0; i < count; ++i) p->icp->slot_boxed[(size_t)slot0 + i] = 1;
    }
    HIP_TRY(hipStreamSynchronize(p->icp->s));
    record_views(p, slot0, count, Ks, Rs, ts, box_wh);
    return LM_OK;
}

// Views rendered on the device: the depth of template first_template + i goes from the rasteriser straight into the
// ICP context's model slot — what the driver does per match at linemod_and_levelup_test.py:352, once per template.
extern "C" int lm_pipeline_set_views_rendered(lm_pipeline* p, lm_mesh* m, const char* class_id, int first_template, int count,
                                              const float* Ks, const float* Rs, const float* ts, float clip_near, float clip_far,
                                              const int32_t* box_wh) {
    if (!p || !m || !class_id || first_template < 0 || count < 0 || (count && (!Ks || !Rs || !ts)))
        return lm_set_error(LM_ERR_INVALID, "null argument");
    if (m->device != p->det->device) return lm_set_error(LM_ERR_INVALID, "mesh and detector live on different devices");
    const int nt = lm_detector_num_templates(p->det, class_id);
    if (nt <= 0) return lm_set_error(LM_ERR_NOT_FOUND, "class '%s' has no templates in the detector", class_id);
    if (first_template + count > nt) return lm_set_error(LM_ERR_INVALID, "views [%d, %d) exceed the %d templates of class '%s'", first_template, first_template + count, nt, class_id);
    int base = 0;
    if (int rc = claim_views(p, class_id, nt, &base)) return rc;
    if (count == 0) return LM_OK;
    HIP_TRY(hipSetDevice(p->det->device));
    HIP_TRY(hipStreamSynchronize(p->det->stream));
    HIP_TRY(hipStreamSynchronize(p->det->mstream));
    const int slot0 = base + first_template;
    int rc = lm_icp_ensure_slots(p->icp, slot0 + count);
    if (rc) return rc;
    const size_t npx = (size_t)p->W * p->H;
    const int chunk = 256;
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int n = std::min(chunk, count - c0);
        if ((rc = lm_mesh_render_device(m, n, p->W, p->H, Ks + 9 * (size_t)c0, Rs + 9 * (size_t)c0, ts + 3 * (size_t)c0, clip_near, clip_far, 0.f,
                                        1, true, false)))
            return rc;
        HIP_TRY(hipMemcpyAsync(p->icp->d_models.p + ((size_t)slot0 + c0) * npx, m->d_depth.p, (size_t)n * npx * sizeof(uint16_t),
                               hipMemcpyDeviceToDevice, m->s));
        HIP_TRY(lm::launch_icp_model_boxes(p->icp->d_models.p, p->icp->d_model_bbox.p, slot0 + c0, n, p->W, p->H, m->s));   // the boxes of the new views, once (LL.cpp:43-50)
        for (int i = 0; i < n; ++i) p->icp->slot_boxed[(size_t)slot0 + c0 + i] = 1;
        HIP_TRY(hipStreamSynchronize(m->s));
    }
    record_views(p, slot0, count, Ks, Rs, ts, box_wh);
    return LM_OK;
}

static int ensure_run_buffers(lm_pipeline* p, int top_k, int num_classes) {
    int rc;
    const size_t views = (size_t)std::max(p->num_views, 1), classes = (size_t)std::max(num_classes, 8);
    if (p->views_dirty || p->d_view_K.cap < views * 9) {          // new views, or tables about to be replaced: upload them
        if ((rc = p->d_view_K.ensure(views * 9)) || (rc = p->d_view_valid.ensure(views)) || (rc = p->d_view_wh.ensure(views * 2))) return rc;
        if (p->num_views) {
            HIP_TRY(hipMemcpy(p->d_view_K.p, p->view_K.data(), (size_t)p->num_views * 9 * sizeof(float), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(p->d_view_valid.p, p->view_valid.data(), (size_t)p->num_views * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(p->d_view_wh.p, p->view_wh.data(), (size_t)p->num_views * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        p->views_dirty = false;
    }
    if ((rc = p->d_sel.ensure((size_t)top_k)) || (rc = p->h_sel.ensure((size_t)top_k)) || (rc = p->d_nsel.ensure(4)) || (rc = p->h_nsel.ensure(4))) return rc;
    if (p->d_class_base.cap < classes) p->class_base_on_device.clear();   // the table is replaced: the next run uploads it
    if ((rc = p->d_class_base.ensure(classes)) || (rc = p->h_class_base.ensure(classes))) return rc;
    return p->d_scratch.ensure(topk_nms_scratch_bytes(p->det->cand_cap));
}

extern "C" int lm_pipeline_run(lm_pipeline* p, float threshold, const char* const* class_ids, int num_class_ids, const float* scene_K,
                               int top_k, double nms_iou, int flags, lm_detection* out, int* n_out, lm_pipeline_timings* tm) {
    if (!p || !scene_K || top_k <= 0 || !out || !n_out) return lm_set_error(LM_ERR_INVALID, "null argument");
    *n_out = 0;
    lm_detector* d = p->det;
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "a frame is in flight on the detector: collect it first");
    if (int rc = lm_parts_refused(d, "lm_pipeline_run")) return rc;
    if (!d->frame_valid || d->fW != p->W || d->fH != p->H)
        return lm_set_error(LM_ERR_INVALID, "the detector's resident frame is not %dx%d", p->W, p->H);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t s = d->mstream;                                   // after the matching kernels of the frame
    lm_icp* c = p->icp;
    int rc;
    if ((rc = lm_icp_ensure_arenas(c, top_k))) return rc;
    int overflows = 0;
    for (;;) {                                                    // one pass normally; again after a candidate-buffer overflow (<= 3) 
        HIP_TRY(hipEventRecord(p->e0, d->stream));
        if ((rc = lm_submit_frame(d, threshold, class_ids, num_class_ids))) return rc;
        // class position (caller's class_ids order, or sorted order) -> first view slot
        std::vector<std::string> order;
        if (class_ids && num_class_ids > 0) for (int i = 0; i < num_class_ids; ++i) order.push_back(class_ids[i] ? class_ids[i] : "");
        else order = d->bank_classes;
        if ((rc = ensure_run_buffers(p, top_k, (int)order.size()))) return rc;
        for (size_t i = 0; i < order.size(); ++i) {
            auto it = p->views.find(order[i]);
            p->h_class_base.p[i] = it == p->views.end() ? -1 : it->second.base;
        }
        if (!order.empty() && (p->class_base_on_device.size() != order.size() ||
                               memcmp(p->class_base_on_device.data(), p->h_class_base.p, order.size() * sizeof(int32_t)) != 0)) {
            // the stream order keeps earlier frames' kernels ahead of this copy; the pinned source is stable until the next change
            HIP_TRY(hipMemcpyAsync(p->d_class_base.p, p->h_class_base.p, order.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            p->class_base_on_device.assign(p->h_class_base.p, p->h_class_base.p + order.size());
        }
        HIP_TRY(hipEventRecord(p->e1, s));
        const int slot = (int)((d->n_submitted - 1) % lm_detector::kSlots);          // the frame just submitted
        HIP_TRY(launch_topk_nms(d->d_matches_dev.p + (size_t)d->buf_cand_cap * slot, d->d_final.p + 8 * (size_t)slot, d->buf_cand_cap, d->d_work.p, d->d_work_cls.p, d->d_work_tid.p,
                                d->d_entries.p, d->pyramid_levels, p->d_class_base.p, p->d_view_wh.p, p->num_views, top_k, nms_iou, p->d_scratch.p, p->d_sel.p, p->d_nsel.p, s));
        HIP_TRY(launch_icp_bind(p->d_sel.p, p->d_nsel.p, p->d_class_base.p, p->d_view_K.p, p->d_view_valid.p, p->num_views, c->ar.in.p, c->ar.st.p, top_k, s));
        HIP_TRY(hipEventRecord(p->e2, s));
        IcpBuffers B = c->buffers();
        B.scene = d->cur_depth;
        B.count = top_k;
        memcpy(B.sK, scene_K, sizeof(B.sK));
        // (k_icp_bind only binds views that were uploaded, and both upload paths work out the boxes: 0x100 = no k_icp_bbox)
        if ((rc = lm_icp_enqueue(c, B, (flags & 0xFF) | 0x100, c->ar.h_st.p, s))) return rc;
        HIP_TRY(hipMemcpyAsync(p->h_sel.p, p->d_sel.p, (size_t)top_k * sizeof(TopkSel), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(p->h_nsel.p, p->d_nsel.p, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        rc = lm_collect_frame(d, -1, nullptr, nullptr);          // retires the frame; 1 = candidate buffer overflow, rerun
        if (rc == 1) {
            if (++overflows >= 3) return lm_set_error(LM_ERR_INVALID, "candidate buffer kept overflowing");
            continue;
        }
        if (rc) return rc;
        if ((rc = lm_icp_finish(c, B, c->ar.h_st.p, s))) return rc;
        break;
    }
    if (p->h_nsel.p[1] != 0)
        return lm_set_error(LM_ERR_INVALID, "on-device NMS: a match field exceeds the packed record (template id >= 2^24, class position >= 128 or |x|,|y| >= 32768)");
    c->last_count = top_k; c->last_flags = flags;
    const int n = p->h_nsel.p[0];
    for (int i = 0; i < n; ++i) {
        const TopkSel& sl = p->h_sel.p[i];
        const IcpState& st = c->ar.h_st.p[i];
        lm_detection& o = out[i];
        memset(&o, 0, sizeof(o));
        o.match.x = sl.x; o.match.y = sl.y; o.match.similarity = sl.similarity;
        o.match.class_index = sl.class_index; o.match.template_id = sl.template_id;
        o.width = sl.width; o.height = sl.height;
        o.pose.residual = -1.f;
        o.status = st.status;
        if (st.status == 2) return lm_set_error(LM_ERR_INVALID, "rendered depth of template %d is empty", sl.template_id);
        if (st.status == 3) return lm_set_error(LM_ERR_INVALID, "detection %d: point cloud too large for 64-bit voxel keys", i);
        if (st.status == lm::kIcpStalled) return lm_set_error(LM_ERR_HIP, "detection %d: the point kernels stalled (strips waited a second for each other)", i);
        if (st.status != 0) continue;                             // 1: window leaves the frame (LL.cpp:52-55); 5: no view for the template
        const int base = p->h_class_base.p[sl.class_index];
        const size_t v = (size_t)base + sl.template_id;
        lm_icp_compose_result(st, &p->view_R[v * 9], &p->view_t[v * 3], &o.pose);
        o.pose.stage = c->stage[(size_t)i];
    }
    *n_out = n;
    if (tm) {
        memset(tm, 0, sizeof(*tm));
        (void)hipEventElapsedTime(&tm->match_ms, p->e0, p->e1);
        (void)hipEventElapsedTime(&tm->nms_ms, p->e1, p->e2);
        (void)hipEventElapsedTime(&tm->icp_ms, p->e2, c->e1);
        (void)hipEventElapsedTime(&tm->total_ms, p->e0, c->e1);
        tm->coarse_candidates = d->timings.coarse_candidates;
        tm->matches_pre_unique = d->timings.matches_pre_unique;
        int its = 0;
        for (int i = 0; i < n; ++i) if (c->ar.h_st.p[i].status == 0) its += c->ar.h_st.p[i].iterations;
        tm->icp_iterations = its;
        tm->nms_records = p->h_nsel.p[2];
    }
    return LM_OK;
}

extern "C" int64_t lm_pipeline_read_icp_debug(lm_pipeline* p, int hypothesis, int kind, double* dst, int64_t capacity) {
    if (!p) return lm_set_error(LM_ERR_INVALID, "null argument");
    return lm_icp_read_debug(p->icp, hypothesis, kind, dst, capacity);
}
