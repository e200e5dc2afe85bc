// The template bank: training on the host and on the device (added frames, rendered views), class and parameter files, the packed
// bank, the bank's device image (upload_bank) and the work list of a class selection (build_work).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "detector_internal.h"
#include "render_internal.h"

// ---- bank -----------------------------------------------------------------------------------------
static int validate_pyramid(const lm_detector* d, const TemplatePyramid& tp) {
    if ((int)tp.size() != d->pyramid_levels * d->nmod)
        return lm_set_error(LM_ERR_INVALID, "template pyramid has %d entries, detector expects %d", (int)tp.size(),
                            d->pyramid_levels * d->nmod);
    for (const Template& t : tp) {
        if (t.features.size() > 8191) return lm_set_error(LM_ERR_INVALID, "templ.features.size() <= 8191 [LL.cpp:1291]");
        for (const Feature& f : t.features) {
            if (f.label < 0 || f.label > 7) return lm_set_error(LM_ERR_INVALID, "feature label %d outside [0,8)", f.label);
            if (f.x < -32768 || f.x > 32767 || f.y < -32768 || f.y > 32767)
                return lm_set_error(LM_ERR_INVALID, "feature coordinate outside the supported int16 range");
        }
    }
    return LM_OK;
}

// Detector::addTemplate on the frame resident in frame_rgb / frame_depth (LL.cpp:1943-1975).
static int resident_host_selection(lm_detector* d, const uint8_t* mask, int width, int height, const char* class_id) {
    // quantise() in addTemplate passes object_mask to every modality (LL.cpp:1957), but the masked
    // quantised image is not used by extractTemplate; only the unmasked maps + the mask are.
    int rc;
    if ((rc = run_frontend_training(d))) return rc;
    d->frame_valid = false;   // LM arena not built for this frame
    const int L = d->pyramid_levels;
    std::vector<TemplatePyramid>& tps = d->class_templates[class_id];   // created even on failure, LL.cpp:1947
    d->bank_dirty = true;
    const int nm = d->nmod;
    TemplatePyramid tp((size_t)nm * L);                                 // levels x modalities of the set (matchClass's layout, LL.cpp:1806-1812)
    std::vector<uint8_t> hmask, nmask;
    if (mask) hmask.assign(mask, mask + (size_t)width * height);
    size_t nf = (size_t)d->num_features;
    int ext = d->extract_threshold;
    std::vector<float> mag;
    std::vector<uint8_t> ang, nrm;
    for (int l = 0; l < L; ++l) {
        const LevelBufs& b = d->lvl[l];
        const size_t n = (size_t)b.W * b.H;
        if (l > 0) {
            nf /= 2;            // LL.cpp:560, 860
            ext /= 2;           // LL.cpp:861
            if (mask) {         // resize(mask, INTER_NEAREST)
                const LevelBufs& a = d->lvl[l - 1];
                nmask.resize(n);
                for (int y = 0; y < b.H; ++y)
                    for (int x = 0; x < b.W; ++x) nmask[(size_t)y * b.W + x] = hmask[(size_t)(2 * y) * a.W + 2 * x];
                hmask.swap(nmask);
            }
        }
        mag.resize(n); ang.resize(n); nrm.resize(n);
        if (d->use[0]) HIP_TRY(hipMemcpyAsync(mag.data(), b.mag.p, n * sizeof(float), hipMemcpyDeviceToHost, d->stream));
        if (d->use[0]) HIP_TRY(hipMemcpyAsync(ang.data(), b.ang.p, n, hipMemcpyDeviceToHost, d->stream));
        if (d->use[1]) HIP_TRY(hipMemcpyAsync(nrm.data(), b.nrm.p, n, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        const uint8_t* mp = mask ? hmask.data() : nullptr;
        // reference order is modality-major (LL.cpp:1954-1968); the outcome (-1 on any failure) is the same
        // (only the modalities of the set decide: a colour-only detector accepts a view with flat depth)
        for (int i = 0; i < nm; ++i) {
            Template& t = tp[(size_t)nm * l + i];
            if (d->mod_kind[i] == 0 ? !extract_color_template(mag.data(), ang.data(), mp, b.W, b.H, nf, d->strong_threshold, l, t)
                                    : !extract_normal_template(nrm.data(), mp, b.W, b.H, nf, ext, l, t)) return -1;
        }
    }
    crop_templates(tp);                                                 // the bounding box of the set's templates only (LL.cpp:234-277)
    if ((rc = validate_pyramid(d, tp))) return rc;
    tps.push_back(std::move(tp));
    return (int)tps.size() - 1;
}

// ... counted for lm_detector_train_stats: a view of the host selection, and whether it failed
static int add_template_resident(lm_detector* d, const uint8_t* mask, int width, int height, const char* class_id) {
    ++d->train_stats[1];
    const int id = resident_host_selection(d, mask, width, height, class_id);
    if (id == -1) ++d->train_stats[2];
    return id;
}

// The scratch of the device selection for `views` views of the current geometry, and the maps it reads (the detector's level buffers).
static int train_buffers(lm_detector* d, int views, TrainGeom& g) {
    lm_detector::Train& T = d->train;
    const int L = d->pyramid_levels;
    const size_t out_words = 4 + 3 * (size_t)std::max(1, d->num_features);
    int rc;
    g.levels = L;
    for (int l = 0; l < L; ++l) {
        const LevelBufs& b = d->lvl[l];
        const size_t nl = (size_t)b.W * b.H;
        if ((rc = T.mask[l].ensure(nl)) || (rc = T.lab[l].ensure(nl)) || (rc = T.hrun[l].ensure(nl))) return rc;
        g.W[l] = b.W; g.H[l] = b.H; g.mag[l] = b.mag.p; g.ang[l] = b.ang.p; g.nrm[l] = b.nrm.p;
        g.mask[l] = T.mask[l].p; g.lab[l] = T.lab[l].p; g.hrun[l] = T.hrun[l].p;
    }
    const size_t keys_view = (size_t)L * 2 * kTrainCap, counts_view = (size_t)L * 16;
    if ((rc = T.keys.ensure(keys_view * views)) || (rc = T.counts.ensure(counts_view * views)) || (rc = T.bbox.ensure(4 * (size_t)views)) ||
        (rc = T.out.ensure((size_t)views * L * 2 * out_words)))
        return rc;
    return LM_OK;
}

// One view's output of k_train_select ([levels][2][out_words], every status 1) as a template pyramid of the class: cropTemplates,
// the bank's limits, push_back.  Returns the template id.
static int push_selected_pyramid(lm_detector* d, std::vector<TemplatePyramid>& tps, const int32_t* out_view, size_t out_words) {
    const int L = d->pyramid_levels;
    const int nm = d->nmod;
    TemplatePyramid tp((size_t)nm * L);
    for (int e = 0; e < nm * L; ++e) {                                  // the device layout stays [levels][2 kinds]; a set of one reads its kind's records
        const int32_t* o = out_view + (size_t)((e / nm) * 2 + d->mod_kind[e % nm]) * out_words;
        Template& t = tp[e];
        t.pyramid_level = e / nm;
        t.features.resize((size_t)o[1]);
        for (int k = 0; k < o[1]; ++k) t.features[k] = Feature{o[4 + 3 * k], o[4 + 3 * k + 1], o[4 + 3 * k + 2]};
    }
    crop_templates(tp);
    int rc = validate_pyramid(d, tp);
    if (rc) return rc;
    tps.push_back(std::move(tp));
    return (int)tps.size() - 1;
}

// Detector::addTemplate with an object mask, selection on the device (train.hip): the quantised maps never leave HBM, only the
// chosen features come back.  Candidate lists beyond what the selection kernel sorts in LDS go to add_template_resident.
static int add_template_device(lm_detector* d, const uint8_t* mask, int width, int height, const char* class_id) {
    int rc;
    if ((rc = run_frontend_training(d))) return rc;
    d->frame_valid = false;   // LM arena not built for this frame
    lm_detector::Train& T = d->train;
    const int L = d->pyramid_levels;
    const int nf_cap = std::max(1, d->num_features);
    const size_t out_words = 4 + 3 * (size_t)nf_cap, npx = (size_t)width * height;
    TrainGeom g{};
    if ((rc = train_buffers(d, 1, g)) || (rc = T.user_mask.ensure(npx))) return rc;
    hipStream_t s = d->stream;
    HIP_TRY(hipMemcpyAsync(T.user_mask.p, mask, npx, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(T.counts.p, 0, (size_t)L * 16 * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(T.bbox.p, 0x80, 4 * sizeof(int32_t), s));
    const int mods = (d->use[0] ? 1 : 0) | (d->use[1] ? 2 : 0);
    HIP_TRY(launch_train_prep(d->frame_depth.p, T.user_mask.p, g, d->strong_threshold * d->strong_threshold, d->extract_threshold, T.keys.p, kTrainCap, T.counts.p,
                              T.bbox.p, s, mods));
    HIP_TRY(launch_train_select(T.keys.p, T.counts.p, g, kTrainCap, d->num_features, nf_cap, 1, T.out.p, s, mods));   // (or the kernel's LDS cannot be reserved)
    std::vector<int32_t> h_out((size_t)L * 2 * out_words);
    HIP_TRY(hipMemcpyAsync(h_out.data(), T.out.p, h_out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    bool ok = true, host_path = false;
    for (int e = 0; e < 2 * L; ++e) {
        if (!d->use[e & 1]) continue;                                   // nothing was selected for a kind outside the set
        const int32_t st = h_out[(size_t)e * out_words];
        host_path |= st == 2;
        ok &= st == 1;
    }
    if (host_path) return add_template_resident(d, mask, width, height, class_id);
    std::vector<TemplatePyramid>& tps = d->class_templates[class_id];   // created even on failure, LL.cpp:1947
    d->bank_dirty = true;
    ++d->train_stats[0];
    if (!ok) { ++d->train_stats[2]; return -1; }
    return push_selected_pyramid(d, tps, h_out.data(), out_words);
}

extern "C" int lm_detector_add_template(lm_detector* d, const uint8_t* rgb, const uint16_t* depth, const uint8_t* mask,
                                        int width, int height, const char* class_id) {
    if (!d || !class_id) return lm_set_error(LM_ERR_INVALID, "null argument");
    int rc = upload_frame(d, rgb, depth, width, height, nullptr, false);   // (checks the sources against the modality set)
    if (rc) return rc;
    // with an object mask (what every training loop of the reference passes) the selection runs on the device; LM_TRAIN_HOST=1 and
    // detectors beyond kTrainMaxFeatures features keep it on the host, as does a call without mask (no erosion, candidates anywhere)
    const char* force_host = getenv("LM_TRAIN_HOST");
    bool on_device = mask && !(force_host && force_host[0] && force_host[0] != '0') && d->num_features >= 1 && d->num_features <= kTrainMaxFeatures;
    if (on_device) {          // the device works on object / background; a grey mask (cv::erode takes minima, cv::subtract differences) stays on the host
        uint8_t v = 0;
        const size_t npx = (size_t)width * height;
        for (size_t i = 0; i < npx && on_device; ++i)
            if (mask[i]) { if (!v) v = mask[i]; else on_device = mask[i] == v; }
    }
    return on_device ? add_template_device(d, mask, width, height, class_id) : add_template_resident(d, mask, width, height, class_id);
}

// render_train (linemod_and_levelup_test.py:170-252) on the device: the rendered colour / depth images go from the
// rasteriser's buffers into the detector's frame buffers without touching the host, the quantisers and the feature selection
// (train.hip) run there too, and only the chosen features, the bounding boxes and the candidate counts come back — once per
// chunk of views, not per view.  A view whose candidate lists exceed what the selection kernel sorts in LDS (very large
// objects), or a detector with more than kTrainMaxFeatures features, takes the host selection (add_template_resident), which
// yields the same templates; LM_TRAIN_HOST=1 forces it (tests compare the two).
// The rasteriser's colour image of a view into the detector's frame buffer: as it is, or — a grey detector — through the fixed-point RGB2GRAY of
// k_rgb_to_grey (what lm_rgb_to_grey gives a caller who trains from colour photographs), without leaving the device.
static int rendered_colour_to_frame(lm_detector* d, const uint8_t* view_rgb, size_t npx, hipStream_t s) {
    if (d->cch == 1) HIP_TRY(launch_rgb_to_grey(view_rgb, d->frame_rgb.p, npx, s));
    else HIP_TRY(hipMemcpyAsync(d->frame_rgb.p, view_rgb, npx * 3, hipMemcpyDeviceToDevice, s));
    return LM_OK;
}

static int add_rendered_view_host(lm_detector* d, lm_mesh* m, int i, int width, int height, const char* class_id, std::vector<uint16_t>& hdepth,
                                  std::vector<uint8_t>& hmask, int32_t* box_wh_view) {
    const size_t npx = (size_t)width * height;
    d->frame_valid = false;
    d->have_mask[0] = d->have_mask[1] = false;
    d->cur_rgb = d->frame_rgb.p; d->cur_depth = d->frame_depth.p;
    if (d->use[0]) { int rc = rendered_colour_to_frame(d, m->d_rgb.p + (size_t)i * npx * 3, npx, d->stream); if (rc) return rc; }
    if (d->use[1]) HIP_TRY(hipMemcpyAsync(d->frame_depth.p, m->d_depth.p + (size_t)i * npx, npx * 2, hipMemcpyDeviceToDevice, d->stream));
    HIP_TRY(hipMemcpyAsync(hdepth.data(), m->d_depth.p + (size_t)i * npx, npx * 2, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    int x0 = width, y0 = height, x1 = -1, y1 = -1;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const bool on = hdepth[(size_t)y * width + x] > 0;
            hmask[(size_t)y * width + x] = on ? 255 : 0;                       // mask = (depth > 0) * 255 (:238)
            if (on) { x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y); }
        }
    if (box_wh_view) {                                                         // xmax - xmin, ymax - ymin (:235-236)
        box_wh_view[0] = x1 >= 0 ? x1 - x0 : 0;
        box_wh_view[1] = y1 >= 0 ? y1 - y0 : 0;
    }
    if (x1 < 0) { ++d->train_stats[3]; return -1; }
    return add_template_resident(d, hmask.data(), width, height, class_id);
}

static int add_templates_rendered(lm_detector* d, lm_mesh* m, const char* class_id, int count, int width, int height, const float* Ks,
                                  const float* Rs, const float* ts, float clip_near, float clip_far, float ambient, int ssaa,
                                  int32_t* template_ids, int32_t* box_wh, const lm_shade_opts* shade) {
    if (!d || !m || !class_id || count < 0 || (count && (!Ks || !Rs || !ts || !template_ids)))
        return lm_set_error(LM_ERR_INVALID, "null argument");
    if (m->device != d->device) return lm_set_error(LM_ERR_INVALID, "mesh and detector live on different devices");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "a frame is in flight: collect it first");
    LM_DIAG_IDLE(d, "lm_detector_add_templates_rendered");
    if (width < 16 || height < 16) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    HIP_TRY(hipSetDevice(d->device));
    const size_t npx = (size_t)width * height;
    const size_t per_view = npx * (size_t)ssaa * ssaa * sizeof(unsigned long long);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(64, ((size_t)2 << 30) / std::max<size_t>(per_view, 1)));
    std::vector<uint16_t> hdepth(npx);
    std::vector<uint8_t> hmask(npx);
    const char* force_host = getenv("LM_TRAIN_HOST");
    const bool on_device = !(force_host && force_host[0] && force_host[0] != '0') && d->num_features >= 1 && d->num_features <= kTrainMaxFeatures;
    const int L = d->pyramid_levels;
    const int nf_cap = std::max(1, d->num_features);
    const size_t out_words = 4 + 3 * (size_t)nf_cap;
    std::vector<int32_t> h_out, h_bbox;
    int rc;
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int n = std::min(chunk, count - c0);
        // the depth image is always resolved: it is the object mask (:238) also where no normals are taken from it; the shaded colour only for a
        // detector that has the colour modality
        rc = shade ? lm_mesh_render_device_shaded(m, n, width, height, Ks + 9 * (size_t)c0, Rs + 9 * (size_t)c0, ts + 3 * (size_t)c0, *shade, true, d->use[0])
                   : lm_mesh_render_device(m, n, width, height, Ks + 9 * (size_t)c0, Rs + 9 * (size_t)c0, ts + 3 * (size_t)c0, clip_near, clip_far,
                                           ambient, ssaa, true, d->use[0]);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(m->s));
        if ((rc = setup_geometry(d, width, height, false))) return rc;
        if (!on_device) {
            for (int i = 0; i < n; ++i) {
                const int id = add_rendered_view_host(d, m, i, width, height, class_id, hdepth, hmask, box_wh ? box_wh + 2 * ((size_t)c0 + i) : nullptr);
                if (id < -1) return id;
                template_ids[(size_t)c0 + i] = id;
            }
            continue;
        }
        // ---- device selection: prepare every view of the chunk, select them all in one launch ----
        lm_detector::Train& T = d->train;
        TrainGeom g{};
        if ((rc = train_buffers(d, n, g))) return rc;
        const size_t keys_view = (size_t)L * 2 * kTrainCap, counts_view = (size_t)L * 16;
        hipStream_t s = d->stream;
        HIP_TRY(hipMemsetAsync(T.counts.p, 0, counts_view * n * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(T.bbox.p, 0x80, 4 * (size_t)n * sizeof(int32_t), s));        // large negative: k_train_mask takes maxima
        d->frame_valid = false;
        d->have_mask[0] = d->have_mask[1] = false;
        const float strong_sq = d->strong_threshold * d->strong_threshold;
        const int mods = (d->use[0] ? 1 : 0) | (d->use[1] ? 2 : 0);
        for (int i = 0; i < n; ++i) {
            d->cur_rgb = d->frame_rgb.p; d->cur_depth = d->frame_depth.p;
            const uint16_t* view_depth = m->d_depth.p + (size_t)i * npx;  // a colour-only detector has no depth frame: the mask comes from the rasteriser's buffer
            if (d->use[0] && (rc = rendered_colour_to_frame(d, m->d_rgb.p + (size_t)i * npx * 3, npx, s))) return rc;
            if (d->use[1]) HIP_TRY(hipMemcpyAsync(d->frame_depth.p, view_depth, npx * 2, hipMemcpyDeviceToDevice, s));
            if ((rc = run_frontend_training(d))) return rc;
            HIP_TRY(launch_train_prep(d->use[1] ? d->frame_depth.p : view_depth, nullptr, g, strong_sq, d->extract_threshold, T.keys.p + keys_view * i, kTrainCap,
                                      T.counts.p + counts_view * i, T.bbox.p + 4 * (size_t)i, s, mods));
        }
        HIP_TRY(launch_train_select(T.keys.p, T.counts.p, g, kTrainCap, d->num_features, nf_cap, n, T.out.p, s, mods));   // (or the kernel's LDS cannot be reserved)
        h_out.resize((size_t)n * L * 2 * out_words);
        h_bbox.resize(4 * (size_t)n);
        HIP_TRY(hipMemcpyAsync(h_out.data(), T.out.p, h_out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_bbox.data(), T.bbox.p, h_bbox.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<TemplatePyramid>& tps = d->class_templates[class_id];   // created even when every view fails, LL.cpp:1947
        d->bank_dirty = true;
        for (int i = 0; i < n; ++i) {
            const int32_t* bb = &h_bbox[4 * (size_t)i];
            const bool any = bb[2] >= 0;
            int id = -1;
            bool host_path = false;
            if (any) {
                bool ok = true;
                for (int e = 0; e < 2 * L; ++e) {
                    if (!d->use[e & 1]) continue;
                    const int32_t st = h_out[((size_t)i * L * 2 + e) * out_words];
                    host_path |= st == 2;
                    ok &= st == 1;
                }
                if (host_path) {                                               // this view through the host selection, in view order
                    id = add_rendered_view_host(d, m, i, width, height, class_id, hdepth, hmask, nullptr);
                    if (id < -1) return id;
                } else {
                    ++d->train_stats[0];
                    if (!ok) ++d->train_stats[2];
                    else if ((id = push_selected_pyramid(d, tps, &h_out[(size_t)i * L * 2 * out_words], out_words)) < -1) return id;
                }
            } else {
                ++d->train_stats[3];
            }
            if (box_wh) {                                                      // xmax - xmin, ymax - ymin (:235-236)
                box_wh[2 * ((size_t)c0 + i)] = any ? bb[2] + bb[0] : 0;
                box_wh[2 * ((size_t)c0 + i) + 1] = any ? bb[3] + bb[1] : 0;
            }
            template_ids[(size_t)c0 + i] = id;
        }
    }
    return LM_OK;
}

extern "C" int lm_detector_add_templates_rendered(lm_detector* d, lm_mesh* m, const char* class_id, int count, int width, int height,
                                                  const float* Ks, const float* Rs, const float* ts, float clip_near, float clip_far,
                                                  float ambient, int ssaa, int32_t* template_ids, int32_t* box_wh) {
    return add_templates_rendered(d, m, class_id, count, width, height, Ks, Rs, ts, clip_near, clip_far, ambient, ssaa, template_ids, box_wh, nullptr);
}

// render_train with renderer.render's texture / shading / bg_color (linemod_and_levelup_test.py:193-227 passes texture=model_texture)
extern "C" int lm_detector_add_templates_rendered_ex(lm_detector* d, lm_mesh* m, const char* class_id, int count, int width, int height,
                                                     const float* Ks, const float* Rs, const float* ts, const lm_render_options* options,
                                                     int32_t* template_ids, int32_t* box_wh) {
    if (!d || !m || !class_id) return lm_set_error(LM_ERR_INVALID, "null argument");
    lm_shade_opts o;
    int rc = lm_parse_render_options(m, options, &o);
    if (rc) return rc;
    if (o.ssaa < 1 || o.ssaa > 8) return lm_set_error(LM_ERR_INVALID, "ssaa must be in 1..8");
    return add_templates_rendered(d, m, class_id, count, width, height, Ks, Rs, ts, o.clip_near, o.clip_far, o.ambient, o.ssaa, template_ids, box_wh, &o);
}

extern "C" int lm_detector_read_class(lm_detector* d, const char* path, const char* class_id_override) {
    if (!d || !path) return lm_set_error(LM_ERR_INVALID, "null argument");
    std::string cid, err;
    std::vector<std::string> mods;
    int levels = 0;
    std::vector<TemplatePyramid> tps;
    if (!read_class_yaml(path, cid, mods, levels, tps, err)) {
        bool assertion = err.find("LL.cpp") != std::string::npos;
        return lm_set_error(assertion ? LM_ERR_INVALID : LM_ERR_IO, "%s", err.c_str());
    }
    bool same = (int)mods.size() == d->nmod;                        // the file's list against the detector's, element by element
    for (int i = 0; same && i < d->nmod; ++i) same = mods[i] == kModalityName[d->mod_kind[i]];
    if (!same) return lm_set_error(LM_ERR_INVALID, "modalities mismatch [LL.cpp:2047-2051]");
    if (levels != d->pyramid_levels)
        return lm_set_error(LM_ERR_INVALID, "(int)fn[\"pyramid_levels\"] == pyramid_levels violated (%d vs %d) [LL.cpp:2052]",
                            levels, d->pyramid_levels);
    if (class_id_override && class_id_override[0]) cid = class_id_override;
    else if (d->class_templates.count(cid))
        return lm_set_error(LM_ERR_INVALID, "class '%s' already present [LL.cpp:2059]", cid.c_str());
    for (const TemplatePyramid& tp : tps) { int rc = validate_pyramid(d, tp); if (rc) return rc; }
    if (!d->class_templates.count(cid)) d->class_templates[cid] = std::move(tps);   // map::insert keeps an existing key
    d->bank_dirty = true;
    return LM_OK;
}

extern "C" int lm_detector_write_class(lm_detector* d, const char* class_id, const char* path) {
    if (!d || !class_id || !path) return lm_set_error(LM_ERR_INVALID, "null argument");
    auto it = d->class_templates.find(class_id);
    if (it == d->class_templates.end()) return lm_set_error(LM_ERR_NOT_FOUND, "unknown class '%s' [LL.cpp:2096]", class_id);
    std::string err;
    const std::string mods = d->nmod == 2 ? "ColorGradient, DepthNormal" : kModalityName[d->mod_kind[0]];
    if (!write_class_yaml(path, it->first, it->second, d->pyramid_levels, err, mods.c_str())) return lm_set_error(LM_ERR_IO, "%s", err.c_str());
    return LM_OK;
}

// Detector::write / Detector::read (LL.cpp:2013-2041) with the modality parameters of ColorGradient::write (:686-692) and
// DepthNormal::write (:1012-1020), OpenCV FileStorage YAML 1.0 layout.  read() clears the classes like the reference.
extern "C" int lm_detector_write_params(const lm_detector* d, const char* path) {
    if (!d || !path) return lm_set_error(LM_ERR_INVALID, "null argument");
    FILE* f = fopen(path, "w");
    if (!f) return lm_set_error(LM_ERR_IO, "cannot open for writing: %s", path);
    auto real = [](float v) {                                   // cv::FileStorage prints 10.f as "10."
        char b[64];
        snprintf(b, sizeof(b), "%.8g", (double)v);
        std::string s(b);
        if (s.find_first_of(".eEn") == std::string::npos) s += ".";
        return s;
    };
    fprintf(f, "%%YAML:1.0\n---\npyramid_levels: %d\nT: [", d->pyramid_levels);
    for (size_t i = 0; i < d->T_at_level.size(); ++i) fprintf(f, "%s %d", i ? "," : "", d->T_at_level[i]);
    fprintf(f, " ]\nmodalities:\n");
    if (d->use[0])
    fprintf(f, "   -\n      type: ColorGradient\n      weak_threshold: %s\n      num_features: %d\n      strong_threshold: %s\n",
            real(d->weak_threshold).c_str(), d->num_features, real(d->strong_threshold).c_str());
    if (d->use[1])
    fprintf(f, "   -\n      type: DepthNormal\n      distance_threshold: %d\n      difference_threshold: %d\n      num_features: %d\n"
               "      extract_threshold: %d\n",
            d->distance_threshold, d->difference_threshold, d->num_features, d->extract_threshold);
    if (fclose(f) != 0) return lm_set_error(LM_ERR_IO, "write failed: %s", path);
    return LM_OK;
}

extern "C" int lm_detector_read_params(lm_detector* d, const char* path) {
    if (!d || !path) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "a frame is in flight: collect it first");
    FILE* f = fopen(path, "r");
    if (!f) return lm_set_error(LM_ERR_IO, "cannot open: %s", path);
    int levels = -1, nf[2] = {-1, -1}, dist = d->distance_threshold, diff = d->difference_threshold, ext = d->extract_threshold;
    float weak = d->weak_threshold, strong = d->strong_threshold;
    std::vector<int> T;
    std::vector<std::string> types;
    char line[1024];
    while (fgets(line, sizeof(line), f)) {
        char* p = line;
        while (*p == ' ' || *p == '\t' || *p == '-') ++p;
        char key[64];
        if (sscanf(p, "%63[A-Za-z_]:", key) != 1) continue;
        const char* v = strchr(p, ':') + 1;
        const std::string k(key);
        const std::string cur = types.empty() ? "" : types.back();
        if (k == "pyramid_levels") levels = atoi(v);
        else if (k == "T") { for (const char* q = v; *q; ++q) if (*q >= '0' && *q <= '9') { T.push_back(atoi(q)); while (*q >= '0' && *q <= '9') ++q; --q; } }
        else if (k == "type") { char t[64] = {0}; sscanf(v, " %63s", t); types.push_back(t); }
        else if (k == "weak_threshold") weak = (float)atof(v);
        else if (k == "strong_threshold") strong = (float)atof(v);
        else if (k == "num_features") { if (cur == "ColorGradient") nf[0] = atoi(v); else if (cur == "DepthNormal") nf[1] = atoi(v); }
        else if (k == "distance_threshold") dist = atoi(v);
        else if (k == "difference_threshold") diff = atoi(v);
        else if (k == "extract_threshold") ext = atoi(v);
    }
    fclose(f);
    if (levels < 1 || levels > kMaxLevels || (int)T.size() != levels) return lm_set_error(LM_ERR_IO, "%s: pyramid_levels / T missing or inconsistent", path);
    // Modality::create (LL.cpp:320-328) knows these two.  The reference's read() REPLACES the modality list; here the set is fixed at creation
    // (buffers, job tables and the bank layout follow from it), so a file with another list is refused.
    bool same = (int)types.size() == d->nmod;
    for (int i = 0; same && i < d->nmod; ++i) same = types[i] == kModalityName[d->mod_kind[i]];
    if (!same) {
        if (d->nmod == 2) return lm_set_error(LM_ERR_INVALID, "%s: modalities must be [ColorGradient, DepthNormal]", path);
        return lm_set_error(LM_ERR_INVALID, "%s: modalities must be [%s], the detector's set", path, kModalityName[d->mod_kind[0]]);
    }
    if (d->nmod == 1) nf[0] = nf[1] = nf[d->mod_kind[0]];
    if (nf[0] <= 0 || nf[0] != nf[1]) return lm_set_error(LM_ERR_INVALID, "%s: the modalities must agree on num_features (one bank layout)", path);
    if ((nf[0] >> (levels - 1)) < 1)
        return lm_set_error(LM_ERR_INVALID, "%s: num_features %d leaves no feature at the last of %d pyramid levels (num_features /= 2 per level, "
                            "LL.cpp:560; LL.cpp:632 then divides by zero)", path, nf[0], levels);
    for (int t : T) if (t < 1) return lm_set_error(LM_ERR_INVALID, "T must be >= 1");
    d->class_templates.clear();                                   // LL.cpp:2015
    d->class_depth_range.clear();                                 // (the ranges go with their classes)
    d->class_train_depth.clear();                                 // (and the training depths)
    d->bank_dirty = true; d->work_valid = false; d->frame_valid = false;
    d->pyramid_levels = levels; d->T_at_level = T;
    d->num_features = nf[0]; d->weak_threshold = weak; d->strong_threshold = strong;
    d->distance_threshold = dist; d->difference_threshold = diff; d->extract_threshold = ext;
    d->fW = d->fH = 0;                                            // geometry depends on T: rebuilt by the next frame
    for (int64_t& c : d->train_stats) c = 0;
    return LM_OK;
}

extern "C" int lm_detector_add_class_packed(lm_detector* d, const char* class_id, int num_pyramids, const int32_t* features,
                                            const int32_t* tmpl_offsets, const int32_t* tmpl_wh) {
    if (!d || !class_id || num_pyramids < 0 || (num_pyramids && (!features || !tmpl_offsets || !tmpl_wh)))
        return lm_set_error(LM_ERR_INVALID, "bad argument");
    if (d->class_templates.count(class_id)) return lm_set_error(LM_ERR_INVALID, "class '%s' already present", class_id);
    const int E = d->pyramid_levels * d->nmod;
    std::vector<TemplatePyramid> tps((size_t)num_pyramids);
    for (int p = 0; p < num_pyramids; ++p) {
        TemplatePyramid& tp = tps[p];
        tp.resize(E);
        for (int e = 0; e < E; ++e) {
            size_t k = (size_t)p * E + e;
            Template& t = tp[e];
            t.width = tmpl_wh[2 * k]; t.height = tmpl_wh[2 * k + 1]; t.pyramid_level = e / d->nmod;
            int a = tmpl_offsets[k], b = tmpl_offsets[k + 1];
            if (a < 0 || b < a) return lm_set_error(LM_ERR_INVALID, "tmpl_offsets not monotone");
            t.features.resize((size_t)(b - a));
            for (int i = a; i < b; ++i) t.features[i - a] = Feature{features[3 * (size_t)i], features[3 * (size_t)i + 1], features[3 * (size_t)i + 2]};
        }
        int rc = validate_pyramid(d, tp);
        if (rc) return rc;
    }
    d->class_templates[class_id] = std::move(tps);
    d->bank_dirty = true;
    return LM_OK;
}

extern "C" int lm_detector_num_classes(const lm_detector* d) { return d ? (int)d->class_templates.size() : 0; }
extern "C" const char* lm_detector_class_id(const lm_detector* d, int index) {
    if (!d || index < 0 || index >= (int)d->class_templates.size()) return nullptr;
    auto it = d->class_templates.begin();
    std::advance(it, index);
    return it->first.c_str();
}
extern "C" int lm_detector_num_templates(const lm_detector* d, const char* class_id) {
    if (!d) return 0;
    if (!class_id) { int n = 0; for (auto& kv : d->class_templates) n += (int)kv.second.size(); return n; }
    auto it = d->class_templates.find(class_id);
    return it == d->class_templates.end() ? 0 : (int)it->second.size();
}
extern "C" int lm_detector_pyramid_levels(const lm_detector* d) { return d ? d->pyramid_levels : 0; }
extern "C" int lm_detector_get_T(const lm_detector* d, int level) {
    return (d && level >= 0 && level < d->pyramid_levels) ? d->T_at_level[level] : -1;
}

extern "C" int lm_detector_get_template(const lm_detector* d, const char* class_id, int template_id, int index, int32_t* width,
                                        int32_t* height, int32_t* pyramid_level, int32_t* num_features, int32_t* features,
                                        int capacity) {
    if (!d || !class_id) return lm_set_error(LM_ERR_INVALID, "null argument");
    auto it = d->class_templates.find(class_id);
    if (it == d->class_templates.end()) return lm_set_error(LM_ERR_NOT_FOUND, "unknown class '%s' [LL.cpp:1979]", class_id);
    if (template_id < 0 || (size_t)template_id >= it->second.size())
        return lm_set_error(LM_ERR_INVALID, "template_id out of range [LL.cpp:1980]");
    const TemplatePyramid& tp = it->second[template_id];
    if (index < 0 || index >= (int)tp.size()) return lm_set_error(LM_ERR_INVALID, "template index out of range");
    const Template& t = tp[index];
    if (width) *width = t.width;
    if (height) *height = t.height;
    if (pyramid_level) *pyramid_level = t.pyramid_level;
    if (num_features) *num_features = (int32_t)t.features.size();
    if (features)
        for (int i = 0; i < capacity && i < (int)t.features.size(); ++i) {
            features[3 * i] = t.features[i].x; features[3 * i + 1] = t.features[i].y; features[3 * i + 2] = t.features[i].label;
        }
    return LM_OK;
}

extern "C" int lm_detector_set_shard(lm_detector* d, int rank, int world) {
    if (!d || world < 1 || rank < 0 || rank >= world) return lm_set_error(LM_ERR_INVALID, "bad shard (%d of %d)", rank, world);
    if (int rc = lm_need_both(d, "lm_detector_set_shard")) return rc;
    if (world > 1 && d->refine_mode == 3) return lm_set_error(LM_ERR_INVALID, "the wide paths are not available on a sharded detector: lm_detector_set_paths first");
    if (world > 1 && d->part_min_parts > 0) return lm_set_error(LM_ERR_INVALID, "part matching is not available on a sharded detector (%d ranks)", world);
    d->shard_rank = rank; d->shard_world = world;
    return LM_OK;
}

// ---- part-based matching (match_parts.hip) ----------------------------------------------------------------------
// The part table of one template entry, on the host alone: feature i at (xs[i], ys[i]) belongs to part (2 x >= width) + 2 (2 y >= height); part p
// owns the slots [start[p], start[p] + npad[p]) of the part-ordered feature arrays, its n[p] features first in their original order, then
// padding up to a multiple of kFeatBatch; it is eligible iff n[p] >= min_part_features.  out16 = start[4], n[4], npad[4], eligible[4] (start
// counted from the entry's first slot); order (may be null; room for n + 28) = per slot the feature's index, -1 for padding.
extern "C" int lm_part_table(int width, int height, const int32_t* xs, const int32_t* ys, int n, int min_part_features, int32_t* out16, int32_t* order) {
    if (n < 0 || (n && (!xs || !ys)) || !out16) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (min_part_features < 1) return lm_set_error(LM_ERR_INVALID, "min_part_features must be at least 1, got %d", min_part_features);
    int cnt[4] = {0, 0, 0, 0};
    auto part_of = [&](int i) { return (2 * (long)xs[i] >= width ? 1 : 0) + (2 * (long)ys[i] >= height ? 2 : 0); };
    for (int i = 0; i < n; ++i) ++cnt[part_of(i)];
    int at = 0;
    for (int p = 0; p < 4; ++p) {
        const int npad = (cnt[p] + kFeatBatch - 1) / kFeatBatch * kFeatBatch;
        out16[p] = at; out16[4 + p] = cnt[p]; out16[8 + p] = npad; out16[12 + p] = cnt[p] >= min_part_features ? 1 : 0;
        if (order) {
            int w = at;
            for (int i = 0; i < n; ++i) if (part_of(i) == p) order[w++] = i;
            while (w < at + npad) order[w++] = -1;
        }
        at += npad;
    }
    return LM_OK;
}

extern "C" int lm_detector_set_part_matching(lm_detector* d, int min_parts, int min_part_features) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (min_parts < 0 || min_parts > 4) return lm_set_error(LM_ERR_INVALID, "min_parts must be 0 (off) or 1..4, got %d", min_parts);
    if (min_part_features < 1) return lm_set_error(LM_ERR_INVALID, "min_part_features must be at least 1, got %d", min_part_features);
    if (min_parts > 0 && d->shard_world > 1) return lm_set_error(LM_ERR_INVALID, "part matching is not available on a sharded detector (%d ranks)", d->shard_world);
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them before changing part matching");
    int rc = lm_launch_pending(d);
    if (rc) return rc;
    if ((min_parts > 0) != (d->part_min_parts > 0) || (min_parts > 0 && min_part_features != d->part_min_features)) d->bank_dirty = true;   // the part tables come and go with the bank's device image
    d->part_min_parts = min_parts; d->part_min_features = min_part_features;
    return LM_OK;
}
extern "C" int lm_detector_get_part_matching(const lm_detector* d, int* min_parts, int* min_part_features) {
    if (!d || !min_parts || !min_part_features) return lm_set_error(LM_ERR_INVALID, "null argument");
    *min_parts = d->part_min_parts; *min_part_features = d->part_min_features;
    return LM_OK;
}
int lm_parts_refused(const lm_detector* d, const char* what) {
    return d->part_min_parts > 0 ? lm_set_error(LM_ERR_INVALID, "%s is not available under part matching: lm_detector_set_part_matching(d, 0, .) first", what) : LM_OK;
}

static inline int floordiv(int a, int b) { int q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// Flatten the bank for the current frame geometry and upload it: TemplEntry per (pyramid, level);
// per feature the byte offset of its linear-memory run from the arena start (accessLinearMemory,
// LL.cpp:1248-1271; floor division so that window offsets that are multiples of T stay exact) and
// packed int16 x,y.  Entries are padded to a multiple of kFeatBatch with features that read the
// level's zero tail; at the top level features outside the image (LL.cpp:1330) are redirected there too.
int upload_bank(lm_detector* d) {
    const int L = d->pyramid_levels;
    d->bank_classes.clear(); d->bank_class_base.clear(); d->bank_class_count.clear();
    d->h_entries.clear();
    d->work_valid = false;
    std::vector<int32_t> off;
    std::vector<uint32_t> xy;
    std::vector<uint32_t> word, rmask;          // levels below the top: feat_word per feature, run_mask per 8 features (lm_kernels.h)
    const uint32_t pad_xy = 0x80008000u;   // x = y = -32768: never inside an image
    const bool with_parts = d->part_min_parts > 0;
    std::vector<PartEntry> ptab;                // part matching: the part table per entry and the part-ordered copies of off / word
    std::vector<int32_t> poff, pxs, pys, porder;
    std::vector<uint32_t> pword;
    int flat = 0;
    for (auto& kv : d->class_templates) {
        d->bank_classes.push_back(kv.first);
        d->bank_class_base.push_back(flat);
        d->bank_class_count.push_back((int)kv.second.size());
        for (const TemplatePyramid& tp : kv.second) {
            for (int l = 0; l < L; ++l) {
                const LevelGeom& lv = d->geom.lv[l];
                const long npos = (long)lv.Wd * lv.Hd;
                const long zero_off = (long)lv.lm_off[1] + (long)8 * lv.T * lv.T * npos;   // tail of the normal block
                const long splane = (long)lv.NS * lv.Hd * 16;
                const uint32_t szero = (uint32_t)((long)lv.sm_off[1] + (long)8 * lv.T * lv.T * splane);   // the all-zero strip plane
                TemplEntry e{};
                e.feat_start = (uint32_t)off.size();
                const int nm = d->nmod;           // templates of the level: tp[nm * l + i], i-th modality of the set (kind mod_kind[i])
                size_t nfeat = 0;
                for (int i = 0; i < nm; ++i) nfeat += tp[(size_t)nm * l + i].features.size();
                e.nf = (uint16_t)nfeat;           // the score's denominator: the features of the set's modalities (LL.cpp:1826-1831)
                e.width = tp[(size_t)nm * l].width;      // matchClass uses tp[start] (first modality) for the clamp,
                e.height = tp[(size_t)nm * l].height;    // similarity() each template's own size: checked equal below
                if (nm == 2 && (tp[2 * l + 1].width != e.width || tp[2 * l + 1].height != e.height))
                    return lm_set_error(LM_ERR_INVALID, "modalities of one pyramid level disagree on width/height");
                int mnx = 32767, mny = 32767, mxx = -32768, mxy = -32768;
                struct Rec { int32_t off; uint32_t xy; uint32_t base0; int cls; };
                std::vector<Rec> recs;
                const bool top = (l == L - 1);
                const long zero16 = (zero_off + 15) & ~15L;      // 16-aligned start of the zero tail
                for (int i = 0; i < nm; ++i)
                    for (const Feature& f : tp[(size_t)nm * l + i].features) {
                        const int T = lv.T, m = d->mod_kind[i];          // the feature reads its KIND's arena block
                        const int gx = f.x - floordiv(f.x, T) * T, gy = f.y - floordiv(f.y, T) * T;   // floor modulo
                        long o = (long)lv.lm_off[m] + ((long)f.label * T * T + (gy * T + gx)) * npos + (long)floordiv(f.y, T) * lv.Wd +
                                 floordiv(f.x, T);
                        const bool inside = f.x >= 0 && f.x < lv.W && f.y >= 0 && f.y < lv.H;
                        if (top && !inside) o = zero16;                                 // LL.cpp:1330
                        if (o < -(1L << 31) || o >= (1L << 31)) return lm_set_error(LM_ERR_INVALID, "feature offset overflow");
                        Rec r{};
                        r.off = (int32_t)o;
                        r.xy = (uint32_t)(uint16_t)(int16_t)f.x | ((uint32_t)(uint16_t)(int16_t)f.y << 16);
                        r.base0 = szero;
                        if (!top && f.x >= 0 && f.y >= 0) {   // only read on the fast path, where x, y >= 0: the 16-byte row of the feature's own cell
                            const long lx = f.x / T, ly = f.y / T;
                            r.base0 = (uint32_t)((long)lv.sm_off[m] + ((long)f.label * T * T + (gy * T + gx)) * splane + ((lx >> 4) * lv.Hd + ly) * 16);
                        }
                        // alignment class: byte phase of the run start (top level: flat offset; below: plane column)
                        r.cls = top ? (int)(o & 15) : (f.x >= 0 ? (f.x / T) & 15 : 0);
                        recs.push_back(r);
                        mnx = std::min(mnx, f.x); mny = std::min(mny, f.y); mxx = std::max(mxx, f.x); mxy = std::max(mxy, f.y);
                    }
                if (e.nf == 0) mnx = mny = mxx = mxy = 0;
                e.min_x = (int16_t)mnx; e.min_y = (int16_t)mny; e.max_x = (int16_t)mxx; e.max_y = (int16_t)mxy;
                if (with_parts) {                        // the features in their own order, part by part; padding reads zeros as in the holistic arrays
                    pxs.clear(); pys.clear();
                    for (int i = 0; i < nm; ++i)
                        for (const Feature& f : tp[(size_t)nm * l + i].features) { pxs.push_back(f.x); pys.push_back(f.y); }
                    porder.assign(recs.size() + 4 * kFeatBatch, -1);
                    int32_t t16[16];
                    if (int rc = lm_part_table(e.width, e.height, pxs.data(), pys.data(), (int)recs.size(), d->part_min_features, t16, porder.data())) return rc;
                    PartEntry pe{};
                    const uint32_t first = (uint32_t)poff.size();
                    for (int p = 0; p < 4; ++p) {
                        pe.start[p] = first + (uint32_t)t16[p]; pe.n[p] = (uint16_t)t16[4 + p]; pe.npad[p] = (uint16_t)t16[8 + p];
                        pe.eligible |= (uint32_t)t16[12 + p] << p;
                    }
                    const int slots = t16[3] + t16[11];
                    for (int k = 0; k < slots; ++k) {
                        const int i = porder[k];
                        poff.push_back(i >= 0 ? recs[i].off : (int32_t)zero16);
                        pword.push_back(i >= 0 ? ((recs[i].base0 & ~15u) | (uint32_t)recs[i].cls) : (szero & ~15u));
                    }
                    ptab.push_back(pe);
                }
                std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.cls < b.cls; });
                std::vector<uint8_t> starts;             // per feature of this entry: 1 = first of a class run
                auto push_feat = [&](int32_t o, uint32_t pxy, uint32_t base0, int cls, bool start) {
                    off.push_back(o); xy.push_back(pxy); word.push_back((base0 & ~15u) | (uint32_t)cls); starts.push_back(start ? 1 : 0);
                };
                auto push_pad = [&](int cls) {           // a feature that reads zeros, in alignment class `cls`
                    push_feat((int32_t)(zero16 + (top ? cls : 0)), pad_xy, szero, cls, false);
                };
                int last_cls = 0;
                for (size_t i = 0; i < recs.size();) {
                    size_t j = i;
                    while (j < recs.size() && recs[j].cls == recs[i].cls) ++j;
                    // a run: <= kRunMax (even) features of one class, so that the packed-byte sums of the refinement cannot overflow
                    for (size_t k = i; k < j; ++k) push_feat(recs[k].off, recs[k].xy, recs[k].base0, recs[k].cls, (k - i) % kRunMax == 0);
                    last_cls = recs[i].cls;
                    if (!top && ((j - i) & 1)) push_pad(last_cls);   // the refinement consumes features in same-class pairs
                    i = j;
                }
                while ((off.size() - e.feat_start) % kFeatBatch) push_pad(last_cls);
                e.nf_padded = (uint16_t)(off.size() - e.feat_start);
                for (size_t k = 0; k < starts.size(); k += kFeatBatch) {           // kFeatBatch == 8: one mask word per batch
                    uint32_t mk = 0;
                    for (int u = 0; u < kFeatBatch; ++u) mk |= (uint32_t)starts[k + u] << u;
                    rmask.push_back(mk);
                }
                d->h_entries.push_back(e);
            }
            ++flat;
        }
    }
    int rc;
    if ((rc = d->d_entries.ensure(std::max<size_t>(1, d->h_entries.size())))) return rc;
    if ((rc = d->d_feat_off.ensure(std::max<size_t>(1, off.size())))) return rc;
    if ((rc = d->d_feat_xy.ensure(std::max<size_t>(1, xy.size())))) return rc;
    if ((rc = d->d_feat_word.ensure(std::max<size_t>(1, word.size())))) return rc;
    if ((rc = d->d_run_mask.ensure(std::max<size_t>(1, rmask.size())))) return rc;
    if (!d->h_entries.empty())
        HIP_TRY(hipMemcpy(d->d_entries.p, d->h_entries.data(), d->h_entries.size() * sizeof(TemplEntry), hipMemcpyHostToDevice));
    if (!off.empty()) {
        HIP_TRY(hipMemcpy(d->d_feat_off.p, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->d_feat_xy.p, xy.data(), xy.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->d_feat_word.p, word.data(), word.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->d_run_mask.p, rmask.data(), rmask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (with_parts) {
        if ((rc = d->d_parts.ensure(std::max<size_t>(1, ptab.size()))) || (rc = d->d_part_off.ensure(std::max<size_t>(1, poff.size()))) ||
            (rc = d->d_part_word.ensure(std::max<size_t>(1, pword.size())))) return rc;
        if (!ptab.empty()) HIP_TRY(hipMemcpy(d->d_parts.p, ptab.data(), ptab.size() * sizeof(PartEntry), hipMemcpyHostToDevice));
        if (!poff.empty()) {
            HIP_TRY(hipMemcpy(d->d_part_off.p, poff.data(), poff.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d->d_part_word.p, pword.data(), pword.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    // counter widths of the bit-plane kernels: the largest entry at the top level (k_coarse_bits) and below it (k_local_bits)
    d->bits_max_nf = 0; d->cbits_max_nf = 0;
    for (size_t i = 0; i < d->h_entries.size(); ++i) {
        int& mx = (int)(i % (size_t)L) == L - 1 ? d->cbits_max_nf : d->bits_max_nf;
        mx = std::max(mx, (int)d->h_entries[i].nf);
    }
    // Does EVERY candidate of this bank have its windows inside their planes at every level below the top (k_local's `all_in`)?  The
    // refinement clamps the window origin to x in [8T, W - width - 8T] (LL.cpp:1871-1880), so with that interval non-empty, gx = x / T - 8 >= 0
    // and (max_x + gx T) / T + 16 <= (max_x + W - width - 16 T) / T + 16 <= W / T whenever max_x <= width (W is a multiple of T); the same in
    // y.  Then k_local_bits leaves nothing for k_local's per-candidate path and the second launch is skipped.
    d->bits_all_in = true;
    for (size_t i = 0; i < d->h_entries.size(); ++i) {
        const int l = (int)(i % (size_t)L);
        if (l == L - 1) continue;
        const LevelGeom& lv = d->geom.lv[l];
        const TemplEntry& e = d->h_entries[i];
        d->bits_all_in = d->bits_all_in && e.min_x >= 0 && e.min_y >= 0 && e.max_x <= e.width && e.max_y <= e.height &&
                         lv.W - e.width - 16 * lv.T >= 0 && lv.H - e.height - 16 * lv.T >= 0 && lv.W % lv.T == 0 && lv.H % lv.T == 0;
    }
    d->bank_dirty = false;
    ++d->bank_generation;
    d->bank_geom_W = d->fW; d->bank_geom_H = d->fH;
    return LM_OK;
}

int build_work(lm_detector* d, const char* const* class_ids, int num_class_ids) {
    std::vector<std::string> key;
    if (class_ids && num_class_ids > 0)
        for (int i = 0; i < num_class_ids; ++i) key.push_back(class_ids[i] ? class_ids[i] : "");
    if (d->work_valid && key == d->work_key && d->work_key_rank == d->shard_rank && d->work_key_world == d->shard_world)
        return LM_OK;   // same selection as the previous call: the device-resident work list is reused
    d->work_pyr.clear();
    d->work_cls = std::make_shared<std::vector<int32_t>>();    // in-flight slots keep the old vectors alive
    d->work_tid = std::make_shared<std::vector<int32_t>>();
    std::vector<int> order;   // bank class index per position (-1 unknown)
    if (key.empty()) {
        for (size_t i = 0; i < d->bank_classes.size(); ++i) order.push_back((int)i);   // std::map order, LL.cpp:1756
    } else {
        for (const std::string& c : key) {
            int found = -1;
            for (size_t k = 0; k < d->bank_classes.size(); ++k)
                if (d->bank_classes[k] == c) { found = (int)k; break; }
            order.push_back(found);   // unknown classes are skipped, LL.cpp:1765-1767
        }
    }
    for (size_t pos = 0; pos < order.size(); ++pos) {
        int k = order[pos];
        if (k < 0) continue;
        for (int t = 0; t < d->bank_class_count[k]; ++t) {
            d->work_pyr.push_back(d->bank_class_base[k] + t);
            d->work_cls->push_back((int)pos);
            d->work_tid->push_back(t);
        }
    }
    // contiguous shard of the work list; template ids stay global
    const long N = (long)d->work_pyr.size();
    const long a = N * d->shard_rank / d->shard_world, b = N * (d->shard_rank + 1) / d->shard_world;
    if (d->shard_world > 1) {
        d->work_pyr = std::vector<int32_t>(d->work_pyr.begin() + a, d->work_pyr.begin() + b);
        *d->work_cls = std::vector<int32_t>(d->work_cls->begin() + a, d->work_cls->begin() + b);
        *d->work_tid = std::vector<int32_t>(d->work_tid->begin() + a, d->work_tid->begin() + b);
    }
    // frames in flight still read the device-resident work list: let them finish before it is replaced
    if (d->n_submitted != d->n_collected) {
        HIP_TRY(hipStreamSynchronize(d->mstream));
        if (d->xchg_stream) HIP_TRY(hipStreamSynchronize(d->xchg_stream));
    }
    int rc = d->d_work.ensure(std::max<size_t>(1, d->work_pyr.size()));
    if (rc) return rc;
    if ((rc = d->d_work_cls.ensure(std::max<size_t>(1, d->work_pyr.size())))) return rc;
    if ((rc = d->d_work_tid.ensure(std::max<size_t>(1, d->work_pyr.size())))) return rc;
    if (!d->work_pyr.empty()) {
        HIP_TRY(hipMemcpy(d->d_work.p, d->work_pyr.data(), d->work_pyr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->d_work_cls.p, d->work_cls->data(), d->work_pyr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->d_work_tid.p, d->work_tid->data(), d->work_pyr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // algorithmic bytes of the coarse pass over this work list: sum_m nfeat_m * template_positions
    {
        const int L = d->pyramid_levels;
        const LevelGeom& lv = d->geom.lv[L - 1];
        int64_t bytes = 0;
        for (int32_t p : d->work_pyr) {
            const TemplEntry& e = d->h_entries[(size_t)p * L + (L - 1)];
            int wf = (e.width - 1) / lv.T + 1, hf = (e.height - 1) / lv.T + 1;
            long tp = (long)(lv.Hd - hf) * lv.Wd + (lv.Wd - wf) + 1;
            if (tp > 0) bytes += (int64_t)e.nf * tp;
        }
        d->work_coarse_bytes = bytes;
    }
    d->work_key = key; d->work_key_rank = d->shard_rank; d->work_key_world = d->shard_world;
    d->work_valid = true;
    return LM_OK;
}
