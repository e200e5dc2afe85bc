// Depth-scaled matching (the reference author's "at each matching pos, scale template depth to scene depth",
// linemodLevelup/notes.md:1-2, 25-31): the training depth of a class (lm_detector_set_class_train_depth), the scaled features of one entry on
// the host (lm_scaled_features) and the match of the RESIDENT frame with every template scaled, per position, by the ladder entry nearest to
// d_train / d of the probed scene depth d (lm_detector_match_scaled).  Kernels: match_scaled.hip; the byte linear memories are the front end's
// own (lm_byte_memories_resident).  The rule is stated in tests/scaled_match_ref.py.
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "detector_internal.h"

static inline int floordiv(int a, int b) { int q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// c + sign(v - c) * ((|v - c| * s + 512) >> 10): a coordinate scaled about the centre c by the Q10 factor s, half away from the centre
static inline int scale_about(int v, int c, int s) {
    const long long dv = (long long)v - c, a = dv < 0 ? -dv : dv, r = (a * s + 512) >> 10;
    return (int)(c + (dv < 0 ? -r : r));
}

extern "C" int lm_scaled_features(int width, int height, const int32_t* xs, const int32_t* ys, int n, int scale_q10, int32_t* out_xs, int32_t* out_ys) {
    if (n < 0 || (n && (!xs || !ys || !out_xs || !out_ys))) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (scale_q10 < 512 || scale_q10 > 2048) return lm_set_error(LM_ERR_INVALID, "scale_q10 must be in [512, 2048], got %d", scale_q10);
    const int cx = floordiv(width, 2), cy = floordiv(height, 2);
    for (int i = 0; i < n; ++i) { out_xs[i] = scale_about(xs[i], cx, scale_q10); out_ys[i] = scale_about(ys[i], cy, scale_q10); }
    return LM_OK;
}

extern "C" void lm_scaled_options_init(lm_scaled_options* o) {
    if (!o) return;
    static const int32_t ladder[9] = {512, 609, 724, 861, 1024, 1218, 1448, 1722, 2048};    // round(1024 * 2^(i / 4 - 1))
    memset(o, 0, sizeof(*o));
    o->num_scales = 9;
    memcpy(o->scales_q10, ladder, sizeof(ladder));
    o->min_scale_q10 = o->max_scale_q10 = 0;
    o->probe = 2;
}

extern "C" int lm_detector_set_class_train_depth(lm_detector* d, const char* class_id, int depth_mm) {
    if (!d || !class_id) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!d->class_templates.count(class_id)) return lm_set_error(LM_ERR_NOT_FOUND, "unknown class '%s'", class_id);
    if (depth_mm < 1 || depth_mm > 65535) return lm_set_error(LM_ERR_INVALID, "training depth of class '%s' must be in 1..65535 mm, got %d", class_id, depth_mm);
    d->class_train_depth[class_id] = depth_mm;
    return LM_OK;
}

extern "C" int lm_detector_get_class_train_depth(const lm_detector* d, const char* class_id, int* depth_mm) {
    if (!d || !class_id || !depth_mm) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!d->class_templates.count(class_id)) return lm_set_error(LM_ERR_NOT_FOUND, "unknown class '%s'", class_id);
    const auto it = d->class_train_depth.find(class_id);
    if (it == d->class_train_depth.end()) return 0;
    *depth_mm = it->second;
    return 1;
}

static int scaled_options(const lm_scaled_options* in, ScaledLadder* lad, int* probe) {
    lm_scaled_options o;
    if (in) o = *in; else lm_scaled_options_init(&o);
    if (o.num_scales < 1 || o.num_scales > kScaledMaxLadder)
        return lm_set_error(LM_ERR_INVALID, "scaled matching: the ladder has 1..%d scales, got %d", kScaledMaxLadder, o.num_scales);
    for (int k = 0; k < o.num_scales; ++k) {
        if (o.scales_q10[k] < 512 || o.scales_q10[k] > 2048)
            return lm_set_error(LM_ERR_INVALID, "scaled matching: scale %d of the ladder is %d, outside [512, 2048] (Q10: 0.5 .. 2)", k, o.scales_q10[k]);
        if (k && o.scales_q10[k] <= o.scales_q10[k - 1])
            return lm_set_error(LM_ERR_INVALID, "scaled matching: the ladder must be strictly ascending, scale %d is %d after %d", k, o.scales_q10[k], o.scales_q10[k - 1]);
    }
    const int lo = o.min_scale_q10 ? o.min_scale_q10 : o.scales_q10[0], hi = o.max_scale_q10 ? o.max_scale_q10 : o.scales_q10[o.num_scales - 1];
    if (lo < 1 || hi > (1 << 20) || lo > hi)
        return lm_set_error(LM_ERR_INVALID, "scaled matching: bad scale bounds: 1 <= min_scale_q10 <= max_scale_q10 <= 1048576 wanted, got %d and %d", lo, hi);
    if (o.probe < 0 || o.probe > kScaledMaxProbe) return lm_set_error(LM_ERR_INVALID, "scaled matching: probe must be in 0..%d, got %d", kScaledMaxProbe, o.probe);
    lad->K = o.num_scales; lad->lo = lo; lad->hi = hi;
    for (int k = 0; k < kScaledMaxLadder; ++k) lad->s[k] = k < o.num_scales ? o.scales_q10[k] : 0;
    *probe = o.probe;
    return LM_OK;
}

// The K-row tables of the work list (build_work) for the current geometry: per (work item, level) nf x K elements, the K ladder entries of a
// feature side by side.  Kept while the bank generation, the ladder and the selection stay what they were.
static int scaled_tables(lm_detector* d, const ScaledLadder& lad) {
    lm_detector::Scaled& S = d->scaled;
    const std::vector<int32_t> ladder(lad.s, lad.s + lad.K);
    if (S.table_valid && S.key_generation == d->bank_generation && S.key_ladder == ladder && S.key_classes == d->work_key) return LM_OK;
    S.table_valid = false;
    const int L = d->pyramid_levels, nm = d->nmod, K = lad.K;
    std::vector<const TemplatePyramid*> flat;                            // flat pyramid index -> pyramid, the order of upload_bank
    for (const auto& kv : d->class_templates)
        for (const TemplatePyramid& tp : kv.second) flat.push_back(&tp);
    std::vector<ScaledEntry> entries;
    std::vector<ScaledFeat> table;
    S.max_nf_top = 0;
    for (int32_t p : d->work_pyr) {
        const TemplatePyramid& tp = *flat[(size_t)p];
        for (int l = 0; l < L; ++l) {
            const LevelGeom& lv = d->geom.lv[l];
            const TemplEntry& te = d->h_entries[(size_t)p * L + l];
            ScaledEntry e{};
            e.tab = (uint32_t)table.size(); e.nf = te.nf; e.width = te.width; e.height = te.height;
            if (table.size() + (size_t)te.nf * K > 0x7FFFFFFFull) return lm_set_error(LM_ERR_INVALID, "scaled matching: the tables of this selection exceed 2^31 elements");
            const int cx = floordiv(te.width, 2), cy = floordiv(te.height, 2);
            const long long npos = (long long)lv.Wd * lv.Hd;
            for (int i = 0; i < nm; ++i)
                for (const Feature& f : tp[(size_t)nm * l + i].features) {
                    if (f.label < 0 || f.label > 7) return lm_set_error(LM_ERR_INVALID, "scaled matching: a feature has label %d", f.label);
                    for (int k = 0; k < K; ++k) {
                        const int sx = scale_about(f.x, cx, lad.s[k]), sy = scale_about(f.y, cy, lad.s[k]);
                        const int cdx = floordiv(sx, lv.T), cdy = floordiv(sy, lv.T);
                        if (cdx < -32768 || cdx > 32767 || cdy < -32768 || cdy > 32767) return lm_set_error(LM_ERR_INVALID, "scaled matching: a scaled feature lies %d, %d cells from its template's origin", cdx, cdy);
                        const long long base = (long long)lv.lm_off[d->mod_kind[i]] + ((long long)f.label * lv.T * lv.T + (long long)(sy - cdy * lv.T) * lv.T + (sx - cdx * lv.T)) * npos;
                        if (base < 0 || base + npos > 0xFFFFFFFFll) return lm_set_error(LM_ERR_INVALID, "scaled matching: a linear memory lies beyond 4 GB of the arena");
                        ScaledFeat sf;
                        sf.base = (uint32_t)base;
                        sf.cdx = (int16_t)cdx; sf.cdy = (int16_t)cdy;
                        table.push_back(sf);
                    }
                }
            if (l == L - 1) S.max_nf_top = std::max(S.max_nf_top, (int)te.nf);
            entries.push_back(e);
        }
    }
    int rc;
    if ((rc = S.entries.ensure(std::max<size_t>(1, entries.size()))) || (rc = S.table.ensure(std::max<size_t>(1, table.size())))) return rc;
    if (!entries.empty()) HIP_TRY(hipMemcpy(S.entries.p, entries.data(), entries.size() * sizeof(ScaledEntry), hipMemcpyHostToDevice));
    if (!table.empty()) HIP_TRY(hipMemcpy(S.table.p, table.data(), table.size() * sizeof(ScaledFeat), hipMemcpyHostToDevice));
    S.key_generation = d->bank_generation; S.key_ladder = ladder; S.key_classes = d->work_key;
    S.table_valid = true;
    return LM_OK;
}

extern "C" int lm_detector_match_scaled(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids, const lm_scaled_options* options,
                                        lm_scaled_match** out, size_t* n) {
    if (!d || !out || !n) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr; *n = 0;
    // nothing is matched unscaled in silence: what this call cannot serve is refused
    if (!d->use[1]) return lm_set_error(LM_ERR_INVALID, "lm_detector_match_scaled needs the DepthNormal modality: this detector has no depth image");
    if (d->shard_world > 1) return lm_set_error(LM_ERR_INVALID, "lm_detector_match_scaled is not available on a sharded detector (%d ranks)", d->shard_world);
    int rc;
    if ((rc = lm_parts_refused(d, "lm_detector_match_scaled"))) return rc;
    if (d->pipelines > 0) return lm_set_error(LM_ERR_INVALID, "lm_detector_match_scaled is not available on a detector that serves a pipeline (lm_pipeline_destroy first)");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    if (!d->frame_valid || !d->cur_depth) return lm_set_error(LM_ERR_INVALID, "no frame resident: call lm_detector_set_frame / select_frame first");
    ScaledLadder lad{};
    int probe = 0;
    if ((rc = scaled_options(options, &lad, &probe))) return rc;
    std::vector<std::string> names;                          // the requested classes; unknown ones are skipped (LL.cpp:1765-1767)
    if (class_ids && num_class_ids > 0)
        for (int i = 0; i < num_class_ids; ++i) names.push_back(class_ids[i] ? class_ids[i] : "");
    else
        for (const auto& kv : d->class_templates) names.push_back(kv.first);
    for (const std::string& c : names)
        if (d->class_templates.count(c) && !d->class_train_depth.count(c))
            return lm_set_error(LM_ERR_INVALID, "class '%s' has no training depth: lm_detector_set_class_train_depth first", c.c_str());
    HIP_TRY(hipSetDevice(d->device));
    if ((rc = lm_launch_pending(d))) return rc;
    if ((d->bank_dirty || d->bank_geom_W != d->fW || d->bank_geom_H != d->fH) && (rc = upload_bank(d))) return rc;
    if ((rc = build_work(d, class_ids, num_class_ids))) return rc;
    const int num_work = (int)d->work_pyr.size(), L = d->pyramid_levels;
    lm_scaled_match* res = (lm_scaled_match*)malloc(sizeof(lm_scaled_match));
    if (!res) return lm_set_error(LM_ERR_INVALID, "out of host memory");
    *out = res;
    if (num_work == 0) return LM_OK;
    auto fail = [&](int code) { free(*out); *out = nullptr; *n = 0; return code; };
    lm_detector::Scaled& S = d->scaled;
    if ((rc = scaled_tables(d, lad))) return fail(rc);
    const size_t lds = (size_t)lad.K * S.max_nf_top * sizeof(ScaledFeat);
    if (lds > kScaledMaxLds)
        return fail(lm_set_error(LM_ERR_INVALID, "scaled matching: %d scales x %d features x 8 bytes = %zu bytes do not fit the %zu bytes of LDS: shorten the ladder",
                                 lad.K, S.max_nf_top, lds, kScaledMaxLds));
    std::vector<int32_t> train((size_t)num_work);
    for (int w = 0; w < num_work; ++w) train[(size_t)w] = d->class_train_depth[names[(size_t)(*d->work_cls)[(size_t)w]]];
    if ((rc = S.train.ensure((size_t)num_work)) || (rc = S.probe.ensure((size_t)d->fW * d->fH)) || (rc = S.counter.ensure(4))) return fail(rc);
    hipStream_t s = d->stream;
    int arena = 0;
    if ((rc = lm_byte_memories_resident(d, &arena))) return fail(rc);
    auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? LM_OK : lm_set_error(LM_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
    if ((rc = hip(hipMemcpyAsync(S.train.p, train.data(), train.size() * sizeof(int32_t), hipMemcpyHostToDevice, s), "hipMemcpyAsync"))) return fail(rc);
    if ((rc = hip(launch_depth_probe(d->cur_depth, d->fW, d->fH, probe, S.probe.p, s), "k_depth_probe"))) return fail(rc);
    S.cap = std::max(S.cap, d->cand_cap);
    uint32_t ncand = 0;
    for (;;) {                                               // one pass normally; grow and rerun when the candidates overflowed
        if ((rc = S.cands.ensure(S.cap))) return fail(rc);
        if ((rc = hip(hipMemsetAsync(S.counter.p, 0, 4 * sizeof(unsigned int), s), "hipMemsetAsync"))) return fail(rc);
        if ((rc = hip(launch_coarse_scaled(d->lm_arena[arena].p, S.probe.p, d->fW, d->fH, d->geom.lv[L - 1], L, S.entries.p, S.table.p, lad, S.train.p, num_work,
                                           threshold, S.cands.p, S.counter.p, S.cap, lds, s), "k_coarse_scaled"))) return fail(rc);
        unsigned int produced = 0;
        if ((rc = hip(hipMemcpyAsync(&produced, S.counter.p, sizeof(produced), hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) ||
            (rc = hip(hipStreamSynchronize(s), "hipStreamSynchronize"))) return fail(rc);
        if (produced > S.cap) {                              // never drop candidates
            uint32_t cap = std::max<uint32_t>(S.cap, 1u);
            while (cap < produced && cap < 0x80000000u) cap <<= 1;
            if (cap < produced) return fail(lm_set_error(LM_ERR_INVALID, "scaled matching: %u candidates", produced));
            S.cap = cap;
            continue;
        }
        ncand = produced;
        break;
    }
    for (int l = L - 2; l >= 0; --l)
        if ((rc = hip(launch_local_scaled(d->lm_arena[arena].p, d->geom.lv[l], l, L, S.entries.p, S.table.p, lad.K, threshold, S.cands.p, ncand, s), "k_local_scaled")))
            return fail(rc);
    std::vector<ScaledCand> recs(ncand);
    if (ncand && (rc = hip(hipMemcpyAsync(recs.data(), S.cands.p, (size_t)ncand * sizeof(ScaledCand), hipMemcpyDeviceToHost, s), "hipMemcpyAsync"))) return fail(rc);
    if ((rc = hip(hipStreamSynchronize(s), "hipStreamSynchronize"))) return fail(rc);
    std::vector<lm_scaled_match> list;
    list.reserve(ncand);
    for (const ScaledCand& c : recs) {
        if (c.work < 0) continue;                            // dropped below the threshold during refinement
        lm_scaled_match m;
        m.x = c.x; m.y = c.y; m.similarity = c.score; m.class_index = (*d->work_cls)[(size_t)c.work]; m.template_id = (*d->work_tid)[(size_t)c.work];
        m.scale_index = c.k; m.depth_mm = c.depth;
        list.push_back(m);
    }
    // similarity descending, then class_index, template_id, y, x, scale_index (and depth_mm, so that the order is total) ascending
    auto key = [](const lm_scaled_match& m) { return std::make_tuple(-m.similarity, m.class_index, m.template_id, m.y, m.x, m.scale_index, m.depth_mm); };
    std::sort(list.begin(), list.end(), [&](const lm_scaled_match& a, const lm_scaled_match& b) { return key(a) < key(b); });
    list.erase(std::unique(list.begin(), list.end(), [&](const lm_scaled_match& a, const lm_scaled_match& b) { return key(a) == key(b); }), list.end());
    if (!list.empty()) {
        res = (lm_scaled_match*)realloc(*out, list.size() * sizeof(lm_scaled_match));
        if (!res) return fail(lm_set_error(LM_ERR_INVALID, "out of host memory"));
        memcpy(res, list.data(), list.size() * sizeof(lm_scaled_match));
        *out = res;
    }
    *n = list.size();
    return LM_OK;
}
