// Depth slabs (the reference's "use depth histogram and 1D nms to find some primary scales", linemodLevelup/readme.md:29-34):
// the primary depths of the resident frame (lm_detector_depth_modes), the depth range a class's templates are valid at
// (lm_detector_set_class_depth_range) and the match that runs every class under the slabs of the primary depths inside its range
// (lm_detector_match_slabs).  Kernels: depth_modes.hip; the passes are ordinary lone frames of detector_launch.cpp.
#include <stdlib.h>
#include <string.h>

#include "detector_internal.h"

static int mode_options(const lm_depth_mode_options* in, lm_depth_mode_options* o, int* nbins) {
    lm_depth_mode_options def;
    lm_depth_mode_options_init(&def);
    *o = in ? *in : def;
    if (o->bin_mm < 1) return lm_set_error(LM_ERR_INVALID, "depth modes: bin_mm must be at least 1, got %d", o->bin_mm);
    if (o->near_mm < 1) return lm_set_error(LM_ERR_INVALID, "depth modes: near_mm must be at least 1 (depth 0 is no measurement), got %d", o->near_mm);
    if (o->far_mm > 65536) return lm_set_error(LM_ERR_INVALID, "depth modes: far_mm must be at most 65536, got %d", o->far_mm);
    if (o->window < 0) return lm_set_error(LM_ERR_INVALID, "depth modes: window must not be negative, got %d", o->window);
    if (o->max_modes < 1 || o->max_modes > kDepthMaxModes) return lm_set_error(LM_ERR_INVALID, "depth modes: max_modes must be in 1..%d, got %d", kDepthMaxModes, o->max_modes);
    if (o->min_pixels < 1) return lm_set_error(LM_ERR_INVALID, "depth modes: min_pixels must be at least 1, got %d", o->min_pixels);
    const long long span = (long long)o->far_mm - o->near_mm;
    const long long nb = span > 0 ? (span + o->bin_mm - 1) / o->bin_mm : 0;
    if (nb < 1 || nb > kDepthMaxBins)
        return lm_set_error(LM_ERR_INVALID, "depth modes: nbins = ceil((far_mm - near_mm) / bin_mm) must be in 1..%d, got %lld", kDepthMaxBins, nb);
    *nbins = (int)nb;
    return LM_OK;
}

static int depth_frame_ready(lm_detector* d, const char* what) {
    if (!d->use[1]) return lm_set_error(LM_ERR_INVALID, "%s needs the DepthNormal modality: this detector has no depth image", what);
    if (!d->frame_valid || !d->cur_depth) return lm_set_error(LM_ERR_INVALID, "no frame resident: call lm_detector_set_frame / select_frame first");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    return LM_OK;
}

// Histogram, NMS + selection and the copy of the mode records to pinned memory, all on the frame stream; modes_ready marks the copy.
static int enqueue_modes(lm_detector* d, const lm_depth_mode_options& o, int nbins) {
    lm_detector::Slabs& S = d->slabs;
    int rc;
    if ((rc = S.hist.ensure(kDepthMaxBins)) || (rc = S.modes.ensure(kDepthModeWords))) return rc;
    if ((rc = S.h_modes.ensure(kDepthModeWords))) return rc;
    if ((rc = S.modes_ready.ensure(hipEventDisableTiming))) return rc;
    HIP_TRY(hipMemsetAsync(S.hist.p, 0, (size_t)nbins * sizeof(uint32_t), d->stream));
    DepthHistArgs a{};
    a.depth = d->cur_depth; a.W = d->fW; a.H = d->fH; a.pitch = d->fW;
    a.near_mm = o.near_mm; a.far_mm = o.far_mm; a.bin_mm = o.bin_mm; a.nbins = nbins;
    a.m_bin = o.bin_mm == 1 ? 0u : (uint32_t)(((1ull << 32) + (uint32_t)o.bin_mm - 1) / (uint32_t)o.bin_mm);
    a.hist = S.hist.p;
    HIP_TRY(launch_depth_hist(a, d->stream));
    HIP_TRY(launch_depth_nms(S.hist.p, nbins, o.near_mm, o.bin_mm, o.window, (uint32_t)o.min_pixels, o.max_modes, S.modes.p, d->stream));
    HIP_TRY(hipMemcpyAsync(S.h_modes.p, S.modes.p, kDepthModeWords * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipEventRecord(S.modes_ready, d->stream));
    return LM_OK;
}

static int wait_modes(lm_detector* d, int max_modes, lm_depth_mode* out, int* n) {
    HIP_TRY(hipEventSynchronize(d->slabs.modes_ready));
    const uint32_t* w = d->slabs.h_modes.p;
    *n = (int)std::min<uint32_t>(w[0], (uint32_t)max_modes);
    for (int k = 0; k < *n; ++k) { out[k].bin = (int32_t)w[4 + 3 * k]; out[k].depth_mm = (int32_t)w[5 + 3 * k]; out[k].pixels = w[6 + 3 * k]; }
    return LM_OK;
}

extern "C" void lm_depth_mode_options_init(lm_depth_mode_options* o) {
    if (!o) return;
    o->bin_mm = 25; o->near_mm = 300; o->far_mm = 4000; o->window = 2; o->min_pixels = 1000; o->max_modes = 8;
}

extern "C" int lm_detector_depth_modes(lm_detector* d, const lm_depth_mode_options* options, lm_depth_mode* out, int capacity, int* n) {
    if (!d || !out || !n) return lm_set_error(LM_ERR_INVALID, "null argument");
    *n = 0;
    lm_depth_mode_options o;
    int nbins = 0, rc;
    if ((rc = mode_options(options, &o, &nbins))) return rc;
    if (capacity < o.max_modes) return lm_set_error(LM_ERR_INVALID, "depth modes: room for %d records, max_modes is %d", capacity, o.max_modes);
    if ((rc = depth_frame_ready(d, "lm_detector_depth_modes"))) return rc;
    HIP_TRY(hipSetDevice(d->device));
    if ((rc = enqueue_modes(d, o, nbins))) return rc;
    return wait_modes(d, o.max_modes, out, n);
}

extern "C" int lm_detector_set_class_depth_range(lm_detector* d, const char* class_id, int lo_mm, int hi_mm, int clear) {
    if (!d || !class_id) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!d->class_templates.count(class_id)) return lm_set_error(LM_ERR_NOT_FOUND, "unknown class '%s'", class_id);
    if (clear) { d->class_depth_range.erase(class_id); return LM_OK; }
    if (lo_mm > hi_mm) return lm_set_error(LM_ERR_INVALID, "depth range of class '%s': lo_mm %d is above hi_mm %d", class_id, lo_mm, hi_mm);
    d->class_depth_range[class_id] = {lo_mm, hi_mm};
    return LM_OK;
}

extern "C" int lm_detector_get_class_depth_range(const lm_detector* d, const char* class_id, int* lo_mm, int* hi_mm) {
    if (!d || !class_id || !lo_mm || !hi_mm) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (!d->class_templates.count(class_id)) return lm_set_error(LM_ERR_NOT_FOUND, "unknown class '%s'", class_id);
    const auto it = d->class_depth_range.find(class_id);
    if (it == d->class_depth_range.end()) return 0;
    *lo_mm = it->second.first; *hi_mm = it->second.second;
    return 1;
}

// The slab of [lo, hi] at every pyramid level, on the frame stream: k_slab_mask writes level 0 — per modality of the set the slab ANDed
// with the user's mask of that modality, or one slab for the modalities without —, the masks' nearest-neighbour pyramid (resize(INTER_NEAREST),
// LL.cpp:573-578, 874-879) follows, one launch per level.  mask_of[][] then names what the front end's writers read.
static int write_slab_masks(lm_detector* d, int lo, int hi) {
    lm_detector::Slabs& S = d->slabs;
    const int L = d->pyramid_levels;
    int rc, which[2] = {-1, -1};                             // buffer of each kind: its own (user mask given) or the shared slab, 2
    SlabMaskArgs a{};
    a.depth = d->cur_depth; a.n = (uint32_t)((size_t)d->fW * d->fH); a.lo = lo; a.hi = hi;
    int buf[3] = {-1, -1, -1};                               // the buffer each output of the launch goes to
    bool shared = false;
    for (int i = 0; i < d->nmod; ++i) {
        const int m = d->mod_kind[i];
        const bool own = d->have_mask[m];
        which[m] = own ? m : 2;
        if (!own && shared) continue;                        // the second modality without a mask reads the same slab
        if (!own) shared = true;
        for (int l = 0; l < L; ++l)
            if ((rc = S.mask[l][which[m]].ensure((size_t)d->lvl[l].W * d->lvl[l].H))) return rc;
        a.user[a.n_out] = own ? d->lvl[0].mask[m].p : nullptr;
        a.out[a.n_out] = S.mask[0][which[m]].p;
        buf[a.n_out++] = which[m];
    }
    HIP_TRY(launch_slab_mask(a, d->stream));
    for (int l = 1; l < L; ++l) {
        FeStage st{};
        for (int o = 0; o < a.n_out; ++o)
            fe_job_nn_down2(st.job[st.njobs++], S.mask[l - 1][buf[o]].p, S.mask[l][buf[o]].p, d->lvl[l - 1].W, d->lvl[l - 1].H);
        HIP_TRY(launch_fe_stage(st, d->stream));
    }
    for (int l = 0; l < L; ++l)
        for (int m = 0; m < 2; ++m) S.mask_of[l][m] = which[m] >= 0 ? S.mask[l][which[m]].p : nullptr;
    return LM_OK;
}

// One pass: the classes at `positions` of the requested list as a lone frame (grow-and-rerun on an overflow, as lm_detector_match_resident),
// its distinct records appended to `all` with class_index = the position in the requested list.  *pre_merge: the records alive before any merge.
static int run_pass(lm_detector* d, float threshold, const std::vector<std::string>& names, const std::vector<int>& positions,
                    std::vector<lm_match>& all, int64_t* pre_merge) {
    std::vector<const char*> ids;
    for (int p : positions) ids.push_back(names[p].c_str());
    lm_match* recs = nullptr;
    size_t n = 0;
    for (;;) {
        int rc = lm_submit_frame(d, threshold, ids.data(), (int)ids.size());
        if (rc) return rc;
        rc = lm_collect_frame(d, 2, &recs, &n);
        if (rc != 1) { if (rc) return rc; break; }
    }
    *pre_merge = d->timings.matches_pre_unique;
    for (size_t i = 0; i < n; ++i) {
        lm_match m = recs[i];
        m.class_index = positions[m.class_index];
        all.push_back(m);
    }
    free(recs);
    return LM_OK;
}

extern "C" int lm_detector_match_slabs(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids, int slab_mm,
                                       const lm_depth_mode_options* options, lm_match** out, size_t* n, lm_slab* slabs, int slab_capacity,
                                       int* num_slabs, int32_t** slab_classes) {
    if (!d || !out || !n || !slabs || !num_slabs || !slab_classes) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr; *n = 0; *num_slabs = 0; *slab_classes = nullptr;
    lm_depth_mode_options o;
    int nbins = 0, rc;
    if ((rc = depth_frame_ready(d, "lm_detector_match_slabs"))) return rc;
    if (d->shard_world > 1) return lm_set_error(LM_ERR_INVALID, "lm_detector_match_slabs is not available on a sharded detector (%d ranks)", d->shard_world);
    if ((rc = lm_parts_refused(d, "lm_detector_match_slabs"))) return rc;
    if (slab_mm < 0) return lm_set_error(LM_ERR_INVALID, "slab_mm must not be negative, got %d", slab_mm);
    if ((rc = mode_options(options, &o, &nbins))) return rc;
    if (slab_capacity < o.max_modes + 1) return lm_set_error(LM_ERR_INVALID, "room for %d slabs, max_modes + 1 = %d may be reported", slab_capacity, o.max_modes + 1);
    HIP_TRY(hipSetDevice(d->device));
    if ((rc = lm_launch_pending(d))) return rc;

    // the requested classes, in their order; position = class_index of the result
    std::vector<std::string> names;
    if (class_ids && num_class_ids > 0)
        for (int i = 0; i < num_class_ids; ++i) names.push_back(class_ids[i] ? class_ids[i] : "");
    else
        for (const auto& kv : d->class_templates) names.push_back(kv.first);
    std::vector<int> ranged, free_of_range;                  // positions of the known classes with / without a range
    for (size_t p = 0; p < names.size(); ++p) {
        if (!d->class_templates.count(names[p])) continue;  // unknown classes are skipped, LL.cpp:1765-1767
        (d->class_depth_range.count(names[p]) ? ranged : free_of_range).push_back((int)p);
    }

    // modes first, then the quantising stages behind them on the same stream: the host waits for the records while the GPU quantises
    if ((rc = enqueue_modes(d, o, nbins))) return rc;
    struct Restore {                                         // whatever happens below, the detector's next match is an ordinary one
        lm_detector* d;
        ~Restore() { d->slabs.quantised = false; d->slabs.mask_on = false; }
    } restore{d};
    if ((rc = lm_quantise_resident(d))) return rc;
    d->slabs.quantised = true;
    lm_depth_mode modes[kDepthMaxModes];
    int nmodes = 0;
    if ((rc = wait_modes(d, o.max_modes, modes, &nmodes))) return rc;

    std::vector<lm_match> all;
    std::vector<int32_t> cls;
    int ns = 0;
    for (int k = 0; k < nmodes; ++k) {
        const int p = modes[k].depth_mm;
        lm_slab& s = slabs[ns++];
        s.depth_mm = p; s.pixels = modes[k].pixels; s.lo_mm = p - slab_mm; s.hi_mm = p + slab_mm;
        s.first_class = (int32_t)cls.size(); s.num_classes = 0; s.records = 0;
        std::vector<int> positions;
        for (int pos : ranged) {
            const std::pair<int, int>& r = d->class_depth_range[names[pos]];
            if (r.first <= p && p <= r.second) positions.push_back(pos);
        }
        if (positions.empty()) continue;                     // never to the matcher: an empty selection means every class there
        cls.insert(cls.end(), positions.begin(), positions.end());
        s.num_classes = (int32_t)positions.size();
        if ((rc = write_slab_masks(d, s.lo_mm, s.hi_mm))) return rc;
        d->slabs.mask_on = true;
        rc = run_pass(d, threshold, names, positions, all, &s.records);
        d->slabs.mask_on = false;
        if (rc) return rc;
    }
    if (!free_of_range.empty()) {                            // classes without a range: once, under the user's masks only
        lm_slab& s = slabs[ns++];
        s.depth_mm = -1; s.pixels = 0; s.lo_mm = s.hi_mm = 0;
        s.first_class = (int32_t)cls.size(); s.num_classes = (int32_t)free_of_range.size(); s.records = 0;
        cls.insert(cls.end(), free_of_range.begin(), free_of_range.end());
        if ((rc = run_pass(d, threshold, names, free_of_range, all, &s.records))) return rc;
    }
    const size_t nm = merge_matches_impl(all.data(), all.size(), false);
    lm_match* res = (lm_match*)malloc(std::max<size_t>(1, nm) * sizeof(lm_match));
    int32_t* rc_cls = (int32_t*)malloc(std::max<size_t>(1, cls.size()) * sizeof(int32_t));
    if (!res || !rc_cls) { free(res); free(rc_cls); return lm_set_error(LM_ERR_INVALID, "out of host memory"); }
    if (nm) memcpy(res, all.data(), nm * sizeof(lm_match));
    if (!cls.empty()) memcpy(rc_cls, cls.data(), cls.size() * sizeof(int32_t));
    *out = res; *n = nm; *num_slabs = ns; *slab_classes = rc_cls;
    return LM_OK;
}
