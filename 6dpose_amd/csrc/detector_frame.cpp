// The detector's frame: geometry and arenas, the blocking upload, frames parked in HBM, the front end of the training views
// and the stage read-back of the tests (lm_detector_read_stage).  The front end of the matching path is run_frontend_batch
// (detector_frontend.cpp).
#include <string.h>

#include "detector_internal.h"

// ---- frame upload + front end --------------------------------------------------------------------
// Zero tail after the 8 labels of one (level, modality) block: covers the reference's reads past a
// phase row and the reads of padded / out-of-image features redirected to it, for any
// position offset < Wd*Hd plus one 16-row window.
static size_t lm_tail_pad(int Wd, int Hd) { return (size_t)Wd * Hd + (size_t)16 * Wd + 2048; }

// (Re)allocates per-level buffers and the LM arena for a W x H frame; validates the reference's
// preconditions (LL.cpp:1136, 1217-1218).
int setup_geometry(lm_detector* d, int W, int H, bool check_match_preconditions) {
    const int L = d->pyramid_levels;
    FrameGeom g{};
    g.levels = L;
    int w = W, h = H;
    size_t arena = 0, sarena = 0;
    for (int l = 0; l < L; ++l) {
        if (l > 0) { w /= 2; h /= 2; }
        if (w < 1 || h < 1) return lm_set_error(LM_ERR_INVALID, "image too small for %d pyramid levels", L);
        int T = d->T_at_level[l];
        if (check_match_preconditions) {
            if (((long)w * h) % 16 != 0)
                return lm_set_error(LM_ERR_INVALID, "(src.rows * src.cols) %% 16 == 0 violated at level %d (%dx%d) [LL.cpp:1136]", l, w, h);
            if (h % T != 0 || w % T != 0)
                return lm_set_error(LM_ERR_INVALID, "response_map.rows/cols %% T == 0 violated at level %d (%dx%d, T=%d) [LL.cpp:1217-1218]", l, w, h, T);
        }
        LevelGeom& lv = g.lv[l];
        lv.W = w; lv.H = h; lv.T = T; lv.Wd = w / T; lv.Hd = h / T;
        size_t block = (size_t)8 * T * T * lv.Wd * lv.Hd + lm_tail_pad(lv.Wd, lv.Hd);
        block = (block + 255) & ~(size_t)255;
        d->lm_block_bytes[l] = block;
        for (int m = 0; m < 2; ++m) {
            if (arena + block > 0xFFFFFFFFull) return lm_set_error(LM_ERR_INVALID, "frame too large for the LM arena");
            lv.lm_off[m] = (uint32_t)arena;
            arena += block;
        }
        // strip-major copy for the refinement (levels below the top): [8 labels][T*T phases][NS strips][Hd rows][16 B]
        // per modality, then one all-zero plane (read by padded features) and slack for the second aligned dword.
        lv.NS = (lv.Wd + 15) / 16;
        lv.sm_off[0] = lv.sm_off[1] = 0;
        if (l < L - 1) {
            const size_t splane = (size_t)lv.NS * lv.Hd * 16;
            const size_t sblock = (size_t)8 * T * T * splane;
            if (sarena + 2 * sblock + 3 * splane + 4096 > 0xFFFFFFFFull) return lm_set_error(LM_ERR_INVALID, "frame too large for the strip arena");
            lv.sm_off[0] = (uint32_t)sarena;
            lv.sm_off[1] = (uint32_t)(sarena + sblock);
            sarena += 2 * sblock + 3 * splane + 4096;
            sarena = (sarena + 255) & ~(size_t)255;
        }
    }
    const size_t n0 = (size_t)W * H;
    int rc;
    // (a modality outside the detector's set has no frame buffer and no intermediates; its arena blocks exist, stay zero and are never written)
    if (d->use[0] && (rc = d->frame_rgb.ensure(n0 * d->cch))) return rc;
    if (d->use[1] && (rc = d->frame_depth.ensure(n0))) return rc;
    if (d->use[1] && (rc = d->nrm_raw.ensure(n0))) return rc;

    for (int a = 0; a < lm_detector::kSlots; ++a) {
        const bool realloc_arena = arena > d->lm_arena[a].cap;
        if ((rc = d->lm_arena[a].ensure(arena))) return rc;
        if (realloc_arena || d->fW != W || d->fH != H)   // zero tails (and everything else) once
            HIP_TRY(hipMemsetAsync(d->lm_arena[a].p, 0, d->lm_arena[a].cap, d->stream));
        const bool realloc_sarena = std::max<size_t>(sarena, 256) > d->sm_arena[a].cap;
        if ((rc = d->sm_arena[a].ensure(std::max<size_t>(sarena, 256)))) return rc;
        if (realloc_sarena || d->fW != W || d->fH != H) HIP_TRY(hipMemsetAsync(d->sm_arena[a].p, 0, d->sm_arena[a].cap, d->stream));
        {   // pair stream of the top level's two blocks (zero tails included); written whole by every front end, so never cleared
            const LevelGeom& top = g.lv[L - 1];
            d->cbits_byte0 = top.lm_off[0] & ~31u;
            d->cbits_npairs = (uint32_t)((top.lm_off[1] + d->lm_block_bytes[L - 1] - d->cbits_byte0 + 31) / 32);
            const size_t cbytes = (size_t)d->cbits_npairs * 8 + 64;
            const bool realloc_cbits = cbytes > d->cbits_arena[a].cap;
            if ((rc = d->cbits_arena[a].ensure(cbytes))) return rc;
            if (realloc_cbits || d->fW != W || d->fH != H) HIP_TRY(hipMemsetAsync(d->cbits_arena[a].p, 0, d->cbits_arena[a].cap, d->stream));
        }
        {   // strip records: the strip arena's layout at half the offsets; its zero planes stay zero
            const size_t bbytes = std::max<size_t>(sarena, 256) / 2 + 64;
            const bool realloc_bits = bbytes > d->bits_arena[a].cap;
            if ((rc = d->bits_arena[a].ensure(bbytes))) return rc;
            if (realloc_bits || d->fW != W || d->fH != H) HIP_TRY(hipMemsetAsync(d->bits_arena[a].p, 0, d->bits_arena[a].cap, d->stream));
        }
        // the second set of the wide paths follows the first where a wide match has allocated it (detector_launch.cpp, ensure_wide_arenas)
        for (DevBuf<uint8_t>* w : {&d->wbits_arena[a], &d->wcbits_arena[a]}) {
            if (!w->cap) continue;
            const size_t bytes = w == &d->wbits_arena[a] ? d->bits_arena[a].cap : d->cbits_arena[a].cap;
            const bool realloc_wide = bytes > w->cap;
            if ((rc = w->ensure(bytes))) return rc;
            if (realloc_wide || d->fW != W || d->fH != H) HIP_TRY(hipMemsetAsync(w->p, 0, w->cap, d->stream));
        }
    }
    for (int l = 0; l < L; ++l) {
        LevelBufs& b = d->lvl[l];
        b.W = g.lv[l].W; b.H = g.lv[l].H;
        size_t n = (size_t)b.W * b.H;
        if (d->use[0] && l > 0 && (rc = b.rgb.ensure(n * d->cch))) return rc;
        if (d->use[0] && (rc = b.mag.ensure(n))) return rc;
        if (d->use[0] && (rc = b.ang.ensure(n))) return rc;
        if (d->use[1] && (rc = b.nrm.ensure(n))) return rc;
    }
    if (d->fW != W || d->fH != H) d->quantised = false;      // the maps of the old size are gone
    d->geom = g;
    d->fW = W; d->fH = H;
    return LM_OK;
}

// The aligned size of a W x H source under the detector's border policy.  Strict hands the source size on as it is: setup_geometry refuses
// it with the reference's own asserts where it is not aligned.
int border_resolve(const lm_detector* d, int W, int H, int* Wa, int* Ha) {
    *Wa = W; *Ha = H;
    if (d->border == kBorderStrict) return LM_OK;
    if (!border_aligned_size(d->T_at_level.data(), d->pyramid_levels, d->border, W, H, Wa, Ha) || *Wa > 16384 || *Ha > 16384)
        return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", W, H);   // (crop: nothing of at least 16 x 16 fits; pad: beyond 16384)
    return LM_OK;
}

int upload_frame(lm_detector* d, const uint8_t* rgb, const uint16_t* depth, int W, int H, const uint8_t* const* masks, bool check_match_preconditions) {
    if ((d->use[0] && !rgb) || (d->use[1] && !depth)) return lm_set_error(LM_ERR_INVALID, "rgb/depth is null");
    if ((!d->use[0] && rgb) || (!d->use[1] && depth)) return lm_set_error(LM_ERR_INVALID, "a source was given for a modality outside the detector's set");
    if (W < 16 || H < 16 || W > 16384 || H > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", W, H);
    HIP_TRY(hipSetDevice(d->device));
    d->frame_valid = false;
    if (d->n_submitted != d->n_collected)   // the front end's buffers (and, on a size change, the arenas) belong to the frames in flight
        return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them before uploading another frame this way (lm_detector_submit_frame streams)");
    LM_DIAG_IDLE(d, "upload_frame");
    int rc, Wa = W, Ha = H;                 // the aligned geometry: the source's own for a training view and under the strict policy
    if (check_match_preconditions && (rc = border_resolve(d, W, H, &Wa, &Ha))) return rc;
    if ((rc = setup_geometry(d, Wa, Ha, check_match_preconditions))) return rc;
    const bool bordered = Wa != W || Ha != H;
    d->cur_rgb = d->frame_rgb.p; d->cur_depth = d->frame_depth.p;
    const size_t n = (size_t)W * H, na = (size_t)Wa * Ha;    // pixels of the source (staged and uploaded) and of the frame buffers
    const bool m0 = masks && masks[0], m1 = masks && d->nmod == 2 && masks[1];
    const size_t nc = d->use[0] ? n * d->cch : 0, nd = d->use[1] ? n * 2 : 0;     // only the sources of the set are staged and uploaded
    size_t bytes = nc + nd + (m0 ? n : 0) + (m1 ? n : 0);
    if ((rc = d->pinned.ensure(bytes))) return rc;
    uint8_t* st = d->pinned.p;
    if (nc) memcpy(st, rgb, nc);
    if (nd) memcpy(st + nc, depth, nd);
    BorderStage bs{};
    if (bordered && (rc = d->border_src.ensure(bytes + 16))) return rc;     // (+16: the kernel fetches the aligned dwords around a unit)
    HIP_TRY(hipEventRecord(d->ev[6], d->stream));
    if (bordered) {                                          // the sources as they are, in the staging buffer's layout; the frame buffers are written by k_frame_border below
        if (nc + nd) HIP_TRY(hipMemcpyAsync(d->border_src.p, st, nc + nd, hipMemcpyHostToDevice, d->stream));
        if (nc) border_job(bs.job[bs.njobs++], d->border_src.p, d->frame_rgb.p, W, H, Wa, Ha, d->cch, true);
        if (nd) border_job(bs.job[bs.njobs++], d->border_src.p + nc, d->frame_depth.p, W, H, Wa, Ha, 2, false);
    } else {
        if (nc) HIP_TRY(hipMemcpyAsync(d->frame_rgb.p, st, nc, hipMemcpyHostToDevice, d->stream));
        if (nd) HIP_TRY(hipMemcpyAsync(d->frame_depth.p, st + nc, nd, hipMemcpyHostToDevice, d->stream));
    }
    size_t off = nc + nd;
    d->have_mask[0] = d->have_mask[1] = false;
    for (int i = 0; i < d->nmod; ++i) {                      // masks[i] belongs to the set's i-th modality; the buffers are indexed by kind
        const int m = d->mod_kind[i];
        d->have_mask[m] = masks && masks[i];
        if (!d->have_mask[m]) continue;
        memcpy(st + off, masks[i], n);
        if ((rc = d->lvl[0].mask[m].ensure(na))) return rc;
        if (bordered) {                                      // a mask comes at the source size and is padded with 0 or cropped like the depth image
            HIP_TRY(hipMemcpyAsync(d->border_src.p + off, st + off, n, hipMemcpyHostToDevice, d->stream));
            border_job(bs.job[bs.njobs++], d->border_src.p + off, d->lvl[0].mask[m].p, W, H, Wa, Ha, 1, false);
        } else
            HIP_TRY(hipMemcpyAsync(d->lvl[0].mask[m].p, st + off, n, hipMemcpyHostToDevice, d->stream));
        off += n;
    }
    if (bordered) HIP_TRY(launch_frame_border(bs, d->stream));
    for (int i = 0; i < d->nmod; ++i) {
        const int m = d->mod_kind[i];
        if (!d->have_mask[m]) continue;
        for (int l = 1; l < d->pyramid_levels; ++l) {       // resize(INTER_NEAREST), LL.cpp:573-578, 874-879
            const LevelBufs& a = d->lvl[l - 1];
            LevelBufs& b = d->lvl[l];
            if ((rc = b.mask[m].ensure((size_t)b.W * b.H))) return rc;
            FeStage st{};                                   // one launch per level: level l reads level l - 1
            st.njobs = 1;
            fe_job_nn_down2(st.job[0], a.mask[m].p, b.mask[m].p, a.W, a.H);
            HIP_TRY(launch_fe_stage(st, d->stream));
        }
    }
    HIP_TRY(hipEventRecord(d->ev[7], d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));   // staging buffer is reused by the next call
    (void)hipEventElapsedTime(&d->last_h2d_ms, d->ev[6], d->ev[7]);
    d->frame_valid = true;
    return LM_OK;
}

// The front end of a training view (addTemplate): quantises every level of the current frame into lvl[]; only the quantised maps and
// the magnitudes are needed, no linear memories (the matching path builds its own: run_frontend_batch).
int run_frontend_training(lm_detector* d) {
    // One stream: measured on MI355X, forking the colour / pyramid / depth chains onto three streams
    // (events, also inside the hipGraph) cost more in cross-stream synchronisation (+26 us) than the
    // ~3 us kernels could overlap.  Instead the jobs of a level that do not depend on each other share a LAUNCH (k_fe_stage):
    // {colour chain, normals + median or their nearest-neighbour pyramid, pyrDown to the next level} — launch latency is the
    // critical path of a training view.
    hipStream_t s = d->stream;
    const int L = d->pyramid_levels;
    const float thr_sq = d->weak_threshold * d->weak_threshold;
    FeStage st{};
    for (int l = 0; l < L; ++l) {
        LevelBufs& b = d->lvl[l];
        const uint8_t* src = l == 0 ? d->cur_rgb : b.rgb.p;
        st.njobs = 0;                                                                                                 // (the chains of the set's modalities only)
        if (d->use[0]) fe_job_colour(st.job[st.njobs++], src, b.mag.p, b.ang.p, b.W, b.H, thr_sq, d->cch);                    // LL.cpp:367-504
        if (d->use[1]) {
            if (l == 0) fe_job_normals(st.job[st.njobs++], d->cur_depth, d->nrm_raw.p, b.nrm.p, b.W, b.H, d->distance_threshold,
                                       d->difference_threshold);                                                      // LL.cpp:729-819
            else fe_job_nn_down2(st.job[st.njobs++], d->lvl[l - 1].nrm.p, b.nrm.p, d->lvl[l - 1].W, d->lvl[l - 1].H); // LL.cpp:857-880
        }
        if (d->use[0] && l + 1 < L) fe_job_pyrdown(st.job[st.njobs++], src, d->lvl[l + 1].rgb.p, b.W, b.H, d->cch);           // LL.cpp:557-581
        HIP_TRY(launch_fe_stage(st, s));
    }
    d->quantised = true;
    return LM_OK;
}

extern "C" int lm_detector_set_frame(lm_detector* d, const uint8_t* rgb, const uint16_t* depth, int width, int height,
                                     const uint8_t* const* masks) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    return upload_frame(d, rgb, depth, width, height, masks, true);
}

extern "C" int lm_detector_store_frame(lm_detector* d, int slot, const uint8_t* rgb, const uint16_t* depth, int width, int height) {
    if (!d || slot < 0 || slot > 4095) return lm_set_error(LM_ERR_INVALID, "bad argument");
    if ((d->use[0] != (rgb != nullptr)) || (d->use[1] != (depth != nullptr))) return lm_set_error(LM_ERR_INVALID, "bad argument: the sources must be those of the detector's modality set");
    if (width < 16 || height < 16 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    HIP_TRY(hipSetDevice(d->device));
    if ((size_t)slot >= d->slot_rgb.size()) {
        d->slot_rgb.resize(slot + 1); d->slot_depth.resize(slot + 1);
        d->slot_w.resize(slot + 1, 0); d->slot_h.resize(slot + 1, 0);
    }
    const size_t n = (size_t)width * height;
    int rc, Wa, Ha;                                                         // a parked frame has the aligned size (strict: the source's, checked when it is selected)
    if ((rc = border_resolve(d, width, height, &Wa, &Ha))) return rc;
    const bool bordered = Wa != width || Ha != height;
    const size_t na = (size_t)Wa * Ha;
    const size_t nc = rgb ? n * d->cch : 0, nd = depth ? n : 0;                   // elements of the set's sources
    const size_t nca = rgb ? na * d->cch : 0, nda = depth ? na : 0;               // ... and of the parked frame
    if (d->slot_rgb[slot].cap < nca || d->slot_depth[slot].cap < nda)       // about to be reallocated: a frame in flight may still be
        HIP_TRY(hipStreamSynchronize(d->stream));                          // copying out of the old buffer
    if (nca && (rc = d->slot_rgb[slot].ensure(nca))) return rc;
    if (nda && (rc = d->slot_depth[slot].ensure(nda))) return rc;
    // staged through the detector's pinned buffer like every other upload (a pageable hipMemcpy stages internally, chunk by chunk)
    if ((rc = d->pinned.ensure(nc + nd * 2))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));                              // the staging buffer is shared with upload_frame
    uint8_t* st = d->pinned.p;
    if (nc) memcpy(st, rgb, nc);
    if (nd) memcpy(st + nc, depth, nd * 2);
    if (bordered) {                                                        // the source as it is, then k_frame_border into the slot
        if ((rc = d->border_src.ensure(nc + nd * 2 + 16))) return rc;
        HIP_TRY(hipMemcpyAsync(d->border_src.p, st, nc + nd * 2, hipMemcpyHostToDevice, d->stream));
        BorderStage bs{};
        if (nc) border_job(bs.job[bs.njobs++], d->border_src.p, d->slot_rgb[slot].p, width, height, Wa, Ha, d->cch, true);
        if (nd) border_job(bs.job[bs.njobs++], d->border_src.p + nc, d->slot_depth[slot].p, width, height, Wa, Ha, 2, false);
        HIP_TRY(launch_frame_border(bs, d->stream));
    } else {
        if (nc) HIP_TRY(hipMemcpyAsync(d->slot_rgb[slot].p, st, nc, hipMemcpyHostToDevice, d->stream));
        if (nd) HIP_TRY(hipMemcpyAsync(d->slot_depth[slot].p, st + nc, nd * 2, hipMemcpyHostToDevice, d->stream));
    }
    HIP_TRY(hipStreamSynchronize(d->stream));
    d->slot_w[slot] = Wa; d->slot_h[slot] = Ha;
    return LM_OK;
}

extern "C" int lm_detector_select_frame(lm_detector* d, int slot) {
    if (!d || slot < 0 || (size_t)slot >= d->slot_rgb.size() || d->slot_w[slot] <= 0)
        return lm_set_error(LM_ERR_INVALID, "no frame stored in slot %d", slot);
    HIP_TRY(hipSetDevice(d->device));
    const int W = d->slot_w[slot], H = d->slot_h[slot];
    if (W != d->fW || H != d->fH || d->lm_arena[0].cap == 0) {
        if (d->n_submitted != d->n_collected)   // setup_geometry reallocates and clears the arenas the frames in flight are reading
            return lm_set_error(LM_ERR_INVALID, "frame size changes (%dx%d -> %dx%d) with frames in flight: collect them first", d->fW, d->fH, W, H);
        d->frame_valid = false;
        LM_DIAG_IDLE(d, "lm_detector_select_frame (geometry change)");
        int rc = setup_geometry(d, W, H, true);
        if (rc) return rc;
    }
    d->frame_valid = false;
    const size_t n = (size_t)W * H;
    d->cur_rgb = d->frame_rgb.p; d->cur_depth = d->frame_depth.p;
    if (d->resident_reader) {                                 // a front end in flight (on the matching stream) may still read the resident frame
        HIP_TRY(hipStreamWaitEvent(d->stream, d->resident_reader, 0));
        d->resident_reader = nullptr;
    }
    if (d->use[0]) HIP_TRY(hipMemcpyAsync(d->frame_rgb.p, d->slot_rgb[slot].p, n * d->cch, hipMemcpyDeviceToDevice, d->stream));
    if (d->use[1]) HIP_TRY(hipMemcpyAsync(d->frame_depth.p, d->slot_depth[slot].p, n * 2, hipMemcpyDeviceToDevice, d->stream));
    d->have_mask[0] = d->have_mask[1] = false;
    d->last_h2d_ms = 0.f;
    d->frame_valid = true;
    return LM_OK;
}

// (every stage has the ALIGNED geometry: under a border policy that is not the source's)
extern "C" int64_t lm_detector_read_stage(lm_detector* d, int level, int kind, uint8_t* dst, int64_t capacity) {
    if (!d || level < 0 || level >= d->pyramid_levels || kind < 0 || kind > 8) return lm_set_error(LM_ERR_INVALID, "bad argument");
    if (d->fW <= 0) return lm_set_error(LM_ERR_INVALID, "no frame processed yet");
    if ((kind < 4 || kind == 8) && !d->use[kind == 8 ? 1 : kind & 1])            // kinds 0, 2: colour; 1, 3, 8: normals
        return lm_set_error(LM_ERR_INVALID, "stage %d belongs to %s, which is not in the detector's modality set", kind, kModalityName[kind == 8 ? 1 : kind & 1]);
    const LevelBufs& b = d->lvl[level];
    const LevelGeom& lv = d->geom.lv[level];
    const uint8_t* src = nullptr;
    int64_t size = 0;
    switch (kind) {
        case 0: src = b.ang.p; size = (int64_t)b.W * b.H; break;
        case 1: src = b.nrm.p; size = (int64_t)b.W * b.H; break;
        case 2: src = d->lm_arena[d->last_arena].p + lv.lm_off[0]; size = (int64_t)8 * lv.T * lv.T * lv.Wd * lv.Hd; break;
        case 3: src = d->lm_arena[d->last_arena].p + lv.lm_off[1]; size = (int64_t)8 * lv.T * lv.T * lv.Wd * lv.Hd; break;
        case 4:       // strip records of a level below the top, colour block then normal block (what k_local_bits reads)
            if (level == d->pyramid_levels - 1) return lm_set_error(LM_ERR_INVALID, "the top level has no strip records");
            // (a set of one: its own block only)
            src = d->bits_arena[d->last_arena].p + (lv.sm_off[d->mod_kind[0]] >> 1); size = (int64_t)d->nmod * 8 * lv.T * lv.T * lv.NS * lv.Hd * 8; break;
        case 5:       // pair stream of the top level (what k_coarse_bits reads)
            if (level != d->pyramid_levels - 1) return lm_set_error(LM_ERR_INVALID, "only the top level has a pair stream");
            src = d->cbits_arena[d->last_arena].p; size = (int64_t)d->cbits_npairs * 8; break;
        case 6:       // the second set of strip records (k_local_wide reads kinds 4 and 6): the layout and size of kind 4
            if (level == d->pyramid_levels - 1) return lm_set_error(LM_ERR_INVALID, "the top level has no strip records");
            if (!d->wbits_arena[d->last_arena].cap) return lm_set_error(LM_ERR_INVALID, "no second set of strip records: the last match did not refine on the wide path");
            src = d->wbits_arena[d->last_arena].p + (lv.sm_off[d->mod_kind[0]] >> 1); size = (int64_t)d->nmod * 8 * lv.T * lv.T * lv.NS * lv.Hd * 8; break;
        case 8:       // the normals of level 0 before the median, as the synchronous front end (a training view, a lone match, frame 0 of a batch) left them
            if (level != 0) return lm_set_error(LM_ERR_INVALID, "only level 0 has normals before the median");
            src = d->nrm_raw.p; size = (int64_t)b.W * b.H; break;
        default:      // the second pair stream (k_coarse_wide reads kinds 5 and 7): the layout and size of kind 5
            if (level != d->pyramid_levels - 1) return lm_set_error(LM_ERR_INVALID, "only the top level has a pair stream");
            if (!d->wcbits_arena[d->last_arena].cap) return lm_set_error(LM_ERR_INVALID, "no second pair stream: the last match did not run its coarse pass on the wide path");
            src = d->wcbits_arena[d->last_arena].p; size = (int64_t)d->cbits_npairs * 8; break;
    }
    if (dst && capacity > 0) {
        if (hipSetDevice(d->device) != hipSuccess) return lm_set_error(LM_ERR_HIP, "hipSetDevice failed");
        (void)hipStreamSynchronize(d->stream);
        (void)hipStreamSynchronize(d->mstream);
        if ((kind == 2 || kind == 3) && (level == d->pyramid_levels - 1 ? !d->fe_bytes_top : !d->fe_bytes_low)) {
            // the last front end wrote this level's bit planes only: build its byte planes now, from the quantised maps it left
            if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
            const LevelPtrs P = d->level_ptrs(0, level, d->last_arena);
            FeStage st{};
            st.resp = d->resp;
            st.njobs = 1;
            fe_job_build_lm(st.job[0], P.quant, P.mask, P.lm, P.strips, b.W, b.H, lv.T, d->mod_kind[0], d->nmod);
            HIP_TRY(launch_fe_stage(st, d->stream));
            (void)hipStreamSynchronize(d->stream);
        }
        hipError_t e = hipMemcpy(dst, src, (size_t)std::min(size, capacity), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return lm_set_error(LM_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
    }
    return size;
}
