// The batched front end of the matching path: run_frontend_batch, which every batch launch (detector_launch.cpp) goes through, and the two
// entry points that run it on the resident frame alone, on the frame stream (depth slabs, depth-scaled matching).  The front end of a
// training view is in detector_frame.cpp.
#include "detector_internal.h"

// Front end of a batch: the same three stages a lone frame takes (k_fe_stage: {colour chain, normals + median or their
// nearest-neighbour pyramid, pyrDown to the next level} per level, then the linear memories of every level), every stage ONE launch
// that carries the jobs of all frames of the batch.  Frame b keeps its intermediates in level_bufs(b, l) and writes the arenas of its
// own result slot.  7 launches per frame (round 2's per-slot graph) -> 3 per batch.
// direct_low / direct_top: nothing will read the byte planes of the levels below the top / of the top level — the bit planes are written
// straight from the quantised maps by one k_fe_bits launch at the end (fe_bits.hip) and the byte planes not at all.
// stages: bit 0 = quantise, bit 1 = the response memories (a slab pass of lm_detector_match_slabs runs 2 alone: the maps do not depend on masks).
int run_frontend_batch(lm_detector* d, int first, int nb, hipStream_t s, bool direct_low, bool direct_top, int stages) {
    const int L = d->pyramid_levels;
    const float thr_sq = d->weak_threshold * d->weak_threshold;
    int rc;
    for (int b = 1; b < nb; ++b) {                       // intermediates of the batch's further frames (frame 0: setup_geometry)
        for (int l = 0; l < L; ++l) {
            LevelBufs& B = d->level_bufs(b, l);
            B.W = d->lvl[l].W; B.H = d->lvl[l].H;
            const size_t n = (size_t)B.W * B.H;
            if (d->use[0] && l > 0 && (rc = B.rgb.ensure(n * d->cch))) return rc;
            if (d->use[0] && (rc = B.mag.ensure(n))) return rc;
            if (d->use[0] && (rc = B.ang.ensure(n))) return rc;
            if (d->use[1] && (rc = B.nrm.ensure(n))) return rc;
        }
        if (d->use[1] && (rc = d->nrm_raw_x[b - 1].ensure((size_t)d->fW * d->fH))) return rc;
    }
    const int m0 = d->mod_kind[0], nm = d->nmod;         // the modality set: the quantising chains and the writers' slices of the set only
    FeStage st{};
    st.resp = d->resp;                                   // the detector's response table: every writer of response memories takes it from the launch
    auto flush = [&]() -> int { if (st.njobs) { LM_CLOCK("launch_fe_stage"); HIP_TRY(launch_fe_stage(st, s)); } st.njobs = 0; return LM_OK; };
    auto room = [&](int jobs) { return st.njobs + jobs > kFeMaxJobs ? flush() : LM_OK; };
    auto build_lm_jobs = [&](int l) -> int {                 // linear memories of level l of every frame (its quantised maps are complete)
        if (!(stages & kFeMemories)) return LM_OK;
        if (l < L - 1 ? direct_low : direct_top) return LM_OK;   // bit planes only: fe_bits_jobs below
        for (int b = 0; b < nb; ++b) {
            const LevelPtrs P = d->level_ptrs(b, l, (first + b) % lm_detector::kSlots);
            if (int e = room(1)) return e;
            fe_job_build_lm(st.job[st.njobs++], P.quant, P.mask, P.lm, P.strips, d->lvl[l].W, d->lvl[l].H, d->geom.lv[l].T, m0, nm);
        }
        return LM_OK;
    };
    // Launch l quantises level l of every frame and — beside it, they only need level l - 1 — builds the linear memories of level
    // l - 1; a last launch builds those of the top level.  (The memories of level 0 are 3/4 of that work: they no longer wait for
    // the quantisation of the small levels, and the last launch is a quarter of what it was.)
    for (int l = 0; l < L; ++l) {
        st.njobs = 0;
        for (int b = 0; b < nb && (stages & kFeQuantise); ++b) {
            const lm_detector::Slot& sl = d->slot[(first + b) % lm_detector::kSlots];
            LevelBufs& B = d->level_bufs(b, l);
            const uint8_t* src = l == 0 ? sl.in_rgb : B.rgb.p;
            if ((rc = room(3))) return rc;
            if (d->use[0]) fe_job_colour(st.job[st.njobs++], src, nullptr /* magnitudes: addTemplate only */, B.ang.p, B.W, B.H, thr_sq, d->cch);      // LL.cpp:367-504
            if (d->use[1]) {
                if (l == 0) fe_job_normals(st.job[st.njobs++], sl.in_depth, b == 0 ? d->nrm_raw.p : d->nrm_raw_x[b - 1].p, B.nrm.p, B.W, B.H,
                                           d->distance_threshold, d->difference_threshold);                                      // LL.cpp:729-819
                else fe_job_nn_down2(st.job[st.njobs++], d->level_bufs(b, l - 1).nrm.p, B.nrm.p, d->level_bufs(b, l - 1).W, d->level_bufs(b, l - 1).H);   // LL.cpp:857-880
            }
            if (d->use[0] && l + 1 < L) fe_job_pyrdown(st.job[st.njobs++], src, d->level_bufs(b, l + 1).rgb.p, B.W, B.H, d->cch);                     // LL.cpp:557-581
        }
        if (l > 0 && (rc = build_lm_jobs(l - 1))) return rc;
        if ((rc = flush())) return rc;
    }
    if ((rc = build_lm_jobs(L - 1)) || (rc = flush())) return rc;
    if (stages & kFeQuantise) d->quantised = true;
    if (!(stages & kFeMemories)) return LM_OK;
    if (direct_low || direct_top) {                      // the bit planes of every frame in one launch
        st.njobs = 0;
        auto flush_bits = [&]() -> int { if (st.njobs) { LM_CLOCK("launch_fe_bits"); HIP_TRY(launch_fe_bits(st, s)); } st.njobs = 0; return LM_OK; };
        for (int b = 0; b < nb; ++b) {
            for (int l = 0; l < L; ++l) {
                const bool top = l == L - 1;
                if (top ? !direct_top : !direct_low) continue;
                const LevelPtrs P = d->level_ptrs(b, l, (first + b) % lm_detector::kSlots);
                const int W = d->lvl[l].W, H = d->lvl[l].H, T = d->geom.lv[l].T;
                if (st.njobs + 1 > kFeMaxJobs && (rc = flush_bits())) return rc;
                if (top) fe_job_top_bits(st.job[st.njobs++], P.quant, P.mask, P.top_stream, P.bit0, W, H, T, d->fe_top_mode, m0, nm);
                else fe_job_bits_rows(st.job[st.njobs++], P.quant, P.mask, P.bits, W, H, T, d->fe_top_mode == 0, m0, nm);
            }
        }
        if ((rc = flush_bits())) return rc;
    }
    d->fe_bytes_low = !direct_low; d->fe_bytes_top = !direct_top;
    d->last_arena = first;                               // read_stage: the maps of level_bufs(0, .) belong to the batch's first frame
    return LM_OK;
}

// The refusals of the entry points that read the resident frame: none resident, and — for those that run on the frame stream — frames in flight.
int lm_need_resident(const lm_detector* d, bool nothing_in_flight) {
    if (!d->frame_valid) return lm_set_error(LM_ERR_INVALID, "no frame resident: call lm_detector_set_frame / select_frame first");
    if (nothing_in_flight && d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    return LM_OK;
}

// The quantising stages of the resident frame into lvl[], on the frame stream, with nothing in flight (lm_detector_match_slabs: its passes
// follow with kFeMemories alone, ordered behind this by order_after_default_stream).
int lm_quantise_resident(lm_detector* d) {
    if (int rc = lm_need_resident(d, true)) return rc;
    LM_DIAG_IDLE(d, "lm_quantise_resident");
    const int si = (int)(d->n_submitted % lm_detector::kSlots);      // the slot the next submit takes: it reads the same frame
    d->slot[si].in_rgb = d->cur_rgb; d->slot[si].in_depth = d->cur_depth;
    return run_frontend_batch(d, si, 1, d->stream, false, false, kFeQuantise);
}

// The whole front end of the resident frame with the byte linear memories of every level (what lm_detector_set_paths' "bytes" paths and
// lm_detector_read_stage kinds 2 and 3 build), on the frame stream, with nothing in flight: depth-scaled matching reads them (detector_scaled.cpp).
int lm_byte_memories_resident(lm_detector* d, int* arena) {
    if (int rc = lm_need_resident(d, true)) return rc;
    LM_DIAG_IDLE(d, "lm_byte_memories_resident");
    const int si = (int)(d->n_submitted % lm_detector::kSlots);
    lm_detector::Slot& sl = d->slot[si];
    sl.in_rgb = d->cur_rgb; sl.in_depth = d->cur_depth; sl.have_mask[0] = d->have_mask[0]; sl.have_mask[1] = d->have_mask[1];
    *arena = si;
    return run_frontend_batch(d, si, 1, d->stream, false, false);
}
