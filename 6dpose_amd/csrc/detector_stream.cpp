// The streamed matching path: result slots, the front end and the launch of a batch, the GPU-time model that decides when a partial
// batch goes out, collect, and the live-stream ingest.  The helper threads and the staging copy are in host_pool.cpp, the result
// lists in match_lists.cpp.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

#include "detector_internal.h"

static int ensure_slot_buffers(lm_detector* d, lm_detector::Slot& sl, uint32_t match_cap) {
    if (!sl.h_counters)
        HIP_TRY(hipHostMalloc((void**)&sl.h_counters, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    if (match_cap > sl.match_cap) {
        if (sl.h_matches) (void)hipHostFree(sl.h_matches);
        sl.h_matches = nullptr; sl.match_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&sl.h_matches, (size_t)match_cap * sizeof(Candidate), hipHostMallocDefault));
        if (sl.h_distinct) (void)hipHostFree(sl.h_distinct);
        sl.h_distinct = nullptr;
        HIP_TRY(hipHostMalloc((void**)&sl.h_distinct, (size_t)match_cap * sizeof(Candidate), hipHostMallocDefault));
        sl.match_cap = match_cap;
    }
    return LM_OK;
}

static int sync_all_streams(lm_detector* d) {
    HIP_TRY(hipStreamSynchronize(d->stream)); HIP_TRY(hipStreamSynchronize(d->mstream));
    if (d->xchg.stream) HIP_TRY(hipStreamSynchronize(d->xchg.stream));
    return LM_OK;
}

static bool tiles_wanted(const lm_detector* d) { return d->use_tiles && d->refine_mode != 2; }   // LM_TILES=0 / lm_detector_set_paths(2, .): every candidate on its own

// Grid of the refinement kernel for a batch of nb frames.  Per-candidate path (LM_TILES=0): 3 workgroups (12 waves) per CU — alone it
// is as fast as with every wave slot taken (it is bound by the vector L1, not by latency), and the free slots let the coarse pass of
// the next frame and the front end run beside it.  With tiles the work items are fewer and larger (a tile = two singles' worth of
// loads; ~5k items per 2k templates): a grid with more waves than items gives every wave at most one item and lets the hardware's
// workgroup dispatch do the balancing — 171 us (3 per CU, items dealt round-robin, slowest wave 2 tiles + 1 single) -> 122 (8) ->
// 103 (16 and more), profiles/r02_sweep_local_blocks.txt.  A batch has nb times the items: the grid grows with it.
static int local_grid(lm_detector* d, int nb) {
    if (knobs().local_blocks > 0) return knobs().local_blocks;
    return d->num_cus * (tiles_wanted(d) ? 16 : 3) * std::max(1, std::min(nb, 4));
}

// Grid of k_local_bits (a wave serves 8 candidates, ~2k groups per frame at configs[1]): the workgroups the chip holds at once (4 waves per SIMD = 4 workgroups of 256 per CU), whatever the batch: the waves stride over
// the items.  (Round 4 launched four times as many for batches of four and more frames; one wave per item and a dispatcher that has to place 4096
// workgroups cost 3-4 %: 204-207 -> 197-199 us per 8-frame launch, profiles/r05_local_sharing/kernel_times_grid_sweep.txt.)
static int bits_grid(lm_detector* d, int nb) {
    (void)nb;
    if (knobs().local_blocks > 0) return knobs().local_blocks;
    return d->num_cus * 4;
}

// Front end of a batch: the same three stages a lone frame takes (k_fe_stage: {colour chain, normals + median or their
// nearest-neighbour pyramid, pyrDown to the next level} per level, then the linear memories of every level), every stage ONE launch
// that carries the jobs of all frames of the batch.  Frame b keeps its intermediates in level_bufs(b, l) and writes the arenas of its
// own result slot.  7 launches per frame (round 2's per-slot graph) -> 3 per batch.
// direct_low / direct_top: nothing will read the byte planes of the levels below the top / of the top level — the bit planes are written
// straight from the quantised maps by one k_fe_bits launch at the end (fe_bits.hip) and the byte planes not at all.
#ifdef LM_DIAG
struct LaunchClock {                                          // LM_LAUNCH_PROF: host time of the steps of a batch launch and of individual HIP calls in them; LM_LAUNCH_SERIES: the first 80 of each, one by one
    const char* name; double t0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit LaunchClock(const char* n) : name(n), t0(now()) {}
    ~LaunchClock() {
        static std::map<std::string, std::pair<double, long>> acc;
        const double dt = now() - t0;
        auto& a = acc[name]; a.first += dt; ++a.second;
        if (getenv("LM_LAUNCH_SERIES") && a.second <= 80) fprintf(stderr, "  %s #%ld: %.0f us\n", name, a.second, 1e6 * dt);
        if (getenv("LM_LAUNCH_PROF") && a.second % 64 == 0) fprintf(stderr, "  call %-22s %.1f us (n=%ld)\n", name, 1e6 * a.first / a.second, a.second);
    }
};
#define LM_CLOCK(n) LaunchClock lm_clock_##__LINE__(n)
#else
#define LM_CLOCK(n)
#endif
// stages: bit 0 = quantise, bit 1 = the response memories (a slab pass of lm_detector_match_slabs runs 2 alone: the maps do not depend on masks).
enum { kFeQuantise = 1, kFeMemories = 2 };
static int run_frontend_batch(lm_detector* d, int first, int nb, hipStream_t s, bool direct_low, bool direct_top, int stages = kFeQuantise | kFeMemories) {
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
    auto flush = [&]() { if (st.njobs) { LM_CLOCK("launch_fe_stage"); launch_fe_stage(st, s); } st.njobs = 0; };
    auto room = [&](int jobs) { if (st.njobs + jobs > kFeMaxJobs) flush(); };
    auto build_lm_jobs = [&](int l) {                        // linear memories of level l of every frame (its quantised maps are complete)
        if (!(stages & kFeMemories)) return;
        if (l < L - 1 ? direct_low : direct_top) return;    // bit planes only: fe_bits_jobs below
        for (int b = 0; b < nb; ++b) {
            const LevelPtrs P = d->level_ptrs(b, l, (first + b) % lm_detector::kSlots);
            room(1);
            fe_job_build_lm(st.job[st.njobs++], P.quant, P.mask, P.lm, P.strips, d->lvl[l].W, d->lvl[l].H, d->geom.lv[l].T, m0, nm);
        }
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
            room(3);
            if (d->use[0]) fe_job_colour(st.job[st.njobs++], src, nullptr /* magnitudes: addTemplate only */, B.ang.p, B.W, B.H, thr_sq, d->cch);      // LL.cpp:367-504
            if (d->use[1]) {
                if (l == 0) fe_job_normals(st.job[st.njobs++], sl.in_depth, b == 0 ? d->nrm_raw.p : d->nrm_raw_x[b - 1].p, B.nrm.p, B.W, B.H,
                                           d->distance_threshold, d->difference_threshold);                                      // LL.cpp:729-819
                else fe_job_nn_down2(st.job[st.njobs++], d->level_bufs(b, l - 1).nrm.p, B.nrm.p, d->level_bufs(b, l - 1).W, d->level_bufs(b, l - 1).H);   // LL.cpp:857-880
            }
            if (d->use[0] && l + 1 < L) fe_job_pyrdown(st.job[st.njobs++], src, d->level_bufs(b, l + 1).rgb.p, B.W, B.H, d->cch);                     // LL.cpp:557-581
        }
        if (l > 0) build_lm_jobs(l - 1);
        flush();
    }
    build_lm_jobs(L - 1);
    flush();
    if (!(stages & kFeMemories)) { HIP_TRY(hipGetLastError()); return LM_OK; }
    if (direct_low || direct_top) {                      // the bit planes of every frame in one launch
        st.njobs = 0;
        auto flush_bits = [&]() { if (st.njobs) { LM_CLOCK("launch_fe_bits"); launch_fe_bits(st, s); } st.njobs = 0; };
        for (int b = 0; b < nb; ++b) {
            for (int l = 0; l < L; ++l) {
                const bool top = l == L - 1;
                if (top ? !direct_top : !direct_low) continue;
                const LevelPtrs P = d->level_ptrs(b, l, (first + b) % lm_detector::kSlots);
                const int W = d->lvl[l].W, H = d->lvl[l].H, T = d->geom.lv[l].T;
                if (st.njobs + 1 > kFeMaxJobs) flush_bits();
                if (top) fe_job_top_bits(st.job[st.njobs++], P.quant, P.mask, P.top_stream, P.bit0, W, H, T, d->fe_top_mode, m0, nm);
                else fe_job_bits_rows(st.job[st.njobs++], P.quant, P.mask, P.bits, W, H, T, d->fe_top_mode == 0, m0, nm);
            }
        }
        flush_bits();
    }
    d->fe_bytes_low = !direct_low; d->fe_bytes_top = !direct_top;
    d->last_arena = first;                               // read_stage: the maps of level_bufs(0, .) belong to the batch's first frame
    HIP_TRY(hipGetLastError());
    return LM_OK;
}

// The bit-plane refinement (match_bits.hip): any pyramid with a level below the top; entries of up to 16383 features (two
// modalities of the reference's 8191, LL.cpp:1291).  LM_BITPLANES=0 / lm_detector_set_paths: the byte paths.  Two bits per cell carry a response
// table of at most two distinct non-zero values; the others (4 3 2 1 0 ...) run on the byte kernels, and lm_detector_get_paths says so.
// Under refine 3 / coarse 2 ("wide") a table of two planes runs exactly this; the others run the wide kernels below.
static bool bits_active(const lm_detector* d, int num_work) {
    return knobs().bitplanes && (d->refine_mode == 0 || d->refine_mode == 3) && d->resp_two_planes && num_work > 0 && d->geom.levels >= 2 && d->bits_max_nf <= 16383;
}
// ... and the coarse pass on the pair stream of the top level (it plans no tiles, so only together with the bit-plane refinement)
static bool cbits_active(const lm_detector* d, int num_work) {
    return bits_active(d, num_work) && knobs().coarse_bits && (d->coarse_mode == 0 || d->coarse_mode == 2) && d->cbits_max_nf <= 16383;
}
// The wide refinement (match_wide.hip): only when the table does not fit two planes and the path was asked for; the
// conditions that send a bank or geometry off the bit planes are those of bits_active.
static bool wide_active(const lm_detector* d, int num_work) {
    return knobs().bitplanes && d->refine_mode == 3 && !d->resp_two_planes && num_work > 0 && d->geom.levels >= 2 && d->bits_max_nf <= kWideMaxFeatures;
}
// ... and the wide coarse pass (no tiles either: only together with the wide refinement)
static bool cwide_active(const lm_detector* d, int num_work) {
    return wide_active(d, num_work) && knobs().coarse_bits && d->coarse_mode == 2 && d->cbits_max_nf <= kWideMaxFeatures;
}
// Part-based matching (match_parts.hip): k_coarse_parts / k_local_parts in place of k_coarse_bits / k_local_bits, for any
// pyramid (with a single level the coarse pass's verdict is final and k_local_parts only hands the candidates on).
static bool parts_active(const lm_detector* d, int num_work) { return d->part_min_parts > 0 && num_work > 0; }
// Nothing is silently holistic: whatever would send a part-mode frame to another kernel is refused when the frame is submitted.
static int parts_check(const lm_detector* d, float threshold) {
    if (d->part_min_parts <= 0) return LM_OK;
    if (!(threshold >= 0.f)) return lm_set_error(LM_ERR_INVALID, "part matching needs a threshold >= 0 (a part without responses must not pass), got %g", (double)threshold);
    if (d->shard_world > 1) return lm_set_error(LM_ERR_INVALID, "part matching is not available on a sharded detector (%d ranks)", d->shard_world);
    if (d->refine_mode != 0 || d->coarse_mode != 0 || !knobs().bitplanes || !knobs().coarse_bits)
        return lm_set_error(LM_ERR_INVALID, "part matching runs on the bit-plane kernels only: lm_detector_set_paths(d, 0, 0)");
    if (!d->resp_two_planes) return lm_set_error(LM_ERR_INVALID, "part matching needs a response table of at most two distinct non-zero values (the bit-plane kernels)");
    if (d->bits_max_nf > 16383 || d->cbits_max_nf > 16383) return lm_set_error(LM_ERR_INVALID, "part matching: a template entry has more than 16383 features");
    if (!d->bits_all_in)
        return lm_set_error(LM_ERR_INVALID, "part matching needs every refinement window inside its planes: a template of this bank has features outside its box, "
                                            "or is too large for the frame (width + 16 T > frame width)");
    return LM_OK;
}
// Device pointers of result slot `si` (everything a frame in flight owns).
static int frame_slot(lm_detector* d, int si, bool tiled, uint32_t tile_cap, FrameSlot* out) {
    lm_detector::Slot& sl = d->slot[si];
    const uint32_t cc = d->buf_cand_cap;
    FrameSlot F{};
    F.lm_arena = d->lm_arena[si].p; F.sm_arena = d->sm_arena[si].p;
    F.cands = d->d_cands.p + (size_t)cc * si;
    F.tiles = tiled ? d->d_tiles.p + (size_t)tile_cap * si : nullptr;
    F.todo = tiled ? d->d_todo.p + (size_t)cc * si : nullptr;
    F.counters = d->d_counters.p + (size_t)kCounterWords * si;
    F.matches_dev = d->d_matches_dev.p + (size_t)cc * si;
    F.dedupe_table = d->d_hash.p + dedupe_table_slots(cc) * (size_t)si;
    F.distinct_keys = d->d_distinct_keys.p + (size_t)cc * si;
    F.final_dev = d->d_final.p + 8 * (size_t)si;
    F.matches = nullptr;                                  // (k_local no longer stores the raw records into host memory: 16-byte PCIe writes per candidate)
    HIP_TRY(hipHostGetDevicePointer((void**)&F.distinct, sl.h_distinct, 0));
    HIP_TRY(hipHostGetDevicePointer((void**)&F.final_host, sl.h_counters, 0));
    *out = F;
    return LM_OK;
}

// Takes the next result slot for a frame (resident frame or ingest ring entry `ring`) and queues it behind the frames that wait for
// their batch; nothing is launched here.  The frames of a batch share threshold, work list and buffers, so a change of any of them
// launches what is waiting first.
static int slot_begin(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids, const uint8_t* rgb, const uint16_t* depth,
                      const bool have_mask[2], int ring) {
    if (d->n_submitted - d->n_collected >= (uint64_t)lm_detector::kSlots)
        return lm_set_error(LM_ERR_INVALID, "%d frames already in flight: call lm_detector_collect first", lm_detector::kSlots);
    HIP_TRY(hipSetDevice(d->device));
    int rc;
    if (d->bank_dirty || d->bank_geom_W != d->fW || d->bank_geom_H != d->fH) {
        if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "bank or frame geometry changed with a frame in flight");
        if ((rc = upload_bank(d))) return rc;
    }
    {   // the same selection as the frames waiting for their batch?  (build_work replaces the device-resident work list otherwise)
        std::vector<std::string> key;
        if (class_ids && num_class_ids > 0)
            for (int i = 0; i < num_class_ids; ++i) key.push_back(class_ids[i] ? class_ids[i] : "");
        const bool same = d->work_valid && key == d->work_key && d->work_key_rank == d->shard_rank && d->work_key_world == d->shard_world;
        if (d->pend_n && (!same || threshold != d->pend_threshold) && (rc = lm_launch_pending(d))) return rc;
    }
    if ((rc = build_work(d, class_ids, num_class_ids))) return rc;
    if ((rc = parts_check(d, threshold))) return rc;
    const int num_work = (int)d->work_pyr.size();
    const int K = lm_detector::kSlots;
    if (d->buf_cand_cap < d->cand_cap) {
        // first use, or the candidate capacity was raised after an overflow: the per-slot buffers are replaced.  Frames waiting for
        // their batch are launched, frames in flight finish on the old buffers first.
        if ((rc = lm_launch_pending(d))) return rc;
        if ((rc = sync_all_streams(d))) return rc;
        const uint32_t cc = d->cand_cap;
        if ((rc = d->d_cands.ensure((size_t)cc * K))) return rc;            // per result slot: coarse(k+1) runs beside local(k)
        if ((rc = d->d_matches_dev.ensure((size_t)cc * K))) return rc;
        if ((rc = d->d_hash.ensure(dedupe_table_slots(cc) * K))) return rc;   // one table per result slot
        if ((rc = d->d_distinct_keys.ensure((size_t)cc * K))) return rc;
        d->buf_cand_cap = cc;
    }
    if (!d->d_counters.p) {                                                          // per result slot; zero from here on (see k_dedupe)
        if ((rc = d->d_counters.ensure((size_t)kCounterWords * K))) return rc;
        if ((rc = d->d_final.ensure(8 * (size_t)K))) return rc;
        HIP_TRY(hipMemset(d->d_counters.p, 0, (size_t)kCounterWords * K * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(d->d_final.p, 0, 8 * (size_t)K * sizeof(unsigned long long)));
    }
    // tile refinement (match_bytes.hip): two-level pyramids with a tileable geometry; the buffers exist per result slot
    const bool tiled = (tiles_wanted(d) && num_work > 0 && tile_plan_possible(d->geom)) || bits_active(d, num_work) || wide_active(d, num_work) || parts_active(d, num_work);   // (the bit-plane paths use the todo bytes)
    const uint32_t tile_cap = d->buf_cand_cap / 2;      // a tile has at least two members
    if (tiled && (d->d_tiles.cap < (size_t)tile_cap * K || d->d_todo.cap < (size_t)d->buf_cand_cap * K)) {
        if ((rc = lm_launch_pending(d))) return rc;
        if ((rc = sync_all_streams(d))) return rc;
        if ((rc = d->d_tiles.ensure((size_t)tile_cap * K))) return rc;
        if ((rc = d->d_todo.ensure((size_t)d->buf_cand_cap * K))) return rc;
    }
    const int si = (int)(d->n_submitted % K);
    lm_detector::Slot& sl = d->slot[si];
    if ((rc = ensure_slot_buffers(d, sl, std::max<uint32_t>(sl.match_cap, d->buf_cand_cap)))) return rc;
    sl.t0 = std::chrono::steady_clock::now();
    sl.threshold = threshold; sl.num_work = num_work; sl.coarse_bytes = d->work_coarse_bytes; sl.h2d_ms = d->last_h2d_ms;
    sl.work_cls = d->work_cls; sl.work_tid = d->work_tid;
    sl.cand_cap = d->buf_cand_cap; sl.cands = d->d_cands.p + (size_t)d->buf_cand_cap * si;
    sl.matches_dev = d->d_matches_dev.p + (size_t)d->buf_cand_cap * si;
    sl.in_rgb = rgb; sl.in_depth = depth; sl.have_mask[0] = have_mask[0]; sl.have_mask[1] = have_mask[1]; sl.ring = ring;
    sl.launched = false; sl.pending = true; sl.leader = -1; sl.batch_n = 0;
    sl.src_w = sl.src_h = 0; sl.src_in_place = false;   // (lm_detector_submit_frame sets them for a source that is not aligned)
    if (d->pend_n == 0) { d->pend_first = si; d->pend_threshold = threshold; }
    ++d->pend_n;
    ++d->n_submitted;
    return LM_OK;
}

static inline double host_seconds(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(t.time_since_epoch()).count(); }

// Batches launched and not yet finished on the GPU (an event query per finished batch, none in the steady state of a full queue).
static int batches_queued(lm_detector* d) {
    while (!d->queued.empty() && hipEventQuery(d->slot[d->queued.front().slot].done) == hipSuccess) d->queued.erase(d->queued.begin());
    (void)hipGetLastError();                                  // hipErrorNotReady is not an error
    return (int)d->queued.size();
}

// GPU time of a batch of n frames: measured, or scaled from the nearest measured size (a batch costs about four frames' worth of
// fixed latency + its frames), or 0 when nothing has been measured yet.
static float batch_ms_estimate(const lm_detector* d, int n) {
    if (d->batch_ms[n] > 0.f) return d->batch_ms[n];
    for (int k = 1; k <= kMaxBatch; ++k)
        for (int m : {n - k, n + k})
            if (m >= 1 && m <= kMaxBatch && d->batch_ms[m] > 0.f) return d->batch_ms[m] * (4.f + (float)n) / (4.f + (float)m);
    return 0.f;
}

// Should the frames waiting for their batch go out now?  `at` = host time the question is asked for.
//   * nothing launched is still uncollected, or everything launched has finished: the GPU is idle, the waiting frames go out (the
//     first frame of a stream, a caller that collects every frame before the next) — in a tight loop once LM_FIRST_BATCH (3) of them
//     wait, and once per burst: the launch occupies the caller for two submits' worth of time and a lone frame costs the GPU twice a
//     batched one (A/B at the driver's 20 steps: 0.1054 -> 0.0997 ms per frame, 200 steps unchanged; profiles/r04_stream_ab.txt);
//   * the caller submits in a tight loop (frames arrive less than 2.5 launches' worth of host time apart): only full batches.  A
//     launch costs the calling thread ~0.1 ms (seven kernel launches + events) whatever the batch size, so a stream of partial
//     batches makes the HOST the bottleneck at the pace of one launch per frame, the GPU keeps up with it, looks about to run dry
//     at every submit — and the stream stays there (measured: 0.213 instead of 0.155 ms per frame).  lm_detector_collect launches
//     what is left when it is about to block on the last launched batch, so nothing waits for frames that never come;
//   * frames arrive sparsely (a camera): the GPU-time model — launch when the GPU's estimated backlog is shorter than the slack.
static bool partial_batch_due(lm_detector* d, double at) {
    if (d->pend_n <= 0 || d->keep_queued <= 0) return false;
    const bool tight = d->submit_gap_ms > 0.f && d->submit_gap_ms < 2.5f * d->launch_cost_ms;   // (submit_gap_ms 0: no second submit yet — sparse until shown otherwise)
    const bool drained = d->n_launched == d->n_collected;
    if (drained) d->early_batch_used = false;                  // nothing in flight: a new burst
    if (tight) {
        // ONE early batch per burst: the GPU is idle (nothing launched is unfinished), LM_FIRST_BATCH frames wait.  Not again until the pipeline has
        // drained: with a host that needs longer for three submits + a launch than the GPU for three frames, every early batch would find the GPU idle
        // again and the stream would settle on three frames per launch (one run in three of a 20-step series did: 0.154 instead of 0.100 ms per frame).
        if (d->early_batch_used || d->pend_n < knobs().first_batch) return false;
        if (!drained && batches_queued(d) != 0) return false;
        d->early_batch_used = true;
        return true;
    }
    // sparse: nothing launched is unfinished (collected or not) -> the GPU is idle, the frames go out; else the GPU-time model
    if (drained || batches_queued(d) == 0) return true;
    if (batch_ms_estimate(d, d->pend_n) <= 0.f) return batches_queued(d) < d->keep_queued;
    return d->gpu_free_at - at <= 1e-3 * d->launch_slack_ms;
}

// Ordering between the detector's two queues.  Every kernel of a batch runs on `mstream`; `stream` carries what the synchronous entry points
// enqueue — a blocking upload, the device-to-device copy of lm_detector_select_frame, the clearing of new arenas, a training view.  A batch must see
// all of that: whatever is still pending on `stream` when the batch is enqueued comes first.  (Nothing pending there — the steady state of a stream
// of uploaded frames — needs no ordering: a query instead of a record, a cross-queue wait and the barrier packet the GPU would process for it.)
// The other direction — work on `stream` that touches what a batch in flight reads or writes (level buffers, arenas, the resident frame) — is not
// ordered by events: such entry points run only with nothing in flight (n_submitted == n_collected, checked where they start) or wait for the
// batch's front end (select_frame: resident_reader).  A new caller that writes those buffers on `stream` has to do the same.
static int order_after_default_stream(lm_detector* d, hipStream_t s) {
    if (s == d->stream || hipStreamQuery(d->stream) == hipSuccess) return LM_OK;
    (void)hipGetLastError();                                  // hipErrorNotReady is not an error
    HIP_TRY(hipEventRecord(d->ev[5], d->stream));
    HIP_TRY(hipStreamWaitEvent(s, d->ev[5], 0));
    return LM_OK;
}

// What one batch launch works with: the frames waiting in slots [first, first + nb) and what is decided for all of them.
struct Batch {
    int nb, first, num_work;
    float threshold;
    bool bits, cbits, tiled;                  // refinement on bit planes / coarse pass on the pair stream / tile refinement
    bool wide, cwide;                         // ... on two sets of bit planes (match_wide.hip): bits / cbits are set as well
    bool parts;                               // ... under the part rule (match_parts.hip): bits / cbits are set as well
    bool direct_low, direct_top, top_ored;    // the front end writes the bit planes below the top / of the top level itself; ... by OR-ing into a zeroed pair stream
    uint32_t tile_cap, cap;
    hipStream_t s;                            // every kernel of a batch on the matching stream (one queue; the end of a stage is the start of the next)
    FrameBatch fb, fb_rest;                   // fb_rest: for k_local's per-candidate path on what k_local_bits leaves (todo = 1)
    BitsBatch bb;
    TopBits tb;
    WidePlanes wb, wt;                        // the second set of strip records / of the pair stream
    BankDev bank;                             // the device bank and work list, as the matching launchers take them
    PartsDev pd;                              // ... and its part tables
    int slot(int b) const { return (first + b) % lm_detector::kSlots; }
};

// The facts of the batch that waits in slots [pend_first, pend_first + pend_n), and its frames' device pointers.
static int batch_begin(lm_detector* d, Batch& B) {
    B.nb = d->pend_n; B.first = d->pend_first;
    d->pend_n = 0;
    const lm_detector::Slot& lead = d->slot[B.first];
    B.num_work = lead.num_work;
    B.threshold = lead.threshold;
    B.wide = wide_active(d, B.num_work);
    B.cwide = cwide_active(d, B.num_work);
    B.parts = parts_active(d, B.num_work);               // (slot_begin has refused what the part kernels do not serve: no wide table, ("bits", "bits"))
    B.bits = B.wide || B.parts || bits_active(d, B.num_work);
    B.cbits = B.cwide || B.parts || cbits_active(d, B.num_work);
    B.tiled = !B.bits && tiles_wanted(d) && B.num_work > 0 && tile_plan_possible(d->geom);
    B.tile_cap = d->buf_cand_cap / 2;
    B.cap = std::min<uint32_t>(lead.match_cap, d->buf_cand_cap);
    B.s = d->mstream;
    B.fb.nb = B.nb;
    B.bank = BankDev{d->d_entries.p, d->d_feat_off.p, d->d_feat_word.p, d->d_run_mask.p, d->d_feat_xy.p, d->d_work.p};
    B.pd = PartsDev{d->d_parts.p, d->d_part_off.p, d->d_part_word.p, d->part_min_parts};
    int rc;
    for (int b = 0; b < B.nb; ++b)
        if ((rc = frame_slot(d, B.slot(b), B.tiled, B.tile_cap, &B.fb.f[b]))) return rc;
    return LM_OK;
}

// The batch comes after its frames' uploads (copy stream) and after whatever the frame stream still holds; then the front end's start event.
static int order_batch(lm_detector* d, const Batch& B) {
    for (int b = B.nb - 1; b >= 0; --b) {                     // (the copy stream is one in-order queue: the upload of the batch's last streamed frame covers the earlier ones)
        const int ring = d->slot[B.slot(b)].ring;
        if (ring < 0) continue;
        if (hipEventQuery(d->ingest.t1[ring]) != hipSuccess) { (void)hipGetLastError(); HIP_TRY(hipStreamWaitEvent(B.s, d->ingest.t1[ring], 0)); }   // (already there: nothing to wait for)
        break;
    }
    int rc;
    if ((rc = order_after_default_stream(d, B.s))) return rc;
    HIP_TRY(hipEventRecord(d->slot[B.first].ev[0], B.s));
    return LM_OK;
}

// Streamed frames whose source size is not aligned (frame_border.h): ONE k_frame_border launch writes the aligned colour and depth images of
// every such frame of the batch, from the source-size copies their uploads left in the ring entries, in front of the front end.
static int enqueue_border(lm_detector* d, const Batch& B) {
    BorderStage bs{};
    for (int b = 0; b < B.nb; ++b) {
        const int si = B.slot(b);
        const lm_detector::Slot& sl = d->slot[si];
        if (sl.ring < 0 || !sl.src_w) continue;
        if (sl.src_in_place && d->fW <= sl.src_w && d->fH <= sl.src_h) continue;            // cropped by the 2-D copies: no margin
        const lm_detector::Ingest& g = d->ingest;
        if (d->use[0]) border_job(bs.job[bs.njobs++], g.d_src[si].p, g.d_rgb[si].p, sl.src_w, sl.src_h, d->fW, d->fH, d->cch, true, sl.src_in_place);
        const size_t src_depth_off = d->use[0] ? ((size_t)sl.src_w * sl.src_h * d->cch + 15) & ~(size_t)15 : 0;   // (the entry's layout at ITS source size: another frame of the batch may have another)
        if (d->use[1]) border_job(bs.job[bs.njobs++], g.d_src[si].p + src_depth_off, g.d_depth[si], sl.src_w, sl.src_h, d->fW, d->fH, 2, false, sl.src_in_place);
    }
    if (bs.njobs) HIP_TRY(launch_frame_border(bs, B.s));
    return LM_OK;
}

// The front end writes the bit planes directly where nothing reads the byte planes: below the top when no candidate can leave its planes
// (then k_local never runs behind k_local_bits), at the top level when the coarse pass runs on the pair stream.
static int choose_bit_writers(lm_detector* d, Batch& B) {
    B.direct_low = knobs().fe_bits && d->fe_direct && B.bits && !B.wide && d->bits_all_in;   // (a wide table: byte planes, packed — the front end's writers know two planes)
    B.direct_top = knobs().fe_bits && d->fe_direct && B.cbits && !B.cwide;
    for (int l = 0; l + 1 < d->geom.levels; ++l) B.direct_low = B.direct_low && fe_bits_rows_possible(d->geom.lv[l].W, d->geom.lv[l].T);
    const LevelGeom& topl = d->geom.lv[d->geom.levels - 1];
    const uint32_t top_bit0[2] = {topl.lm_off[0] - d->cbits_byte0, topl.lm_off[1] - d->cbits_byte0};
    B.top_ored = B.direct_top && fe_top_bits_kind(topl.W, topl.H, topl.T, top_bit0, d->fe_top_mode, d->mod_kind[0], d->nmod) == kFeTopBits;   // (else whole bytes / dwords are stored: nothing to clear)
    if (B.top_ored)                                      // the pair stream is OR-ed together: it has to be zero (k_local_bits leaves it so; k_pack_top and first use do not)
        for (int b = 0; b < B.nb; ++b) {
            const int si = B.slot(b);
            if (!d->cbits_clean[si]) HIP_TRY(hipMemsetAsync(d->cbits_arena[si].p, 0, (size_t)d->cbits_npairs * 8, B.s));
            d->cbits_clean[si] = false;                  // dirty from the front end on, until k_local_bits (top_clear) is enqueued behind it: an error return in between must not leave it marked clean
        }
    return LM_OK;
}

// The second arenas of the batch's slots, at the sizes of the first: allocated and zeroed (the zero planes and tails of set 1 are read like
// those of set 0) when a slot first serves a wide batch.  The slot is free — its previous frame was collected —, so nothing reads what is replaced.
static int ensure_wide_arenas(lm_detector* d, const Batch& B) {
    for (int b = 0; b < B.nb; ++b) {
        const int si = B.slot(b);
        DevBuf<uint8_t>* w[2] = {B.wide ? &d->wbits_arena[si] : nullptr, B.cwide ? &d->wcbits_arena[si] : nullptr};
        const size_t bytes[2] = {d->bits_arena[si].cap, d->cbits_arena[si].cap};
        for (int k = 0; k < 2; ++k) {
            if (!w[k] || w[k]->cap >= bytes[k]) continue;
            if (int rc = w[k]->ensure(bytes[k])) return rc;
            HIP_TRY(hipMemsetAsync(w[k]->p, 0, w[k]->cap, B.s));
        }
    }
    return LM_OK;
}

// The tables of the bit-plane kernels (BitsBatch, TopBits), and the bit planes themselves where the front end left byte planes.
static void pack_bit_planes(lm_detector* d, Batch& B) {
    B.fb_rest = B.fb;
    if (B.bits) {
        for (int b = 0; b < B.nb; ++b) {
            const int si = B.slot(b);
            B.bb.strips[b] = d->sm_arena[si].p; B.bb.bits[b] = d->bits_arena[si].p;
            B.fb.f[b].todo = B.fb_rest.f[b].todo = d->d_todo.p + (size_t)d->buf_cand_cap * si;
            B.fb_rest.f[b].tiles = d->d_tiles.p + (size_t)B.tile_cap * si;   // non-null: "only the candidates marked todo"; no tile was planned
        }
        if (B.wide) {
            for (int b = 0; b < B.nb; ++b) B.wb.set1[b] = d->wbits_arena[B.slot(b)].p;
            for (int l = 0; l + 1 < d->geom.levels; ++l) launch_pack_wide(B.bb, B.wb, B.nb, d->geom.lv[l], B.s);
        } else
        if (!B.direct_low)
            for (int l = 0; l + 1 < d->geom.levels; ++l) launch_pack_bits(B.bb, B.nb, d->geom.lv[l], B.s);
    }
    if (B.cbits) {
        for (int b = 0; b < B.nb; ++b) {
            const int si = B.slot(b);
            B.tb.lm[b] = d->lm_arena[si].p; B.tb.bits[b] = d->cbits_arena[si].p;
            if (B.top_ored && !d->fe_keep_top) B.bb.top_clear[b] = d->cbits_arena[si].p;     // zeroed again by k_local_bits, after k_coarse_bits has read it
            else d->cbits_clean[si] = false;
        }
        if (B.top_ored && !d->fe_keep_top) B.bb.top_clear_units = (d->cbits_npairs * 8u + 15u) / 16u;
        if (B.cwide) {
            for (int b = 0; b < B.nb; ++b) B.wt.set1[b] = d->wcbits_arena[B.slot(b)].p;
            launch_pack_top_wide(B.tb, B.wt, B.nb, d->cbits_byte0, d->cbits_npairs, B.s);
        } else
        if (!B.direct_top) launch_pack_top(B.tb, B.nb, d->cbits_byte0, d->cbits_npairs, B.s);
    }
}

// One queue for the whole batch: the end of a stage IS the start of the next — one timing record between two kernels instead of two or
// three, and fe_done only when something outside the batch waits for this front end (a resident frame).
static int record_front_end(lm_detector* d, const Batch& B) {
    lm_detector::Slot& lead = d->slot[B.first];
    bool resident_in = false;
    for (int b = 0; b < B.nb; ++b) resident_in = resident_in || d->slot[B.slot(b)].ring < 0;
    HIP_TRY(hipEventRecord(lead.ev[1], B.s));
    if (resident_in) HIP_TRY(hipEventRecord(lead.fe_done, B.s));
    for (int b = 0; b < B.nb; ++b)                            // the resident frame is read by this front end: the next lm_detector_select_frame copy waits for it
        if (d->slot[B.slot(b)].ring < 0) d->resident_reader = lead.fe_done;
    for (int b = 0; b < B.nb; ++b) {                          // a resident re-match of a streamed frame reads its ring entry: the entry's next upload waits for this front end
        const lm_detector::Slot& sl = d->slot[B.slot(b)];
        if (sl.ring < 0 && d->ingest.stream)
            for (int r = 0; r < lm_detector::kSlots; ++r)
                if (d->ingest.d_rgb[r].p && (sl.in_rgb ? sl.in_rgb == d->ingest.d_rgb[r].p : (const void*)sl.in_depth == (const void*)d->ingest.d_rgb[r].p)) d->ingest.reader[r] = lead.fe_done;   // (a depth-only entry starts with the depth image)
    }
    return LM_OK;
}

static int enqueue_coarse(lm_detector* d, const Batch& B) {
    // the counters are zero on entry (reset by the slots' previous k_dedupe)
    { LM_CLOCK("launch_coarse");
    if (B.cwide) launch_coarse_wide(B.fb, B.tb, B.wt, d->geom, B.bank, B.num_work, B.threshold, d->buf_cand_cap, d->cbits_byte0, d->cbits_max_nf, B.s);
    else if (B.parts) { launch_coarse_parts(B.fb, B.tb, d->geom, B.bank, B.pd, B.num_work, B.threshold, d->buf_cand_cap, d->cbits_byte0, d->cbits_max_nf, d->resp_low_weight, B.s); d->coarse_batched = false; }
    else if (B.cbits) d->coarse_batched = launch_coarse_bits(B.fb, B.tb, d->geom, B.bank, B.num_work, B.threshold, d->buf_cand_cap, d->cbits_byte0, d->cbits_max_nf, d->resp_low_weight, B.s, d->coarse_batch);
    else launch_coarse(B.fb, d->geom, B.bank, B.num_work, B.threshold, d->buf_cand_cap, B.tile_cap, B.s);
    }
    HIP_TRY(hipEventRecord(d->slot[B.first].ev[3], B.s));
    return LM_OK;
}

// persistent refinement grid over the tiles and then the remaining candidates of every frame of the batch; the counts are
// read on the device (no host round trip), the records stored straight into the slots' pinned host memory; it also empties
// the hash tables k_dedupe uses
static int enqueue_match(lm_detector* d, const Batch& B) {
    const uint32_t dedupe_slots = (uint32_t)dedupe_table_slots(d->buf_cand_cap);
    if (B.bits) {
        { LM_CLOCK("launch_local_bits");
        if (B.wide) launch_local_wide(B.fb, B.bb, B.wb, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, bits_grid(d, B.nb), d->bits_max_nf, B.s);
        else if (B.parts) launch_local_parts(B.fb, B.bb, d->geom, B.bank, B.pd, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, bits_grid(d, B.nb), d->bits_max_nf, d->resp_low_weight, B.s);
        else launch_local_bits(B.fb, B.bb, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, bits_grid(d, B.nb), d->bits_max_nf, d->resp_low_weight, B.s); }
        if (B.bb.top_clear_units)     // the pair streams this launch zeroes again are clean for their slots' next frames
            for (int b = 0; b < B.nb; ++b)
                if (B.bb.top_clear[b]) d->cbits_clean[B.slot(b)] = true;
        if (!d->bits_all_in)          // candidates whose windows leave their planes (marked in todo): k_local's per-candidate path
            launch_local(B.fb_rest, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, B.tile_cap, d->num_cus * 2, B.s);
    } else
    if (B.num_work > 0)
        launch_local(B.fb, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, B.tile_cap, local_grid(d, B.nb), B.s);
    HIP_TRY(hipEventRecord(d->slot[B.first].ev[4], B.s));
    return LM_OK;
}

// exact duplicates out (they never survive std::unique): distinct records + counts to the slots' pinned memory; then the batch's `done` event
static int enqueue_dedupe(lm_detector* d, const Batch& B) {
    // k_dedupe's grid per frame: a workgroup per 256 candidates of the LAST collected frame (the kernel strides over whatever the count turns out to
    // be), between 64 and two per CU.  Every workgroup takes a ticket at the frame's counter and most of a 2-per-CU grid had nothing else to do:
    // 31 -> 19.5 us per 8-frame batch at 16k candidates per frame (profiles/r04_stream_ab.txt).
    const int dedupe_blocks = knobs().dedupe_blocks > 0 ? knobs().dedupe_blocks
                                                        : std::max(64, std::min(d->num_cus * 2, (int)((d->ncand_hint + 255) / 256)));
    if (B.num_work > 0) {
        LM_CLOCK("launch_dedupe");
        launch_dedupe(B.fb, d->buf_cand_cap, dedupe_table_slots(d->buf_cand_cap), d->d_work_cls.p, d->d_work_tid.p, dedupe_blocks, B.s);
    }
    else
        for (int b = 0; b < B.nb; ++b) HIP_TRY(hipMemsetAsync(B.fb.f[b].final_dev, 0, 8 * sizeof(unsigned long long), B.s));   // nothing searched: no records for NMS / exchange
    { LM_CLOCK("record done"); HIP_TRY(hipEventRecord(d->slot[B.first].done, B.s)); }
    return LM_OK;
}

// The slots are launched; the batch joins the queue of the GPU-time model.
static void batch_launched(lm_detector* d, const Batch& B) {
    const auto now = std::chrono::steady_clock::now();
    for (int b = 0; b < B.nb; ++b) {
        lm_detector::Slot& sl = d->slot[B.slot(b)];
        sl.launched = true; sl.leader = B.first; sl.batch_n = B.nb; sl.t1 = now;
    }
    const double t = host_seconds(now);
    const bool idle = batches_queued(d) == 0;
    if (idle) d->gpu_free_at = std::min(d->gpu_free_at, t);
    d->gpu_free_at = std::max(d->gpu_free_at, t) + 1e-3 * batch_ms_estimate(d, B.nb);
    d->queued.push_back({d->n_launched, B.first, B.nb, t, idle});
    d->n_launched += (uint64_t)B.nb;
}

// Enqueue the whole device pipeline of the frames waiting in slots [pend_first, pend_first + pend_n): ONE front end, coarse pass,
// refinement and duplicate removal for all of them (asynchronous).
int lm_launch_pending(lm_detector* d) {
    if (d->pend_n <= 0) return LM_OK;
    Batch B{};
    int rc;
    {
        LM_CLOCK("step waits+ev0");
        HIP_TRY(hipSetDevice(d->device));
        if ((rc = batch_begin(d, B)) || (rc = order_batch(d, B)) || (rc = enqueue_border(d, B)) || (rc = choose_bit_writers(d, B))) return rc;
        if ((B.wide || B.cwide) && (rc = ensure_wide_arenas(d, B))) return rc;
    }
    const int stages = d->slabs.quantised && B.nb == 1 ? kFeMemories : kFeQuantise | kFeMemories;
    { LM_CLOCK("step front end"); if ((rc = run_frontend_batch(d, B.first, B.nb, B.s, B.direct_low, B.direct_top, stages))) return rc; }
    { LM_CLOCK("step bits tables+ev1"); pack_bit_planes(d, B); if ((rc = record_front_end(d, B))) return rc; }
    { LM_CLOCK("step coarse"); if ((rc = enqueue_coarse(d, B))) return rc; }
    { LM_CLOCK("step refine"); if ((rc = enqueue_match(d, B))) return rc; }
    { LM_CLOCK("step dedupe+done"); if ((rc = enqueue_dedupe(d, B))) return rc; }
    batch_launched(d, B);
    return LM_OK;
}

// The quantising stages of the resident frame into lvl[], on the frame stream, with nothing in flight (lm_detector_match_slabs: its passes
// follow with kFeMemories alone, ordered behind this by order_after_default_stream).
int lm_quantise_resident(lm_detector* d) {
    if (!d->frame_valid) return lm_set_error(LM_ERR_INVALID, "no frame resident: call lm_detector_set_frame / select_frame first");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    LM_DIAG_IDLE(d, "lm_quantise_resident");
    const int si = (int)(d->n_submitted % lm_detector::kSlots);      // the slot the next submit takes: it reads the same frame
    d->slot[si].in_rgb = d->cur_rgb; d->slot[si].in_depth = d->cur_depth;
    return run_frontend_batch(d, si, 1, d->stream, false, false, kFeQuantise);
}

// The whole front end of the resident frame with the byte linear memories of every level (what lm_detector_set_paths' "bytes" paths and
// lm_detector_read_stage kinds 2 and 3 build), on the frame stream, with nothing in flight: depth-scaled matching reads them (detector_scaled.cpp).
int lm_byte_memories_resident(lm_detector* d, int* arena) {
    if (!d->frame_valid) return lm_set_error(LM_ERR_INVALID, "no frame resident: call lm_detector_set_frame / select_frame first");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    LM_DIAG_IDLE(d, "lm_byte_memories_resident");
    const int si = (int)(d->n_submitted % lm_detector::kSlots);
    lm_detector::Slot& sl = d->slot[si];
    sl.in_rgb = d->cur_rgb; sl.in_depth = d->cur_depth; sl.have_mask[0] = d->have_mask[0]; sl.have_mask[1] = d->have_mask[1];
    *arena = si;
    return run_frontend_batch(d, si, 1, d->stream, false, false);
}

// The detector's current frame (lm_detector_set_frame / select_frame, or the frame a previous submit_frame left current) as a
// batch of one, launched at once.
int lm_submit_frame(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids) {
    if (!d->frame_valid) return lm_set_error(LM_ERR_INVALID, "no frame resident: call lm_detector_set_frame / select_frame first");
    int rc;
    if ((rc = lm_launch_pending(d))) return rc;               // frames waiting for their batch go first (results come back in order)
    if ((rc = slot_begin(d, threshold, class_ids, num_class_ids, d->cur_rgb, d->cur_depth, d->have_mask, -1))) return rc;
    return lm_launch_pending(d);
}

static float ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<float, std::milli>(b - a).count();
}

// `nsrc` records of a frame (the distinct ones k_dedupe left in the slot's pinned memory, or the raw ones) as lm_match, without those the
// refinement dropped; merge: canonically sorted + uniqued (Detector::match's list under the canonical order of SURVEY A12; distinct: the
// records hold no exact duplicates).  Returns the count; *res_out is malloc'ed for `room` entries (null: out of memory).
static size_t canonical_list_of(const lm_detector::Slot& sl, const Candidate* src, uint64_t nsrc, size_t room, bool merge, bool distinct,
                                lm_match** res_out, ListClock* clock) {
    lm_match* res = (lm_match*)malloc(std::max<size_t>(1, room) * sizeof(lm_match));
    *res_out = res;
    if (!res) return 0;
    const std::vector<int32_t>& wcls = *sl.work_cls;
    const std::vector<int32_t>& wtid = *sl.work_tid;
    size_t w = 0;
    for (uint64_t i = 0; i < nsrc; ++i) {
        const Candidate& c = src[i];
        if (c.work < 0) continue;                     // dropped below the threshold during refinement
        res[w].x = c.x; res[w].y = c.y; res[w].similarity = c.score;
        res[w].class_index = wcls[c.work];
        res[w].template_id = wtid[c.work];
        ++w;
    }
    clock->converted = std::chrono::steady_clock::now();
    const size_t n = merge ? merge_matches_impl(res, w, distinct) : w;
    clock->merged = std::chrono::steady_clock::now();
    return n;
}

// The canonical list of a finished frame on a helper thread (its records are in pinned memory: the caller has seen the batch's event)
static void prepare_list_job(lm_detector::Slot* sl) {
    int state = 2;
    sl->prep = nullptr; sl->prep_n = 0;
    const unsigned long long* hc = sl->h_counters;
    if (sl->num_work > 0 && hc[0] <= sl->cand_cap && hc[0] <= sl->match_cap && hc[1] <= hc[0]) {
        const auto t0 = std::chrono::steady_clock::now();
        ListClock lc{};
        sl->prep_n = canonical_list_of(*sl, sl->h_distinct, hc[1], (size_t)hc[1], true, true, &sl->prep, &lc);
        sl->prep_collect_ms = ms_between(t0, lc.converted); sl->prep_merge_ms = ms_between(lc.converted, lc.merged);
        if (sl->prep) state = 1;
    }
    sl->ready.store(state, std::memory_order_release);
}

// Takes over the list a helper thread prepared for the slot, if a job covers it.  Returns whether there is one (*list may be set without:
// the caller frees it).
static bool take_prepared_list(lm_detector* d, lm_detector::Slot& sl, lm_match** list, size_t* n) {
    if (!sl.prep_queued) return false;                  // a helper thread owns the slot until it has marked it ready (a job of ~35 us, posted when the batch's first frame was collected)
    for (int spin = 0; sl.ready.load(std::memory_order_acquire) == 0;) {    // (a job still queued — this slot's, possibly — is run here)
        if (pool_run_one(d)) continue;
        if (++spin < 20000) __builtin_ia32_pause(); else std::this_thread::yield();
    }
    const bool have = sl.ready.load(std::memory_order_acquire) == 1;
    *list = sl.prep; *n = sl.prep_n;
    sl.prep = nullptr; sl.prep_n = 0; sl.prep_queued = false;
    return have;
}

// Keeping the GPU-time model current around a collect's wait.  If the wait blocks on the first frame of a batch, the batch finished when
// the wait returned: that pins the estimate of when the GPU runs dry and — with the start of the batch known too (the previous batch's
// end seen the same way, or an idle GPU at launch) — gives the batch's duration.  Frames waiting for their batch go out BEFORE
// the wait if the GPU would have (almost) nothing left when it ends, or after it if it has by then.
struct CollectWait {
    bool batch_head, blocked;                           // the frame is the first of the oldest queued batch; the wait will block on it
    lm_detector::QueuedBatch head;
};
static double later_batches_ms(const lm_detector* d) {  // estimated GPU time of the batches launched after the frame being collected
    double ms = 0.0;
    for (const lm_detector::QueuedBatch& q : d->queued)
        if (q.first_frame > d->n_collected) { const float e = batch_ms_estimate(d, q.frames); ms += e > 0.f ? e : 1e3; }   // not timed yet: plenty
    return ms;
}
static int model_before_wait(lm_detector* d, const lm_detector::Slot& sl, CollectWait* w) {
    w->batch_head = !d->queued.empty() && d->queued.front().first_frame == d->n_collected && d->queued.front().slot == sl.leader;
    w->blocked = false;
    if (!w->batch_head) return LM_OK;
    w->head = d->queued.front();
    w->blocked = hipEventQuery(d->slot[sl.leader].done) == hipErrorNotReady;
    (void)hipGetLastError();
    if (w->blocked && d->pend_n > 0 && d->keep_queued > 0 && later_batches_ms(d) <= d->launch_slack_ms)   // (no batch launched after this one: 0, with or without a GPU-time model)
        return lm_launch_pending(d);
    return LM_OK;
}
static int model_after_wait(lm_detector* d, const CollectWait& w, double now) {
    const lm_detector::QueuedBatch& head = w.head;
    const double dry_at = now + 1e-3 * later_batches_ms(d);
    if (w.batch_head && w.blocked) {
        const bool start_known = head.gpu_idle_at_launch || (d->last_done_at >= 0.0 && d->last_done_end == head.first_frame);
        if (start_known) {
            const double start = head.gpu_idle_at_launch ? head.launched_at : std::max(d->last_done_at, head.launched_at);
            const float ms = (float)((now - start) * 1e3);
            float& e = d->batch_ms[head.frames];
            if (ms > 0.f && ms < 1e3f) e = e > 0.f ? 0.75f * e + 0.25f * ms : ms;
        }
        d->gpu_free_at = dry_at;
        d->last_done_at = now;
        d->last_done_end = head.first_frame + (uint64_t)head.frames;
    } else {
        d->gpu_free_at = std::min(d->gpu_free_at, dry_at);
        if (w.batch_head) { d->last_done_at = -1.0; d->last_done_end = head.first_frame + (uint64_t)head.frames; }
    }
    const bool idle_after = d->n_launched == d->n_collected + 1;         // this was the last launched frame: the GPU has nothing left
    if (d->pend_n > 0 && d->keep_queued > 0 && (idle_after || (batch_ms_estimate(d, d->pend_n) > 0.f && partial_batch_due(d, now))))
        return lm_launch_pending(d);
    return LM_OK;
}

// The batch has finished: the records of ALL its frames are in pinned memory.  The helper threads prepare the lists of the later frames
// while the calling thread does the first one's (sort_unique = 1, the Detector.match list, is what a stream asks for frame after frame).
static void post_list_jobs(lm_detector* d, const lm_detector::Slot& sl, int slot_index) {
    if (!d->async_collect || d->reference_order || sl.leader != slot_index || sl.batch_n <= 1 || sl.num_work <= 0 || !pool_ready(d)) return;
    for (int b = 1; b < sl.batch_n; ++b) {
        lm_detector::Slot& later = d->slot[(slot_index + b) % lm_detector::kSlots];
        if (!later.pending || !later.launched || later.leader != slot_index || later.prep_queued) continue;
        later.ready.store(0, std::memory_order_relaxed);
        later.prep_queued = true;
        lm_detector::Slot* lp = &later;
        pool_post(d, [lp]() { prepare_list_job(lp); });
    }
}

// The frame's candidate count, published by the last block of its k_dedupe (candidates, distinct, alive, key overflow, tiles, evaluations,
// bytes).  Returns 1 when a buffer overflowed: never drop silently — the capacity grows and the caller reruns the frame.
static int read_counters(lm_detector* d, const lm_detector::Slot& sl, int slot_index, uint64_t* ncand_out) {
    const uint64_t ncand = sl.num_work > 0 ? sl.h_counters[0] : 0;
    *ncand_out = ncand;
    if (ncand > 0xFFFFFFF0ull) return lm_set_error(LM_ERR_INVALID, "too many coarse candidates (%llu)", (unsigned long long)ncand);
    if (ncand > sl.cand_cap || ncand > sl.match_cap) {
        d->cand_cap = std::max<uint32_t>(d->cand_cap, (uint32_t)(ncand + ncand / 4 + 1024));
        d->ingest.used[slot_index] = false;
        return 1;
    }
    return LM_OK;
}

// lm_timings of the frame from its counters and its batch's events; fetches the raw per-candidate records for the callers that want them.
// *nm_out: the records alive before std::unique.
static int fill_timings(lm_detector* d, lm_detector::Slot& sl, int slot_index, int sort_unique, uint64_t ncand, lm_timings* tm_out, uint64_t* nm_out) {
    const lm_detector::Slot& lead = d->slot[sl.leader];
    const unsigned long long* hc = sl.h_counters;
    lm_timings tm{};
    tm.h2d_ms = sl.h2d_ms; tm.templates = sl.num_work; tm.coarse_bytes = sl.coarse_bytes;
    if (d->ingest.used[slot_index]) {   // streamed frame: its H2D ran on the copy stream
        d->ingest.used[slot_index] = false;
        float h = 0.f;
        if (hipEventElapsedTime(&h, d->ingest.t0[slot_index], d->ingest.t1[slot_index]) == hipSuccess) tm.h2d_ms = h;
    }
    const uint64_t evals = sl.num_work > 0 ? hc[5] : 0, lbytes = sl.num_work > 0 ? hc[6] : 0;
    uint64_t nm = 0;
    const Candidate* hm = sl.h_matches;
    if (sl.num_work > 0 && ncand > 0 && (sort_unique == 0 || sort_unique == 3 || d->reference_order))   // the raw per-candidate records, for the callers that want them
        HIP_TRY(hipMemcpy(sl.h_matches, sl.matches_dev, (size_t)ncand * sizeof(Candidate), hipMemcpyDeviceToHost));
    if (sl.num_work == 0) nm = 0;
    else if (sort_unique == 0) { for (uint64_t i = 0; i < ncand; ++i) nm += hm[i].work >= 0; }
    else nm = hc[2];                                   // counted on the device by k_dedupe: no pass over the raw records
    tm.coarse_candidates = (int64_t)ncand;
    d->ncand_hint = (uint64_t)ncand;
    tm.local_evals = (int64_t)evals;
    tm.local_bytes = (int64_t)lbytes;
    tm.matches_pre_unique = (int64_t)nm;
    tm.d2h_ms = 0.f;                                   // the records are stored straight into pinned memory by the refinement
    tm.batch_frames = sl.batch_n;
    // the stage times are those of the LAUNCHES, which serve batch_frames frames: per frame = time / batch_frames
    if (hipEventElapsedTime(&tm.frontend_ms, lead.ev[0], lead.ev[1]) != hipSuccess ||
        hipEventElapsedTime(&tm.coarse_ms, lead.ev[1], lead.ev[3]) != hipSuccess ||
        hipEventElapsedTime(&tm.local_ms, lead.ev[3], lead.ev[4]) != hipSuccess ||
        hipEventElapsedTime(&tm.total_ms, lead.ev[0], lead.ev[4]) != hipSuccess) {
        (void)hipGetLastError();
        tm.frontend_ms = tm.coarse_ms = tm.local_ms = tm.d2h_ms = tm.total_ms = 0.f;
    }
    *tm_out = tm; *nm_out = nm;
    return LM_OK;
}

// The frame's result list.  sort_unique = 0: every record alive (the raw pre-unique multiset); 1 / 2: the records without exact
// duplicates (k_dedupe) — what std::unique would leave of them anyway — canonically sorted + uniqued (1) or as they are (2);
// 3: the reference's own output, permutation and surviving duplicates included (reference_order_list, match_lists.cpp).
static int build_list(const lm_detector::Slot& sl, int sort_unique, uint64_t ncand, uint64_t nm, lm_match** out, size_t* n_out, ListClock* clock) {
    if (sort_unique == 3) {
        std::vector<Candidate> coarse((size_t)ncand);                            // from the buffer the frame was submitted with: d->cand_cap may have grown since
        if (ncand) HIP_TRY(hipMemcpy(coarse.data(), sl.cands, (size_t)ncand * sizeof(Candidate), hipMemcpyDeviceToHost));
        *out = reference_order_list(sl.h_matches, coarse.data(), ncand, (size_t)nm, *sl.work_cls, *sl.work_tid, n_out, clock);
    } else {
        const bool use_distinct = sort_unique != 0 && sl.num_work > 0;
        const uint64_t nd = use_distinct ? sl.h_counters[1] : 0;
        if (use_distinct && (nd > ncand || nd > nm || nm > ncand))
            return lm_set_error(LM_ERR_HIP, "duplicate removal out of step with the refinement (%llu distinct of %llu alive, %llu candidates)",
                                (unsigned long long)nd, (unsigned long long)nm, (unsigned long long)ncand);
        *n_out = canonical_list_of(sl, use_distinct ? sl.h_distinct : sl.h_matches, use_distinct ? nd : ncand, use_distinct ? (size_t)nd : (size_t)nm,
                                   sort_unique == 1, use_distinct, out, clock);
    }
    if (!*out) return lm_set_error(LM_ERR_INVALID, "out of host memory");
    return LM_OK;
}

// Wait for the oldest frame in flight and turn its records into lm_match.  Returns 1 when a buffer
// overflowed (capacity has been raised; the frame has to be submitted again), 0 on success.
int lm_collect_frame(lm_detector* d, int sort_unique, lm_match** out, size_t* n_out) {
    if (d->n_collected == d->n_submitted) return lm_set_error(LM_ERR_INVALID, "no frame in flight");
    const auto t_enter = std::chrono::steady_clock::now();
    const int slot_index = (int)(d->n_collected % lm_detector::kSlots);
    lm_detector::Slot& sl = d->slot[slot_index];
    HIP_TRY(hipSetDevice(d->device));
    int rc;
    if (!sl.launched && (rc = lm_launch_pending(d))) return rc;   // still waiting for its batch to fill: launch what is there
    lm_match* prepared = nullptr;
    size_t prepared_n = 0;
    const bool have_prepared = take_prepared_list(d, sl, &prepared, &prepared_n);
    CollectWait wait{};
    if ((rc = model_before_wait(d, sl, &wait))) return rc;
    // (blocking wait: polling the event with hipEventQuery instead was slower, 0.107 against 0.092 ms per frame — profiles/r04_stream_ab.txt)
    HIP_TRY(hipEventSynchronize(d->slot[sl.leader].done));        // the events are those of the batch's first slot
    const auto t2 = std::chrono::steady_clock::now();
    if (sort_unique == 1) post_list_jobs(d, sl, slot_index);
    if ((rc = model_after_wait(d, wait, host_seconds(t2)))) return rc;
    sl.pending = false;
    while (!d->queued.empty() && d->queued.front().first_frame <= d->n_collected) d->queued.erase(d->queued.begin());   // this frame's batch and everything before it are done
    if (d->xchg.state[slot_index] != 0) {               // exchange work of this frame may still read the slot's buffers
        HIP_TRY(hipStreamSynchronize(d->xchg.stream));
        d->xchg.state[slot_index] = 0;
    }
    ++d->n_collected;
    HIP_TRY(hipGetLastError());
    uint64_t ncand = 0, nm = 0;
    lm_timings tm{};
    if ((rc = read_counters(d, sl, slot_index, &ncand)) || (rc = fill_timings(d, sl, slot_index, sort_unique, ncand, &tm, &nm))) {
        free(prepared);
        return rc;
    }
    if (sort_unique < 0) {                            // pipeline mode: the records stay on the device
        free(prepared);
        d->timings = tm;
        if (out) *out = nullptr;
        if (n_out) *n_out = 0;
        return LM_OK;
    }
    tm.host_submit_ms = ms_between(sl.t0, sl.t1);
    tm.host_wait_ms = ms_between(sl.t1, t2);          // includes whatever the caller did between submit and collect
    if (have_prepared && sort_unique == 1 && !d->reference_order) {   // a helper thread has the list ready: hand it over
        tm.host_collect_ms = sl.prep_collect_ms; tm.host_merge_ms = sl.prep_merge_ms;   // spent on the helper thread
        d->timings = tm;
        *out = prepared; *n_out = prepared_n;
        return LM_OK;
    }
    free(prepared);
    if (sort_unique == 1 && d->reference_order) sort_unique = 3;
    ListClock lc{};
    if ((rc = build_list(sl, sort_unique, ncand, nm, out, n_out, &lc))) return rc;
    tm.host_collect_ms = ms_between(t2, lc.converted);
    tm.host_merge_ms = ms_between(lc.converted, lc.merged);
    if (sort_unique != 3) {
        d->host_prof[5] += std::chrono::duration<double>(t2 - t_enter).count();
        d->host_prof[6] += tm.host_collect_ms * 1e-3; d->host_prof[7] += tm.host_merge_ms * 1e-3;
    }
    d->timings = tm;
    return LM_OK;
}

extern "C" int lm_detector_submit(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    return lm_submit_frame(d, threshold, class_ids, num_class_ids);
}

// ---- live-stream ingest ---------------------------------------------------------------------------
// The per-frame call of a camera / dataset loop (linemod_ros/detect.py:83-138, linemod_and_levelup_test.py:314-327 hand a NEW
// host frame to every match): stage -> H2D on the copy stream -> front end + matching of lm_detector_submit, up to kSlots
// frames in flight; results come back through lm_detector_collect in submission order.
static int ingest_entry(lm_detector* d, int r, size_t n, size_t nsrc) {   // pixels of the aligned frame and of the source
    lm_detector::Ingest& g = d->ingest;
    if (!g.stream) {
        HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
        for (int i = 0; i < lm_detector::kSlots; ++i) { HIP_TRY(hipEventCreate(&g.t0[i])); HIP_TRY(hipEventCreate(&g.t1[i])); }
    }
    g.depth_off = d->use[0] ? (n * d->cch + 15) & ~(size_t)15 : 0;       // the depth image behind the colour image, 16-byte aligned (host entry and device entry alike);
    const size_t bytes = g.depth_off + (d->use[1] ? n * 2 : 0);     // a detector with one modality keeps (and uploads) only that modality's image
    // A source that is not aligned: the pinned entry (and its copy on the device, d_src) has the same layout at the SOURCE size — only those bytes
    // cross PCIe —, the device entry the front end reads keeps the aligned size.
    g.src_depth_off = d->use[0] ? (nsrc * d->cch + 15) & ~(size_t)15 : 0;
    const size_t src_bytes = g.src_depth_off + (d->use[1] ? nsrc * 2 : 0);
    if (g.pinned_bytes[r] < src_bytes) {
        if (g.pinned[r]) (void)hipHostFree(g.pinned[r]);
        g.pinned[r] = nullptr; g.pinned_bytes[r] = 0;
        HIP_TRY(hipHostMalloc(&g.pinned[r], src_bytes, hipHostMallocDefault));
        g.pinned_bytes[r] = src_bytes;
    }
    int rc;
    if ((rc = g.d_rgb[r].ensure(bytes))) return rc;
    if (nsrc != n && (rc = g.d_src[r].ensure(src_bytes + 16))) return rc;   // (+16: k_frame_border fetches the aligned dwords around a unit)
    g.d_depth[r] = d->use[1] ? reinterpret_cast<uint16_t*>(g.d_rgb[r].p + g.depth_off) : nullptr;
    return LM_OK;
}

static int ingest_geometry(lm_detector* d, int width, int height) {
    if (width < 16 || height < 16 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    if (width != d->fW || height != d->fH || d->lm_arena[0].cap == 0) {
        if (d->n_submitted != d->n_collected)
            return lm_set_error(LM_ERR_INVALID, "frame size changes (%dx%d -> %dx%d) with frames in flight: collect them first", d->fW, d->fH, width, height);
        d->frame_valid = false;
        int rc = setup_geometry(d, width, height, true);
        if (rc) return rc;
    }
    return LM_OK;
}

// The ring entry (== result slot: free, its previous frame was collected) for the next frame of this size.
static int ingest_begin(lm_detector* d, int width, int height, int* r) {
    if (d->n_submitted - d->n_collected >= (uint64_t)lm_detector::kSlots)
        return lm_set_error(LM_ERR_INVALID, "%d frames already in flight: call lm_detector_collect first", lm_detector::kSlots);
    HIP_TRY(hipSetDevice(d->device));
    if (width < 16 || height < 16 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    int Wa, Ha, rc = border_resolve(d, width, height, &Wa, &Ha);   // the geometry is that of the aligned size (the source's own under the strict policy)
    if (rc || (rc = ingest_geometry(d, Wa, Ha))) return rc;
    *r = (int)(d->n_submitted % lm_detector::kSlots);
    return ingest_entry(d, *r, (size_t)Wa * Ha, (size_t)width * height);
}

extern "C" int lm_detector_ingest_buffer(lm_detector* d, int width, int height, uint8_t** rgb, uint16_t** depth) {
    if (!d || !rgb || !depth) return lm_set_error(LM_ERR_INVALID, "null argument");
    *rgb = nullptr; *depth = nullptr;
    int r, rc = ingest_begin(d, width, height, &r);
    if (rc) return rc;
    if (d->use[0]) *rgb = (uint8_t*)d->ingest.pinned[r];             // (null stays for a modality outside the set)
    if (d->use[1]) *depth = (uint16_t*)((uint8_t*)d->ingest.pinned[r] + d->ingest.src_depth_off);
    return LM_OK;
}

extern "C" int lm_detector_submit_frame(lm_detector* d, const uint8_t* rgb, const uint16_t* depth, int width, int height, float threshold,
                                        const char* const* class_ids, int num_class_ids) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null argument");
    if ((d->use[0] && !rgb) || (d->use[1] && !depth)) return lm_set_error(LM_ERR_INVALID, "null argument");
    if ((!d->use[0] && rgb) || (!d->use[1] && depth)) return lm_set_error(LM_ERR_INVALID, "a source was given for a modality outside the detector's set");
    int r, rc = ingest_begin(d, width, height, &r);
    if (rc) return rc;
    const size_t n = (size_t)width * height;
    lm_detector::Ingest& g = d->ingest;
    uint8_t* st = (uint8_t*)g.pinned[r];
    const auto tp0 = std::chrono::steady_clock::now();
    const size_t nc = d->use[0] ? n * d->cch : 0, nd = d->use[1] ? n * 2 : 0;
    const bool bordered = width != d->fW || height != d->fH;     // the source is not aligned: the entry holds it as it is, k_frame_border (enqueue_border) writes the frame the front end reads
    const bool copy_2d = bordered && knobs().border_copy2d;      // ... or 2-D copies put its rows into the aligned frame and the kernel writes the margins only
    staged_copy(d, st, rgb, nc, st + g.src_depth_off, (const uint8_t*)depth, nd);  // zero-copy when the caller filled lm_detector_ingest_buffer's pointers
    const auto tp1 = std::chrono::steady_clock::now();
    if (g.reader[r]) {                                            // a resident re-match of the entry's previous frame may still read it (another slot's front end)
        HIP_TRY(hipStreamWaitEvent(g.stream, g.reader[r], 0));
        g.reader[r] = nullptr;
    }
    HIP_TRY(hipEventRecord(g.t0[r], g.stream));
    if (copy_2d) {
        const size_t cw = (size_t)std::min(width, d->fW), ch = (size_t)std::min(height, d->fH);
        if (nc) HIP_TRY(hipMemcpy2DAsync(g.d_rgb[r].p, (size_t)d->fW * d->cch, st, (size_t)width * d->cch, cw * d->cch, ch, hipMemcpyHostToDevice, g.stream));
        if (nd) HIP_TRY(hipMemcpy2DAsync(g.d_depth[r], (size_t)d->fW * 2, st + g.src_depth_off, (size_t)width * 2, cw * 2, ch, hipMemcpyHostToDevice, g.stream));
    } else
    HIP_TRY(hipMemcpyAsync(bordered ? g.d_src[r].p : g.d_rgb[r].p, st, g.src_depth_off + nd, hipMemcpyHostToDevice, g.stream));   // colour + depth: one copy (two cost the copy engine a second set-up: 0.061 -> ~0.05 ms, and the host a call)
    HIP_TRY(hipEventRecord(g.t1[r], g.stream));                   // the batch's front end waits for it (lm_launch_pending)
    const uint8_t* const in_rgb = d->use[0] ? g.d_rgb[r].p : nullptr;
    d->cur_rgb = in_rgb; d->cur_depth = g.d_depth[r];
    d->have_mask[0] = d->have_mask[1] = false;
    d->last_h2d_ms = 0.f;
    d->frame_valid = true;
    const uint64_t before = d->n_submitted;
    const auto tp2 = std::chrono::steady_clock::now();
    rc = slot_begin(d, threshold, class_ids, num_class_ids, in_rgb, g.d_depth[r], d->have_mask, r);
    if (rc) return rc;
    if (d->n_submitted == before + 1) g.used[r] = true;
    if (bordered) { d->slot[r].src_w = width; d->slot[r].src_h = height; d->slot[r].src_in_place = copy_2d; }
    const auto tp3 = std::chrono::steady_clock::now();
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    d->host_prof[0] += 1; d->host_prof[1] += secs(tp0, tp1); d->host_prof[2] += secs(tp1, tp2); d->host_prof[3] += secs(tp2, tp3);
    // A full batch goes out at once; a partial one when the GPU is about to run out of work (partial_batch_due); lm_detector_flush /
    // lm_detector_collect launch what is left.  So the batches are as large as the GPU's backlog allows and no larger.
    {   // how fast the frames arrive (moving average of the gap between submits; a pause counts as 10 ms)
        const double t = host_seconds(tp3);
        if (d->last_submit_at > 0.0) {
            float gap = (float)std::min(10.0, (t - d->last_submit_at) * 1e3);
            // one long gap is a pause, not a change of pace: a tight loop that stops to synchronise (the fence between a warm-up and a timed
            // region, a caller that drains the pipeline now and then) must not look like a camera for its next few frames — they would go
            // out one frame per launch, 0.3 ms of GPU time each.  A stream that has really slowed down is told apart within four frames (the average grows by a quarter per frame).
            if (d->submit_gap_ms > 0.f) gap = std::min(gap, 2.f * d->submit_gap_ms);
            d->submit_gap_ms = d->submit_gap_ms > 0.f ? 0.75f * d->submit_gap_ms + 0.25f * gap : gap;
        }
        d->last_submit_at = t;
    }
    if (d->pend_n >= std::max(1, std::min(d->batch_max, kMaxBatch)) || partial_batch_due(d, host_seconds(tp3))) {
        rc = lm_launch_pending(d);
        const double cost = secs(tp3, std::chrono::steady_clock::now());
        d->host_prof[4] += cost;
        d->launch_cost_ms = 0.75f * d->launch_cost_ms + 0.25f * (float)std::min(1.0, cost * 1e3);
        return rc;
    }
    return LM_OK;
}

// 1 when the refinement of the current bank and frame geometry runs on bit planes (k_local_bits), 0 when on the byte strip planes
// (k_local: single-level pyramids have no refinement; LM_BITPLANES=0; lm_detector_set_paths).  Valid after a match.
extern "C" int lm_detector_refines_on_bit_planes(const lm_detector* d) {
    return d && !d->bank_dirty && (bits_active(d, 1) || wide_active(d, 1)) ? 1 : 0;   // (k_local_bits or k_local_wide)
}

extern "C" int lm_detector_get_paths(const lm_detector* d, int* refine, int* coarse) {
    if (!d || !refine || !coarse) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (d->bank_dirty) return lm_set_error(LM_ERR_INVALID, "no match yet: the paths follow from the bank and the frame geometry");
    const bool bits = bits_active(d, 1);
    if (wide_active(d, 1)) { *refine = 3; *coarse = cwide_active(d, 1) ? 2 : 1; return LM_OK; }
    *refine = bits ? 0 : (d->geom.levels >= 2 && tiles_wanted(d) && tile_plan_possible(d->geom) ? 1 : 2);
    *coarse = cbits_active(d, 1) ? 0 : 1;
    return LM_OK;
}

// Which kernel serves the coarse pass on the pair stream, and which one served the last batch (tests, A/B measurements).
extern "C" int lm_detector_set_coarse_batch(lm_detector* d, int mode) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (mode < -1 || mode > 1) return lm_set_error(LM_ERR_INVALID, "mode must be -1 (the launcher's rule), 0 (k_coarse_bits) or 1 (k_coarse_bits_batch)");
    int rc = lm_launch_pending(d);                      // frames waiting for their batch go out under the setting they were submitted with
    if (rc) return rc;
    d->coarse_batch = mode;
    return LM_OK;
}
extern "C" int lm_detector_get_coarse_batch(const lm_detector* d) { return d && d->coarse_batched ? 1 : 0; }

// The candidate buffers are laid out at the first frame and grow when a frame overflows them: a smaller start is for the tests of the overflow.
extern "C" int lm_detector_set_candidate_capacity(lm_detector* d, int candidates) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (candidates < 1024) return lm_set_error(LM_ERR_INVALID, "candidate capacity must be at least 1024, got %d", candidates);
    if (d->buf_cand_cap) return lm_set_error(LM_ERR_INVALID, "the candidate buffers exist already (%u candidates): set the capacity before the first match", d->buf_cand_cap);
    d->cand_cap = (uint32_t)candidates;
    return LM_OK;
}

// The coarse candidates of a collected frame, as the coarse kernel left them in the frame's slot: {x, y, score bits, work-list index} per slot.
extern "C" int64_t lm_detector_read_candidates(lm_detector* d, uint64_t frame_no, int32_t* dst, int64_t capacity) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (frame_no >= d->n_collected || d->n_submitted - frame_no > (uint64_t)lm_detector::kSlots)
        return lm_set_error(LM_ERR_INVALID, "frame %llu is not collected yet or its slot serves a later frame", (unsigned long long)frame_no);
    const int si = (int)(frame_no % lm_detector::kSlots);
    const lm_detector::Slot& sl = d->slot[si];
    if (sl.cand_cap != d->buf_cand_cap || sl.cands != d->d_cands.p + (size_t)d->buf_cand_cap * si)
        return lm_set_error(LM_ERR_INVALID, "the candidate buffers have been replaced since frame %llu", (unsigned long long)frame_no);
    const int64_t produced = sl.num_work > 0 ? (int64_t)(sl.h_counters[0] & kCandMask) : 0;
    const int64_t n = std::min<int64_t>(std::min<int64_t>(produced, (int64_t)sl.cand_cap), capacity);
    if (dst && n > 0) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipMemcpy(dst, sl.cands, (size_t)n * sizeof(Candidate), hipMemcpyDeviceToHost));
    }
    return produced;
}

extern "C" int lm_detector_flush(lm_detector* d) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    return lm_launch_pending(d);
}

extern "C" int lm_detector_collect(lm_detector* d, int sort_unique, lm_match** out, size_t* n_out) {
    if (!d || !out || !n_out) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr; *n_out = 0;
    int rc = lm_collect_frame(d, sort_unique, out, n_out);
    if (rc == 1)
        return lm_set_error(LM_ERR_OVERFLOW, "candidate buffer overflow: capacity raised to %u, submit the frame again "
                            "(lm_detector_match_resident does this by itself)", d->cand_cap);
    return rc;
}

extern "C" int lm_detector_match_resident(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids,
                                          int sort_unique, lm_match** out, size_t* n_out) {
    if (!d || !out || !n_out) return lm_set_error(LM_ERR_INVALID, "null argument");
    *out = nullptr; *n_out = 0;
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    for (;;) {   // one pass normally; grow-and-rerun when a buffer overflowed
        int rc = lm_submit_frame(d, threshold, class_ids, num_class_ids);
        if (rc) return rc;
        rc = lm_collect_frame(d, sort_unique, out, n_out);
        if (rc != 1) return rc;
    }
}

extern "C" int lm_detector_match(lm_detector* d, const uint8_t* rgb, const uint16_t* depth, int width, int height, float threshold,
                                 const char* const* class_ids, int num_class_ids, const uint8_t* const* masks, lm_match** out,
                                 size_t* n) {
    int rc = lm_detector_set_frame(d, rgb, depth, width, height, masks);
    if (rc) return rc;
    return lm_detector_match_resident(d, threshold, class_ids, num_class_ids, 1, out, n);
}
