// Collecting the frames of the matching path: the wait for a frame's batch, with the launch-timing model (launch_model.h) kept current
// around it, the frame's counters and timings, and its result list — built here or taken over from a helper thread (host_pool.cpp; the
// lists themselves: match_lists.cpp) —, and the entry points that collect, flush, or submit and collect in one call.
#include <stdlib.h>

#include "detector_internal.h"

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
    const unsigned long long* hc = sl->h_counters.p;
    if (sl->num_work > 0 && hc[0] <= sl->cand_cap && hc[0] <= sl->h_matches.cap && hc[1] <= hc[0]) {
        const auto t0 = std::chrono::steady_clock::now();
        ListClock lc{};
        sl->prep_n = canonical_list_of(*sl, sl->h_distinct.p, hc[1], (size_t)hc[1], true, true, &sl->prep, &lc);
        sl->prep_collect_ms = (float)(1e3 * seconds_between(t0, lc.converted)); sl->prep_merge_ms = (float)(1e3 * seconds_between(lc.converted, lc.merged));
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

// The launch-timing model around a collect's wait (LaunchModel::CollectWait): whether the wait will block is the one thing it asks the GPU here.
static int model_before_wait(lm_detector* d, const lm_detector::Slot& sl, LaunchModel::CollectWait* w) {
    *w = d->launch.before_wait(d->n_collected, sl.leader);
    if (!w->batch_head) return LM_OK;
    w->blocked = hipEventQuery(d->slot[sl.leader].done) == hipErrorNotReady;
    (void)hipGetLastError();                              // hipErrorNotReady is not an error
    if (w->blocked && d->launch.due_before_wait(d->pend_n, d->n_collected)) return lm_launch_pending(d);
    return LM_OK;
}
static int model_after_wait(lm_detector* d, const LaunchModel::CollectWait& w, double now) {
    if (d->launch.after_wait(w, now, d->pend_n, d->n_collected, d->n_launched, BatchEvents{d})) return lm_launch_pending(d);
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
    const uint64_t ncand = sl.num_work > 0 ? sl.h_counters.p[0] : 0;
    *ncand_out = ncand;
    if (ncand > 0xFFFFFFF0ull) return lm_set_error(LM_ERR_INVALID, "too many coarse candidates (%llu)", (unsigned long long)ncand);
    if (ncand > sl.cand_cap || ncand > sl.h_matches.cap) {
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
    const unsigned long long* hc = sl.h_counters.p;
    lm_timings tm{};
    tm.h2d_ms = sl.h2d_ms; tm.templates = sl.num_work; tm.coarse_bytes = sl.coarse_bytes;
    if (d->ingest.used[slot_index]) {   // streamed frame: its H2D ran on the copy stream
        d->ingest.used[slot_index] = false;
        float h = 0.f;
        if (hipEventElapsedTime(&h, d->ingest.t0[slot_index], d->ingest.t1[slot_index]) == hipSuccess) tm.h2d_ms = h;
    }
    const uint64_t evals = sl.num_work > 0 ? hc[5] : 0, lbytes = sl.num_work > 0 ? hc[6] : 0;
    uint64_t nm = 0;
    const Candidate* hm = sl.h_matches.p;
    if (sl.num_work > 0 && ncand > 0 && (sort_unique == 0 || sort_unique == 3 || d->reference_order))   // the raw per-candidate records, for the callers that want them
        HIP_TRY(hipMemcpy(sl.h_matches.p, sl.matches_dev, (size_t)ncand * sizeof(Candidate), hipMemcpyDeviceToHost));
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
        (void)hipGetLastError();                          // an event that was never recorded (hipErrorInvalidHandle / NotReady): no timings, not an error
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
        *out = reference_order_list(sl.h_matches.p, coarse.data(), ncand, (size_t)nm, *sl.work_cls, *sl.work_tid, n_out, clock);
    } else {
        const bool use_distinct = sort_unique != 0 && sl.num_work > 0;
        const uint64_t nd = use_distinct ? sl.h_counters.p[1] : 0;
        if (use_distinct && (nd > ncand || nd > nm || nm > ncand))
            return lm_set_error(LM_ERR_HIP, "duplicate removal out of step with the refinement (%llu distinct of %llu alive, %llu candidates)",
                                (unsigned long long)nd, (unsigned long long)nm, (unsigned long long)ncand);
        *n_out = canonical_list_of(sl, use_distinct ? sl.h_distinct.p : sl.h_matches.p, use_distinct ? nd : ncand, use_distinct ? (size_t)nd : (size_t)nm,
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
    LaunchModel::CollectWait wait{};
    if ((rc = model_before_wait(d, sl, &wait))) return rc;
    // (blocking wait: polling the event with hipEventQuery instead was slower, 0.107 against 0.092 ms per frame — profiles/r04_stream_ab.txt)
    HIP_TRY(hipEventSynchronize(d->slot[sl.leader].done));        // the events are those of the batch's first slot
    const auto t2 = std::chrono::steady_clock::now();
    if (sort_unique == 1) post_list_jobs(d, sl, slot_index);
    if ((rc = model_after_wait(d, wait, host_seconds(t2)))) return rc;
    sl.pending = false;
    d->launch.frame_done(d->n_collected);              // this frame's batch and everything before it are done
    if (d->xchg.state[slot_index] != 0) {               // exchange work of this frame may still read the slot's buffers
        HIP_TRY(hipStreamSynchronize(d->xchg_stream));
        d->xchg.state[slot_index] = 0;
    }
    ++d->n_collected;
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
    tm.host_submit_ms = (float)(1e3 * seconds_between(sl.t0, sl.t1));
    tm.host_wait_ms = (float)(1e3 * seconds_between(sl.t1, t2));          // includes whatever the caller did between submit and collect
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
    tm.host_collect_ms = (float)(1e3 * seconds_between(t2, lc.converted));
    tm.host_merge_ms = (float)(1e3 * seconds_between(lc.converted, lc.merged));
    if (sort_unique != 3) {
        d->host_prof[5] += seconds_between(t_enter, t2);
        d->host_prof[6] += tm.host_collect_ms * 1e-3; d->host_prof[7] += tm.host_merge_ms * 1e-3;
    }
    d->timings = tm;
    return LM_OK;
}

extern "C" int lm_detector_submit(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    return lm_submit_frame(d, threshold, class_ids, num_class_ids);
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
    const int64_t produced = sl.num_work > 0 ? (int64_t)(sl.h_counters.p[0] & kCandMask) : 0;
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
