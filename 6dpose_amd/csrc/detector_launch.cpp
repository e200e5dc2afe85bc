// The launch of a batch of the matching path: which kernels serve a bank and a geometry (the path predicates, and the getters and setters
// that report or choose them), the grids, the result slot a submitted frame takes (slot_begin), and lm_launch_pending — ONE front end
// (detector_frontend.cpp), coarse pass, refinement and duplicate removal for the frames that wait for their batch.  When a partial batch
// goes out is decided by the launch-timing model (launch_model.h); the results come back through detector_collect.cpp.
#include "detector_internal.h"

static int sync_all_streams(lm_detector* d) {
    HIP_TRY(hipStreamSynchronize(d->stream)); HIP_TRY(hipStreamSynchronize(d->mstream));
    if (d->xchg_stream) HIP_TRY(hipStreamSynchronize(d->xchg_stream));
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
static int bits_grid(lm_detector* d) {
    if (knobs().local_blocks > 0) return knobs().local_blocks;
    return d->num_cus * 4;
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
    HIP_TRY(hipHostGetDevicePointer((void**)&F.distinct, sl.h_distinct.p, 0));
    HIP_TRY(hipHostGetDevicePointer((void**)&F.final_host, sl.h_counters.p, 0));
    *out = F;
    return LM_OK;
}

// Takes the next result slot for a frame (resident frame or ingest ring entry `ring`) and queues it behind the frames that wait for
// their batch; nothing is launched here.  The frames of a batch share threshold, work list and buffers, so a change of any of them
// launches what is waiting first.
int slot_begin(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids, const uint8_t* rgb, const uint16_t* depth,
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
    if ((rc = sl.h_counters.ensure(8)) || (rc = sl.h_matches.ensure(d->buf_cand_cap)) || (rc = sl.h_distinct.ensure(d->buf_cand_cap))) return rc;
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
    hipStream_t s;                            // (not owned: the detector's) every kernel of a batch on the matching stream (one queue; the end of a stage is the start of the next)
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
    B.cap = std::min<uint32_t>((uint32_t)lead.h_matches.cap, d->buf_cand_cap);
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
static int pack_bit_planes(lm_detector* d, Batch& B) {
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
            for (int l = 0; l + 1 < d->geom.levels; ++l) HIP_TRY(launch_pack_wide(B.bb, B.wb, B.nb, d->geom.lv[l], B.s));
        } else
        if (!B.direct_low)
            for (int l = 0; l + 1 < d->geom.levels; ++l) HIP_TRY(launch_pack_bits(B.bb, B.nb, d->geom.lv[l], B.s));
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
            HIP_TRY(launch_pack_top_wide(B.tb, B.wt, B.nb, d->cbits_byte0, d->cbits_npairs, B.s));
        } else
        if (!B.direct_top) HIP_TRY(launch_pack_top(B.tb, B.nb, d->cbits_byte0, d->cbits_npairs, B.s));
    }
    return LM_OK;
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
        if (sl.ring < 0 && d->ingest_stream)
            for (int r = 0; r < lm_detector::kSlots; ++r)
                if (d->ingest.d_rgb[r].p && (sl.in_rgb ? sl.in_rgb == d->ingest.d_rgb[r].p : (const void*)sl.in_depth == (const void*)d->ingest.d_rgb[r].p)) d->ingest.reader[r] = lead.fe_done;   // (a depth-only entry starts with the depth image)
    }
    return LM_OK;
}

static int enqueue_coarse(lm_detector* d, const Batch& B) {
    // the counters are zero on entry (reset by the slots' previous k_dedupe)
    { LM_CLOCK("launch_coarse");
    if (B.cwide) HIP_TRY(launch_coarse_wide(B.fb, B.tb, B.wt, d->geom, B.bank, B.num_work, B.threshold, d->buf_cand_cap, d->cbits_byte0, d->cbits_max_nf, B.s));
    else if (B.parts) { d->coarse_batched = false; HIP_TRY(launch_coarse_parts(B.fb, B.tb, d->geom, B.bank, B.pd, B.num_work, B.threshold, d->buf_cand_cap, d->cbits_byte0, d->cbits_max_nf, d->resp_low_weight, B.s)); }
    else if (B.cbits) HIP_TRY(launch_coarse_bits(B.fb, B.tb, d->geom, B.bank, B.num_work, B.threshold, d->buf_cand_cap, d->cbits_byte0, d->cbits_max_nf, d->resp_low_weight, B.s, &d->coarse_batched, d->coarse_batch));
    else HIP_TRY(launch_coarse(B.fb, d->geom, B.bank, B.num_work, B.threshold, d->buf_cand_cap, B.tile_cap, B.s));
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
        if (B.wide) HIP_TRY(launch_local_wide(B.fb, B.bb, B.wb, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, bits_grid(d), d->bits_max_nf, B.s));
        else if (B.parts) HIP_TRY(launch_local_parts(B.fb, B.bb, d->geom, B.bank, B.pd, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, bits_grid(d), d->bits_max_nf, d->resp_low_weight, B.s));
        else HIP_TRY(launch_local_bits(B.fb, B.bb, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, bits_grid(d), d->bits_max_nf, d->resp_low_weight, B.s)); }
        if (B.bb.top_clear_units)     // the pair streams this launch zeroes again are clean for their slots' next frames
            for (int b = 0; b < B.nb; ++b)
                if (B.bb.top_clear[b]) d->cbits_clean[B.slot(b)] = true;
        if (!d->bits_all_in)          // candidates whose windows leave their planes (marked in todo): k_local's per-candidate path
            HIP_TRY(launch_local(B.fb_rest, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, B.tile_cap, d->num_cus * 2, B.s));
    } else
    if (B.num_work > 0)
        HIP_TRY(launch_local(B.fb, d->geom, B.bank, d->buf_cand_cap, B.threshold, B.cap, dedupe_slots, B.tile_cap, local_grid(d, B.nb), B.s));
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
        HIP_TRY(launch_dedupe(B.fb, d->buf_cand_cap, dedupe_table_slots(d->buf_cand_cap), d->d_work_cls.p, d->d_work_tid.p, dedupe_blocks, B.s));
    }
    else
        for (int b = 0; b < B.nb; ++b) HIP_TRY(hipMemsetAsync(B.fb.f[b].final_dev, 0, 8 * sizeof(unsigned long long), B.s));   // nothing searched: no records for NMS / exchange
    { LM_CLOCK("record done"); HIP_TRY(hipEventRecord(d->slot[B.first].done, B.s)); }
    return LM_OK;
}

// The slots are launched; the batch joins the queue of the launch-timing model.
static void batch_launched(lm_detector* d, const Batch& B) {
    const auto now = std::chrono::steady_clock::now();
    for (int b = 0; b < B.nb; ++b) {
        lm_detector::Slot& sl = d->slot[B.slot(b)];
        sl.launched = true; sl.leader = B.first; sl.batch_n = B.nb; sl.t1 = now;
    }
    d->launch.batch_launched(d->n_launched, B.first, B.nb, host_seconds(now), BatchEvents{d});
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
    { LM_CLOCK("step bits tables+ev1"); if ((rc = pack_bit_planes(d, B)) || (rc = record_front_end(d, B))) return rc; }
    { LM_CLOCK("step coarse"); if ((rc = enqueue_coarse(d, B))) return rc; }
    { LM_CLOCK("step refine"); if ((rc = enqueue_match(d, B))) return rc; }
    { LM_CLOCK("step dedupe+done"); if ((rc = enqueue_dedupe(d, B))) return rc; }
    batch_launched(d, B);
    return LM_OK;
}

// The detector's current frame (lm_detector_set_frame / select_frame, or the frame a previous submit_frame left current) as a
// batch of one, launched at once.
int lm_submit_frame(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids) {
    int rc;
    if ((rc = lm_need_resident(d, false))) return rc;
    if ((rc = lm_launch_pending(d))) return rc;               // frames waiting for their batch go first (results come back in order)
    if ((rc = slot_begin(d, threshold, class_ids, num_class_ids, d->cur_rgb, d->cur_depth, d->have_mask, -1))) return rc;
    return lm_launch_pending(d);
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
