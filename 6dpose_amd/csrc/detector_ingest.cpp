// Live-stream ingest of the matching path.
// The per-frame call of a camera / dataset loop (linemod_ros/detect.py:83-138, linemod_and_levelup_test.py:314-327 hand a NEW
// host frame to every match): stage -> H2D on the copy stream -> front end + matching of lm_detector_submit, up to kSlots
// frames in flight; results come back through lm_detector_collect in submission order.  A submit takes a result slot (slot_begin,
// detector_launch.cpp) and asks the launch-timing model (launch_model.h) whether the frames waiting for their batch go out now.
#include "detector_internal.h"

static int ingest_entry(lm_detector* d, int r, size_t n, size_t nsrc) {   // pixels of the aligned frame and of the source
    lm_detector::Ingest& g = d->ingest;
    int rc = d->ingest_stream.ensure(hipStreamNonBlocking);          // all three kept where lm_detector_create made them; a call that fails part-way is continued by the next
    if (!rc) rc = g.t0[r].ensure();
    if (!rc) rc = g.t1[r].ensure();
    if (rc) return rc;
    g.depth_off = d->use[0] ? (n * d->cch + 15) & ~(size_t)15 : 0;       // the depth image behind the colour image, 16-byte aligned (host entry and device entry alike);
    const size_t bytes = g.depth_off + (d->use[1] ? n * 2 : 0);     // a detector with one modality keeps (and uploads) only that modality's image
    // A source that is not aligned: the pinned entry (and its copy on the device, d_src) has the same layout at the SOURCE size — only those bytes
    // cross PCIe —, the device entry the front end reads keeps the aligned size.
    g.src_depth_off = d->use[0] ? (nsrc * d->cch + 15) & ~(size_t)15 : 0;
    const size_t src_bytes = g.src_depth_off + (d->use[1] ? nsrc * 2 : 0);
    if ((rc = g.pinned[r].ensure(src_bytes)) || (rc = g.d_rgb[r].ensure(bytes))) return rc;
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
    if (d->use[0]) *rgb = d->ingest.pinned[r].p;                      // (null stays for a modality outside the set)
    if (d->use[1]) *depth = (uint16_t*)(d->ingest.pinned[r].p + d->ingest.src_depth_off);
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
    uint8_t* st = g.pinned[r].p;
    const auto tp0 = std::chrono::steady_clock::now();
    const size_t nc = d->use[0] ? n * d->cch : 0, nd = d->use[1] ? n * 2 : 0;
    const bool bordered = width != d->fW || height != d->fH;     // the source is not aligned: the entry holds it as it is, k_frame_border (enqueue_border) writes the frame the front end reads
    const bool copy_2d = bordered && knobs().border_copy2d;      // ... or 2-D copies put its rows into the aligned frame and the kernel writes the margins only
    staged_copy(d, st, rgb, nc, st + g.src_depth_off, (const uint8_t*)depth, nd);  // zero-copy when the caller filled lm_detector_ingest_buffer's pointers
    const auto tp1 = std::chrono::steady_clock::now();
    if (g.reader[r]) {                                            // a resident re-match of the entry's previous frame may still read it (another slot's front end)
        HIP_TRY(hipStreamWaitEvent(d->ingest_stream, g.reader[r], 0));
        g.reader[r] = nullptr;
    }
    HIP_TRY(hipEventRecord(g.t0[r], d->ingest_stream));
    if (copy_2d) {
        const size_t cw = (size_t)std::min(width, d->fW), ch = (size_t)std::min(height, d->fH);
        if (nc) HIP_TRY(hipMemcpy2DAsync(g.d_rgb[r].p, (size_t)d->fW * d->cch, st, (size_t)width * d->cch, cw * d->cch, ch, hipMemcpyHostToDevice, d->ingest_stream));
        if (nd) HIP_TRY(hipMemcpy2DAsync(g.d_depth[r], (size_t)d->fW * 2, st + g.src_depth_off, (size_t)width * 2, cw * 2, ch, hipMemcpyHostToDevice, d->ingest_stream));
    } else
    HIP_TRY(hipMemcpyAsync(bordered ? g.d_src[r].p : g.d_rgb[r].p, st, g.src_depth_off + nd, hipMemcpyHostToDevice, d->ingest_stream));   // colour + depth: one copy (two cost the copy engine a second set-up: 0.061 -> ~0.05 ms, and the host a call)
    HIP_TRY(hipEventRecord(g.t1[r], d->ingest_stream));                   // the batch's front end waits for it (lm_launch_pending)
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
    d->host_prof[0] += 1; d->host_prof[1] += seconds_between(tp0, tp1); d->host_prof[2] += seconds_between(tp1, tp2); d->host_prof[3] += seconds_between(tp2, tp3);
    d->launch.submitted(host_seconds(tp3));
    if (d->launch.batch_full(d->pend_n) || d->launch.partial_batch_due(d->pend_n, d->n_launched == d->n_collected, host_seconds(tp3), BatchEvents{d})) {
        rc = lm_launch_pending(d);
        const double cost = seconds_between(tp3, std::chrono::steady_clock::now());
        d->host_prof[4] += cost;
        d->launch.launch_cost(cost);
        return rc;
    }
    return LM_OK;
}
