// libamdlinemod.so — host orchestration + C ABI (include/amd_linemod.h) of the MI355X LINE-MOD
// detector.  Mirrors linemodLevelup::Detector (LL.cpp:1663-2146): bank bookkeeping and the greedy
// template extraction on the host, every per-pixel / per-template stage in HIP kernels
// (fe_quant.hip, fe_bits.hip, match_bytes.hip, match_bits.hip).  No CPU fallback: creation fails without a HIP device.
// This file: errors, thread binding, creation / destruction and the small setters and getters.  The frame and the training front
// end are in detector_frame.cpp, the template bank in detector_bank.cpp, the streamed matching path in detector_frontend.cpp,
// detector_launch.cpp, detector_collect.cpp and detector_ingest.cpp (when a partial batch goes out: launch_model.h; the helper threads:
// host_pool.cpp), the host-side result lists and NMS in match_lists.cpp.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <ctype.h>
#include <sched.h>

#include "detector_internal.h"

// ---- errors -----------------------------------------------------------------------------------
static thread_local std::string g_err;
int lm_set_error(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int lm_open_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return lm_set_error(LM_ERR_NO_DEVICE, "no HIP device visible; libamdlinemod has no CPU fallback");
    if (device < 0 || device >= ndev) return lm_set_error(LM_ERR_INVALID, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));
    return LM_OK;
}
extern "C" const char* lm_last_error(void) { return g_err.c_str(); }
extern "C" const char* lm_version(void) { return "amd-linemod 0.1 (gfx950)"; }
// Binds the calling thread to the CPUs next to `device` (its PCI function's local_cpulist in sysfs): pinned staging buffers are then
// allocated, filled and read by the copy engine on the GPU's own NUMA node.  On a two-socket host a process that happens to start on
// the far socket otherwise uploads every frame across the socket link (0.12 instead of 0.065 ms per VGA frame).
extern "C" int lm_bind_thread_near_device(int device, char* cpulist_out, size_t cap) {
    if (cpulist_out && cap) cpulist_out[0] = 0;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) {
        (void)hipGetLastError();                              // the refusal above (an invalid device): not left for the caller's next check
        return lm_set_error(LM_ERR_NO_DEVICE, "no PCI bus id for device %d", device);
    }
    for (char* c = bdf; *c; ++c) *c = (char)tolower(*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/local_cpulist";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return lm_set_error(LM_ERR_IO, "cannot read %s", path.c_str());
    char line[4096] = {0};
    const bool got = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    if (!got) return lm_set_error(LM_ERR_IO, "empty %s", path.c_str());
    cpu_set_t want, have;
    CPU_ZERO(&want);
    int ncpu = 0;
    for (const char* p = line; *p;) {                          // "0-47,96-143"
        if (*p < '0' || *p > '9') { ++p; continue; }
        char* e = nullptr;
        long a = strtol(p, &e, 10), b = a;
        if (*e == '-') b = strtol(e + 1, &e, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET((int)c, &want); ++ncpu; }
        p = e;
    }
    if (ncpu == 0) return lm_set_error(LM_ERR_IO, "no CPUs listed in %s", path.c_str());
    if (sched_getaffinity(0, sizeof(have), &have) == 0) {       // never widen what the caller (cgroup, numactl, taskset) allowed
        cpu_set_t both;
        CPU_AND(&both, &want, &have);
        if (CPU_COUNT(&both) == 0) return lm_set_error(LM_ERR_INVALID, "none of the device's local CPUs (%s) is allowed for this thread", line);
        want = both;
    }
    if (sched_setaffinity(0, sizeof(want), &want) != 0) return lm_set_error(LM_ERR_INVALID, "sched_setaffinity failed");
    if (cpulist_out && cap) {
        size_t n = strlen(line);
        while (n && (line[n - 1] == '\n' || line[n - 1] == ' ')) line[--n] = 0;
        snprintf(cpulist_out, cap, "%s", line);
    }
    return LM_OK;
}

extern "C" int lm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" void lm_free(void* p) { free(p); }

// NORMAL_LUT plane (normal_lut.i): round(atan2(y-10, x-10)/45deg) mod 8, one-hot (z-independent)
static void make_normal_lut(uint8_t lut[400]) {
    const double PI = 3.14159265358979323846;
    for (int iy = 0; iy < 20; ++iy)
        for (int ix = 0; ix < 20; ++ix) {
            double ang = atan2((double)(iy - 10), (double)(ix - 10)) * 180.0 / PI;
            if (ang < 0) ang += 360.0;
            int lab = ((int)floor(ang / 45.0 + 0.5)) % 8;
            lut[iy * 20 + ix] = (uint8_t)(1u << lab);
        }
}

const char* const kModalityName[2] = {"ColorGradient", "DepthNormal"};
int lm_need_both(const lm_detector* d, const char* what) {
    return d->nmod == 2 ? LM_OK : lm_set_error(LM_ERR_INVALID, "%s needs both modalities (this detector has %s only)", what, kModalityName[d->mod_kind[0]]);
}

extern "C" int lm_detector_create(int num_features, const int* T, int num_levels, int device, lm_detector** out) {
    return lm_detector_create_modalities(num_features, T, num_levels, device, nullptr, 0, out);
}

extern "C" int lm_detector_get_modalities(const lm_detector* d, const char* names[2]) {
    if (!d) return 0;
    for (int i = 0; names && i < d->nmod; ++i) names[i] = kModalityName[d->mod_kind[i]];
    return d->nmod;
}

extern "C" int lm_detector_set_colour_channels(lm_detector* d, int channels) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (channels != 1 && channels != 3) return lm_set_error(LM_ERR_INVALID, "colour_channels must be 3 (interleaved colour) or 1 (grey), got %d", channels);
    if (channels == 1 && !d->use[0]) return lm_set_error(LM_ERR_INVALID, "colour_channels = 1 on a detector without the ColorGradient modality: it takes no colour image");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them before changing colour_channels");
    int rc = lm_launch_pending(d);
    if (rc) return rc;
    if (channels == d->cch) return LM_OK;
    d->cch = channels;
    // buffers are sized per channel count: the next frame lays the geometry out again; the resident frame and the parked ones are in the old format
    d->frame_valid = false;
    d->fW = d->fH = 0;
    std::fill(d->slot_w.begin(), d->slot_w.end(), 0);
    return LM_OK;
}

// The border policy: what the matching entry points do with a frame whose size is not aligned to the T grid — the sizes
// the reference refuses at LL.cpp:1136 and 1217-1218.  Training views are not concerned (they take any size).
extern "C" int lm_detector_set_border(lm_detector* d, int policy) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (policy != kBorderStrict && policy != kBorderPad && policy != kBorderCrop)
        return lm_set_error(LM_ERR_INVALID, "unknown border policy %d: 0 (strict), 1 (pad) or 2 (crop)", policy);
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them before changing the border policy");
    d->border = policy;          // the resident frame and the parked ones stay what they are: frames of an aligned size
    return LM_OK;
}

extern "C" int lm_detector_get_border(const lm_detector* d) { return d ? d->border : lm_set_error(LM_ERR_INVALID, "null detector"); }

// The one rule (border_aligned_size, frame_border.h) for this detector's T: the size of the frame buffers a width x height source gets under
// `policy` (-1: the detector's own).  Strict answers with the source size itself, or refuses it with the reference's asserts.
extern "C" int lm_detector_aligned_size(const lm_detector* d, int policy, int width, int height, int* aligned_width, int* aligned_height) {
    if (!d || !aligned_width || !aligned_height) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (policy < 0) policy = d->border;
    if (policy != kBorderStrict && policy != kBorderPad && policy != kBorderCrop)
        return lm_set_error(LM_ERR_INVALID, "unknown border policy %d: 0 (strict), 1 (pad) or 2 (crop)", policy);
    if (width < 16 || height < 16 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    const int* T = d->T_at_level.data();
    const int L = d->pyramid_levels;
    if (policy == kBorderStrict) {
        for (int l = 0; l < L; ++l) {                          // setup_geometry's checks and words
            const int w = width >> l, h = height >> l;
            if (w < 1 || h < 1) return lm_set_error(LM_ERR_INVALID, "image too small for %d pyramid levels", L);
            if (((long)w * h) % 16 != 0)
                return lm_set_error(LM_ERR_INVALID, "(src.rows * src.cols) %% 16 == 0 violated at level %d (%dx%d) [LL.cpp:1136]", l, w, h);
            if (h % T[l] != 0 || w % T[l] != 0)
                return lm_set_error(LM_ERR_INVALID, "response_map.rows/cols %% T == 0 violated at level %d (%dx%d, T=%d) [LL.cpp:1217-1218]", l, w, h, T[l]);
        }
        *aligned_width = width; *aligned_height = height;
        return LM_OK;
    }
    if (!border_aligned_size(T, L, policy, width, height, aligned_width, aligned_height) || *aligned_width > 16384 || *aligned_height > 16384)
        return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    return LM_OK;
}

extern "C" int lm_detector_get_colour_channels(const lm_detector* d) { return d ? d->cch : lm_set_error(LM_ERR_INVALID, "null detector"); }

extern "C" int lm_rgb_to_grey(int device, const uint8_t* rgb, int64_t pixels, uint8_t* grey) {
    if (pixels < 0 || (pixels && (!rgb || !grey))) return lm_set_error(LM_ERR_INVALID, "bad argument");
    if (!pixels) return LM_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint8_t> in, out;
    int rc = in.ensure((size_t)pixels * 3);
    if (!rc) rc = out.ensure((size_t)pixels);
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpy(in.p, rgb, (size_t)pixels * 3, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_rgb_to_grey(in.p, out.p, (size_t)pixels, nullptr);
        if (e == hipSuccess) e = hipMemcpy(grey, out.p, (size_t)pixels, hipMemcpyDeviceToHost);   // (synchronises with the null stream)
    }
    in.release(); out.release();
    if (rc) return rc;
    return e == hipSuccess ? LM_OK : lm_set_error(LM_ERR_HIP, "lm_rgb_to_grey: %s", hipGetErrorString(e));
}

// The events a detector owns from its creation on (those of exchange.cpp and detector_slabs.cpp come with their first use); the ingest
// ring's only beside its stream.  Returns the step that failed (lm_last_error: the HIP call), or null.
static const char* create_events(lm_detector* d) {
    if (d->ingest_stream)
        for (int i = 0; i < lm_detector::kSlots; ++i)
            if (d->ingest.t0[i].ensure() || d->ingest.t1[i].ensure()) return "the ingest ring's timing events";
    for (auto& ev : d->ev)
        if (ev.ensure()) return "the frame events";
    for (auto& sl : d->slot) {
        for (auto& e : sl.ev)
            if (e.ensure(hipEventDisableSystemFence)) return "a slot's timing events";   // timing only: nobody synchronises on them, and a default record costs the queue a cache write-back + invalidate (5-6 us between two kernels; sl.done keeps the fence)
        if (sl.done.ensure(hipEventDisableTiming) || sl.fe_done.ensure(hipEventDisableTiming)) return "a slot's done / fe_done events";
    }
    return nullptr;
}

extern "C" int lm_detector_create_modalities(int num_features, const int* T, int num_levels, int device, const char* const* modalities,
                                             int num_modalities, lm_detector** out) {
    if (!out) return lm_set_error(LM_ERR_INVALID, "out is null");
    *out = nullptr;
    // the sets the kernels serve: the reference's pair in its order (LL.cpp:1684-1692), or one of the two alone
    int nmod = 2, kind0 = 0;
    if (modalities) {
        nmod = num_modalities;
        bool ok = nmod == 1 || nmod == 2;
        for (int i = 0; ok && i < nmod; ++i) ok = modalities[i] && (!strcmp(modalities[i], kModalityName[0]) || !strcmp(modalities[i], kModalityName[1]));
        if (ok && nmod == 2) ok = !strcmp(modalities[0], kModalityName[0]) && !strcmp(modalities[1], kModalityName[1]);
        if (!ok)
            return lm_set_error(LM_ERR_INVALID, "modalities must be [ColorGradient, DepthNormal], [ColorGradient] or [DepthNormal] "
                                "(Modality::create, LL.cpp:320-328, knows these two; no duplicates)");
        kind0 = !strcmp(modalities[0], kModalityName[1]) ? 1 : 0;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return lm_set_error(LM_ERR_NO_DEVICE, "no HIP device visible (%s); libamdlinemod has no CPU fallback",
                            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return lm_set_error(LM_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);
    if (T && (num_levels < 1 || num_levels > kMaxLevels))
        return lm_set_error(LM_ERR_INVALID, "num_levels must be in 1..%d", kMaxLevels);
    lm_detector* d = new lm_detector();
    d->nmod = nmod;
    if (nmod == 1) { d->mod_kind[0] = kind0; d->mod_kind[1] = -1; d->use[kind0] = true; d->use[1 - kind0] = false; }
    if (num_features > 0) d->num_features = num_features;
    if (T) {
        d->T_at_level.assign(T, T + num_levels);
        for (int t : d->T_at_level)
            if (t < 1) { delete d; return lm_set_error(LM_ERR_INVALID, "T must be >= 1"); }
    }
    d->pyramid_levels = (int)d->T_at_level.size();
    if ((d->num_features >> (d->pyramid_levels - 1)) < 1) {       // every level halves it: the last one would select 0 features
        const int nf = d->num_features, L = d->pyramid_levels;
        delete d;
        return lm_set_error(LM_ERR_INVALID, "num_features %d leaves no feature at the last of %d pyramid levels (num_features /= 2 per level, "
                            "LL.cpp:560; LL.cpp:632 then divides by zero)", nf, L);
    }
    d->device = device;
    // Four streams: front end | coarse pass | refinement | duplicate removal + multi-GPU exchange.  Streams that share a hardware
    // queue run in submission order, so they must land on different queues.  The HIP runtime pools its hardware queues
    // (GPU_MAX_HW_QUEUES, 4 by default) PER PRIORITY and hands a new stream the least used queue of its pool; a process that
    // holds other streams (torch's default stream, RCCL's high-priority one) competes for the same pools.  Spread over all three:
    // front end and coarse pass HIGH (short kernels on the latency path of the next frame), the refinement — the one long kernel,
    // which fills whatever the short ones leave free — alone in the LOW pool, duplicate removal + exchange NORMAL.
    // Measured, ms/frame, stand-alone process / torch + RCCL process (world 1, device exchange):
    //   everything normal 0.223 / 0.34 (front end and matching serialised on one queue);   this assignment 0.223 / 0.222;
    //   coarse or front end at normal priority 0.223 / 0.230-0.237 (coarse shares a queue: half overlapped);
    //   exchange at low priority: its five dependent steps take ~50 us each and the frames in flight no longer hide the latency;
    //   GPU_MAX_HW_QUEUES=8: 0.223 / 0.40-0.50 (more queues than the hardware runs at once: they are time-sliced).
    // LM_STREAM_PRIO="f-mx" overrides (digits: 0 normal, 1 low, 2 high; position 0 = frame / front-end stream, 2 = matching stream, 3 = exchange
    // stream; position 1 belonged to the coarse stream that round 5 removed and is ignored).
    int prio_least = 0, prio_greatest = 0;
    if (hipSetDevice(device) == hipSuccess) (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    int prio[4] = {prio_greatest, prio_greatest, prio_least, 0};
    if (const char* pe = getenv("LM_STREAM_PRIO"))
        for (int i = 0; i < 4 && pe[i]; ++i) prio[i] = pe[i] == '1' ? prio_least : (pe[i] == '2' ? prio_greatest : 0);
    if (hipSetDevice(device) != hipSuccess || d->stream.ensure(hipStreamNonBlocking, prio[0]) || d->mstream.ensure(hipStreamNonBlocking, prio[2]) ||
        d->xchg_stream.ensure(hipStreamNonBlocking, prio[3])) {
        delete d;
        return lm_set_error(LM_ERR_NO_DEVICE, "cannot initialise HIP device %d", device);
    }
    // the copy stream of the live-stream ingest too, now: every stream of the detector takes its hardware queue before anything created
    // later (torch, RCCL) does.  The one creation that may fail: the first streamed frame tries again (ingest_entry).
    (void)d->ingest_stream.ensure(hipStreamNonBlocking);
    if (const char* step = create_events(d)) {
        const std::string why = lm_last_error();
        delete d;
        return lm_set_error(LM_ERR_HIP, "lm_detector_create: %s: %s", step, why.c_str());
    }
    d->work_cls = std::make_shared<std::vector<int32_t>>();
    d->work_tid = std::make_shared<std::vector<int32_t>>();
    if (knobs().frame_batch > 0) d->launch.batch_max = std::min(knobs().frame_batch, kMaxBatch);
    if (knobs().batch_queue > 0) d->launch.keep_queued = knobs().batch_queue;
    if (knobs().launch_slack_us > 0) d->launch.launch_slack_ms = knobs().launch_slack_us * 1e-3f;
    d->launch.first_batch = knobs().first_batch;
    if (const char* ac = getenv("LM_ASYNC_COLLECT")) d->async_collect = ac[0] && ac[0] != '0';
    if (const char* ht = getenv("LM_HOST_THREADS")) d->pool.threads = std::max(0, std::min(8, atoi(ht)));
    if (const char* tl = getenv("LM_TILES")) d->use_tiles = tl[0] && tl[0] != '0';
    if (const char* ro = getenv("LM_REFERENCE_ORDER")) d->reference_order = ro[0] && ro[0] != '0';
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) d->num_cus = prop.multiProcessorCount;
    }
    uint8_t lut[400];
    make_normal_lut(lut);
    if (const hipError_t e = upload_normal_lut(lut); e != hipSuccess) {
        delete d;
        return lm_set_error(LM_ERR_HIP, "lm_detector_create: upload_normal_lut: %s", hipGetErrorString(e));
    }
    *out = d;
    return LM_OK;
}

extern "C" void lm_detector_destroy(lm_detector* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)lm_launch_pending(d);
    pool_stop(d);
    for (auto& sl : d->slot) { free(sl.prep); sl.prep = nullptr; }
    (void)hipStreamSynchronize(d->stream);
    if (d->mstream) (void)hipStreamSynchronize(d->mstream);
    if (d->xchg_stream) (void)hipStreamSynchronize(d->xchg_stream);
    delete d;                                                         // every buffer and event, then the streams (detector_internal.h): device selected, streams idle
}

extern "C" int lm_detector_max_in_flight(void) { return lm_detector::kSlots; }

extern "C" int lm_detector_set_reference_order(lm_detector* d, int on) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    d->reference_order = on != 0;
    return LM_OK;
}

extern "C" int lm_detector_set_paths(lm_detector* d, int refine, int coarse) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (refine < 0 || refine > 3 || coarse < 0 || coarse > 2)
        return lm_set_error(LM_ERR_INVALID, "refine must be 0 (bit planes), 1 (tiles), 2 (per candidate) or 3 (wide bit planes), coarse 0 (bit planes), 1 (bytes) or 2 (wide bit planes)");
    if (coarse == 2 && refine != 3) return lm_set_error(LM_ERR_INVALID, "coarse 2 (wide bit planes) plans no tiles: it needs refine 3 (wide bit planes)");
    if (refine == 3 && d->shard_world > 1) return lm_set_error(LM_ERR_INVALID, "the wide paths are not available on a sharded detector (%d ranks)", d->shard_world);
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    int rc = lm_launch_pending(d);
    if (rc) return rc;
    d->refine_mode = refine; d->coarse_mode = coarse;
    return LM_OK;
}

extern "C" int lm_detector_set_response_table(lm_detector* d, const uint8_t r[5]) {
    if (!d || !r) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (r[0] != 4) return lm_set_error(LM_ERR_INVALID, "response table: r[0] must be 4 (the score is raw * 100 / (4 * features)), got %d", (int)r[0]);
    for (int k = 1; k < 5; ++k)
        if (r[k] > r[k - 1]) return lm_set_error(LM_ERR_INVALID, "response table: must not increase with the distance, r[%d] = %d > r[%d] = %d", k, (int)r[k], k - 1, (int)r[k - 1]);
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them before changing the response table");
    int rc = lm_launch_pending(d);
    if (rc) return rc;
    for (int k = 0; k < 5; ++k) d->resp_table[k] = r[k];
    d->resp = resp_pack(r);
    d->resp_low_weight = resp_low_weight(r);
    d->resp_two_planes = resp_two_planes(r);
    // The byte planes the last front end left belong to the old table: lm_detector_read_stage kinds 2 / 3 build them again, from the quantised
    // maps, under the new one.  (The bit planes, kinds 4 / 5, stay what the last match read until the next match rewrites them.)
    d->fe_bytes_low = d->fe_bytes_top = false;
    return LM_OK;
}

extern "C" int lm_detector_train_stats(const lm_detector* d, int64_t out[4]) {
    if (!d || !out) return lm_set_error(LM_ERR_INVALID, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = d->train_stats[i];
    return LM_OK;
}

extern "C" int lm_detector_bit_arena_bytes(const lm_detector* d, uint64_t* strip_records, uint64_t* pair_stream) {
    if (!d || !strip_records || !pair_stream) return lm_set_error(LM_ERR_INVALID, "null argument");
    *strip_records = *pair_stream = 0;
    for (int s = 0; s < lm_detector::kSlots; ++s) {                 // what is allocated, over all result slots (DevBuf holds bytes)
        *strip_records += d->bits_arena[s].cap;
        *pair_stream += d->cbits_arena[s].cap;
    }
    return LM_OK;
}

extern "C" int lm_detector_wide_arena_bytes(const lm_detector* d, uint64_t* strip_records, uint64_t* pair_stream) {
    if (!d || !strip_records || !pair_stream) return lm_set_error(LM_ERR_INVALID, "null argument");
    *strip_records = *pair_stream = 0;
    for (int s = 0; s < lm_detector::kSlots; ++s) {                 // the second set: nothing until a wide table has run on a wide path
        *strip_records += d->wbits_arena[s].cap;
        *pair_stream += d->wcbits_arena[s].cap;
    }
    return LM_OK;
}

extern "C" int lm_detector_get_response_table(const lm_detector* d, uint8_t r[5]) {
    if (!d || !r) return lm_set_error(LM_ERR_INVALID, "null argument");
    for (int k = 0; k < 5; ++k) r[k] = d->resp_table[k];
    return LM_OK;
}

extern "C" int lm_detector_set_direct_bits(lm_detector* d, int on) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (d->n_submitted != d->n_collected) return lm_set_error(LM_ERR_INVALID, "frames in flight: collect them first");
    int rc = lm_launch_pending(d);
    if (rc) return rc;
    d->fe_direct = on != 0;
    d->fe_keep_top = (on & 2) != 0;  // tests: the pair stream stays readable after the match (lm_detector_read_stage kind 5) and is cleared before the next frame instead
    d->fe_top_mode = (on & 4) ? 1 : ((on & 8) ? 2 : 0);   // tests: 4 = the OR-ing writer of the pair stream also where whole bytes / dwords could be stored, 8 = no pixel tiles (the whole-dword writer where the geometry allows it)
    return LM_OK;
}

extern "C" int lm_detector_set_batch(lm_detector* d, int frames) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (frames < 1 || frames > kMaxBatch) return lm_set_error(LM_ERR_INVALID, "frames per launch must be in [1, %d]", kMaxBatch);
    int rc = lm_launch_pending(d);
    if (rc) return rc;
    d->launch.batch_max = frames;
    return LM_OK;
}

extern "C" int lm_detector_get_batch(const lm_detector* d) { return d ? d->launch.batch_max : 0; }

extern "C" int lm_detector_host_profile(lm_detector* d, double* out8, int reset) {
    if (!d || !out8) return lm_set_error(LM_ERR_INVALID, "null argument");
    for (int i = 0; i < 8; ++i) { out8[i] = d->host_prof[i]; if (reset) d->host_prof[i] = 0; }
    return LM_OK;
}

extern "C" int lm_detector_set_async_collect(lm_detector* d, int on) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    d->async_collect = on != 0;       // frames already launched keep what they were launched with
    return LM_OK;
}

extern "C" int lm_detector_set_batch_queue(lm_detector* d, int batches) {
    if (!d) return lm_set_error(LM_ERR_INVALID, "null detector");
    if (batches < 0 || batches > lm_detector::kSlots) return lm_set_error(LM_ERR_INVALID, "batches queued on the GPU must be in [0, %d]", lm_detector::kSlots);
    d->launch.keep_queued = batches;
    return LM_OK;
}

extern "C" int lm_detector_last_timings(const lm_detector* d, lm_timings* t) {
    if (!d || !t) return lm_set_error(LM_ERR_INVALID, "null argument");
    *t = d->timings;
    return LM_OK;
}
