// The launch-timing model of the streamed path: when does a streamed frame that does not fill its batch go out?  Plain arithmetic over
// host clocks (seconds, steady_clock) and frame counts, with no HIP in it: it compiles with a plain host compiler, and
// tests/cpp/launch_model_cases.cpp runs every rule below on a CPU.  The detector holds one by value (lm_detector::launch) and tells it
// of every submit, launch and collect; whether a launched batch has finished stays an event query in the detector's code
// (BatchEvents, detector_internal.h), which the model receives as `gpu` and asks lazily, only on the branches that need the answer.
//
// The GPU must never wait for a batch to fill, and a batch launched early is a small one (a lone frame costs ~2.5x its share of a
// batch of four).  The model therefore keeps an estimate of when the GPU will have finished what it was given (`gpu_free_at`: launch
// times + the measured duration of batches of each size, corrected whenever a collect sees a batch finish) and launches a partial
// batch when that moment is closer than `launch_slack_ms` — the enqueue latency of a batch — either at a submit or just before a
// collect blocks.  Without a measured duration yet the rule is the backlog in batches: launch while fewer than `keep_queued` are
// unfinished.  keep_queued = 0 switches both off (batches of exactly batch_max frames; flush / collect launch what is left).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace lm {

struct __attribute__((visibility("hidden"))) LaunchModel {   // (hidden: its inline functions add nothing to the dynamic symbols of a library that holds one)
    static constexpr int kMaxFrames = 8;            // frames of the largest batch (= kMaxBatch: detector_internal.h asserts it)
    struct QueuedBatch {
        uint64_t first_frame;                       // index of the batch's first frame
        int slot, frames;                           // its leader slot, its size
        double launched_at;                         // host clock (seconds, steady_clock)
        bool gpu_idle_at_launch;                    // nothing unfinished before it: it started when it was launched
    };
    std::vector<QueuedBatch> queued;                // launched batches the GPU may still be working on, oldest first
    int batch_max = 8;                              // frames per launch in stream mode (lm_detector_set_batch, LM_FRAME_BATCH; <= kMaxFrames).  8 since round 4: 0.074 against 0.089 ms per frame over 200 steps, the same at 20 (profiles/r04_stream_ab.txt)
    int first_batch = 3;                            // LM_FIRST_BATCH: frames an idle GPU waits for before a partial batch goes out while the caller submits in a tight loop
    int keep_queued = 2;                            // LM_BATCH_QUEUE
    float batch_ms[kMaxFrames + 1] = {};            // measured GPU time of a batch of n frames (moving average); 0 = not seen yet
    double gpu_free_at = 0.0;                       // estimate, host clock
    double last_done_at = -1.0;                     // when the most recently collected batch finished, if a collect saw it happen (-1: unknown)
    uint64_t last_done_end = 0;                     // index of the frame after that batch
    float launch_slack_ms = 0.15f;                  // LM_LAUNCH_SLACK_US
    double last_submit_at = 0.0;                    // lm_detector_submit_frame: host clock of the previous call,
    float submit_gap_ms = 0.f;                      // moving average of the gap between calls (0 = no second call yet: treated as sparse),
    float launch_cost_ms = 0.1f;                    // and of the host time one lm_launch_pending takes
    bool early_batch_used = false;                  // the burst's one early (partial) batch of a tight stream has gone out (partial_batch_due)

    // `gpu` in the calls below: gpu.finished(slot) — has the batch whose leader is `slot` finished on the GPU (the detector: an event
    // query) —, and gpu.queries_end(), called once after every run of such queries, of none too (the detector: clears "not ready", which
    // is not an error).

    // Batches launched and not yet finished on the GPU (a query per finished batch, none in the steady state of a full queue).
    template <class Gpu>
    int batches_queued(Gpu&& gpu) {
        while (!queued.empty() && gpu.finished(queued.front().slot)) queued.erase(queued.begin());
        gpu.queries_end();
        return (int)queued.size();
    }

    // GPU time of a batch of n frames: measured, or scaled from the nearest measured size (a batch costs about four frames' worth of
    // fixed latency + its frames), or 0 when nothing has been measured yet.
    float batch_ms_estimate(int n) const {
        if (batch_ms[n] > 0.f) return batch_ms[n];
        for (int k = 1; k <= kMaxFrames; ++k)
            for (int m : {n - k, n + k})
                if (m >= 1 && m <= kMaxFrames && batch_ms[m] > 0.f) return batch_ms[m] * (4.f + (float)n) / (4.f + (float)m);
        return 0.f;
    }

    // A submit at host time t: how fast the frames arrive (moving average of the gap between submits; a pause counts as 10 ms).
    void submitted(double t) {
        if (last_submit_at > 0.0) {
            float gap = (float)std::min(10.0, (t - last_submit_at) * 1e3);
            // one long gap is a pause, not a change of pace: a tight loop that stops to synchronise (the fence between a warm-up and a timed
            // region, a caller that drains the pipeline now and then) must not look like a camera for its next few frames — they would go
            // out one frame per launch, 0.3 ms of GPU time each.  A stream that has really slowed down is told apart within four frames (the average grows by a quarter per frame).
            if (submit_gap_ms > 0.f) gap = std::min(gap, 2.f * submit_gap_ms);
            submit_gap_ms = submit_gap_ms > 0.f ? 0.75f * submit_gap_ms + 0.25f * gap : gap;
        }
        last_submit_at = t;
    }

    // A full batch goes out at once; a partial one when the GPU is about to run out of work (partial_batch_due); lm_detector_flush /
    // lm_detector_collect launch what is left.  So the batches are as large as the GPU's backlog allows and no larger.
    bool batch_full(int waiting) const { return waiting >= std::max(1, std::min(batch_max, kMaxFrames)); }

    // The launch a submit made took the calling thread `seconds` (at most 1 ms counts).
    void launch_cost(double seconds) { launch_cost_ms = 0.75f * launch_cost_ms + 0.25f * (float)std::min(1.0, seconds * 1e3); }

    // Should the `waiting` frames that wait for their batch go out now?  `at` = host time the question is asked for; drained = every
    // launched frame has been collected.
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
    template <class Gpu>
    bool partial_batch_due(int waiting, bool drained, double at, Gpu&& gpu) {
        if (waiting <= 0 || keep_queued <= 0) return false;
        const bool tight = submit_gap_ms > 0.f && submit_gap_ms < 2.5f * launch_cost_ms;   // (submit_gap_ms 0: no second submit yet — sparse until shown otherwise)
        if (drained) early_batch_used = false;                     // nothing in flight: a new burst
        if (tight) {
            // ONE early batch per burst: the GPU is idle (nothing launched is unfinished), LM_FIRST_BATCH frames wait.  Not again until the pipeline has
            // drained: with a host that needs longer for three submits + a launch than the GPU for three frames, every early batch would find the GPU idle
            // again and the stream would settle on three frames per launch (one run in three of a 20-step series did: 0.154 instead of 0.100 ms per frame).
            if (early_batch_used || waiting < first_batch) return false;
            if (!drained && batches_queued(gpu) != 0) return false;
            early_batch_used = true;
            return true;
        }
        // sparse: nothing launched is unfinished (collected or not) -> the GPU is idle, the frames go out; else the GPU-time model
        if (drained || batches_queued(gpu) == 0) return true;
        if (batch_ms_estimate(waiting) <= 0.f) return batches_queued(gpu) < keep_queued;
        return gpu_free_at - at <= 1e-3 * launch_slack_ms;
    }

    // A batch of `frames` frames, the first of them frame number first_frame, was launched at host time t from leader slot `slot`: it joins the queue.
    template <class Gpu>
    void batch_launched(uint64_t first_frame, int slot, int frames, double t, Gpu&& gpu) {
        const bool idle = batches_queued(gpu) == 0;
        if (idle) gpu_free_at = std::min(gpu_free_at, t);
        gpu_free_at = std::max(gpu_free_at, t) + 1e-3 * batch_ms_estimate(frames);
        queued.push_back({first_frame, slot, frames, t, idle});
    }

    // Keeping the model current around a collect's wait.  If the wait blocks on the first frame of a batch, the batch finished when
    // the wait returned: that pins the estimate of when the GPU runs dry and — with the start of the batch known too (the previous batch's
    // end seen the same way, or an idle GPU at launch) — gives the batch's duration.  Frames waiting for their batch go out BEFORE
    // the wait if the GPU would have (almost) nothing left when it ends, or after it if it has by then.
    struct CollectWait {
        bool batch_head, blocked;                           // the frame is the first of the oldest queued batch; the wait will block on it (the caller's query says)
        QueuedBatch head;
    };
    // `collected` = frames collected so far = the number of the frame being collected, `leader` = the leader slot of its batch
    CollectWait before_wait(uint64_t collected, int leader) const {
        CollectWait w{};
        w.batch_head = !queued.empty() && queued.front().first_frame == collected && queued.front().slot == leader;
        if (w.batch_head) w.head = queued.front();
        return w;
    }
    double later_batches_ms(uint64_t collected) const {     // estimated GPU time of the batches launched after the frame being collected
        double ms = 0.0;
        for (const QueuedBatch& q : queued)
            if (q.first_frame > collected) { const float e = batch_ms_estimate(q.frames); ms += e > 0.f ? e : 1e3; }   // not timed yet: plenty
        return ms;
    }
    // the wait will block: do the waiting frames go out first?
    bool due_before_wait(int waiting, uint64_t collected) const {
        return waiting > 0 && keep_queued > 0 && later_batches_ms(collected) <= launch_slack_ms;   // (no batch launched after this one: 0, with or without a GPU-time model)
    }
    // The wait returned at host time `now`.  Returns whether the waiting frames go out now: this was the last launched frame (the GPU has
    // nothing left), or the rule of a submit says so.
    template <class Gpu>
    bool after_wait(const CollectWait& w, double now, int waiting, uint64_t collected, uint64_t launched, Gpu&& gpu) {
        const QueuedBatch& head = w.head;
        const double dry_at = now + 1e-3 * later_batches_ms(collected);
        if (w.batch_head && w.blocked) {
            const bool start_known = head.gpu_idle_at_launch || (last_done_at >= 0.0 && last_done_end == head.first_frame);
            if (start_known) {
                const double start = head.gpu_idle_at_launch ? head.launched_at : std::max(last_done_at, head.launched_at);
                const float ms = (float)((now - start) * 1e3);
                float& e = batch_ms[head.frames];
                if (ms > 0.f && ms < 1e3f) e = e > 0.f ? 0.75f * e + 0.25f * ms : ms;
            }
            gpu_free_at = dry_at;
            last_done_at = now;
            last_done_end = head.first_frame + (uint64_t)head.frames;
        } else {
            gpu_free_at = std::min(gpu_free_at, dry_at);
            if (w.batch_head) { last_done_at = -1.0; last_done_end = head.first_frame + (uint64_t)head.frames; }
        }
        const bool idle_after = launched == collected + 1;         // this was the last launched frame: the GPU has nothing left
        return waiting > 0 && keep_queued > 0 && (idle_after || (batch_ms_estimate(waiting) > 0.f && partial_batch_due(waiting, launched == collected, now, gpu)));
    }
    // Frame `collected` has been waited for: its batch and everything before it are done.
    void frame_done(uint64_t collected) {
        while (!queued.empty() && queued.front().first_frame <= collected) queued.erase(queued.begin());
    }
};

}  // namespace lm
