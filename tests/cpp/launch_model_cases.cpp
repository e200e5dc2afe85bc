// Stand-alone cases of the launch-timing model of the streamed path (6dpose_amd/csrc/launch_model.h): every rule that decides when a
// partial batch goes out, on a CPU.  Includes the model alone — no HIP, no detector —; the GPU is a table of which batches have finished
// that counts how often it is asked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I6dpose_amd/csrc
//       tests/cpp/launch_model_cases.cpp -o launch_model_cases && ./launch_model_cases
// Exit 0 and a last line "ok": every case holds.  The expected values are those of the arithmetic as it stood inside the detector.
#include <math.h>
#include <stdio.h>

#include "launch_model.h"

using lm::LaunchModel;

struct FakeGpu {
    bool done[16] = {};                 // per leader slot
    int queries = 0, ends = 0;
    bool finished(int slot) { ++queries; return done[slot]; }
    void queries_end() { ++ends; }
};

static int failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failed; } } while (0)
static bool near(double a, double b) { return fabs(a - b) <= 1e-6 * std::max(1.0, fabs(b)); }

static void estimate_cases() {
    LaunchModel m;
    for (int n = 1; n <= LaunchModel::kMaxFrames; ++n) CHECK(m.batch_ms_estimate(n) == 0.f);      // nothing measured
    m.batch_ms[8] = 1.0f;
    CHECK(m.batch_ms_estimate(8) == 1.0f);
    CHECK(m.batch_ms_estimate(4) == 1.0f * 8.f / 12.f);                                           // (4 + n) / (4 + m)
    LaunchModel k;
    k.batch_ms[2] = 1.0f; k.batch_ms[6] = 3.0f;
    CHECK(k.batch_ms_estimate(4) == 1.0f * 8.f / 6.f);                                            // equal distance: the smaller size first
    CHECK(k.batch_ms_estimate(5) == 3.0f * 9.f / 10.f);
}

static void submit_gap_cases() {
    LaunchModel m;
    m.submitted(1.0);
    CHECK(m.submit_gap_ms == 0.f && m.last_submit_at == 1.0);                                     // first submit: no gap yet
    m.submitted(1.0002);
    CHECK(near(m.submit_gap_ms, 0.2));
    const float a = m.submit_gap_ms;
    m.submitted(1.0502);                                                                          // 50 ms: counts as 10, then as 2 x the average
    CHECK(m.submit_gap_ms == 0.75f * a + 0.25f * (2.f * a));
    CHECK(near(m.submit_gap_ms, 0.25));
    LaunchModel p;                                                                                // a pause as the first gap: 10 ms
    p.submitted(1.0); p.submitted(3.0);
    CHECK(p.submit_gap_ms == 10.f);
}

static void launch_cost_cases() {
    LaunchModel m;
    CHECK(m.launch_cost_ms == 0.1f);
    m.launch_cost(0.005);                                                                         // 5 ms: counts as 1
    CHECK(m.launch_cost_ms == 0.75f * 0.1f + 0.25f * 1.0f);
    LaunchModel k;
    k.launch_cost(0.0002);
    CHECK(k.launch_cost_ms == 0.75f * 0.1f + 0.25f * (float)(0.0002 * 1e3));
    CHECK(m.batch_full(8) && !m.batch_full(7));
    m.batch_max = 3; CHECK(m.batch_full(3) && !m.batch_full(2));
    m.batch_max = 0; CHECK(m.batch_full(1) && !m.batch_full(0));
    m.batch_max = 99; CHECK(m.batch_full(8) && !m.batch_full(7));
}

static void never_due_cases() {
    for (int which = 0; which < 2; ++which) {
        LaunchModel m;
        FakeGpu g;
        m.queued.push_back({0, 0, 4, 1.0, true});
        m.early_batch_used = true;
        if (which) m.keep_queued = 0;
        const int waiting = which ? 3 : 0;
        for (int drained = 0; drained < 2; ++drained)
            for (float gap : {0.f, 0.1f}) {                                                       // sparse and tight
                m.submit_gap_ms = gap;
                CHECK(!m.partial_batch_due(waiting, drained != 0, 2.0, g));
            }
        CHECK(g.queries == 0 && g.ends == 0);
        CHECK(m.early_batch_used);                                                                // the latch is not reset
        CHECK(m.queued.size() == 1);
    }
}

static void sparse_cases() {
    for (float gap : {0.f, 0.25f, 0.3f}) {                                                        // no second submit yet; exactly and above 2.5 x the launch cost
        LaunchModel m;
        FakeGpu g;
        m.submit_gap_ms = gap;
        m.queued.push_back({0, 0, 4, 1.0, true});
        CHECK(m.partial_batch_due(1, true, 2.0, g));                                              // drained
        CHECK(g.queries == 0);
    }
    {   // not drained, every queued batch has finished
        LaunchModel m;
        FakeGpu g;
        m.queued.push_back({0, 0, 4, 1.0, true});
        m.queued.push_back({4, 4, 4, 1.1, false});
        g.done[0] = g.done[4] = true;
        CHECK(m.partial_batch_due(1, false, 2.0, g));
        CHECK(m.queued.empty() && g.queries == 2 && g.ends == 1);
    }
    for (int keep = 1; keep <= 3; ++keep)
        for (int unfinished = 1; unfinished <= 2; ++unfinished) {                                 // no estimate: the backlog in batches
            LaunchModel m;
            FakeGpu g;
            m.keep_queued = keep;
            m.queued.push_back({0, 0, 4, 1.0, true});                                             // finished
            g.done[0] = true;
            for (int u = 0; u < unfinished; ++u) m.queued.push_back({(uint64_t)(4 + 4 * u), 4 + 4 * u, 4, 1.1, false});
            CHECK(m.partial_batch_due(1, false, 2.0, g) == (unfinished < keep));
            CHECK((int)m.queued.size() == unfinished);
        }
    {   // with an estimate: the backlog in time against the slack
        LaunchModel m;
        FakeGpu g;
        m.batch_ms[1] = 1.0f;
        m.queued.push_back({0, 0, 4, 1.0, true});
        const double slack = 1e-3 * m.launch_slack_ms;
        m.gpu_free_at = 10.0;
        CHECK(m.partial_batch_due(1, false, 10.0 - 0.5 * slack, g));
        CHECK(!m.partial_batch_due(1, false, 10.0 - 1.5 * slack, g));
        m.gpu_free_at = slack;                                                                    // the boundary itself, asked at time 0
        CHECK(m.partial_batch_due(1, false, 0.0, g));
        m.gpu_free_at = nextafter(slack, 1.0);
        CHECK(!m.partial_batch_due(1, false, 0.0, g));
        m.batch_ms[1] = 0.f; m.batch_ms[3] = 1.0f;                                                // a scaled estimate serves as well
        CHECK(!m.partial_batch_due(1, false, 0.0, g));
        CHECK(m.queued.size() == 1);
    }
}

static void tight_cases() {
    LaunchModel m;
    FakeGpu g;
    m.submit_gap_ms = 0.1f;                                                                       // < 2.5 x 0.1
    CHECK(m.first_batch == 3);
    CHECK(!m.partial_batch_due(2, false, 2.0, g));                                                // fewer than first_batch
    CHECK(g.queries == 0 && g.ends == 0);
    CHECK(m.partial_batch_due(3, false, 2.0, g));                                                 // the GPU is idle: nothing queued
    CHECK(g.queries == 0 && g.ends == 1 && m.early_batch_used);
    CHECK(!m.partial_batch_due(3, false, 2.0, g));                                                // once per burst
    CHECK(!m.partial_batch_due(8, false, 2.0, g));
    CHECK(g.ends == 1);
    CHECK(!m.partial_batch_due(2, true, 2.0, g));                                                 // an ask that saw the pipeline drained: a new burst
    CHECK(!m.early_batch_used);
    m.queued.push_back({0, 0, 4, 1.0, true});                                                     // unfinished
    CHECK(!m.partial_batch_due(3, false, 2.0, g));                                                // the GPU is busy: no early batch, the latch stays open
    CHECK(!m.early_batch_used && g.queries == 1 && g.ends == 2);
    g.done[0] = true;
    CHECK(m.partial_batch_due(3, false, 2.0, g));                                                 // it has finished
    CHECK(m.early_batch_used && m.queued.empty() && g.queries == 2 && g.ends == 3);
    m.queued.push_back({4, 4, 4, 1.0, true});
    const int q = g.queries, e = g.ends;
    CHECK(m.partial_batch_due(3, true, 2.0, g));                                                  // drained: due, and the GPU is not asked
    CHECK(g.queries == q && g.ends == e && m.queued.size() == 1 && m.early_batch_used);
}

static void launch_cases() {
    {   // idle at launch: the estimate comes down to t first
        LaunchModel m;
        FakeGpu g;
        m.batch_ms[4] = 2.0f;
        m.gpu_free_at = 100.0;
        m.batch_launched(12, 5, 4, 5.0, g);
        CHECK(m.gpu_free_at == 5.0 + 1e-3 * 2.0f);
        CHECK(m.queued.size() == 1);
        const LaunchModel::QueuedBatch& q = m.queued.back();
        CHECK(q.first_frame == 12 && q.slot == 5 && q.frames == 4 && q.launched_at == 5.0 && q.gpu_idle_at_launch);
        CHECK(g.queries == 0 && g.ends == 1);
    }
    for (double free_at : {7.0, 3.0}) {                                                           // not idle: behind what is queued, never before t
        LaunchModel m;
        FakeGpu g;
        m.batch_ms[8] = 1.0f;
        m.gpu_free_at = free_at;
        m.queued.push_back({0, 0, 8, 4.9, true});
        m.batch_launched(8, 8, 4, 5.0, g);
        CHECK(m.gpu_free_at == std::max(free_at, 5.0) + 1e-3 * (1.0f * 8.f / 12.f));
        CHECK(m.queued.size() == 2 && !m.queued.back().gpu_idle_at_launch && g.queries == 1);
    }
    {   // everything queued has finished: idle
        LaunchModel m;
        FakeGpu g;
        m.gpu_free_at = 7.0;
        m.queued.push_back({0, 0, 8, 4.9, true});
        g.done[0] = true;
        m.batch_launched(8, 8, 4, 5.0, g);
        CHECK(m.gpu_free_at == 5.0 && m.queued.size() == 1 && m.queued.back().gpu_idle_at_launch);
    }
}

static void wait_cases() {
    LaunchModel m;
    FakeGpu g;
    m.keep_queued = 0;                                                                            // the bookkeeping alone: nothing is ever due
    m.queued.push_back({0, 0, 4, 1.0, true});
    m.queued.push_back({4, 4, 4, 1.001, false});
    CHECK(!m.before_wait(0, 1).batch_head && !m.before_wait(1, 0).batch_head);
    LaunchModel::CollectWait w = m.before_wait(0, 0);
    CHECK(w.batch_head && !w.blocked && w.head.frames == 4 && w.head.launched_at == 1.0);
    w.blocked = true;
    CHECK(!m.after_wait(w, 1.002, 0, 0, 8, g));                                                   // start known: idle at launch
    const float first = (float)((1.002 - 1.0) * 1e3);
    CHECK(m.batch_ms[4] == first && near(first, 2.0));
    CHECK(m.last_done_at == 1.002 && m.last_done_end == 4);
    CHECK(m.gpu_free_at == 1.002 + 1e-3 * 1e3);                                                   // the later batch, untimed when the wait returned: plenty
    m.frame_done(0);
    CHECK(m.queued.size() == 1 && m.queued.front().first_frame == 4);
    for (uint64_t f = 1; f < 4; ++f) {                                                            // the batch's other frames: no batch head
        w = m.before_wait(f, 0);
        CHECK(!w.batch_head);
        const double free_at = m.gpu_free_at;
        CHECK(!m.after_wait(w, 1.0021, 0, f, 8, g));
        CHECK(m.gpu_free_at <= free_at && m.last_done_at == 1.002 && m.last_done_end == 4);
        m.frame_done(f);
    }
    w = m.before_wait(4, 4);
    CHECK(w.batch_head);
    w.blocked = true;
    CHECK(!m.after_wait(w, 1.006, 0, 4, 8, g));                                                   // start known: the previous batch was seen to finish
    const float second = (float)((1.006 - std::max(1.002, 1.001)) * 1e3);
    CHECK(m.batch_ms[4] == 0.75f * first + 0.25f * second && near(m.batch_ms[4], 2.5));
    CHECK(m.last_done_at == 1.006 && m.last_done_end == 8 && m.gpu_free_at == 1.006);
    m.frame_done(4);
    CHECK(m.queued.empty());

    const float kept = m.batch_ms[4];
    for (double now : {2.0, 1.5, 3.5}) {                                                          // durations 0, < 0 and >= 1000 ms: not a measurement
        m.queued.assign(1, {8, 8, 4, 2.0, true});
        w = m.before_wait(8, 8); w.blocked = true;
        m.after_wait(w, now, 0, 8, 12, g);
        CHECK(m.batch_ms[4] == kept && m.last_done_at == now && m.last_done_end == 12);
    }
    m.queued.assign(1, {20, 4, 4, 2.0, false});                                                   // start unknown: busy at launch, the previous end not seen
    w = m.before_wait(20, 4); w.blocked = true;
    m.after_wait(w, 2.001, 0, 20, 24, g);
    CHECK(m.batch_ms[4] == kept && m.last_done_end == 24);

    // a wait that did not block
    m.queued.assign(1, {24, 8, 4, 3.0, true});
    m.gpu_free_at = 0.5;
    w = m.before_wait(24, 8);
    m.after_wait(w, 3.0, 0, 24, 28, g);
    CHECK(m.gpu_free_at == 0.5 && m.last_done_at == -1.0 && m.last_done_end == 28 && m.batch_ms[4] == kept);
    m.gpu_free_at = 9.0; m.last_done_at = 2.5;
    m.after_wait(w, 3.0, 0, 24, 28, g);
    CHECK(m.gpu_free_at == 3.0 && m.last_done_at == -1.0);
    CHECK(g.queries == 0 && g.ends == 0);
}

static void later_batches_cases() {
    LaunchModel m;
    FakeGpu g;
    m.queued.push_back({0, 0, 4, 1.0, true});
    CHECK(m.later_batches_ms(0) == 0.0);
    CHECK(m.due_before_wait(1, 0) && !m.due_before_wait(0, 0));                                   // no batch launched after this one
    m.queued.push_back({4, 4, 2, 1.0, false});
    CHECK(m.later_batches_ms(0) == 1e3);                                                          // not timed yet: plenty
    CHECK(!m.due_before_wait(1, 0));
    m.batch_ms[2] = 0.125f;
    CHECK(m.later_batches_ms(0) == 0.125 && m.later_batches_ms(4) == 0.0);
    CHECK(m.due_before_wait(1, 0));                                                               // 0.125 <= 0.15
    m.batch_ms[2] = 0.25f;
    CHECK(!m.due_before_wait(1, 0));
    m.keep_queued = 0;
    CHECK(!m.due_before_wait(1, 4));

    // after the wait: the last launched frame, or the rule of a submit (which needs an estimate here)
    LaunchModel k;
    LaunchModel::CollectWait w{};
    CHECK(k.after_wait(w, 1.0, 1, 3, 4, g));                                                      // idle after
    CHECK(!k.after_wait(w, 1.0, 0, 3, 4, g));
    CHECK(!k.after_wait(w, 1.0, 1, 2, 4, g));                                                     // no estimate: collect does not ask
    k.batch_ms[1] = 1.0f;
    CHECK(k.after_wait(w, 1.0, 1, 2, 4, g));                                                      // sparse, nothing queued is unfinished
    k.keep_queued = 0;
    CHECK(!k.after_wait(w, 1.0, 1, 3, 4, g));
}

int main() {
    estimate_cases();
    submit_gap_cases();
    launch_cost_cases();
    never_due_cases();
    sparse_cases();
    tight_cases();
    launch_cases();
    wait_cases();
    later_batches_cases();
    if (failed) { printf("FAILED: %d\n", failed); return 1; }
    printf("ok\n");
    return 0;
}
