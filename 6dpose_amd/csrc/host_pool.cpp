// Helper threads of the streamed path and the staging copy they share with the calling thread.  Nothing here calls into the HIP runtime
// (detector_internal.h, HostPool, says why).
#include <sched.h>
#include <string.h>

#include <system_error>

#include "detector_internal.h"

static void pool_main(lm_detector* d) {
    lm_detector::HostPool& P = d->pool;
    for (;;) {
        std::function<void()> job;
        int spins = 0;
        for (;;) {
            if (P.posted.load(std::memory_order_acquire) > 0) {
                std::lock_guard<std::mutex> lk(P.mu);
                if (!P.jobs.empty()) { job = std::move(P.jobs.front()); P.jobs.pop_front(); P.posted.fetch_sub(1, std::memory_order_acq_rel); break; }
            }
            if (++spins < 30000) { __builtin_ia32_pause(); continue; }          // ~0.3 ms of spinning, then sleep
            std::unique_lock<std::mutex> lk(P.mu);
            if (P.stop) return;
            P.asleep.fetch_add(1, std::memory_order_seq_cst);
            P.cv.wait(lk, [&] { return P.stop || !P.jobs.empty(); });
            P.asleep.fetch_sub(1, std::memory_order_seq_cst);
            if (P.stop && P.jobs.empty()) return;
            spins = 0;
        }
        job();
    }
}
// Starts the helpers on first use.  Never more than the CPUs this process may run on leave free (a cgroup / affinity mask of a few cores, eight
// ranks on one node), and a thread the system refuses (std::system_error: a container's thread limit) only shrinks the pool: the streamed path
// works without helpers (the caller copies and sorts on its own).
bool pool_ready(lm_detector* d) {
    lm_detector::HostPool& P = d->pool;
    if (P.threads <= 0) return false;
    if (!P.started) {
        int cpus = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = CPU_COUNT(&set);
        P.threads = std::max(0, std::min(P.threads, cpus - 1));        // one CPU stays with the calling thread
        P.stop = false;
        int started = 0;
        for (int i = 0; i < P.threads; ++i) {
            try { P.th.emplace_back(pool_main, d); ++started; }
            catch (const std::system_error&) { break; }
        }
        P.threads = started;
        P.started = started > 0;
    }
    return P.threads > 0;
}
// The calling thread takes a queued job itself (while it waits for the helpers: a helper that was descheduled must not hold the caller up)
bool pool_run_one(lm_detector* d) {
    lm_detector::HostPool& P = d->pool;
    if (P.posted.load(std::memory_order_acquire) <= 0) return false;
    std::function<void()> job;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        if (P.jobs.empty()) return false;
        job = std::move(P.jobs.front()); P.jobs.pop_front(); P.posted.fetch_sub(1, std::memory_order_acq_rel);
    }
    job();
    return true;
}
void pool_post(lm_detector* d, std::function<void()> job) {
    lm_detector::HostPool& P = d->pool;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        P.jobs.push_back(std::move(job));
        P.posted.fetch_add(1, std::memory_order_seq_cst);
    }
    if (P.asleep.load(std::memory_order_seq_cst) > 0) P.cv.notify_one();
}
void pool_stop(lm_detector* d) {
    lm_detector::HostPool& P = d->pool;
    if (!P.started) return;
    { std::lock_guard<std::mutex> lk(P.mu); P.stop = true; }
    P.cv.notify_all();
    for (auto& t : P.th) if (t.joinable()) t.join();
    P.th.clear();
    P.started = false;
}

// memcpy into a pinned staging buffer with non-temporal stores: the buffer is read next by the copy engine, not by a core, and a slice
// (a few hundred KB) is below the size from which glibc's memcpy streams on its own — ordinary stores first READ every destination line
// (read for ownership).  Falls back to memcpy for small or unaligned pieces and on hosts without AVX2.
#if !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
__attribute__((target("avx2"))) static void copy_stream_avx2(uint8_t* dst, const uint8_t* src, size_t n) {
    size_t i = 0;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i)), b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 32));
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 64)), e = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i), a); _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 64), c); _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 96), e);
    }
    _mm_sfence();
    if (i < n) memcpy(dst + i, src + i, n - i);
}
static void copy_staging(uint8_t* dst, const uint8_t* src, size_t n) {
    static const bool avx2 = __builtin_cpu_supports("avx2") && knobs().nt_copy;
    if (avx2 && n >= 16384 && (reinterpret_cast<uintptr_t>(dst) & 31) == 0) copy_stream_avx2(dst, src, n);
    else memcpy(dst, src, n);
}
#else
static void copy_staging(uint8_t* dst, const uint8_t* src, size_t n) { memcpy(dst, src, n); }
#endif

// dst <- a, dst_b <- b (the two images of a frame), cut into slices for the caller's thread and the helpers
void staged_copy(lm_detector* d, uint8_t* dst, const uint8_t* a, size_t na, uint8_t* dst_b, const uint8_t* b, size_t nb) {
    const bool same_a = a == dst, same_b = b == dst_b;              // zero-copy: the caller filled lm_detector_ingest_buffer's pointers
    if (same_a || same_b || na + nb < (1u << 19) || !pool_ready(d)) {   // small frames: one thread
        if (!same_a && na) memcpy(dst, a, na);                      // (na / nb = 0, a / b null: a detector without that modality)
        if (!same_b && nb) memcpy(dst_b, b, nb);
        return;
    }
    const int parts = d->pool.threads + 1;
    const size_t total = na + nb, per = ((total + (size_t)parts - 1) / (size_t)parts + 4095) & ~(size_t)4095;
    auto copy_range = [=](size_t lo, size_t hi) {                   // bytes [lo, hi) of the two images taken as one run
        if (lo < na) copy_staging(dst + lo, a + lo, std::min(hi, na) - lo);
        if (hi > na) { const size_t l2 = std::max(lo, na); copy_staging(dst_b + (l2 - na), b + (l2 - na), hi - l2); }
    };
    std::atomic<int> left{0};
    for (int p = 1; p < parts; ++p) {
        const size_t lo = std::min(total, per * (size_t)p), hi = std::min(total, per * (size_t)(p + 1));
        if (lo >= hi) break;
        left.fetch_add(1, std::memory_order_relaxed);
        std::atomic<int>* lp = &left;
        pool_post(d, [=]() { copy_range(lo, hi); lp->fetch_sub(1, std::memory_order_release); });
    }
    copy_range(0, std::min(total, per));
    // queued jobs nobody has taken yet are run here — the copy slices above, and whatever else is queued: a list-preparation job of another
    // slot (~35 us, no HIP calls) may so run inside this submit; results do not depend on who runs a job —; then a bounded spin for the
    // slices in progress, then the CPU is given up between looks
    for (int spin = 0; left.load(std::memory_order_acquire) != 0;) {
        if (pool_run_one(d)) continue;
        if (++spin < 4000) __builtin_ia32_pause(); else std::this_thread::yield();
    }
}
