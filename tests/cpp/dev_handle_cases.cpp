// DevStream and DevEvent (csrc/dev_buf.h) alone: what ensure() creates and what it keeps, release() twice, the moves, a std::vector of
// events that reallocates, and that the handles are real ones: a stream of each creation form takes a 256-byte memset, events of each of
// the three flag kinds in use are recorded, waited on from a second stream and synchronised.  Nothing is called on a released handle.
// Prints "ok: <checks>" and returns 0, or the first failed check and 1.  Driven by tests/test_gpu_dev_buf.py.
#include <stdarg.h>
#include <stdio.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "dev_buf.h"

int lm_set_error(int code, const char* fmt, ...) {          // the library's lives in detector.cpp
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

template <typename T>
constexpr bool move_only() {
    return !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value && std::is_nothrow_move_constructible<T>::value &&
           std::is_nothrow_move_assignable<T>::value;
}
static_assert(move_only<DevStream>(), "DevStream: no copy (the stream would be destroyed twice), nothrow moves");
static_assert(move_only<DevEvent>(), "DevEvent: no copy, nothrow moves (std::vector must move events when it grows)");
static_assert(!std::is_convertible<DevStream, DevEvent>::value && !std::is_convertible<DevEvent, DevStream>::value, "a stream is no event");

static int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// ensure / release / moves, the same for both types; make(h) is the type's ensure with the arguments of the case
template <typename Handle, typename Make>
static int ownership(Make make) {
    using Raw = decltype(Handle().h);
    {   // ensure, release
        Handle a;
        CHECK(a.h == nullptr && !a);
        CHECK(make(a) == LM_OK && a.h != nullptr && a);
        const Raw first = a;
        CHECK(make(a) == LM_OK && a.h == first);                             // kept, not replaced
        a.release();
        CHECK(a.h == nullptr);
        a.release();
        CHECK(a.h == nullptr);
        CHECK(make(a) == LM_OK && a.h != nullptr);                           // usable again after release
    }
    {   // moves
        Handle a;
        CHECK(make(a) == LM_OK);
        const Raw ra = a;
        Handle b(std::move(a));
        CHECK(a.h == nullptr && b.h == ra);
        Handle c;
        CHECK(make(c) == LM_OK && c.h != ra);                                // the target's own handle is released, not leaked or kept
        c = std::move(b);
        CHECK(b.h == nullptr && c.h == ra);
        Handle& self = c;
        c = std::move(self);
        CHECK(c.h == ra);
        CHECK(make(a) == LM_OK && a.h != nullptr && a.h != ra);              // a moved-from handle is an empty one
    }
    return 0;
}

static int memset_on(hipStream_t s, void* p) {
    CHECK(hipMemsetAsync(p, 0x5a, 256, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
    return 0;
}

int main() {
    CHECK(hipSetDevice(0) == hipSuccess);
    if (ownership<DevStream>([](DevStream& s) { return s.ensure(hipStreamNonBlocking); })) return 1;
    if (ownership<DevStream>([](DevStream& s) { return s.ensure(hipStreamNonBlocking, 0); })) return 1;
    if (ownership<DevEvent>([](DevEvent& e) { return e.ensure(); })) return 1;
    if (ownership<DevEvent>([](DevEvent& e) { return e.ensure(hipEventDisableTiming); })) return 1;

    DevBuf<unsigned char> buf;
    CHECK(buf.ensure(256) == LM_OK);
    DevStream plain, high, low, other;
    int least = 0, greatest = 0;
    CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess);
    CHECK(plain.ensure(hipStreamNonBlocking) == LM_OK && high.ensure(hipStreamNonBlocking, greatest) == LM_OK &&
          low.ensure(hipStreamNonBlocking, least) == LM_OK && other.ensure(hipStreamNonBlocking) == LM_OK);
    CHECK(plain.h != high.h && high.h != low.h && low.h != other.h);
    if (memset_on(plain, buf.p) || memset_on(high, buf.p) || memset_on(low, buf.p)) return 1;
    int prio = 12345;
    CHECK(hipStreamGetPriority(high, &prio) == hipSuccess && prio == greatest);
    CHECK(hipStreamGetPriority(low, &prio) == hipSuccess && prio == least);
    {   // two default events around a memset time it
        DevEvent t0, t1;
        CHECK(t0.ensure() == LM_OK && t1.ensure() == LM_OK);
        CHECK(hipEventRecord(t0, plain) == hipSuccess && hipMemsetAsync(buf.p, 1, 256, plain) == hipSuccess && hipEventRecord(t1, plain) == hipSuccess);
        CHECK(hipEventSynchronize(t1) == hipSuccess);
        float ms = -1.f;
        CHECK(hipEventElapsedTime(&ms, t0, t1) == hipSuccess && ms >= 0.f);
    }
    for (unsigned flags : {(unsigned)hipEventDefault, (unsigned)hipEventDisableTiming, (unsigned)hipEventDisableSystemFence}) {
        DevEvent e;                                                          // recorded on one stream, waited on from another, synchronised
        CHECK(e.ensure(flags) == LM_OK);
        CHECK(hipMemsetAsync(buf.p, 2, 256, plain) == hipSuccess && hipEventRecord(e, plain) == hipSuccess);
        CHECK(hipStreamWaitEvent(other, e, 0) == hipSuccess && hipMemsetAsync(buf.p, 3, 256, other) == hipSuccess);
        CHECK(hipEventSynchronize(e) == hipSuccess && hipStreamSynchronize(other) == hipSuccess);
        unsigned char back[256] = {0};
        CHECK(hipMemcpy(back, buf.p, 256, hipMemcpyDeviceToHost) == hipSuccess && back[0] == 3 && back[255] == 3);
    }
    {   // a vector that reallocates keeps every handle, and they still work
        std::vector<DevEvent> v;
        v.resize(3);
        std::vector<hipEvent_t> raw;
        for (auto& e : v) { CHECK(e.ensure(hipEventDisableTiming) == LM_OK); raw.push_back(e); }
        const DevEvent* const before = v.data();
        v.resize(v.capacity() + 5);
        CHECK(v.data() != before);
        for (size_t i = 0; i < v.size(); ++i) CHECK(v[i].h == (i < 3 ? raw[i] : nullptr));
        for (size_t i = 0; i < 3; ++i) CHECK(hipEventRecord(v[i], plain) == hipSuccess && hipEventSynchronize(v[i]) == hipSuccess);
        v.resize(1);                                                         // destroys two, keeps the first
        CHECK(v[0].h == raw[0] && hipEventQuery(v[0]) == hipSuccess);
    }
    CHECK(hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess);
    printf("ok: %d\n", checks);
    return 0;
}
