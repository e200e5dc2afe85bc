// DevBuf<T> and PinBuf<T> (csrc/dev_buf.h) alone, on buffers of a few hundred bytes: what ensure() keeps and what it replaces, release()
// twice, the moves, and a std::vector of buffers that reallocates (lm_detector::slot_rgb).  The same cases run for both: device memory
// is written and read with hipMemcpy, pinned memory directly through the host pointer.  Prints "ok: <checks>" and returns 0, or the
// first failed check and 1.  Driven by tests/test_gpu_dev_buf.py.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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

static_assert(!std::is_copy_constructible<DevBuf<uint8_t>>::value && !std::is_copy_assignable<DevBuf<uint8_t>>::value, "DevBuf must not copy");
static_assert(std::is_nothrow_move_constructible<DevBuf<uint8_t>>::value && std::is_nothrow_move_assignable<DevBuf<uint8_t>>::value,
              "std::vector must move DevBufs when it grows");
static_assert(!std::is_copy_constructible<PinBuf<uint8_t>>::value && !std::is_copy_assignable<PinBuf<uint8_t>>::value, "PinBuf must not copy");
static_assert(std::is_nothrow_move_constructible<PinBuf<uint8_t>>::value && std::is_nothrow_move_assignable<PinBuf<uint8_t>>::value,
              "std::vector must move PinBufs when it grows");
static_assert(!std::is_same<DevBuf<uint8_t>, PinBuf<uint8_t>>::value, "a pinned buffer must not convert into a device buffer");

static int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

struct DeviceIo {                                            // device memory: through hipMemcpy
    static bool put(uint8_t* dst, uint8_t seed, size_t n) {
        std::vector<uint8_t> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = (uint8_t)(seed + 7 * i);
        return hipMemcpy(dst, h.data(), n, hipMemcpyHostToDevice) == hipSuccess;
    }
    static bool holds(const uint8_t* src, uint8_t seed, size_t n) {
        std::vector<uint8_t> h(n, 0);
        if (hipMemcpy(h.data(), src, n, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (size_t i = 0; i < n; ++i)
            if (h[i] != (uint8_t)(seed + 7 * i)) return false;
        return true;
    }
    static bool zero(void* p, size_t bytes) { return hipMemset(p, 0, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess; }
};
struct HostIo {                                              // pinned memory: the host pointer itself
    static bool put(uint8_t* dst, uint8_t seed, size_t n) {
        for (size_t i = 0; i < n; ++i) dst[i] = (uint8_t)(seed + 7 * i);
        return true;
    }
    static bool holds(const uint8_t* src, uint8_t seed, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (src[i] != (uint8_t)(seed + 7 * i)) return false;
        return true;
    }
    static bool zero(void* p, size_t bytes) { memset(p, 0, bytes); return true; }
};

template <template <typename> class Buf, typename Io>
static int cases() {
    {   // ensure
        Buf<uint32_t> b;
        CHECK(b.ensure(0) == LM_OK && b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(100) == LM_OK && b.p != nullptr && b.cap == 100);
        uint32_t* const p100 = b.p;
        CHECK(b.ensure(100) == LM_OK && b.p == p100 && b.cap == 100);
        CHECK(b.ensure(37) == LM_OK && b.p == p100 && b.cap == 100);
        CHECK(b.ensure(0) == LM_OK && b.p == p100 && b.cap == 100);
        CHECK(b.ensure(101) == LM_OK && b.p != nullptr && b.cap == 101);   // exactly n, counted in elements
        CHECK(Io::zero(b.p, 101 * sizeof(uint32_t)));
        b.release();
        CHECK(b.p == nullptr && b.cap == 0);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(5) == LM_OK && b.p != nullptr && b.cap == 5);       // usable again after release
    }
    {   // moves
        Buf<uint8_t> a;
        CHECK(a.ensure(200) == LM_OK && Io::put(a.p, 11, 200));
        uint8_t* const pa = a.p;
        Buf<uint8_t> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 200 && Io::holds(b.p, 11, 200));
        Buf<uint8_t> c;
        CHECK(c.ensure(64) == LM_OK);                                      // the target's own allocation is released, not leaked or kept
        c = std::move(b);
        CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 200 && Io::holds(c.p, 11, 200));
        Buf<uint8_t>& self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.cap == 200 && Io::holds(c.p, 11, 200));
        CHECK(a.ensure(300) == LM_OK && a.cap == 300);                     // a moved-from buffer is an empty one
    }
    {   // a vector that reallocates
        std::vector<Buf<uint8_t>> v;
        v.resize(3);
        std::vector<uint8_t*> ptr;
        for (size_t i = 0; i < v.size(); ++i) {
            CHECK(v[i].ensure(100 + i) == LM_OK && Io::put(v[i].p, (uint8_t)(40 + i), 100 + i));
            ptr.push_back(v[i].p);
        }
        const Buf<uint8_t>* const before = v.data();
        v.resize(v.capacity() + 5);
        CHECK(v.data() != before);
        for (size_t i = 0; i < v.size(); ++i) {
            if (i < 3) CHECK(v[i].p == ptr[i] && v[i].cap == 100 + i && Io::holds(v[i].p, (uint8_t)(40 + i), 100 + i));
            else CHECK(v[i].p == nullptr && v[i].cap == 0);
        }
        v.resize(1);                                                       // frees two, keeps the first
        CHECK(v[0].p == ptr[0] && Io::holds(v[0].p, 40, 100));
    }
    return 0;
}

int main() {
    CHECK(hipSetDevice(0) == hipSuccess);
    if (cases<DevBuf, DeviceIo>() || cases<PinBuf, HostIo>()) return 1;
    {   // pinned memory is what the copy engine takes: a round trip through a device buffer, asynchronously
        PinBuf<uint8_t> src, dst;
        DevBuf<uint8_t> dev;
        CHECK(src.ensure(300) == LM_OK && dst.ensure(300) == LM_OK && dev.ensure(300) == LM_OK && HostIo::put(src.p, 90, 300) && HostIo::zero(dst.p, 300));
        CHECK(hipMemcpyAsync(dev.p, src.p, 300, hipMemcpyHostToDevice, nullptr) == hipSuccess &&
              hipMemcpyAsync(dst.p, dev.p, 300, hipMemcpyDeviceToHost, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess);
        CHECK(HostIo::holds(dst.p, 90, 300));
    }
    CHECK(hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess);
    printf("ok: %d\n", checks);
    return 0;
}
