// DevBuf<T> (csrc/dev_buf.h) alone, on buffers of a few hundred bytes: what ensure() keeps and what it replaces, release() twice,
// the moves, and a std::vector of buffers that reallocates (lm_detector::slot_rgb).  Prints "ok: <checks>" and returns 0, or the
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

static int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

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

int main() {
    CHECK(hipSetDevice(0) == hipSuccess);
    {   // ensure
        DevBuf<uint32_t> b;
        CHECK(b.ensure(0) == LM_OK && b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(100) == LM_OK && b.p != nullptr && b.cap == 100);
        uint32_t* const p100 = b.p;
        CHECK(b.ensure(100) == LM_OK && b.p == p100 && b.cap == 100);
        CHECK(b.ensure(37) == LM_OK && b.p == p100 && b.cap == 100);
        CHECK(b.ensure(0) == LM_OK && b.p == p100 && b.cap == 100);
        CHECK(b.ensure(101) == LM_OK && b.p != nullptr && b.cap == 101);   // exactly n, counted in elements
        CHECK(hipMemset(b.p, 0, 101 * sizeof(uint32_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(5) == LM_OK && b.p != nullptr && b.cap == 5);       // usable again after release
    }
    {   // moves
        DevBuf<uint8_t> a;
        CHECK(a.ensure(200) == LM_OK && put(a.p, 11, 200));
        uint8_t* const pa = a.p;
        DevBuf<uint8_t> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 200 && holds(b.p, 11, 200));
        DevBuf<uint8_t> c;
        CHECK(c.ensure(64) == LM_OK);                                      // the target's own allocation is released, not leaked or kept
        c = std::move(b);
        CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 200 && holds(c.p, 11, 200));
        DevBuf<uint8_t>& self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.cap == 200 && holds(c.p, 11, 200));
        CHECK(a.ensure(300) == LM_OK && a.cap == 300);                     // a moved-from buffer is an empty one
    }
    {   // a vector that reallocates
        std::vector<DevBuf<uint8_t>> v;
        v.resize(3);
        std::vector<uint8_t*> ptr;
        for (size_t i = 0; i < v.size(); ++i) {
            CHECK(v[i].ensure(100 + i) == LM_OK && put(v[i].p, (uint8_t)(40 + i), 100 + i));
            ptr.push_back(v[i].p);
        }
        const DevBuf<uint8_t>* const before = v.data();
        v.resize(v.capacity() + 5);
        CHECK(v.data() != before);
        for (size_t i = 0; i < v.size(); ++i) {
            if (i < 3) CHECK(v[i].p == ptr[i] && v[i].cap == 100 + i && holds(v[i].p, (uint8_t)(40 + i), 100 + i));
            else CHECK(v[i].p == nullptr && v[i].cap == 0);
        }
        v.resize(1);                                                       // frees two, keeps the first
        CHECK(v[0].p == ptr[0] && holds(v[0].p, 40, 100));
    }
    CHECK(hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess);
    printf("ok: %d\n", checks);
    return 0;
}
