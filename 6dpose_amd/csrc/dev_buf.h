// DevBuf<T>: one device allocation and its capacity, owned.  Grow-only; move-only (a copy would free the pointer twice).
// The owner selects the device and synchronises whatever still uses the memory before a DevBuf dies; none has static
// storage duration (a hipFree during process teardown is unsafe).
#pragma once
#include <stddef.h>

#include "lm_error.h"

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    // At least n elements; growing frees first and does NOT keep the contents.  A failed allocation leaves the buffer empty.
    int ensure(size_t n) {
        if (n <= cap) return LM_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        HIP_TRY(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return LM_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
