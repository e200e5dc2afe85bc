// DevBuf<T>: one device allocation and its capacity, owned.  Grow-only; move-only (a copy would free the pointer twice).
// PinBuf<T>: its twin for pinned host memory (hipHostMalloc with hipHostMallocDefault / hipHostFree).
// The owner selects the device and synchronises whatever still uses the memory before a buffer dies; none has static
// storage duration (a hipFree during process teardown is unsafe).
#pragma once
#include <stddef.h>

#include "lm_error.h"

struct DevMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
};
struct PinMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
};

template <typename T, typename Mem>
struct OwnedBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~OwnedBuf() { release(); }
    // At least n elements; growing frees first and does NOT keep the contents.  A failed allocation leaves the buffer empty.
    int ensure(size_t n) {
        if (n <= cap) return LM_OK;
        release();
        HIP_TRY(Mem::alloc((void**)&p, n * sizeof(T)));
        cap = n;
        return LM_OK;
    }
    void release() { if (p) (void)Mem::free(p); p = nullptr; cap = 0; }
};

template <typename T> using DevBuf = OwnedBuf<T, DevMem>;
template <typename T> using PinBuf = OwnedBuf<T, PinMem>;
