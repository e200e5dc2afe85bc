// DevBuf<T>: one device allocation and its capacity, owned.  Grow-only; move-only (a copy would free the pointer twice).
// PinBuf<T>: its twin for pinned host memory (hipHostMalloc with hipHostMallocDefault / hipHostFree).
// DevStream / DevEvent: one hipStream_t / hipEvent_t, owned the same way: move-only, ensure() creates the handle once, release() and the
// destructor destroy it.  Both convert to the raw handle, which is what launches, records, waits and `if (c->s)` take; a raw hipStream_t or
// hipEvent_t anywhere else refers to a handle that somebody else owns.
// The owner selects the device and synchronises whatever still uses the memory or the handle before it dies; none has static
// storage duration (a hipFree or a destroy during process teardown is unsafe).
// Teardown order is declaration order, reversed: a context declares its streams first, then its events and buffers, so that every buffer
// is freed while all of the context's streams still exist and every event is destroyed before any stream.
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

struct StreamHandle {
    static hipError_t destroy(hipStream_t h) { return hipStreamDestroy(h); }
};
struct EventHandle {
    static hipError_t destroy(hipEvent_t h) { return hipEventDestroy(h); }
};

template <typename H, typename Kind>
struct OwnedHandle {
    H h = nullptr;
    OwnedHandle() = default;
    OwnedHandle(const OwnedHandle&) = delete;
    OwnedHandle& operator=(const OwnedHandle&) = delete;
    OwnedHandle(OwnedHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    OwnedHandle& operator=(OwnedHandle&& o) noexcept {
        if (this != &o) { release(); h = o.h; o.h = nullptr; }
        return *this;
    }
    ~OwnedHandle() { release(); }
    operator H() const { return h; }
    void release() { if (h) (void)Kind::destroy(h); h = nullptr; }
};

// ensure: creates the handle if none is held and keeps it otherwise (the flags and the priority of a kept handle are those of its creation).
// A failed creation leaves the handle null.
struct DevStream : OwnedHandle<hipStream_t, StreamHandle> {
    int ensure(unsigned flags) {
        if (h) return LM_OK;
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&s, flags));
        h = s;
        return LM_OK;
    }
    int ensure(unsigned flags, int priority) {
        if (h) return LM_OK;
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithPriority(&s, flags, priority));
        h = s;
        return LM_OK;
    }
};

struct DevEvent : OwnedHandle<hipEvent_t, EventHandle> {
    int ensure(unsigned flags = hipEventDefault) {
        if (h) return LM_OK;
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        h = e;
        return LM_OK;
    }
};
