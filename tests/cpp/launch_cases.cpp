// lm_launch (csrc/launch.h) alone: one 64-thread kernel writes its arguments to a 64-byte buffer.  The helper converts the arguments to
// the kernel's parameter types as kernel<<<...>>>(...) does (an int for an unsigned, a double for a float, a const T& for a 160-byte
// struct by value, a templated kernel instance); a refused launch returns its own status and the next launch on the stream succeeds; the
// hipErrorNotReady of an event query just before a launch is not reported by it.
// Prints "ok: <checks>" and returns 0, or the first failed check and 1.  Driven by tests/test_gpu_launch.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "launch.h"

static int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

struct Big { uint32_t w[40]; };                                             // 160 bytes, by value
static_assert(sizeof(Big) == 160, "the by-value struct of the case");

// out[0] = u, out[1] = the bits of f, out[2] = kTag, out[3 + i] = the sum of big.w[i], w[i + 13], w[i + 26] and w[i + 39] (13 words: all 40 count)
template <uint32_t kTag>
__global__ void k_args(unsigned u, float f, Big big, uint32_t* out) {
    const unsigned t = threadIdx.x;
    if (t == 0) out[0] = u;
    if (t == 1) out[1] = __float_as_uint(f);
    if (t == 2) out[2] = kTag;
    if (t >= 3 && t < 16) {
        uint32_t sum = 0;
        for (unsigned i = t - 3; i < 40; i += 13) sum += big.w[i];
        out[t] = sum;
    }
}

static void expected(unsigned u, float f, uint32_t tag, const Big& big, uint32_t want[16]) {
    want[0] = u; memcpy(&want[1], &f, 4); want[2] = tag;
    for (int t = 3; t < 16; ++t) {
        want[t] = 0;
        for (int i = t - 3; i < 40; i += 13) want[t] += big.w[i];
    }
}

static int read_back(hipStream_t s, const uint32_t* d_out, uint32_t got[16]) {
    CHECK(hipMemcpyAsync(got, d_out, 64, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
    return 0;
}

int main() {
    CHECK(hipSetDevice(0) == hipSuccess);
    hipStream_t s;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    uint32_t* d_out = nullptr;
    CHECK(hipMalloc((void**)&d_out, 64) == hipSuccess);
    Big big;
    for (int i = 0; i < 40; ++i) big.w[i] = 0x9E3779B9u * (uint32_t)(i + 1);
    const Big& big_ref = big;
    uint32_t got[16], ref[16], want[16];

    // ---- conversions: the same arguments through <<< >>> and through lm_launch, both against what the host works out
    const struct { int u; double f; } cases[] = {{7, 0.1}, {-3, 1.0 / 3.0}, {0, -2.5e-40 /* a float denormal */}, {2147483647, 16777217.0 /* rounds in float */}};
    for (const auto& c : cases) {
        CHECK(hipMemsetAsync(d_out, 0xEE, 64, s) == hipSuccess);
        k_args<0xA5u><<<dim3(1), dim3(64), 0, s>>>(c.u, c.f, big_ref, d_out);
        CHECK(hipGetLastError() == hipSuccess);
        if (read_back(s, d_out, ref)) return 1;
        CHECK(hipMemsetAsync(d_out, 0xEE, 64, s) == hipSuccess);
        CHECK(lm::lm_launch(k_args<0xA5u>, dim3(1), dim3(64), 0, s, c.u, c.f, big_ref, d_out) == hipSuccess);
        if (read_back(s, d_out, got)) return 1;
        expected((unsigned)c.u, (float)c.f, 0xA5u, big, want);
        CHECK(memcmp(got, ref, 64) == 0);
        CHECK(memcmp(got, want, 64) == 0);
    }
    // a second instance of the template is another kernel
    CHECK(lm::lm_launch(k_args<0x5Au>, dim3(1), dim3(64), 0, s, 1, 2.0, big_ref, d_out) == hipSuccess);
    if (read_back(s, d_out, got)) return 1;
    expected(1u, 2.0f, 0x5Au, big, want);
    CHECK(memcmp(got, want, 64) == 0);

    // ---- a failure is this launch's own: 2048 threads per block are refused on the host, the next launch on the stream runs
    CHECK(hipMemsetAsync(d_out, 0xEE, 64, s) == hipSuccess);
    CHECK(lm::lm_launch(k_args<0xA5u>, dim3(1), dim3(2048), 0, s, 9, 9.0, big_ref, d_out) != hipSuccess);
    CHECK(lm::lm_launch(k_args<0xA5u>, dim3(1), dim3(64), 0, s, 11, 0.5, big_ref, d_out) == hipSuccess);
    if (read_back(s, d_out, got)) return 1;
    expected(11u, 0.5f, 0xA5u, big, want);
    CHECK(memcmp(got, want, 64) == 0);                                        // written by the second launch alone
    (void)hipGetLastError();                                                 // (the refusal: not left behind for the checks below)

    // ---- no stale error: an event query that may answer hipErrorNotReady, and a launch directly after it
    hipEvent_t ev;
    uint8_t* d_fill = nullptr;
    CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipMalloc((void**)&d_fill, 256) == hipSuccess);
    CHECK(hipMemsetAsync(d_fill, 1, 256, s) == hipSuccess && hipEventRecord(ev, s) == hipSuccess);
    const hipError_t q = hipEventQuery(ev);
    const hipError_t l = lm::lm_launch(k_args<0xA5u>, dim3(1), dim3(64), 0, s, 13, 0.25, big_ref, d_out);
    CHECK(q == hipSuccess || q == hipErrorNotReady);
    CHECK(l == hipSuccess);
    if (read_back(s, d_out, got)) return 1;
    expected(13u, 0.25f, 0xA5u, big, want);
    CHECK(memcmp(got, want, 64) == 0);
    (void)hipGetLastError();                                                 // (hipErrorNotReady, when the query met the memset unfinished)

    CHECK(hipDeviceSynchronize() == hipSuccess);
    CHECK(hipEventDestroy(ev) == hipSuccess && hipFree(d_fill) == hipSuccess && hipFree(d_out) == hipSuccess && hipStreamDestroy(s) == hipSuccess);
    printf("ok: %d\n", checks);
    return 0;
}
