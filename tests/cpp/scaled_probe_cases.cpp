// Drives the probe kernel of depth-scaled matching (csrc/match_scaled.hip: k_depth_probe through lm::launch_depth_probe) on depth images a test
// chose.  Inside the library the probe map is visible only as depth_mm under template centres; this program is compiled TOGETHER with
// csrc/match_scaled.hip (the source at the Makefile's device flags, not the shipped object) and writes the whole map back.
// tests/test_gpu_scaled_probe.py writes the case file, runs the program once and compares every pixel.
//
//   scaled_probe_cases <cases> <maps>
//
// cases (little endian):  u32 magic 'SPC1', u32 cases; per case: i32 W, i32 H, i32 probe, then W * H u16 depths (none when W < 1 or H < 1).
// maps:                   per case: i32 status of launch_depth_probe, u32 pixels, then `pixels` u16 of the output buffer, which held 0xABAB in
//                         every pixel before the launch.  pixels = W * H; a case the launcher must refuse (probe outside 0..4, W < 1, H < 1) gets
//                         input and output buffers of one pixel, so that nothing could read or write beyond them.
// Every HIP call but the launcher's own status is checked; the first error ends the program (exit 2) before anything else is launched.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "scaled_kernels.h"

#define HIP_OK(call)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) {                                                                                   \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));                 \
            exit(2);                                                                                              \
        }                                                                                                         \
    } while (0)

static void die(const char* what) {
    fprintf(stderr, "scaled_probe_cases: %s\n", what);
    exit(1);
}

template <class T>
static T take(FILE* f) {
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) die("case file too short");
    return v;
}

template <class T>
static void put(FILE* f, T v) {
    if (fwrite(&v, sizeof(T), 1, f) != 1) die("cannot write the maps");
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: scaled_probe_cases <cases> <maps>");
    FILE* in = fopen(argv[1], "rb");
    if (!in) die("cannot open the case file");
    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot open the output file");
    if (take<uint32_t>(in) != 0x31435053u) die("not a case file");
    const uint32_t cases = take<uint32_t>(in);

    constexpr size_t kMaxPixels = 1u << 20;
    constexpr uint16_t kFill = 0xABABu;
    HIP_OK(hipSetDevice(0));
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    uint16_t *d_in = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc((void**)&d_in, kMaxPixels * sizeof(uint16_t)));
    HIP_OK(hipMalloc((void**)&d_out, kMaxPixels * sizeof(uint16_t)));
    std::vector<uint16_t> depth, map;
    uint32_t refused = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        const int32_t W = take<int32_t>(in), H = take<int32_t>(in), probe = take<int32_t>(in);
        const bool sized = W >= 1 && H >= 1;
        if (sized && (size_t)W * (size_t)H > kMaxPixels) die("a case has more than 2^20 pixels");
        const bool valid = sized && probe >= 0 && probe <= lm::kScaledMaxProbe;
        if (!valid && (W > 1 || H > 1)) die("a case the launcher must refuse is at most 1 x 1");
        // a case the launcher must refuse runs on one-pixel buffers: a launcher that let it through would be caught by its status, not by a fault
        const size_t given = sized ? (size_t)W * (size_t)H : 0, pixels = valid ? given : 1;
        depth.assign(std::max(given, pixels), 0);
        if (given && fread(depth.data(), sizeof(uint16_t), given, in) != given) die("case file too short");
        map.assign(pixels, kFill);
        HIP_OK(hipMemcpyAsync(d_in, depth.data(), pixels * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(d_out, map.data(), pixels * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        HIP_OK(hipStreamSynchronize(s));                          // the staging vectors are reused by the next case
        const hipError_t st = lm::launch_depth_probe(d_in, W, H, probe, d_out, s);
        if (valid) HIP_OK(st);                                    // a refusal of a valid case ends the run like any HIP error
        if (!valid && st == hipSuccess) die("the launcher accepted a case it must refuse; nothing further is launched");
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(map.data(), d_out, pixels * sizeof(uint16_t), hipMemcpyDeviceToHost));
        put<int32_t>(out, (int32_t)st);
        put<uint32_t>(out, (uint32_t)pixels);
        if (fwrite(map.data(), sizeof(uint16_t), pixels, out) != pixels) die("cannot write the maps");
        refused += valid ? 0 : 1;
    }
    if (fclose(out) != 0) die("cannot write the maps");
    fclose(in);
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
    HIP_OK(hipStreamDestroy(s));
    printf("ok: %u cases, %u refused\n", cases, refused);
    return 0;
}
