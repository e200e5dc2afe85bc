// Drives the pack kernels of the multi-GPU exchange (csrc/exchange.hip: k_exchange_sort256, k_exchange_merge256) on key buffers a test chose.
// Inside the library they read the detector's own key buffer, which no public call can fill; this program is compiled TOGETHER with
// csrc/exchange.hip (the source at the Makefile's device flags, not the shipped object), fills lm::XchgFrame by hand and calls
// lm::launch_exchange_pack_group.  tests/test_gpu_exchange_keys.py writes the case file, runs the program once and compares the blocks.
//
//   exchange_pack_keys <cases> <blocks>
//
// cases (little endian):  u32 magic 'XPK1', u32 launches, u32 fill; per launch: u32 frames (1..3), u32 cap, u32 cand_cap; per frame: u32 keys,
//                         u64 counters[8], `keys` 128-bit keys {hi, lo}.
// blocks:                 per launch and frame the 4 + 4 * cap words of the block, which held `fill` in every word before the launch.
// Every HIP call is checked; the first error ends the program (exit 2) before anything else is launched.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lm_kernels.h"

#define HIP_OK(call)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) {                                                                                   \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));                 \
            exit(2);                                                                                              \
        }                                                                                                         \
    } while (0)

static void die(const char* what) {
    fprintf(stderr, "exchange_pack_keys: %s\n", what);
    exit(1);
}

template <class T>
static T take(FILE* f) {
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) die("case file too short");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: exchange_pack_keys <cases> <blocks>");
    FILE* in = fopen(argv[1], "rb");
    if (!in) die("cannot open the case file");
    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot open the output file");
    if (take<uint32_t>(in) != 0x314B5058u) die("not a case file");
    const uint32_t launches = take<uint32_t>(in), fill = take<uint32_t>(in);

    constexpr int kFrames = 3;
    ulonglong2 *d_keys[kFrames], *d_runs[kFrames];
    unsigned long long* d_counters[kFrames];
    uint32_t* d_block[kFrames];
    const size_t max_keys = (size_t)lm::kXchgMaxCapacity + 1, max_block = 4 + 4 * (size_t)lm::kXchgMaxCapacity;
    HIP_OK(hipSetDevice(0));
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    for (int i = 0; i < kFrames; ++i) {
        HIP_OK(hipMalloc((void**)&d_keys[i], max_keys * sizeof(ulonglong2)));
        HIP_OK(hipMalloc((void**)&d_runs[i], (size_t)lm::kXchgMaxCapacity * sizeof(ulonglong2)));
        HIP_OK(hipMalloc((void**)&d_counters[i], 8 * sizeof(unsigned long long)));
        HIP_OK(hipMalloc((void**)&d_block[i], max_block * sizeof(uint32_t)));
    }
    std::vector<ulonglong2> keys;
    std::vector<uint32_t> block;
    for (uint32_t l = 0; l < launches; ++l) {
        const uint32_t frames = take<uint32_t>(in), cap = take<uint32_t>(in), cand_cap = take<uint32_t>(in);
        if (frames < 1 || frames > (uint32_t)kFrames) die("1 to 3 frames per launch");
        if (cap < 256 || cap > lm::kXchgMaxCapacity || (cap & (cap - 1))) die("capacity must be a power of two in [256, 65536]");
        const size_t words = 4 + 4 * (size_t)cap;
        lm::XchgGroup G{};
        G.n = (int)frames;
        for (uint32_t i = 0; i < frames; ++i) {
            const uint32_t n = take<uint32_t>(in);
            unsigned long long counters[8];
            for (int c = 0; c < 8; ++c) counters[c] = take<uint64_t>(in);
            if (n > max_keys) die("too many keys");
            // the kernels read keys[0 .. counters[1]) unless a flag is set (more than cap records, a field or candidate overflow): the buffer must hold them
            const bool flagged = counters[0] > cand_cap || counters[1] > cap || counters[3] != 0;
            if (!flagged && counters[1] > n) die("counters[1] exceeds the keys of the frame");
            keys.resize(n);
            if (n && fread(keys.data(), sizeof(ulonglong2), n, in) != n) die("case file too short");
            block.assign(words, fill);
            if (n) HIP_OK(hipMemcpyAsync(d_keys[i], keys.data(), n * sizeof(ulonglong2), hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(d_counters[i], counters, sizeof(counters), hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(d_block[i], block.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            HIP_OK(hipStreamSynchronize(s));                      // the staging vectors are reused by the next frame
            G.f[i].keys = d_keys[i];
            G.f[i].counters = d_counters[i];
            G.f[i].runs = d_runs[i];
            G.f[i].block = d_block[i];
        }
        HIP_OK(lm::launch_exchange_pack_group(G, cand_cap, cap, s));
        HIP_OK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < frames; ++i) {
            block.resize(words);
            HIP_OK(hipMemcpy(block.data(), d_block[i], words * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (fwrite(block.data(), sizeof(uint32_t), words, out) != words) die("cannot write the blocks");
        }
    }
    if (fclose(out) != 0) die("cannot write the blocks");
    fclose(in);
    for (int i = 0; i < kFrames; ++i) {
        HIP_OK(hipFree(d_keys[i]));
        HIP_OK(hipFree(d_runs[i]));
        HIP_OK(hipFree(d_counters[i]));
        HIP_OK(hipFree(d_block[i]));
    }
    HIP_OK(hipStreamDestroy(s));
    printf("ok: %u launches\n", launches);
    return 0;
}
