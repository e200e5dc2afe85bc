// Stand-alone check of the host feature selection with num_features == 0 (what `num_features >> level` gives for
// num_features < 2^level, LL.cpp:560): extract_color_template used to evaluate `cands.size() / num_features` (LL.cpp:632), an integer
// division by zero.  Links host_templates.cpp only, no GPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I6dpose_amd/csrc \
//       tests/cpp/host_templates_zero_features.cpp 6dpose_amd/csrc/host_templates.cpp -o zero_features && ./zero_features
// Exit 0: both extractors refuse num_features == 0 (return false, no features) with and without a mask, and still select with 4.
#include <stdio.h>

#include <vector>

#include "host_templates.h"

int main() {
    const int W = 24, H = 20;
    std::vector<float> mag((size_t)W * H, 0.f);
    std::vector<uint8_t> ang((size_t)W * H, 0), nrm((size_t)W * H, 0), mask((size_t)W * H, 0);
    for (int y = 4; y < 16; ++y)
        for (int x = 5; x < 19; ++x) {
            const size_t o = (size_t)y * W + x;
            mask[o] = 255;
            mag[o] = 4000.f + (float)(x * 7 + y * 3);
            ang[o] = (uint8_t)(1u << ((x + y) & 7));
            nrm[o] = (uint8_t)(x < 12 ? 4 : 32);
        }
    int bad = 0;
    for (int with_mask = 0; with_mask < 2; ++with_mask) {
        const uint8_t* m = with_mask ? mask.data() : nullptr;
        lm::Template c0, n0, c4, n4;
        const bool rc0 = lm::extract_color_template(mag.data(), ang.data(), m, W, H, 0, 55.f, 1, c0);
        const bool rn0 = lm::extract_normal_template(nrm.data(), m, W, H, 0, 1, 1, n0);
        const bool rc4 = lm::extract_color_template(mag.data(), ang.data(), m, W, H, 4, 55.f, 0, c4);
        const bool rn4 = lm::extract_normal_template(nrm.data(), m, W, H, 4, 1, 0, n4);
        printf("mask %d: num_features 0 -> colour %d (%zu features), normal %d (%zu features); num_features 4 -> colour %d (%zu), normal %d (%zu)\n",
               with_mask, (int)rc0, c0.features.size(), (int)rn0, n0.features.size(), (int)rc4, c4.features.size(), (int)rn4, n4.features.size());
        bad += rc0 || rn0 || !c0.features.empty() || !n0.features.empty();
        bad += !rc4 || !rn4 || c4.features.size() != 4 || n4.features.size() != 4;
    }
    if (bad) { printf("FAILED\n"); return 1; }
    printf("ok\n");
    return 0;
}
