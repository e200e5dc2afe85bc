// Interface between detector_scaled.cpp and match_scaled.hip: depth-scaled matching (the rule is stated in
// tests/scaled_match_ref.py).  gfx950 only.  Not part of the public C ABI.
#pragma once
#include "lm_kernels.h"

namespace lm {

constexpr int kScaledMaxLadder = 16;            // entries of the scale ladder
constexpr size_t kScaledMaxLds = 160 * 1024;    // LDS of a CU: the largest K-row table k_coarse_scaled can hold
constexpr int kScaledMaxProbe = 4;

// One scaled feature of one ladder entry: the byte of modality block + label + phase plane `base` (an offset into the LM arena) at cell
// (i + cdx, j + cdy) of the position's cell (i, j); outside [0, Wd) x [0, Hd) the response is 0.
struct ScaledFeat { uint32_t base; int16_t cdx, cdy; };
static_assert(sizeof(ScaledFeat) == 8, "a table element is one 8-byte LDS read");
// One (work item, level): its table is tab[(f * K + k)], f < nf — the K ladder entries of a feature side by side, so that lanes of a wave that
// differ in k read consecutive 8-byte words (K <= 16 of them: 32 distinct banks, no conflict; equal k broadcasts).
struct ScaledEntry { uint32_t tab; int32_t nf, width, height; };
struct ScaledCand { int32_t x, y; float score; int32_t work, k, depth; };   // work < 0: dropped by the refinement
struct ScaledLadder { int32_t K, lo, hi; int32_t s[kScaledMaxLadder]; };    // Q10 scales, ascending; bounds lo <= d_train * 1024 / d <= hi

// probe map: out[y * W + x] = the smallest non-zero depth of the (2 probe + 1)^2 window around (x, y) clipped to the frame, 0 if there is none
[[nodiscard]] hipError_t launch_depth_probe(const uint16_t* depth, int W, int H, int probe, uint16_t* out, hipStream_t s);
// One workgroup per work item; counter[0] += candidates (may exceed cap: nothing is written past cap).  lds_bytes = K * (largest nf) * 8.
[[nodiscard]] hipError_t launch_coarse_scaled(const uint8_t* lm_arena, const uint16_t* probe_map, int W0, int H0, LevelGeom top, int levels, const ScaledEntry* entries,
                                              const ScaledFeat* table, ScaledLadder ladder, const int32_t* train_depth, int num_work, float threshold,
                                              ScaledCand* cands, unsigned int* counter, uint32_t cap, size_t lds_bytes, hipStream_t s);
// Level `level` (below the top) for the n candidates, in place: position, score, work = -1 for a dropped one.
[[nodiscard]] hipError_t launch_local_scaled(const uint8_t* lm_arena, LevelGeom lv, int level, int levels, const ScaledEntry* entries, const ScaledFeat* table, int K,
                                             float threshold, ScaledCand* cands, uint32_t n, hipStream_t s);

}  // namespace lm
