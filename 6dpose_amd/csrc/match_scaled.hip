// Depth-scaled matching: the reference author's third answer to scale, "at each matching pos, scale template depth
// to scene depth" (linemodLevelup/notes.md:1-2, 25-31), dropped there because a template scaled per position read the response maps at random.
// With the scale taken from a ladder of K <= 16 values a scaled feature of entry k is again a fixed offset into a linear memory — base + (j +
// cdy) Wd + (i + cdx) for the position's cell (i, j) — so neighbouring positions of equal k read neighbouring bytes: LINE-MOD's own gather with
// a K-row offset table (ScaledFeat, scaled_kernels.h; built by detector_scaled.cpp).  Three kernels: k_depth_probe (the smallest non-zero
// depth around every pixel), k_coarse_scaled (top level: k from the probed depth, the sum, candidates) and k_local_scaled (one level below the
// top per launch: the 16 x 16 window of the carried k).  The byte linear memories are those of the front end (fe_job_build_lm), whatever the
// response table.  A cell outside the level reads 0: no wrap into the next row or memory (the one departure from the reference's reads).
// Integers throughout; the only float is the score.  The rule itself is stated in tests/scaled_match_ref.py.
#include "launch.h"
#include "match_device.h"
#include "scaled_kernels.h"

namespace lm {

static __device__ __forceinline__ int floor_div(int a, int b) { const int q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// ---- probe map: a separable min-non-zero filter through LDS.  A workgroup owns 64 x 16 pixels: the tile with its halo (0 and pixels outside the
// frame become kNone), row minima over 2 p + 1 columns, then column minima over 2 p + 1 rows.
constexpr int kPW = 64, kPH = 16;
constexpr uint32_t kNone = 0x10000u;            // above every depth
__global__ void __launch_bounds__(256) k_depth_probe(const uint16_t* __restrict__ depth, int W, int H, int p, uint16_t* __restrict__ out) {
    __shared__ uint32_t s_in[kPH + 2 * kScaledMaxProbe][kPW + 2 * kScaledMaxProbe];
    __shared__ uint32_t s_row[kPH + 2 * kScaledMaxProbe][kPW];
    const int x0 = (int)blockIdx.x * kPW, y0 = (int)blockIdx.y * kPH;
    const int tw = kPW + 2 * p, th = kPH + 2 * p;
    for (int t = (int)threadIdx.x; t < tw * th; t += 256) {
        const int ty = t / tw, tx = t - ty * tw;
        const int x = x0 - p + tx, y = y0 - p + ty;
        uint32_t v = kNone;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const uint32_t dd = depth[(size_t)y * W + x];
            if (dd) v = dd;
        }
        s_in[ty][tx] = v;
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < th * kPW; t += 256) {
        const int ty = t >> 6, tx = t & 63;
        uint32_t m = kNone;
        for (int u = 0; u <= 2 * p; ++u) m = min(m, s_in[ty][tx + u]);
        s_row[ty][tx] = m;
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < kPH * kPW; t += 256) {
        const int ty = t >> 6, tx = t & 63;
        uint32_t m = kNone;
        for (int u = 0; u <= 2 * p; ++u) m = min(m, s_row[ty + u][tx]);
        const int x = x0 + tx, y = y0 + ty;
        if (x < W && y < H) out[(size_t)y * W + x] = (uint16_t)(m == kNone ? 0u : m);
    }
}

hipError_t launch_depth_probe(const uint16_t* depth, int W, int H, int probe, uint16_t* out, hipStream_t s) {
    if (probe < 0 || probe > kScaledMaxProbe || W < 1 || H < 1) return hipErrorInvalidValue;
    return lm_launch(k_depth_probe, dim3((W + kPW - 1) / kPW, (H + kPH - 1) / kPH), dim3(256), 0, s, depth, W, H, probe, out);
}

// ---- Coarse pass: one workgroup per work item, its K-row table in LDS, a lane = a cell of the top level.  The lane reads the probe value under
// the template's centre, selects k with 64-bit integer multiplies and sums the features' bytes in 32 bits.  The lanes of a wave are consecutive
// cells of a row: with equal k they read one table word (a broadcast) and consecutive bytes; where k differs the words are neighbours in LDS.
__global__ void __launch_bounds__(256)
k_coarse_scaled(const uint8_t* __restrict__ lm, const uint16_t* __restrict__ probe_map, int W0, int H0, LevelGeom lv, int levels,
                const ScaledEntry* __restrict__ entries, const ScaledFeat* __restrict__ table, ScaledLadder lad, const int32_t* __restrict__ train_depth,
                float threshold, ScaledCand* __restrict__ cands, unsigned int* __restrict__ counter, uint32_t cap) {
    extern __shared__ uint2 s_tab[];
    const int work = (int)blockIdx.x;
    const ScaledEntry e = entries[(size_t)work * levels + (levels - 1)];
    const int K = lad.K, nf = e.nf;
    {
        const uint2* src = reinterpret_cast<const uint2*>(table + e.tab);
        for (int t = (int)threadIdx.x; t < nf * K; t += 256) s_tab[t] = src[t];
    }
    __syncthreads();
    const int T = lv.T, Wd = lv.Wd, Hd = lv.Hd, sh = levels - 1;
    const int wf = floor_div(e.width - 1, T) + 1, hf = floor_div(e.height - 1, T) + 1;
    const long long lim = (long long)(Hd - hf) * Wd + (Wd - wf) + 1;                     // the template's position count (LL.cpp:1299-1309)
    const int limit = (int)max(0ll, min(lim, (long long)Wd * Hd));
    const int offset = T / 2 + (T % 2 - 1);
    const long long t1024 = (long long)train_depth[work] * 1024;
    for (int pos = (int)threadIdx.x; pos < limit; pos += 256) {
        const int j = pos / Wd, i = pos - j * Wd;
        const int px = min(max((i * T + e.width / 2) << sh, 0), W0 - 1), py = min(max((j * T + e.height / 2) << sh, 0), H0 - 1);
        const long long d = probe_map[(size_t)py * W0 + px];
        if (d == 0 || t1024 < (long long)lad.lo * d || t1024 > (long long)lad.hi * d) continue;
        int k = 0;
        long long best = lad.s[0] * d - t1024;
        best = best < 0 ? -best : best;
        for (int q = 1; q < K; ++q) {
            long long v = lad.s[q] * d - t1024;
            v = v < 0 ? -v : v;
            if (v < best) { best = v; k = q; }                                           // a tie stays with the lower entry
        }
        int sum = 0;
        for (int f = 0; f < nf; ++f) {
            const uint2 w = s_tab[f * K + k];
            const int ci = i + (int)(int16_t)(w.y & 0xFFFFu), cj = j + (int)(int16_t)(w.y >> 16);
            if ((unsigned)ci < (unsigned)Wd && (unsigned)cj < (unsigned)Hd) sum += lm[(size_t)w.x + (size_t)cj * Wd + ci];
        }
        const float score = score_of(sum, nf);
        if (score > threshold) {                                                         // LL.cpp:1842-1844
            const unsigned int slot = atomicAdd(counter, 1u);
            if (slot < cap) {
                ScaledCand c;
                c.x = i * T + offset; c.y = j * T + offset; c.score = score; c.work = work; c.k = k; c.depth = (int)d;
                cands[slot] = c;
            }
        }
    }
}

hipError_t launch_coarse_scaled(const uint8_t* lm_arena, const uint16_t* probe_map, int W0, int H0, LevelGeom top, int levels, const ScaledEntry* entries,
                                const ScaledFeat* table, ScaledLadder ladder, const int32_t* train_depth, int num_work, float threshold,
                                ScaledCand* cands, unsigned int* counter, uint32_t cap, size_t lds_bytes, hipStream_t s) {
    if (num_work <= 0) return hipSuccess;
    if (lds_bytes > kScaledMaxLds) return hipErrorInvalidValue;
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_coarse_scaled), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    return lm_launch(k_coarse_scaled, dim3(num_work), dim3(256), std::max<size_t>(lds_bytes, 8), s, lm_arena, probe_map, W0, H0, top, levels, entries, table,
                     ladder, train_depth, threshold, cands, counter, cap);
}

// ---- Refinement of one level: a wave per candidate, lane = window row lane / 4, columns 4 (lane % 4) .. + 3 (four positions per lane, four
// consecutive bytes per feature).  The window is the reference's (LL.cpp:1871-1931): origin cell x / T - 8 of the clamped position, 16 x 16
// cells; the first maximum in raster order wins through the packed key sum << 8 | 255 - position.
__global__ void __launch_bounds__(256)
k_local_scaled(const uint8_t* __restrict__ lm, LevelGeom lv, int level, int levels, const ScaledEntry* __restrict__ entries,
               const ScaledFeat* __restrict__ table, int K, float threshold, ScaledCand* __restrict__ cands, uint32_t n) {
    const int lane = (int)threadIdx.x & 63;
    const uint32_t ci = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (ci >= n) return;
    const ScaledCand c = cands[ci];
    if (c.work < 0) return;
    const ScaledEntry e = entries[(size_t)c.work * levels + level];
    const int T = lv.T, Wd = lv.Wd, Hd = lv.Hd, border = 8 * T, offset = T / 2 + (T % 2 - 1);
    const int x = min(max(c.x * 2 + 1, border), lv.W - e.width - border);                // LL.cpp:1871-1880 (the lower clamp first)
    const int y = min(max(c.y * 2 + 1, border), lv.H - e.height - border);
    const int gx = floor_div(x, T) - 8, gy = floor_div(y, T) - 8;
    const int r = lane >> 2, c0 = (lane & 3) * 4;
    int sum[4] = {0, 0, 0, 0};
    const ScaledFeat* row = table + e.tab + c.k;
    for (int f = 0; f < e.nf; ++f) {
        const ScaledFeat w = row[(size_t)f * K];
        const int cj = gy + r + w.cdy, cx0 = gx + c0 + w.cdx;
        if ((unsigned)cj < (unsigned)Hd) {
            const uint8_t* src = lm + (size_t)w.base + (size_t)cj * Wd;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if ((unsigned)(cx0 + u) < (unsigned)Wd) sum[u] += src[cx0 + u];
        }
    }
    unsigned long long key = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) key = max(key, ((unsigned long long)(uint32_t)sum[u] << 8) | (unsigned long long)(255 - (r * 16 + c0 + u)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, o, 64));
    if (lane == 0) {
        const int rawmax = (int)(key >> 8), best = 255 - (int)(key & 255u);
        const int br = rawmax > 0 ? best >> 4 : -1, bc = rawmax > 0 ? best & 15 : -1;    // LL.cpp:1910-1911
        const float sim = rawmax > 0 ? score_of(rawmax, e.nf) : 0.f;
        ScaledCand o = c;
        o.x = (gx + bc) * T + offset; o.y = (gy + br) * T + offset; o.score = sim;
        if (sim < threshold) o.work = -1;                                                // LL.cpp:1935
        cands[ci] = o;
    }
}

hipError_t launch_local_scaled(const uint8_t* lm_arena, LevelGeom lv, int level, int levels, const ScaledEntry* entries, const ScaledFeat* table, int K,
                               float threshold, ScaledCand* cands, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return lm_launch(k_local_scaled, dim3((n + 3) / 4), dim3(256), 0, s, lm_arena, lv, level, levels, entries, table, K, threshold, cands, n);
}

}  // namespace lm
