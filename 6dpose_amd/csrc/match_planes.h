// The stages that the bit-plane kernels share (match_bits.hip: k_coarse_bits, k_coarse_bits_batch, k_local_bits, k_pack_*; match_wide.hip:
// k_coarse_wide, k_local_wide, k_pack_*_wide; match_parts.hip: k_coarse_parts, k_local_parts; DESIGN.md sections 3.1, 3.1.2, 3.1.3, 3.1.4), each once: every one of them states a rule of the
// reference (LL.cpp:1299-1309, 1842-1852, 1871-1880, 1910-1935), so a change to a rule is made here and reaches every kernel.  What differs
// between the kernels stays in them: how a lane finds its loads, how many counters it keeps (two or three) and, in the coarse pass, how the
// candidate slots are reserved.  Everything is __forceinline__ and takes values: the kernels keep their registers, LDS and launch bounds.
#pragma once
#include "match_device.h"
#include <type_traits>

namespace lm {

// ================================================== coarse pass (top level, pair stream) ==================================================

// the smallest raw sum whose score passes (score_of is monotone in raw): LL.cpp:1844 `> threshold`; 4 nf + 1 when none does
static __device__ __forceinline__ int coarse_rmin(float threshold, int nf) {
    int rmin = (int)(threshold * (float)(4 * nf) / 100.f);
    if (!(rmin >= 0)) rmin = 0;
    if (rmin > 4 * nf + 1) rmin = 4 * nf + 1;
    while (rmin > 0 && score_of(rmin, nf) > threshold) --rmin;
    while (rmin <= 4 * nf && !(score_of(rmin, nf) > threshold)) ++rmin;
    return rmin;
}

// ... and the smallest raw sum whose score is >= threshold, the test a refined candidate must not fail (LL.cpp:1935 drops `sim < threshold`)
static __device__ __forceinline__ int local_rmin(float threshold, int nf) {
    int rmin = (int)(threshold * (float)(4 * nf) / 100.f);
    if (!(rmin >= 0)) rmin = 0;
    if (rmin > 4 * nf + 1) rmin = 4 * nf + 1;
    while (rmin > 0 && score_of(rmin - 1, nf) >= threshold) --rmin;
    while (rmin <= 4 * nf && !(score_of(rmin, nf) >= threshold)) ++rmin;
    return rmin;
}

// What a wave knows about its template on the top level.  work_raw = the template the wave was dealt (a wave per template, or several waves)
struct CoarseHead {
    bool live;                  // work_raw is a template; idle waves of the last workgroup shadow a real one (work) and emit nothing
    int work, nf, nfp;          // work-list index, true and padded feature count of its top-level entry
    const int32_t* fo;          // the entry's feature offsets (bytes into the flat linear memories)
    int Wd, T, npos;            // the level's map: width, sampling step, positions
    int limit;                  // positions that carry sums: the template's position count (LL.cpp:1299-1309), at most npos
    int offset;                 // of a cell's centre, LL.cpp:1846
    int rmin;                   // coarse_rmin
    bool zero_passes;           // a raw sum of 0 passes: the positions without sums are hits too
};
static __device__ __forceinline__ CoarseHead coarse_head(int work_raw, int num_work, const TemplEntry* __restrict__ entries, const int32_t* __restrict__ feat_off,
                                                         const int32_t* __restrict__ work_pyramids, const LevelGeom& lv, int level, int levels, float threshold) {
    CoarseHead h;
    h.live = work_raw < num_work;
    h.work = h.live ? work_raw : num_work - 1;
    const int pyr = work_pyramids[h.work];
    const TemplEntry e = entries[(size_t)pyr * levels + level];
    h.nf = e.nf; h.nfp = e.nf_padded;
    h.fo = feat_off + e.feat_start;
    const int Hd = lv.Hd;
    h.Wd = lv.Wd; h.T = lv.T; h.npos = h.Wd * Hd;
    const int wf = (e.width - 1) / h.T + 1, hf = (e.height - 1) / h.T + 1;  // LL.cpp:1299-1309
    const int tp = (Hd - hf) * h.Wd + (h.Wd - wf) + 1;
    h.offset = h.T / 2 + (h.T % 2 - 1);
    h.limit = tp < h.npos ? tp : h.npos;
    h.rmin = coarse_rmin(threshold, h.nf);
    h.zero_passes = score_of(0, h.nf) > threshold;
    return h;
}

// The hits among the 32 positions [pos0, pos0 + 32) of a lane whose bit-sliced sums are S: S >= rmin as a bit-sliced comparison (rmin is
// wave-uniform), so integers are formed only for the hits.  Positions at or beyond the template's position count hold zero sums
// (LL.cpp:1299-1309): they are hits only if zero passes.  summed = the lane's positions that carry sums.
template <int kS>
static __device__ __forceinline__ uint32_t coarse_hit_mask(const uint32_t (&S)[kS], int rmin, bool zero_passes, int limit, int npos, int pos0, uint32_t& summed) {
    uint32_t gt = 0, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int k = kS - 1; k >= 0; --k) {
        if ((rmin >> k) & 1) eq &= S[k];
        else { gt |= eq & S[k]; eq &= ~S[k]; }
    }
    const uint32_t hit_mask = rmin < (1 << kS) ? (gt | eq) : 0u;
    const int sums = limit - pos0;
    summed = sums >= 32 ? 0xFFFFFFFFu : (sums > 0 ? (1u << sums) - 1u : 0u);
    const int inmap = npos - pos0;
    const uint32_t mapped = inmap >= 32 ? 0xFFFFFFFFu : (inmap > 0 ? (1u << inmap) - 1u : 0u);
    return (hit_mask & summed) | (zero_passes ? (mapped & ~summed) : 0u);
}

// The candidate slots of a workgroup of four waves (k_coarse_bits, k_coarse_wide): ONE atomic per workgroup and pass on the frame's counter
// (same-address atomics serialise in the L2: 2000 per frame cost the byte kernel 16 us).  Returns the lane's first slot; total = the wave's hits.
// Every wave of the workgroup calls it, once per pass.
static __device__ __forceinline__ unsigned long long coarse_reserve_slots(uint32_t (&s_tot)[4], unsigned long long& s_base, unsigned long long* __restrict__ counters,
                                                                          uint32_t hit_mask, int lane, int wave, int& total) {
    const int before = wave_excl_scan(__popc(hit_mask), lane, total);
    if (lane == 0) s_tot[wave] = (uint32_t)total;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long all = (unsigned long long)s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
        s_base = all ? atomicAdd(&counters[0], all) : 0ull;
    }
    __syncthreads();
    unsigned long long slot = s_base + (unsigned long long)before;
    for (int w = 0; w < wave; ++w) slot += s_tot[w];
    __syncthreads();                                                        // s_tot / s_base are rewritten by the next pass
    return slot;
}

// The lane's hits as candidates in the slots from `slot` on, in raster order; past the capacity the slots count on and nothing is written.
// The raw sum is rebuilt from the slices for positions that carry sums only (the others are zero by rule, whatever the slices hold).
template <int kS>
static __device__ __forceinline__ void coarse_emit(uint32_t hit_mask, uint32_t summed, const uint32_t (&S)[kS], unsigned long long slot, uint32_t cap, int pos0,
                                                   int Wd, int T, int offset, int nf, int work, Candidate* __restrict__ cands) {
    uint32_t m = hit_mask;
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1;
        if (slot < cap) {
            int raw = 0;
            if ((summed >> b) & 1u) {
#pragma unroll
                for (int k = 0; k < kS; ++k) raw |= (int)((S[k] >> b) & 1u) << k;
            }
            const int jpos = pos0 + b;
            const int cy = jpos / Wd, cx = jpos - cy * Wd;
            Candidate c;
            c.x = cx * T + offset; c.y = cy * T + offset; c.score = score_of(raw, nf); c.work = work;
            cands[slot] = c;
        }
        ++slot;
    }
}

// ================================================ refinement (levels below the top, strip records) ================================================

// The wave's share of the candidate groups: frames [f_lo, f_hi), groups w_first, w_first + w_step, ...
// Frame -> XCD affinity as in k_local (an XCD's L2 holds ONE frame's planes), for ANY batch size up to 8: frame f is served by the workgroups of
// the XCDs x with x % nb == f — 8 / nb of them each when nb divides 8, else some frames get one XCD more than others.  (Round 3 fell back to
// dealing the items of all frames to all workgroups unless nb divided 8: a 5-frame launch — the first and last launches of a short stream —
// then cost 35 us per frame against 26 in an 8-frame launch.)
struct LocalShare { int f_lo, f_hi; uint32_t w_first, w_step; };
static __device__ __forceinline__ LocalShare local_share(int nb) {
    LocalShare s;
    s.f_lo = 0; s.f_hi = nb;
    s.w_first = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s.w_step = gridDim.x * (blockDim.x >> 6);
    if (nb > 1 && nb <= 8 && (gridDim.x & 7) == 0) {
        const int xcd = (int)(blockIdx.x & 7);
        s.f_lo = xcd % nb; s.f_hi = s.f_lo + 1;
        const uint32_t mine = (uint32_t)((7 - s.f_lo) / nb + 1);    // XCDs serving this frame: f_lo, f_lo + nb, ...
        const uint32_t wpb = blockDim.x >> 6;
        s.w_first = ((blockIdx.x >> 3) * mine + (uint32_t)(xcd / nb)) * wpb + (threadIdx.x >> 6);
        s.w_step = (gridDim.x >> 3) * mine * wpb;
    }
    return s;
}

// Prologue: every frame's candidate count (at most cand_cap) and zeroed statistics in LDS, then k_dedupe's hash table, emptied here like k_local does
static __device__ __forceinline__ void local_prologue(const FrameBatch& fb, uint32_t (&s_cnt)[kMaxBatch], unsigned long long (&s_acc)[kMaxBatch][2], uint32_t cand_cap,
                                                      uint32_t dedupe_cap_slots) {
    const int nb = fb.nb;
    if ((int)threadIdx.x < nb) {
        const unsigned long long nc = fb.f[threadIdx.x].counters[0] & kCandMask;
        s_cnt[threadIdx.x] = nc < cand_cap ? (uint32_t)nc : cand_cap;
        s_acc[threadIdx.x][0] = 0; s_acc[threadIdx.x][1] = 0;
    }
    __syncthreads();
    for (int f = 0; f < nb; ++f) {
        unsigned long long* table = fb.f[f].dedupe_table;
        if (!table) continue;
        const uint32_t tsize = dedupe_slots_for(s_cnt[f], dedupe_cap_slots);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < tsize; i += gridDim.x * blockDim.x) table[i] = ~0ull;
    }
}

// A candidate's 16 x 16 window on one level: LL.cpp:1871-1880 (the clamp) and 1380-1381 (window origin), exactly as k_local
struct LocalWindow {
    int x, y;                   // the candidate's position on this level, clamped
    int gx, gy;                 // window origin in cells: x / T - 8, y / T - 8
    bool all_in;                // every feature's window lies inside its plane: the strip records can serve it
    bool run;                   // this lane's candidate is evaluated on this level
    int nf, nfp;                // feature count of the entry; padded count, 0 when not run
    int nmax;                   // the wave's largest nfp (wave-uniform)
    uint32_t Kbase, gxl;        // record offset of the origin's strip and row; the origin's column inside its strip
    uint32_t zero_off, HS8;     // the level's all-zero plane (in either arena); bytes from a strip's records to the next strip's
};
// leave: k_local's per-candidate path takes this candidate (from the top) — set here for a live candidate whose windows leave their planes
static __device__ __forceinline__ LocalWindow local_window(const LevelGeom& lv, const TemplEntry& e, int mx, int my, bool alive, bool& leave) {
    LocalWindow w;
    const int T = lv.T, W = lv.W, H = lv.H, Wd = lv.Wd, Hd = lv.Hd;
    const int border = 8 * T;
    w.HS8 = (uint32_t)Hd * 8u;
    w.zero_off = (lv.sm_off[1] + 8u * (uint32_t)(T * T) * ((uint32_t)lv.NS * (uint32_t)Hd * 16u)) >> 1;
    const int max_x = W - e.width - border, max_y = H - e.height - border;
    int x = mx * 2 + 1, y = my * 2 + 1;
    x = x > border ? x : border;  y = y > border ? y : border;
    x = x < max_x ? x : max_x;    y = y < max_y ? y : max_y;
    w.x = x; w.y = y;
    w.gx = x / T - 8; w.gy = y / T - 8;
    const int off_x = w.gx * T, off_y = w.gy * T;
    w.all_in = e.min_x >= 0 && e.min_y >= 0 && w.gx >= 0 && w.gy >= 0 &&
               ((e.max_x + off_x) / T + 16 <= Wd) && ((e.max_y + off_y) / T + 16 <= Hd);
    const bool want = alive && !leave;
    leave = leave || (want && !w.all_in);                           // (as an expression: `if (...) leave = true` costs k_local_bits / k_local_wide a VGPR)
    w.run = want && w.all_in;
    w.nf = e.nf; w.nfp = w.run ? (int)e.nf_padded : 0;
    int nmax = w.nfp;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(nmax, o, 64); nmax = t > nmax ? t : nmax; }
    w.nmax = __builtin_amdgcn_readfirstlane(nmax);
    w.Kbase = (uint32_t)(((w.gx >> 4) * Hd + w.gy) * 8);
    w.gxl = (uint32_t)(w.gx & 15);
    return w;
}

// lane j fetches the words of features f0 + 2j, f0 + 2j + 1 (entries start at multiples of 8 words, f0 is a multiple of 16)
static __device__ __forceinline__ uint2 local_fetch(const uint32_t* fw, int f0, int j, int nfp) {
    uint2 w = make_uint2(0u, 0u);
    if (f0 + 2 * j < nfp) w = *reinterpret_cast<const uint2*>(fw + f0 + 2 * j);
    return w;
}
// a feature word (base0 | column class, lm_kernels.h) -> offset of its first record in the bit arena(s), 2 x the window's cell inside it
static __device__ __forceinline__ void local_prep(uint32_t w, bool on, uint32_t gxl, uint32_t Kbase, uint32_t HS8, uint32_t zero_off, uint32_t& off, uint32_t& s2) {
    s2 = ((w & 15u) + gxl) << 1;
    const uint32_t o = ((w & ~15u) >> 1) + Kbase + ((s2 >> 5) ? HS8 : 0u);
    off = on ? o : zero_off;                                        // beyond this candidate's features (or no candidate): the zero plane
}

// The counters of the lane's two rows (cA: row 2j, cB: row 2j + 1; even bits one plane, odd bits the other) side by side per plane: bit 2c = row 2j,
// bit 2c + 1 = row 2j + 1 of window column c
template <int kN>
static __device__ __forceinline__ void local_interleave(uint32_t (&n1)[kN], uint32_t (&n4)[kN], const uint32_t (&cA)[kN], const uint32_t (&cB)[kN]) {
#pragma unroll
    for (int k = 0; k < kN; ++k) {
        n1[k] = (cA[k] & 0x55555555u) | ((cB[k] << 1) & 0xAAAAAAAAu);
        n4[k] = ((cA[k] >> 1) & 0x55555555u) | (cB[k] & 0xAAAAAAAAu);
    }
}

// The candidate's maximum over its 16 x 16 window and the FIRST position attaining it in raster order, from the bit-sliced sums S of the lanes'
// interleaved rows: the lane's maximum by a descent from the top bit, the candidate's by three exchanges among its 8 lanes (a key of the
// value above 255 - position).  raw <= 0: br = bc = -1, LL.cpp:1910-1911.
template <int kS>
static __device__ __forceinline__ void local_argmax(const uint32_t (&S)[kS], int j, int& raw, int& br, int& bc) {
    uint32_t mask = 0xFFFFFFFFu, val = 0;
#pragma unroll
    for (int k = kS - 1; k >= 0; --k) {
        const uint32_t t = mask & S[k];
        if (t) { mask = t; val |= 1u << k; }
    }
    const uint32_t upper = mask & 0x55555555u;                      // positions of row 2j attaining the maximum come first in raster order
    const uint32_t pick = upper ? upper : mask;
    const uint32_t bitp = (uint32_t)__ffs((int)pick) - 1u;
    const uint32_t pos = ((2u * (uint32_t)j + (bitp & 1u)) << 4) + (bitp >> 1);   // row * 16 + column
    uint32_t key = (val << 8) | (255u - pos);
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)key, o, 64); key = t > key ? t : key; }
    raw = (int)(key >> 8);
    br = -1; bc = -1;
    if (raw > 0) {
        const int idx = 255 - (int)(key & 0xFF);
        br = idx >> 4; bc = idx & 15;
    }
}

// What a level leaves of an evaluated candidate: its score and position (LL.cpp:1930-1931), dropped below the threshold (LL.cpp:1935)
static __device__ __forceinline__ void local_update(const LocalWindow& w, int T, int raw, int br, int bc, float threshold, float& sim, int& mx, int& my, bool& alive,
                                                    uint32_t& evals, uint32_t& bytes) {
    const float best = raw > 0 ? score_of(raw, w.nf) : 0.f;
    if (w.run) {
        const int offset = T / 2 + (T % 2 - 1);
        ++evals;
        bytes += 256u * (uint32_t)w.nf;                             // algorithmic response bytes of this 16x16 evaluation
        sim = best;
        mx = (w.x / T - 8 + bc) * T + offset;
        my = (w.y / T - 8 + br) * T + offset;
        if (sim < threshold) alive = false;
    }
}

// Epilogue of a candidate (its lane 0): the `todo` mark, the refined record (work = -1: dropped) unless k_local takes the candidate, the statistics
static __device__ __forceinline__ void local_store(const FrameSlot& F, uint32_t ci, bool leave, uint32_t cap, int mx, int my, float sim, bool alive, int work,
                                                   unsigned long long (&acc)[2], uint32_t evals, uint32_t bytes) {
    F.todo[ci] = leave ? 1 : 0;
    if (!leave) {
        if (ci < cap) {
            Candidate m;
            m.x = mx; m.y = my; m.score = sim;
            m.work = alive ? work : -1;
            F.matches_dev[ci] = m;
        }
        atomicAdd(&acc[0], (unsigned long long)evals);
        atomicAdd(&acc[1], (unsigned long long)bytes);
    }
}
// ... and of the workgroup: its statistics into one of the frame's shards
static __device__ __forceinline__ void local_flush_stats(const FrameBatch& fb, unsigned long long (&s_acc)[kMaxBatch][2]) {
    __syncthreads();
    if ((int)threadIdx.x < fb.nb && s_acc[threadIdx.x][0] != 0) {
        unsigned long long* st = fb.f[threadIdx.x].counters + 8 + 2 * (blockIdx.x & (kStatShards - 1));
        atomicAdd(st, s_acc[threadIdx.x][0]);
        atomicAdd(st + 1, s_acc[threadIdx.x][1]);
    }
}

// ================================================================ packing ================================================================

// bit sh of each of 16 response bytes -> 16 bits (the multiply gathers bit sh of 4 bytes into 4 bits)
static __device__ __forceinline__ uint32_t byte_bits16(const uint4& v, int sh) {
    auto four = [](uint32_t d, int sh) -> uint32_t { return ((((d >> sh) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; };
    return four(v.x, sh) | (four(v.y, sh) << 4) | (four(v.z, sh) << 8) | (four(v.w, sh) << 12);
}
// ... of the 32 bytes of a pair of the pair stream
static __device__ __forceinline__ uint32_t byte_bits32(const uint4& a, const uint4& b, int sh) { return byte_bits16(a, sh) | (byte_bits16(b, sh) << 16); }

// Strip record i = ((plane * NS + s) * Hd + row) of a level whose strip bytes start at sm_off0: the 32 cells [16 s, 16 s + 32) of its row are two
// 16-byte rows of the strip arena, a (strip s) and b (strip s + 1, zero behind the last strip); returns the record's byte offset in a bit arena
static __device__ __forceinline__ size_t strip_cells(const uint8_t* strips, uint32_t sm_off0, uint32_t i, int NS, int Hd, uint4& a, uint4& b) {
    const uint32_t q = i / (uint32_t)Hd, s = q % (uint32_t)NS;
    const uint8_t* src = strips + sm_off0 + (size_t)i * 16;
    a = *reinterpret_cast<const uint4*>(src);
    b = make_uint4(0, 0, 0, 0);
    if (s + 1 < (uint32_t)NS) b = *reinterpret_cast<const uint4*>(src + (size_t)Hd * 16);      // the next strip of this row
    return (sm_off0 >> 1) + (size_t)i * 8;
}

// ============================================================ launching ============================================================

// The instantiation for a bank and a table, for every two-plane kernel: counters of 9 bits (kHi = 5) for entries of up to kBitsSmallMax features, of
// 14 (kHi = 10) beyond, each at the waves per SIMD the kernel declares for it; kA = the table's low weight.  launch(kHi, kWaves, kA) receives them
// as std::integral_constants, i.e. as template arguments, and its status is the result.
template <int kWavesSmall, int kWavesBig, class Launch>
[[nodiscard]] static hipError_t with_bits_instance(int max_features, int low_weight, Launch launch) {
    auto with_a = [&](auto a) {
        if (max_features > kBitsSmallMax) return launch(std::integral_constant<int, 10>(), std::integral_constant<int, kWavesBig>(), a);
        return launch(std::integral_constant<int, 5>(), std::integral_constant<int, kWavesSmall>(), a);
    };
    if (low_weight == 2) return with_a(std::integral_constant<int, 2>());
    if (low_weight == 3) return with_a(std::integral_constant<int, 3>());
    return with_a(std::integral_constant<int, 1>());
}

}  // namespace lm
