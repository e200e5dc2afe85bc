// Similarity kernels of Detector::matchClass on gfx950, on byte planes (reference LL.cpp:1284-1428 similarity /
// similarityLocal, LL.cpp:1788-1941 matchClass): k_coarse with its tile planner, k_local, launch_coarse, launch_local,
// tile_plan_possible, coarse_plan_lds_bytes.  The bit-plane kernels (k_local_bits, k_coarse_bits and their packers) are in
// match_bits.hip, what both use in match_device.h.  Pure integer byte work: every response is a
// u8 in {0,1,4}, summed per template position.  Nothing here is a dense contraction, so no MFMA;
// the linear memories of one frame (1.2 MB coarse + 4.9 MB fine at VGA) live in L2 / Infinity
// Cache; the byte kernels (k_coarse, k_local) are bound by the vector-L1 access rate (see "Gather discipline" below), the bit-plane refinement
// (k_local_bits, the default) by the number of 16-byte wave loads it issues — not by HBM and not by arithmetic.
//
// Data layout (built by fe_quant.hip, fe_bits.hip / detector_frame.cpp, offsets in FrameGeom):
//   LM arena: per level, per modality: u8 [8 labels][T*T phases][(W/T)*(H/T)] + zero tail.
//   Bank:     TemplEntry per (pyramid, level).  Its features (both modalities) are sorted by alignment
//             class and padded to a multiple of kFeatBatch with entries that read zeros, so the inner
//             loops are branch-free.  feat_off[] = byte offset of the feature's linear-memory run
//             from the arena start (accessLinearMemory, LL.cpp:1248-1271, resolved on the host for
//             the current frame geometry with floor division, so adding a multiple-of-T window
//             offset stays exact).  At the top level, features outside the image (LL.cpp:1330) are
//             already redirected to the zero tail.  feat_xy[] = int16 x | int16 y << 16 is only
//             read on the slow path of the refinement (bounds test of LL.cpp:1394).
#include <algorithm>

#include "launch.h"
#include "knobs.h"
#include "match_device.h"

namespace lm {

static __device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);   // unaligned global_load_dword (gfx950 unaligned access mode)
    return v;
}

// ---------------------------------------------------------------------------------------------
// Gather discipline (measured, profiles/r01_pmc_*.txt): the vector L1 (TCP) services one access per
// cycle and an access moves at most 64 aligned bytes.  Unaligned or narrow per-lane gathers explode
// into 3-4 accesses per quad of lanes and the kernels become TCP-access bound, so both kernels only
// issue ALIGNED 16-byte loads (1 KB per wave instruction in 16 accesses).  The byte misalignment of
// a feature's run is handled without per-feature shifting: the host sorts the features of every
// template entry by their alignment class (run offset mod 16), the kernel adds the aligned chunks of
// one class into packed-u8 accumulators (<= 63 features x 4 < 256, the reference's own no-overflow
// argument, README.md:67-69) and realigns ONCE per class run (v_alignbyte + one neighbour exchange)
// into the u16 position accumulators.
// ---------------------------------------------------------------------------------------------

// widen 4 packed bytes of `v` into two packed u16x2 accumulators: e gets bytes 0,2 ; o gets bytes 1,3
static __device__ __forceinline__ void add_bytes(uint32_t v, uint32_t& e, uint32_t& o) {
    e += v & 0x00FF00FFu;
    o += (v >> 8) & 0x00FF00FFu;
}

static __device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------
// Coarse pass (LL.cpp:1284-1354 similarity + :1835-1852 scan): one workgroup per template pyramid.
// Lane i of wave w owns the 16 positions [16*(63w+i), +16) of the decimated top-level grid and loads
// the aligned 16-byte chunk that starts at or before them; the tail of its positions lives in lane
// i+1's chunk, hence 63 producing lanes per wave plus one feeder lane.
// ---------------------------------------------------------------------------------------------
constexpr int kChunksPerWave = 63;
constexpr int kMaxTilesPerTemplate = 48;       // tiles planned per template and frame (more candidates stay singles)
constexpr int kPlanHits = 64;                  // hits per template (raster order) the planner looks at: one per lane

// Everything the planner of k_coarse needs to know about the level below the top (two-level pyramids whose coarse cells are
// kTileStep fine cells apart; plan.enabled == 0 otherwise).
struct TilePlanGeom {
    int enabled;                               // the hits of a workgroup's templates are collected in LDS and their slots reserved with ONE atomic
    int tiles;                                 // ... and grouped into tiles (k_local's tile path); 0: every hit stays a single (bit-plane refinement: it needs no tiles)
    int W0, H0, T0, Wd0, Hd0;                  // level 0: image size, step, decimated grid
    uint32_t tile_cap;
    int dbg;                                   // LM_COARSE_DBG (timing experiments only): 1 = no grouping, 2 = no global atomic (wrong results)
};

static __device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
static __device__ __forceinline__ unsigned long long bcast_u64(unsigned long long v, int src) {
    return ((unsigned long long)(uint32_t)__shfl((int)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}

// A workgroup serves `group` templates at once, `wpt` waves each (blockDim = group * wpt * 64).  With tile planning ONE atomic
// per WORKGROUP reserves the candidate slots and the tile records of all its templates.  (Measured, 2000 templates at VGA: a
// workgroup per template with its own atomic on the frame's counter word takes 47 us, 17 us of them queueing at that word —
// the L2 serialises same-address atomics at ~120 per us — and a second atomic for the tiles another 20 us; without atomics the
// pass takes 31 us.)  The two counts share counters[0]: candidates in the low kCandBits bits, tiles above.
// Dynamic LDS when tiles are planned, per template of the group: [npos] f32 score of every hit | [nw] hit bitmap |
// kMaxTilesPerTemplate x 4 words of tile records | the first kPlanHits hit positions; then 4 words per template + 4 for the
// group's scan.
__global__ void __launch_bounds__(1024)
k_coarse(FrameBatch fb, LevelGeom lv, int level, int levels,
         const TemplEntry* __restrict__ entries, const int32_t* __restrict__ feat_off,
         const int32_t* __restrict__ work_pyramids, int num_work, int wpt, int cpw, float threshold, uint32_t cap, TilePlanGeom plan) {
    extern __shared__ uint32_t s_dyn[];
    const FrameSlot& F = fb.f[blockIdx.y];                        // the frame of the batch this workgroup serves
    const uint8_t* __restrict__ lm_arena = F.lm_arena;
    Candidate* __restrict__ cands = F.cands;
    unsigned long long* __restrict__ counters = F.counters;
    TileRec* __restrict__ tiles = F.tiles;
    uint8_t* __restrict__ todo = F.todo;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform, and the compiler must know it: the
                                                                                         // template's entry and feature offsets then come through SMEM into SGPRs
    const int group = (int)(blockDim.x >> 6) / wpt;
    const int tslot = wave_in_block / wpt, wave = wave_in_block - tslot * wpt, nwaves = wpt;
    const int work_raw = blockIdx.x * group + tslot;
    const bool live = work_raw < num_work;
    const int work = live ? work_raw : num_work - 1;              // idle slots of the last workgroup shadow a real template and write nothing
    const int pyr = work_pyramids[work];
    const TemplEntry e = entries[(size_t)pyr * levels + level];
    const int nf = e.nf, nfp = e.nf_padded;
    const int32_t* fo = feat_off + e.feat_start;
    const int Wd = lv.Wd, Hd = lv.Hd, T = lv.T;
    const int npos = Wd * Hd;
    // LL.cpp:1299-1309
    const int wf = (e.width - 1) / T + 1, hf = (e.height - 1) / T + 1;
    const int tp = (Hd - hf) * Wd + (Wd - wf) + 1;
    const int offset = T / 2 + (T % 2 - 1);   // LL.cpp:1846
    const int nw = (npos + 31) >> 5;
    const int per_template = npos + nw + 4 * kMaxTilesPerTemplate + kPlanHits;
    uint32_t* s_mine = s_dyn + (size_t)tslot * per_template;
    float* s_score = reinterpret_cast<float*>(s_mine);
    volatile uint32_t* s_hit = s_mine + npos;
    volatile uint32_t* s_tile = s_mine + npos + nw;
    volatile uint32_t* s_list = s_tile + 4 * kMaxTilesPerTemplate;
    volatile uint32_t* s_agg = s_dyn + (size_t)group * per_template;       // [group][4]: hits, tiles, first slot, first tile; then the atomic's result
    if (plan.enabled) {
        for (int i = wave * 64 + lane; i < nw; i += wpt * 64) s_hit[i] = 0;
        __syncthreads();
    }

    // A wave owns cpw <= kChunksPerWave consecutive 16-position chunks, one per lane; lane cpw reads the chunk after them (the
    // realignment of a run needs the next lane's bytes) and the lanes above it sit the loads out.  Only the chunks below the
    // template's position count tp carry sums: those are split EVENLY over as few waves as hold them — a template with tp <= 1008
    // keeps one wave (of ceil(tp / 16) + 1 lanes) and its second wave only scans zeros, 1200 positions are 38 + 37 lanes, not
    // 63 + 12 — because a 16-byte wave load costs the texture path ~24 cycles at 40 lanes, 31.5 at 64 and still 22.7 at 12
    // (profiles/r03_tcp_rotation_microbench.txt).
    {
        const int nch = ((tp < npos ? tp : npos) + 15) >> 4;
        const int wn = (nch + kChunksPerWave - 1) / kChunksPerWave;
        cpw = wn >= 1 && wn <= nwaves ? (nch + wn - 1) / wn : kChunksPerWave;
        if (cpw < 1) cpw = 1;
    }
    for (int chunk0 = wave * cpw; chunk0 * 16 < npos; chunk0 += nwaves * cpw) {
        const int j0 = (chunk0 + lane) * 16;                   // first position owned by this lane
        uint32_t even[4] = {0, 0, 0, 0}, odd[4] = {0, 0, 0, 0};
        if (chunk0 * 16 < tp && nfp > 0 && lane <= cpw) {      // wave-uniform but for the idle lanes
            const BufRsrc arena = make_rsrc(lm_arena);
            uint32_t r8[4] = {0, 0, 0, 0};                      // packed-u8 sums of the current class run
            int cur = -1, cnt = 0;
            auto flush = [&](int cls) {                         // realign the run: bytes [cls, cls+16) of {own, next lane}
                uint32_t x[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[k] = r8[k]; x[4 + k] = (uint32_t)__shfl_down((int)r8[k], 1, 64); r8[k] = 0; }
                const int d = cls >> 2;
                const uint32_t sb = (uint32_t)(cls & 3);
                uint32_t o4[4];
                switch (d) {                                    // wave-uniform
                    case 0:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], sb);
                        break;
                    case 1:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 2], x[k + 1], sb);
                        break;
                    case 2:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 3], x[k + 2], sb);
                        break;
                    default:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 4], x[k + 3], sb);
                        break;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) add_bytes(o4[k], even[k], odd[k]);
            };
            int32_t o[kFeatBatch];
#pragma unroll
            for (int u = 0; u < kFeatBatch; ++u) o[u] = fo[u];                      // wave-uniform -> SMEM
            for (int f = 0; f < nfp; f += kFeatBatch) {
                const int fn = f + kFeatBatch < nfp ? f + kFeatBatch : f;             // prefetch next batch of offsets
                int32_t on[kFeatBatch];
#pragma unroll
                for (int u = 0; u < kFeatBatch; ++u) on[u] = fo[fn + u];
                uint4 v[kFeatBatch];
#pragma unroll
                for (int u = 0; u < kFeatBatch; ++u) v[u] = ld_buf16(arena, (uint32_t)j0, (uint32_t)(o[u] & ~15));
#pragma unroll
                for (int u = 0; u < kFeatBatch; ++u) {
                    const int cls = o[u] & 15;
                    if (cls != cur || cnt == 63) {
                        if (cur >= 0) flush(cur);
                        cur = cls; cnt = 0;
                    }
                    r8[0] += v[u].x; r8[1] += v[u].y; r8[2] += v[u].z; r8[3] += v[u].w;   // bytes never carry (<= 252)
                    ++cnt;
                }
#pragma unroll
                for (int u = 0; u < kFeatBatch; ++u) o[u] = on[u];
            }
            if (cur >= 0) flush(cur);
        }
        // Threshold scan (LL.cpp:1835-1852).
        auto raw_at = [&](int k) -> int {                        // the lane's k-th position sum (positions >= template_positions stay 0)
            const uint32_t pk = (k & 1) ? odd[k >> 2] : even[k >> 2];
            const int rawk = (int)((k & 2) ? (pk >> 16) : (pk & 0xFFFF));
            return j0 + k < tp ? rawk : 0;
        };
        uint32_t hit_mask = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (live && lane < cpw && j0 + k < npos && score_of(raw_at(k), nf) > threshold) hit_mask |= 1u << k;   // LL.cpp:1844
        if (plan.enabled) {
            // the hits of the whole template are collected in LDS; slots, tiles and records follow once all of them are known
            if (hit_mask) {
                atomicOr(const_cast<uint32_t*>(&s_hit[j0 >> 5]), hit_mask << (j0 & 31));
#pragma unroll
                for (int k = 0; k < 16; ++k) if (hit_mask & (1u << k)) s_score[j0 + k] = score_of(raw_at(k), nf);
            }
            continue;
        }
        // Without planning: one atomicAdd per WAVE reserves the slots of all its hits, then every lane writes its hits at the
        // reserved base + its exclusive prefix.
        int total;
        const int before = wave_excl_scan(__popc(hit_mask), lane, total);
        if (total > 0) {                                       // wave-uniform
            unsigned long long wbase = 0;
            if (lane == 0) wbase = atomicAdd(&counters[0], (unsigned long long)total);
            wbase = bcast_u64(wbase, 0);
            unsigned long long slot = wbase + (unsigned long long)before;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (hit_mask & (1u << k)) {
                    if (slot < cap) {
                        const int j = j0 + k;
                        const int cy = j / Wd, cx = j - cy * Wd;
                        Candidate c;
                        c.x = cx * T + offset; c.y = cy * T + offset; c.score = score_of(raw_at(k), nf); c.work = work;
                        cands[slot] = c;
                    }
                    ++slot;
                }
            }
        }
    }
    if (!plan.enabled) return;

    // ---- planning (the first wave of every template): hits whose level-0 windows lie kTileStep cells apart are grouped into
    // tiles of kTileNx x kTileNy coarse cells (one accumulation of the shared window region in k_local instead of one per
    // candidate); the rest are singles (todo = 1).  See "Tile refinement" below.  The first kPlanHits hits (raster order) sit
    // one per lane and the grouping is ballots over those lanes — no serial pass over the grid.
    __syncthreads();
    const bool planner = wave == 0 && live;
    uint32_t nhit = 0;
    if (planner) {
        for (int w = lane; w < nw; w += 64) nhit += (uint32_t)__popc(s_hit[w]);
        nhit = wave_sum_u32(nhit);
    }
    int ntile = 0, nplan = 0, p = 0;
    uint32_t my_rel = 0;                                                    // this lane's slot relative to the template's first; top bit: a single
    if (planner && nhit > 0) {
        // hit h (raster order) -> lane h for h < kPlanHits (through LDS)
        uint32_t before = 0;
        for (int w0 = 0; w0 < nw && before < (uint32_t)kPlanHits; w0 += 64) {
            uint32_t w = (w0 + lane < nw) ? s_hit[w0 + lane] : 0u;
            int total;
            uint32_t h = before + (uint32_t)wave_excl_scan(__popc(w), lane, total);
            while (w && h < (uint32_t)kPlanHits) {
                const int b = __ffs((int)w) - 1;
                w &= w - 1;
                s_list[h++] = (uint32_t)((w0 + lane) * 32 + b);
            }
            before += (uint32_t)total;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        nplan = nhit < (uint32_t)kPlanHits ? (int)nhit : kPlanHits;
        const TemplEntry e0 = entries[(size_t)pyr * levels];
        const int T0 = plan.T0, border = 8 * T0;
        const int max_x = plan.W0 - e0.width - border, max_y = plan.H0 - e0.height - border;
        auto fine_x0 = [&](int c) { return (c * T + offset) * 2 + 1; };   // LL.cpp:1868-1869 for the coarse cell's candidate
        int cx = -100, cy = -100;
        bool elig = false;
        if (lane < nplan) p = (int)s_list[lane];
        if (lane < nplan && plan.tiles) {
            cy = p / Wd; cx = p - cy * Wd;
            // a tile may serve the hit iff LL.cpp:1871-1880 does not clamp it and it is on the fast path of the refinement (all
            // windows inside their planes) — from the entry's feature bounding box, exactly like k_local's `all_in`
            const int x = fine_x0(cx), y = fine_x0(cy);
            if (e0.min_x >= 0 && e0.min_y >= 0 && e0.nf_padded > 0 && x >= border && x <= max_x && y >= border && y <= max_y) {
                const int gx = x / T0 - 8, gy = y / T0 - 8;
                elig = gx >= 0 && gy >= 0 && (e0.max_x + gx * T0) / T0 + 16 <= plan.Wd0 && (e0.max_y + gy * T0) / T0 + 16 <= plan.Hd0;
            }
        }
        uint32_t next = 0;                                                  // slots handed out so far
        bool member = false;
        while (plan.tiles && ntile < kMaxTilesPerTemplate && !(plan.dbg & 1)) {
            const unsigned long long eb = __ballot(elig);
            if (!eb) break;
            const int seed = __ffsll((long long)eb) - 1;                   // first eligible hit in raster order: top row of its block
            const int r = __shfl(cy, seed, 64), c = __shfl(cx, seed, 64);
            // the block of kTileNx x kTileNy cells holding the seed and the most eligible hits (how far it reaches to the left)
            int best_n = 0, best_c0 = c;
#pragma unroll
            for (int dc = 0; dc < kTileNx; ++dc) {
                const int c0 = c - dc < 0 ? 0 : c - dc;
                const int n = __popcll(__ballot(elig && (cy == r || cy == r + 1) && cx >= c0 && cx < c0 + kTileNx));
                if (n > best_n) { best_n = n; best_c0 = c0; }
            }
            if (best_n < 2) {                                               // alone in its neighbourhood: a single
                if (lane == seed) elig = false;
                continue;
            }
            const bool in = elig && (cy == r || cy == r + 1) && cx >= best_c0 && cx < best_c0 + kTileNx;
            int c0 = best_c0;
#pragma unroll
            for (int sft = 0; sft < kTileNx - 1; ++sft)                     // tight on the left: a lone column of members needs two strips, not three
                if (!__ballot(in && cx == c0)) ++c0;
            const int bit = in ? (cx - c0) + kTileNx * (cy - r) : 0;
            uint32_t mask = in ? 1u << bit : 0u;                              // (members only: kTileMaskBits bits)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mask |= (uint32_t)__shfl_xor((int)mask, o, 64);
            if (in) { my_rel = next + (uint32_t)__popc(mask & ((1u << bit) - 1u)); member = true; elig = false; }
            if (lane == seed) {
                s_tile[4 * ntile + 0] = (uint32_t)work;
                s_tile[4 * ntile + 1] = (uint32_t)(uint16_t)(int16_t)(fine_x0(c0) / T0 - 8) | ((uint32_t)(uint16_t)(int16_t)(fine_x0(r) / T0 - 8) << 16);
                s_tile[4 * ntile + 2] = next;
                // window origins of the block's columns / second row relative to the first, in level-0 cells: 2 T_top / T_0 apart on
                // average, e.g. always 4 for T = {4, 8} and 3, 3, 3, 3, 4, ... for the reference's default T = {5, 8} (LL.cpp:1868-1881)
                uint32_t steps = 0;
#pragma unroll
                for (int i = 1; i < kTileNx; ++i) steps |= (uint32_t)(fine_x0(c0 + i) / T0 - fine_x0(c0 + i - 1) / T0) << (3 * (i - 1));
                steps |= (uint32_t)(fine_x0(r + 1) / T0 - fine_x0(r) / T0) << (3 * (kTileNx - 1));
                s_tile[4 * ntile + 3] = mask | (steps << kTileMaskBits);
            }
            next += (uint32_t)best_n;
            ++ntile;
        }
        const bool single = lane < nplan && !member;
        const unsigned long long sb = __ballot(single);
        if (single) my_rel = (next + (uint32_t)__popcll(sb & ((1ull << lane) - 1ull))) | 0x80000000u;
    }
    // the workgroup's templates line up: exclusive scan of their hit / tile counts, one atomic on the packed counter
    if (wave == 0 && lane == 0) { s_agg[4 * tslot] = nhit; s_agg[4 * tslot + 1] = (uint32_t)ntile; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long hs = 0, ts = 0;
        for (int t = 0; t < group; ++t) {
            const uint32_t h = s_agg[4 * t], n = s_agg[4 * t + 1];
            s_agg[4 * t + 2] = (uint32_t)hs; s_agg[4 * t + 3] = (uint32_t)ts;
            hs += h; ts += n;
        }
        unsigned long long got = 0;
        if (hs && !(plan.dbg & 2)) got = atomicAdd(&counters[0], hs | (ts << kCandBits));
        s_agg[4 * group] = (uint32_t)got; s_agg[4 * group + 1] = (uint32_t)(got >> 32);
    }
    __syncthreads();
    if (!planner || nhit == 0) return;
    const unsigned long long packed = (unsigned long long)s_agg[4 * group] | ((unsigned long long)s_agg[4 * group + 1] << 32);
    const unsigned long long base = (packed & kCandMask) + s_agg[4 * tslot + 2];
    const unsigned long long tbase = (packed >> kCandBits) + s_agg[4 * tslot + 3];
    auto put = [&](unsigned long long slot, int pos, int flag) {            // candidate record of coarse position pos
        if (slot >= cap) return;
        const int py = pos / Wd, px = pos - py * Wd;
        Candidate c;
        c.x = px * T + offset; c.y = py * T + offset; c.score = s_score[pos]; c.work = work;
        cands[slot] = c;
        todo[slot] = (uint8_t)flag;
    };
    if (lane < nplan) put(base + (my_rel & 0x7FFFFFFFu), p, (int)(my_rel >> 31));
    if (nhit > (uint32_t)kPlanHits) {                                       // hits beyond the planned ones: singles, slot = first + h
        uint32_t before = 0;
        for (int w0 = 0; w0 < nw; w0 += 64) {
            uint32_t w = (w0 + lane < nw) ? s_hit[w0 + lane] : 0u;
            int total;
            uint32_t h = before + (uint32_t)wave_excl_scan(__popc(w), lane, total);
            while (w) {
                const int b = __ffs((int)w) - 1;
                w &= w - 1;
                if (h >= (uint32_t)kPlanHits) put(base + h, (w0 + lane) * 32 + b, 1);
                ++h;
            }
            before += (uint32_t)total;
        }
    }
    if (lane < ntile && tiles && tbase + lane < plan.tile_cap) {
        TileRec t;
        t.work = (int32_t)s_tile[4 * lane]; t.gxy = s_tile[4 * lane + 1];
        t.slot_base = (uint32_t)(base + s_tile[4 * lane + 2]); t.mask = s_tile[4 * lane + 3];
        tiles[tbase + lane] = t;
    }
}

// Tiles are planned for two-level pyramids whose neighbouring coarse cells have level-0 windows at most kTileStep cells apart
// (T_0 <= T_top <= 2 T_0: T = {4, 8}, {2, 4}, and the reference's default {5, 8}, where the step alternates between 3 and 4 cells)
// and whose coarse grid fits the planner's LDS; anything else keeps the plain per-wave candidate emission.
bool tile_plan_possible(const FrameGeom& g) {
    if (g.levels != 2) return false;
    const LevelGeom& top = g.lv[1];
    const LevelGeom& l0 = g.lv[0];
    if (2 * top.T > kTileStep * l0.T || top.T < l0.T) return false;      // 2 <= step <= kTileStep: 5 columns span <= 16 cells, a second row <= 4
    const size_t npos = (size_t)top.Wd * top.Hd;
    return npos >= 1 && coarse_plan_lds_bytes(top.Wd, top.Hd) <= 60 * 1024;   // at least one template per workgroup
}

size_t coarse_plan_lds_bytes(int Wd, int Hd) {                 // per template of a workgroup
    const size_t npos = (size_t)Wd * Hd, nw = (npos + 31) / 32;
    return (npos + nw + 4 * (size_t)kMaxTilesPerTemplate + kPlanHits) * sizeof(uint32_t);   // scores | hit bitmap | tile records | hit list
}

hipError_t launch_coarse(const FrameBatch& fb, const FrameGeom& g, const BankDev& bank, int num_work, float threshold, uint32_t cap, uint32_t tile_cap, hipStream_t s) {
    if (num_work <= 0 || fb.nb <= 0) return hipSuccess;
    const TileRec* tiles = fb.f[0].tiles;                      // tiles are planned for all frames of a batch or for none
    const uint8_t* todo = fb.f[0].todo;
    const int level = g.levels - 1;
    const LevelGeom lv = g.lv[level];
    int npos = lv.Wd * lv.Hd;
    const int nchunks = (npos + 15) / 16;
    int waves = (nchunks + kChunksPerWave - 1) / kChunksPerWave;
    if (waves > 16) waves = 16;
    if (waves < 1) waves = 1;
    const int cpw = std::min(kChunksPerWave, std::max(1, (nchunks + waves - 1) / waves));   // the map's chunks evenly over the waves
    TilePlanGeom plan{};
    size_t lds = 0;
    int group = 1;
    // Tiles are planned for k_local's tile path (tiles != null); with only `todo` given (the bit-plane refinement overwrites it) the hits are
    // still collected per workgroup — one reservation atomic instead of one per wave — but nothing is grouped: no tile half of counters[0].
    const bool plan_tiles = tiles && todo && tile_cap > 0 && tile_plan_possible(g);
    const bool group_only = !tiles && todo && npos >= 1 && coarse_plan_lds_bytes(lv.Wd, lv.Hd) <= 60 * 1024;
    if (plan_tiles || group_only) {
        plan.enabled = 1;
        plan.tiles = plan_tiles ? 1 : 0;
        plan.W0 = g.lv[0].W; plan.H0 = g.lv[0].H; plan.T0 = g.lv[0].T; plan.Wd0 = g.lv[0].Wd; plan.Hd0 = g.lv[0].Hd;
        plan.tile_cap = tile_cap;
        const int max_group = knobs().coarse_group;
#ifdef LM_DIAG
        plan.dbg = knobs().coarse_dbg;
#endif
        // Templates per workgroup: up to 4 (<= 16 waves, <= 64 KB of LDS).  More templates mean fewer atomics on the frame's counter,
        // but workgroups of 7-8 templates (14-16 waves) leave room for one workgroup per CU only: 16k templates at VGA 162 us with
        // 2-6 per workgroup, 300 us with 7-8; 2k templates 45 us with 2-8, 57 us with 1 (profiles/r02_coarse_group_sweep.txt).
        const size_t per = coarse_plan_lds_bytes(lv.Wd, lv.Hd);
        group = std::max(1, std::min(std::min(4, std::max(1, max_group)), std::min(16 / waves, (int)((64 * 1024 - 256) / per))));
        lds = per * group + (4 * (size_t)group + 4) * sizeof(uint32_t);
    }
    return lm_launch(k_coarse, dim3((num_work + group - 1) / group, fb.nb), dim3(group * waves * 64), lds, s, fb, lv, level, g.levels, bank.entries,
                     bank.feat_off, bank.work, num_work, waves, cpw, threshold, cap, plan);
}

// ---------------------------------------------------------------------------------------------
// Local refinement (LL.cpp:1855-1938, similarityLocal :1366-1428): one wave64 per candidate, marching
// up the pyramid; the grid is persistent and strides over the candidate list whose length is read
// from device memory (no host round trip between the coarse and the local pass).
//
// Fast path (every feature's 16x16 window inside its plane — always, except for oversized templates):
// gathers from the strip-major copy of the linear memories ([strip of 16 columns][row][16 B]).  A
// window spans two strips, so 32 lanes x one aligned 16-byte load cover it: lane (strip h, row r), rows fastest.
// The two half-waves work on two features of the same alignment class at a time; class runs are
// accumulated in packed u8 and realigned once per run: half-waves combined (lane ^ 32), strip pairs
// exchanged (lane ^ 16), v_alignbyte by the run's byte phase, widened into the u16 window
// accumulators (lane (r,h) keeps window columns 8h..8h+7 of row r).
// Slow path: flat layout, per-feature bounds test, exactly the reference's reads (wrap-around included).
// First strict maximum (LL.cpp:1920) = wave max-reduction of the packed key (raw << 8 | 255 - index).
// ---------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_local(FrameBatch fb, FrameGeom g, const TemplEntry* __restrict__ entries, const int32_t* __restrict__ feat_off,
        const uint32_t* __restrict__ feat_word, const uint32_t* __restrict__ run_mask, const uint32_t* __restrict__ feat_xy,
        const int32_t* __restrict__ work_pyramids, uint32_t cand_cap, float threshold, uint32_t cap,
        uint32_t dedupe_cap_slots, uint32_t tile_cap, int dbg) {
    // What bounds it (profiles/r02_pmc_tiles.txt, r02_local_experiments.txt): the vector L1.  Per CU 139k cycles of accesses +
    // 56k cycles stalled on pending misses of the 247k the kernel lasts (round 1: 345k + 37k of 363k) — every 128-byte line is
    // used by exactly one load instruction, so a third of the accesses miss.  Tried and measured WORSE: four waves sharing an
    // item through LDS (119 us: 104 VGPRs), 16 loads in flight per wave (123 us: 99 VGPRs) — occupancy matters more than the
    // length of a wave's chain of load batches —, tiles and singles on different workgroups (117 us: any alternation in the
    // workgroup index aliases with the round-robin over XCDs / shader engines) or on different waves of a workgroup (121 us).
    // Tiles alone take 72 us, singles alone 58 us, an empty launch of this grid 11 us (make DIAG=1, LM_LOCAL_DBG = 1 / 2 / 3).
    //
    // Work items of a BATCH of frames: the tiles of frame 0, 1, ... then the candidates of frame 0, 1, ...; s_tend / s_cend hold
    // the running ends, so a flat item index resolves to (frame, index) with at most nb comparisons (wave-uniform).
    __shared__ unsigned long long s_acc[kMaxBatch][2];            // per frame: 16x16 evaluations of this block, their algorithmic bytes
    __shared__ uint32_t s_tend[kMaxBatch + 1], s_cend[kMaxBatch + 1];
    const int lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));   // wave-uniform, and the
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);                                       // compiler must know it: item -> frame -> the frame's pointers stay in SGPRs
    const int nb = fb.nb;
    // Frame -> XCD affinity.  Workgroup b runs on XCD b % 8 (observed on gfx950, not a contract: only speed depends on it), each XCD has
    // its own 4 MB L2, and the strip planes of ONE frame are 4.9 MB at VGA.  With the items of a batch dealt to the waves in flat order
    // every L2 holds lines of all the batch's frames: L2 hit rate 94 % -> 76 %, fabric traffic per frame x4 (profiles/r03_pmc_batch_flat.txt).
    // So when the batch size divides 8, frame f is served by the workgroups of XCDs [f * 8 / nb, (f + 1) * 8 / nb) only.
    int f_lo = 0, f_hi = nb;
    uint32_t w_first = wave0, w_step = nwaves;
    if (nb > 1 && (8 % nb) == 0 && (gridDim.x & 7) == 0) {
        const int per = 8 / nb, xcd = (int)(blockIdx.x & 7);
        f_lo = xcd / per; f_hi = f_lo + 1;
        const uint32_t wpb = blockDim.x >> 6;
        w_first = ((blockIdx.x >> 3) * (uint32_t)per + (uint32_t)(xcd % per)) * wpb + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        w_step = (gridDim.x >> 3) * (uint32_t)per * wpb;
    }
    const bool tiled = fb.f[0].tiles != nullptr && !(dbg & 2);
    if (threadIdx.x == 0) {
        uint32_t te = 0, ce = 0;
        s_tend[0] = 0; s_cend[0] = 0;
        for (int f = 0; f < nb; ++f) {
            const unsigned long long packed = fb.f[f].counters[0];
            const unsigned long long nc = packed & kCandMask, nt = packed >> kCandBits;
            ce += nc < cand_cap ? (uint32_t)nc : cand_cap;
            te += !tiled ? 0u : (nt < tile_cap ? (uint32_t)nt : tile_cap);
            s_tend[f + 1] = te; s_cend[f + 1] = ce;
            s_acc[f][0] = 0; s_acc[f][1] = 0;
        }
    }
    __syncthreads();
    // the part of k_dedupe's hash table every frame will use, emptied here (k_dedupe runs next on the stream): no memset node
    for (int f = 0; f < nb; ++f) {
        unsigned long long* table = fb.f[f].dedupe_table;
        if (!table) continue;
        const uint32_t tsize = dedupe_slots_for(s_cend[f + 1] - s_cend[f], dedupe_cap_slots);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < tsize; i += gridDim.x * blockDim.x) table[i] = ~0ull;
    }

    // ---- Tile refinement: the candidates of one template whose coarse cells are neighbours have level-0 windows kTileStep
    // cells apart, so most of every feature's window is shared.  A tile (planned by k_coarse) covers up to kTileNx x kTileNy
    // such candidates: R = 16 + kTileStep * (rows of candidates - 1) rows x S strips of the strip-major planes, lane = (strip q,
    // row r), ONE aligned 16-byte load per lane and feature.  Class runs are summed in packed bytes and realigned once per run
    // like everywhere else ({own strip, next strip's lane r} shifted by the run's byte phase) into u16 sums of tile columns
    // [16 q, 16 q + 16); every member then takes the first strict maximum of its own 16 x 16 window of those sums — the same
    // integers, the same tie-break (packed key) and the same float expression as the per-candidate path below.
    if (tiled) {
        const uint32_t ntiles = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tend[f_hi]);
        const LevelGeom lv = g.lv[0];
        const int T = lv.T, Hd = lv.Hd, offset = T / 2 + (T % 2 - 1);
        int fr = f_lo;
        for (uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tend[f_lo]) + w_first; gi < ntiles; gi += w_step) {
            while (gi >= (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tend[fr + 1])) ++fr;           // wave-uniform: item -> frame
            const FrameSlot& F = fb.f[fr];
            const uint8_t* __restrict__ sm_arena = F.sm_arena;
            Candidate* __restrict__ matches_dev = F.matches_dev;
            const TileRec t = F.tiles[gi - (uint32_t)__builtin_amdgcn_readfirstlane((int)s_tend[fr])];
            const int work = __builtin_amdgcn_readfirstlane(t.work);
            const uint32_t gxy = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.gxy);
            const uint32_t mask_word = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.mask);
            const uint32_t mask = mask_word & ((1u << kTileMaskBits) - 1u), steps = mask_word >> kTileMaskBits;   // members | window steps (3 bits each)
            const int dy1 = (int)((steps >> (3 * (kTileNx - 1))) & 7u);        // window origin of the second row of members
            const uint32_t slot_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.slot_base);
            const int gx0 = (int16_t)(gxy & 0xFFFF), gy0 = (int16_t)(gxy >> 16);
            const int pyr = __builtin_amdgcn_readfirstlane(work_pyramids[work]);
            const TemplEntry e = entries[(size_t)pyr * g.levels];
            const int nf = e.nf, nfp = e.nf_padded;
            const uint32_t cols = (mask | (mask >> kTileNx)) & ((1u << kTileNx) - 1u);
            const int S = cols > 1u ? 3 : 2;                                   // a second column of candidates needs a third strip
            const int R = (mask >> kTileNx) ? 16 + dy1 : 16;
            int q = (lane >= R) + (lane >= 2 * R), r = lane - q * R;
            const bool active = lane < R * S;
            if (!active) { q = 0; r = 0; }                                     // idle lanes repeat lane 0's (valid) loads
            // Addressing (lm_kernels.h, feat_word): a feature's load = arena resource + lane VGPR + the feature's word (less its class
            // bits) as scalar offset.  The VGPR carries the lane's (strip, row) offset, the item's window origin K and the strip
            // carry of the run's class, rebuilt once per class run: ONE scalar instruction per feature.  (Every offset stays a
            // multiple of 16: folding the class bits into the VGPR as well made the loads return wrong data.)
            const BufRsrc strips = make_rsrc(sm_arena);
            const uint32_t lane_off = (uint32_t)(q * Hd + r) * 16u;
            const uint32_t K0 = (uint32_t)((gx0 >> 4) * Hd + gy0) * 16u, HS = (uint32_t)Hd * 16u;
            const int gxl = gx0 & 15;
            const int nb_lane = (lane + R < 64 ? lane + R : lane) << 2;       // the lane holding the next strip of this row
            uint32_t aE[4] = {0, 0, 0, 0}, aO[4] = {0, 0, 0, 0};              // u16x2 sums: aE[k] = cols 4k, 4k+2; aO[k] = cols 4k+1, 4k+3
            const uint32_t* fw = feat_word + e.feat_start;
            const uint32_t* rm = run_mask + (e.feat_start >> 3);
            uint32_t r8[4] = {0, 0, 0, 0};
            int cur = -1;
            auto flush = [&](int cls) {
                uint32_t x[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[k] = r8[k]; x[4 + k] = (uint32_t)__builtin_amdgcn_ds_bpermute(nb_lane, (int)r8[k]); r8[k] = 0; }
                const int c0 = (cls + gx0) & 15;                               // byte phase of the tile's first column in its strip
                const uint32_t sb = (uint32_t)(c0 & 3);
                uint32_t o4[4];
                switch (c0 >> 2) {                                             // wave-uniform
                    case 0:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], sb);
                        break;
                    case 1:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 2], x[k + 1], sb);
                        break;
                    case 2:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 3], x[k + 2], sb);
                        break;
                    default:
#pragma unroll
                        for (int k = 0; k < 4; ++k) o4[k] = __builtin_amdgcn_alignbyte(x[k + 4], x[k + 3], sb);
                        break;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) add_bytes(o4[k], aE[k], aO[k]);
            };
            if (nfp > 0) {
                uint32_t c[kFeatBatch], m = rm[0];
#pragma unroll
                for (int u = 0; u < kFeatBatch; ++u) c[u] = fw[u];                    // wave-uniform -> SMEM
                uint32_t vK = lane_off;                                                 // rebuilt at the first feature (always a run start)
                for (int f = 0; f < nfp; f += kFeatBatch) {
                    const int fn = f + kFeatBatch < nfp ? f + kFeatBatch : f;           // prefetch the next batch
                    uint32_t cn[kFeatBatch];
                    const uint32_t mn = rm[fn >> 3];
#pragma unroll
                    for (int u = 0; u < kFeatBatch; ++u) cn[u] = fw[fn + u];
                    uint4 v[kFeatBatch];
#pragma unroll
                    for (int u = 0; u < kFeatBatch; ++u) {
                        if (m & (1u << u)) {                                            // a class run starts: its lane offset
                            const int cls = (int)(c[u] & 15);
                            vK = lane_off + K0 + (cls + gxl >= 16 ? HS : 0u);
                        }
                        v[u] = ld_buf16(strips, vK, c[u] & ~15u);
                    }
#pragma unroll
                    for (int u = 0; u < kFeatBatch; ++u) {
                        if (m & (1u << u)) {
                            if (cur >= 0) flush(cur);
                            cur = (int)(c[u] & 15);
                        }
                        r8[0] += v[u].x; r8[1] += v[u].y; r8[2] += v[u].z; r8[3] += v[u].w;   // <= 62 x 4 per byte (host: runs of <= kRunMax)
                    }
#pragma unroll
                    for (int u = 0; u < kFeatBatch; ++u) c[u] = cn[u];
                    m = mn;
                }
                if (cur >= 0) flush(cur);
            }
            // members, in slot order
            uint32_t rest = mask;
            int member = 0;
            if (lane == 0) {
                const unsigned long long nmem = (unsigned long long)__popc(mask);
                atomicAdd(&s_acc[fr][0], nmem);
                atomicAdd(&s_acc[fr][1], nmem * 256ull * (unsigned long long)nf);          // algorithmic response bytes: 256 per feature and member
            }
            while (rest) {
                const int bit = __ffs((int)rest) - 1;
                rest &= rest - 1;
                const int j = bit / kTileNx, i = bit - j * kTileNx;
                int dx = 0;                                                     // window origin of the member's column (wave-uniform)
                for (int u = 0; u < i; ++u) dx += (int)((steps >> (3 * u)) & 7u);
                const int dy = j ? dy1 : 0;
                const int rr = r - dy;                                          // row of this lane inside the member's window
                uint32_t key = 0;
                if (active && q < 2 && rr >= 0 && rr < 16 && (dx & 3)) {        // a window that starts inside a 4-column group: column by column
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t raws4[4] = {aE[k] & 0xFFFF, aO[k] & 0xFFFF, aE[k] >> 16, aO[k] >> 16};
#pragma unroll
                        for (int tcol = 0; tcol < 4; ++tcol) {
                            const int col = 16 * q + 4 * k + tcol - dx;
                            if (col >= 0 && col < 16) {
                                const uint32_t kk = (raws4[tcol] << 8) | (255u - (uint32_t)(rr * 16 + col));
                                key = kk > key ? kk : key;
                            }
                        }
                    }
                } else if (active && q < 2 && rr >= 0 && rr < 16) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int col = 16 * q + 4 * k - dx;                    // window column of the lane's 4-column group k
                        if (col >= 0 && col < 16) {
                            const uint32_t idx = (uint32_t)(rr * 16 + col);
                            const uint32_t k0 = ((aE[k] & 0xFFFF) << 8) | (255u - idx), k1 = ((aO[k] & 0xFFFF) << 8) | (255u - (idx + 1));
                            const uint32_t k2 = ((aE[k] >> 16) << 8) | (255u - (idx + 2)), k3 = ((aO[k] >> 16) << 8) | (255u - (idx + 3));
                            const uint32_t ka = k0 > k1 ? k0 : k1, kb = k2 > k3 ? k2 : k3;
                            const uint32_t kk = ka > kb ? ka : kb;
                            key = kk > key ? kk : key;
                        }
                    }
                }
                const uint32_t k = wave_max_u32(key);
                const int raw = (int)(k >> 8);
                int br = -1, bc = -1;                                           // LL.cpp:1910-1911
                float best = 0.f;
                if (raw > 0) {
                    const int idx = 255 - (int)(k & 0xFF);
                    br = idx >> 4; bc = idx & 15;
                    best = score_of(raw, nf);
                }
                const uint32_t slot = slot_base + (uint32_t)member;
                ++member;
                if (lane == 0 && slot < cap) {
                    Candidate m;
                    m.x = (gx0 + dx + bc) * T + offset;                         // LL.cpp:1930-1931: x / T - 8 = the member's window origin
                    m.y = (gy0 + dy + br) * T + offset;
                    m.score = best;
                    m.work = best < threshold ? -1 : work;                      // LL.cpp:1935
                    matches_dev[slot] = m;
                }
            }
        }
    }

    const uint32_t num_cands = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cend[f_hi]);
    int fr = f_lo;
    for (uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cend[f_lo]) + w_first; gi < num_cands && !(dbg & 1); gi += w_step) {
        while (gi >= (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cend[fr + 1])) ++fr;               // wave-uniform: item -> frame
        const FrameSlot& F = fb.f[fr];
        const uint32_t ci = gi - (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cend[fr]);
        if (tiled && !F.todo[ci]) continue;                  // a tile member: refined above (wave-uniform)
        const uint8_t* __restrict__ lm_arena = F.lm_arena;
        const uint8_t* __restrict__ sm_arena = F.sm_arena;
        Candidate* __restrict__ matches_dev = F.matches_dev;
        const Candidate cd = F.cands[ci];
        unsigned long long evals = 0, bytes = 0;
        const int work = __builtin_amdgcn_readfirstlane(cd.work);
        const int pyr = __builtin_amdgcn_readfirstlane(work_pyramids[work]);
        int mx = __builtin_amdgcn_readfirstlane(cd.x), my = __builtin_amdgcn_readfirstlane(cd.y);
        float sim = cd.score;
        bool alive = true;

        for (int l = g.levels - 2; l >= 0 && alive; --l) {
            const LevelGeom lv = g.lv[l];
            const TemplEntry e = entries[(size_t)pyr * g.levels + l];
            const int T = lv.T, W = lv.W, H = lv.H, Wd = lv.Wd, Hd = lv.Hd;
            const int border = 8 * T, offset = T / 2 + (T % 2 - 1);
            const int max_x = W - e.width - border, max_y = H - e.height - border;
            int x = mx * 2 + 1, y = my * 2 + 1;               // LL.cpp:1871-1880
            x = x > border ? x : border;  y = y > border ? y : border;
            x = x < max_x ? x : max_x;    y = y < max_y ? y : max_y;
            const int gx = x / T - 8, gy = y / T - 8;          // C division (truncation), LL.cpp:1380-1381
            const int off_x = gx * T, off_y = gy * T;
            const int nf = e.nf, nfp = e.nf_padded;
            uint32_t key;                                        // lane-local best (raw << 8 | 255 - index)
            // Fast path iff every feature's 16x16 window lies inside its plane (no feature is discarded by
            // LL.cpp:1394, no row wrap, no spill into the next phase) — decided once per candidate from the
            // entry's feature bounding box; true unless the template is oversized for the frame.
            const bool all_in = e.min_x >= 0 && e.min_y >= 0 && gx >= 0 && gy >= 0 &&
                                ((e.max_x + off_x) / T + 16 <= Wd) && ((e.max_y + off_y) / T + 16 <= Hd);
            if (all_in) {
                // lane = (feature of the pair, strip h, row r) with the ROWS fastest: a quad of lanes reads 4 consecutive 16-byte rows of one strip
                // (one or two 64-byte lines) instead of 2 rows x 2 strips (profiles/r03_tcp_rotation_microbench.txt: 41 -> 36.6 cycles per wave load)
                const int half = lane >> 5, l5 = lane & 31, r = l5 & 15, h = l5 >> 4;
                const uint32_t HS = (uint32_t)Hd * 16u;
                const BufRsrc strips = make_rsrc(sm_arena);        // addressing as in the tile path: lane VGPR (rebuilt per class run) + feature word
                const uint32_t lane_off = h * HS + (uint32_t)r * 16u;
                const uint32_t K0 = (uint32_t)((gx >> 4) * Hd + gy) * 16u;
                const int gxl = gx & 15;
                uint32_t w[4] = {0, 0, 0, 0};                   // u16x2: cols (0,2) (1,3) (4,6) (5,7) of this lane's 8 columns
                if (nfp > 0) {
                    const uint32_t* fw = feat_word + e.feat_start;
                    const uint32_t* rm = run_mask + (e.feat_start >> 3);
                    uint32_t r8[4] = {0, 0, 0, 0};
                    int cur = -1;
                    auto flush = [&](int cls) {
                        uint32_t own[4], par[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            own[k] = r8[k] + (uint32_t)__shfl_xor((int)r8[k], 32, 64);   // both features of the pair
                            par[k] = (uint32_t)__shfl_xor((int)own[k], 16, 64);           // the other strip of this row
                            r8[k] = 0;
                        }
                        // bytes [c0 + 8h, +8) of the 32-byte row {strip S0, strip S0+1}; c0 = window start inside strip S0
                        const int c0 = (cls + gx) & 15;
                        uint32_t u6[6];
                        u6[0] = h ? par[2] : own[0]; u6[1] = h ? par[3] : own[1]; u6[2] = h ? own[0] : own[2];
                        u6[3] = h ? own[1] : own[3]; u6[4] = h ? own[2] : par[0]; u6[5] = h ? own[3] : par[1];
                        const uint32_t sb = (uint32_t)(c0 & 3);
                        uint32_t o0, o1;
                        switch (c0 >> 2) {                       // wave-uniform
                            case 0: o0 = __builtin_amdgcn_alignbyte(u6[1], u6[0], sb); o1 = __builtin_amdgcn_alignbyte(u6[2], u6[1], sb); break;
                            case 1: o0 = __builtin_amdgcn_alignbyte(u6[2], u6[1], sb); o1 = __builtin_amdgcn_alignbyte(u6[3], u6[2], sb); break;
                            case 2: o0 = __builtin_amdgcn_alignbyte(u6[3], u6[2], sb); o1 = __builtin_amdgcn_alignbyte(u6[4], u6[3], sb); break;
                            default: o0 = __builtin_amdgcn_alignbyte(u6[4], u6[3], sb); o1 = __builtin_amdgcn_alignbyte(u6[5], u6[4], sb); break;
                        }
                        add_bytes(o0, w[0], w[1]);
                        add_bytes(o1, w[2], w[3]);
                    };
                    uint32_t c[kFeatBatch], m = rm[0];
#pragma unroll
                    for (int u = 0; u < kFeatBatch; ++u) c[u] = fw[u];                    // wave-uniform -> SMEM
                    uint32_t vK = lane_off;
                    for (int f = 0; f < nfp; f += kFeatBatch) {
                        const int fn = f + kFeatBatch < nfp ? f + kFeatBatch : f;           // prefetch the next batch
                        uint32_t cn[kFeatBatch];
                        const uint32_t mn = rm[fn >> 3];
#pragma unroll
                        for (int u = 0; u < kFeatBatch; ++u) cn[u] = fw[fn + u];
                        uint4 v[kFeatBatch / 2];
#pragma unroll
                        for (int k = 0; k < kFeatBatch / 2; ++k) {
                            // features 2k (lanes 0-31) and 2k+1 (lanes 32-63): one class run by construction (runs start at even indices)
                            if (m & (1u << (2 * k))) {
                                const int cls = (int)(c[2 * k] & 15);
                                vK = lane_off + K0 + (cls + gxl >= 16 ? HS : 0u);
                            }
                            v[k] = ld_buf16(strips, vK + ((half ? c[2 * k + 1] : c[2 * k]) & ~15u), 0u);   // (a lane offset that wraps below zero against the scalar offset reads zeros)
                        }
#pragma unroll
                        for (int k = 0; k < kFeatBatch / 2; ++k) {
                            if (m & (1u << (2 * k))) {
                                if (cur >= 0) flush(cur);
                                cur = (int)(c[2 * k] & 15);
                            }
                            r8[0] += v[k].x; r8[1] += v[k].y; r8[2] += v[k].z; r8[3] += v[k].w;   // <= 31 x 4 per byte and half (host: runs of <= kRunMax)
                        }
#pragma unroll
                        for (int u = 0; u < kFeatBatch; ++u) c[u] = cn[u];
                        m = mn;
                    }
                    if (cur >= 0) flush(cur);
                }
                const uint32_t idx0 = (uint32_t)(r * 16 + 8 * h);
                const uint32_t raws[8] = {w[0] & 0xFFFF, w[1] & 0xFFFF, w[0] >> 16, w[1] >> 16,
                                          w[2] & 0xFFFF, w[3] & 0xFFFF, w[2] >> 16, w[3] >> 16};
                key = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    uint32_t kk = (raws[k] << 8) | (255u - (idx0 + k));
                    key = kk > key ? kk : key;
                }
            } else {
                const int row = lane >> 2, col = (lane & 3) * 4;
                const int32_t* fo = feat_off + e.feat_start;
                const uint32_t* fxy = feat_xy + e.feat_start;
                const uint8_t* base = lm_arena + ((int64_t)gy * Wd + gx + row * Wd + col);
                uint32_t even = 0, odd = 0;
                for (int f = 0; f < nfp; ++f) {
                    uint32_t xy = fxy[f];
                    int fx = (int16_t)(xy & 0xFFFF) + off_x, fy = (int16_t)(xy >> 16) + off_y;
                    if (fx < 0 || fy < 0 || fx >= W || fy >= H) continue;   // LL.cpp:1394 (padding: x = y = -32768)
                    uint32_t v = ld_u32(base + fo[f]);
                    add_bytes(v, even, odd);
                }
                const uint32_t idx0 = (uint32_t)(row * 16 + col);
                uint32_t k0 = ((even & 0xFFFF) << 8) | (255u - idx0);
                uint32_t k1 = ((odd & 0xFFFF) << 8) | (255u - (idx0 + 1));
                uint32_t k2 = ((even >> 16) << 8) | (255u - (idx0 + 2));
                uint32_t k3 = ((odd >> 16) << 8) | (255u - (idx0 + 3));
                uint32_t ka = k0 > k1 ? k0 : k1, kb = k2 > k3 ? k2 : k3;
                key = ka > kb ? ka : kb;
            }
            ++evals;
            bytes += 256ull * nf;   // algorithmic response bytes of this 16x16 evaluation
            const uint32_t k = wave_max_u32(key);
            const int raw = (int)(k >> 8);
            int br = -1, bc = -1;                               // LL.cpp:1910-1911
            float best = 0.f;
            if (raw > 0) {
                int idx = 255 - (int)(k & 0xFF);
                br = idx >> 4; bc = idx & 15;
                best = score_of(raw, nf);
            }
            sim = best;
            mx = (x / T - 8 + bc) * T + offset;                 // LL.cpp:1930-1931
            my = (y / T - 8 + br) * T + offset;
            if (sim < threshold) alive = false;                 // remove_if(MatchPredicate), LL.cpp:1935
        }
        // No atomics: the result of candidate ci goes to slot ci (work = -1 when it dropped below the
        // threshold on the way up, LL.cpp:1935).
        if (lane == 0 && ci < cap) {
            Candidate m;
            m.x = mx; m.y = my; m.score = sim; m.work = alive ? work : -1;
            matches_dev[ci] = m;                 // in HBM: k_dedupe, the on-device NMS / top-K (pipeline.cpp) and the exchange read it there; the host
                                                 // fetches the raw records only when asked for them (lm_collect_frame, sort_unique = 0)
        }
        if (lane == 0) { atomicAdd(&s_acc[fr][0], evals); atomicAdd(&s_acc[fr][1], bytes); }
    }
    // statistics (16x16 evaluations, their algorithmic bytes) per frame: summed per block in LDS, then one pair of atomics per
    // block and frame it worked on into the frame's sharded counters (k_dedupe's last block publishes the totals)
    __syncthreads();
    if ((int)threadIdx.x < nb && s_acc[threadIdx.x][0] != 0) {
        unsigned long long* st = fb.f[threadIdx.x].counters + 8 + 2 * (blockIdx.x & (kStatShards - 1));
        atomicAdd(st, s_acc[threadIdx.x][0]);
        atomicAdd(st + 1, s_acc[threadIdx.x][1]);
    }
}

hipError_t launch_local(const FrameBatch& fb, const FrameGeom& g, const BankDev& bank, uint32_t cand_cap, float threshold, uint32_t cap, uint32_t dedupe_cap_slots, uint32_t tile_cap, int grid_blocks, hipStream_t s) {
    if (grid_blocks <= 0 || fb.nb <= 0) return hipSuccess;
    int dbg = 0;
#ifdef LM_DIAG
    dbg = knobs().local_dbg;                                    // timing experiments (wrong results): 1 = tiles only, 2 = singles only
#endif
    return lm_launch(k_local, dim3(grid_blocks), dim3(256), 0, s, fb, g, bank.entries, bank.feat_off, bank.feat_word, bank.run_mask, bank.feat_xy, bank.work, cand_cap,
                     threshold, cap, dedupe_cap_slots, tile_cap, dbg);
}

}  // namespace lm
