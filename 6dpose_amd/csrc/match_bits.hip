// Similarity kernels of Detector::matchClass on gfx950, on bit planes (the default): k_pack_bits /
// k_local_bits (strip records of the levels below the top, reference similarityLocal LL.cpp:1366-1428, 1855-1938), k_pack_top / k_coarse_bits /
// k_coarse_bits_batch (pair stream of the top level, LL.cpp:1284-1354, 1835-1852), their launchers and the dispatcher that picks the
// instantiation.  A kernel here holds what is particular to it — its load scheme, its counters, how it reserves candidate slots —; the stages
// it shares with match_wide.hip's kernels (template head, hit test and emission of the coarse pass; window, arg-max, update and epilogue of
// the refinement; the packers' indexing) are in match_planes.h, the bit-sliced adders in match_device.h.  The byte kernels are in
// match_bytes.hip; data layout and bank: match_bytes.hip.
#include "launch.h"
#include "match_planes.h"
#include <algorithm>
#include <type_traits>

namespace lm {

// ---- Bit planes: the default encoding of the response memories for both matching kernels --------------------------
// A response is 0, 1 or 4, so a position's sum is n1 + 4 n4 with n1 / n4 = the number of features whose response there is 1 / 4: two bits
// per cell carry what the byte planes do, and the sums can be kept BIT-SLICED (one dword = 32 positions of one counter bit), features
// entering through carry-save adders; integers are formed once per candidate / only for the hits.
//
// Levels below the top ("strip records", read by k_local_bits): the strip arena at half the offsets — per plane row and 16-column strip s an
// 8-byte record holding cells [16 s, 16 s + 32) of that row with TWO BITS PER CELL, bit 2c = "the response of cell 16 s + c is 1", bit
// 2c + 1 = "it is 4".  Strips are 32 cells wide at a stride of 16, so any 16-cell window of a row lies inside ONE record and comes out of it
// with ONE funnel shift, v_alignbit(hi, lo, 2 (column & 15)): a dword of 16 positions x {is-1, is-4}.  (Round 3 kept the two planes in
// separate dwords: 4 shifts + 2 ands + 2 or per lane and feature to cut the windows out, and every lane redid the address arithmetic of
// every feature — 30 VALU instructions per lane and feature at 0.92 of the issue slots)
// The top level ("pair stream", read by k_coarse_bits): the flat linear memories [label][phase][position] as one pair {is-1 dword, is-4
// dword} per 32 consecutive arena bytes, so the reference's reads that run from one plane into the next stay what they are.
// (the carry-save adders, the Harley-Seal counters and weighted_sum: match_device.h — match_wide.hip counts three planes with them)
// 4 response bytes -> 8 bits, cell k at bits 2k (is 1 = bit 0 of the byte) and 2k + 1 (is 4 = bit 2 of the byte); the multiply gathers the
// four 2-bit fields into the top byte (partial products land on distinct bits: no carries)
// (any table of two planes: the bytes are 0, a or 4 with a = 1, 2 or 3 — "is a" = bit 0 or bit 1 of the byte)
static __device__ __forceinline__ uint32_t pack4(uint32_t d) {
    const uint32_t t = ((d | (d >> 1)) & 0x01010101u) | ((d >> 1) & 0x02020202u);
    return (t * 0x01041040u) >> 24;
}
static __device__ __forceinline__ uint32_t pack16(const uint4& v) { return pack4(v.x) | (pack4(v.y) << 8) | (pack4(v.z) << 16) | (pack4(v.w) << 24); }

// Strip records from the strip bytes (the front end writes the records itself when nothing reads the bytes: fe_bits.hip, bits_rows_body;
// this kernel serves the banks and geometries that keep the byte planes — a fallback launch of k_local may follow — and the tests of both).
__global__ void __launch_bounds__(256)
k_pack_bits(BitsBatch B, uint32_t sm_off0, uint32_t records, int NS, int Hd) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= records) return;
    uint4 a, b;
    const size_t at = strip_cells(B.strips[blockIdx.y], sm_off0, i, NS, Hd, a, b);
    uint2 r;
    r.x = pack16(a);
    r.y = pack16(b);
    *reinterpret_cast<uint2*>(B.bits[blockIdx.y] + at) = r;
}

// Refinement on strip records (LL.cpp:1855-1938, similarityLocal :1366-1428).  8 lanes per candidate — lane j owns window rows 2j and 2j + 1,
// ONE 16-byte load = their two records —, 8 candidates per wave, one feature per candidate and load instruction: a wave load serves 8
// (candidate, feature) pairs.  Per 16 features a lane fetches two feature words and forms, ONCE for its group, their record offsets (window
// origin, strip carry) and shift amounts; the group's lanes pick them up with two ds_bpermute per feature and add only their own row term.
// Per lane and feature: 1 add, 2 v_alignbit, 5 adder operations (two dwords x 2.5).  Counters of kN = 4 + kHi bits: kHi = 5 serves entries
// of up to 511 features, kHi = 10 up to 16383 (the reference allows 8191 per modality, LL.cpp:1291, 1816).
// What bounds it (round 5, profiles/r05_local_sharing/README.txt): the number of wave loads — one takes 20-23 CU cycles whatever the lanes or addresses —, and
// what keeps its L2 traffic down is that the 8 candidates of a wave are CONSECUTIVE candidates of one template (x-neighbours: ~5 distinct lines per wave load
// instead of 23).  Three schemes that share loads between neighbouring candidates by regrouping them (vertical runs, interleaved pairs, same-lane pairs) were
// built, bit-exact, and ran no faster: fewer wave loads, more L2 requests.  Hence: candidates in slot order, a grid of the resident workgroups.
// All pyramid levels below the top are walked here (LL.cpp:1855: level by level, dropping a candidate as soon as it falls below the
// threshold); a candidate whose windows leave their planes at some level (oversized template, features outside the frame) is marked in
// `todo` and left, from the top, to k_local's per-candidate path.
template <int kHi, int kWaves, int kA>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_local_bits(FrameBatch fb, BitsBatch B, FrameGeom g, const TemplEntry* __restrict__ entries, const uint32_t* __restrict__ feat_word,
             const int32_t* __restrict__ work_pyramids, uint32_t cand_cap, float threshold, uint32_t cap, uint32_t dedupe_cap_slots) {
    constexpr int kN = 4 + kHi;                                     // counter bits per plane
    constexpr int kS = kN + 3;                                      // bits of n1 + 4 n4
    __shared__ unsigned long long s_acc[kMaxBatch][2];
    __shared__ uint32_t s_cnt[kMaxBatch];
    const int lane = threadIdx.x & 63, grp = lane >> 3, j = lane & 7;
    const int nb = fb.nb;
    const LocalShare share = local_share(nb);
    local_prologue(fb, s_cnt, s_acc, cand_cap, dedupe_cap_slots);
    // The pair stream k_coarse_bits has just read is zeroed for the slot's next frame: the front end ORs it together (fe_bits.hip, top_bits_body)
    if (B.top_clear_units)
        for (int f = 0; f < nb; ++f)
            for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < B.top_clear_units; i += gridDim.x * blockDim.x)
                reinterpret_cast<uint4*>(B.top_clear[f])[i] = make_uint4(0u, 0u, 0u, 0u);
    const int src0 = (lane & ~7) << 2;                              // ds_bpermute address of the group's first lane
    const uint32_t rowoff = 16u * (uint32_t)j;                      // records of rows 2j, 2j + 1 behind the window's first row
    for (int fr = share.f_lo; fr < share.f_hi; ++fr) {
        const FrameSlot& F = fb.f[fr];
        const BufRsrc bits = make_rsrc(B.bits[fr]);
        const uint32_t nc = s_cnt[fr], ngroups = (nc + 7u) >> 3;
        for (uint32_t gi = share.w_first; gi < ngroups; gi += share.w_step) {
            const uint32_t ci = gi * 8u + (uint32_t)grp;
            const bool valid = ci < nc;
            Candidate cd{0, 0, 0.f, 0};
            if (valid) cd = F.cands[ci];
            const int work = cd.work;
            const int pyr = work_pyramids[work];
            int mx = cd.x, my = cd.y;
            float sim = cd.score;
            bool alive = valid, leave = false;                      // leave: k_local's per-candidate path takes this candidate (from the top)
            uint32_t evals = 0, bytes = 0;
            for (int l = g.levels - 2; l >= 0; --l) {
                const LevelGeom& lv = g.lv[l];
                const TemplEntry e = entries[(size_t)pyr * g.levels + l];
                const LocalWindow win = local_window(lv, e, mx, my, alive, leave);
                const int nfp = win.nfp, nmax = win.nmax;
                const uint32_t* fw = feat_word + e.feat_start;
                uint32_t cA[kN], cB[kN];                            // bit-sliced counters of rows 2j / 2j + 1: even bits count the 1s, odd bits the 4s
#pragma unroll
                for (int k = 0; k < kN; ++k) { cA[k] = 0; cB[k] = 0; }
                uint32_t offx = 0, offy = 0, sx = 0, sy = 0;
                auto batch = [&](int half, uint32_t& eA, uint32_t& eB) {           // features 8 half .. 8 half + 7 of the current 16
                    uint4 v[8];
                    uint32_t sh[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int src = src0 + 4 * (4 * half + (u >> 1));          // the lane that fetched feature 8 half + u
                        const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)((u & 1) ? offy : offx));
                        sh[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)((u & 1) ? sy : sx));
                        v[u] = ld_buf16(bits, o + rowoff, 0u);      // rows 2j, 2j + 1: 32 cells x 2 bits each
                    }
                    uint32_t xa[8], xb[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        xa[u] = __builtin_amdgcn_alignbit(v[u].y, v[u].x, sh[u]);      // 16 window cells of row 2j: bits 2c (is 1), 2c + 1 (is 4)
                        xb[u] = __builtin_amdgcn_alignbit(v[u].w, v[u].z, sh[u]);      // ... of row 2j + 1
                    }
                    eA = add8(xa, cA[0], cA[1], cA[2]);
                    eB = add8(xb, cB[0], cB[1], cB[2]);
                };
                uint2 wn = local_fetch(fw, 0, j, nfp);
                for (int f0 = 0; f0 < nmax; f0 += 16) {
                    const uint2 wd = wn;
                    const bool on = f0 + 2 * j < nfp;
                    wn = local_fetch(fw, f0 + 16, j, nfp);          // the next 16 words while these are worked on
                    local_prep(wd.x, on, win.gxl, win.Kbase, win.HS8, win.zero_off, offx, sx);
                    local_prep(wd.y, on, win.gxl, win.Kbase, win.HS8, win.zero_off, offy, sy);
                    uint32_t e1A, e1B;
                    batch(0, e1A, e1B);
                    if (f0 + 8 < nmax) {                            // wave-uniform
                        uint32_t e2A, e2B;
                        batch(1, e2A, e2B);
                        add_eights2<kN>(cA, e1A, e2A);
                        add_eights2<kN>(cB, e1B, e2B);
                    } else {
                        add_eights1<kN>(cA, e1A);
                        add_eights1<kN>(cB, e1B);
                    }
                }
                // Once per candidate and level: the two rows of the lane side by side, S = n1 + 4 n4 bit-sliced, its maximum and where
                uint32_t S[kS];
                {
                    uint32_t n1[kN], n4[kN];
                    local_interleave<kN>(n1, n4, cA, cB);
                    weighted_sum<kA, kN>(S, n1, n4);
                }
                int raw, br, bc;
                local_argmax<kS>(S, j, raw, br, bc);
                local_update(win, lv.T, raw, br, bc, threshold, sim, mx, my, alive, evals, bytes);
            }
            if (valid && j == 0) local_store(F, ci, leave, cap, mx, my, sim, alive, work, s_acc[fr], evals, bytes);
        }
    }
    local_flush_stats(fb, s_acc);
}

hipError_t launch_pack_bits(const BitsBatch& B, int nb, const LevelGeom& lv, hipStream_t s) {
    const uint32_t records = (uint32_t)(2 * 8 * lv.T * lv.T) * (uint32_t)lv.NS * (uint32_t)lv.Hd;
    if (records == 0 || nb <= 0) return hipSuccess;   // an empty level / batch: nothing to pack
    return lm_launch(k_pack_bits, dim3((records + 255) / 256, nb), dim3(256), 0, s, B, lv.sm_off[0], records, lv.NS, lv.Hd);
}
hipError_t launch_local_bits(const FrameBatch& fb, const BitsBatch& B, const FrameGeom& g, const BankDev& bank, uint32_t cand_cap, float threshold,
                       uint32_t cap, uint32_t dedupe_cap_slots, int grid_blocks, int max_features, int low_weight, hipStream_t s) {
    return with_bits_instance<4, 4>(max_features, low_weight, [&](auto hi, auto waves, auto a) {
        return lm_launch(k_local_bits<hi(), waves(), a()>, dim3(grid_blocks), dim3(256), 0, s, fb, B, g, bank.entries, bank.feat_word, bank.work, cand_cap, threshold, cap,
                         dedupe_cap_slots);
    });
}

// ---- Coarse pass on the pair stream (LL.cpp:1284-1354 similarity + :1835-1852 scan).  A wave per template, a lane = 32 consecutive
// positions of the template's map: a feature's load = two consecutive pairs per lane (16 bytes) at pair index (offset >> 5) + lane,
// funnel-shifted by offset & 31 — the offset is wave-uniform, so both are scalar —, i.e. ONE wave load per feature and 2048 positions
// (the byte kernel: one per 1008 positions and 16 bytes per position and lane).  Sums bit-sliced as in k_local_bits; template head, hit
// test, slot reservation (one atomic per workgroup of 4 templates and pass) and emission: match_planes.h.  No tiles: the bit-plane
// refinement needs none.
__global__ void __launch_bounds__(256)
k_pack_top(TopBits B, uint32_t byte0, uint32_t npairs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npairs) return;
    const uint8_t* src = B.lm[blockIdx.y] + byte0 + (size_t)i * 32;
    const uint4 a = *reinterpret_cast<const uint4*>(src), b = *reinterpret_cast<const uint4*>(src + 16);
    // the low plane's response a = 1, 2 or 3: bit 0 or bit 1 of the byte; response 4 = bit 2
    *reinterpret_cast<uint2*>(B.bits[blockIdx.y] + (size_t)i * 8) = make_uint2(byte_bits32(a, b, 0) | byte_bits32(a, b, 1), byte_bits32(a, b, 2));
}

template <int kHi, int kWaves, int kA>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_coarse_bits(FrameBatch fb, TopBits B, LevelGeom lv, int level, int levels, const TemplEntry* __restrict__ entries, const int32_t* __restrict__ feat_off,
              const int32_t* __restrict__ work_pyramids, int num_work, float threshold, uint32_t cap, uint32_t byte0) {
    constexpr int kN = 4 + kHi, kS = kN + 3;
    __shared__ uint32_t s_tot[4];
    __shared__ unsigned long long s_base;
    const FrameSlot& F = fb.f[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const CoarseHead h = coarse_head((int)blockIdx.x * 4 + wave, num_work, entries, feat_off, work_pyramids, lv, level, levels, threshold);   // a wave per template
    const bool live = h.live;
    const int nfp = h.nfp, npos = h.npos, limit = h.limit;
    const int32_t* fo = h.fo;
    const BufRsrc bits = make_rsrc(B.bits[blockIdx.y]);
    for (int P0 = 0; P0 < npos; P0 += 2048) {                               // (the same number of passes for every wave of the workgroup)
        const int pos0 = P0 + 32 * lane;                                    // first position of this lane
        uint32_t c1[kN], c4[kN];
#pragma unroll
        for (int k = 0; k < kN; ++k) { c1[k] = 0; c4[k] = 0; }
        if (live && P0 < limit && nfp > 0 && pos0 < limit) {                // (lanes beyond the map sit the loads out)
            auto batch = [&](int f, uint32_t& e1, uint32_t& e4) {
                uint4 v[8];
                uint32_t sh[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t ob = (uint32_t)fo[f + u] - byte0 + (uint32_t)P0;      // wave-uniform -> SMEM / SALU
                    sh[u] = ob & 31u;
                    v[u] = ld_buf16(bits, (uint32_t)lane * 8u, (ob >> 5) * 8u);          // pairs q + lane and q + lane + 1
                }
                uint32_t x1[8], x4[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    x1[u] = __builtin_amdgcn_alignbit(v[u].z, v[u].x, sh[u]);            // bits [s, s + 32) of {is-1 of pair q + lane + 1 : pair q + lane}
                    x4[u] = __builtin_amdgcn_alignbit(v[u].w, v[u].y, sh[u]);
                }
                e1 = add8(x1, c1[0], c1[1], c1[2]);
                e4 = add8(x4, c4[0], c4[1], c4[2]);
            };
            for (int f = 0; f < nfp; f += 16) {
                uint32_t a1, a4;
                batch(f, a1, a4);
                if (f + 8 < nfp) {
                    uint32_t b1, b4;
                    batch(f + 8, b1, b4);
                    add_eights2<kN>(c1, a1, b1);
                    add_eights2<kN>(c4, a4, b4);
                } else {
                    add_eights1<kN>(c1, a1);
                    add_eights1<kN>(c4, a4);
                }
            }
        }
        uint32_t S[kS];
        weighted_sum<kA, kN>(S, c1, c4);
        uint32_t summed;
        uint32_t hit_mask = coarse_hit_mask<kS>(S, h.rmin, h.zero_passes, limit, npos, pos0, summed);
        if (!live) hit_mask = 0;
        int total;
        const unsigned long long slot = coarse_reserve_slots(s_tot, s_base, F.counters, hit_mask, lane, wave, total);
        if (total > 0)                                                      // wave-uniform
            coarse_emit<kS>(hit_mask, summed, S, slot, cap, pos0, h.Wd, h.T, h.offset, h.nf, h.work, F.cands);
    }
}

// ---- The coarse pass of a BATCH with the frames sharing a template's waves.  k_coarse_bits is bound by its wave loads and
// a wave load costs the same whatever the live lanes: at VGA a frame's 1200 positions are 38 lanes, the other 26 sit every load out.  A feature's
// offset is the same for every frame, so here the lanes of a (template, frame group) are ONE flat index g = frame * L + lane of the frame,
// L = ceil(positions / 32), dealt to consecutive waves: a wave may straddle frames, idle lanes exist only behind a group's last frame, and a frame
// of more than 64 lanes spans waves (no pass loop).  Only the base of a lane's loads differs — its frame's pair stream, a 64-bit address per lane:
// the slots' streams are separate allocations —; offsets and shifts stay scalar, head, hit test and emission are the shared stages of match_planes.h.
// A workgroup = kWg waves per template x the templates that fit, on the frames [f0, f0 + fpg) of the batch (a group = as many frames as 16 waves
// hold); it reserves the slots of each of its frames with ONE atomic, and inside them a template's hits lie together in raster order (the wave
// scan, cut at the frame boundaries; the waves' counts per frame prefix-summed in LDS), which k_local_bits's L2 locality rests on.
constexpr int kCoarseBatchWaves = 16;                                       // waves per workgroup at most: 1024 lanes hold a group's frames
typedef uint32_t pair2_t __attribute__((ext_vector_type(4), aligned(8)));   // two consecutive pairs: a stream's pairs are 8-byte aligned
template <int kHi, int kWaves, int kA>
__global__ void __launch_bounds__(64 * kCoarseBatchWaves) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_coarse_bits_batch(FrameBatch fb, TopBits B, LevelGeom lv, int level, int levels, const TemplEntry* __restrict__ entries, const int32_t* __restrict__ feat_off,
                    const int32_t* __restrict__ work_pyramids, int num_work, float threshold, uint32_t cap, uint32_t byte0, int L, int fpg, int Wg) {
    constexpr int kN = 4 + kHi, kS = kN + 3;
    __shared__ uint32_t s_cnt[kCoarseBatchWaves][kMaxBatch];               // hits of (wave, frame of the group), then their exclusive prefix over the waves
    __shared__ unsigned long long s_base[kMaxBatch];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = (int)(blockDim.x >> 6);
    const int tl = wv / Wg, ww = wv - tl * Wg;                              // template of the workgroup, wave of the template
    const CoarseHead h = coarse_head((int)blockIdx.x * (nwaves / Wg) + tl, num_work, entries, feat_off, work_pyramids, lv, level, levels, threshold);
    const bool live = h.live;
    const int nfp = h.nfp, limit = h.limit;
    const int32_t* fo = h.fo;
    const int f0 = (int)blockIdx.y * fpg;                                   // the group's frames
    const int nfr = fb.nb - f0 < fpg ? fb.nb - f0 : fpg;
    const int g = ww * 64 + lane;                                           // flat lane of the (template, group)
    const int fl = g / L, li = g - fl * L;                                  // frame of the group, lane of the frame
    const bool act = live && fl < nfr;                                      // (behind the group's last frame: idle)
    const int frame = f0 + (fl < nfr ? fl : 0);
    const int pos0 = 32 * li;                                               // first position of this lane
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kCoarseBatchWaves * kMaxBatch); i += blockDim.x) (&s_cnt[0][0])[i] = 0u;
    uint32_t c1[kN], c4[kN];
#pragma unroll
    for (int k = 0; k < kN; ++k) { c1[k] = 0; c4[k] = 0; }
    if (act && nfp > 0 && pos0 < limit) {                                   // (lanes beyond the sums sit the loads out)
        const uint8_t* base = B.bits[frame] + (size_t)li * 8u;
        auto batch = [&](int f, uint32_t& e1, uint32_t& e4) {
            pair2_t v[8];
            uint32_t sh[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t ob = (uint32_t)fo[f + u] - byte0;            // wave-uniform -> SMEM / SALU
                sh[u] = ob & 31u;
                v[u] = *reinterpret_cast<const pair2_t*>(base + (size_t)(ob >> 5) * 8u);   // pairs q + li and q + li + 1 of the lane's frame
            }
            uint32_t x1[8], x4[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                x1[u] = __builtin_amdgcn_alignbit(v[u].z, v[u].x, sh[u]);
                x4[u] = __builtin_amdgcn_alignbit(v[u].w, v[u].y, sh[u]);
            }
            e1 = add8(x1, c1[0], c1[1], c1[2]);
            e4 = add8(x4, c4[0], c4[1], c4[2]);
        };
        for (int f = 0; f < nfp; f += 16) {
            uint32_t a1, a4;
            batch(f, a1, a4);
            if (f + 8 < nfp) {
                uint32_t b1, b4;
                batch(f + 8, b1, b4);
                add_eights2<kN>(c1, a1, b1);
                add_eights2<kN>(c4, a4, b4);
            } else {
                add_eights1<kN>(c1, a1);
                add_eights1<kN>(c4, a4);
            }
        }
    }
    uint32_t S[kS];
    weighted_sum<kA, kN>(S, c1, c4);
    uint32_t summed;
    uint32_t hit_mask = coarse_hit_mask<kS>(S, h.rmin, h.zero_passes, limit, h.npos, pos0, summed);
    if (!act) hit_mask = 0;
    // the wave's scan, cut where a frame begins: a frame's lanes are consecutive, so its part of the scan starts at its first lane in this wave
    int total;
    const int mine = __popc(hit_mask);
    const int before = wave_excl_scan(mine, lane, total);
    const int head = lane - li > 0 ? lane - li : 0;                         // the first lane of this lane's frame in the wave
    const int in_frame = before - __shfl(before, head, 64);                 // hits of this (template, frame) in the wave before this lane's
    __syncthreads();                                                        // s_cnt is zero
    if (act && (lane == 63 || li == L - 1)) s_cnt[wv][fl] = (uint32_t)(in_frame + mine);   // the last lane of the frame in the wave
    __syncthreads();
    if ((int)threadIdx.x < nfr) {                                           // one atomic per frame and workgroup
        uint32_t run = 0;
        for (int w = 0; w < nwaves; ++w) { const uint32_t c = s_cnt[w][threadIdx.x]; s_cnt[w][threadIdx.x] = run; run += c; }
        s_base[threadIdx.x] = run ? atomicAdd(&fb.f[f0 + (int)threadIdx.x].counters[0], (unsigned long long)run) : 0ull;
    }
    __syncthreads();
    if (hit_mask) {
        const unsigned long long slot = s_base[fl] + (unsigned long long)s_cnt[wv][fl] + (unsigned long long)in_frame;
        coarse_emit<kS>(hit_mask, summed, S, slot, cap, pos0, h.Wd, h.T, h.offset, h.nf, h.work, fb.f[frame].cands);
    }
}

hipError_t launch_pack_top(const TopBits& B, int nb, uint32_t byte0, uint32_t npairs, hipStream_t s) {
    if (npairs == 0 || nb <= 0) return hipSuccess;   // an empty pair stream / batch: nothing to pack
    return lm_launch(k_pack_top, dim3((npairs + 255) / 256, nb), dim3(256), 0, s, B, byte0, npairs);
}
bool coarse_batch_plan(int nb, int npos, CoarseBatchPlan* p) {
    const int lanes_max = 64 * kCoarseBatchWaves;
    p->L = (npos + 31) / 32;
    if (nb < 1 || npos < 1 || p->L > lanes_max) return false;              // a frame has to fit a workgroup (32768 positions)
    const int fit = lanes_max / p->L;                                       // frames a workgroup holds
    p->groups = (nb + fit - 1) / fit;
    p->fpg = (nb + p->groups - 1) / p->groups;                              // dealt evenly: 8 frames of 150 lanes are 4 + 4, not 6 + 2
    p->groups = (nb + p->fpg - 1) / p->fpg;
    p->Wg = (p->fpg * p->L + 63) / 64;
    // templates per workgroup: workgroups of about four waves, as k_coarse_bits's.  Larger ones cost more than their fewer atomics save — VGA, 8 frames,
    // 2000 templates: 66.5 us with one template (5 waves) per workgroup, 75.5 / 75.2 us with two / three (profiles/coarse_batch_kernel_ab.txt)
    p->tpw = std::max(1, 4 / p->Wg);
    p->waves = 0;
    for (int f = 0; f < nb; f += p->fpg) p->waves += (std::min(p->fpg, nb - f) * p->L + 63) / 64;
    p->waves_per_frame_kernel = nb * ((p->L + 63) / 64);
    return true;
}
hipError_t launch_coarse_bits(const FrameBatch& fb, const TopBits& B, const FrameGeom& g, const BankDev& bank, int num_work, float threshold, uint32_t cap, uint32_t byte0, int max_features, int low_weight, hipStream_t s,
                              bool* batched_out, int batch_mode) {
    *batched_out = false;
    if (num_work <= 0 || fb.nb <= 0) return hipSuccess;
    const int level = g.levels - 1;
    CoarseBatchPlan p;
    const bool can = coarse_batch_plan(fb.nb, g.lv[level].Wd * g.lv[level].Hd, &p);
    const bool batched = can && (batch_mode > 0 || (batch_mode < 0 && fb.nb >= 2 && p.waves < p.waves_per_frame_kernel));
    *batched_out = batched;
    return with_bits_instance<6, 5>(max_features, low_weight, [&](auto hi, auto waves, auto a) {
        if (batched)
            return lm_launch(k_coarse_bits_batch<hi(), waves(), a()>, dim3((num_work + p.tpw - 1) / p.tpw, p.groups), dim3(64 * p.tpw * p.Wg), 0, s, fb, B, g.lv[level], level,
                             g.levels, bank.entries, bank.feat_off, bank.work, num_work, threshold, cap, byte0, p.L, p.fpg, p.Wg);
        return lm_launch(k_coarse_bits<hi(), waves(), a()>, dim3((num_work + 3) / 4, fb.nb), dim3(256), 0, s, fb, B, g.lv[level], level, g.levels, bank.entries,
                         bank.feat_off, bank.work, num_work, threshold, cap, byte0);
    });
}

}  // namespace lm
