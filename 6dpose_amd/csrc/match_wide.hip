// Similarity kernels of Detector::matchClass on gfx950 for response tables of three or four distinct non-zero values (4 3 2 1 0, 4 2 1 0 0,
// 4 3 1 0 0, ...), selected with lm_detector_set_paths(3, 2): the schemes of match_bits.hip on TWO sets of bit planes —
// its kernels' stages through match_planes.h; here only what the second set changes: the loads, the third counter, the sum, the packing.
// A response v = 0..4 is three binary digits: set 0 keeps the two-plane layout with bit 2c = v & 1 and bit 2c + 1 = (v == 4), set 1 — a second
// arena of the same layout and size — holds (v >> 1) & 1 at bit 2c and nothing at bit 2c + 1, so the same v_alignbit windows cut both.  The sum of
// a position is c0 + 2 c1 + 4 c2 with c_i = the number of features whose digit i is set there: three bit-sliced counters instead of two.
// k_pack_wide / k_local_wide: strip records of the levels below the top; k_pack_top_wide / k_coarse_wide: pair stream of the top level.  The
// front end writes the byte planes for such tables and these kernels pack them (the front end's own bit-plane writers know two planes).
#include "launch.h"
#include "match_planes.h"

namespace lm {

// S = n1 + 2 n2 + 4 n4, bit-sliced: each count <= features < 2^kN, so n1 + 2 n2 fits kN + 2 bits and S <= 4 features fits kN + 3
template <int kN>
static __device__ __forceinline__ void weighted_sum_wide(uint32_t (&S)[kN + 3], const uint32_t (&n1)[kN], const uint32_t (&n2)[kN], const uint32_t (&n4)[kN]) {
    constexpr int kS = kN + 3;
    uint32_t t[kN + 2];
    uint32_t carry = 0;
    t[0] = n1[0];
#pragma unroll
    for (int k = 1; k < kN + 2; ++k) csa(t[k], carry, k < kN ? n1[k] : 0u, k - 1 < kN ? n2[k - 1] : 0u, carry);
    carry = 0;
    S[0] = t[0]; S[1] = t[1];
#pragma unroll
    for (int k = 2; k < kS; ++k) csa(S[k], carry, k < kN + 2 ? t[k] : 0u, k - 2 < kN ? n4[k - 2] : 0u, carry);
}

// 4 response bytes -> 8 bits, cell k at bits 2k and 2k + 1 (the multiply of match_bits.hip's pack4: partial products land on distinct bits).
// Set 0: bit 0 of the byte (v & 1) and bit 2 (v == 4); set 1: bit 1 of the byte, nothing above it.
static __device__ __forceinline__ uint32_t wide4_set0(uint32_t d) { return ((((d & 0x01010101u) | ((d >> 1) & 0x02020202u)) * 0x01041040u) >> 24); }
static __device__ __forceinline__ uint32_t wide4_set1(uint32_t d) { return ((((d >> 1) & 0x01010101u) * 0x01041040u) >> 24); }
static __device__ __forceinline__ uint32_t wide16_set0(const uint4& v) { return wide4_set0(v.x) | (wide4_set0(v.y) << 8) | (wide4_set0(v.z) << 16) | (wide4_set0(v.w) << 24); }
static __device__ __forceinline__ uint32_t wide16_set1(const uint4& v) { return wide4_set1(v.x) | (wide4_set1(v.y) << 8) | (wide4_set1(v.z) << 16) | (wide4_set1(v.w) << 24); }

// Both sets of strip records from the strip bytes
__global__ void __launch_bounds__(256)
k_pack_wide(BitsBatch B, WidePlanes P, uint32_t sm_off0, uint32_t records, int NS, int Hd) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= records) return;
    uint4 a, b;
    const size_t at = strip_cells(B.strips[blockIdx.y], sm_off0, i, NS, Hd, a, b);
    *reinterpret_cast<uint2*>(B.bits[blockIdx.y] + at) = make_uint2(wide16_set0(a), wide16_set0(b));
    *reinterpret_cast<uint2*>(P.set1[blockIdx.y] + at) = make_uint2(wide16_set1(a), wide16_set1(b));
}

// Refinement on two sets of strip records: k_local_bits's scheme — 8 lanes per candidate, lane j owns window rows 2j and 2j + 1, 8 consecutive
// candidates of one template per wave, the record offsets and shifts of 16 features formed once per group and handed round with ds_bpermute —
// with TWO 16-byte loads per lane and feature (the same offset into either arena) and THREE counters: cA / cB count set 0 of rows 2j / 2j + 1
// (even bits: digit 0, odd bits: v == 4), cC counts digit 1 of both rows at once — set 1 has nothing in its odd bits, so row 2j + 1's window
// goes there (one v_lshl_or_b32).  Per lane and feature: 1 add, 4 v_alignbit, 1 shift-or, 7.5 adder operations.  All levels below the top are
// walked here; candidates whose windows leave their planes are marked in `todo` for k_local's per-candidate path, exactly as k_local_bits does.
template <int kHi, int kWaves, int kInFlight>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_local_wide(FrameBatch fb, BitsBatch B, WidePlanes P, FrameGeom g, const TemplEntry* __restrict__ entries, const uint32_t* __restrict__ feat_word,
             const int32_t* __restrict__ work_pyramids, uint32_t cand_cap, float threshold, uint32_t cap, uint32_t dedupe_cap_slots) {
    constexpr int kN = 4 + kHi;                                     // counter bits per digit
    constexpr int kS = kN + 3;                                      // bits of n1 + 2 n2 + 4 n4
    __shared__ unsigned long long s_acc[kMaxBatch][2];
    __shared__ uint32_t s_cnt[kMaxBatch];
    const int lane = threadIdx.x & 63, grp = lane >> 3, j = lane & 7;
    const LocalShare share = local_share(fb.nb);
    local_prologue(fb, s_cnt, s_acc, cand_cap, dedupe_cap_slots);
    const int src0 = (lane & ~7) << 2;                              // ds_bpermute address of the group's first lane
    const uint32_t rowoff = 16u * (uint32_t)j;                      // records of rows 2j, 2j + 1 behind the window's first row
    for (int fr = share.f_lo; fr < share.f_hi; ++fr) {
        const FrameSlot& F = fb.f[fr];
        const BufRsrc bits0 = make_rsrc(B.bits[fr]), bits1 = make_rsrc(P.set1[fr]);
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
                uint32_t cA[kN], cB[kN], cC[kN];
#pragma unroll
                for (int k = 0; k < kN; ++k) { cA[k] = 0; cB[k] = 0; cC[k] = 0; }
                uint32_t offx = 0, offy = 0, sx = 0, sy = 0;
                auto batch = [&](int half, uint32_t& eA, uint32_t& eB, uint32_t& eC) {   // features 8 half .. 8 half + 7 of the current 16
                    uint32_t xa[8], xb[8], xc[8];
#pragma unroll
                    for (int q = 0; q < 8; q += kInFlight) {        // kInFlight features x 2 sets = the loads a lane keeps in flight
                        uint4 v[kInFlight], w[kInFlight];
                        uint32_t sh[kInFlight];
#pragma unroll
                        for (int u = 0; u < kInFlight; ++u) {
                            const int src = src0 + 4 * (4 * half + ((q + u) >> 1));    // the lane that fetched feature 8 half + q + u
                            const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(((q + u) & 1) ? offy : offx));
                            sh[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(((q + u) & 1) ? sy : sx));
                            v[u] = ld_buf16(bits0, o + rowoff, 0u); // rows 2j, 2j + 1 of set 0: 32 cells x {v & 1, v == 4} each
                            w[u] = ld_buf16(bits1, o + rowoff, 0u); // ... of set 1: 32 cells x {(v >> 1) & 1, -}
                        }
#pragma unroll
                        for (int u = 0; u < kInFlight; ++u) {
                            xa[q + u] = __builtin_amdgcn_alignbit(v[u].y, v[u].x, sh[u]);      // 16 window cells of row 2j: bits 2c (digit 0), 2c + 1 (is 4)
                            xb[q + u] = __builtin_amdgcn_alignbit(v[u].w, v[u].z, sh[u]);      // ... of row 2j + 1
                            xc[q + u] = __builtin_amdgcn_alignbit(w[u].y, w[u].x, sh[u]) | (__builtin_amdgcn_alignbit(w[u].w, w[u].z, sh[u]) << 1);   // digit 1: bit 2c row 2j, bit 2c + 1 row 2j + 1
                        }
                    }
                    eA = add8(xa, cA[0], cA[1], cA[2]);
                    eB = add8(xb, cB[0], cB[1], cB[2]);
                    eC = add8(xc, cC[0], cC[1], cC[2]);
                };
                uint2 wn = local_fetch(fw, 0, j, nfp);
                for (int f0 = 0; f0 < nmax; f0 += 16) {
                    const uint2 wd = wn;
                    const bool on = f0 + 2 * j < nfp;
                    wn = local_fetch(fw, f0 + 16, j, nfp);          // the next 16 words while these are worked on
                    local_prep(wd.x, on, win.gxl, win.Kbase, win.HS8, win.zero_off, offx, sx);
                    local_prep(wd.y, on, win.gxl, win.Kbase, win.HS8, win.zero_off, offy, sy);
                    uint32_t e1A, e1B, e1C;
                    batch(0, e1A, e1B, e1C);
                    if (f0 + 8 < nmax) {                            // wave-uniform
                        uint32_t e2A, e2B, e2C;
                        batch(1, e2A, e2B, e2C);
                        add_eights2<kN>(cA, e1A, e2A);
                        add_eights2<kN>(cB, e1B, e2B);
                        add_eights2<kN>(cC, e1C, e2C);
                    } else {
                        add_eights1<kN>(cA, e1A);
                        add_eights1<kN>(cB, e1B);
                        add_eights1<kN>(cC, e1C);
                    }
                }
                // Once per candidate and level: the two rows of the lane side by side (cC is kept that way), S bit-sliced, its maximum and where
                uint32_t S[kS];
                {
                    uint32_t n1[kN], n4[kN];
                    local_interleave<kN>(n1, n4, cA, cB);
                    weighted_sum_wide<kN>(S, n1, cC, n4);
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

hipError_t launch_pack_wide(const BitsBatch& B, const WidePlanes& P, int nb, const LevelGeom& lv, hipStream_t s) {
    const uint32_t records = (uint32_t)(2 * 8 * lv.T * lv.T) * (uint32_t)lv.NS * (uint32_t)lv.Hd;
    if (records == 0 || nb <= 0) return hipSuccess;   // an empty level / batch: nothing to pack
    return lm_launch(k_pack_wide, dim3((records + 255) / 256, nb), dim3(256), 0, s, B, P, lv.sm_off[0], records, lv.NS, lv.Hd);
}
hipError_t launch_local_wide(const FrameBatch& fb, const BitsBatch& B, const WidePlanes& P, const FrameGeom& g, const BankDev& bank, uint32_t cand_cap, float threshold,
                       uint32_t cap, uint32_t dedupe_cap_slots, int grid_blocks, int max_features, hipStream_t s) {
    const auto kernel = max_features > kBitsSmallMax ? k_local_wide<10, 3, 4> : k_local_wide<5, 4, 2>;   // 158 / 126 VGPRs, no spills (5, 4, 4 spills one)
    return lm_launch(kernel, dim3(grid_blocks), dim3(256), 0, s, fb, B, P, g, bank.entries, bank.feat_word, bank.work, cand_cap, threshold, cap, dedupe_cap_slots);
}

// ---- Coarse pass on two pair streams: k_coarse_bits's scheme — a wave per template, a lane = 32 consecutive positions, a feature's load =
// two consecutive pairs per lane at a wave-uniform pair index, funnel-shifted by a wave-uniform amount — with one such load per set and
// three counters.  Template head, hit test, slot reservation and emission are k_coarse_bits's, through match_planes.h.
__global__ void __launch_bounds__(256)
k_pack_top_wide(TopBits B, WidePlanes P, uint32_t byte0, uint32_t npairs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npairs) return;
    const uint8_t* src = B.lm[blockIdx.y] + byte0 + (size_t)i * 32;
    const uint4 a = *reinterpret_cast<const uint4*>(src), b = *reinterpret_cast<const uint4*>(src + 16);
    *reinterpret_cast<uint2*>(B.bits[blockIdx.y] + (size_t)i * 8) = make_uint2(byte_bits32(a, b, 0), byte_bits32(a, b, 2));   // v & 1, v == 4
    *reinterpret_cast<uint2*>(P.set1[blockIdx.y] + (size_t)i * 8) = make_uint2(byte_bits32(a, b, 1), 0u);                    // (v >> 1) & 1, -
}

template <int kHi, int kWaves, int kInFlight>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_coarse_wide(FrameBatch fb, TopBits B, WidePlanes P, LevelGeom lv, int level, int levels, const TemplEntry* __restrict__ entries, const int32_t* __restrict__ feat_off,
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
    const BufRsrc bits0 = make_rsrc(B.bits[blockIdx.y]), bits1 = make_rsrc(P.set1[blockIdx.y]);
    for (int P0 = 0; P0 < npos; P0 += 2048) {                               // (the same number of passes for every wave of the workgroup)
        const int pos0 = P0 + 32 * lane;                                    // first position of this lane
        uint32_t c1[kN], c2[kN], c4[kN];
#pragma unroll
        for (int k = 0; k < kN; ++k) { c1[k] = 0; c2[k] = 0; c4[k] = 0; }
        if (live && P0 < limit && nfp > 0 && pos0 < limit) {                // (lanes beyond the map sit the loads out)
            auto batch = [&](int f, uint32_t& e1, uint32_t& e2, uint32_t& e4) {
                uint32_t x1[8], x2[8], x4[8];
#pragma unroll
                for (int q = 0; q < 8; q += kInFlight) {                                 // kInFlight features x 2 sets = the loads a lane keeps in flight
                    uint4 v[kInFlight], w[kInFlight];
                    uint32_t sh[kInFlight];
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u) {
                        const uint32_t ob = (uint32_t)fo[f + q + u] - byte0 + (uint32_t)P0;   // wave-uniform -> SMEM / SALU
                        sh[u] = ob & 31u;
                        v[u] = ld_buf16(bits0, (uint32_t)lane * 8u, (ob >> 5) * 8u);     // pairs p + lane and p + lane + 1 of set 0
                        w[u] = ld_buf16(bits1, (uint32_t)lane * 8u, (ob >> 5) * 8u);     // ... of set 1
                    }
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u) {
                        x1[q + u] = __builtin_amdgcn_alignbit(v[u].z, v[u].x, sh[u]);    // bits [s, s + 32) of {digit 0 of pair p + lane + 1 : pair p + lane}
                        x4[q + u] = __builtin_amdgcn_alignbit(v[u].w, v[u].y, sh[u]);
                        x2[q + u] = __builtin_amdgcn_alignbit(w[u].z, w[u].x, sh[u]);
                    }
                }
                e1 = add8(x1, c1[0], c1[1], c1[2]);
                e2 = add8(x2, c2[0], c2[1], c2[2]);
                e4 = add8(x4, c4[0], c4[1], c4[2]);
            };
            for (int f = 0; f < nfp; f += 16) {
                uint32_t a1, a2, a4;
                batch(f, a1, a2, a4);
                if (f + 8 < nfp) {
                    uint32_t b1, b2, b4;
                    batch(f + 8, b1, b2, b4);
                    add_eights2<kN>(c1, a1, b1);
                    add_eights2<kN>(c2, a2, b2);
                    add_eights2<kN>(c4, a4, b4);
                } else {
                    add_eights1<kN>(c1, a1);
                    add_eights1<kN>(c2, a2);
                    add_eights1<kN>(c4, a4);
                }
            }
        }
        uint32_t S[kS];
        weighted_sum_wide<kN>(S, c1, c2, c4);
        uint32_t summed;
        uint32_t hit_mask = coarse_hit_mask<kS>(S, h.rmin, h.zero_passes, limit, npos, pos0, summed);
        if (!live) hit_mask = 0;
        int total;
        const unsigned long long slot = coarse_reserve_slots(s_tot, s_base, F.counters, hit_mask, lane, wave, total);
        if (total > 0)                                                      // wave-uniform
            coarse_emit<kS>(hit_mask, summed, S, slot, cap, pos0, h.Wd, h.T, h.offset, h.nf, h.work, F.cands);
    }
}

hipError_t launch_pack_top_wide(const TopBits& B, const WidePlanes& P, int nb, uint32_t byte0, uint32_t npairs, hipStream_t s) {
    if (npairs == 0 || nb <= 0) return hipSuccess;   // an empty pair stream / batch: nothing to pack
    return lm_launch(k_pack_top_wide, dim3((npairs + 255) / 256, nb), dim3(256), 0, s, B, P, byte0, npairs);
}
hipError_t launch_coarse_wide(const FrameBatch& fb, const TopBits& B, const WidePlanes& P, const FrameGeom& g, const BankDev& bank, int num_work, float threshold, uint32_t cap,
                        uint32_t byte0, int max_features, hipStream_t s) {
    if (num_work <= 0 || fb.nb <= 0) return hipSuccess;
    const int level = g.levels - 1;
    const auto kernel = max_features > kBitsSmallMax ? k_coarse_wide<10, 4, 2> : k_coarse_wide<5, 5, 2>;   // 109 / 89 VGPRs
    return lm_launch(kernel, dim3((num_work + 3) / 4, fb.nb), dim3(256), 0, s, fb, B, P, g.lv[level], level, g.levels, bank.entries, bank.feat_off, bank.work, num_work,
                     threshold, cap, byte0);
}

}  // namespace lm
