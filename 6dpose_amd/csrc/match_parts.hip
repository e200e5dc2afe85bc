// Part-based matching on bit planes: k_coarse_parts and k_local_parts, what k_coarse_bits and k_local_bits
// (match_bits.hip) are under the rule "at least min_parts of the template's 4 quadrants pass the threshold on their own" — the reference
// author's first answer to occlusion (linemodLevelup/notes.md:1-9), dropped there because four sets of sums were slow on the CPU.  Here the
// loads are those of the holistic kernels — the same features in another order (part by part, each padded to kFeatBatch: PartEntry,
// lm_kernels.h) — and a part costs an epilogue: its bit-sliced sum S_p, ONE bit-sliced comparison against the part's bound, an increment of a
// 3-bit bit-sliced pass count, and a ripple add of S_p into the holistic sum S.  A lane keeps one part's counters, S and three words, not
// four sets of counters.  Positions, slot order, window, arg-max (on S) and scores (of S) are the holistic kernels': the stages of
// match_planes.h.  The rule itself is stated in tests/part_match_ref.py.
#include "launch.h"
#include "match_planes.h"

namespace lm {

// ---- Coarse pass: k_coarse_bits's load scheme (a wave per template, a lane = 32 consecutive positions, the pair stream through buffer
// loads with scalar offsets and shifts).  A part passes at a position iff it is eligible and score_of(raw_p, n_p) > threshold: raw_p >=
// coarse_rmin(threshold, n_p), wave-uniform.  threshold >= 0 (the host refuses anything else), so a sum of zero never passes and the
// positions without sums (at or beyond the template's position count) are never candidates.
template <int kHi, int kWaves, int kA>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_coarse_parts(FrameBatch fb, TopBits B, LevelGeom lv, int level, int levels, const TemplEntry* __restrict__ entries, const PartEntry* __restrict__ parts,
               const int32_t* __restrict__ part_off, const int32_t* __restrict__ work_pyramids, int num_work, float threshold, int min_parts, uint32_t cap, uint32_t byte0) {
    constexpr int kN = 4 + kHi, kS = kN + 3;
    __shared__ uint32_t s_tot[4];
    __shared__ unsigned long long s_base;
    const FrameSlot& F = fb.f[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const CoarseHead h = coarse_head((int)blockIdx.x * 4 + wave, num_work, entries, part_off, work_pyramids, lv, level, levels, threshold);   // (h.fo, h.rmin: the holistic ones, unused)
    const bool live = h.live;
    const int npos = h.npos, limit = h.limit;
    const PartEntry* pe = parts + (size_t)work_pyramids[h.work] * levels + level;
    const BufRsrc bits = make_rsrc(B.bits[blockIdx.y]);
    for (int P0 = 0; P0 < npos; P0 += 2048) {                               // (the same number of passes for every wave of the workgroup)
        const int pos0 = P0 + 32 * lane;                                    // first position of this lane
        const bool loads = live && P0 < limit && pos0 < limit;              // (lanes beyond the map sit the loads out)
        uint32_t S[kS];                                                     // the holistic sum
#pragma unroll
        for (int k = 0; k < kS; ++k) S[k] = 0;
        uint32_t q0 = 0, q1 = 0, q2 = 0, summed = 0;                        // the parts that pass, counted per position
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int np = pe->n[p], npp = pe->npad[p];
            const int32_t* fo = part_off + pe->start[p];
            uint32_t c1[kN], c4[kN];
#pragma unroll
            for (int k = 0; k < kN; ++k) { c1[k] = 0; c4[k] = 0; }
            if (loads) {
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
                        x1[u] = __builtin_amdgcn_alignbit(v[u].z, v[u].x, sh[u]);
                        x4[u] = __builtin_amdgcn_alignbit(v[u].w, v[u].y, sh[u]);
                    }
                    e1 = add8(x1, c1[0], c1[1], c1[2]);
                    e4 = add8(x4, c4[0], c4[1], c4[2]);
                };
                for (int f = 0; f < npp; f += 16) {
                    uint32_t a1, a4;
                    batch(f, a1, a4);
                    if (f + 8 < npp) {
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
            uint32_t Sp[kS];
            weighted_sum<kA, kN>(Sp, c1, c4);
            const int rmin = (pe->eligible >> p) & 1u ? coarse_rmin(threshold, np) : (1 << kS);   // an ineligible part never passes
            count3_add(q0, q1, q2, coarse_hit_mask<kS>(Sp, rmin, false, limit, npos, pos0, summed));
            sliced_add<kS>(S, Sp);
        }
        uint32_t hit_mask = count3_ge(q0, q1, q2, min_parts);               // (within `summed`: every part's mask is)
        if (!live) hit_mask = 0;
        int total;
        const unsigned long long slot = coarse_reserve_slots(s_tot, s_base, F.counters, hit_mask, lane, wave, total);
        if (total > 0)                                                      // wave-uniform
            coarse_emit<kS>(hit_mask, summed, S, slot, cap, pos0, h.Wd, h.T, h.offset, h.nf, h.work, F.cands);
    }
}

// ---- Refinement: k_local_bits's load scheme (8 lanes per candidate, lane j = window rows 2j and 2j + 1, two feature words per lane and 16
// features, shared through ds_bpermute), all levels below the top walked here.  Window, clamp, arg-max (first maximum of the holistic sum) and
// position update are the holistic ones; only the drop test differs: the candidate stays alive iff at least min_parts eligible parts have
// score_of(raw_p at the arg-max position, n_p) >= threshold, i.e. raw_p >= local_rmin(threshold, n_p).  The bound differs between the 8
// candidates of a wave, so the comparison takes it per lane (sliced_ge); lane j of a candidate works out part j's bound for the others.
// The host launches this kernel only for banks and geometries whose windows never leave their planes (bits_all_in): `leave` stays false.
template <int kHi, int kWaves, int kA>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kWaves, kWaves)))
k_local_parts(FrameBatch fb, BitsBatch B, FrameGeom g, const TemplEntry* __restrict__ entries, const PartEntry* __restrict__ parts, const uint32_t* __restrict__ part_word,
              const int32_t* __restrict__ work_pyramids, uint32_t cand_cap, float threshold, int min_parts, uint32_t cap, uint32_t dedupe_cap_slots) {
    constexpr int kN = 4 + kHi;                                     // counter bits per plane
    constexpr int kS = kN + 3;                                      // bits of n1 + 4 n4
    __shared__ unsigned long long s_acc[kMaxBatch][2];
    __shared__ uint32_t s_cnt[kMaxBatch];
    const int lane = threadIdx.x & 63, grp = lane >> 3, j = lane & 7;
    const int nb = fb.nb;
    const LocalShare share = local_share(nb);
    local_prologue(fb, s_cnt, s_acc, cand_cap, dedupe_cap_slots);
    // The pair stream k_coarse_parts has just read is zeroed for the slot's next frame, as k_local_bits does
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
            bool alive = valid, leave = false;
            uint32_t evals = 0, bytes = 0;
            for (int l = g.levels - 2; l >= 0; --l) {
                const LevelGeom& lv = g.lv[l];
                const TemplEntry e = entries[(size_t)pyr * g.levels + l];
                const uint32_t ei = (uint32_t)(pyr * g.levels + l);     // (an index, not a pointer: a register less across the part loop)
                const LocalWindow win = local_window(lv, e, mx, my, alive, leave);
                // part (j & 3)'s bound, worked out by lanes j and j + 4 of the candidate
                const int my_bound = (parts[ei].eligible >> (j & 3)) & 1u ? local_rmin(threshold, (int)parts[ei].n[j & 3]) : (1 << kS);
                uint32_t S[kS];                                     // the holistic sum of the lane's two rows, interleaved as local_argmax takes it
#pragma unroll
                for (int k = 0; k < kS; ++k) S[k] = 0;
                uint32_t q0 = 0, q1 = 0, q2 = 0;                    // the parts that pass, counted per position
#pragma unroll 1
                for (int p = 0; p < 4; ++p) {
                    const int nfp = win.run ? (int)parts[ei].npad[p] : 0;
                    int nmax = nfp;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(nmax, o, 64); nmax = t > nmax ? t : nmax; }
                    nmax = __builtin_amdgcn_readfirstlane(nmax);
                    const uint32_t* fw = part_word + parts[ei].start[p];
                    uint32_t cA[kN], cB[kN];                        // bit-sliced counters of rows 2j / 2j + 1: even bits count the 1s, odd bits the 4s
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
                            xa[u] = __builtin_amdgcn_alignbit(v[u].y, v[u].x, sh[u]);
                            xb[u] = __builtin_amdgcn_alignbit(v[u].w, v[u].z, sh[u]);
                        }
                        eA = add8(xa, cA[0], cA[1], cA[2]);
                        eB = add8(xb, cB[0], cB[1], cB[2]);
                    };
                    uint2 wn = local_fetch(fw, 0, j, nfp);
                    for (int f0 = 0; f0 < nmax; f0 += 16) {
                        const uint2 wd = wn;
                        const bool on = f0 + 2 * j < nfp;
                        wn = local_fetch(fw, f0 + 16, j, nfp);      // the next 16 words while these are worked on
                        local_prep(wd.x, on, win.gxl, win.Kbase, win.HS8, win.zero_off, offx, sx);
                        local_prep(wd.y, on, win.gxl, win.Kbase, win.HS8, win.zero_off, offy, sy);
                        uint32_t e1A, e1B;
                        batch(0, e1A, e1B);
                        if (f0 + 8 < nmax) {                        // wave-uniform
                            uint32_t e2A, e2B;
                            batch(1, e2A, e2B);
                            add_eights2<kN>(cA, e1A, e2A);
                            add_eights2<kN>(cB, e1B, e2B);
                        } else {
                            add_eights1<kN>(cA, e1A);
                            add_eights1<kN>(cB, e1B);
                        }
                    }
                    uint32_t Sp[kS];
                    {
                        uint32_t n1[kN], n4[kN];
                        local_interleave<kN>(n1, n4, cA, cB);
                        weighted_sum<kA, kN>(Sp, n1, n4);
                    }
                    const int bound = __shfl(my_bound, (lane & ~7) + p, 64);
                    count3_add(q0, q1, q2, sliced_ge<kS>(Sp, bound));
                    sliced_add<kS>(S, Sp);
                }
                int raw, br, bc;
                local_argmax<kS>(S, j, raw, br, bc);
                // the pass count at the arg-max position: row br = bit (br & 1) of column bc in lane br >> 1 (raw <= 0: every sum is zero, any position serves)
                const int at = raw > 0 ? 2 * bc + (br & 1) : 0;
                const int mine = (int)((q0 >> at) & 1u) + 2 * (int)((q1 >> at) & 1u) + 4 * (int)((q2 >> at) & 1u);
                const int passed = __shfl(mine, (lane & ~7) + (raw > 0 ? br >> 1 : 0), 64);
                local_update(win, lv.T, raw, br, bc, -__builtin_inff() /* no score lies below: the drop test is the parts' */, sim, mx, my, alive, evals, bytes);
                if (win.run && passed < min_parts) alive = false;
            }
            if (valid && j == 0) local_store(F, ci, leave, cap, mx, my, sim, alive, work, s_acc[fr], evals, bytes);
        }
    }
    local_flush_stats(fb, s_acc);
}

hipError_t launch_coarse_parts(const FrameBatch& fb, const TopBits& B, const FrameGeom& g, const BankDev& bank, const PartsDev& parts, int num_work, float threshold, uint32_t cap,
                         uint32_t byte0, int max_features, int low_weight, hipStream_t s) {
    if (num_work <= 0 || fb.nb <= 0) return hipSuccess;
    const int level = g.levels - 1;
    return with_bits_instance<5, 4>(max_features, low_weight, [&](auto hi, auto waves, auto a) {
        return lm_launch(k_coarse_parts<hi(), waves(), a()>, dim3((num_work + 3) / 4, fb.nb), dim3(256), 0, s, fb, B, g.lv[level], level, g.levels, bank.entries, parts.table,
                         parts.feat_off, bank.work, num_work, threshold, parts.min_parts, cap, byte0);
    });
}
hipError_t launch_local_parts(const FrameBatch& fb, const BitsBatch& B, const FrameGeom& g, const BankDev& bank, const PartsDev& parts, uint32_t cand_cap, float threshold,
                        uint32_t cap, uint32_t dedupe_cap_slots, int grid_blocks, int max_features, int low_weight, hipStream_t s) {
    return with_bits_instance<4, 3>(max_features, low_weight, [&](auto hi, auto waves, auto a) {   // (14-bit counters + the holistic sum: 3 waves per SIMD keep them in registers)
        return lm_launch(k_local_parts<hi(), waves(), a()>, dim3(grid_blocks), dim3(256), 0, s, fb, B, g, bank.entries, parts.table, parts.feat_word, bank.work, cand_cap, threshold,
                         parts.min_parts, cap, dedupe_cap_slots);
    });
}

}  // namespace lm
