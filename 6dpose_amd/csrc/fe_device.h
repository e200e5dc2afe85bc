// What both front-end translation units use (fe_quant.hip: the quantising chains and the byte linear memories, k_fe_stage;
// fe_bits.hip: the bit planes, k_fe_bits): the exact division by a prepared multiplier, spread (LL.cpp:1094-1109), the byte rotation
// under both forms of the response table (LL.cpp:1112-1124), and the host side of the job table that both launchers share.  What one unit alone uses stays in that unit.  gfx950 only.
#pragma once
#include "lm_kernels.h"

namespace lm {

// n / d by a multiplier the host prepares (lm_kernels.h, FeJob): exact while n * d < 2^32; m = 0 stands for d = 1
static __host__ __device__ __forceinline__ uint32_t div_magic(uint32_t d) { return d <= 1 ? 0u : (uint32_t)((0x100000000ull + d - 1) / d); }
// n / d with m = div_magic(d) = ceil(2^32 / d): umulhi(n, m) is floor(n / d) or one more (the excess n e / (d 2^32), e = m d - 2^32 < d, stays
// below 1 for every 32-bit n), so one comparison makes it exact for ANY n — an 8000 x 6000 frame puts n d past 2^32, where the bare product
// was wrong for the last blocks of a job.  The comparison itself cannot wrap: q d <= n + d, and every caller passes non-negative `int`
// values (block / pixel / phase indices and image sizes), so n + d < 2^31 + 2^31 = 2^32 — asserted in the debug build below.
static __device__ __forceinline__ uint32_t fast_div(uint32_t n, uint32_t m, uint32_t d) {
#ifdef LM_DIAG
    if ((n | d) >> 31) __builtin_trap();                   // n, d < 2^31: q * d <= n + d < 2^32
#endif
    if (!m) return n;
    const uint32_t q = __umulhi(n, m);
    return q - (q * d > n ? 1u : 0u);
}

// OR of the T x T quantised pixels at and right / below (x, y) (zero beyond the edges; the mask applied as quantize() does): spread, LL.cpp:1094-1109.
// kT > 0: T known at compile time — the rows' loads are all issued before the first is waited for (with a run-time T the compiler
// emitted load, wait, OR per row: T dependent L2 round trips per thread were most of the linear-memory launch).
template <int kT>
static __device__ __forceinline__ uint32_t spread_or_t(const LmJob& J, const int x, const int y, const int W, const int H, const int Trt) {
    const int T = kT > 0 ? kT : Trt;
    uint32_t v = 0;
    const int ye = y + T < H ? y + T : H, xe = x + T < W ? x + T : W;
    if (!J.mask && x + T <= W && (kT == 0 || y + T <= H)) {
        // the T pixels of a row as (unaligned) dwords
        uint32_t acc = 0;
        if (kT > 0) {
            uint32_t w[kT > 0 ? kT * ((kT + 3) / 4) : 1];
#pragma unroll
            for (int r = 0; r < kT; ++r) {
                const uint8_t* row = J.quant + (size_t)(y + r) * W + x;
#pragma unroll
                for (int c = 0; c < (kT + 3) / 4; ++c) {
                    if (4 * c + 4 <= kT) __builtin_memcpy(&w[r * ((kT + 3) / 4) + c], row + 4 * c, 4);
                    else {                                               // the last 1-3 pixels of the row
                        uint32_t t = 0;
#pragma unroll
                        for (int b = 4 * c; b < kT; ++b) t |= row[b];
                        w[r * ((kT + 3) / 4) + c] = t;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < kT * ((kT + 3) / 4); ++i) acc |= w[i];
        } else {
            for (int r = y; r < ye; ++r) {
                const uint8_t* row = J.quant + (size_t)r * W + x;
                int c = 0;
                for (; c + 4 <= T; c += 4) { uint32_t w; __builtin_memcpy(&w, row + c, 4); acc |= w; }
                for (; c < T; ++c) acc |= row[c];
            }
        }
        v = (acc | (acc >> 8) | (acc >> 16) | (acc >> 24)) & 0xFFu;
    } else {
        for (int r = y; r < ye; ++r) {
            const uint8_t* row = J.quant + (size_t)r * W;
            if (J.mask) {
                const uint8_t* mrow = J.mask + (size_t)r * W;
                for (int c = x; c < xe; ++c) v |= mrow[c] ? (uint32_t)row[c] : 0u;
            } else {
                for (int c = x; c < xe; ++c) v |= row[c];
            }
        }
    }
    return v;
}
static __device__ __forceinline__ uint32_t spread_or(const LmJob& J, const int x, const int y, const int W, const int H, const int T) {
    switch (T) {                                                         // wave-uniform
        case 2: return spread_or_t<2>(J, x, y, W, H, T);
        case 4: return spread_or_t<4>(J, x, y, W, H, T);
        case 5: return spread_or_t<5>(J, x, y, W, H, T);
        case 8: return spread_or_t<8>(J, x, y, W, H, T);
        default: return spread_or_t<0>(J, x, y, W, H, T);
    }
}

// the response table (lm_kernels.h, resp_pack) on words whose every byte is a spread byte: every byte rotated left by d (1..7) inside itself
static __device__ __forceinline__ uint32_t rot_bytes(uint32_t v, uint32_t d) {
    const uint32_t keep = (0xFFu >> d) * 0x01010101u;                   // the bits that stay inside their byte
    return ((v & keep) << d) | ((v >> (8u - d)) & ~(keep << d));
}

// (The block decode of the persistent walk — job lookup, then (bx, by, bz) by two fast_div — is NOT here: k_fe_stage and k_fe_bits each state
// its six lines.  As one function, in any of four forms (references out, a struct by value, with or without the lookup loop), it changed
// k_fe_bits: one scalar instruction more, or the same number with other registers.)

// What the writers of response memories have in common (fe_job_build_lm, fe_job_bits_rows, fe_job_top_bits): a job over the T x T phases
// (gy) of the W / T x H / T grid of a level, gz = nm slices of blocks, one per modality.  gx and j.lm[] are the caller's.
static void fe_job_lm_grid(FeJob& j, int kind, int W, int H, int T, int nm) {
    j = FeJob{}; j.kind = kind; j.a = T; j.gy = T * T; j.gz = nm; j.W = W; j.H = H;
    j.Wd = W / T; j.Hd = H / T; j.m_wd = div_magic((uint32_t)j.Wd); j.m_t = div_magic((uint32_t)T);
}

static int fe_prepare(FeStage& st) {                             // drops empty jobs, lays the jobs' blocks out on one flat index; returns the number of blocks
    int total = 0, n = 0;
    for (int i = 0; i < st.njobs; ++i) {
        const int blocks = st.job[i].gx * st.job[i].gy * st.job[i].gz;
        if (blocks <= 0) continue;                         // an empty job (degenerate level) is dropped
        st.job[n] = st.job[i]; st.job[n].first = total; total += blocks;
        st.job[n].m_gx = div_magic((uint32_t)st.job[n].gx); st.job[n].m_gxgy = div_magic((uint32_t)(st.job[n].gx * st.job[n].gy));
        ++n;
    }
    st.njobs = n;
    return total;
}
static int fe_cus() {                                                // CUs of the CURRENT device (a process may drive several)
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev] && (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus[dev] <= 0)) cus[dev] = 256;
    return cus[dev];
}

}  // namespace lm
