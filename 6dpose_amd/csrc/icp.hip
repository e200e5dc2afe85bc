// What poseRefine::process builds over the clouds before RegistrationICP: the two VoxelDownSample calls (reference LL.cpp:108-109),
// the search grid of the target cloud, and EstimateNormals(KDTreeSearchParamKNN(30)) (LL.cpp:127), which walks that grid.
//   k_icp_voxel       VoxelDownSample by one workgroup per cloud: stable radix sort of the point indices by voxel, segment means
//   k_icp_grid        bins the target cloud into <= 64 x 64 xy columns (cell >= 5 mm), sorted by (column, depth step), one workgroup
//   k_icp_voxel_wide  the same two by kIcpSortGroups workgroups per cloud, each a contiguous range of the leading key coordinate;
//   k_icp_grid_wide   the one-workgroup kernels run behind them and take what they left (IcpState::vox_done / grid_done)
//   k_icp_knn         eight lanes per target point: ring search over the columns of the grid, the k nearest selected by counting
//                     passes (ties by index), cumulants; whole waves for the points whose ring grows
//   k_icp_knn_far     a workgroup per point for those k_icp_knn could not finish within 8 rings
//   k_icp_normals     covariance from the cumulants, eigenvector of its smallest eigenvalue in closed form (cyclic Jacobi where the
//                     closed form gives up), one thread per point
// launch_icp_prepare: the clouds (icp_clouds.hip), then these, as one stream of launches per batch of hypotheses, no host round trip
// in between.
// The sorts and the kNN search share this unit although they share no helper.  Observed, cause not found: compiled in a module
// without k_icp_knn, k_icp_voxel comes out with another register allocation (same number of instructions, 63 VGPRs instead of 54);
// every helper here but smallest_eigvec is __forceinline__, so it is an effect of the module, not of a shared function.
// Part of poseRefine::process on gfx950 (reference LL.cpp:27-155; the stages and their files: icp_kernels.h).  The cloud arithmetic is
// Open3D's (un-vendored), restated per SURVEY Appendix B with the deterministic rules of DESIGN.md §5 (shared with
// oracle/linemod_oracle.py).  All arithmetic is double like Open3D's (f64 VALU; nothing here is a dense contraction, so no MFMA).
#include <limits.h>

#include "launch.h"
#include "icp_device.h"
#include "icp_kernels.h"
#include "knobs.h"

namespace lm {

constexpr int kWG = 1024;          // workgroup size of the per-hypothesis kernels
constexpr int kSortLds = 16384;    // 64-bit keys sorted in LDS (128 KiB); longer lists use the global scratch
constexpr double kCellMin = 0.005; // search-grid cell edge (m), grown until the grid fits kIcpGrid / kIcpCells
constexpr int kIdxBits = 22;       // point-index bits of the grid sort key

// min / max of K doubles over the workgroup; result in s_out[0..K) (min) and s_out[K..2K) (max), visible after return.
template <int K>
static __device__ __forceinline__ void block_minmax(const double (&mn)[K], const double (&mx)[K], double* s_part /*[16][2K]*/,
                                                    double* s_out /*[2K]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double a[K], b[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        a[k] = mn[k]; b[k] = mx[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a[k] = fmin(a[k], shfl_xor_d(a[k], o));
            b[k] = fmax(b[k], shfl_xor_d(b[k], o));
        }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) { s_part[wave * 2 * K + k] = a[k]; s_part[wave * 2 * K + K + k] = b[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * K) {
        double v = s_part[threadIdx.x];
        for (int w = 1; w < nw; ++w) {
            const double u = s_part[w * 2 * K + threadIdx.x];
            v = threadIdx.x < K ? fmin(v, u) : fmax(v, u);
        }
        s_out[threadIdx.x] = v;
    }
    __syncthreads();
}

// Ascending bitonic sort of npad (power of two) 64-bit keys by one workgroup.
template <typename P>
static __device__ __forceinline__ void bitonic_sort(P A, int npad) {
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (npad >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned long long a = A[i], b = A[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { A[i] = b; A[l] = a; }
            }
            __syncthreads();
        }
    }
}

// The same for lists longer than the LDS buffer (npad > kSortLds keys in HBM): chunks of kSortLds keys are
// sorted / merged in LDS, only the compare-exchange steps whose partner lies in another chunk touch HBM —
// log2(npad / kSortLds) * (log2(npad / kSortLds) + 1) / 2 passes instead of ~log2(npad)^2 / 2.
static __device__ __forceinline__ void bitonic_sort_hybrid(unsigned long long* g, int npad, unsigned long long* s) {
    const int C = kSortLds;
    auto chunk_steps = [&](int c0, int k, int jmax) {            // steps j = jmax .. 1 of merge size k on the chunk at c0
        for (int i = threadIdx.x; i < C; i += blockDim.x) s[i] = g[c0 + i];
        __syncthreads();
        for (int j = jmax; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (C >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned long long a = s[i], b = s[l];
                const bool up = ((c0 + i) & k) == 0;
                if ((a > b) == up) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < C; i += blockDim.x) g[c0 + i] = s[i];
        __syncthreads();
    };
    for (int c0 = 0; c0 < npad; c0 += C)
        for (int k = 2; k <= C; k <<= 1) {
            if (k == 2) {                                          // load once, run every k <= C in LDS, store once
                for (int i = threadIdx.x; i < C; i += blockDim.x) s[i] = g[c0 + i];
                __syncthreads();
            }
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = threadIdx.x; t < (C >> 1); t += blockDim.x) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int l = i | j;
                    const unsigned long long a = s[i], b = s[l];
                    const bool up = ((c0 + i) & k) == 0;
                    if ((a > b) == up) { s[i] = b; s[l] = a; }
                }
                __syncthreads();
            }
            if (k == C) {
                for (int i = threadIdx.x; i < C; i += blockDim.x) g[c0 + i] = s[i];
                __syncthreads();
            }
        }
    for (int k = 2 * C; k <= npad; k <<= 1) {
        for (int j = k >> 1; j >= C; j >>= 1) {                    // partner in another chunk: HBM pass
            for (int t = threadIdx.x; t < (npad >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned long long a = g[i], b = g[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { g[i] = b; g[l] = a; }
            }
            __syncthreads();
        }
        for (int c0 = 0; c0 < npad; c0 += C) chunk_steps(c0, k, C >> 1);
    }
}

// Stable LSD radix sort by one workgroup of 1024 threads: n <= kSortLds 16-bit indices ordered by their 32-bit keys (the keys
// stay put in LDS, the indices move), 8 bits per pass.  Every wave owns a contiguous chunk of the list; inside a round of 64
// the lanes with the same digit find each other with 8 ballots (rank = lanes before me with my digit), the per-wave digit
// counts are prefix-summed digit-major / wave-minor, and the second walk scatters.  3 passes for the 24-bit voxel index of
// a 0.6 m cloud, 4 for the grid key — against ~105 barrier-separated compare-exchange steps of the bitonic network.
// Lists of up to 2 x kSortLds points keep their keys in HBM (u32, read through L2) and have the whole buffer for indices:
// keys | idx | idx | counts = 64 | 32 | 32 | 16 KiB for n <= 16384, idx | idx | counts = 64 | 64 | 16 KiB for n <= 32768.
constexpr int kRadixBig = 2 * kSortLds;
constexpr int kRadixLdsBytes = 2 * kRadixBig * 2 + 16 * 256 * 4;   // 144 KiB
struct RadixView { unsigned short* idx[2]; unsigned short* hist; unsigned int* key_lds; };   // hist: [16 waves][2^digit bits] 16-bit counts / positions
static __device__ __forceinline__ RadixView radix_view(unsigned char* raw, const bool big) {
    RadixView v;
    v.key_lds = reinterpret_cast<unsigned int*>(raw);
    v.idx[0] = reinterpret_cast<unsigned short*>(raw + (big ? 0 : kSortLds * 4));
    v.idx[1] = v.idx[0] + (big ? kRadixBig : kSortLds);
    v.hist = reinterpret_cast<unsigned short*>(raw + 2 * kRadixBig * 2);
    return v;
}

// One pass structure for 8- and 9-bit digits (DB): 9 bits when that saves a pass (a 25-bit voxel index: 3 passes instead of 4, a
// ninth ballot per round of 64 keys); the counts of a wave's chunk (<= 2048 keys) and the positions (< 32768) fit 16 bits, so
// 16 waves x 512 digits still are 16 KiB.
template <int DB, typename KeyF>
static __device__ __forceinline__ const unsigned short* wg_radix_passes(const RadixView& m, const int n, const int bits, int* s_wave /*[32]*/, KeyF&& key_of) {
    constexpr int ND = 1 << DB, E = ND / 64;                      // digits; (digit, wave) entries a thread owns in the prefix
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = ((n + 1023) >> 10) << 6;                         // chunk of a wave: a multiple of 64, 16 chunks cover n
    unsigned short* hist = m.hist;
    for (int i = tid; i < n; i += kWG) m.idx[0][i] = (unsigned short)i;
    int cur = 0;
    for (int shift = 0; shift < bits; shift += DB) {
        const unsigned short* in = m.idx[cur];
        unsigned short* out = m.idx[cur ^ 1];
        for (int d = lane; d < ND; d += 64) hist[wave * ND + d] = 0;
        __syncthreads();                                             // (the indices of the previous pass are written)
        for (int walk = 0; walk < 2; ++walk) {
            for (int r = 0; r < C; r += 64) {
                const int i = wave * C + r + lane;
                const bool active = i < n;
                const unsigned int id = active ? in[i] : 0;
                const unsigned int d = active ? (key_of(id) >> shift) & (unsigned int)(ND - 1) : 0;
                unsigned long long peers = __ballot(active);
#pragma unroll
                for (int b = 0; b < DB; ++b) {
                    const unsigned long long bb = __ballot(active && ((d >> b) & 1u));
                    peers &= ((d >> b) & 1u) ? bb : ~bb;
                }
                const int cnt = __popcll(peers), rank = __popcll(peers & ((1ull << lane) - 1ull));
                if (walk == 0) {
                    if (active && rank == 0) hist[wave * ND + d] = (unsigned short)(hist[wave * ND + d] + cnt);
                } else {
                    unsigned int base = 0;
                    if (active) base = hist[wave * ND + d];
                    if (active) out[base + rank] = (unsigned short)id;
                    if (active && rank == 0) hist[wave * ND + d] = (unsigned short)(base + cnt);
                }
            }
            if (walk == 0) {
                // exclusive prefix over (digit, wave), digit-major: thread t owns the E consecutive entries from t * E
                __syncthreads();
                const int d = (tid * E) >> 4, w0 = (tid * E) & 15;
                unsigned int c[E], sum = 0;
#pragma unroll
                for (int q = 0; q < E; ++q) { c[q] = hist[(w0 + q) * ND + d]; sum += c[q]; }
                unsigned int incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                if (lane == 63) s_wave[wave] = (int)incl;
                __syncthreads();
                unsigned int base = incl - sum;
                for (int w = 0; w < wave; ++w) base += (unsigned int)s_wave[w];
#pragma unroll
                for (int q = 0; q < E; ++q) { hist[(w0 + q) * ND + d] = (unsigned short)base; base += c[q]; }
                __syncthreads();
            }
        }
        cur ^= 1;
    }
    __syncthreads();
    return m.idx[cur];
}
template <typename KeyF>
static __device__ __forceinline__ const unsigned short* wg_radix_sort(const RadixView& m, const int n, const int bits, int* s_wave /*[32]*/, KeyF&& key_of) {
    return (bits + 8) / 9 < (bits + 7) / 8 ? wg_radix_passes<9>(m, n, bits, s_wave, key_of) : wg_radix_passes<8>(m, n, bits, s_wave, key_of);
}

static __device__ __forceinline__ int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

static __device__ __forceinline__ int bits_for(long long vmax) {   // bits needed for values 0..vmax
    return vmax <= 0 ? 1 : 64 - __clzll((unsigned long long)vmax);
}

// ---------------------------------------------------------------------------------------------
// k_icp_voxel: open3d PointCloud::VoxelDownSample — mean per voxel, output in ascending
// (ix,iy,iz) order, the points of a voxel summed in input order.  key = voxel index | point index
// with just enough bits per field; one workgroup sorts its cloud (LDS up to 16k points).
// blockIdx.y: 0 = model cloud -> src (and tgt in verbatim mode, LL.cpp:109), 1 = scene cloud -> tgt.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWG)
k_icp_voxel(IcpBuffers B, int flags, double voxel) {
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[kRadixLdsBytes];   // radix layout, or 128 KiB of 64-bit keys (bitonic)
    unsigned long long* s_keys = reinterpret_cast<unsigned long long*>(s_raw);
    __shared__ int s_wave[32];
    __shared__ double s_part[16 * 6];
    __shared__ double s_mm[6];
    const int h = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
    IcpState& S = B.st[h];
    const bool scene_mode = (flags & 1) != 0;
    if (S.vox_done[which] == kIcpSortGroups) return;               // k_icp_voxel_wide did this cloud
    if (S.status != 0) {
        if (tid == 0) { if (which == 0) { S.n_src = 0; if (!scene_mode) S.n_tgt = 0; } else S.n_tgt = 0; }
        return;
    }
    const int n = which ? S.n_scene : S.n_model;
    const double* pts = (which ? B.scene_pts : B.model_pts) + (size_t)h * B.cap * 3;
    double* out = (which ? B.tgt : B.src) + (size_t)h * B.cap * 3;
    if (n == 0) {
        if (tid == 0) { if (which == 0) { S.n_src = 0; if (!scene_mode) S.n_tgt = 0; } else S.n_tgt = 0; }
        return;
    }
    const long long v_t0 = (long long)__builtin_amdgcn_s_memtime();
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int i = tid; i < n; i += kWG) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double v = pts[3 * (size_t)i + k]; mn[k] = fmin(mn[k], v); mx[k] = fmax(mx[k], v); }
    }
    block_minmax<3>(mn, mx, s_part, s_mm);
    const double mnx = s_mm[0] - voxel * 0.5, mny = s_mm[1] - voxel * 0.5, mnz = s_mm[2] - voxel * 0.5;
    const double fx = floor(__ddiv_rn(s_mm[3] - mnx, voxel)), fy = floor(__ddiv_rn(s_mm[4] - mny, voxel)),
                 fz = floor(__ddiv_rn(s_mm[5] - mnz, voxel));
    const bool finite = fx >= 0 && fx < 4e18 && fy >= 0 && fy < 4e18 && fz >= 0 && fz < 4e18;
    const int bx = finite ? bits_for((long long)fx) : 64, by = finite ? bits_for((long long)fy) : 64,
              bz = finite ? bits_for((long long)fz) : 64, bi = bits_for(n - 1);
    if (bx + by + bz + bi > 64) {
        if (tid == 0) S.status = 3;
        return;
    }
    const long long v_t1 = (long long)__builtin_amdgcn_s_memtime();
    const int npad = next_pow2(n < 2 ? 2 : n);
    const bool in_lds = npad <= kSortLds;
    const bool radix = n <= kRadixBig && bx + by + bz <= 32;       // voxel index in 32 bits: stable radix sort of the point indices
    const bool big = n > kSortLds;                                 // ... whose keys then stay in HBM
    const RadixView s_rx = radix_view(s_raw, big);
    unsigned long long* gk = B.keys + ((size_t)h * 2 + which) * B.cap2;
    unsigned int* gk32 = reinterpret_cast<unsigned int*>(gk);
    for (int i = tid; i < (radix ? n : npad); i += kWG) {
        unsigned long long key = ~0ull;
        if (i < n) {
            const unsigned long long ix = (unsigned long long)(long long)floor(__ddiv_rn(pts[3 * (size_t)i] - mnx, voxel));
            const unsigned long long iy = (unsigned long long)(long long)floor(__ddiv_rn(pts[3 * (size_t)i + 1] - mny, voxel));
            const unsigned long long iz = (unsigned long long)(long long)floor(__ddiv_rn(pts[3 * (size_t)i + 2] - mnz, voxel));
            key = (((ix << by) | iy) << bz | iz);
            if (!radix) key = (key << bi) | (unsigned long long)i;
        }
        if (radix) { if (big) gk32[i] = (unsigned int)key; else s_rx.key_lds[i] = (unsigned int)key; }
        else if (in_lds) s_keys[i] = key; else gk[i] = key;
    }
    __syncthreads();
    const long long v_t2 = (long long)__builtin_amdgcn_s_memtime();
    const unsigned short* order = nullptr;
    if (radix && big) order = wg_radix_sort(s_rx, n, bx + by + bz, s_wave, [&](unsigned int id) { return gk32[id]; });
    else if (radix) order = wg_radix_sort(s_rx, n, bx + by + bz, s_wave, [&](unsigned int id) { return s_rx.key_lds[id]; });
    else if (in_lds) bitonic_sort(s_keys, npad);
    else bitonic_sort_hybrid(gk, npad, s_keys);
    // sorted position -> (voxel index << bi) | point index, whichever way the list was sorted
    auto key_at = [&](int i) -> unsigned long long {
        if (radix) { const unsigned int id = order[i]; return ((unsigned long long)(big ? gk32[id] : s_rx.key_lds[id]) << bi) | id; }
        return in_lds ? s_keys[i] : gk[i];
    };
    const long long v_t3 = (long long)__builtin_amdgcn_s_memtime();
    const unsigned long long imask = (1ull << bi) - 1ull;
    int nout = 0;
    if (radix) {
        // the points of 1024 sorted positions are gathered into LDS side by side (the index buffer the sort left free), then
        // the first thread of every voxel adds its points up in input order — out of LDS, not one dependent HBM gather each
        unsigned short* spare = order == s_rx.idx[0] ? s_rx.idx[1] : s_rx.idx[0];
        double* st = reinterpret_cast<double*>(spare);                       // [kWG][3]
        unsigned int* sv = reinterpret_cast<unsigned int*>(st + 3 * kWG);    // [kWG] voxel index per position
        auto vox_of = [&](int i) -> unsigned int { const unsigned int id = order[i]; return big ? gk32[id] : s_rx.key_lds[id]; };
        for (int base = 0; base < n; base += kWG) {
            const int i = base + tid;
            unsigned int v = 0;
            if (i < n) {
                const unsigned int id = order[i];
                v = big ? gk32[id] : s_rx.key_lds[id];
                st[3 * tid] = pts[3 * (size_t)id]; st[3 * tid + 1] = pts[3 * (size_t)id + 1]; st[3 * tid + 2] = pts[3 * (size_t)id + 2];
                sv[tid] = v;
            }
            __syncthreads();
            const bool head = i < n && (i == 0 || (tid > 0 ? sv[tid - 1] : vox_of(i - 1)) != v);
            int tot;
            const int pos = nout + block_scan_flag(head, s_wave, tot);
            nout += tot;
            if (head) {
                double sx = 0, sy = 0, sz = 0;
                int cnt = 0;
                for (int j = i; j < n; ++j) {
                    const int t = j - base;
                    if (t < kWG) {
                        if (sv[t] != v) break;
                        sx += st[3 * t]; sy += st[3 * t + 1]; sz += st[3 * t + 2];
                    } else {                                             // the voxel runs on into the next 1024 positions
                        if (vox_of(j) != v) break;
                        const size_t idx = order[j];
                        sx += pts[3 * idx]; sy += pts[3 * idx + 1]; sz += pts[3 * idx + 2];
                    }
                    ++cnt;
                }
                const double c = (double)cnt;
                out[3 * (size_t)pos] = sx / c; out[3 * (size_t)pos + 1] = sy / c; out[3 * (size_t)pos + 2] = sz / c;
            }
            __syncthreads();
        }
    } else
    for (int base = 0; base < n; base += kWG) {
        const int i = base + tid;
        bool head = false;
        unsigned long long vox = 0;
        if (i < n) {
            const unsigned long long k = key_at(i);
            vox = k >> bi;
            head = i == 0 || (key_at(i - 1) >> bi) != vox;
        }
        int tot;
        const int pos = nout + block_scan_flag(head, s_wave, tot);
        nout += tot;
        if (head) {
            double sx = 0, sy = 0, sz = 0;
            int cnt = 0, j = i;
            for (;;) {
                const unsigned long long k = key_at(j);
                if ((k >> bi) != vox) break;
                const size_t idx = (size_t)(k & imask);
                sx += pts[3 * idx]; sy += pts[3 * idx + 1]; sz += pts[3 * idx + 2];
                ++cnt; ++j;
                if (j >= n) break;
            }
            const double c = (double)cnt;
            out[3 * (size_t)pos] = sx / c; out[3 * (size_t)pos + 1] = sy / c; out[3 * (size_t)pos + 2] = sz / c;
        }
    }
    if (tid == 0) {
        if (which == 0) { S.n_src = nout; if (!scene_mode) S.n_tgt = nout; }
        else S.n_tgt = nout;
        if (which == 0) {                                          // diagnostics (model cloud): cycles for extent, keys, sort, voxel means
            const long long v_t4 = (long long)__builtin_amdgcn_s_memtime();
            S.vox_clk[0] = v_t1 - v_t0; S.vox_clk[1] = v_t2 - v_t1; S.vox_clk[2] = v_t3 - v_t2; S.vox_clk[3] = v_t4 - v_t3;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_icp_grid: the target cloud binned into xy columns (cell edge >= 5 mm, <= 64 x 64 columns) and, inside
// a column, ordered by quantised depth (>= 1 mm steps): points sorted by (x column, y column, z step,
// original index).  A search visits one run per column and finds the depth range it needs by bisection,
// so the table stays a few thousand entries however deep the cloud is (a scene cloud carries background
// far behind the object); an x slab of columns is one contiguous range of cells and of points (what a
// source slice stages in LDS).  cell_start[c] = first sorted position of column c.
// ---------------------------------------------------------------------------------------------
constexpr int kZBits = 20;         // quantised-depth bits of the grid sort key

__global__ void __launch_bounds__(kWG)
k_icp_grid(IcpBuffers B, int flags) {
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[kRadixLdsBytes];   // radix layout, or 128 KiB of 64-bit keys (bitonic)
    unsigned long long* s_keys = reinterpret_cast<unsigned long long*>(s_raw);
    __shared__ int s_wave[32];
    __shared__ double s_part[16 * 6];
    __shared__ double s_mm[6];
    const int h = blockIdx.x, tid = threadIdx.x;
    IcpState& S = B.st[h];
    if (S.grid_done == kIcpSortGroups) return;                     // k_icp_grid_wide did this cloud
    if (tid == 0 && S.status == 0) {                               // init_guess: centroid difference (LL.cpp:91-104), strips added in order
        double t[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < kIcpStrips; ++k)
            for (int q = 0; q < 7; ++q) t[q] += B.strip_sum[((size_t)h * kIcpStrips + k) * 8 + q];
        const double n = (double)S.n_model;
        S.init[0] = t[3] / t[6] - t[0] / n;      // NaN when no scene point is near the anchor, as the reference
        S.init[1] = t[4] / t[6] - t[1] / n;
        S.init[2] = t[5] / t[6] - t[2] / n;
    }
    int* cs = B.cell_start + (size_t)h * kIcpCells;
    const int nt = S.status == 0 ? S.n_tgt : 0;
    if (nt == 0 || nt >= (1 << kIdxBits)) {
        if (tid == 0) {
            if (nt > 0) { S.status = 3; S.n_tgt = 0; }
            S.gx = 1; S.gy = 1; S.zq_max = 0; S.gminx = 0; S.gminy = 0; S.gminz = 0; S.cell = kCellMin; S.inv_cell = 1.0 / kCellMin; S.inv_z = 1e4;
            cs[0] = 0; cs[1] = 0;
        }
        return;
    }
    const double* T = ((flags & 1) ? B.tgt : B.src) + (size_t)h * B.cap * 3;
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int i = tid; i < nt; i += kWG) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double v = T[3 * (size_t)i + k]; mn[k] = fmin(mn[k], v); mx[k] = fmax(mx[k], v); }
    }
    block_minmax<3>(mn, mx, s_part, s_mm);
    const double minx = s_mm[0], miny = s_mm[1], minz = s_mm[2];
    const double ext = fmax(s_mm[3] - minx, s_mm[4] - miny), extz = s_mm[5] - minz;
    double cell = ext / (double)kIcpGrid;
    if (!(cell > kCellMin)) cell = kCellMin;                       // also catches NaN
    double zres = extz / (double)((1 << kZBits) - 1);
    if (!(zres > 1e-3)) zres = 1e-3;                               // 1 mm steps: a metre of depth is 10 bits, so the sort key (column, step) is 3 radix passes, not 4
    const double inv = 1.0 / cell, inv_z = 1.0 / zres;
    if (!(ext < 1e30) || !(extz < 1e30)) {                         // non-finite coordinates
        if (tid == 0) { S.status = 3; S.n_tgt = 0; S.gx = 1; S.gy = 1; S.zq_max = 0; cs[0] = 0; cs[1] = 0; }
        return;
    }
    const int gx = grid_coord(s_mm[3], minx, inv, kIcpGrid) + 1, gy = grid_coord(s_mm[4], miny, inv, kIcpGrid) + 1;
    const int zq_max = zq_of(s_mm[5], minz, inv_z, (1 << kZBits) - 1);
    const int npad = next_pow2(nt < 2 ? 2 : nt);
    const bool radix = nt <= kRadixBig;                            // (column, depth step) is 32 bits: stable radix sort of the point indices
    const bool big = nt > kSortLds;                                // ... whose keys then stay in HBM
    const RadixView s_rx = radix_view(s_raw, big);
    const int cell_bits = bits_for((long long)gx * gy - 1), z_bits = bits_for(zq_max);
    unsigned long long* gk = B.keys + (size_t)h * 2 * B.cap2;
    unsigned int* gk32 = reinterpret_cast<unsigned int*>(gk);
    for (int i = tid; i < (radix ? nt : npad); i += kWG) {
        unsigned long long key = ~0ull;
        if (i < nt) {
            const int cx = grid_coord(T[3 * (size_t)i], minx, inv, gx), cy = grid_coord(T[3 * (size_t)i + 1], miny, inv, gy);
            const int zq = zq_of(T[3 * (size_t)i + 2], minz, inv_z, zq_max);
            if (radix) key = ((unsigned long long)(cx * gy + cy) << z_bits) | (unsigned long long)zq;
            else key = ((((unsigned long long)(cx * gy + cy) << kZBits) | (unsigned long long)zq) << kIdxBits) | (unsigned long long)i;
        }
        if (radix) { if (big) gk32[i] = (unsigned int)key; else s_rx.key_lds[i] = (unsigned int)key; }
        else gk[i] = key;
    }
    __syncthreads();
    const unsigned short* order = nullptr;
    if (radix && big) order = wg_radix_sort(s_rx, nt, cell_bits + z_bits, s_wave, [&](unsigned int id) { return gk32[id]; });
    else if (radix) order = wg_radix_sort(s_rx, nt, cell_bits + z_bits, s_wave, [&](unsigned int id) { return s_rx.key_lds[id]; });
    else bitonic_sort_hybrid(gk, npad, s_keys);
    // sorted position -> ((column << kZBits | depth step) << kIdxBits) | point index, whichever way the list was sorted
    auto key_at = [&](int i) -> unsigned long long {
        if (radix) {
            const unsigned int id = order[i], k32 = big ? gk32[id] : s_rx.key_lds[id];
            return ((((unsigned long long)(k32 >> z_bits) << kZBits) | (unsigned long long)(k32 & ((1u << z_bits) - 1u))) << kIdxBits) | id;
        }
        return gk[i];
    };
    double* Ts = B.tgt_sorted + (size_t)h * B.cap * 3;
    int* orig = B.tgt_orig + (size_t)h * B.cap;
    TgtRec* rec = B.tgt_rec + (size_t)h * B.cap;
    unsigned short* cs16 = B.cell_start16 + (size_t)h * kIcpCells16;
    for (int p = tid; p < nt; p += kWG) {
        const unsigned long long k = key_at(p);
        const size_t i = (size_t)(k & ((1ull << kIdxBits) - 1ull));
        Ts[3 * (size_t)p] = T[3 * i]; Ts[3 * (size_t)p + 1] = T[3 * i + 1]; Ts[3 * (size_t)p + 2] = T[3 * i + 2];
        orig[p] = (int)i;
        TgtRec r;
        r.x = T[3 * i]; r.y = T[3 * i + 1]; r.z = T[3 * i + 2]; r.orig = (int)i;
        r.zq = (int)((k >> kIdxBits) & ((1ull << kZBits) - 1ull));
        rec[p] = r;
    }
    const int ncell = gx * gy;
    for (int c = tid; c <= ncell; c += kWG) {                       // lower_bound of the column's smallest key
        const unsigned long long want = (unsigned long long)c << (kZBits + kIdxBits);
        int lo = 0, hi = nt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const unsigned long long k = key_at(mid);
            if (k < want) lo = mid + 1; else hi = mid;
        }
        cs[c] = lo;
        cs16[c] = (unsigned short)lo;
    }
    if (tid == 0) {
        S.gx = gx; S.gy = gy; S.zq_max = zq_max; S.gminx = minx; S.gminy = miny; S.gminz = minz; S.cell = cell; S.inv_cell = inv;
        S.inv_z = inv_z;
    }
}

// ---------------------------------------------------------------------------------------------
// The two sorts above, spread over the chip (round 6).  One workgroup sorting a cloud of 12-17k points took 120-200 us with 15 of 16 CUs
// of the hypothesis' share idle.  k_icp_voxel_wide / k_icp_grid_wide give a cloud kIcpSortGroups workgroups, each a contiguous range of
// the LEADING coordinate of the sort key (voxel index ix, grid column cx: equal shares of its span):
//   a group walks the x coordinates of the whole cloud — every wave a contiguous piece: count, prefix over the waves, second walk — and
//   takes the points of its range in input order with the key relative to its range; the cloud's extent comes from the strips of
//   k_icp_points, not from a scan;
//   it orders them in LDS (group_sort: the keys are (column, depth) with a handful of points per column: count per column, prefix, rank
//   inside the column; the radix passes above only when a column is crowded);
//   the grid group then writes its part of the sorted cloud (its first position = the points below its range, counted on the way) and the
//   starts of its columns; the voxel group needs the number of voxels of the groups before it, which every group publishes as soon as its
//   order stands (one agent-scope word each; a group waits only for lower block indices, which were dispatched before it).
// The voxel means are those of k_icp_voxel bit for bit (same keys, stable order, the points of a voxel added up in input order); the grid
// spans the extent of the cloud the target was down-sampled FROM (a bound of the means' extent that costs no scan).  The one-workgroup
// kernels stay behind them for the clouds they leave: voxel index beyond 32 bits, a group of more than kGroupCap points, empty or rejected
// hypotheses — IcpState::vox_done / grid_done say which.
// ---------------------------------------------------------------------------------------------
constexpr int kGroupCap = 8192;     // points a group sorts (LDS: keys 32 KiB, point indices 32 KiB, two index lists 32 KiB, digit counts 16 KiB)
constexpr unsigned int kLookFail = 0xFFFFFFFFu;
constexpr long long kLookTimeout = 100ll * 100000;   // wall_clock64 ticks: 100 ms

// Extent of one of the two back-projected clouds of a hypothesis from its strips; all threads of wave 0 call it, result in s_mm[6] (after a barrier).
static __device__ __forceinline__ void strips_extent(const double* __restrict__ strip_mm /*[kIcpStrips][12]*/, const int which, double* s_mm) {
    const int lane = threadIdx.x & 63;
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    if (lane < kIcpStrips) {
        const double* p = strip_mm + (size_t)lane * 12 + which * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = p[k]; mx[k] = p[3 + k]; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[k] = fmin(mn[k], shfl_xor_d(mn[k], o)); mx[k] = fmax(mx[k], shfl_xor_d(mx[k], o)); }
    if (lane == 0) { s_mm[0] = mn[0]; s_mm[1] = mn[1]; s_mm[2] = mn[2]; s_mm[3] = mx[0]; s_mm[4] = mx[1]; s_mm[5] = mx[2]; }
}

// floor(a / v) as the one-workgroup kernels compute it (IEEE division, then floor), without the division where the answer cannot depend on it:
// a * (1 / v) is within 2^-52 of a / v relatively, so below 2^32 and further than 1e-6 from an integer both floor alike.
static __device__ __forceinline__ long long floor_quotient(const double a, const double v, const double inv_v) {
    const double q = a * inv_v, f = floor(q), d = q - f;
    if (!(d > 1e-6 && d < 1.0 - 1e-6)) return (long long)floor(__ddiv_rn(a, v));
    return (long long)f;
}

// A wave's piece of a cloud of n points in group_collect: positions [i0, i1), a multiple of 64 long, 16 pieces cover n.
static __device__ __forceinline__ void collect_piece(const int n, int& i0, int& i1) {
    const int piece = (((n + 15) >> 4) + 63) & ~63;
    i0 = (int)(threadIdx.x >> 6) * piece; i1 = min(n, i0 + piece);
}

// The points whose leading coordinate lead(x) lies in [lo, hi), in input order: key_of(lead, y, z) -> s_key[j], i -> s_gid[j].  Returns their
// number (nothing is written when it exceeds kGroupCap) and the number of points below lo.  Every wave walks the x coordinates of its piece
// twice (count, prefix over the waves, take), four rounds of 64 points at a time so that their loads are in flight together; x0 = the x
// coordinates of the first four rounds, which the caller loaded before it knew the cloud's extent; then the keys of the taken points, spread
// over all threads.  1024 threads; s_wave: 32 ints.
template <typename LoadF, typename LeadF, typename KeyF>
static __device__ __forceinline__ int group_collect(const int n, const long long lo, const long long hi, unsigned int* s_key, unsigned int* s_gid, int* s_wave,
                                                    int& below_out, const double (&x0)[4], LoadF&& load, LeadF&& lead, KeyF&& key_of, long long* tick = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int i0, i1;
    collect_piece(n, i0, i1);
    int mine = 0, below = 0;
    long long v0[4];
    auto leads = [&](const int r0, const double (&x)[4], long long (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = r0 + 64 * u + lane < i1 ? lead(x[u]) : hi;      // (hi: neither below nor inside)
    };
    auto fetch = [&](const int r0, double (&x)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = r0 + 64 * u + lane; x[u] = i < i1 ? load(i, 0) : 0.0; }
    };
    auto count = [&](const long long (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { below += v[u] < lo ? 1 : 0; mine += (v[u] >= lo && v[u] < hi) ? 1 : 0; }
    };
    leads(i0, x0, v0);
    count(v0);
    for (int r0 = i0 + 256; r0 < i1; r0 += 256) {
        double x[4]; long long v[4];
        fetch(r0, x); leads(r0, x, v); count(v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mine += __shfl_xor(mine, o, 64); below += __shfl_xor(below, o, 64); }
    __syncthreads();
    if (lane == 0) { s_wave[wave] = mine; s_wave[16 + wave] = below; }
    __syncthreads();
    int base = 0, m = 0, nb = 0;
    for (int w = 0; w < 16; ++w) { const int c = s_wave[w]; if (w < wave) base += c; m += c; nb += s_wave[16 + w]; }
    below_out = nb;
    if (tick) tick[0] = (long long)__builtin_amdgcn_s_memtime();
    if (m > kGroupCap) return m;
    auto take = [&](const int r0, const long long (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = v[u] >= lo && v[u] < hi;
            const unsigned long long b = __ballot(in);
            if (in) { const int j = base + __popcll(b & ((1ull << lane) - 1ull)); s_key[j] = (unsigned int)(v[u] - lo); s_gid[j] = (unsigned int)(r0 + 64 * u + lane); }
            base += __popcll(b);
        }
    };
    if (i0 < i1) {
        take(i0, v0);
        for (int r0 = i0 + 256; r0 < i1; r0 += 256) {
            double x[4]; long long v[4];
            fetch(r0, x); leads(r0, x, v); take(r0, v);
        }
    }
    __syncthreads();
    if (tick) tick[1] = (long long)__builtin_amdgcn_s_memtime();
    // the keys, one taken point per thread (a wave's 64 points of an image row hold a few points of every group: in the walk above seven
    // of eight lanes would compute keys nobody needs)
    for (int j = tid; j < m; j += kWG) {
        const int i = (int)s_gid[j];
        const double y = load(i, 1), z = load(i, 2);
        s_key[j] = key_of(lo + (long long)s_key[j], y, z);
    }
    __syncthreads();
    return m;
}

// Stable order of the m <= kGroupCap keys s_key[0..m) of `bits` bits: order[r] = index of the r-th.  The keys are (column, depth) with a
// handful of points per column, so: count the points of every column (key >> zb, at most 4096 columns: LDS atomics, which also hand every
// point a slot in its column), prefix the counts, drop the points into their columns, and rank every point among the ones that share its
// column by (key, input position) — four barriers, where a radix pass over the same keys has five and the key needs two or three.
// col_start (if not null): set to the columns' starts when that path was taken (start[c], c < 1 << (bits - zb)), else to null: columns with more
// than kColumnMax points, or more than 4096 columns, go through the radix passes.  s_idx: 2 x kGroupCap, s_cnt: 16 KiB.
constexpr int kColumnMax = 64;
static __device__ __forceinline__ const unsigned short* group_sort(const unsigned int* s_key, const int m, const int bits, int zb, unsigned short* s_idx, unsigned short* s_cnt,
                                                                   int* s_wave, const unsigned int** col_start) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (zb < bits - 12) zb = bits - 12;
    if (zb > bits) zb = bits;
    const int ncol = 1 << (bits - zb);
    unsigned int* cnt = reinterpret_cast<unsigned int*>(s_cnt);   // [4096]: counts, then starts
    unsigned short* slot = s_idx + kGroupCap;                      // a point's slot in its column (until the points are dropped), then the order
    unsigned short* tmp = s_idx;                                   // the points column by column, unordered inside
    for (int c = tid; c < ncol; c += kWG) cnt[c] = 0;
    __syncthreads();
    for (int j = tid; j < m; j += kWG) slot[j] = (unsigned short)atomicAdd(&cnt[s_key[j] >> zb], 1u);
    __syncthreads();
    {   // exclusive prefix of the counts in place: thread t owns columns [4t, 4t + 4); largest count on the way
        unsigned int c[4], sum = 0, big = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = 4 * tid + q < ncol ? cnt[4 * tid + q] : 0; sum += c[q]; big = max(big, c[q]); }
        unsigned int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) big = max(big, (unsigned int)__shfl_xor((int)big, o, 64));
        if (lane == 63) { s_wave[wave] = (int)incl; s_wave[16 + wave] = (int)big; }
        __syncthreads();
        unsigned int base = incl - sum, worst = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) base += (unsigned int)s_wave[w]; worst = max(worst, (unsigned int)s_wave[16 + w]); }
        if (worst > (unsigned int)kColumnMax) {                     // (every thread alike)
            __syncthreads();
            if (col_start) *col_start = nullptr;
            RadixView rx;
            rx.key_lds = const_cast<unsigned int*>(s_key); rx.idx[0] = s_idx; rx.idx[1] = s_idx + kGroupCap; rx.hist = s_cnt;
            return wg_radix_sort(rx, m, bits, s_wave, [&](unsigned int id) { return s_key[id]; });
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { if (4 * tid + q < ncol) cnt[4 * tid + q] = base; base += c[q]; }
    }
    __syncthreads();
    for (int j = tid; j < m; j += kWG) tmp[cnt[s_key[j] >> zb] + slot[j]] = (unsigned short)j;
    __syncthreads();
    for (int j = tid; j < m; j += kWG) {
        const unsigned int k = s_key[j], col = k >> zb;
        const int a = (int)cnt[col], b = (int)col + 1 < ncol ? (int)cnt[col + 1] : m;
        int rank = 0;
        for (int q = a; q < b; ++q) {
            const int jj = tmp[q];
            const unsigned int kk = s_key[jj];
            rank += (kk < k || (kk == k && jj < j)) ? 1 : 0;
        }
        slot[a + rank] = (unsigned short)j;
    }
    __syncthreads();
    if (col_start) *col_start = cnt;
    return slot;
}

__global__ void __launch_bounds__(kWG)
k_icp_voxel_wide(IcpBuffers B, int flags, double voxel) {
    __shared__ __attribute__((aligned(16))) unsigned int s_key[kGroupCap];
    __shared__ __attribute__((aligned(16))) unsigned int s_gid[kGroupCap];
    __shared__ __attribute__((aligned(16))) unsigned short s_idx[2 * kGroupCap];
    __shared__ __attribute__((aligned(16))) unsigned short s_cnt[16 * 512];
    __shared__ __attribute__((aligned(16))) double s_st[3 * kWG];
    __shared__ unsigned int s_sv[kWG];
    __shared__ int s_wave[32];
    __shared__ double s_mm[6];
    __shared__ int s_nv, s_base;
    const int g = blockIdx.x, h = blockIdx.y, which = blockIdx.z, tid = threadIdx.x;
    const int cloud = h * 2 + which;
    IcpState& S = B.st[h];
    const bool scene_mode = (flags & 1) != 0;
    if (g == 0 && which == 0 && tid < kIcpStrips) B.strip_pub[(size_t)h * kIcpStrips + tid] = 0;   // (k_icp_points_fused is through: its strips' counts are the next run's to publish)
    const int n = S.status == 0 ? (which ? S.n_scene : S.n_model) : 0;
    if (n == 0) return;                                            // (k_icp_voxel sets the counts of these)
    long long clk[6];
    clk[0] = (long long)__builtin_amdgcn_s_memtime();
    unsigned int* look = B.sort_look + (size_t)cloud * kIcpSortGroups;
    const double* pts = (which ? B.scene_pts : B.model_pts) + (size_t)h * B.cap * 3;
    double x0[4];                                                  // (on their way while the extent is worked out)
    {
        int i0, i1;
        collect_piece(n, i0, i1);
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + 64 * u + (tid & 63); x0[u] = i < i1 ? pts[3 * (size_t)i] : 0.0; }
    }
    if (tid < 64) {
        strips_extent(B.strip_mm + (size_t)h * kIcpStrips * 12, which, s_mm);
        if (tid == 0) {                                            // the arithmetic of k_icp_voxel (one lane: sixteen waves dividing alike is a thousand cycles of the SIMDs)
            const double mnx = s_mm[0] - voxel * 0.5, mny = s_mm[1] - voxel * 0.5, mnz = s_mm[2] - voxel * 0.5;
            const double fx = floor(__ddiv_rn(s_mm[3] - mnx, voxel)), fy = floor(__ddiv_rn(s_mm[4] - mny, voxel)),
                         fz = floor(__ddiv_rn(s_mm[5] - mnz, voxel));
            s_mm[0] = mnx; s_mm[1] = mny; s_mm[2] = mnz; s_mm[3] = fx; s_mm[4] = fy; s_mm[5] = fz;
        }
    }
    if (tid == 64) s_nv = 0;
    __syncthreads();
    const double mnx = s_mm[0], mny = s_mm[1], mnz = s_mm[2], fx = s_mm[3], fy = s_mm[4], fz = s_mm[5];
    const double inv_voxel = 1.0 / voxel;
    const bool finite = fx >= 0 && fx < 4e18 && fy >= 0 && fy < 4e18 && fz >= 0 && fz < 4e18;
    const int bx = finite ? bits_for((long long)fx) : 64, by = finite ? bits_for((long long)fy) : 64, bz = finite ? bits_for((long long)fz) : 64;
    if (bx + by + bz > 32) return;                                 // every group alike: the cloud is k_icp_voxel's
    const long long span = (long long)fx + 1;                      // ix = 0 .. fx
    const long long lo = span * g / kIcpSortGroups, hi = span * (g + 1) / kIcpSortGroups;
    const int bits = (hi > lo ? bits_for(hi - lo - 1) : 1) + by + bz;
    double* out = (which ? B.tgt : B.src) + (size_t)h * B.cap * 3;
    int below;
    const int m = group_collect(n, lo, hi, s_key, s_gid, s_wave, below, x0,
        [&](int i, int k) { return pts[3 * (size_t)i + k]; },
        [&](double x) { return floor_quotient(x - mnx, voxel, inv_voxel); },
        [&](long long ix, double y, double z) {
            const unsigned long long iy = (unsigned long long)floor_quotient(y - mny, voxel, inv_voxel);
            const unsigned long long iz = (unsigned long long)floor_quotient(z - mnz, voxel, inv_voxel);
            return (unsigned int)(((((unsigned long long)(ix - lo)) << by) | iy) << bz | iz);
        });
    clk[1] = (long long)__builtin_amdgcn_s_memtime();
    if (m > kGroupCap) {                                           // the groups behind must not wait for this one
        if (tid == 0) __hip_atomic_store(look + g, kLookFail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const unsigned short* order = m > 0 ? group_sort(s_key, m, bits, bz, s_idx, s_cnt, s_wave, nullptr) : s_idx;
    clk[2] = (long long)__builtin_amdgcn_s_memtime();
    // voxels of this group: published before the means are taken, so that the groups behind find it there
    {
        int heads = 0;
        for (int i = tid; i < m; i += kWG) heads += (i == 0 || s_key[order[i - 1]] != s_key[order[i]]) ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) heads += __shfl_xor(heads, o, 64);
        if ((tid & 63) == 0 && heads) atomicAdd(&s_nv, heads);
    }
    __syncthreads();
    const int nv = s_nv;
    if (tid == 0) __hip_atomic_store(look + g, (unsigned int)nv + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
        unsigned int v = 1;
        if (tid < g) {
            const long long t0 = wall_clock64();
            do { v = __hip_atomic_load(look + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (v == 0 && wall_clock64() - t0 < kLookTimeout);
        }
        const bool lost = __ballot(v == 0 || v == kLookFail) != 0ull;
        int before = (int)v - 1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
        if (tid == 0) s_base = lost ? -1 : before;
    }
    __syncthreads();
    const int base_out = s_base;
    clk[3] = (long long)__builtin_amdgcn_s_memtime();
    if (base_out < 0) {                                            // a group before this one gave up or never came: the cloud is k_icp_voxel's
        if (tid == 0) __hip_atomic_store(look + g, kLookFail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    int nout = base_out;
    auto vox_of = [&](int i) -> unsigned int { return s_key[order[i]]; };
    for (int base = 0; base < m; base += kWG) {                     // as k_icp_voxel: 1024 sorted positions side by side in LDS, the first thread of a voxel adds them up in input order
        const int i = base + tid;
        unsigned int v = 0;
        if (i < m) {
            const unsigned int id = order[i];
            v = s_key[id];
            const size_t p = s_gid[id];
            s_st[3 * tid] = pts[3 * p]; s_st[3 * tid + 1] = pts[3 * p + 1]; s_st[3 * tid + 2] = pts[3 * p + 2];
            s_sv[tid] = v;
        }
        __syncthreads();
        const bool head = i < m && (i == 0 || (tid > 0 ? s_sv[tid - 1] : vox_of(i - 1)) != v);
        int tot;
        const int pos = nout + block_scan_flag(head, s_wave, tot);
        nout += tot;
        if (head) {
            double sx = 0, sy = 0, sz = 0;
            int cnt = 0;
            for (int j = i; j < m; ++j) {
                const int t = j - base;
                if (t < kWG) {
                    if (s_sv[t] != v) break;
                    sx += s_st[3 * t]; sy += s_st[3 * t + 1]; sz += s_st[3 * t + 2];
                } else {
                    if (vox_of(j) != v) break;
                    const size_t p = s_gid[order[j]];
                    sx += pts[3 * p]; sy += pts[3 * p + 1]; sz += pts[3 * p + 2];
                }
                ++cnt;
            }
            const double cd = (double)cnt;
            out[3 * (size_t)pos] = sx / cd; out[3 * (size_t)pos + 1] = sy / cd; out[3 * (size_t)pos + 2] = sz / cd;
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (g == kIcpSortGroups - 1) {
            if (which == 0) { S.n_src = nout; if (!scene_mode) S.n_tgt = nout; }
            else S.n_tgt = nout;
        }
        atomicAdd(&S.vox_done[which], 1);
        if (which == 0) {
            clk[4] = (long long)__builtin_amdgcn_s_memtime();
            for (int k = 0; k < 4; ++k) atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[k]), (unsigned long long)(clk[k + 1] - clk[k]));
            atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[6]), (unsigned long long)m);
        }
    }
}

__global__ void __launch_bounds__(kWG)
k_icp_grid_wide(IcpBuffers B, int flags) {
    __shared__ __attribute__((aligned(16))) unsigned int s_key[kGroupCap];
    __shared__ __attribute__((aligned(16))) unsigned int s_gid[kGroupCap];
    __shared__ __attribute__((aligned(16))) unsigned short s_idx[2 * kGroupCap];
    __shared__ __attribute__((aligned(16))) unsigned short s_cnt[16 * 512];
    __shared__ int s_wave[32];
    __shared__ double s_mm[6], s_par[3];
    __shared__ int s_geo[3];
    const int g = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    IcpState& S = B.st[h];
    if (S.status != 0) return;
    long long clk[5];
    clk[0] = (long long)__builtin_amdgcn_s_memtime();
    const int which = (flags & 1) ? 1 : 0;
    if (g == 0 && tid >= 64 && tid < 128) {                        // init_guess: centroid difference (LL.cpp:91-104), strips added in order (as k_icp_grid)
        double v[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) v[q] = lane < kIcpStrips ? B.strip_sum[((size_t)h * kIcpStrips + lane) * 8 + q] : 0.0;
        double t[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < kIcpStrips; ++k)
#pragma unroll
            for (int q = 0; q < 7; ++q) t[q] += __shfl(v[q], k, 64);
        if (lane == 0) {
            const double n = (double)S.n_model;
            S.init[0] = t[3] / t[6] - t[0] / n;
            S.init[1] = t[4] / t[6] - t[1] / n;
            S.init[2] = t[5] / t[6] - t[2] / n;
        }
    }
    const int nt = S.n_tgt;
    if (nt == 0 || nt >= (1 << kIdxBits)) return;                  // (k_icp_grid sets the state of these)
    const double* T = (which ? B.tgt : B.src) + (size_t)h * B.cap * 3;
    double x0[4];                                                  // (on their way while the extent is worked out)
    {
        int i0, i1;
        collect_piece(nt, i0, i1);
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + 64 * u + lane; x0[u] = i < i1 ? T[3 * (size_t)i] : 0.0; }
    }
    if (tid < 64) {
        strips_extent(B.strip_mm + (size_t)h * kIcpStrips * 12, which, s_mm);
        if (tid == 0) {                                            // the arithmetic of k_icp_grid, on the extent of the cloud the target was down-sampled from (one lane)
            const double minx = s_mm[0], miny = s_mm[1], minz = s_mm[2];
            const double ext = fmax(s_mm[3] - minx, s_mm[4] - miny), extz = s_mm[5] - minz;
            double cell = ext / (double)kIcpGrid;
            if (!(cell > kCellMin)) cell = kCellMin;
            double zres = extz / (double)((1 << kZBits) - 1);
            if (!(zres > 1e-3)) zres = 1e-3;
            const double inv = 1.0 / cell, inv_z = 1.0 / zres;
            const bool ok = ext < 1e30 && extz < 1e30;
            s_par[0] = cell; s_par[1] = inv; s_par[2] = inv_z;
            s_geo[0] = ok ? grid_coord(s_mm[3], minx, inv, kIcpGrid) + 1 : 0;
            s_geo[1] = ok ? grid_coord(s_mm[4], miny, inv, kIcpGrid) + 1 : 0;
            s_geo[2] = ok ? zq_of(s_mm[5], minz, inv_z, (1 << kZBits) - 1) : 0;
        }
    }
    __syncthreads();
    const double minx = s_mm[0], miny = s_mm[1], minz = s_mm[2], cell = s_par[0], inv = s_par[1], inv_z = s_par[2];
    const int gx = s_geo[0], gy = s_geo[1], zq_max = s_geo[2];
    if (gx == 0) return;                                           // non-finite coordinates: k_icp_grid rejects the hypothesis
    long long tick[3];
    tick[0] = (long long)__builtin_amdgcn_s_memtime();
    const int z_bits = bits_for(zq_max);
    const int lo = gx * g / kIcpSortGroups, hi = gx * (g + 1) / kIcpSortGroups;      // x columns of this group
    const int bits = (hi > lo ? bits_for((long long)(hi - lo) * gy - 1) : 1) + z_bits;
    int p0;
    const int m = group_collect(nt, lo, hi, s_key, s_gid, s_wave, p0, x0,
        [&](int i, int k) { return T[3 * (size_t)i + k]; },
        [&](double x) { return (long long)grid_coord(x, minx, inv, gx); },
        [&](long long cx, double y, double z) {
            const int cy = grid_coord(y, miny, inv, gy), zq = zq_of(z, minz, inv_z, zq_max);
            return ((unsigned int)(((int)cx - lo) * gy + cy) << z_bits) | (unsigned int)zq;
        }, tick + 1);
    clk[1] = (long long)__builtin_amdgcn_s_memtime();
    if (m > kGroupCap) return;                                     // grid_done stays short: k_icp_grid does the cloud
    const unsigned int* col_start = nullptr;
    const unsigned short* order = m > 0 ? group_sort(s_key, m, bits, z_bits, s_idx, s_cnt, s_wave, &col_start) : s_idx;
    if (bits - z_bits > 12) col_start = nullptr;                   // (the columns of the sort were coarser than the grid's)
    clk[2] = (long long)__builtin_amdgcn_s_memtime();
    double* Ts = B.tgt_sorted + (size_t)h * B.cap * 3;
    int* orig = B.tgt_orig + (size_t)h * B.cap;
    TgtRec* rec = B.tgt_rec + (size_t)h * B.cap;
    int* cs = B.cell_start + (size_t)h * kIcpCells;
    unsigned short* cs16 = B.cell_start16 + (size_t)h * kIcpCells16;
    for (int j = tid; j < m; j += kWG) {
        const unsigned int id = order[j];
        const size_t i = s_gid[id], p = (size_t)p0 + j;
        TgtRec r;
        r.x = T[3 * i]; r.y = T[3 * i + 1]; r.z = T[3 * i + 2]; r.orig = (int)i;
        r.zq = (int)(s_key[id] & ((1u << z_bits) - 1u));
        Ts[3 * p] = r.x; Ts[3 * p + 1] = r.y; Ts[3 * p + 2] = r.z;
        orig[p] = (int)i;
        rec[p] = r;
    }
    clk[3] = (long long)__builtin_amdgcn_s_memtime();
    // starts of this group's columns (column c of the grid = column c - lo * gy of the group); the last group also writes the end marker
    const int c_lo = lo * gy, c_hi = hi * gy;
    for (int c = c_lo + tid; c < c_hi; c += kWG) {
        if (col_start) { cs[c] = p0 + (int)col_start[c - c_lo]; cs16[c] = (unsigned short)(p0 + (int)col_start[c - c_lo]); continue; }
        const unsigned int want = (unsigned int)(c - c_lo) << z_bits;
        int a = 0, b = m;
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (s_key[order[mid]] < want) a = mid + 1; else b = mid;
        }
        cs[c] = p0 + a;
        cs16[c] = (unsigned short)(p0 + a);
    }
    if (g == kIcpSortGroups - 1 && tid == 0) { cs[gx * gy] = nt; cs16[gx * gy] = (unsigned short)nt; }
    if (tid == 0) {
        if (g == 0) {
            S.gx = gx; S.gy = gy; S.zq_max = zq_max; S.gminx = minx; S.gminy = miny; S.gminz = minz; S.cell = cell; S.inv_cell = inv;
            S.inv_z = inv_z;
        }
        atomicAdd(&S.grid_done, 1);
        clk[4] = (long long)__builtin_amdgcn_s_memtime();
        for (int k = 0; k < 4; ++k) atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[8 + k]), (unsigned long long)(clk[k + 1] - clk[k]));
        atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[4]), (unsigned long long)(tick[0] - clk[0]));
        atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[5]), (unsigned long long)(tick[1] - tick[0]));
        atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[7]), (unsigned long long)(tick[2] - tick[1]));
        atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[13]), (unsigned long long)m);
        atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[14]), (unsigned long long)(c_hi - c_lo));
        atomicMax(reinterpret_cast<unsigned long long*>(&S.sort_clk[15]), (unsigned long long)bits);
    }
}

// ---------------------------------------------------------------------------------------------
// k_icp_knn: open3d EstimateNormals(KDTreeSearchParamKNN(30)), neighbour search part.  The columns within ring R of a point's
// column hold every point closer than R*cell, so once >= k candidates are closer than that, the k nearest of them are the
// k nearest of the cloud.  A workgroup owns a contiguous range of sorted positions (= an x slab of the grid) and stages the
// columns its base rings reach in LDS (grown rings read HBM where they leave it).
// EIGHT LANES per point, eight points per wave.  (A wave per point — candidates across 64 lanes, ballots for the selection —
// was bound by instruction issue, ~4000 wave instructions per point; a lane per point needs ~400 but leaves the chip
// underfilled at the pipeline's sizes — 128k points are 2000 waves, two per SIMD, each a 300k-cycle serial walk — and stalls
// whole waves on the isolated points whose rings grow to thousands of candidates.  Eight lanes keep the instruction count
// of the lane-per-point version, give 16k waves, and share a grown ring eight ways.)
// Nothing is stored per candidate: every pass walks the ring again and recomputes the squared distances (the oracle's
// expression); the lanes of a point take the candidates four at a time, round robin, and add up their counts (DPP) —
//   pass 1   the candidates closer than the guarantee radius g and than three fractions of it (grows the ring when < k);
//   pass 2   counts below four thresholds interpolated inside the bracket pass 1 left (the distances of a surface patch are
//            close to uniform in d^2);
//   pass 3+  every lane keeps the 4 smallest DISTINCT distances of the bracket it sees, with multiplicities (equal distances
//            are common in a cloud that comes off a pixel grid); the lanes' lists are merged smallest first until the
//            running count reaches k, or the bracket moves past what was collected;
//   ties at the k-th distance go to the lower original index (one pass per tie taken, rare);
//   last     the cumulants of the selected points and the distance to the nearest other point.
// ---------------------------------------------------------------------------------------------
constexpr int kKnnWG = 512;
constexpr int kKnnLanes = 8;       // lanes per point
constexpr int kKnnSlabPts = 2048;  // target points staged per workgroup (32-byte records, 64 KiB: two workgroups per CU)
constexpr int kKnnRuns = 16;       // x columns of a ring kept as separate runs (R <= 7; wider rings take whole x columns)
constexpr int kKnnHard = 512;      // points per round of a workgroup, any of which may be handed to a whole wave
constexpr int kKnnFarBlocks = 96;  // ... with this many workgroups per hypothesis
constexpr int kKnnFew = 4;         // distinct distances a lane sorts in registers in a collecting pass

// reductions over the 8 lanes of a point (xor 1, xor 2, mirror within the half row): every lane ends with the result
static __device__ __forceinline__ int sum8(int v) { v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); v += dpp_mov<0x141>(v); return v; }
static __device__ __forceinline__ double sum8(double v) { v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); v += dpp_mov<0x141>(v); return v; }
static __device__ __forceinline__ double min8(double v) {
    v = fmin(v, dpp_mov<0xB1>(v)); v = fmin(v, dpp_mov<0x4E>(v)); v = fmin(v, dpp_mov<0x141>(v)); return v;
}
static __device__ __forceinline__ int min8(int v) { v = min(v, dpp_mov<0xB1>(v)); v = min(v, dpp_mov<0x4E>(v)); v = min(v, dpp_mov<0x141>(v)); return v; }

// f(j, d): this lane's share of the candidates of the ring — nx runs [runs[i].x, runs[i].y) of sorted positions (the columns
// ya..yb of one x are contiguous; the runs of a point sit in LDS) — with their squared distances to p: four consecutive
// candidates per trip, the lanes of the point side by side.  A run inside the staged slab [p0, p0 + np) comes from LDS.
template <int L, bool kFromLds, typename F>
static __device__ __forceinline__ void knn_scan_run(const int a, const int b, const int sub, const TgtRec* s_rel /*s_tgt - p0*/,
                                                    const TgtRec* __restrict__ g_rec, const double px, const double py, const double pz, F&& f) {
    constexpr int U = kFromLds ? 4 : 8;                            // candidates per lane and trip (HBM: more bytes in flight)
    // candidate v of a trip: j0 + v * L + sub — the lanes of a point read consecutive records (LDS: all banks once per group of
    // eight; HBM: coalesced), U per lane
    for (int j0 = a + sub; j0 < b; j0 += U * L) {
        double d4[U], q4[U][3];
#pragma unroll
        for (int v = 0; v < U; ++v) {
            const int j = j0 + v * L < b ? j0 + v * L : b - 1;
            if (kFromLds) { const TgtRec& r = s_rel[j]; q4[v][0] = r.x; q4[v][1] = r.y; q4[v][2] = r.z; }
            else { const double2 xy = *reinterpret_cast<const double2*>(&g_rec[j].x); q4[v][0] = xy.x; q4[v][1] = xy.y; q4[v][2] = g_rec[j].z; }
        }
#pragma unroll
        for (int v = 0; v < U; ++v) d4[v] = sqdist(px, py, pz, q4[v][0], q4[v][1], q4[v][2]);
        // (the squared distance as the unsigned integer its bit pattern is: it is >= 0, so the order is the same, and a dependent integer
        // compare + select costs a lone wave a few cycles where the f64 pair costs ~30 — profiles/r06_latency_microbench.txt)
#pragma unroll
        for (int v = 0; v < U; ++v)
            if (j0 + v * L < b) f(j0 + v * L, (unsigned long long)__double_as_longlong(d4[v]), q4[v][0], q4[v][1], q4[v][2]);
    }
}
// (two loops, not one loop with a choice of pointer inside: a pointer that may be LDS or HBM makes every load a FLAT load,
// which costs an LDS read the latency of a trip to memory)
template <int L, typename F>
static __device__ __forceinline__ void knn_scan(const int2* runs, const int nx, const int sub, const TgtRec* s_tgt, const int p0, const int np,
                                                const TgtRec* __restrict__ T, const double px, const double py, const double pz, F&& f) {
    for (int xi = 0; xi < nx; ++xi) {
        const int2 ab = runs[xi];
        if (ab.x >= p0 && ab.y <= p0 + np) knn_scan_run<L, true>(ab.x, ab.y, sub, s_tgt - p0, T, px, py, pz, f);
        else knn_scan_run<L, false>(ab.x, ab.y, sub, s_tgt - p0, T, px, py, pz, f);
    }
}

// One point, L lanes (8: the lane group of the main loop; 64: a whole wave, for the points whose ring has to grow).
template <int L> struct Red;
static __device__ __forceinline__ unsigned long long min8(unsigned long long v) {
    unsigned long long o = dpp_mov64<0xB1>(v); v = o < v ? o : v;
    o = dpp_mov64<0x4E>(v); v = o < v ? o : v;
    o = dpp_mov64<0x141>(v); v = o < v ? o : v;
    return v;
}
template <> struct Red<8> {
    static __device__ __forceinline__ unsigned long long mn(unsigned long long v) { return min8(v); }
    static __device__ __forceinline__ int sum(int v) { return sum8(v); }
    static __device__ __forceinline__ double sum(double v) { return sum8(v); }
    static __device__ __forceinline__ int mn(int v) { return min8(v); }
    static __device__ __forceinline__ double mn(double v) { return min8(v); }
};
template <> struct Red<64> {
    static __device__ __forceinline__ unsigned long long mn(unsigned long long v) { v = min8(v); for (int o = 8; o < 64; o <<= 1) { const unsigned long long t = shfl_xor_u64(v, o); v = t < v ? t : v; } return v; }
    static __device__ __forceinline__ int sum(int v) { v = sum8(v); for (int o = 8; o < 64; o <<= 1) v += __shfl_xor(v, o, 64); return v; }
    static __device__ __forceinline__ double sum(double v) { v = sum8(v); for (int o = 8; o < 64; o <<= 1) v += shfl_xor_d(v, o); return v; }
    static __device__ __forceinline__ int mn(int v) { v = min8(v); for (int o = 8; o < 64; o <<= 1) v = min(v, __shfl_xor(v, o, 64)); return v; }
    static __device__ __forceinline__ double mn(double v) { v = min8(v); for (int o = 8; o < 64; o <<= 1) v = fmin(v, shfl_xor_d(v, o)); return v; }
};

// a whole workgroup of 512 threads per point (k_icp_knn_far): wave reduction, then the 8 waves meet in LDS.  Every thread of
// the workgroup must make the same calls (the point's state is the same in all of them, so the control flow is).
template <> struct Red<512> {
    template <typename V, typename Op> static __device__ __forceinline__ V all(V v, Op op) {
        __shared__ V s_v[8];
        v = op(v, dpp_mov<0xB1>(v)); v = op(v, dpp_mov<0x4E>(v)); v = op(v, dpp_mov<0x141>(v));
        for (int o = 8; o < 64; o <<= 1) v = op(v, shfl_any(v, o));
        __syncthreads();                                             // (the previous reduction has been read)
        if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
        __syncthreads();
        V r = s_v[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) r = op(r, s_v[w]);
        return r;
    }
    static __device__ __forceinline__ int shfl_any(int v, int o) { return __shfl_xor(v, o, 64); }
    static __device__ __forceinline__ double shfl_any(double v, int o) { return shfl_xor_d(v, o); }
    static __device__ __forceinline__ unsigned long long shfl_any(unsigned long long v, int o) { return shfl_xor_u64(v, o); }
    static __device__ __forceinline__ unsigned long long mn(unsigned long long v) { return all(v, [](unsigned long long a, unsigned long long b) { return a < b ? a : b; }); }
    static __device__ __forceinline__ int sum(int v) { return all(v, [](int a, int b) { return a + b; }); }
    static __device__ __forceinline__ double sum(double v) { return all(v, [](double a, double b) { return a + b; }); }
    static __device__ __forceinline__ int mn(int v) { return all(v, [](int a, int b) { return a < b ? a : b; }); }
    static __device__ __forceinline__ double mn(double v) { return all(v, [](double a, double b) { return fmin(a, b); }); }
};

template <int L>
static __device__ __forceinline__ bool knn_point(const int pos, const int sub, int2* runs, const int k, const int R0, const int Rmax, const TgtRec* s_tgt, const int p0,
                                                 const int np, const double* __restrict__ T, const TgtRec* __restrict__ rec, const int* __restrict__ orig,
                                                 const int* __restrict__ cs, double* __restrict__ cov, const int gx, const int gy, const double minx, const double miny,
                                                 const double inv, const double cell) {
    const double kInfD = __longlong_as_double(0x7FF0000000000000ll);
    auto key = [](const double d) { return (unsigned long long)__double_as_longlong(d); };
    auto val = [](const unsigned long long k) { return __longlong_as_double((long long)k); };
    const double px = T[3 * (size_t)pos], py = T[3 * (size_t)pos + 1], pz = T[3 * (size_t)pos + 2];
    const int cx = grid_coord(px, minx, inv, gx), cy = grid_coord(py, miny, inv, gy);
    int R = R0, nx, c0, c1, c2, c3, M;
        double g2;
    bool all;
    for (;;) {
        const int xa = max(cx - R, 0), xb = min(cx + R, gx - 1), ya = max(cy - R, 0), yb = min(cy + R, gy - 1);
        all = xa == 0 && ya == 0 && xb == gx - 1 && yb == gy - 1;
        nx = xb - xa + 1;
        if (nx > kKnnRuns) {                                   // a ring that wide (tiny cloud): whole x columns, which are one run
            nx = 1;
            if (sub == 0) runs[0] = make_int2(cs[xa * gy], cs[(xb + 1) * gy]);
        } else {
            for (int xi = sub; xi < nx; xi += L) runs[xi] = make_int2(cs[(xa + xi) * gy + ya], cs[(xa + xi) * gy + yb + 1]);
        }
        if (L > 64) __syncthreads();                               // (within a wave the LDS operations are in order)
        const double g = (double)R * cell * (1.0 - 1e-9);     // margin >> the rounding of grid_coord
        g2 = g * g;
        // pass 1: how many candidates are closer than g, g/sqrt(2), g/2, g/sqrt(8)
        const unsigned long long kg = key(g2), k1 = key(g2 * 0.5), k2 = key(g2 * 0.25), k3 = key(g2 * 0.125);
        c0 = 0; c1 = 0; c2 = 0; c3 = 0; M = 0;
        knn_scan<L>(runs, nx, sub, s_tgt, p0, np, rec, px, py, pz, [&](int, unsigned long long d, double, double, double) {
            ++M; c0 += d < kg ? 1 : 0; c1 += d < k1 ? 1 : 0; c2 += d < k2 ? 1 : 0; c3 += d < k3 ? 1 : 0;
        });
        c0 = Red<L>::sum(c0); c1 = Red<L>::sum(c1); c2 = Red<L>::sum(c2); c3 = Red<L>::sum(c3); M = Red<L>::sum(M);
        if (c0 >= k || all) break;
        if (R >= Rmax) return false;                            // the ring has to grow further: the caller hands the point to a whole wave
        // isolated points: grow geometrically, not ring by ring (a whole wave doubles)
        R = L == 64 ? 2 * R : R + (R > 1 ? R >> 1 : 1);
    }
    // bracket: `cl` distances are < lo, `ch` are < hi, cl < k <= ch.  Selected in the end: d < v, and of the candidates at
    // d == v none (ties 0), all (1) or those up to original index last_o (2).
    unsigned long long lo = 0ull, hi = c0 >= k ? key(g2) : key(kInfD);     // (keys: see knn_scan_run)
    int cl = 0, ch = c0 >= k ? c0 : M;
    if (c0 >= k) {
        const unsigned long long h1 = key(g2 * 0.5), h2 = key(g2 * 0.25), h3 = key(g2 * 0.125);
        if (c1 >= k) { hi = h1; ch = c1; } else if (c1 > cl) { lo = h1; cl = c1; }
        if (c2 >= k) { hi = h2; ch = c2; } else if (c2 > cl) { lo = h2; cl = c2; }
        if (c3 >= k) { hi = h3; ch = c3; } else if (c3 > cl) { lo = h3; cl = c3; }
    }
    unsigned long long v = hi;
    int ties = ch == k ? 0 : -1, last_o = -1;
    if (ties < 0 && hi < key(kInfD)) {
        // pass 2: four thresholds around where the k-th smallest should be if the count is linear in between
        const double dlo = val(lo), dhi = val(hi);
        const double w = dhi - dlo, f0 = ((double)(k - cl) + 0.5) / (double)(ch - cl + 1), df = 1.5 / (double)(ch - cl + 1);
        const double td[4] = {dlo + w * (f0 - 3.0 * df), dlo + w * (f0 - df), dlo + w * (f0 + df), dlo + w * (f0 + 3.0 * df)};
        unsigned long long t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = key(td[q] > dlo ? (td[q] < dhi ? td[q] : dhi) : dlo);
        int n4[4] = {0, 0, 0, 0};
        knn_scan<L>(runs, nx, sub, s_tgt, p0, np, rec, px, py, pz, [&](int, unsigned long long d, double, double, double) {
#pragma unroll
            for (int q = 0; q < 4; ++q) n4[q] += d < t[q] ? 1 : 0;
        });
#pragma unroll
        for (int q = 0; q < 4; ++q) {                          // ascending thresholds: the last one below k raises lo, the first one at or above k lowers hi
            const int n = Red<L>::sum(n4[q]);
            if (n < k) { if (n >= cl && t[q] > lo) { lo = t[q]; cl = n; } }
            else if (t[q] < hi) { hi = t[q]; ch = n; }
        }
        if (ch == k) { ties = 0; v = hi; }
    }
    while (ties < 0) {
        // the kKnnFew smallest distinct distances in [lo, hi) this lane sees, with their multiplicities
        const unsigned long long kInf = key(kInfD);
        unsigned long long sv[kKnnFew];
        int sc[kKnnFew];
#pragma unroll
        for (int q = 0; q < kKnnFew; ++q) { sv[q] = kInf; sc[q] = 0; }
        knn_scan<L>(runs, nx, sub, s_tgt, p0, np, rec, px, py, pz, [&](int, unsigned long long d, double, double, double) {
            if (d >= lo && d < hi) {
                unsigned long long x = d;
                int xc = 1;
#pragma unroll
                for (int q = 0; q < kKnnFew; ++q) {
                    if (x == sv[q]) { sc[q] += xc; xc = 0; x = kInf; }
                    else if (x < sv[q]) { const unsigned long long tt = sv[q]; const int tc = sc[q]; sv[q] = x; sc[q] = xc; x = tt; xc = tc; }
                }
            }
        });
        // merge the 8 lists smallest value first.  A lane whose list ran empty after being full may have dropped larger
        // values: nothing above the smallest such "last kept" value can be trusted (limit)
        const unsigned long long limit = Red<L>::mn(sc[kKnnFew - 1] > 0 ? sv[kKnnFew - 1] : kInf);
        int cum = cl, less = -1, eq = 0;
        for (int it = 0; it < kKnnFew * L && less < 0; ++it) {
            const unsigned long long head = Red<L>::mn(sv[0]);
            if (!(head < kInf) || head > limit) break;
            const int mult = Red<L>::sum(sv[0] == head ? sc[0] : 0);
            if (cum + mult >= k) { v = head; less = cum; eq = mult; break; }
            cum += mult;
            if (sv[0] == head) {                                // pop
#pragma unroll
                for (int q = 0; q + 1 < kKnnFew; ++q) { sv[q] = sv[q + 1]; sc[q] = sc[q + 1]; }
                sv[kKnnFew - 1] = kInf; sc[kKnnFew - 1] = 0;
            }
            if (head == limit) break;                           // everything up to the limit is counted; beyond it lists are incomplete
        }
        if (less < 0) {                                          // the k-th is above what was collected: go on from there
            // every distance <= the last merged value is counted in cum; restart just above it
            const unsigned long long top = limit < kInf ? limit : hi;       // (limit == inf: all lists complete, so cum == ch >= k cannot happen here)
            lo = top + 1ull; cl = cum;                            // (the next double above)
            continue;
        }
        if (less + eq == k) { ties = 1; break; }
        ties = 2;                                                // k - less of the eq candidates at v, by original index
        for (int n = less; n < k; ++n) {
            int bo = INT_MAX;
            const int lo_o = last_o;
        knn_scan<L>(runs, nx, sub, s_tgt, p0, np, rec, px, py, pz, [&](int j, unsigned long long d, double, double, double) {
                if (d == v) { const int o = orig[j]; if (o > lo_o && o < bo) bo = o; }
            });
            last_o = Red<L>::mn(bo);
        }
    }
    double sum[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) sum[q] = 0.0;
    unsigned long long sep2 = key(1e300);
    int taken = 0;
    knn_scan<L>(runs, nx, sub, s_tgt, p0, np, rec, px, py, pz, [&](int j, unsigned long long d, double qx, double qy, double qz) {
        if (j != pos && d < sep2) sep2 = d;
        bool sel = d < v;
        if (ties && d == v) sel = ties == 1 || orig[j] <= last_o;
        if (sel) {
            sum[0] += qx; sum[1] += qy; sum[2] += qz;
            sum[3] += qx * qx; sum[4] += qx * qy; sum[5] += qx * qz; sum[6] += qy * qy; sum[7] += qy * qz; sum[8] += qz * qz;
            ++taken;
        }
    });
#pragma unroll
    for (int q = 0; q < 9; ++q) sum[q] = Red<L>::sum(sum[q]);
    taken = Red<L>::sum(taken);
    sep2 = Red<L>::mn(sep2);
    if (sub == 0) {
        double* c = cov + (size_t)pos * kIcpCovStride;
#pragma unroll
        for (int q = 0; q < 9; ++q) c[q] = sum[q];
        c[9] = (double)taken;
        c[10] = val(sep2);
    }
    return true;
}

__global__ void __launch_bounds__(kKnnWG, 4)       // two workgroups per CU (their LDS allows it): 128 VGPRs — at 165 a CU held one, and the ~26 workgroups of a cloud ran in two rounds
k_icp_knn(IcpBuffers B, int knn) {
    __shared__ TgtRec s_tgt[kKnnSlabPts];
    __shared__ int2 s_runs[kKnnWG / kKnnLanes][kKnnRuns];
    __shared__ int s_hard[kKnnHard];
    __shared__ int s_nhard;
    const int h = blockIdx.y;
    const IcpState& S = B.st[h];
    if (S.status != 0 || S.n_tgt == 0) return;
    const int nt = S.n_tgt;
    const double* T = B.tgt_sorted + (size_t)h * B.cap * 3;
    const int* orig = B.tgt_orig + (size_t)h * B.cap;
    const int* cs = B.cell_start + (size_t)h * kIcpCells;
    const TgtRec* rec = B.tgt_rec + (size_t)h * B.cap;
    double* cov = B.cov + (size_t)h * B.cap * kIcpCovStride;
    int* far_list = reinterpret_cast<int*>(B.keys + (size_t)h * 2 * B.cap2);   // the sort scratch is free by now
    const int gx = S.gx, gy = S.gy;
    const double minx = S.gminx, miny = S.gminy, inv = S.inv_cell, cell = S.cell;
    const int k = knn < nt ? knn : nt;
    int R0 = (int)ceil(0.009 / cell);
    if (R0 < 1) R0 = 1;
    // workgroups at work on this cloud: ~64 points each = one trip of the lane groups (a small cloud on all of the grid's workgroups would stage itself 64 times)
    const int want = (nt + 63) / 64, nb = want < 16 ? 16 : want > (int)gridDim.x ? (int)gridDim.x : want;
    if ((int)blockIdx.x >= nb) return;
    const int q0 = (int)((long long)nt * blockIdx.x / nb), q1 = (int)((long long)nt * (blockIdx.x + 1) / nb);
    if (q0 >= q1) return;
    // the slab: the columns the rings R0 + 1 of this workgroup's points reach (R0 if that is too much for the LDS)
    int xlo = max(grid_coord(T[3 * (size_t)q0], minx, inv, gx) - (R0 + 1), 0);
    int xhi = min(grid_coord(T[3 * (size_t)(q1 - 1)], minx, inv, gx) + (R0 + 1), gx - 1);
    if (cs[(xhi + 1) * gy] - cs[xlo * gy] > kKnnSlabPts) { xlo = min(xlo + 1, xhi); xhi = max(xhi - 1, xlo); }
    if (nt <= kKnnSlabPts) { xlo = 0; xhi = gx - 1; }             // a small cloud is staged whole: grown rings stay in LDS too
    const int p0 = cs[xlo * gy];
    int np = cs[(xhi + 1) * gy] - p0;
    if (np > kKnnSlabPts) np = 0;                                 // slab too large for LDS: every ring reads HBM
    const long long k_t0 = (long long)__builtin_amdgcn_s_memtime();
    {
        const uint4* src = reinterpret_cast<const uint4*>(rec + p0);
        uint4* dst = reinterpret_cast<uint4*>(s_tgt);
        for (int j = threadIdx.x; j < np * 2; j += kKnnWG) dst[j] = src[j];
    }
    __syncthreads();
    const long long k_t1 = (long long)__builtin_amdgcn_s_memtime();
    long long k_main = 0, k_hard = 0;
    const int sub = threadIdx.x & (kKnnLanes - 1), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = q0; base < q1; base += kKnnHard) {
        const int end = base + kKnnHard < q1 ? base + kKnnHard : q1;
        if (threadIdx.x == 0) s_nhard = 0;
        __syncthreads();
        // every lane group takes a point per trip; groups past the end idle (their lanes stay together: the DPP exchanges only
        // ever pair lanes of one group)
        for (int pos = base + threadIdx.x / kKnnLanes; pos < end; pos += kKnnWG / kKnnLanes) {
            const bool done = knn_point<kKnnLanes>(pos, sub, s_runs[threadIdx.x / kKnnLanes], k, R0, R0 + 1, s_tgt, p0, np, T, rec, orig, cs, cov, gx, gy, minx, miny,
                                                          inv, cell);
            if (!done && sub == 0) s_hard[atomicAdd(&s_nhard, 1)] = pos;
        }
        __syncthreads();
        const long long k_t2 = (long long)__builtin_amdgcn_s_memtime();
        // the points whose base ring held fewer than k candidates inside the guarantee radius (isolated points, flying pixels:
        // 2-15 % of a scene cloud, rings of hundreds to thousands of candidates): a wave each
        // (packing them onto the 8-lane groups once more, rings growing to 8, was measured: 117k cycles for that pass against 71k, and its
        // code cost the main trip 17k cycles in spilled registers)
        const int nhard = s_nhard;
        for (int i = wave; i < nhard; i += kKnnWG / 64) {
            const int pos = s_hard[i];
            int2* runs = s_runs[wave * (64 / kKnnLanes)];
            if (knn_point<64>(pos, lane, runs, k, R0 + 1 + ((R0 + 1) >> 1), 8, s_tgt, p0, np, T, rec, orig, cs, cov, gx, gy, minx, miny, inv, cell)) continue;
            // more than 8 rings from its k-th neighbour (a depth outlier, or a blob of fewer than k points away from the rest):
            // such a point needs the whole cloud — left to k_icp_knn_far, a workgroup each
            int slot = 0;
            if (lane == 0) slot = atomicAdd(&B.st[h].n_far, 1);
            slot = __shfl(slot, 0, 64);
            // (the list holds every target: 2 * cap2 keys of scratch per hypothesis.  It was cut at 256 entries once, the points beyond summed by
            // their wave: which ones depended on the order the waves arrived, and a run did not repeat bit for bit — 64 lanes and 512 threads
            // group the same 30 terms differently)
            if (lane == 0 && slot < nt) far_list[slot] = pos;       // (a point is handed over once, so slot < nt)
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long k_t3 = (long long)__builtin_amdgcn_s_memtime();
            k_main += k_t2 - (base == q0 ? k_t1 : k_t2); k_hard += k_t3 - k_t2;
            if (base == q0) k_main = k_t2 - k_t1;
            atomicAdd((unsigned long long*)&B.st[h].knn_clk[3], (unsigned long long)nhard);
        }
    }
    if (threadIdx.x == 0) {
        atomicMax((unsigned long long*)&B.st[h].knn_clk[0], (unsigned long long)(k_t1 - k_t0));
        atomicMax((unsigned long long*)&B.st[h].knn_clk[1], (unsigned long long)k_main);
        atomicMax((unsigned long long*)&B.st[h].knn_clk[2], (unsigned long long)k_hard);
    }
}

// (Round 6 built this search twice more with the candidates of a ring held in registers — one walk instead of 5-7, the selection passes over
// the slots; 16 lanes x 8-16 slots per point, then 8 lanes x 16 slots with whole waves x 8 slots for grown rings — exact on every test and
// slower both times: 198 and 130 us against 85 on the icp leg's clouds.  The kernel is bound by instruction issue, not by the walks: a pass
// is 4 sixty-four-bit compares + adds per slot whether the key comes out of a register or out of eight f64 operations, and the unrolled
// slots cost the idle ones in full.  profiles/r06_knn_notes.txt.)
// The points k_icp_knn could not finish within 8 rings: a workgroup each, the whole cloud as one coalesced run (one wave
// streaming 12k records four times over took ~1 M cycles, and a blob of such points sits in ONE workgroup of k_icp_knn).
__global__ void __launch_bounds__(512)
k_icp_knn_far(IcpBuffers B, int knn) {
    __shared__ int2 s_runs[kKnnRuns];
    const int h = blockIdx.y;
    const IcpState& S = B.st[h];
    if (S.status != 0 || S.n_tgt == 0) return;
    const int nt_all = S.n_tgt;
    const int nfar = S.n_far < nt_all ? S.n_far : nt_all;
    if ((int)blockIdx.x >= nfar) return;
    const int nt = nt_all;
    const int big = S.gx > S.gy ? S.gx : S.gy;
    // (kKnnFarBlocks workgroups per cloud walk the list: a workgroup per possible entry was 4096 workgroups to dispatch for 16 clouds — 11 us
    // when the lists are empty, as they are for clouds without depth outliers)
    for (int i = blockIdx.x; i < nfar; i += gridDim.x) {
        const int pos = reinterpret_cast<const int*>(B.keys + (size_t)h * 2 * B.cap2)[i];
        (void)knn_point<512>(pos, (int)threadIdx.x, s_runs, knn < nt ? knn : nt, big, INT_MAX, nullptr, 0, 0, B.tgt_sorted + (size_t)h * B.cap * 3,
                             B.tgt_rec + (size_t)h * B.cap, B.tgt_orig + (size_t)h * B.cap, B.cell_start + (size_t)h * kIcpCells,
                             B.cov + (size_t)h * B.cap * kIcpCovStride, S.gx, S.gy, S.gminx, S.gminy, S.inv_cell, S.cell);
        __syncthreads();                                             // (s_runs and the reduction scratch are the next point's)
    }
}

// ---- 3x3 symmetric eigen decomposition (cyclic Jacobi), eigenvector of the smallest eigenvalue ----
static __device__ __attribute__((noinline)) void smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double n[3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        // (the sweeps converge quadratically: 1e-4, 1e-8, 1e-16, 1e-32 of the diagonal ... waiting for an exact zero was four more sweeps)
        if (off <= 1e-30 * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]))) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double apq = A[p][q];
                if (apq == 0.0) continue;
                double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {   // A <- A * G
                    double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {   // A <- G^T * A
                    double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    n[0] = V[0][m]; n[1] = V[1][m]; n[2] = V[2][m];
}

// The same eigenvector in closed form: the smallest root of the characteristic polynomial by the trigonometric formula (q + 2 p cos(phi + 2 pi / 3),
// absolute error ~1e-16 of the largest eigenvalue), then the cross product of the two best-conditioned rows of A - lambda I.  Its angle to the
// exact eigenvector is ~1e-15 / (relative gap to the next eigenvalue) — measured against LAPACK on 10^6 covariances of 30-point surface patches:
// 2e-14 at gaps of 0.05, 1e-11 at 1e-3 — where the Jacobi sweeps above are a chain of ~17 rotations of two square roots and three divisions each
// (~35k cycles of one lane; this is ~5k).  False (nothing written) when the matrix is a multiple of the identity or not finite.
static __device__ __forceinline__ bool smallest_eigvec_closed(double a00, double a01, double a02, double a11, double a12, double a22, double n[3]) {
    const double q = (a00 + a11 + a22) * (1.0 / 3.0);
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double p2 = (b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1) * (1.0 / 6.0);
    if (!(p2 > 0.0) || !(p2 < 1e300)) return false;
    const double ip = rsqrt(p2), p = p2 * ip;
    const double c00 = b00 * ip, c01 = a01 * ip, c02 = a02 * ip, c11 = b11 * ip, c12 = a12 * ip, c22 = b22 * ip;
    double r = 0.5 * (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02));
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    const double phi = acos(r) * (1.0 / 3.0);
    const double lam = q + 2.0 * p * cos(phi + 2.0943951023931954923);      // the smallest eigenvalue
    const double r0[3] = {a00 - lam, a01, a02}, r1[3] = {a01, a11 - lam, a12}, r2[3] = {a02, a12, a22 - lam};
    auto cross = [](const double (&u)[3], const double (&w)[3], double (&o)[3]) {
        o[0] = u[1] * w[2] - u[2] * w[1]; o[1] = u[2] * w[0] - u[0] * w[2]; o[2] = u[0] * w[1] - u[1] * w[0];
        return o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
    };
    double x01[3], x02[3], x12[3];
    const double n01 = cross(r0, r1, x01), n02 = cross(r0, r2, x02), n12 = cross(r1, r2, x12);
    const bool f01 = n01 >= n02 && n01 >= n12, f02 = n02 >= n12;
    const double nn = f01 ? n01 : (f02 ? n02 : n12);
    if (!(nn > 0.0) || !(nn < 1e300)) return false;
    const double s = rsqrt(nn);
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (f01 ? x01[k] : (f02 ? x02[k] : x12[k])) * s;
    return true;
}

// k_icp_normals: open3d ComputeNormal from the cumulants: covariance = E[xx^T] - E[x]E[x]^T,
// normal = eigenvector of its smallest eigenvalue ((0,0,1) for fewer than 3 neighbours).
__global__ void __launch_bounds__(256)
k_icp_normals(IcpBuffers B) {
    const int h = blockIdx.y;
    const IcpState& S = B.st[h];
    const int nt = S.status == 0 ? S.n_tgt : 0;
    const double* cov = B.cov + (size_t)h * B.cap * kIcpCovStride;
    double* N = B.normals + (size_t)h * B.cap * 3;
    for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < nt; pos += gridDim.x * blockDim.x) {
        const double* c = cov + (size_t)pos * kIcpCovStride;
        const double k = c[9];
        double nrm[3] = {0, 0, 1};
        if (k >= 3.0) {
            const double mx = c[0] / k, my = c[1] / k, mz = c[2] / k;
            const double a00 = c[3] / k - mx * mx, a01 = c[4] / k - mx * my, a02 = c[5] / k - mx * mz, a11 = c[6] / k - my * my, a12 = c[7] / k - my * mz,
                         a22 = c[8] / k - mz * mz;
            if (!smallest_eigvec_closed(a00, a01, a02, a11, a12, a22, nrm)) smallest_eigvec(a00, a01, a02, a11, a12, a22, nrm);
            if (nrm[0] == 0 && nrm[1] == 0 && nrm[2] == 0) nrm[2] = 1;
        }
        N[3 * (size_t)pos] = nrm[0]; N[3 * (size_t)pos + 1] = nrm[1]; N[3 * (size_t)pos + 2] = nrm[2];
    }
}

hipError_t launch_icp_prepare(const IcpBuffers& B, int count, int W, int H, int flags, double voxel, int knn, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const Knobs& kn = knobs();
    const int scene_mode = flags & 1;
    LAUNCH_TRY(launch_icp_clouds(B, count, W, H, flags, s));
    // voxel down-sampling and the search grid by kIcpSortGroups workgroups per cloud; the one-workgroup kernels behind them take what those
    // left (IcpState::vox_done / grid_done) and cost ~2 us when there is nothing
    if (kn.icp_wide_sort) LAUNCH_TRY(lm_launch(k_icp_voxel_wide, dim3(kIcpSortGroups, count, scene_mode ? 2 : 1), dim3(kWG), 0, s, B, flags, voxel));
    LAUNCH_TRY(lm_launch(k_icp_voxel, dim3(count, scene_mode ? 2 : 1), dim3(kWG), 0, s, B, flags, voxel));
    if (kn.icp_wide_sort) LAUNCH_TRY(lm_launch(k_icp_grid_wide, dim3(kIcpSortGroups, count), dim3(kWG), 0, s, B, flags));
    LAUNCH_TRY(lm_launch(k_icp_grid, dim3(count), dim3(kWG), 0, s, B, flags));
    LAUNCH_TRY(lm_launch(k_icp_knn, dim3(kn.knn_blocks > 0 ? kn.knn_blocks : (count <= 32 ? 64 : 32), count), dim3(kKnnWG), 0, s, B, knn));
    LAUNCH_TRY(lm_launch(k_icp_knn_far, dim3(kKnnFarBlocks, count), dim3(512), 0, s, B, knn));
    return flags & 2 ? hipSuccess : lm_launch(k_icp_normals, dim3(count <= 32 ? 64 : 16, count), dim3(256), 0, s, B);   // (point-to-point reads no normals)
}

}  // namespace lm
