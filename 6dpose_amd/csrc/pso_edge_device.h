// The device bodies pso_edges.hip and pso_orient.hip share: the two passes of the truncated squared distance
// transform, and the contour cost of a rendered window.  Each kernel of the two units is one instantiation; the rule is stated in
// tests/pso_edges_ref.py and tests/pso_orient_ref.py.  gfx950 only.
#pragma once
#include "pso_kernels.h"

namespace lm {

constexpr int kEdtRun = 256;             // rows pass: columns of a row per workgroup, one per lane
constexpr int kEdtCols = 64;             // columns pass: columns per workgroup, one per lane of a wave
constexpr int kEdtRows = 32;             // columns pass: rows per workgroup, 8 per wave
constexpr int kEdgeBand = 32;            // contour cost: rows of the window staged at a time (plus one above and below)

// One workgroup per run of 256 columns of a row.  LDS holds the row's edge bytes for the run and M - 1 columns either side, 0 beyond
// the row's ends; a lane looks outwards from its column, d = 0, 1, .. M - 1, and stops at the first edge.  kBits: an edge is a pixel
// with bit `bit` set and g is written to plane `bit`; otherwise an edge is a pixel that is not 0 and there is one plane.
template <bool kBits>
__device__ __forceinline__ void edt_rows_body(const uint8_t* __restrict__ edges, int W, int H, int M, int bit, uint8_t* __restrict__ g) {
    __shared__ uint8_t s_e[kEdtRun + 2 * 254];
    const int y = blockIdx.y, c0 = blockIdx.x * kEdtRun, halo = M - 1;
    const int n = kEdtRun + 2 * halo;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int x = c0 - halo + i;
        uint8_t e = 0;
        if (x >= 0 && x < W) {
            const uint8_t v = edges[(size_t)y * W + x];
            e = kBits ? (uint8_t)((v >> bit) & 1) : (uint8_t)(v != 0);
        }
        s_e[i] = e;
    }
    __syncthreads();
    const int x = c0 + threadIdx.x;
    if (x >= W) return;
    const int at = halo + threadIdx.x;
    int d = 0;
    while (d < M && !(s_e[at - d] | s_e[at + d])) ++d;
    g[((size_t)(kBits ? bit : 0) * H + y) * W + x] = (uint8_t)d;
}

// One workgroup per tile of 64 columns x 32 rows of the plane at offset `plane`; LDS holds g for the tile and M - 1 rows above and below,
// M beyond the frame (where it cannot lower a minimum).  A wave reads a row of the tile as 64 consecutive bytes.  A lane looks up and
// down from its pixel, dy = 1, 2, .. and stops as soon as dy^2 alone reaches the best so far.
__device__ __forceinline__ void edt_cols_body(const uint8_t* __restrict__ g, int W, int H, int M, size_t plane, uint16_t* __restrict__ d2) {
    extern __shared__ uint8_t s_g[];                                   // [kEdtRows + 2 (M - 1)][kEdtCols]
    const int c0 = blockIdx.x * kEdtCols, r0 = blockIdx.y * kEdtRows, halo = M - 1;
    const int rows = kEdtRows + 2 * halo;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = c0 + lane;
    for (int i = wave; i < rows; i += 4) {
        const int y = r0 - halo + i;
        s_g[i * kEdtCols + lane] = (x < W && y >= 0 && y < H) ? g[plane + (size_t)y * W + x] : (uint8_t)M;
    }
    __syncthreads();
    if (x >= W) return;
    for (int j = wave; j < kEdtRows; j += 4) {
        const int y = r0 + j;
        if (y >= H) break;
        const int at = halo + j;
        int v = s_g[at * kEdtCols + lane];
        int best = v * v;                                              // <= M^2
        for (int dy = 1; dy < M && dy * dy < best; ++dy) {
            const int a = s_g[(at - dy) * kEdtCols + lane], b = s_g[(at + dy) * kEdtCols + lane];
            best = min(best, min(a * a, b * b) + dy * dy);
        }
        d2[plane + (size_t)y * W + x] = (uint16_t)best;
    }
}

// One workgroup (4 waves) per (hypothesis, particle), like k_pso_cost.  The window is walked in bands of 32 rows: the z-buffer keys of
// the band and of one row above and below are resolved to uint16 (k_resolve_depth's rule) into LDS, read coalesced as one contiguous
// run, so a key is read once (the two halo rows of a band twice) and the neighbours come from LDS.  Rows and columns outside the window
// are never consulted.  Per lane at most 256 pixels of at most 255^2 each: 32-bit sums; the reduction is k_pso_cost's.
// kOriented: d2 holds nine planes and a contour pixel reads the plane of its bin, from the Sobel sums of o over its eight neighbours
// (the four diagonal ones are formed for contour pixels only) through the 81-entry table `bins`; otherwise d2 is one plane.
template <bool kOriented>
__device__ __forceinline__ void pso_contour_cost_body(const PsoParams& prm, int edge_step, const PsoHyp* __restrict__ hyp,
                                                      const unsigned long long* __restrict__ zbuf, const uint16_t* __restrict__ d2,
                                                      const uint8_t* __restrict__ bins, unsigned long long* __restrict__ sum_out, unsigned int* __restrict__ nr_out) {
    __shared__ uint16_t s_r[(kEdgeBand + 2) * 256];                    // row i of LDS is window row b0 - 1 + i, w entries each
    const int view = blockIdx.x;
    const int x0 = hyp[view / prm.P].x0, y0 = hyp[view / prm.P].y0;
    const int w = prm.w, h = prm.h;
    const unsigned long long* Z = zbuf + (size_t)view * w * h;
    const int tau2 = prm.tau * prm.tau;
    unsigned int sum = 0, n_c = 0;
    for (int b0 = 0; b0 < h; b0 += kEdgeBand) {
        const int rows = min(kEdgeBand, h - b0);
        const int ya = max(b0 - 1, 0), yb = min(b0 + rows + 1, h);     // the window rows staged: [ya, yb)
        const int first = (ya - (b0 - 1)) * w;
        if (b0 > 0) __syncthreads();                                   // the band before has been read
        for (int i = threadIdx.x; i < (yb - ya) * w; i += 256) {
            const unsigned long long k = Z[ya * w + i];
            int r = 0;
            if (k != ~0ull) {
                const float z = __uint_as_float((unsigned int)(k >> 32));
                r = z >= 65535.f ? 65535 : (int)(uint16_t)z;
            }
            s_r[first + i] = (uint16_t)r;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < rows * w; i += 256) {
            const int j = i / w, wx = i - j * w, wy = b0 + j;
            const uint16_t* row = s_r + (j + 1) * w;
            const int r = row[wx];
            if (r == 0) continue;
            const bool left = wx > 0, right = wx < w - 1, up = wy > 0, down = wy < h - 1;
            auto o = [&](bool inside, int at) -> int {                 // 1: the neighbour is inside the window and empty or behind a depth jump
                if (!inside) return 0;
                const int n = row[at];
                return n == 0 || (edge_step > 0 && n - r > edge_step);
            };
            const int ol = o(left, wx - 1), orr = o(right, wx + 1), ou = o(up, wx - w), od = o(down, wx + w);
            if (!(ol | orr | ou | od)) continue;
            size_t plane = 0;
            if (kOriented) {
                const int oul = o(up && left, wx - w - 1), our = o(up && right, wx - w + 1);
                const int odl = o(down && left, wx + w - 1), odr = o(down && right, wx + w + 1);
                const int gx = (our + 2 * orr + odr) - (oul + 2 * ol + odl);
                const int gy = (odl + 2 * od + odr) - (oul + 2 * ou + our);
                plane = (size_t)bins[(gy + 4) * 9 + gx + 4] * prm.W * prm.H;
            }
            const int fx = x0 + wx, fy = y0 + wy;
            int t = tau2;
            if (fx >= 0 && fx < prm.W && fy >= 0 && fy < prm.H) t = min((int)d2[plane + (size_t)fy * prm.W + fx], tau2);
            sum += (unsigned int)t;
            n_c += 1u;
        }
    }
    unsigned long long wsum = sum;
    for (int o = 32; o > 0; o >>= 1) {
        wsum += __shfl_down(wsum, o, 64);
        n_c += __shfl_down(n_c, o, 64);
    }
    __shared__ unsigned long long s_sum[4];
    __shared__ unsigned int s_nc[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sum[wave] = wsum; s_nc[wave] = n_c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum_out[view] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        nr_out[view] = (s_nc[0] + s_nc[1]) + (s_nc[2] + s_nc[3]);
    }
}

}  // namespace lm
