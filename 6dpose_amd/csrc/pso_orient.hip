// The directional chamfer cost of the particle-swarm refiner: the edge cost of pso_edges.hip with the distance taken
// in (x, y, orientation).  The scene is Q, LINE-MOD's quantised gradient orientations: bit k (0..7) of a pixel set = an edge of bin k there.
// tests/pso_orient_ref.py states the rule in numpy and IS the definition; everything here is an integer, so the kernels are held to it
// bit for bit.  With M = max_dist, P = orient_penalty (px^2 per bin^2) and d(k, j) = min(|k - j|, 8 - |k - j|):
//   D2_j   = the truncated squared distance of pso_edges.hip to the pixels with bit j                 (k_edt_rows_bits, k_edt_cols_planes)
//   DD2[k] = min(M^2, min over j of D2_j + P d(k, j)^2), k = 0..7;  DD2[8] = min over j of D2_j       (k_edt_orient, uint16)
//   contour: pso_edges.hip's; o(n) = 1 for a neighbour n of the 8 inside the window with n == 0 or (step > 0 and n - r > step);
//   (gx, gy) = the 3 x 3 Sobel sums of o, y downwards; k_p = the bin of atan2(gy, gx) (kBinOf), 8 where gx == gy == 0;
//   sum += min(DD2[k_p], tau^2) at a contour pixel inside the frame, tau^2 outside; n_c counts the contour pixels.
// The two channel passes are k_edt_rows' and k_edt_cols' bodies (pso_edge_device.h) with the channel as the grid's z, and k_pso_orient_cost
// is k_pso_edge_cost's body with the plane chosen per contour pixel: one copy of each, instantiated here and in pso_edges.hip.
#include "launch.h"
#include "pso_edge_device.h"

namespace lm {

// (gx, gy) -> bin: round(atan2(gy, gx) in degrees mod 360 * 16 / 360) & 7, row gy + 4, column gx + 4; 8 = no orientation.  Every entry is
// at least 0.0599 degrees from a bin boundary (tests/pso_orient_ref.py builds the table in float64 and asserts the margin).
__constant__ const uint8_t kBinOf[81] = {
    2, 2, 3, 3, 4, 5, 5, 6, 6,
    2, 2, 3, 3, 4, 5, 5, 6, 6,
    1, 1, 2, 3, 4, 5, 6, 7, 7,
    1, 1, 1, 2, 4, 6, 7, 7, 7,
    0, 0, 0, 0, 8, 0, 0, 0, 0,
    7, 7, 7, 6, 4, 2, 1, 1, 1,
    7, 7, 6, 5, 4, 3, 2, 1, 1,
    6, 6, 5, 5, 4, 3, 3, 2, 2,
    6, 6, 5, 5, 4, 3, 3, 2, 2,
};

__global__ __launch_bounds__(256) void k_edt_rows_bits(const uint8_t* __restrict__ q, int W, int H, int M, uint8_t* __restrict__ g) {
    edt_rows_body<true>(q, W, H, M, blockIdx.z, g);
}
__global__ __launch_bounds__(256) void k_edt_cols_planes(const uint8_t* __restrict__ g, int W, int H, int M, uint16_t* __restrict__ d2) {
    edt_cols_body(g, W, H, M, (size_t)blockIdx.z * W * H, d2);
}

// One lane per pixel: the eight D2_j in, the nine planes out; lane i of a wave reads and writes element i of every plane.  The penalty
// P d^2 takes five values, wave-uniform; the 8 x 8 minimum is unrolled, so which of them an entry takes is known at compile time.
// D2_j <= 255^2 and P d^2 <= 4096 x 16: the sums fit 32 bits with room.
__global__ __launch_bounds__(256) void k_edt_orient(const uint16_t* __restrict__ d2, size_t n, int M, int P, uint16_t* __restrict__ dd2) {
    const int pen[5] = {0, P, 4 * P, 9 * P, 16 * P};
    const int cap = M * M;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = d2[(size_t)j * n + i];
        int any = v[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) any = min(any, v[j]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int best = cap;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int a = k > j ? k - j : j - k;
                best = min(best, v[j] + pen[a < 8 - a ? a : 8 - a]);
            }
            dd2[(size_t)k * n + i] = (uint16_t)best;
        }
        dd2[(size_t)8 * n + i] = (uint16_t)any;
    }
}

__global__ __launch_bounds__(256) void k_pso_orient_cost(PsoParams prm, int edge_step, const PsoHyp* __restrict__ hyp, const unsigned long long* __restrict__ zbuf,
                                                         const uint16_t* __restrict__ dd2, unsigned long long* __restrict__ sum_out,
                                                         unsigned int* __restrict__ nr_out) {
    pso_contour_cost_body<true>(prm, edge_step, hyp, zbuf, dd2, kBinOf, sum_out, nr_out);
}

hipError_t launch_edt_orient(const uint8_t* q, int W, int H, int M, int P, uint8_t* g, uint16_t* d2, uint16_t* dd2, hipStream_t s) {
    LAUNCH_TRY(lm_launch(k_edt_rows_bits, dim3((W + kEdtRun - 1) / kEdtRun, H, 8), dim3(256), 0, s, q, W, H, M, g));
    const size_t lds = (size_t)(kEdtRows + 2 * (M - 1)) * kEdtCols;
    LAUNCH_TRY(lm_launch(k_edt_cols_planes, dim3((W + kEdtCols - 1) / kEdtCols, (H + kEdtRows - 1) / kEdtRows, 8), dim3(256), lds, s, g, W, H, M, d2));
    const size_t n = (size_t)W * H, blocks = (n + 255) / 256;
    return lm_launch(k_edt_orient, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, d2, n, M, P, dd2);
}
hipError_t launch_pso_orient_cost(const PsoParams& p, int H, int edge_step, const PsoHyp* hyp, const unsigned long long* zbuf, const uint16_t* dd2,
                            unsigned long long* sum, unsigned int* n_r, hipStream_t s) {
    return lm_launch(k_pso_orient_cost, dim3(H * p.P), dim3(256), 0, s, p, edge_step, hyp, zbuf, dd2, sum, n_r);
}

}  // namespace lm
