// The edge (chamfer) cost of the particle-swarm refiner: for cameras without depth.  The scene is an edge map,
// turned once per frame into D2, the squared distance to the nearest edge pixel truncated at M = max_dist; a particle's rendered
// window is scored by the D2 under its contour pixels.  tests/pso_edges_ref.py states the rule in numpy and IS the definition;
// everything here is an integer, so the kernels are held to it bit for bit.
//   g[y][x]  = min(M, |x - x'| over the edge pixels x' of row y)                                   (k_edt_rows, uint8)
//   D2[y][x] = min(M^2, min over |dy| < M, 0 <= y + dy < H of g[y + dy][x]^2 + dy^2)               (k_edt_cols, uint16)
//   contour: r > 0 and a 4-neighbour n inside the window with n == 0 or (step > 0 and n - r > step);
//   sum += min(D2, tau^2) at a contour pixel inside the frame, tau^2 outside; n_c counts the contour pixels.
// The swarm around it (k_pso_init, k_pso_views, k_project, k_raster, k_pso_step) is pso.hip's, used as it is: k_pso_edge_cost
// writes (sum, n_c) where k_pso_cost writes (sum, n_r).  The kernels' bodies are pso_edge_device.h's, shared with pso_orient.hip.
#include "launch.h"
#include "pso_edge_device.h"

namespace lm {

__global__ __launch_bounds__(256) void k_edt_rows(const uint8_t* __restrict__ edges, int W, int H, int M, uint8_t* __restrict__ g) {
    edt_rows_body<false>(edges, W, H, M, 0, g);
}
__global__ __launch_bounds__(256) void k_edt_cols(const uint8_t* __restrict__ g, int W, int H, int M, uint16_t* __restrict__ d2) {
    edt_cols_body(g, W, H, M, 0, d2);
}
__global__ __launch_bounds__(256) void k_pso_edge_cost(PsoParams prm, int edge_step, const PsoHyp* __restrict__ hyp, const unsigned long long* __restrict__ zbuf,
                                                       const uint16_t* __restrict__ d2, unsigned long long* __restrict__ sum_out,
                                                       unsigned int* __restrict__ nr_out) {
    pso_contour_cost_body<false>(prm, edge_step, hyp, zbuf, d2, nullptr, sum_out, nr_out);
}

hipError_t launch_edt(const uint8_t* edges, int W, int H, int M, uint8_t* g, uint16_t* d2, hipStream_t s) {
    LAUNCH_TRY(lm_launch(k_edt_rows, dim3((W + kEdtRun - 1) / kEdtRun, H), dim3(256), 0, s, edges, W, H, M, g));
    const size_t lds = (size_t)(kEdtRows + 2 * (M - 1)) * kEdtCols;
    return lm_launch(k_edt_cols, dim3((W + kEdtCols - 1) / kEdtCols, (H + kEdtRows - 1) / kEdtRows), dim3(256), lds, s, g, W, H, M, d2);
}
hipError_t launch_pso_edge_cost(const PsoParams& p, int H, int edge_step, const PsoHyp* hyp, const unsigned long long* zbuf, const uint16_t* d2,
                          unsigned long long* sum, unsigned int* n_r, hipStream_t s) {
    return lm_launch(k_pso_edge_cost, dim3(H * p.P), dim3(256), 0, s, p, edge_step, hyp, zbuf, d2, sum, n_r);
}

}  // namespace lm
