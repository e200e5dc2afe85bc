// Internal interface between pso.cpp (host) and pso.hip (kernels).  gfx950 only.
#pragma once
#include "render_kernels.h"

namespace lm {

struct PsoHyp {              // one hypothesis: the start pose and the origin of its window in the frame
    double R0[9], t0[3];
    int x0, y0;
};
struct PsoParams {           // the same for every hypothesis of a call
    double K[9];             // the scene's camera
    double range[6];         // +-range per dimension: trans_range_mm x 3, rot_range x 3
    double inertia, c1, c2;
    unsigned long long seed;
    int P, G;                // particles per hypothesis, generations
    int w, h;                // window size
    int W, H;                // frame size
    int tau;
    int cover_pixels;        // > 0: n_0 is this instead of the initial pose's rendered pixels
};
struct PsoBest {             // the global best of one hypothesis
    double x[6];
    double cost, initial_cost;
    int particle, generation, n_r, n_0;
};
struct PsoResultDev {        // lm_pso_result as the last k_pso_step writes it
    double R[9], t[3];
    double cost, initial_cost;
    int n_rendered, n_initial, best_particle, best_generation;
};
struct PsoState {            // [HP] unless stated
    double* x;               // [HP][6]
    double* v;               // [HP][6]
    double* pbest_x;         // [HP][6]
    double* pbest_cost;
    unsigned long long* sum;
    unsigned int* n_r;
    PsoBest* best;           // [H]
    // the record of every generation for lm_pso_read_debug
    double* rec_x;           // [G + 1][HP][6]
    double* rec_cost;        // [G + 1][HP]
    unsigned long long* rec_sum;   // [G + 1][HP]
    unsigned int* rec_nr;    // [G + 1][HP]
    int* rec_best;           // [G + 1][H][2]: particle, generation of the global best after the generation
    PsoResultDev* result;    // [H]
};

[[nodiscard]] hipError_t launch_pso_init(const PsoParams& p, int H, const PsoState& st, hipStream_t s);
[[nodiscard]] hipError_t launch_pso_views(const PsoParams& p, int H, const PsoHyp* hyp, const double* x, ViewParams* views, hipStream_t s);
[[nodiscard]] hipError_t launch_pso_cost(const PsoParams& p, int H, const PsoHyp* hyp, const unsigned long long* zbuf, const uint16_t* scene,
                                         unsigned long long* sum, unsigned int* n_r, hipStream_t s);
[[nodiscard]] hipError_t launch_pso_step(const PsoParams& p, int H, int g, const PsoHyp* hyp, const PsoState& st, hipStream_t s);

// pso_edges.hip: the edge cost.  launch_edt: k_edt_rows (edges -> g, uint8) and k_edt_cols (g -> d2, uint16), 1 <= M <= 255.
// launch_pso_edge_cost: p.W, p.H are the edge frame's, p.tau is in pixels (<= M); it writes what launch_pso_cost writes.
[[nodiscard]] hipError_t launch_edt(const uint8_t* edges, int W, int H, int M, uint8_t* g, uint16_t* d2, hipStream_t s);
[[nodiscard]] hipError_t launch_pso_edge_cost(const PsoParams& p, int H, int edge_step, const PsoHyp* hyp, const unsigned long long* zbuf, const uint16_t* d2,
                                              unsigned long long* sum, unsigned int* n_r, hipStream_t s);

// pso_orient.hip: the directional edge cost.  launch_edt_orient: q (bit k = an edge of bin k) -> g [8][H][W] uint8 and
// d2 [8][H][W] uint16 per channel (k_edt_rows_bits, k_edt_cols_planes), then dd2 [9][H][W] uint16 (k_edt_orient); 1 <= M <= 255, 0 <= P <= 4096.
// launch_pso_orient_cost: launch_pso_edge_cost with the nine planes dd2 in d2's place.
[[nodiscard]] hipError_t launch_edt_orient(const uint8_t* q, int W, int H, int M, int P, uint8_t* g, uint16_t* d2, uint16_t* dd2, hipStream_t s);
[[nodiscard]] hipError_t launch_pso_orient_cost(const PsoParams& p, int H, int edge_step, const PsoHyp* hyp, const unsigned long long* zbuf, const uint16_t* dd2,
                                                unsigned long long* sum, unsigned int* n_r, hipStream_t s);

}  // namespace lm
