/* The plain structures of the particle-swarm refiner of amd_linemod.h (lm_pso_*).
 * Included by amd_linemod.h; not meant to be included on its own. */
#ifndef AMD_LINEMOD_PSO_H
#define AMD_LINEMOD_PSO_H

#include <stdint.h>

/* lm_pso_options_init fills in: particles 64, generations 30, tau 20, cover_pixels 0, seed 0, trans_range_mm 20,
 * rot_range tan(radians(10) / 2), inertia 0.7298, c1 = c2 = 1.49618, clip 10 / 10000. */
typedef struct lm_pso_options {
    uint32_t size;          /* sizeof(lm_pso_options); anything else -> LM_ERR_INVALID */
    int32_t particles;      /* P, 1..256 per hypothesis; hypotheses x P <= 4096 */
    int32_t generations;    /* 0..256, no early stop; 0 = evaluate-only: particle 0 (the given pose) alone is scored */
    int32_t tau;            /* 1..65535 mm: the largest cost of a pixel, and the cost of one whose scene depth is 0 */
    int32_t cover_pixels;   /* 0: n_0 of the cover floor is the rendered pixel count of the given pose; > 0: this count instead
                               (the area the caller expects to see, e.g. of the matched template) */
    int32_t reserved;
    uint64_t seed;
    double trans_range_mm;  /* particles move within +- this of t0 on every axis; finite, > 0 */
    double rot_range;       /* and within +- this per Cayley component: tan(angle / 2) of the largest rotation about an axis */
    double inertia, c1, c2; /* v = inertia v + c1 u1 (pbest - x) + c2 u2 (gbest - x) */
    double clip_near, clip_far;
} lm_pso_options;

/* The global best of one hypothesis. */
typedef struct lm_pso_result {
    double R[9];            /* dR(a) R0, row-major */
    double t[3];            /* t0 + dt, mm */
    double cost;            /* mean clamped depth difference (mm) of the best pose; +inf when nothing was ever rendered */
    double initial_cost;    /* of the given pose */
    int32_t n_rendered;     /* rendered pixels of the best pose */
    int32_t n_initial;      /* n_0 */
    int32_t best_particle, best_generation;
} lm_pso_result;

#endif /* AMD_LINEMOD_PSO_H */
