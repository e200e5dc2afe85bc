// Pose refinement by particle swarm over rendered depth: the refiner the reference's author left as a todo
// (linemodLevelup/readme.md:41-46, "PSO or some other method rather than ICP").  Correspondence-free: every particle of every
// hypothesis is a pose, rendered depth-only into a small window by k_project / k_raster (render.hip) and scored against the
// scene depth of that window.  tests/pso_ref.py states the rule in numpy and IS the definition; these kernels are held to it
// bit for bit, so everything that is not an integer is f64 through the __d*_rn intrinsics in the order written there.
//   particle x = (dt[3] mm, a[3]);  dR(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a)  (Cayley: + - * / only);
//   R = dR(a) R0, t = t0 + dt;  the window's camera is K with cx - x0, cy - y0.
//   cost: over window pixels with rendered depth r > 0 (n_r of them), sum += tau where the scene s == 0, else min(|r - s|, tau);
//   cost = sum / n_r when n_r >= (n_0 + 1) / 2 and n_r > 0, else +inf (the cover floor).
//   random numbers: the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 (1 + counter), counter = ((g P + p) 6 + d) 2 + draw;
//   g = 0 draws the initial positions, generation g >= 1 draws u1 (draw 0) and u2 (draw 1).  No state, the same for every hypothesis.
// The z-buffer: launch_raster clears it before every generation (its hipMemsetAsync), so k_pso_cost only reads it.
#include "launch.h"
#include "pso_kernels.h"

namespace lm {

static __device__ __forceinline__ double pso_uniform(unsigned long long seed, unsigned long long counter) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (1ull + counter);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return __dmul_rn(__ull2double_rn(z >> 11), 0x1.0p-53);              // 53 bits: the conversion is exact
}
static __device__ __forceinline__ unsigned long long pso_counter(int g, int P, int p, int d, int draw) {
    return (((unsigned long long)g * (unsigned long long)P + (unsigned long long)p) * 6ull + (unsigned long long)d) * 2ull + (unsigned long long)draw;
}

// R = dR(a) R0, t = t0 + dt
static __device__ __forceinline__ void pso_pose(const double x[6], const PsoHyp& h, double R[9], double t[3]) {
    const double a0 = x[3], a1 = x[4], a2 = x[5];
    const double aa = __dadd_rn(__dadd_rn(__dmul_rn(a0, a0), __dmul_rn(a1, a1)), __dmul_rn(a2, a2));
    const double den = __dadd_rn(1.0, aa), num = __dsub_rn(1.0, aa);
    const double b0 = __dmul_rn(2.0, a0), b1 = __dmul_rn(2.0, a1), b2 = __dmul_rn(2.0, a2);
    double m[9];
    m[0] = __dadd_rn(num, __dmul_rn(b0, a0)); m[1] = __dsub_rn(__dmul_rn(b0, a1), b2); m[2] = __dadd_rn(__dmul_rn(b0, a2), b1);
    m[3] = __dadd_rn(__dmul_rn(b1, a0), b2); m[4] = __dadd_rn(num, __dmul_rn(b1, a1)); m[5] = __dsub_rn(__dmul_rn(b1, a2), b0);
    m[6] = __dsub_rn(__dmul_rn(b2, a0), b1); m[7] = __dadd_rn(__dmul_rn(b2, a1), b0); m[8] = __dadd_rn(num, __dmul_rn(b2, a2));
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = __ddiv_rn(m[k], den);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = __dadd_rn(__dadd_rn(__dmul_rn(m[3 * i], h.R0[j]), __dmul_rn(m[3 * i + 1], h.R0[3 + j])), __dmul_rn(m[3 * i + 2], h.R0[6 + j]));
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = __dadd_rn(h.t0[k], x[k]);
}

// One thread per particle: particle 0 at x = 0, the others uniform in +-range; v = 0; the personal best is the start, at cost +inf.
__global__ void k_pso_init(PsoParams prm, int HP, PsoState st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HP) return;
    const int p = i % prm.P;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        double x = 0.0;
        if (p > 0) {
            const double u = pso_uniform(prm.seed, pso_counter(0, prm.P, p, d, 0));
            x = __dmul_rn(__dsub_rn(__dmul_rn(2.0, u), 1.0), prm.range[d]);
        }
        st.x[6 * (size_t)i + d] = x;
        st.v[6 * (size_t)i + d] = 0.0;
        st.pbest_x[6 * (size_t)i + d] = x;
    }
    st.pbest_cost[i] = __longlong_as_double(0x7FF0000000000000ll);
}

// One thread per particle: its pose and the camera of its hypothesis' window.
__global__ void k_pso_views(PsoParams prm, int HP, const PsoHyp* __restrict__ hyp, const double* __restrict__ x, ViewParams* __restrict__ views) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HP) return;
    const PsoHyp h = hyp[i / prm.P];
    double xi[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) xi[d] = x[6 * (size_t)i + d];
    ViewParams V;
    pso_pose(xi, h, V.R, V.t);
#pragma unroll
    for (int k = 0; k < 9; ++k) V.K[k] = prm.K[k];
    V.K[2] = __dsub_rn(prm.K[2], (double)h.x0);
    V.K[5] = __dsub_rn(prm.K[5], (double)h.y0);
    views[i] = V;
}

// One workgroup (4 waves) per (hypothesis, particle).  The window's z-buffer keys are one contiguous run, read coalesced; the
// scene window is read row by row (a run of w pixels per row), pixels outside the frame read as 0.  The key is resolved to
// uint16 in registers with k_resolve_depth's rule; sum and n_r are integers, reduced across the lanes of a wave with shuffles
// and across the waves through LDS.
__global__ __launch_bounds__(256) void k_pso_cost(PsoParams prm, const PsoHyp* __restrict__ hyp, const unsigned long long* __restrict__ zbuf,
                                                  const uint16_t* __restrict__ scene, unsigned long long* __restrict__ sum_out,
                                                  unsigned int* __restrict__ nr_out) {
    const int view = blockIdx.x;
    const int x0 = hyp[view / prm.P].x0, y0 = hyp[view / prm.P].y0;
    const int npx = prm.w * prm.h;
    const unsigned long long* Z = zbuf + (size_t)view * npx;
    unsigned int sum = 0, n_r = 0;                                     // a lane sees at most 256 pixels of at most 65535 each
    for (int i = threadIdx.x; i < npx; i += 256) {
        const unsigned long long k = Z[i];
        if (k == ~0ull) continue;
        const float z = __uint_as_float((unsigned int)(k >> 32));
        const int r = z >= 65535.f ? 65535 : (int)(uint16_t)z;
        if (r <= 0) continue;
        const int wy = i / prm.w, wx = i - wy * prm.w;
        const int fx = x0 + wx, fy = y0 + wy;
        int s = 0;
        if (fx >= 0 && fx < prm.W && fy >= 0 && fy < prm.H) s = scene[(size_t)fy * prm.W + fx];
        const int d = r > s ? r - s : s - r;
        sum += (unsigned int)(s == 0 ? prm.tau : min(d, prm.tau));
        n_r += 1u;
    }
    unsigned long long wsum = sum;
    for (int o = 32; o > 0; o >>= 1) {
        wsum += __shfl_down(wsum, o, 64);
        n_r += __shfl_down(n_r, o, 64);
    }
    __shared__ unsigned long long s_sum[4];
    __shared__ unsigned int s_nr[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sum[wave] = wsum; s_nr[wave] = n_r; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum_out[view] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        nr_out[view] = (s_nr[0] + s_nr[1]) + (s_nr[2] + s_nr[3]);
    }
}

// One workgroup per hypothesis, thread p = particle p (P <= 256).  Generation g: the cost of every particle from (sum, n_r, n_0),
// the personal bests, the global best (strictly smaller only; among equal costs of one generation the lower particle), the
// generation's record, then, unless it is the last, the velocity and position update for generation g + 1.  The last one writes
// the result.
__global__ __launch_bounds__(256) void k_pso_step(PsoParams prm, int g, const PsoHyp* __restrict__ hyp, PsoState st) {
    __shared__ double s_cost[256];
    __shared__ int s_idx[256];
    __shared__ double s_gb[6];
    __shared__ int s_n0;
    const int h = blockIdx.x, p = threadIdx.x, P = prm.P, H = gridDim.x;
    const bool active = p < P;
    const size_t i = (size_t)h * P + (active ? p : 0);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    if (p == 0) s_n0 = g == 0 ? (prm.cover_pixels > 0 ? prm.cover_pixels : (int)st.n_r[i]) : st.best[h].n_0;
    __syncthreads();
    const int n0 = s_n0;
    const unsigned long long sum = st.sum[i];
    const unsigned int nr = st.n_r[i];
    double cost = inf;
    if (active && nr > 0u && nr >= (unsigned int)((n0 + 1) / 2)) cost = __ddiv_rn(__ull2double_rn(sum), (double)nr);
    double x[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) x[d] = st.x[6 * i + d];
    double pb_cost = st.pbest_cost[i];
    const bool better = active && cost < pb_cost;
    if (better) {
        pb_cost = cost;
        st.pbest_cost[i] = cost;
#pragma unroll
        for (int d = 0; d < 6; ++d) st.pbest_x[6 * i + d] = x[d];
    }
    s_cost[p] = active ? cost : inf;
    s_idx[p] = p;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (p < s) {
            const double co = s_cost[p + s], cm = s_cost[p];
            const int io = s_idx[p + s], im = s_idx[p];
            if (co < cm || (co == cm && io < im)) { s_cost[p] = co; s_idx[p] = io; }
        }
        __syncthreads();
    }
    if (p == 0) {
        PsoBest b;
        if (g == 0) {
#pragma unroll
            for (int d = 0; d < 6; ++d) b.x[d] = 0.0;
            b.cost = inf; b.initial_cost = cost; b.particle = 0; b.generation = 0; b.n_r = (int)nr; b.n_0 = n0;
        } else b = st.best[h];
        const int bi = s_idx[0];
        if (s_cost[0] < b.cost) {
            b.cost = s_cost[0]; b.particle = bi; b.generation = g; b.n_r = (int)st.n_r[(size_t)h * P + bi];
#pragma unroll
            for (int d = 0; d < 6; ++d) b.x[d] = st.x[6 * ((size_t)h * P + bi) + d];
        }
        st.best[h] = b;
#pragma unroll
        for (int d = 0; d < 6; ++d) s_gb[d] = b.x[d];
        st.rec_best[2 * ((size_t)g * H + h)] = b.particle;
        st.rec_best[2 * ((size_t)g * H + h) + 1] = b.generation;
        if (g == prm.G) {
            PsoResultDev r;
            pso_pose(b.x, hyp[h], r.R, r.t);
            r.cost = b.cost; r.initial_cost = b.initial_cost; r.n_rendered = b.n_r; r.n_initial = b.n_0;
            r.best_particle = b.particle; r.best_generation = b.generation;
            st.result[h] = r;
        }
    }
    __syncthreads();                                                   // s_gb; thread 0 has read the winner's x
    if (!active) return;
    const size_t rec = (size_t)g * H * P + i;
#pragma unroll
    for (int d = 0; d < 6; ++d) st.rec_x[6 * rec + d] = x[d];
    st.rec_cost[rec] = cost; st.rec_sum[rec] = sum; st.rec_nr[rec] = nr;
    if (g == prm.G) return;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const double u1 = pso_uniform(prm.seed, pso_counter(g + 1, P, p, d, 0)), u2 = pso_uniform(prm.seed, pso_counter(g + 1, P, p, d, 1));
        const double pb = better ? x[d] : st.pbest_x[6 * i + d];
        const double cog = __dmul_rn(__dmul_rn(prm.c1, u1), __dsub_rn(pb, x[d]));
        const double soc = __dmul_rn(__dmul_rn(prm.c2, u2), __dsub_rn(s_gb[d], x[d]));
        const double v = __dadd_rn(__dadd_rn(__dmul_rn(prm.inertia, st.v[6 * i + d]), cog), soc);
        double xn = __dadd_rn(x[d], v);
        if (xn > prm.range[d]) xn = prm.range[d];
        if (xn < -prm.range[d]) xn = -prm.range[d];
        st.v[6 * i + d] = v;
        st.x[6 * i + d] = xn;
    }
}

hipError_t launch_pso_init(const PsoParams& p, int H, const PsoState& st, hipStream_t s) {
    const int HP = H * p.P;
    return lm_launch(k_pso_init, dim3((HP + 255) / 256), dim3(256), 0, s, p, HP, st);
}
hipError_t launch_pso_views(const PsoParams& p, int H, const PsoHyp* hyp, const double* x, ViewParams* views, hipStream_t s) {
    const int HP = H * p.P;
    return lm_launch(k_pso_views, dim3((HP + 255) / 256), dim3(256), 0, s, p, HP, hyp, x, views);
}
hipError_t launch_pso_cost(const PsoParams& p, int H, const PsoHyp* hyp, const unsigned long long* zbuf, const uint16_t* scene,
                     unsigned long long* sum, unsigned int* n_r, hipStream_t s) {
    return lm_launch(k_pso_cost, dim3(H * p.P), dim3(256), 0, s, p, hyp, zbuf, scene, sum, n_r);
}
hipError_t launch_pso_step(const PsoParams& p, int H, int g, const PsoHyp* hyp, const PsoState& st, hipStream_t s) {
    return lm_launch(k_pso_step, dim3(H), dim3(256), 0, s, p, g, hyp, st);
}

}  // namespace lm
