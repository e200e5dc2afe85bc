"""The particle-swarm pose refiner of 6dpose_amd/csrc/pso.hip, stated in numpy — TEST INFRASTRUCTURE ONLY.  This file IS the
definition of the refiner; the device is held to it bit for bit (tests/test_gpu_pso.py).  Everything that is
not an integer is float64, one rounding per + - * / in the order written here, no fused operations.

A particle is x = (dt[3] mm, a[3]); a is a Cayley rotation vector, dR(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a).  Its pose is
R = dR(a) R0, t = t0 + dt.  It is rendered depth-only (oracle/render_oracle.py) into the w x h window of the frame at (x0, y0), i.e.
with the camera K whose cx, cy are cx - x0, cy - y0, and scored against the scene depth of that window (0 outside the frame).

Random numbers: uniform(seed, counter) with counter = ((g P + p) 6 + d) 2 + draw.  g = 0, draw 0: the initial position of particle
p > 0 in dimension d; generation g >= 1: draw 0 is u1, draw 1 is u2.  The hypothesis is not part of the counter: two hypotheses with
the same inputs run the same swarm."""
import numpy as np

import render_oracle as ro

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
# the first three outputs of splitmix64 seeded with 0 (Vigna's splitmix64.c): counters 0, 1, 2 at seed 0
KNOWN_ANSWERS = ((0, 0, 0xE220A8397B1DCDAF), (0, 1, 0x6E789E6AA1B965F4), (0, 2, 0x06C45D188009454F))
DEFAULTS = dict(particles=64, generations=30, tau=20, cover_pixels=0, seed=0, trans_range_mm=20.0, rot_range=float(np.tan(np.radians(10.0) / 2.0)),
                inertia=0.7298, c1=1.49618, c2=1.49618, clip_near=10.0, clip_far=10000.0)


def mix(seed: int, counter: int) -> int:
    """The splitmix64 finaliser of seed + GOLDEN (1 + counter), 64-bit."""
    z = (seed + GOLDEN * (1 + counter)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def uniform(seed: int, counter: int) -> float:
    return float(mix(seed, counter) >> 11) * 2.0 ** -53


def counter(g: int, P: int, p: int, d: int, draw: int) -> int:
    return ((g * P + p) * 6 + d) * 2 + draw


def cayley(a) -> np.ndarray:
    a0, a1, a2 = (np.float64(v) for v in a)
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    den, num = 1.0 + aa, 1.0 - aa
    b0, b1, b2 = 2.0 * a0, 2.0 * a1, 2.0 * a2
    m = np.array([[num + b0 * a0, b0 * a1 - b2, b0 * a2 + b1],
                  [b1 * a0 + b2, num + b1 * a1, b1 * a2 - b0],
                  [b2 * a0 - b1, b2 * a1 + b0, num + b2 * a2]], np.float64)
    return m / den


def particle_pose(R0, t0, x):
    """(R, t) of particle x for the hypothesis (R0, t0)."""
    R0 = np.asarray(R0, np.float64).reshape(3, 3); t0 = np.asarray(t0, np.float64).reshape(3); x = np.asarray(x, np.float64)
    m = cayley(x[3:])
    R = np.empty((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            R[i, j] = (m[i, 0] * R0[0, j] + m[i, 1] * R0[1, j]) + m[i, 2] * R0[2, j]
    return R, t0 + x[:3]


def window_K(K, x0: int, y0: int) -> np.ndarray:
    Kw = np.array(K, np.float64).reshape(3, 3).copy()
    Kw[0, 2] = Kw[0, 2] - float(x0)
    Kw[1, 2] = Kw[1, 2] - float(y0)
    return Kw


def window_scene(scene, x0: int, y0: int, w: int, h: int) -> np.ndarray:
    """The scene depth of the window, 0 where it leaves the frame."""
    H, W = scene.shape
    out = np.zeros((h, w), np.uint16)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, W), max(y0, 0), min(y0 + h, H)
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = scene[ya:yb, xa:xb]
    return out


def render_window(V, F, K, R, t, x0, y0, w, h, clip_near=10.0, clip_far=10000.0) -> np.ndarray:
    return ro.render_depth(V, F, window_K(K, x0, y0), R, t, w, h, clip_near, clip_far)[0]


def cost_terms(r, s, tau: int):
    """(sum, n_r) of a rendered window r against the scene window s, in integers."""
    r = np.asarray(r).astype(np.int64); s = np.asarray(s).astype(np.int64)
    m = r > 0
    per = np.where(s == 0, tau, np.minimum(np.abs(r - s), tau))
    return int(per[m].sum()), int(m.sum())


def cost(total: int, n_r: int, n_0: int) -> float:
    if n_r > 0 and n_r >= (n_0 + 1) // 2:
        return float(np.float64(total) / np.float64(n_r))
    return float("inf")


def evaluate(V, F, K, scene, R, t, x0, y0, w, h, tau=20, clip_near=10.0, clip_far=10000.0):
    return cost_terms(render_window(V, F, K, R, t, x0, y0, w, h, clip_near, clip_far), window_scene(scene, x0, y0, w, h), tau)


def run(V, F, K, scene, Rs, ts, windows, w, h, **options):
    """The whole call.  Returns one dict per hypothesis: x [G + 1][P][6], cost [G + 1][P], sum and n_r [G + 1][P] (int64), best [G + 1][2]
    (particle, generation of the global best after each generation) and the result fields R, t, cost, initial_cost, n_rendered,
    n_initial, best_particle, best_generation."""
    o = dict(DEFAULTS); o.update(options)
    G, seed, tau = int(o["generations"]), int(o["seed"]), int(o["tau"])
    P = 1 if G == 0 else int(o["particles"])                 # evaluate-only: the given pose alone
    rng = np.array([o["trans_range_mm"]] * 3 + [o["rot_range"]] * 3, np.float64)
    wi, c1, c2 = np.float64(o["inertia"]), np.float64(o["c1"]), np.float64(o["c2"])
    Rs = np.asarray(Rs, np.float64).reshape(-1, 3, 3); ts = np.asarray(ts, np.float64).reshape(-1, 3)
    x_init = np.zeros((P, 6), np.float64)
    for p in range(1, P):
        for d in range(6):
            x_init[p, d] = (2.0 * uniform(seed, counter(0, P, p, d, 0)) - 1.0) * rng[d]
    out = []
    for hyp in range(len(Rs)):
        x0, y0 = int(windows[hyp][0]), int(windows[hyp][1])
        sw = window_scene(scene, x0, y0, w, h)
        x, v = x_init.copy(), np.zeros((P, 6), np.float64)
        pb_x, pb_c = x.copy(), np.full(P, np.inf)
        gb_x, gb_c, gb_p, gb_g, gb_n = np.zeros(6, np.float64), np.inf, 0, 0, 0
        rec = dict(x=np.zeros((G + 1, P, 6)), cost=np.zeros((G + 1, P)), sum=np.zeros((G + 1, P), np.int64), n_r=np.zeros((G + 1, P), np.int64),
                   best=np.zeros((G + 1, 2), np.int64))
        n_0 = initial = None
        for g in range(G + 1):
            for p in range(P):
                R, t = particle_pose(Rs[hyp], ts[hyp], x[p])
                rec["sum"][g, p], rec["n_r"][g, p] = cost_terms(render_window(V, F, K, R, t, x0, y0, w, h, o["clip_near"], o["clip_far"]), sw, tau)
            if g == 0:
                n_0 = int(o["cover_pixels"]) if int(o["cover_pixels"]) > 0 else int(rec["n_r"][0, 0])
                gb_n = int(rec["n_r"][0, 0])
            for p in range(P):
                c = cost(int(rec["sum"][g, p]), int(rec["n_r"][g, p]), n_0)
                rec["cost"][g, p] = c
                if c < pb_c[p]:
                    pb_c[p], pb_x[p] = c, x[p]
            if g == 0:
                initial = rec["cost"][0, 0]
            for p in range(P):                                # strictly smaller: the earlier generation, then the lower particle, keeps a tie
                if rec["cost"][g, p] < gb_c:
                    gb_c, gb_x, gb_p, gb_g, gb_n = rec["cost"][g, p], x[p].copy(), p, g, int(rec["n_r"][g, p])
            rec["x"][g] = x
            rec["best"][g] = (gb_p, gb_g)
            if g == G:
                break
            for p in range(P):
                for d in range(6):
                    u1, u2 = uniform(seed, counter(g + 1, P, p, d, 0)), uniform(seed, counter(g + 1, P, p, d, 1))
                    vn = (wi * v[p, d] + (c1 * u1) * (pb_x[p, d] - x[p, d])) + (c2 * u2) * (gb_x[d] - x[p, d])
                    xn = x[p, d] + vn
                    xn = rng[d] if xn > rng[d] else xn
                    xn = -rng[d] if xn < -rng[d] else xn
                    v[p, d], x[p, d] = vn, xn
        R, t = particle_pose(Rs[hyp], ts[hyp], gb_x)
        rec.update(R=R, t=t, final_cost=float(gb_c), initial_cost=float(initial), n_rendered=gb_n, n_initial=n_0, best_particle=gb_p, best_generation=gb_g)
        out.append(rec)
    return out
