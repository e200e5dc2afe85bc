"""The edge (chamfer) cost of the particle-swarm refiner, 6dpose_amd/csrc/pso_edges.hip, stated in numpy — TEST INFRASTRUCTURE ONLY.
This file IS the definition of that cost; the device is held to it bit for bit (tests/test_gpu_pso_edges.py).  The
swarm, its random numbers, the bests and the records are those of tests/pso_ref.py; only (sum, n_r) of a particle change, to (sum, n_c).

Edge map E: uint8 H x W, a pixel is an edge where E != 0.  D2: uint16 H x W, the squared distance in pixels to the nearest edge pixel,
truncated at M = max_dist (1..255): D2 = min(M^2, min (x - x')^2 + (y - y')^2), M^2 everywhere without an edge.  Stated separably:
g[y, x] = min(M, the distance to the nearest edge of row y), D2[y, x] = min(M^2, min over |dy| < M of g[y + dy, x]^2 + dy^2).

A particle's window is rendered as in pso_ref (depth r, uint16).  A pixel is a contour pixel iff r > 0 and one of its four neighbours n
inside the window has n == 0 or, with edge_step_mm > 0, n - r > edge_step_mm (the near side of a depth jump).  Neighbours outside the
window are ignored.  A contour pixel at frame position (fx, fy) adds min(D2[fy, fx], tau^2), tau^2 outside the frame; n_c counts them.
cost = sum / n_c (px^2) under pso_ref.cost's cover floor with n_0 the given pose's n_c."""
import numpy as np

import pso_ref
from pso_ref import DEFAULTS, cost, counter, particle_pose, render_window, uniform  # noqa: F401  (the swarm's parts, unchanged)

MAX_DIST = 32


def row_distance(E, max_dist: int = MAX_DIST) -> np.ndarray:
    """g: uint8 H x W, min(M, |x - x'| over the edge pixels x' of the row)."""
    E = np.asarray(E) != 0
    H, W = E.shape
    M = int(max_dist)
    assert 1 <= M <= 255
    g = np.full((H, W), M, np.int64)
    for d in range(min(M, W)):
        hit = np.zeros((H, W), bool)
        hit[:, d:] |= E[:, :W - d]
        hit[:, :W - d] |= E[:, d:]
        g = np.where(hit & (g > d), d, g)
    return g.astype(np.uint8)


def distance(E, max_dist: int = MAX_DIST) -> np.ndarray:
    """D2: uint16 H x W, the truncated squared distance to the nearest edge pixel."""
    M = int(max_dist)
    g = row_distance(E, M).astype(np.int64)
    H, W = g.shape
    g2 = g * g
    d2 = np.full((H, W), M * M, np.int64)
    for dy in range(-min(M - 1, H - 1), min(M - 1, H - 1) + 1):
        ya, yb = max(0, -dy), min(H, H - dy)                       # rows y with y + dy inside the frame
        d2[ya:yb] = np.minimum(d2[ya:yb], g2[ya + dy:yb + dy] + dy * dy)
    return d2.astype(np.uint16)


def distance_brute(E, max_dist: int = MAX_DIST) -> np.ndarray:
    """The definition itself: every pixel against every edge pixel."""
    E = np.asarray(E) != 0
    H, W = E.shape
    M = int(max_dist)
    ys, xs = np.nonzero(E)
    out = np.full((H, W), M * M, np.int64)
    for y in range(H):
        for x in range(W):
            if len(ys):
                out[y, x] = min(M * M, int(((xs - x) ** 2 + (ys - y) ** 2).min()))
    return out.astype(np.uint16)


def contour(r, edge_step_mm: int = 0) -> np.ndarray:
    """The contour pixels (bool h x w) of a rendered window r."""
    r = np.asarray(r).astype(np.int64)
    step = int(edge_step_mm)
    assert 0 <= step <= 65535
    h, w = r.shape
    out = np.zeros((h, w), bool)

    def mark(here, there):                                       # here, there: views of r, a pixel and its neighbour
        m = there == 0
        if step > 0:
            m = m | (there - here > step)
        return m

    out[:, 1:] |= mark(r[:, 1:], r[:, :-1])
    out[:, :-1] |= mark(r[:, :-1], r[:, 1:])
    out[1:, :] |= mark(r[1:, :], r[:-1, :])
    out[:-1, :] |= mark(r[:-1, :], r[1:, :])
    return out & (r > 0)


def window_distance(D2, x0: int, y0: int, w: int, h: int, tau: int) -> np.ndarray:
    """min(D2, tau^2) of the window as int64, tau^2 where it leaves the frame."""
    D2 = np.asarray(D2)
    H, W = D2.shape
    t2 = int(tau) * int(tau)
    out = np.full((h, w), t2, np.int64)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, W), max(y0, 0), min(y0 + h, H)
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = np.minimum(D2[ya:yb, xa:xb].astype(np.int64), t2)
    return out


def cost_terms(r, D2, x0: int, y0: int, tau: int, edge_step_mm: int = 0):
    """(sum, n_c) of a rendered window r whose origin in the frame is (x0, y0), in integers."""
    m = contour(r, edge_step_mm)
    return int(window_distance(D2, int(x0), int(y0), m.shape[1], m.shape[0], tau)[m].sum()), int(m.sum())


def evaluate(V, F, K, D2, R, t, x0, y0, w, h, tau=20, edge_step_mm=0, clip_near=10.0, clip_far=10000.0):
    return cost_terms(render_window(V, F, K, R, t, x0, y0, w, h, clip_near, clip_far), D2, x0, y0, tau, edge_step_mm)


def run(V, F, K, D2, Rs, ts, windows, w, h, edge_step_mm=0, **options):
    """pso_ref.run with the edge cost terms: D2 = distance(E, max_dist) takes the scene depth's place and n_r reads n_c; the swarm, the
    random numbers, the bests and the record are pso_ref.run's own lines, run with its two cost hooks exchanged for the call."""
    tau = int(dict(DEFAULTS, **options)["tau"])

    def terms(r, dw, _tau):
        m = contour(r, edge_step_mm)
        return int(dw[m].sum()), int(m.sum())

    saved = pso_ref.window_scene, pso_ref.cost_terms
    pso_ref.window_scene, pso_ref.cost_terms = (lambda d2, x0, y0, ww, hh: window_distance(d2, x0, y0, ww, hh, tau)), terms
    try:
        return pso_ref.run(V, F, K, D2, Rs, ts, windows, w, h, **options)
    finally:
        pso_ref.window_scene, pso_ref.cost_terms = saved
