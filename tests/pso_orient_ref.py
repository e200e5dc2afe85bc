"""The directional chamfer cost of the particle-swarm refiner, 6dpose_amd/csrc/pso_orient.hip, stated in numpy — TEST INFRASTRUCTURE ONLY.
This file IS the definition of that cost; the device is held to it bit for bit (tests/test_gpu_pso_orient.py).  The
swarm, its random numbers, the bests, the records, render_window, cost and the cover floor are those of tests/pso_ref.py, the contour
pixels those of tests/pso_edges_ref.py; only the plane a contour pixel reads changes.  Everything below is an integer.

Scene Q: uint8 H x W, bit k (0..7) set = an edge of orientation bin k (LINE-MOD's quantised colour gradients; several bits may be set),
0 = no edge.  With E_k = (Q >> k) & 1, M = max_dist (1..255), P = orient_penalty (0..4096 px^2 per bin^2) and the circular bin distance
d(k, j) = min(|k - j|, 8 - |k - j|):  D2_j = pso_edges_ref.distance(E_j, M);  DD2[k] = min(M^2, min over j of D2_j + P d(k, j)^2) for
k = 0..7, the truncated squared distance in (x, y, sqrt(P) bin) to the nearest oriented edge;  DD2[8] = min over j of D2_j, the
undirected plane pso_edges_ref.distance(Q != 0, M).

A contour pixel p (pso_edges_ref.contour) with resolved depth r_p looks at its 8 neighbours: o(n) = 1 iff n lies inside the window and
r_n == 0 or (edge_step_mm > 0 and r_n - r_p > edge_step_mm), else 0.  gx, gy are the 3 x 3 Sobel sums of o (x kernel [-1 0 1; -2 0 2;
-1 0 1], y kernel its transpose, y downwards), both in -4..4.  gx == gy == 0: no orientation, the pixel reads plane 8.  Otherwise
k_p = round(atan2(gy, gx) in degrees mod 360 * 16 / 360) & 7, the front end's own quantisation, taken from the 81-entry table BIN_OF.
The pixel adds min(DD2[k_p][fy][fx], tau^2), tau^2 outside the frame; n_c counts contour pixels and is used as in pso_edges_ref."""
import numpy as np

import pso_edges_ref as pe
import pso_ref
from pso_edges_ref import DEFAULTS, contour, cost, render_window, window_distance  # noqa: F401  (the parts that do not change)

MAX_DIST = 32
ORIENT_PENALTY = 16                              # a choice, not a measurement: one bin off costs as much as 4 px
MARGIN_DEG = 0.05                                # every (gx, gy) is at least this far from a bin boundary


def bin_distance(k: int, j: int) -> int:
    d = abs(int(k) - int(j))
    return min(d, 8 - d)


def _bin_table():
    """((gy + 4, gx + 4) -> bin as uint8 9 x 9, 8 at (0, 0); the smallest distance in degrees of an entry from a bin boundary)."""
    t = np.full((9, 9), 8, np.uint8)
    margin = np.inf
    for gy in range(-4, 5):
        for gx in range(-4, 5):
            if gx == 0 and gy == 0:
                continue
            s = (np.degrees(np.arctan2(np.float64(gy), np.float64(gx))) % 360.0) * 16.0 / 360.0
            margin = min(margin, abs(s - np.floor(s) - 0.5) * 22.5)
            t[gy + 4, gx + 4] = int(np.rint(s)) & 7
    return t, float(margin)


BIN_OF, BIN_MARGIN_DEG = _bin_table()
assert BIN_MARGIN_DEG >= MARGIN_DEG, BIN_MARGIN_DEG     # so any correct evaluation of atan2 gives this table


def channel_distances(Q, max_dist: int = MAX_DIST) -> np.ndarray:
    """D2_j, j = 0..7: int64 8 x H x W."""
    Q = np.asarray(Q)
    assert Q.dtype == np.uint8 and Q.ndim == 2
    return np.stack([pe.distance((Q >> j) & 1, max_dist).astype(np.int64) for j in range(8)])


def orient_distance(Q, max_dist: int = MAX_DIST, orient_penalty: int = ORIENT_PENALTY) -> np.ndarray:
    """DD2: uint16 9 x H x W."""
    M, P = int(max_dist), int(orient_penalty)
    assert 1 <= M <= 255 and 0 <= P <= 4096
    d2 = channel_distances(Q, M)
    out = np.empty((9,) + d2.shape[1:], np.int64)
    for k in range(8):
        out[k] = np.minimum(M * M, np.min([d2[j] + P * bin_distance(k, j) ** 2 for j in range(8)], axis=0))
    out[8] = d2.min(0)
    return out.astype(np.uint16)


def orient_distance_brute(Q, max_dist: int = MAX_DIST, orient_penalty: int = ORIENT_PENALTY) -> np.ndarray:
    """The definition itself: every pixel and bin against every oriented edge pixel, in (x, y, sqrt(P) bin)."""
    Q = np.asarray(Q)
    H, W = Q.shape
    M, P = int(max_dist), int(orient_penalty)
    ex, ey, ej = [], [], []
    for j in range(8):
        ys, xs = np.nonzero((Q >> j) & 1)
        ex += list(xs); ey += list(ys); ej += [j] * len(ys)
    ex, ey, ej = np.array(ex, np.int64), np.array(ey, np.int64), np.array(ej, np.int64)
    out = np.full((9, H, W), M * M, np.int64)
    if not len(ex):
        return out.astype(np.uint16)
    pen = np.array([[P * bin_distance(k, j) ** 2 for j in range(8)] for k in range(8)] + [[0] * 8], np.int64)
    for y in range(H):
        for x in range(W):
            flat = (ex - x) ** 2 + (ey - y) ** 2
            for k in range(9):
                out[k, y, x] = min(M * M, int((flat + pen[k][ej]).min()))
    return out.astype(np.uint16)


def sobel_of_outside(r, edge_step_mm: int = 0):
    """(gx, gy): int64 h x w, the Sobel sums of o around every pixel of the rendered window r."""
    r = np.asarray(r).astype(np.int64)
    step = int(edge_step_mm)
    assert 0 <= step <= 65535
    h, w = r.shape
    gx, gy = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ya, yb, xa, xb = max(0, -dy), h - max(0, dy), max(0, -dx), w - max(0, dx)      # the pixels whose neighbour is inside the window
            here, there = r[ya:yb, xa:xb], r[ya + dy:yb + dy, xa + dx:xb + dx]
            o = there == 0
            if step > 0:
                o = o | (there - here > step)
            gx[ya:yb, xa:xb] += o * (dx * (2 if dy == 0 else 1))
            gy[ya:yb, xa:xb] += o * (dy * (2 if dx == 0 else 1))
    return gx, gy


def contour_bins(r, edge_step_mm: int = 0):
    """(the contour pixels, bool h x w; k_p, uint8 h x w: 0..7, 8 = no orientation, meaningful on the contour only)."""
    gx, gy = sobel_of_outside(r, edge_step_mm)
    return contour(r, edge_step_mm), BIN_OF[gy + 4, gx + 4]


def window_planes(DD2, x0: int, y0: int, w: int, h: int, tau: int) -> np.ndarray:
    """min(DD2, tau^2) of the window for the nine planes, int64 9 x h x w, tau^2 where it leaves the frame."""
    return np.stack([window_distance(DD2[k], x0, y0, w, h, tau) for k in range(9)])


def plane_terms(r, dw, edge_step_mm: int = 0):
    """(sum, n_c) of a rendered window r against its window planes dw."""
    m, k = contour_bins(r, edge_step_mm)
    ys, xs = np.nonzero(m)
    return int(dw[k[ys, xs], ys, xs].sum()), int(m.sum())


def cost_terms(r, DD2, x0: int, y0: int, tau: int, edge_step_mm: int = 0):
    """(sum, n_c) of a rendered window r whose origin in the frame is (x0, y0), in integers."""
    r = np.asarray(r)
    return plane_terms(r, window_planes(DD2, int(x0), int(y0), r.shape[1], r.shape[0], tau), edge_step_mm)


def evaluate(V, F, K, DD2, R, t, x0, y0, w, h, tau=20, edge_step_mm=0, clip_near=10.0, clip_far=10000.0):
    return cost_terms(render_window(V, F, K, R, t, x0, y0, w, h, clip_near, clip_far), DD2, x0, y0, tau, edge_step_mm)


def run(V, F, K, DD2, Rs, ts, windows, w, h, edge_step_mm=0, **options):
    """pso_edges_ref.run with the nine planes DD2 = orient_distance(Q, max_dist, orient_penalty) in D2's place: pso_ref.run's own lines,
    run with its two cost hooks exchanged for the call."""
    tau = int(dict(DEFAULTS, **options)["tau"])
    saved = pso_ref.window_scene, pso_ref.cost_terms
    pso_ref.window_scene = lambda dd2, x0, y0, ww, hh: window_planes(dd2, x0, y0, ww, hh, tau)
    pso_ref.cost_terms = lambda r, dw, _tau: plane_terms(r, dw, edge_step_mm)
    try:
        return pso_ref.run(V, F, K, DD2, Rs, ts, windows, w, h, **options)
    finally:
        pso_ref.window_scene, pso_ref.cost_terms = saved
