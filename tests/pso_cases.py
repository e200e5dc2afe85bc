"""The inputs tests/test_pso_ref.py and tests/test_gpu_pso.py share, and the reference's answers for them (computed once per
process by tests/pso_ref.py).  The mesh is the 80-triangle icosphere of radius 40 mm, the frame 96 x 80, the window 48 x 40."""
import functools

import numpy as np

import pso_ref
import render_oracle as ro
from synth import icosphere

W, H = 96, 80
WIN = (48, 40)
K = np.array([140.0, 0, 48.0, 0, 140.0, 40.0, 0, 0, 1], np.float64).reshape(3, 3)
P, G, SEED, TAU = 8, 4, 7, 20
OPTIONS = dict(particles=P, generations=G, seed=SEED, tau=TAU)


def rot(axis, deg):
    """Rodrigues; test input only, the refiner itself never needs sin / cos."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return c * np.eye(3) + s * X + (1 - c) * np.outer(a, a)


@functools.lru_cache(maxsize=None)
def mesh():
    V, F, _, _ = icosphere(1, radius=40.0, seed=5)
    return V, F


def centre_t(u, v, z):
    """The translation that puts the model origin at pixel (u, v), depth z."""
    return np.array([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z], np.float64)


# planted poses: A top left, B bottom right (its window hangs over the frame's right and bottom edge), C top right
R_A, T_A = rot((1, 2, 3), 25.0), centre_t(26, 22, 400.0)
R_B, T_B = rot((3, -1, 2), -40.0), centre_t(80, 66, 395.0)
R_C, T_C = rot((-2, 1, 1), 70.0), centre_t(72, 22, 410.0)
D_ROT, D_T = rot((2, -1, 1), 4.0), np.array([4.0, -3.0, 3.3])          # the start is 4 degrees and 6 mm off
WINDOWS = np.array([[2, 2], [56, 46], [48, 2], [2, 2]], np.int32)


@functools.lru_cache(maxsize=None)
def scene():
    """The three planted objects; around C a band of zeros (sensor holes) and an occluder 100 mm in front over a third of it."""
    V, F = mesh()
    s = np.zeros((H, W), np.uint16)
    for R, t in ((R_A, T_A), (R_B, T_B), (R_C, T_C)):
        d = ro.render_depth(V, F, K, R, t, W, H)[0]
        s = np.where((d > 0) & ((s == 0) | (d < s)), d, s).astype(np.uint16)
    s[18:21, 48:96] = 0
    s[0:44, 78:90] = 310
    return s


def hypotheses():
    """(a) a clean start, (b) its window over the frame edge, (c) holes and an occluder, (d) = (a)."""
    Rs = np.stack([D_ROT @ R_A, D_ROT @ R_B, D_ROT @ R_C, D_ROT @ R_A])
    ts = np.stack([T_A + D_T, T_B + D_T, T_C + D_T, T_A + D_T])
    return Rs, ts


PLANTED_T = np.stack([T_A, T_B, T_C, T_A])


@functools.lru_cache(maxsize=None)
def reference(**options):
    V, F = mesh()
    Rs, ts = hypotheses()
    o = dict(OPTIONS); o.update(options)
    win = o.pop("window_size", WIN)
    return pso_ref.run(V, F, K, scene(), Rs, ts, WINDOWS, win[0], win[1], **o)


# ---- evaluate-only: 16 hand-placed poses against a scene made from pose 0's own rendering -------------------------------------
E_WINDOW = (52, 42)                             # hangs over the frame's right and bottom edge by 4 and 2 pixels
E_R0, E_T0 = rot((1, 1, 0), 15.0), centre_t(76, 62, 400.0)
E_SLIDE_AT, E_SLIDE_BELOW = -70.55, -70.65      # x offsets (mm) at which n_r is (n_0 + 1) // 2 and one less (found by a scan in 0.05 mm steps)


def eval_scene():
    """Pose 0's rendering with a column pattern of offsets: 0, +tau, +(tau - 1), +(tau + 1), -tau, 65535, and a row of holes."""
    V, F = mesh()
    base = ro.render_depth(V, F, K, E_R0, E_T0, W, H)[0].astype(np.int64)
    off = np.array([0, TAU, TAU - 1, TAU + 1, -TAU, 0])[np.arange(W) % 6][None, :]
    s = np.where(base > 0, base + off, 0)
    s[:, 5::6] = np.where(base[:, 5::6] > 0, 65535, 0)
    s[60, :] = 0
    return s.astype(np.uint16)


def eval_poses():
    """16 poses and their windows.  0: the scene's own pose; 10: behind the far plane (renders nothing); 11, 12: slid out of the window
    until n_r is exactly (n_0 + 1) // 2 and one below it; 13-15: pushed across the frame's edge, where the scene reads 0."""
    ts = [E_T0 + np.array(d, np.float64) for d in ([0, 0, 0], [3, 0, 0], [0, -4, 0], [0, 0, 12], [0, 0, -19], [5, 5, 25], [-7, 2, 40], [1, 1, 1],
                                                   [10, -10, 0], [0, 0, 100], [0, 0, 20000], [E_SLIDE_AT, 0, 0], [E_SLIDE_BELOW, 0, 0], [15, 0, 0],
                                                   [0, 12, 0], [20, 18, -5])]
    Rs = [E_R0 if i not in (5, 6, 8) else rot((0, 1, 1), 3.0 * i) @ E_R0 for i in range(16)]
    return np.stack(Rs), np.array(ts, np.float64), np.tile(np.array(E_WINDOW, np.int32), (16, 1))


@functools.lru_cache(maxsize=None)
def eval_reference():
    """(sum, n_r) of the 16 poses, n_0 = pose 0's n_r, and their costs against that n_0."""
    V, F = mesh()
    Rs, ts, wins = eval_poses()
    s = eval_scene()
    terms = [pso_ref.evaluate(V, F, K, s, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), WIN[0], WIN[1], TAU) for i in range(16)]
    n_0 = terms[0][1]
    return terms, n_0, [pso_ref.cost(t[0], t[1], n_0) for t in terms]
