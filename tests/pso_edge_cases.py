"""The inputs tests/test_pso_edges_ref.py and tests/test_gpu_pso_edges.py share, and the reference's answers for them (computed once per
process by tests/pso_edges_ref.py).  Mesh, K, the 96 x 80 frame, hypotheses and windows are those of tests/pso_cases.py; the scene is
an edge map made from its depth scene."""
import functools

import numpy as np

import pso_cases as pc
import pso_edges_ref as pe
import render_oracle as ro

M, TAU = 32, 10                                  # max_dist and tau (pixels) of the swarm cases
JUMP = 30                                        # a depth step of the scene (mm) that counts as an edge
OPTIONS = dict(pc.OPTIONS, tau=TAU)


def depth_edges(s, jump=JUMP) -> np.ndarray:
    """The silhouette and the near side of the depth discontinuities of a depth image, as uint8 0 / 1."""
    return pe.contour(s, jump).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def edge_scene():
    """pso_cases.scene()'s depth edges, two clutter lines (one straight through object A, one diagonal), and a band without any edge
    across object C."""
    e = depth_edges(pc.scene())
    e[30, 4:60] = 1
    for i in range(40):
        e[40 + i, 10 + 2 * i] = 1
    e[14:20, 48:96] = 0
    return e


@functools.lru_cache(maxsize=None)
def scene_d2(max_dist=M):
    return pe.distance(edge_scene(), max_dist)


@functools.lru_cache(maxsize=None)
def reference(**options):
    V, F = pc.mesh()
    Rs, ts = pc.hypotheses()
    o = dict(OPTIONS); o.update(options)
    win = o.pop("window_size", pc.WIN)
    return pe.run(V, F, pc.K, scene_d2(), Rs, ts, pc.WINDOWS, win[0], win[1], **o)


# ---- "it refines": chosen on the CPU so that the numpy reference meets the test's conditions (tests/test_pso_edges_ref.py) ------
REFINE = dict(particles=16, generations=6, seed=1, tau=TAU)
REFINE_T0 = pc.T_A + 2.0 * pc.D_T               # hypothesis (a) displaced twice as far: (a) itself starts 1.8 px off, this one 3.6 px


def centre_px(t):
    """The pixel the model origin projects to."""
    t = np.asarray(t, np.float64)
    return np.array([pc.K[0, 0] * t[0] / t[2] + pc.K[0, 2], pc.K[1, 1] * t[1] / t[2] + pc.K[1, 2]])


@functools.lru_cache(maxsize=None)
def refine_reference():
    V, F = pc.mesh()
    Rs, _ = pc.hypotheses()
    return pe.run(V, F, pc.K, scene_d2(), Rs[:1], REFINE_T0[None], pc.WINDOWS[:1], pc.WIN[0], pc.WIN[1], **REFINE)[0]


# ---- evaluate-only: pso_cases' 16 poses against the edges of pose 0's own rendering -----------------------------------------------
E_SLIDE_AT, E_SLIDE_BELOW = -72.20, -72.25      # x offsets (mm) at which n_c is (n_0 + 1) // 2 and one less (found by a scan in 0.05 mm steps)


@functools.lru_cache(maxsize=None)
def eval_edges():
    """The silhouette of pose 0 in the frame, a clutter column through it and a row without edges."""
    V, F = pc.mesh()
    e = depth_edges(ro.render_depth(V, F, pc.K, pc.E_R0, pc.E_T0, pc.W, pc.H)[0], 0)
    e[40:80, 70] = 1
    e[60, :] = 0
    return e


def eval_poses():
    """pso_cases.eval_poses() with 11 and 12 slid until the CONTOUR count is exactly (n_0 + 1) // 2 and one below it."""
    Rs, ts, wins = pc.eval_poses()
    ts = ts.copy()
    ts[11] = pc.E_T0 + np.array([E_SLIDE_AT, 0, 0])
    ts[12] = pc.E_T0 + np.array([E_SLIDE_BELOW, 0, 0])
    return Rs, ts, wins


@functools.lru_cache(maxsize=None)
def eval_reference(edge_step_mm=0):
    """(sum, n_c) of the 16 poses, n_0 = pose 0's n_c, and their costs against that n_0."""
    V, F = pc.mesh()
    Rs, ts, wins = eval_poses()
    d2 = pe.distance(eval_edges(), M)
    terms = [pe.evaluate(V, F, pc.K, d2, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), pc.WIN[0], pc.WIN[1], TAU, edge_step_mm) for i in range(16)]
    n_0 = terms[0][1]
    return terms, n_0, [pe.cost(t[0], t[1], n_0) for t in terms]


# ---- the steps mesh: three fronto-parallel squares whose resolved depths are exact integers -----------------------------------------
STEPS_T = np.array([0.0, 0.0, 400.0])
STEPS_WINDOW, STEPS_WIN = (24, 20), (48, 40)
STEPS = (0, 10, 11, 21)                          # the edge_step_mm values of the test


@functools.lru_cache(maxsize=None)
def steps_mesh():
    """Squares (half side mm, centre x, z offset): the far one 60 wide at +21, a middle one at +10 on its left half, a near one at 0 that
    straddles the middle one's right border, so the rendering has depth jumps of exactly 10 (near to middle), 11 (middle to far) and 21
    (near to far)."""
    V, F = [], []
    for half, cx, cy, z in ((30.0, 0.0, 0.0, 21.0), (18.0, -8.0, 0.0, 10.0), (8.0, 10.0, 2.0, 0.0)):
        n = len(V)
        V += [(cx - half, cy - half, z), (cx + half, cy - half, z), (cx + half, cy + half, z), (cx - half, cy + half, z)]
        F += [(n, n + 1, n + 2), (n, n + 2, n + 3)]
    return np.array(V, np.float32), np.array(F, np.int32)


def steps_render():
    V, F = steps_mesh()
    return pe.render_window(V, F, pc.K, np.eye(3), STEPS_T, STEPS_WINDOW[0], STEPS_WINDOW[1], *STEPS_WIN)


# ---- distance transform cases ------------------------------------------------------------------------------------------------------
EDT_FRAMES = ((1, 1), (1, 300), (300, 1), (67, 45), (300, 70))        # (W, H)
EDT_M = (1, 2, 5, 32)


def exact_d2(E) -> np.ndarray:
    """The squared distance to the nearest edge pixel, not truncated (int64; a large number without an edge)."""
    E = np.asarray(E) != 0
    H, W = E.shape
    ys, xs = np.nonzero(E)
    if not len(ys):
        return np.full((H, W), 1 << 40, np.int64)
    y, x = np.mgrid[0:H, 0:W]
    return ((x[..., None] - xs) ** 2 + (y[..., None] - ys) ** 2).min(-1)


def edt_maps(W, H):
    """name -> uint8 H x W.  'corners': one pixel in each corner; 'pair': two edges equidistant (3 px) from the pixel between them, on
    the middle row; 'random': density 1 / 200."""
    maps = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    c = np.zeros((H, W), np.uint8); c[0, 0] = c[0, W - 1] = c[H - 1, 0] = c[H - 1, W - 1] = 1
    maps["corners"] = c
    p = np.zeros((H, W), np.uint8); p[H // 2, max(W // 2 - 3, 0)] = p[H // 2, min(W // 2 + 3, W - 1)] = 7
    maps["pair"] = p
    o = np.zeros((H, W), np.uint8); o[0, 0] = 1                        # distances M - 1, M, M + 1 along the first row and column
    maps["one"] = o
    maps["random"] = (np.random.default_rng(W * 1000 + H).random((H, W)) < 1.0 / 200.0).astype(np.uint8)
    return maps


DIAGONAL_M = (4, 5, 6)


def diagonal_map():
    """One edge pixel on a 16 x 16 frame: the pixel at offset (3, 4) is at distance exactly 5, which is M + 1, M, M - 1 for M = 4, 5, 6."""
    e = np.zeros((16, 16), np.uint8); e[2, 3] = 1
    return e
