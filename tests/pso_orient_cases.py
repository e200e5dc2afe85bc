"""The inputs tests/test_pso_orient_ref.py and tests/test_gpu_pso_orient.py share, and the reference's answers for them (computed once per
process by tests/pso_orient_ref.py).  Mesh, K, the 96 x 80 frame, hypotheses and windows are those of tests/pso_cases.py, the edge maps
those of tests/pso_edge_cases.py with a bin given to every edge pixel."""
import functools

import numpy as np

import pso_cases as pc
import pso_edge_cases as ec
import pso_orient_ref as po
import render_oracle as ro

M, TAU, P = ec.M, ec.TAU, 16                     # max_dist, tau (pixels) and orient_penalty of the swarm cases
PLANE_M = ec.EDT_M                               # (1, 2, 5, 32)
PLANE_P = (0, 1, 16, 4096)


# ---- the planes ---------------------------------------------------------------------------------------------------------------------------
def with_bins(e) -> np.ndarray:
    """Every edge pixel of e gets the one bin (x + 3 y) % 8."""
    e = np.asarray(e) != 0
    y, x = np.mgrid[0:e.shape[0], 0:e.shape[1]]
    return np.where(e, 1 << ((x + 3 * y) % 8), 0).astype(np.uint8)


def tie_map(W, H):
    """For the pixel q in the middle and bin 2: an edge of bin 3 at distance 3 and one of bin 2 at distance 5, so that with P = 16
    3^2 + 16 x 1^2 == 5^2 exactly.  Along x where the frame is wide enough, else along y; (None, None) on a frame shorter than 11."""
    q = np.zeros((H, W), np.uint8)
    if W >= 11:
        cy, cx = H // 2, W // 2
        q[cy, cx + 3], q[cy, cx - 5] = 1 << 3, 1 << 2
    elif H >= 11:
        cy, cx = H // 2, W // 2
        q[cy + 3, cx], q[cy - 5, cx] = 1 << 3, 1 << 2
    else:
        return None, None
    return q, (cy, cx)


def plane_maps(W, H):
    """name -> uint8 H x W orientation map: pso_edge_cases.edt_maps with bins, one bin per quadrant (1, 3, 5, 7) on a sparse grid,
    pixels with several bits (0x25, 0xFF and 0x81 beside each other), and the tie."""
    maps = {name: with_bins(e) for name, e in ec.edt_maps(W, H).items()}
    y, x = np.mgrid[0:H, 0:W]
    maps["quadrants"] = np.where((x % 5 == 0) & (y % 4 == 0), 1 << (1 + 2 * (x >= W // 2) + 4 * (y >= H // 2)), 0).astype(np.uint8)
    mb = np.zeros((H, W), np.uint8)
    mb[H // 2, W // 2] = 0x25; mb[H // 3, W // 4] = 0xFF; mb[H // 3, min(W // 4 + 1, W - 1)] |= 0x81
    maps["multibit"] = mb
    t, _ = tie_map(W, H)
    if t is not None:
        maps["tie"] = t
    return maps


@functools.lru_cache(maxsize=None)
def uniform_planes(j: int, max_dist=32, orient_penalty=1):
    """The planes of the frame with Q = 1 << j everywhere: DD2[k] = min(M^2, P d(k, j)^2) uniformly, plane 8 is 0."""
    return po.orient_distance(np.full((pc.H, pc.W), 1 << j, np.uint8), max_dist, orient_penalty)


# ---- the orientation of rendered contours, through the uniform scenes ----------------------------------------------------------------------
H_TAU = 32                                       # tau = M = 32, P = 1: a contour pixel of bin k under Q = 1 << j adds d(k, j)^2
SLIVER_T = np.array([0.0, 0.0, 400.0])
CUT_WIN = (24, 24)
CUT_WINDOWS = np.array([[24, 10], [4, 10], [14, 20], [14, 0]], np.int32)    # object A cut by the window's left, right, top and bottom border


@functools.lru_cache(maxsize=None)
def sliver_mesh():
    """A vertical strip 2.8 mm wide and 60 mm high at 400 mm: one pixel wide under K (2.857 mm per pixel), about 21 pixels high."""
    V = [(1.6, -30.0, 0.0), (4.4, -30.0, 0.0), (4.4, 30.0, 0.0), (1.6, 30.0, 0.0)]
    return np.array(V, np.float32), np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def contour_groups():
    """name -> (V, F, Rs, ts, windows, window size, edge_step_mm values): the hypotheses of a group go through one call per step."""
    Vs, Fs = ec.steps_mesh()
    rots = np.stack([np.eye(3), pc.rot((0, 0, 1), 45.0), pc.rot((0, 0, 1), 22.5)])
    V, F = pc.mesh()
    Vl, Fl = sliver_mesh()
    return {
        "steps": (Vs, Fs, rots, np.tile(ec.STEPS_T, (3, 1)), np.tile(np.array(ec.STEPS_WINDOW, np.int32), (3, 1)), ec.STEPS_WIN, ec.STEPS),
        "sliver": (Vl, Fl, np.eye(3)[None], SLIVER_T[None], np.array([ec.STEPS_WINDOW], np.int32), ec.STEPS_WIN, (0,)),
        "cut": (V, F, np.tile(pc.R_A, (4, 1, 1)), np.tile(pc.T_A, (4, 1)), CUT_WINDOWS, CUT_WIN, (0,)),
    }


@functools.lru_cache(maxsize=None)
def contour_render(name, i):
    V, F, Rs, ts, wins, win, _ = contour_groups()[name]
    return po.render_window(V, F, pc.K, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), *win)


def histogram(r, edge_step_mm=0):
    """The number of contour pixels of r per bin 0..7 and without orientation (index 8)."""
    m, k = po.contour_bins(r, edge_step_mm)
    return np.bincount(k[m], minlength=9)


@functools.lru_cache(maxsize=None)
def contour_reference(name, step, j):
    """(sum, n_c) per hypothesis of the group under Q = 1 << j with P = 1, tau = M = 32."""
    V, F, Rs, ts, wins, win, _ = contour_groups()[name]
    dd2 = uniform_planes(j)
    return [po.cost_terms(contour_render(name, i), dd2, int(wins[i][0]), int(wins[i][1]), H_TAU, step) for i in range(len(Rs))]


# ---- the oriented scenes ----------------------------------------------------------------------------------------------------------------
def bins_of_depth_edges(s, jump) -> np.ndarray:
    """The orientation map of a depth image's own edges: pso_edge_cases.depth_edges' pixels, each with the bin the contour rule gives it
    (bin 0 where it gives none)."""
    m, k = po.contour_bins(s, jump)
    return np.where(m, 1 << (k & 7), 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def orient_scene():
    """pso_edge_cases.edge_scene() with bins: the objects' edges with their own, the straight clutter line through object A with bin 4
    (a horizontal line's), the diagonal one with bin 5 (its normal's), the band without edges across object C."""
    q = bins_of_depth_edges(pc.scene(), ec.JUMP)
    q[30, 4:60] = 1 << 4
    for i in range(40):
        q[40 + i, 10 + 2 * i] = 1 << 5
    q[14:20, 48:96] = 0
    assert np.array_equal(q != 0, ec.edge_scene() != 0)
    return q


@functools.lru_cache(maxsize=None)
def scene_planes(orient_penalty=P, max_dist=M):
    return po.orient_distance(orient_scene(), max_dist, orient_penalty)


@functools.lru_cache(maxsize=None)
def reference(orient_penalty=P, **options):
    """The first three hypotheses of pso_cases under pso_edge_cases.OPTIONS."""
    V, F = pc.mesh()
    Rs, ts = pc.hypotheses()
    o = dict(ec.OPTIONS); o.update(options)
    return po.run(V, F, pc.K, scene_planes(orient_penalty), Rs[:3], ts[:3], pc.WINDOWS[:3], pc.WIN[0], pc.WIN[1], **o)


# ---- evaluate-only: pso_edge_cases' 16 poses against pose 0's own oriented contour -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eval_orientations():
    """Pose 0's silhouette in the frame with the bins of the contour rule, a clutter column of bin 4 (perpendicular to a vertical line's
    own bin 0) through it, and a row without edges."""
    V, F = pc.mesh()
    q = bins_of_depth_edges(ro.render_depth(V, F, pc.K, pc.E_R0, pc.E_T0, pc.W, pc.H)[0], 0)
    q[40:80, 70] = 1 << 4
    q[60, :] = 0
    assert np.array_equal(q != 0, ec.eval_edges() != 0)
    return q


@functools.lru_cache(maxsize=None)
def eval_reference():
    """(sum, n_c) of the 16 poses, n_0 = pose 0's n_c, and their costs against that n_0."""
    V, F = pc.mesh()
    Rs, ts, wins = ec.eval_poses()
    dd2 = po.orient_distance(eval_orientations(), M, P)
    terms = [po.evaluate(V, F, pc.K, dd2, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), pc.WIN[0], pc.WIN[1], TAU) for i in range(16)]
    n_0 = terms[0][1]
    return terms, n_0, [po.cost(t[0], t[1], n_0) for t in terms]


# ---- "it helps": chosen on the CPU (a scan of clutter columns and seeds) so that the numpy reference under cost="oriented" ends nearer the
# planted pose than the numpy reference under cost="edges" (tests/test_pso_orient_ref.py asserts it of the two references) -------------------
HELPS_COLUMN, HELPS_SEED = 38, 1
HELPS = dict(ec.REFINE, seed=HELPS_SEED)


@functools.lru_cache(maxsize=None)
def helps_scene():
    """Object A's own oriented edges and a vertical clutter line of bin 4 (foreign to the contour's right side, which it runs along two
    pixels inside) through the object at column HELPS_COLUMN."""
    V, F = pc.mesh()
    q = bins_of_depth_edges(ro.render_depth(V, F, pc.K, pc.R_A, pc.T_A, pc.W, pc.H)[0], 0)
    q[2:44, HELPS_COLUMN] = 1 << 4
    return q


@functools.lru_cache(maxsize=None)
def helps_references():
    """(the oriented reference, the edges reference) of hypothesis (a) displaced by 2 D_T on helps_scene()."""
    V, F = pc.mesh()
    Rs, _ = pc.hypotheses()
    args = (Rs[:1], ec.REFINE_T0[None], pc.WINDOWS[:1], pc.WIN[0], pc.WIN[1])
    q = helps_scene()
    return (po.run(V, F, pc.K, po.orient_distance(q, M, P), *args, **HELPS)[0],
            po.pe.run(V, F, pc.K, po.pe.distance(q != 0, M), *args, **HELPS)[0])


# ---- the hand-over -------------------------------------------------------------------------------------------------------------------------
HAND_SIZE = (160, 160)
HAND_K = np.array([200.0, 0, 80.0, 0, 200.0, 80.0, 0, 0, 1], np.float64).reshape(3, 3)
