"""Named, seeded inputs for the pixel passes of the pose errors (k_vsd, k_gt_stats) and for every chunked path of csrc/pose_error.cpp, with
the numpy oracle's answers (tests/pose_error_ref.py, tests/pose_sym_ref.py, fed with the rasteriser's numpy twin oracle/render_oracle.py).
Shared by tests/test_pose_pixel_cases.py (CPU: the cases hold what they claim) and tests/test_gpu_pose_pixels.py (the library).

The mesh is the 80-triangle icosphere of pso_cases.mesh() (42 vertices, radius 40 mm), so one numpy render costs milliseconds.  Every builder is
cached; treat what it returns as read-only.

Constants of csrc/pose_error.cpp and csrc/pose_error.hip the chunk sizes are derived from (tests/test_pose_pixel_cases.py reads them back from
the sources, so a change there fails loudly instead of quietly un-testing a path):

    kZbufBudget = 512 MiB, 8 bytes of z-buffer per pixel     views_per_render(W, H) = max(2, min(256, 512 MiB / (8 W H)))
    kMaxViewsPerRender = 256                                 n_gt + n_est > cap: gch = min(n_gt, max(1, cap / 2)), ech = min(n_est, cap - gch)
    kMaxPtsPairs = 16384                                     pairs per k_pose_pts / k_pose_sym launch
    kSymPartialBudget = 256 MiB, kSymThreads = 256           batch = max(1, min(16384, (256 MiB / 8) / (chunks * nm * n_sym)))
    kPixThreads = 256, 4 pixels per lane, at most 128 blocks pix_blocks(npx) = clamp(ceil(npx / 1024), 1, 128)
"""
import functools
import math

import numpy as np

import pose_error_ref as per
import pose_sym_ref as psr
import pso_cases
import render_oracle as ro
import synth

ZBUF_BUDGET = 512 << 20
MAX_VIEWS_PER_RENDER = 256
MAX_PTS_PAIRS = 16384
SYM_PARTIAL_BUDGET = 256 << 20
SYM_THREADS = 256
PIX_THREADS = 256
PIX_PER_LANE = 4
MAX_PIX_BLOCKS = 128

rot = pso_cases.rot
mesh = pso_cases.mesh
F32 = np.float32
Z0 = 400.0                                        # the usual object distance: the blob spans about 355 .. 445 mm


# ---- the host's arithmetic, restated ---------------------------------------------------------------------------------------------------------
def views_per_render(W, H):
    return max(2, min(MAX_VIEWS_PER_RENDER, ZBUF_BUDGET // (8 * W * H)))


def pix_blocks(npx):
    return max(1, min(MAX_PIX_BLOCKS, -(-npx // (PIX_PER_LANE * PIX_THREADS))))


def chunks_of(n, size):
    """[(offset, count)] of a loop `for (o = 0; o < n; o += size)`."""
    return [(o, min(size, n - o)) for o in range(0, n, size)]


def vsd_chunking(n_est, n_gt, W, H):
    """(gch, ech) of lm_mesh_pose_errors: the GT and estimate chunk sizes of the render loops."""
    cap = views_per_render(W, H)
    gch, ech = n_gt, n_est
    if n_gt + n_est > cap:
        gch = min(n_gt, max(1, cap // 2))
        ech = min(n_est, cap - gch)
    return gch, ech


def sym_batch(nv, nm, n_sym):
    """Pairs per launch of lm_mesh_pose_errors_sym."""
    per_pair = -(-nv // SYM_THREADS) * nm * n_sym
    return max(1, min(MAX_PTS_PAIRS, (SYM_PARTIAL_BUDGET // 8) // per_pair))


# ---- cameras, poses, renders -----------------------------------------------------------------------------------------------------------------
def cam(fx, fy, cx, cy):
    return np.array([fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0], np.float64).reshape(3, 3)


def centre_t(K, u, v, z):
    """The translation that puts the model origin at pixel (u, v), depth z."""
    return np.array([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z], np.float64)


def render(V, F, K, R, t, W, H, near=100.0, far=10000.0):
    """What the library renders for the pixel passes: float32 eye depth of the rasteriser with R, t, K cast to float32, background 0
    (tests/test_gpu_pose_error.py::oracle_depth)."""
    z, tri = ro.rasterise(V, F, np.asarray(K, F32), np.asarray(R, F32), np.asarray(t, F32).ravel(), W, H, near, far)
    return np.where(tri >= 0, z, 0).astype(F32)


OFFSETS = (0.0, 14.5, -14.5, 15.5, -15.5, 60.0, -60.0, None)   # mm added to the rendered depth; None = a hole (0).  Both sides of delta = 15


def pattern_scene(depths, W, H, offsets=OFFSETS, shift=0.0):
    """A float32 scene: the nearest of `depths` per pixel plus a pattern of offsets that runs along the columns and is shifted by 3 per row
    (so that frames a few pixels wide see every offset too), as pso_cases.eval_scene; elsewhere a background of 900 mm with bands of holes."""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    base = np.zeros((H, W), np.float64)
    for d in depths:
        d = d.astype(np.float64)
        base = np.where((d > 0) & ((base == 0) | (d < base)), d, base)
    idx = (x + 3 * y) % len(offsets)
    off = np.array([0.0 if o is None else o for o in offsets])[idx]
    hole = np.array([o is None for o in offsets])[idx]
    s = np.where(base > 0, base + shift + off, np.where((x // 5 + y // 3) % 3 == 0, 0.0, 900.0 + x - y))
    return np.where((base > 0) & hole, 0.0, s).astype(F32)


def quiet(fn, *a, **k):
    """The oracle on hostile values: numpy warns about inf * 0 and about a float64 beyond float32's range, and computes what pysixd would."""
    with np.errstate(all="ignore"):
        return fn(*a, **k)


def pixel_tables(V, F, K, W, H, scene, eR, et, gR, gt, delta=15.0, tau=20.0, near=100.0, far=10000.0, gt_far=None):
    """The oracle's answers for E x G poses in one frame: {"vsd", "vsd_tlinear", "cou": (E, G) float64, "counts": [e][g] dict,
    "stats": [g] dict (gt_stats with clip_far = gt_far, None = far), "ed", "gd": the renders}.  Each pose is rendered and turned into a
    distance image once."""
    ed = [render(V, F, K, R, t, W, H, near, far) for R, t in zip(eR, et)]
    gd = [render(V, F, K, R, t, W, H, near, far) for R, t in zip(gR, gt)]
    dt = quiet(per.dist_image, scene.astype(F32), K)
    De, Dg = [per.dist_image(d, K) for d in ed], [per.dist_image(d, K) for d in gd]
    out = {k: np.zeros((len(eR), len(gR))) for k in ("vsd", "vsd_tlinear", "cou")}
    out["counts"] = [[None] * len(gR) for _ in eR]
    for e in range(len(eR)):
        for g in range(len(gR)):
            c = quiet(per.vsd_counts_dist, dt, Dg[g], De[e], delta, tau)
            out["counts"][e][g] = c
            out["vsd"][e, g] = per.vsd_of_counts(c, "step")
            out["vsd_tlinear"][e, g] = per.vsd_of_counts(c, "tlinear")
            out["cou"][e, g] = per.cou(ed[e], gd[g])
    sd = gd if gt_far is None else [render(V, F, K, R, t, W, H, near, gt_far) for R, t in zip(gR, gt)]
    out["stats"] = [quiet(per.gt_stats, sd[g], scene.astype(F32), K, gR[g], gt[g], V, delta) for g in range(len(gR))]
    out["ed"], out["gd"] = ed, gd
    return out


# ---- frame sizes -----------------------------------------------------------------------------------------------------------------------------
# name: (W, H, K).  1024 pixels = 1 block, 1025 = 2; 131072 = 128 blocks of 4 pixels per lane, 131073 = the first frame a lane walks a fifth time.
FRAMES = {
    "1x1": (1, 1, cam(30.0, 30.0, 0.25, -0.125)),
    "7x5": (7, 5, cam(22.0, 22.0, 3.3, 2.4)),
    "32x32": (32, 32, cam(100.0, 100.0, 15.6, 16.3)),
    "41x25": (41, 25, cam(80.0, 80.0, 20.4, 12.7)),
    "257x3": (257, 3, cam(400.0, 12.0, 128.5, 1.25)),                   # fx != fy
    "100x77": (100, 77, cam(250.0, 250.0, 50.0, 38.25)),                # cx on pixel column 50: (u - cx) == 0 occurs
    "512x256": (512, 256, cam(700.0, 700.0, 255.5, 127.5)),
    "513x256": (513, 256, cam(700.0, 700.0, 256.3, 127.8)),
}
FRAME_NAMES = list(FRAMES)
D_ROT, D_T = rot((2, -1, 1), 4.0), np.array([4.0, -3.0, 3.3])


def frame_poses(W, H, K):
    """3 GTs: the frame's centre, its bottom right corner (so the LAST pixel is rendered, the one a strided lane reaches last) and its left edge;
    4 estimates: each GT a few degrees and mm off, and GT 0 itself."""
    gR = np.stack([rot((1, 2, 3), 25.0), rot((3, -1, 2), -40.0), rot((-2, 1, 1), 70.0)])
    gt = np.stack([centre_t(K, (W - 1) / 2.0, (H - 1) / 2.0, Z0), centre_t(K, W - 1.0, H - 1.0, Z0 - 5.0), centre_t(K, 0.0, (H - 1) * 0.4, Z0 + 10.0)])
    eR = np.stack([D_ROT @ gR[0], gR[1], rot((0, 1, 1), 9.0) @ gR[2], gR[0]])
    et = np.stack([gt[0] + D_T, gt[1] + [1.5, -2.0, 6.0], gt[2] + [-3.0, 2.0, 19.0], gt[0]])
    return eR, et, gR, gt


@functools.lru_cache(maxsize=None)
def frame_case(name):
    W, H, K = FRAMES[name]
    V, F = mesh()
    eR, et, gR, gt = frame_poses(W, H, K)
    gd = [render(V, F, K, R, t, W, H) for R, t in zip(gR, gt)]
    return {"W": W, "H": H, "K": K, "eR": eR, "et": et, "gR": gR, "gt": gt, "scene": pattern_scene(gd, W, H)}


@functools.lru_cache(maxsize=None)
def frame_expected(name):
    c = frame_case(name)
    V, F = mesh()
    return pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"], c["eR"], c["et"], c["gR"], c["gt"], gt_far=2000.0)


# ---- delta at equality -------------------------------------------------------------------------------------------------------------------------
# visible() compares f32(D_model) - f32(D_test) <= delta in float32.  With both distances near 400 mm (ulp 2^-15) every difference near 15 is a
# multiple of 2^-15, far coarser than the float32 neighbours of 15 (ulp 2^-20): no pixel could ever sit on the NEXT float32 above a delta that
# occurs.  So the model stands at 640 mm (distances in [512, 1024), ulp 2^-14) behind a scene about 330 mm in front of it (distances in
# [256, 512), ulp 2^-15): the differences lie in [256, 512) themselves and take every float32 there.  Three pixels of the scene are then tuned,
# by stepping their float32 depth, so that the difference is the chosen delta, the float32 below it and the float32 above it.
DELTA_SIDES = ("gt", "est")
DELTA_OFFSETS = (0.0, 0.5, -0.5, 3.0, -3.0, 20.0, -20.0, None)
DELTA_GAP = -330.0


def _pixel_dist(d, x, y, K):
    """misc.depth_im_to_dist_im for candidate depths d of ONE pixel (the builders' search; the result is checked with the oracle proper)."""
    d = np.asarray(d, np.float64)
    X = ((float(x) - K[0, 2]) * d) * (1.0 / K[0, 0])
    Y = ((float(y) - K[1, 2]) * d) * (1.0 / K[1, 1])
    return np.sqrt((X * X + Y * Y) + d * d)


def _tune(scene, K, dm, y, x, target, want_f64_above=False):
    """A float32 scene depth at (y, x) for which f32(dm) - f32(D_test) == target, or None.  want_f64_above: also dm - D_test > target in float64."""
    dm32 = F32(dm)
    d0 = F32((np.float64(dm32) - np.float64(target)) / _pixel_dist(1.0, x, y, K))
    cand = (d0.view(np.int32) + np.arange(-48, 49)).astype(np.int32).view(F32)
    Dt = _pixel_dist(cand, x, y, K)
    hit = (dm32 - Dt.astype(F32)) == F32(target)
    if want_f64_above:
        hit &= (np.float64(dm) - Dt) > np.float64(target)
    return cand[np.flatnonzero(hit)[0]] if hit.any() else None


@functools.lru_cache(maxsize=None)
def delta_case(side):
    """One (estimate, GT) pair.  side = "gt": the tuned pixels lie where only the GT renders (visible(D_t, D_g)); "est": where only the estimate
    renders, so that the estimate's own comparison decides (there vis_g is false and `|| (vis_g && De > 0)` cannot help).  "deltas": the float32
    below, the chosen value, the float32 above.  "pixels": {"occurs", "at", "below", "above"} -> (y, x)."""
    W, H, K = FRAMES["100x77"]
    V, F = mesh()
    Rm, tm = rot((1, 2, 3), 25.0), centre_t(K, 40.0, 38.0, 640.0)          # the model whose distances are compared
    Ro, to = rot((3, -1, 2), -40.0), centre_t(K, 62.0, 40.0, 640.0)        # the other pose of the pair, overlapping it partly
    dm, do = render(V, F, K, Rm, tm, W, H), render(V, F, K, Ro, to, W, H)
    scene = pattern_scene([dm, do], W, H, DELTA_OFFSETS, DELTA_GAP)
    Dm = per.dist_image(dm, K)
    only = (dm > 0) & (do == 0) & (scene > 0)
    diff = Dm.astype(F32) - per.dist_image(scene, K).astype(F32)
    ys, xs = np.nonzero(only & (np.abs(diff - 330.0) < 1.0))
    assert len(ys) > 8
    pixels = {"occurs": (int(ys[0]), int(xs[0]))}
    v = F32(diff[ys[0], xs[0]])
    lo, hi = np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))
    k = 1
    for tag, target, f64 in (("at", v, True), ("below", lo, False), ("above", hi, False)):
        while True:
            y, x = int(ys[k]), int(xs[k])
            k += 1
            d = _tune(scene, K, Dm[y, x], y, x, target, f64)
            if d is not None:
                scene[y, x] = d
                pixels[tag] = (y, x)
                break
    poses = {"eR": Ro[None], "et": to[None], "gR": Rm[None], "gt": tm[None]} if side == "gt" else {"eR": Rm[None], "et": tm[None], "gR": Ro[None], "gt": to[None]}
    poses.update({"W": W, "H": H, "K": K, "scene": scene, "deltas": (float(lo), float(v), float(hi)), "pixels": pixels, "model_depth": dm})
    return poses


@functools.lru_cache(maxsize=None)
def delta_expected(side):
    c = delta_case(side)
    V, F = mesh()
    return [pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"], c["eR"], c["et"], c["gR"], c["gt"], delta=d) for d in c["deltas"]]


# ---- tau at equality ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tau_case():
    """One pair 4 degrees and 19 mm apart, so that the costs |D_g - D_e| spread around 20 mm.  "taus": nextafter below, a cost that occurs in the
    intersection (the one nearest to 20), nextafter above, all float64.  The renders are fixed by the poses, so no pixel can be moved onto the
    neighbours: seen from the three taus the SAME pixel sits one ulp above, at, and one ulp below the threshold."""
    W, H, K = FRAMES["100x77"]
    V, F = mesh()
    gR, gt = rot((1, 2, 3), 25.0)[None], centre_t(K, 45.0, 38.0, Z0)[None]
    eR, et = (D_ROT @ gR[0])[None], (gt[0] + [2.0, -1.0, 19.0])[None]
    dg, de = render(V, F, K, gR[0], gt[0], W, H), render(V, F, K, eR[0], et[0], W, H)
    scene = pattern_scene([dg], W, H)
    dt, Dg, De = per.dist_image(scene, K), per.dist_image(dg, K), per.dist_image(de, K)
    vg = per.visib_mask(dt, Dg, 15.0)
    inter = vg & (per.visib_mask(dt, De, 15.0) | (vg & (De > 0)))
    cost = np.abs(Dg - De)
    ys, xs = np.nonzero(inter)
    i = int(np.argmin(np.abs(cost[ys, xs] - 20.0)))
    c = float(cost[ys[i], xs[i]])
    return {"W": W, "H": H, "K": K, "eR": eR, "et": et, "gR": gR, "gt": gt, "scene": scene, "taus": (math.nextafter(c, 0.0), c, math.nextafter(c, math.inf)),
            "pixel": (int(ys[i]), int(xs[i])), "cost": cost, "inter": inter}


@functools.lru_cache(maxsize=None)
def tau_expected():
    c = tau_case()
    V, F = mesh()
    return [pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"], c["eR"], c["et"], c["gR"], c["gt"], tau=t) for t in c["taus"]]


# ---- hostile scenes ----------------------------------------------------------------------------------------------------------------------------
HOSTILE_K = cam(120.0, 120.0, 24.0, 19.5)                                # cx on pixel column 24: (u - cx) * inf = NaN there
HOSTILE_W, HOSTILE_H = 48, 40
FLT_MAX = float(np.finfo(F32).max)
DENORMAL = 1e-40
# row y of the scene holds kind y % len(kinds): "plain" = the offset pattern, "neg" = minus (the pattern's depth or 500): its distance is positive,
# so pysixd counts it valid (and visible where it mirrors the render)
HOSTILE_ROWS = {"float32": ("plain", 0.0, "neg", 65535.0, float("nan"), float("inf"), 3.0e38, FLT_MAX, DENORMAL),
                "uint16": ("plain", 0, 65535, "plain", 1)}                 # uint16 holds no negative value, NaN or inf


@functools.lru_cache(maxsize=None)
def hostile_case(dtype):
    W, H, K = HOSTILE_W, HOSTILE_H, HOSTILE_K
    V, F = mesh()
    gR, gt = rot((1, 2, 3), 25.0)[None], centre_t(K, 24.0, 20.0, Z0)[None]
    eR, et = (D_ROT @ gR[0])[None], (gt[0] + [14.0, -6.0, 5.0])[None]     # shifted by about 4 pixels: each renders where the other does not
    dg, de = render(V, F, K, gR[0], gt[0], W, H), render(V, F, K, eR[0], et[0], W, H)
    plain = pattern_scene([dg, de], W, H).astype(np.float64)
    kinds = HOSTILE_ROWS[dtype]
    s = plain.copy()
    kind_of_row = []
    for y in range(H):
        k = kinds[y % len(kinds)]
        kind_of_row.append(k)
        if isinstance(k, str):
            s[y] = plain[y] if k == "plain" else -np.where(plain[y] > 0, plain[y], 500.0)
        else:
            s[y] = k
    scene = s.astype(F32) if dtype == "float32" else np.rint(s).astype(np.uint16)
    return {"W": W, "H": H, "K": K, "eR": eR, "et": et, "gR": gR, "gt": gt, "scene": scene, "kind_of_row": kind_of_row, "kinds": kinds}


@functools.lru_cache(maxsize=None)
def hostile_expected(dtype):
    c = hostile_case(dtype)
    V, F = mesh()
    return pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"].astype(F32), c["eR"], c["et"], c["gR"], c["gt"], gt_far=2000.0)


# ---- empty results -----------------------------------------------------------------------------------------------------------------------------
EMPTY_K = cam(140.0, 140.0, 47.6, 40.3)
EMPTY_W, EMPTY_H = 96, 80
EMPTY_NEAR, EMPTY_FAR = 100.0, 2000.0
EMPTY_GT = ("visible", "beyond_far", "outside", "occluded", "one_pixel")
EMPTY_EST = ("visible", "before_near", "one_pixel", "outside")


@functools.lru_cache(maxsize=None)
def empty_case():
    """GTs: 0 visible; 1 beyond clip_far; 2 entirely outside the frame; 3 fully occluded by a scene 100 mm in front of it; 4 occluded the same way
    but for ONE pixel, where the scene lies 1 mm behind it.  Estimates: 0 next to GT 0; 1 in front of clip_near (the whole blob at z < 100);
    2 = GT 4; 3 outside the frame."""
    W, H, K = EMPTY_W, EMPTY_H, EMPTY_K
    V, F = mesh()
    R = [rot((1, 2, 3), 25.0), rot((3, -1, 2), -40.0), rot((-2, 1, 1), 70.0)]
    gR = np.stack([R[0], R[1], R[2], R[1], R[2]])
    gt = np.stack([centre_t(K, 26.0, 22.0, Z0), centre_t(K, 48.0, 40.0, 2500.0), centre_t(K, -70.0, 22.0, Z0), centre_t(K, 70.0, 56.0, Z0 + 10.0),
                   centre_t(K, 72.0, 21.0, Z0 - 10.0)])
    eR = np.stack([D_ROT @ R[0], R[0], gR[4], R[1]])
    et = np.stack([gt[0] + D_T, np.array([0.0, 0.0, 50.0]), gt[4], centre_t(K, 48.0, 160.0, Z0)])
    d = [render(V, F, K, gR[g], gt[g], W, H, EMPTY_NEAR, EMPTY_FAR) for g in range(5)]
    scene = pattern_scene([d[0]], W, H)
    for g in (3, 4):
        scene = np.where(d[g] > 0, d[g] - F32(100.0), scene).astype(F32)
    ys, xs = np.nonzero(d[4] > 0)
    i = int(np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2))
    one = (int(ys[i]), int(xs[i]))
    scene[one] = d[4][one] + F32(1.0)
    return {"W": W, "H": H, "K": K, "eR": eR, "et": et, "gR": gR, "gt": gt, "scene": scene, "one": one}


@functools.lru_cache(maxsize=None)
def empty_expected():
    c = empty_case()
    V, F = mesh()
    return pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"], c["eR"], c["et"], c["gR"], c["gt"], near=EMPTY_NEAR, far=EMPTY_FAR)


# ---- options -----------------------------------------------------------------------------------------------------------------------------------
OPTION_DELTAS = (0.0, -5.0, 15.0, 1e9)
OPTION_TAUS = (1e-3, 20.0, 1e9)
# clip planes through the blob (its front is at about 355 mm, its back at about 445); float32 values, as the library casts them
OPTION_CLIPS = ((395.5, 10000.0), (100.0, 404.25), (395.5, 404.25))


@functools.lru_cache(maxsize=None)
def option_expected(delta=15.0, tau=20.0, near=100.0, far=10000.0):
    """The 100x77 frame case under other options (gt_stats with the same clip planes)."""
    c = frame_case("100x77")
    V, F = mesh()
    return pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"], c["eR"], c["et"], c["gR"], c["gt"], delta=delta, tau=tau, near=near, far=far)


# ---- chunked paths -----------------------------------------------------------------------------------------------------------------------------
# Pose i of a long batch is distinct pose i % period, so the oracle renders each distinct pose once.  The periods divide no chunk size and no
# chunk offset (asserted by the CPU test), so a pair mapped back with a wrong offset or a wrong chunk length lands on another pose.
PERIOD_EST, PERIOD_GT = 13, 17
CHUNK_K = cam(120.0, 120.0, 23.7, 19.4)
BIG_K = cam(500.0, 500.0, 1023.6, 511.3)                                 # 2048 x 1024: the blob is 100 pixels across, 0.4 % of the frame
# name: (W, H, n_est, n_gt, estimate period, GT period)
CHUNKED_VSD = {
    "a_200x60": (48, 40, 200, 60, PERIOD_EST, PERIOD_GT),              # gch 60, ech 196: estimate chunks 196 + 4
    "b_5x300": (48, 40, 5, 300, 5, PERIOD_GT),                         # gch 128: GT chunks 128 + 128 + 44, ech 5
    "c_140x140": (48, 40, 140, 140, PERIOD_EST, PERIOD_GT),            # gch 128, ech 128: 2 x 2 chunks, 128 + 12 both ways
    "e_2048x1024": (2048, 1024, 30, 4, 5, 4),                          # the pixel budget sets the cap: 32; gch 4, ech 28: 28 + 2
}
CHUNKED_VSD_NAMES = list(CHUNKED_VSD)
GT_STATS_N = 300                                                         # (d) 48 x 40: cap 256, chunks 256 + 44
PTS_SHAPE = (200, 90)                                                    # (f) 18000 pairs of a 12-vertex mesh: 16384 + 1616
SYM_SHAPE = (100, 70)                                                    # (g) 7000 pairs of an 8-vertex mesh, 3141 symmetries: 5341 + 1659
SYM_STEP = 0.001


def _random_poses(rng, n, K, W, H, spread):
    R = np.stack([rot(rng.normal(size=3), rng.uniform(0.0, 180.0)) for _ in range(n)])
    t = np.stack([centre_t(K, rng.uniform(W * (0.5 - spread), W * (0.5 + spread)), rng.uniform(H * (0.5 - spread), H * (0.5 + spread)),
                           rng.uniform(Z0 - 20.0, Z0 + 30.0)) for _ in range(n)])
    return R, t


@functools.lru_cache(maxsize=None)
def chunked_vsd_case(name):
    """"eR" .. "gt": the long batches; "eRd" .. "gtd": the distinct poses they repeat."""
    W, H, n_est, n_gt, pe, pg = CHUNKED_VSD[name]
    V, F = mesh()
    rng = np.random.default_rng(sum(name.encode()))
    if W == 2048:
        K = BIG_K
        gRd = np.stack([rot(rng.normal(size=3), rng.uniform(0.0, 180.0)) for _ in range(pg)])
        gtd = np.stack([centre_t(K, u, v, z) for u, v, z in ((300.0, 200.0, 400.0), (1000.0, 500.0, 410.0), (1700.0, 800.0, 395.0), (2030.0, 1010.0, 405.0))])
        eRd = np.stack([rot(rng.normal(size=3), 2.0 + 3.0 * i) @ gRd[i % pg] for i in range(pe)])
        etd = np.stack([gtd[i % pg] + rng.uniform(-6.0, 6.0, 3) + [0.0, 0.0, 3.0 * i] for i in range(pe)])
    else:
        K = CHUNK_K
        gRd, gtd = _random_poses(rng, pg, K, W, H, 0.3)
        eRd, etd = _random_poses(rng, pe, K, W, H, 0.3)
    gd = [render(V, F, K, R, t, W, H) for R, t in zip(gRd[:4], gtd[:4])]
    ie, ig = np.arange(n_est) % pe, np.arange(n_gt) % pg
    return {"W": W, "H": H, "K": K, "n_est": n_est, "n_gt": n_gt, "pe": pe, "pg": pg, "eRd": eRd, "etd": etd, "gRd": gRd, "gtd": gtd,
            "eR": eRd[ie], "et": etd[ie], "gR": gRd[ig], "gt": gtd[ig], "scene": pattern_scene(gd, W, H)}


@functools.lru_cache(maxsize=None)
def chunked_vsd_distinct(name):
    """pixel_tables of the distinct poses: (pe, pg) tables."""
    c = chunked_vsd_case(name)
    V, F = mesh()
    return pixel_tables(V, F, c["K"], c["W"], c["H"], c["scene"], c["eRd"], c["etd"], c["gRd"], c["gtd"], gt_far=2000.0)


def expand(table, src_e, src_g, pe, pg):
    """The (E, G) table whose cell (e, g) holds the distinct table's entry of poses (src_e[e, g], src_g[e, g]); a source of -1 (a cell no pair was
    written to) reads 0.0, what the zero-filled output keeps."""
    return np.where((src_e >= 0) & (src_g >= 0), np.asarray(table)[src_e % pe, src_g % pg], 0.0)


VSD_MISTAKES = ("drop_e0", "drop_g0", "swap_div_mod", "ech_for_short_ne")


def vsd_sources(n_est, n_gt, gch, ech, mistake=None):
    """The pair loop of lm_mesh_pose_errors restated on indices: (src_e, src_g, written), each (E, G): which estimate and GT the value stored in
    cell (e, g) was computed from.  The kernel's pair p of a chunk is views (g0 + p / ne, e0 + p % ne); the host maps p back to a cell.
    mistake: the host's map-back with one error."""
    src_e = np.full((n_est, n_gt), -1, np.int64)
    src_g = np.full((n_est, n_gt), -1, np.int64)
    for g0, ng in chunks_of(n_gt, gch):
        for e0, ne in chunks_of(n_est, ech):
            p = np.arange(ng * ne)
            from_g, from_e = g0 + p // ne, e0 + p % ne                  # what the kernel computed for pair p
            n = ech if mistake == "ech_for_short_ne" else ne
            gi, ei = (p % n, p // n) if mistake == "swap_div_mod" else (p // n, p % n)
            g = gi + (0 if mistake == "drop_g0" else g0)
            e = ei + (0 if mistake == "drop_e0" else e0)
            ok = (g < n_gt) & (e < n_est)                               # a restatement may not write out of bounds
            src_e[e[ok], g[ok]], src_g[e[ok], g[ok]] = from_e[ok], from_g[ok]
    return src_e, src_g, src_e >= 0


def flat_sources(n_pairs, batch, mistake=None):
    """run_pts and the batch loop of lm_mesh_pose_errors_sym: out[p0 + p] = result of pair p0 + p.  mistake "drop_p0": out[p]."""
    src = np.full(n_pairs, -1, np.int64)
    for p0, n in chunks_of(n_pairs, batch):
        p = np.arange(n)
        src[p + (0 if mistake == "drop_p0" else p0)] = p0 + p
    return src


def gt_sources(n_gt, cap, mistake=None):
    """lm_mesh_gt_stats: g = g0 + i.  mistake "drop_g0": g = i."""
    src = np.full(n_gt, -1, np.int64)
    for g0, n in chunks_of(n_gt, cap):
        i = np.arange(n)
        src[i + (0 if mistake == "drop_g0" else g0)] = g0 + i
    return src


@functools.lru_cache(maxsize=None)
def gt_stats_case():
    """(d) 300 GTs of PERIOD_GT distinct poses at 48 x 40."""
    W, H, K = 48, 40, CHUNK_K
    V, F = mesh()
    rng = np.random.default_rng(44)
    gRd, gtd = _random_poses(rng, PERIOD_GT, K, W, H, 0.45)
    gd = [render(V, F, K, R, t, W, H, 100.0, 2000.0) for R, t in zip(gRd, gtd)]
    scene = pattern_scene(gd[:3], W, H)
    stats = [per.gt_stats(gd[g], scene, K, gRd[g], gtd[g], V, 15.0) for g in range(PERIOD_GT)]
    ig = np.arange(GT_STATS_N) % PERIOD_GT
    return {"W": W, "H": H, "K": K, "gR": gRd[ig], "gt": gtd[ig], "scene": scene, "stats": stats}


def _point_poses(seed, pe, pg):
    """GTs around z = 800 mm and estimates from a degree to a wrong pose off them (tests/test_gpu_pose_sym.py::poses)."""
    rng = np.random.default_rng(seed)
    gR = np.stack([rot(rng.normal(size=3), rng.uniform(0.0, 180.0)) for _ in range(pg)])
    gt = np.array([0.0, 0.0, 800.0]) + rng.uniform(-150.0, 150.0, (pg, 3))
    eR = np.stack([rot(rng.normal(size=3), [0.5, 8.0, 90.0][e % 3]) @ gR[e % pg] for e in range(pe)])
    et = gt[np.arange(pe) % pg] + rng.uniform(-1.0, 1.0, (pe, 3)) * np.array([2.0, 15.0, 60.0])[np.arange(pe) % 3, None]
    return eR, et, gR, gt


@functools.lru_cache(maxsize=None)
def pts_case():
    """(f) ADD / ADI: the 12 vertices of the unrefined icosphere; "add", "adi": the (13, 17) tables of the distinct poses."""
    V, F, _, _ = synth.icosphere(0, radius=40.0, seed=5)
    eRd, etd, gRd, gtd = _point_poses(61, PERIOD_EST, PERIOD_GT)
    V64 = V.astype(np.float64)
    add = np.array([[per.add(eRd[e], etd[e], gRd[g], gtd[g], V64) for g in range(PERIOD_GT)] for e in range(PERIOD_EST)])
    adi = np.array([[per.adi(eRd[e], etd[e], gRd[g], gtd[g], V64) for g in range(PERIOD_GT)] for e in range(PERIOD_EST)])
    ie, ig = np.arange(PTS_SHAPE[0]) % PERIOD_EST, np.arange(PTS_SHAPE[1]) % PERIOD_GT
    return {"V": V, "F": F, "eR": eRd[ie], "et": etd[ie], "gR": gRd[ig], "gt": gtd[ig], "add": add, "adi": adi}


SYM_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float64)


@functools.lru_cache(maxsize=None)
def sym_case():
    """(g) MSSD + MSPD: 8 vertices, one continuous symmetry about z at max_sym_disc_step = 0.001 (3141 transformations); "mssd", "mspd": the
    (13, 17) tables of the distinct poses."""
    V = (np.random.default_rng(8).normal(size=(8, 3)) * [40.0, 30.0, 20.0]).astype(F32)
    F = np.array([[0, 1, 2]], np.int32)
    eRd, etd, gRd, gtd = _point_poses(62, PERIOD_EST, PERIOD_GT)
    Rs, ts = psr.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_sym_disc_step=SYM_STEP)
    want = psr.errors_batched(eRd, etd, gRd, gtd, SYM_K, V.astype(np.float64), Rs, ts)
    ie, ig = np.arange(SYM_SHAPE[0]) % PERIOD_EST, np.arange(SYM_SHAPE[1]) % PERIOD_GT
    return {"V": V, "F": F, "eR": eRd[ie], "et": etd[ie], "gR": gRd[ig], "gt": gtd[ig], "n_sym": len(Rs), "Rs": Rs, "ts": ts,
            "mssd": want["mssd"], "mspd": want["mspd"]}


def flat_expand(table, src, n_gt):
    """The (E, G) table, flattened, whose entry p holds the distinct table's entry of pair src[p] = e * n_gt + g; -1 reads 0.0."""
    e, g = src // n_gt, src % n_gt
    return np.where(src >= 0, np.asarray(table)[e % PERIOD_EST, g % PERIOD_GT], 0.0)
