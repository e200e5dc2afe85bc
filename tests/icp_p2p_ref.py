"""numpy restatement of RegistrationICP with TransformationEstimationPointToPoint (the reference built without USE_OPEN3D_P2PL,
LL.cpp:132-134), of EvaluateRegistration (LL.cpp:111-115, max_iter = 0) and of the convergence criteria, on top of the oracle's own
correspondence search, summation and cloud preparation (oracle/linemod_oracle.py, imported, not edited).

UNPINNED, like MSSD / MSPD: Open3D is not available, so this follows Open3D's TransformationEstimationPointToPoint
(Eigen::umeyama(source, target, with_scaling = false)) and ICPConvergenceCriteria from knowledge of them; the deterministic rules are
the oracle's (ties to the lower index, d^2 < max_dist^2, sequential sums) plus one of this file: the update is the identity when
there are fewer than 3 correspondences or an entry of the result is not finite.

Also here: the case table the CPU test (well-posedness) and the GPU test (the product against this file) share, and a cache of what
this file computed per hypothesis, so that nothing is restated twice in one session."""
import numpy as np

import linemod_oracle as lo
from linemod_oracle import (ICP_MAX_DIST, ICP_MAX_ITER, ICP_REL, _seq_sum, _sqdist, backproject_clouds, nearest,   # noqa: F401
                            voxel_down_sample)

f32 = np.float32


# ---- the estimator -------------------------------------------------------------------------------------------
def icp_eval_p2p(src, tgt, max_dist, nn="brute", tree=None):
    """GetRegistrationResultAndCorrespondences and the sums of the point-to-point update over its correspondences (p = source as
    it stands, q = its nearest target): (fitness, inlier_rmse, sums) with sums = [n, sum d^2, sum p (3), sum q (3), sum q p^T (9,
    row-major)], 17 doubles, each a sequential sum in source order."""
    sums = np.zeros(17)
    if len(src) == 0 or len(tgt) == 0:
        return 0.0, 0.0, sums
    j, best = nearest(src, tgt, nn, tree)
    ok = best < max_dist * max_dist
    n = int(ok.sum())
    if n == 0:
        return 0.0, 0.0, sums
    p, q = src[ok], tgt[j[ok]]
    sums[0] = n
    sums[1] = _seq_sum(best[ok][:, None])[0]
    sums[2:5] = _seq_sum(p)
    sums[5:8] = _seq_sum(q)
    sums[8:17] = _seq_sum(q[:, :, None] * p[:, None, :]).reshape(9)
    return n / float(len(src)), float(np.sqrt(sums[1] / n)), sums


def centred_h(sums):
    """H = sum q p^T - n qm pm^T (3x3), None without correspondences."""
    n = int(sums[0])
    if n == 0:
        return None
    pm, qm = sums[2:5] / n, sums[5:8] / n
    return sums[8:17].reshape(3, 3) - n * np.outer(qm, pm)


def kabsch(sums):
    """Eigen::umeyama(source, target, false) from the sums: R = U diag(1, 1, det(U) det(V)) V^T of H = U D V^T, t = qm - R pm, as a
    4x4; the identity when n < 3 or an entry is not finite."""
    T = np.eye(4)
    n = int(sums[0])
    if n < 3 or not np.all(np.isfinite(sums)):
        return T
    H = centred_h(sums)
    try:
        U, _, Vt = np.linalg.svd(H)
    except np.linalg.LinAlgError:
        return T
    S = np.diag([1.0, 1.0, float(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    t = sums[5:8] / n - R @ (sums[2:5] / n)
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return T
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def _sv_ratio(sums) -> float:
    """Second singular value of H over the first (0 without correspondences): how well the rotation is pinned."""
    H = centred_h(sums)
    if H is None or not np.all(np.isfinite(H)):
        return 0.0
    s = np.linalg.svd(H, compute_uv=False)
    return float(s[1] / s[0]) if s[0] > 0 else 0.0


def icp_point_to_point(src, tgt, init, max_dist=ICP_MAX_DIST, max_iter=ICP_MAX_ITER, rel_fitness=ICP_REL, rel_rmse=ICP_REL, history=None,
                       nn="brute"):
    """open3d RegistrationICP(source, target, max_dist, init, PointToPoint, ICPConvergenceCriteria(rel_fitness, rel_rmse, max_iter)):
    the loop of the oracle's icp_point_to_plane with the other update.  max_iter = 0 is EvaluateRegistration: (init, fitness and
    rmse of init, 0).  history: one dict per evaluation (fitness, rmse, n, sv_ratio)."""
    T = np.array(init, np.float64)
    tree = None
    if nn == "kdtree":
        from scipy.spatial import cKDTree
        tree = cKDTree(tgt)
    pts = src @ T[:3, :3].T + T[:3, 3]
    fit, rmse, sums = icp_eval_p2p(pts, tgt, max_dist, nn, tree)

    def note():
        if history is not None:
            history.append({"fitness": fit, "rmse": rmse, "n": int(sums[0]), "sv_ratio": _sv_ratio(sums)})
    note()
    iters = 0
    for _ in range(max_iter):
        iters += 1
        upd = kabsch(sums)
        T = upd @ T
        pts = pts @ upd[:3, :3].T + upd[:3, 3]
        bfit, brmse = fit, rmse
        fit, rmse, sums = icp_eval_p2p(pts, tgt, max_dist, nn, tree)
        note()
        if abs(bfit - fit) < rel_fitness and abs(brmse - rmse) < rel_rmse:
            break
    return T, fit, rmse, iters


def icp_point_to_plane(src, tgt, nrm, init, max_iter=ICP_MAX_ITER, rel=ICP_REL, history=None, nn="brute"):
    """The oracle's icp_point_to_plane at another max_iteration and relative_fitness = relative_rmse = rel (its tolerance is the
    module global ICP_REL: set for the call and restored)."""
    keep = lo.ICP_REL
    lo.ICP_REL = rel
    try:
        return lo.icp_point_to_plane(src, tgt, nrm, init, max_iter=max_iter, nn=nn, history=history)
    finally:
        lo.ICP_REL = keep


def ill_posed_p2p(history, rel_fitness=ICP_REL, rel_rmse=ICP_REL) -> str:
    """Why a point-to-point run is ill-posed on this file's own evidence ('' when well-posed): the oracle's convergence-margin rule
    (a test within 1e-9 of its threshold), or a final H whose second singular value is below 1e-8 of the first (an axis the
    correspondences do not pin).  With fewer than 3 correspondences the update is the identity by rule: nothing is left to pin."""
    for e in range(1, len(history)):
        for key, rel in (("fitness", rel_fitness), ("rmse", rel_rmse)):
            d = abs(history[e - 1][key] - history[e][key])
            if abs(d - rel) < 1e-9:
                return "convergence test of %s at evaluation %d within 1e-9 of the threshold (%.3g)" % (key, e, d)
    if history and history[-1]["n"] >= 3 and history[-1]["sv_ratio"] < 1e-8:
        return "final H singular value ratio %.3g" % history[-1]["sv_ratio"]
    return ""


# ---- poseRefine::process ----------------------------------------------------------------------------------------
def init_base(modelR, modelT):
    b = np.zeros((4, 4), f32)
    b[:3, :3] = np.asarray(modelR, f32).reshape(3, 3)
    b[:3, 3] = np.asarray(modelT, f32).reshape(3)
    b[2, 3] = b[2, 3] / f32(1000.0)                           # only t.z is converted (LL.cpp:37)
    b[3, 3] = 1
    return b.astype(np.float64)


_CLOUDS = {}


def clouds(scene_depth, model_depth, sceneK, modelK, detect_x, detect_y, scene_from_scene):
    """LL.cpp:43-109 by the oracle's functions: None when the window leaves the frame, else dict(src, tgt, init_guess, nn); computed
    once per distinct input."""
    from helpers import h16
    key = (h16(scene_depth), h16(model_depth), np.asarray(sceneK, f32).tobytes(), np.asarray(modelK, f32).tobytes(), int(detect_x), int(detect_y),
           bool(scene_from_scene))
    if key not in _CLOUDS:
        bp = backproject_clouds(np.asarray(scene_depth), np.asarray(model_depth), sceneK, modelK, detect_x, detect_y)
        if bp is None:
            _CLOUDS[key] = None
        else:
            model_pts, scene_pts, tr = bp
            g = np.eye(4)
            g[:3, 3] = tr
            src = voxel_down_sample(model_pts)
            tgt = voxel_down_sample(scene_pts if scene_from_scene else model_pts)   # LL.cpp:109 (sic: model)
            _CLOUDS[key] = {"src": src, "tgt": tgt, "init_guess": g, "nn": "kdtree" if max(len(src), len(tgt)) > 3000 else "brute"}
    return _CLOUDS[key]


def normals_of(c):
    """EstimateNormals of the target cloud of clouds(...), once."""
    if "normals" not in c:
        c["normals"] = lo.estimate_normals(c["tgt"], nn=c["nn"])
    return c["normals"]


def _result(T, fit, rmse, iters, c, base, history):
    M = T @ base
    return {"residual": float(f32(fit)), "R": M[:3, :3].copy(), "t": M[:3, 3] * 1000.0, "T_icp": T, "rmse": rmse, "iterations": iters,
            "n_source": len(c["src"]), "n_target": len(c["tgt"]), "init_guess": c["init_guess"], "history": history}


_RUNS = {}


def pose_refine_p2p(scene_depth, model_depth, sceneK, modelK, modelR, modelT, detect_x, detect_y, scene_from_scene=False,
                    max_iter=ICP_MAX_ITER, rel_fitness=ICP_REL, rel_rmse=ICP_REL, estimation="point_to_point"):
    """poseRefine::process (LL.cpp:27-155) like the oracle's pose_refine, with the point-to-point estimator and the criteria as
    arguments; estimation="point_to_plane" runs the oracle's own loop (rel_fitness must equal rel_rmse).  Cached per input."""
    c = clouds(scene_depth, model_depth, sceneK, modelK, detect_x, detect_y, scene_from_scene)
    if c is None:
        return {"residual": -1.0, "R": None, "t": None}
    key = (id(c), np.asarray(modelR, f32).tobytes(), np.asarray(modelT, f32).tobytes(), max_iter, rel_fitness, rel_rmse, estimation)
    if key not in _RUNS:
        history = []
        if estimation == "point_to_point":
            T, fit, rmse, iters = icp_point_to_point(c["src"], c["tgt"], c["init_guess"], ICP_MAX_DIST, max_iter, rel_fitness, rel_rmse, history,
                                                     nn=c["nn"])
        else:
            assert estimation == "point_to_plane" and rel_fitness == rel_rmse
            T, fit, rmse, iters = icp_point_to_plane(c["src"], c["tgt"], normals_of(c), c["init_guess"], max_iter, rel_fitness, history, nn=c["nn"])
        _RUNS[key] = _result(T, fit, rmse, iters, c, init_base(modelR, modelT), history)
    return _RUNS[key]


def ill_posed_run(ref, rel_fitness=ICP_REL, rel_rmse=ICP_REL, estimation="point_to_point") -> str:
    """ill_posed_p2p, or the oracle's ill_posed for a point-to-plane run.  The oracle's eigenvalue rule is about a 6x6 that is solved:
    with fewer than 6 correspondences at the end its update is the identity by rule (as here with fewer than 3), and only the
    convergence-margin rule is applied."""
    if estimation == "point_to_point":
        return ill_posed_p2p(ref["history"], rel_fitness, rel_rmse)
    hist = [dict(e) for e in ref["history"]]
    if hist and round(hist[-1]["fitness"] * ref["n_source"]) < 6:
        hist[-1]["eig_ratio"] = 1.0
    return lo.ill_posed(hist, rel=rel_fitness)


# ---- the shared case table ----------------------------------------------------------------------------------------
W, H = 640, 480


def _scene_tools():
    import test_gpu_icp_oracle as T0                          # the scene builders of the point-to-plane tests (imported, not edited)
    return T0


def _small():
    """One small cloud (a few hundred points): every slice of the sliced launches holds a handful of points, most none."""
    T0 = _scene_tools()
    from synth import bump
    rng = np.random.default_rng(41)
    md = bump(910, 13, 11)
    mK = T0.model_K(rng)
    L = T0.place(md, mK, (40, -30), 911, rot_deg=2.5, t_mm=(2.5, -2.0, 3.0))
    c = T0.Case(T0.compose([L]))
    c.add("small", md, mK, *T0._pose(rng), T0.window_of(md, L))
    return c


def _large(copies=1):
    """A curved, rippled surface of ~19k points: several slices per hypothesis, each with more points than the workgroup has threads.
    copies: the same hypothesis that many times (the 16-hypothesis batch of the timing)."""
    T0 = _scene_tools()
    md = T0.surface(80, 60)
    L = T0.place(md, T0.K_CAM, (0, 0), 780, rot_deg=1.5, t_mm=(3.0, -2.0, 3.0))
    c = T0.Case(T0.compose([L]))
    ys, xs = np.nonzero(md)
    pose = T0._pose(np.random.default_rng(780))
    for k in range(copies):
        c.add("surface 159x119" + (" #%d" % k if copies > 1 else ""), md, T0.K_CAM, *pose, (int(xs.min()), int(ys.min())))
    return c


def _batch3():
    """Three hypotheses of one frame: an ordinary one; one whose window leaves the frame (LL.cpp:52-55: residual -1, nothing else
    touched); one whose scene window holds an 8x8-pixel speck (some 40 points, 2 cm across) 0.2 m behind the object and nothing else: the
    init guess puts the model's centroid on the speck, and the deep cap-shaped model has no point within 3 cm of its own centroid: no
    correspondences."""
    T0 = _scene_tools()
    from synth import bump
    rng = np.random.default_rng(43)
    md_a, md_c = bump(920, 22, 18), bump(921, 24, 20, amp=120.0)
    mK_a, mK_c = T0.model_K(rng), T0.model_K(rng)
    L_a = T0.place(md_a, mK_a, (-180, 40), 922, rot_deg=-2.0, t_mm=(-2.0, 3.0, 2.5))
    # the speck: under the model pixel at the image centre, for a window at (430, 120)
    ys, xs = np.nonzero(md_c)
    dx, dy = 430, 120
    sy, sx = H // 2 - int(ys.min()) + dy, W // 2 - int(xs.min()) + dx
    L_c = np.zeros((H, W), np.float64)
    L_c[sy - 4:sy + 4, sx - 4:sx + 4] = float(md_c[H // 2, W // 2]) + 200.0
    c = T0.Case(T0.compose([L_a, L_c]))
    c.add("ordinary", md_a, mK_a, *T0._pose(rng), T0.window_of(md_a, L_a))
    bw, _ = T0.dilated_box(md_a)
    c.add("out of frame", md_a, mK_a, *T0._pose(rng), (W - bw, 100))
    c.add("no correspondences", md_c, mK_c, *T0._pose(rng), (dx, dy))
    return c


def _verbatim():
    """The two well-posed regimes of the verbatim mode (LL.cpp:109 registers the model cloud against itself, moved by the
    centroid difference): a scene 3 mm behind the model (the registration walks back to the identity, fitness 1) and one 0.3 m behind
    (no correspondences: T = init guess, fitness 0)."""
    T0 = _scene_tools()
    from synth import bump
    rng = np.random.default_rng(44)
    md = bump(930, 20, 16)
    ys, xs = np.nonzero(md)
    out = []
    for name, dz in (("verbatim, 3 mm", 3), ("verbatim, 0.3 m", 300)):
        c = T0.Case(np.where(md > 0, md + dz, 0).astype(np.uint16))
        c.add(name, md, T0.K_CAM, *T0._pose(rng), (int(xs.min()), int(ys.min())))
        out.append(c)
    return out


_CASES = {}


def cases():
    """name -> (Case, scene_from_scene): built once."""
    if not _CASES:
        _CASES["small"] = (_small(), True)
        _CASES["large"] = (_large(), True)
        _CASES["batch3"] = (_batch3(), True)
        v = _verbatim()
        _CASES["verbatim_near"] = (v[0], False)
        _CASES["verbatim_far"] = (v[1], False)
    return _CASES


def large_batch16():
    return _large(16)


# the runs the GPU test compares with this file: (case, estimation, max_iteration, relative_fitness = relative_rmse)
RUNS = ([(n, "point_to_point", 30, ICP_REL) for n in ("small", "large", "batch3", "verbatim_near", "verbatim_far")]
        + [(n, "point_to_point", 1, ICP_REL) for n in ("small", "large", "batch3")]
        + [(n, est, 0, ICP_REL) for n in ("small", "large", "batch3") for est in ("point_to_point", "point_to_plane")]
        + [(n, "point_to_plane", k, 1e-3) for n in ("small", "large", "batch3") for k in (2, 5)])


def reference(case, sfs, i, estimation, max_iter, rel):
    from helpers import K_CAM
    return pose_refine_p2p(case.scene, case.mds[i], K_CAM, case.Ks[i], case.Rs[i], case.ts[i], case.xy[i][0], case.xy[i][1], scene_from_scene=sfs,
                           max_iter=max_iter, rel_fitness=rel, rel_rmse=rel, estimation=estimation)
