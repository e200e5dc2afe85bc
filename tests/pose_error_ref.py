"""numpy / scipy restatement of the pose errors of pysixd (pose_error.py, visibility.py, misc.py) and of the GT statistics of
tools/calc_gt_stats.py — TEST INFRASTRUCTURE ONLY: the oracle of lm_mesh_pose_errors / lm_mesh_gt_stats.  Written from the
semantics of those files (line numbers cited per function); rendering stays outside: every function that needs a render takes
the float32 depth images as arguments (0 = background)."""
import math

import numpy as np
from scipy import spatial


def dist_image(depth, K):
    """misc.depth_im_to_dist_im (misc.py:43-62): X = ((u - cx) * d) * (1 / fx), Y likewise, dist = sqrt((X^2 + Y^2) + d^2), f64."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    H, W = depth.shape
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    d = depth.astype(np.float64)
    X = ((u - K[0, 2]) * d) * (1.0 / K[0, 0])
    Y = ((v - K[1, 2]) * d) * (1.0 / K[1, 1])
    return np.sqrt((X * X + Y * Y) + d * d)


def visib_mask(d_test, d_model, delta):
    """visibility.estimate_visib_mask (visibility.py:6-20): both distance images cast to float32 before the difference."""
    valid = (d_test > 0) & (d_model > 0)
    diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    return (diff <= np.float32(delta)) & valid


def vsd_counts_dist(dt, dg, de, delta, tau):
    """vsd_counts on distance images already built (dist_image of the scene, the GT render and the estimate's render): the same
    statements, so that a table of many pairs builds each pose's distance image once."""
    vg = visib_mask(dt, dg, delta)                                       # visibility.py:23-25
    ve = visib_mask(dt, de, delta) | (vg & (de > 0))                     # visibility.py:27-30
    inter, union = vg & ve, vg | ve
    cost = np.abs(dg[inter] - de[inter])                                 # f64
    return {"union": int(union.sum()), "inter": int(inter.sum()), "step": int((cost >= tau).sum()),
            "tlinear": float(np.minimum(cost * (1.0 / tau), 1.0).sum())}


def vsd_counts(depth_est, depth_gt, depth_test, K, delta, tau):
    """The quantities behind pose_error.vsd (pose_error.py:41-78): |union|, |inter|, the step cost count and the tlinear cost
    sum over the intersection."""
    return vsd_counts_dist(dist_image(depth_test, K), dist_image(depth_gt, K), dist_image(depth_est, K), delta, tau)


def vsd_of_counts(c, cost="step"):
    """pose_error.py:74-81: the mean of the costs over the union, the pixels outside the intersection counting 1; 1.0 for an
    empty union."""
    if c["union"] == 0:
        return 1.0
    costs = c["step"] if cost == "step" else c["tlinear"]
    return (costs + (c["union"] - c["inter"])) / float(c["union"])


def vsd(depth_est, depth_gt, depth_test, K, delta=15.0, tau=20.0, cost="step"):
    """pose_error.vsd (pose_error.py:12-81) on given renders."""
    return vsd_of_counts(vsd_counts(depth_est, depth_gt, depth_test, K, delta, tau), cost)


def cou_counts(depth_est, depth_gt):
    me, mg = depth_est > 0, depth_gt > 0
    return {"inter": int((me & mg).sum()), "union": int((me | mg).sum())}


def cou(depth_est, depth_gt):
    """pose_error.cou (pose_error.py:83-115): 1 - |inter| / |union| of the masks depth > 0; 1.0 for an empty union."""
    c = cou_counts(depth_est, depth_gt)
    return 1.0 - c["inter"] / float(c["union"]) if c["union"] > 0 else 1.0


def _xf(pts, R, t):
    """misc.transform_pts_Rt (misc.py:129-140)."""
    return (np.asarray(R, np.float64).reshape(3, 3) @ pts.T + np.asarray(t, np.float64).reshape(3, 1)).T


def add(R_est, t_est, R_gt, t_gt, pts):
    """pose_error.add (pose_error.py:117-131): mean distance of corresponding model points."""
    pts = np.asarray(pts, np.float64)
    return float(np.linalg.norm(_xf(pts, R_est, t_est) - _xf(pts, R_gt, t_gt), axis=1).mean())


def adi(R_est, t_est, R_gt, t_gt, pts):
    """pose_error.adi (pose_error.py:133-152): mean distance from each GT-posed point to the nearest estimate-posed point."""
    pts = np.asarray(pts, np.float64)
    d, _ = spatial.cKDTree(_xf(pts, R_est, t_est)).query(_xf(pts, R_gt, t_gt), k=1)
    return float(d.mean())


def re(R_est, R_gt):
    """pose_error.re (pose_error.py:154-167): degrees; inv(R_gt), not the transpose."""
    c = 0.5 * (np.trace(np.asarray(R_est, np.float64).reshape(3, 3) @ np.linalg.inv(np.asarray(R_gt, np.float64).reshape(3, 3))) - 1.0)
    return 180.0 * math.acos(min(1.0, max(-1.0, c))) / np.pi


def te(t_est, t_gt):
    """pose_error.te (pose_error.py:169-180)."""
    return float(np.linalg.norm(np.asarray(t_gt, np.float64).ravel() - np.asarray(t_est, np.float64).ravel()))


def diameter(pts):
    """misc.calc_pts_diameter (misc.py:142-158), brute force."""
    pts = np.asarray(pts, np.float64)
    best = 0.0
    for i in range(len(pts)):
        best = max(best, float(((pts[i:] - pts[i]) ** 2).sum(1).max()))
    return math.sqrt(best)


def bbox_2d(xs, ys):
    """misc.calc_2d_bbox (misc.py:82-89), no clipping."""
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def gt_stats(depth_gt, depth_test, K, R_gt, t_gt, pts, delta=15.0):
    """tools/calc_gt_stats.py:103-155 for one GT, given its render."""
    dg, dt = dist_image(depth_gt, K), dist_image(depth_test, K)
    vg = visib_mask(dt, dg, delta)
    obj = dg > 0
    n_all, n_valid, n_vis = int(obj.sum()), int((dt[obj] > 0).sum()), int(vg.sum())
    K3 = np.asarray(K, np.float64).reshape(3, 3)
    P = K3 @ np.hstack((np.asarray(R_gt, np.float64).reshape(3, 3), np.asarray(t_gt, np.float64).reshape(3, 1)))   # misc.project_pts
    ph = P @ np.hstack((np.asarray(pts, np.float64), np.ones((len(pts), 1)))).T
    uv = np.round((ph[:2] / ph[2]).T).astype(np.int64)                  # misc.calc_pose_2d_bbox
    ys, xs = vg.nonzero()
    return {"px_count_all": n_all, "px_count_visib": n_vis, "px_count_valid": n_valid,
            "visib_fract": n_vis / float(n_all) if n_all > 0 else 0.0,
            "bbox_obj": bbox_2d(uv[:, 0], uv[:, 1]), "bbox_visib": bbox_2d(xs, ys) if n_vis > 0 else [-1, -1, -1, -1]}
