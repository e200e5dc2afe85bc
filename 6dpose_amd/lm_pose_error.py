"""Pose errors and BOP recall: pysixd's and the BOP toolkit's errors on the device (lm_mesh_pose_errors*, lm_mesh_gt_stats), the
symmetry sets, and the host-side matching of estimates to ground truths."""
from __future__ import annotations

import numpy as np

from lm_abi import _check, _ptr, load_library
from lm_render import Mesh


POSE_METRICS = ("vsd", "cou", "add", "adi", "re", "te")           # bit i of lm_mesh_pose_errors' mask = POSE_METRICS[i]
POSE_METRICS_SYM = ("mssd", "mspd")                               # bit 6 + i of lm_mesh_pose_errors_sym's mask


def _pose_batch(R, t, what):
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    if R.shape == (3, 3):
        R, t = R.reshape(1, 3, 3), t.reshape(1, 3)
    if R.ndim != 3 or R.shape[1:] != (3, 3) or t.size != 3 * len(R):
        raise ValueError("%s: R must be (3,3) or (n,3,3) and t (3,) or (n,3), got %s and %s" % (what, R.shape, t.shape))
    return np.ascontiguousarray(R.reshape(-1, 9)), np.ascontiguousarray(t.reshape(-1, 3))


def _scene_mm(scene_depth):
    """Scene depth in mm as float32 (load_depth * depth_scale); uint16 is converted exactly."""
    d = np.asarray(scene_depth)
    if d.ndim != 2:
        raise ValueError("scene_depth must be a (H, W) image")
    if d.dtype not in (np.float32, np.uint16):
        raise ValueError("scene_depth must be float32 (mm) or uint16 (mm), got %s" % d.dtype)
    return np.ascontiguousarray(d, np.float32)


def pose_errors(mesh: Mesh, R_est, t_est, R_gt, t_gt, K=None, scene_depth=None, metrics=POSE_METRICS, delta=15.0, tau=20.0, cost="step",
                clip_near=100.0, clip_far=10000.0, im_size=None, symmetries=None):
    """pysixd.pose_error (vsd, cou, add, adi, re, te) for E estimates x G ground truths of one object in one frame, on the device
    (lm_mesh_pose_errors).  Returns {metric: (E, G) float64}.  A single pose (3x3, 3) is a batch of one.  vsd needs scene_depth
    (H, W); cou needs K and the image size, taken from scene_depth or im_size = (width, height) (pose_error.cou's im_size).
    Defaults: the SIXD-17 settings of eval_calc_errors.py:40-42 and pysixd's clip planes for vsd / cou (pose_error.py:35-39).
    "mssd" and "mspd" (lm_mesh_pose_errors_sym, not in the default) are the BOP toolkit's symmetry-aware maxima over
    symmetries = (Rs, ts) as symmetry_transforms returns them (None: the identity only); mspd needs K."""
    Re, te = _pose_batch(R_est, t_est, "estimate")
    Rg, tg = _pose_batch(R_gt, t_gt, "ground truth")
    if isinstance(metrics, str):
        metrics = (metrics,)
    mask = sym_mask = 0
    for name in metrics:
        if name in POSE_METRICS:
            mask |= 1 << POSE_METRICS.index(name)
        elif name in POSE_METRICS_SYM:
            sym_mask |= 64 << POSE_METRICS_SYM.index(name)
        else:
            raise ValueError("unknown metric %r (one of %s)" % (name, ", ".join(POSE_METRICS + POSE_METRICS_SYM)))
    if cost not in ("step", "tlinear"):
        raise ValueError("unknown vsd cost %r (step or tlinear)" % (cost,))
    scene = None if scene_depth is None else _scene_mm(scene_depth)
    if scene is not None:
        W, H = scene.shape[1], scene.shape[0]
        if im_size is not None and (int(im_size[0]), int(im_size[1])) != (W, H):
            raise ValueError("im_size %s does not match scene_depth %s" % (tuple(im_size), scene.shape))
    elif im_size is not None:
        W, H = int(im_size[0]), int(im_size[1])
    else:
        W = H = 0
    Kd = None if K is None else np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    res = {}
    if mask or not sym_mask:
        order = [n for n in POSE_METRICS if mask >> POSE_METRICS.index(n) & 1]
        out = np.zeros((len(order), len(Re), len(Rg)), np.float64)
        _check(load_library().lm_mesh_pose_errors(mesh._h, len(Re), _ptr(Re), _ptr(te), len(Rg), _ptr(Rg), _ptr(tg), _ptr(Kd), W, H, _ptr(scene),
                                                  mask, float(delta), float(tau), 0 if cost == "step" else 1, float(clip_near), float(clip_far),
                                                  _ptr(out)))
        res.update({n: out[i] for i, n in enumerate(order)})
    if sym_mask:
        if symmetries is None:
            Rs, ts = np.eye(3).reshape(1, 9), np.zeros((1, 3))
        else:
            Rs, ts = np.asarray(symmetries[0], np.float64), np.asarray(symmetries[1], np.float64)
            if Rs.ndim != 3 or Rs.shape[1:] != (3, 3) or ts.shape != (len(Rs), 3):
                raise ValueError("symmetries must be (Rs (S,3,3), ts (S,3)), got %s and %s" % (Rs.shape, ts.shape))
            Rs, ts = np.ascontiguousarray(Rs.reshape(-1, 9)), np.ascontiguousarray(ts)
        order = [n for i, n in enumerate(POSE_METRICS_SYM) if sym_mask >> (6 + i) & 1]
        out = np.zeros((len(order), len(Re), len(Rg)), np.float64)
        _check(load_library().lm_mesh_pose_errors_sym(mesh._h, len(Re), _ptr(Re), _ptr(te), len(Rg), _ptr(Rg), _ptr(tg), len(Rs), _ptr(Rs), _ptr(ts),
                                                      _ptr(Kd), sym_mask, _ptr(out)))
        res.update({n: out[i] for i, n in enumerate(order)})
    return res


def gt_stats(mesh: Mesh, R_gt, t_gt, K, scene_depth, delta=15.0, clip_near=100.0, clip_far=2000.0):
    """tools/calc_gt_stats.py:103-155 for each GT pose on the device (lm_mesh_gt_stats): a list of dicts with px_count_all,
    px_count_visib, px_count_valid, visib_fract, bbox_obj and bbox_visib.  Clip planes: renderer.render's defaults."""
    Rg, tg = _pose_batch(R_gt, t_gt, "ground truth")
    scene = _scene_mm(scene_depth)
    Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    n = len(Rg)
    counts = np.zeros((n, 3), np.int64)
    fract = np.zeros(n, np.float64)
    bo = np.zeros((n, 4), np.int32)
    bv = np.zeros((n, 4), np.int32)
    _check(load_library().lm_mesh_gt_stats(mesh._h, n, _ptr(Rg), _ptr(tg), _ptr(Kd), scene.shape[1], scene.shape[0], _ptr(scene), float(delta),
                                           float(clip_near), float(clip_far), _ptr(counts), _ptr(fract), _ptr(bo), _ptr(bv)))
    return [{"px_count_all": int(counts[i, 0]), "px_count_visib": int(counts[i, 2]), "px_count_valid": int(counts[i, 1]),
             "visib_fract": float(fract[i]), "bbox_obj": [int(e) for e in bo[i]], "bbox_visib": [int(e) for e in bv[i]]} for i in range(n)]


def symmetry_transforms(discrete=(), continuous=(), max_sym_disc_step=0.01):
    """The set of symmetry transformations of an object model, as the BOP toolkit builds it from a model's
    symmetries_discrete / symmetries_continuous: (Rs (S,3,3), ts (S,3)) float64, S >= 1.
    discrete: 4x4 matrices or flat lists of 16 numbers (row-major); D = the identity followed by them (R the upper-left 3x3,
    t the last column, mm).  continuous: pairs (axis[3], offset[3]); with n = ceil(pi / max_sym_disc_step) and step = 2 pi / n,
    each contributes for i = 1 .. n-1 the rotation R_i by i * step about the axis (Rodrigues) with t_i = offset - R_i offset;
    C concatenates them in the order given.  Without continuous symmetries the result is D; otherwise, for d in D (outer)
    and c in C (inner), R = R_c R_d and t = R_c t_d + t_c (D's plain entries are not kept, as in the BOP toolkit)."""
    D = [(np.eye(3), np.zeros(3))]
    for sym in discrete:
        M = np.asarray(sym, np.float64)
        if M.size != 16:
            raise RuntimeError("a discrete symmetry is a 4x4 matrix or 16 numbers, got shape %s" % (M.shape,))
        M = M.reshape(4, 4)
        if not np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]):
            raise RuntimeError("a discrete symmetry's bottom row must be 0 0 0 1, got %s" % (M[3].tolist(),))
        D.append((M[:3, :3].copy(), M[:3, 3].copy()))
    if not max_sym_disc_step > 0:
        raise RuntimeError("max_sym_disc_step must be > 0")
    C = []
    n = int(np.ceil(np.pi / max_sym_disc_step))
    step = 2.0 * np.pi / n
    for axis, offset in continuous:
        a = np.asarray(axis, np.float64).reshape(3)
        off = np.asarray(offset, np.float64).reshape(3)
        norm = np.sqrt(a.dot(a))
        if not norm > 0 or not np.isfinite(norm):
            raise RuntimeError("a continuous symmetry's axis must have a non-zero length, got %s" % (a.tolist(),))
        a = a / norm
        Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        for i in range(1, n):
            R = np.eye(3) + np.sin(i * step) * Kx + (1.0 - np.cos(i * step)) * (Kx @ Kx)
            C.append((R, off - R @ off))
    if C:
        D = [(Rc @ Rd, Rc @ td + tc) for Rd, td in D for Rc, tc in C]
    return np.stack([R for R, _ in D]), np.stack([t for _, t in D])


def match_poses(errs, scores, error_thresh, max_ests_count=-1, gt_valid_mask=None):
    """pysixd/pose_matching.py:4-36 on the (E, G) error table of one metric, GT ids 0..G-1: estimates in the order of
    decreasing score (stable: equal scores keep their input order), the best max_ests_count of them if that is > 0, each
    greedily matched to the unmatched valid GT of the lowest error (strict <: the first lowest wins) if that error is
    < error_thresh.  gt_valid_mask: None or empty = all valid.  Returns [{est_id, gt_id, score, error, error_norm}]."""
    errs = np.asarray(errs, np.float64)
    scores = np.asarray(scores, np.float64).reshape(-1)
    if errs.ndim != 2 or len(scores) != errs.shape[0]:
        raise ValueError("errs must be (E, G) with one score per estimate, got %s and %s" % (errs.shape, scores.shape))
    valid = None if gt_valid_mask is None or len(gt_valid_mask) == 0 else [bool(v) for v in gt_valid_mask]
    if valid is not None and len(valid) != errs.shape[1]:
        raise ValueError("gt_valid_mask has %d entries for %d GTs" % (len(valid), errs.shape[1]))
    order = sorted(range(len(scores)), key=lambda e: scores[e], reverse=True)
    if max_ests_count > 0:
        order = order[:max_ests_count]
    matches, matched = [], set()
    for e in order:
        best_gt, best_error = -1, float("inf")
        for g in range(errs.shape[1]):
            error = float(errs[e, g])
            if (valid is None or valid[g]) and g not in matched and error < best_error:
                best_gt, best_error = g, error
        if best_error < error_thresh:
            matched.add(best_gt)
            matches.append({"est_id": int(e), "gt_id": best_gt, "score": float(scores[e]), "error": best_error,
                            "error_norm": best_error / float(error_thresh)})
    return matches


def recall(errs_per_image, scores_per_image, error_thresholds, max_ests_count=-1, gt_valid_masks=None):
    """The recall of one error type over a set of images (tools/eval_loc.py:81-125 for one object): the fraction of valid GT
    instances that match_poses matches, per threshold, averaged over error_thresholds (a number or a sequence; the BOP
    average recall of one error type when given bop19_thresholds).  errs_per_image: (E_i, G_i) tables; scores_per_image:
    (E_i,); gt_valid_masks: None or one mask (or None) per image.  With max_ests_count > 0 an image counts at most that many
    targets (eval_loc.py:107-108).  No targets: 0.0 (calc_recall)."""
    ths = np.atleast_1d(np.asarray(error_thresholds, np.float64))
    if len(errs_per_image) != len(scores_per_image) or (gt_valid_masks is not None and len(gt_valid_masks) != len(errs_per_image)):
        raise ValueError("one score array (and one mask) per error table")
    if ths.size == 0:
        raise ValueError("no error threshold")
    masks = [None] * len(errs_per_image) if gt_valid_masks is None else list(gt_valid_masks)
    targets = 0
    for errs, mask in zip(errs_per_image, masks):
        n = np.asarray(errs).shape[1] if mask is None or len(mask) == 0 else int(np.count_nonzero(mask))
        targets += min(n, max_ests_count) if max_ests_count > 0 else n
    if targets == 0:
        return 0.0
    recalls = []
    for th in ths:
        tp = sum(len(match_poses(errs, sc, float(th), max_ests_count, mask)) for errs, sc, mask in zip(errs_per_image, scores_per_image, masks))
        recalls.append(tp / float(targets))
    return float(np.mean(recalls))


def bop19_thresholds(diameter, width):
    """The BOP-19 thresholds of correctness: (MSSD: 0.05, 0.10 .. 0.50 of the object diameter (mm);
    MSPD: 5 r, 10 r .. 50 r pixels, r = image width / 640)."""
    r = width / 640.0
    return [k / 20.0 * diameter for k in range(1, 11)], [5.0 * k * r for k in range(1, 11)]
