"""Shared helpers for the test-suite (image loading, hashing, the scene camera, the oracle-only match -> NMS -> poseRefine
chain, the layout of the ICP read-back)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the scene camera of the ICP and pipeline tests (the reference fixture's)
K_CAM = np.array([572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1], np.float32).reshape(3, 3)

# entries of IcpContext.read_debug(h, 3) (lm_icp_read_debug kind 3, pose_refine.cpp)
DBG3_TEAM_NOTE, DBG3_TEAM_SIZE, DBG3_RESUME_IT, DBG3_BUILD = 33, 65, 66, 67


def load_bgr(name):
    """cv::imread order (BGR) as test.cpp does."""
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, name)).convert("RGB"))[:, :, ::-1])


def load_u16(name):
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, name))).astype(np.uint16)


def load_gray(name):
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, name)).convert("L"))


def h16(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def oracle_matches(od, rgb, dep, bank_arrays, T, thr, cls=0):
    """match_oracle.c on a packed bank: the raw (pre-unique) match records and the pass statistics."""
    import linemod_oracle as lo
    feat, offs, wh = bank_arrays
    lms, sizes = od.linear_memories(rgb, dep)
    P = (len(offs) - 1) // (2 * len(T))
    raw, st = lo.match_bank_c(lo.PackedBank(P, len(T), feat, offs, wh), lms, sizes, T, thr)
    raw["cls"] = cls
    return raw, st


def pipeline_oracle(od, rgb, dep, bank, T, wh, E, views, thr, top_k, iou, box=None, scene_K=K_CAM):
    """The driver loop (linemod_and_levelup_test.py:324-372) on the CPU ORACLE only (nothing of the product): match_oracle.c ->
    canonical sort/unique -> numpy nms (the driver's own function) -> oracle poseRefine per kept match."""
    import linemod_oracle as lo
    raw, _ = oracle_matches(od, rgb, dep, bank, T, thr)
    m = lo.canonical_sort_unique(raw)
    dets = np.zeros((len(m), 5))
    for i, r in enumerate(m):
        w, h = wh[int(r["tid"]) * E] if box is None else box[int(r["tid"])]
        dets[i] = (r["x"], r["y"], r["x"] + w, r["y"] + h, r["sim"])
    keep = lo.nms_boxes(dets, iou, stable=True)[:top_k] if len(m) else []      # planted templates tie in score
    sel = [m[i] for i in keep]
    poses = []
    for r in sel:
        md, K, R, t = views[int(r["tid"])]
        poses.append(lo.pose_refine(dep, md, scene_K, K, R, t, int(r["x"]), int(r["y"]), scene_from_scene=True))
    return sel, poses
