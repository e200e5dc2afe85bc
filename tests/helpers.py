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
# which kernels prepared the clouds: groups of k_icp_voxel_wide that finished the model / scene cloud and of k_icp_grid_wide (SORT_GROUPS: the
# wide path did the cloud; less: k_icp_voxel / k_icp_grid did), points handed to k_icp_knn_far, points its list had no room for (its list holds
# every target, so 0)
DBG3_VOX_DONE_MODEL, DBG3_VOX_DONE_SCENE, DBG3_GRID_DONE, DBG3_KNN_FAR, DBG3_KNN_FAR_REFUSED = 68, 69, 70, 71, 72
SORT_GROUPS = 8                                                   # kIcpSortGroups (icp_kernels.h)


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


def class_raw(od, lms_sizes, bank_arrays, T, thr, cls):
    """match_oracle.c on one class of a request (cls = its position in the request) against prepared linear memories."""
    import linemod_oracle as lo
    feat, offs, wh = bank_arrays
    lms, sizes = lms_sizes
    P = (len(offs) - 1) // (2 * len(T))
    raw, st = lo.match_bank_c(lo.PackedBank(P, len(T), feat, offs, wh), lms, sizes, T, thr)
    raw["cls"] = cls
    return raw, st


def box_of(cls_spec, tid, E):
    """NMS box of template tid of a class: the caller's box_wh where one is given and its width is not negative (lm_pipeline_set_views:
    NULL / negative = the template's own size), else the level-0 size of the template."""
    box = cls_spec.get("box")
    b = None if box is None else (box.get(tid) if isinstance(box, dict) else box[tid])
    if b is not None and int(b[0]) >= 0:
        return int(b[0]), int(b[1])
    w, h = cls_spec["bank"][2][tid * E]
    return int(w), int(h)


def nms_chain_oracle(od, rgb, dep, classes, T, thr, iou, top_k, lms_sizes=None, raws=None):
    """The driver loop up to the selection, on the CPU ORACLE only, for a request of several classes: classes[i] = dict(bank=(feat,
    offs, wh), box=None | list | {tid: (w, h)}) is the class at position i of the request (= class_index of its matches).
    match_oracle.c per class -> canonical sort / unique -> boxes x, y, x+w, y+h -> numpy nms, stable.  raws: the per-class raw records
    when the caller has them already (a list like classes).  Returns a dict: sel = the first top_k kept (x, y, sim, cls, tid, w, h),
    survivors = what the nms keeps in all, m = distinct (x, y, tid, cls) among the raw records (what the device's greedy loop runs
    over), unique = the list after adjacent-unique, coarse = coarse candidates of the frame, and the tie statistics of tie_stats."""
    import linemod_oracle as lo
    E = 2 * len(T)
    if lms_sizes is None:
        lms_sizes = od.linear_memories(rgb, dep)
    coarse = 0
    if raws is None:
        raws = []
        for i, c in enumerate(classes):
            r, st = class_raw(od, lms_sizes, c["bank"], T, thr, i)
            coarse += st["coarse_candidates"]
            raws.append(r)
    else:
        raws = [r.copy() for r in raws]
        for i, r in enumerate(raws):
            r["cls"] = i
    raw = np.concatenate(raws) if raws else np.zeros(0, lo.MATCH_DTYPE)
    distinct = set(zip(raw["x"].tolist(), raw["y"].tolist(), raw["tid"].tolist(), raw["cls"].tolist()))
    u = lo.canonical_sort_unique(raw)
    dets = np.zeros((len(u), 5))
    wh = np.zeros((len(u), 2), np.int64)
    for i, r in enumerate(u):
        wh[i] = box_of(classes[int(r["cls"])], int(r["tid"]), E)
        dets[i] = (r["x"], r["y"], r["x"] + wh[i, 0], r["y"] + wh[i, 1], r["sim"])
    keep = lo.nms_boxes(dets, iou, stable=True) if len(u) else []
    sel = [(int(u[i]["x"]), int(u[i]["y"]), float(u[i]["sim"]), int(u[i]["cls"]), int(u[i]["tid"]), int(wh[i, 0]), int(wh[i, 1]))
           for i in keep[:top_k]]
    out = {"sel": sel, "survivors": len(keep), "m": len(distinct), "unique": u, "dets": dets, "keep": keep, "coarse": coarse, "raws": raws}
    out.update(tie_stats(u, len(distinct)))
    return out


def tie_stats(u, m):
    """What a canonical, adjacent-unique match list u (of m distinct raw records) holds for the tie rules of the NMS: tied = entries
    whose similarity another TEMPLATE's entry has too; removed = distinct records adjacent-unique dropped (equal x, y, similarity and
    class across template ids); apart_class / apart_entry = entries that have an equal in (x, y, similarity) left in the list, in
    another class / in their own class (then another entry sits between the two in the canonical order)."""
    by_sim, by_pos = {}, {}
    for r in u:
        by_sim.setdefault(float(r["sim"]), []).append((int(r["cls"]), int(r["tid"])))
        by_pos.setdefault((int(r["x"]), int(r["y"]), float(r["sim"])), []).append(int(r["cls"]))
    tied = sum(len(v) for v in by_sim.values() if len(set(v)) > 1)
    apart_class = sum(len(v) for v in by_pos.values() if len(set(v)) > 1)
    apart_entry = sum(len(v) - len(set(v)) for v in by_pos.values())
    return {"tied": tied, "removed": m - len(u), "apart_class": apart_class, "apart_entry": apart_entry}


def det_fields(g):
    """The exactly comparable fields of a Pipeline.run detection, in the order of nms_chain_oracle's sel."""
    return (g["x"], g["y"], g["similarity"], g["class_index"], g["template_id"], g["width"], g["height"])


def pipeline_oracle(od, rgb, dep, bank, T, wh, E, views, thr, top_k, iou, box=None, scene_K=K_CAM):
    """The driver loop (linemod_and_levelup_test.py:324-372) on the CPU ORACLE only (nothing of the product): match_oracle.c ->
    canonical sort/unique -> numpy nms (the driver's own function) -> oracle poseRefine per kept match.  One class; wh = the
    bank's sizes (bank[2]); the several-class chain is nms_chain_oracle."""
    import linemod_oracle as lo
    ch = nms_chain_oracle(od, rgb, dep, [{"bank": (bank[0], bank[1], wh), "box": box}], T, thr, iou, top_k)
    sel = [ch["unique"][i] for i in ch["keep"][:top_k]]         # planted templates tie in score: stable nms
    poses = []
    for r in sel:
        md, K, R, t = views[int(r["tid"])]
        poses.append(lo.pose_refine(dep, md, scene_K, K, R, t, int(r["x"]), int(r["y"]), scene_from_scene=True))
    return sel, poses
