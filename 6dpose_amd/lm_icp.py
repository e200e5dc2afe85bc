"""Pose refinement of the drop-in: poseRefine, the batched calls, the resident IcpContext and the per-frame Pipeline
(lm_pose_refine*, lm_icp_*, lm_pipeline_*)."""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

from lm_abi import (LM_ICP_POINT_TO_POINT, LM_ICP_SCENE_FROM_SCENE, IcpOptions, PipelineTimings, _CDetection, _CPoseResult, _as_depth,
                    _check, _ptr, load_library)
from lm_detector import nms_norms
from lm_render import Mesh


ICP_ESTIMATIONS = ("point_to_plane", "point_to_point")


def _icp_flags(scene_from_scene, estimation) -> int:
    if estimation not in ICP_ESTIMATIONS:
        raise RuntimeError("estimation must be 'point_to_plane' or 'point_to_point' (got %r)" % (estimation,))
    return (LM_ICP_SCENE_FROM_SCENE if scene_from_scene else 0) | (LM_ICP_POINT_TO_POINT if estimation == "point_to_point" else 0)


def _icp_options(max_iteration, relative_fitness, relative_rmse) -> Optional[IcpOptions]:
    """The criteria as lm_icp_options, None when they are the defaults; the checks of lm_icp_set_options, made before anything is
    created or launched."""
    if int(max_iteration) != max_iteration or max_iteration < 0 or max_iteration > 2 ** 31 - 3:
        raise RuntimeError("max_iteration must be an integer >= 0 (got %r)" % (max_iteration,))
    for name, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        if not (float(v) > 0.0 and np.isfinite(float(v))):
            raise RuntimeError("%s must be a positive finite number (got %r)" % (name, v))
    o = IcpOptions(int(max_iteration), 0, float(relative_fitness), float(relative_rmse))
    return None if (o.max_iteration, o.relative_fitness, o.relative_rmse) == (30, 1e-6, 1e-6) else o


class poseRefine:
    """poseRefine (LL.h:8-19, LL.cpp:27-170).  `scene_from_scene=True` registers against the scene
    cloud instead of reproducing LL.cpp:109 (which down-samples the model cloud twice).  estimation: "point_to_plane" (LL.cpp:128-130)
    or "point_to_point" (the reference built without USE_OPEN3D_P2PL, LL.cpp:132-134); max_iteration, relative_fitness, relative_rmse:
    open3d's ICPConvergenceCriteria (max_iteration=0: EvaluateRegistration of the initial guess).  With criteria other than the defaults
    the object runs an IcpContext of its own instead of the shared per-device one."""

    def __init__(self, device: Optional[int] = None, scene_from_scene: bool = False, estimation: str = "point_to_plane",
                 max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6):
        self.residual = -1.0                                   # poseRefine(): residual(-1)
        self._R = None
        self._t = None
        self.device = device
        self.flags = _icp_flags(scene_from_scene, estimation)
        self._criteria = (max_iteration, relative_fitness, relative_rmse) if _icp_options(max_iteration, relative_fitness, relative_rmse) is not None else None
        self._ctx = None
        self.info = {}

    def process(self, sceneDepth, modelDepth, sceneK, modelK, modelR, modelT, detectX: int, detectY: int) -> None:
        lib = load_library()
        sd, md = _as_depth(sceneDepth, "sceneDepth"), _as_depth(modelDepth, "modelDepth")
        if sd.shape != md.shape:
            raise RuntimeError("sceneDepth and modelDepth sizes differ")
        def f32(a, n, what):
            a = np.asarray(a)
            if a.dtype != np.float32 or a.size != n:
                raise RuntimeError("%s must be float32 with %d elements (got %s %s)" % (what, n, a.dtype, a.shape))
            return np.ascontiguousarray(a).reshape(-1)
        sK, mK, R, t = f32(sceneK, 9, "sceneK"), f32(modelK, 9, "modelK"), f32(modelR, 9, "modelR"), f32(modelT, 3, "modelT")
        dev = self.device
        if dev is None:
            dev = int(os.environ.get("LOCAL_RANK", "0")) if lib.lm_device_count() > 1 else 0
        res = _CPoseResult()
        if self._criteria is not None:
            if self._ctx is None:
                self._ctx = IcpContext(dev, max_iteration=self._criteria[0], relative_fitness=self._criteria[1], relative_rmse=self._criteria[2])
                self._ctx.flags = self.flags
            self._ctx.set_scene(sd, sK)
            self._ctx.set_models([md])
            res = self._ctx._run_raw(mK, R, t, [(int(detectX), int(detectY))])[0][0]
        else:
            _check(lib.lm_pose_refine(dev, _ptr(sd), _ptr(md), sd.shape[1], sd.shape[0], _ptr(sK), _ptr(mK), _ptr(R), _ptr(t),
                                      int(detectX), int(detectY), self.flags, ctypes.byref(res)))
        self.residual = float(res.residual)
        if self.residual == -1.0:                              # LL.cpp:52-55: outputs untouched
            return
        self._R = np.array(res.R, np.float64).reshape(3, 3)
        self._t = np.array(res.t, np.float64).reshape(3, 1)
        self.info = {"inlier_rmse": float(res.inlier_rmse), "iterations": int(res.iterations),
                     "n_source": int(res.n_source), "n_target": int(res.n_target), "stage": int(res.stage)}

    def getResidual(self) -> float:
        return self.residual

    def getR(self):
        return self._R

    def getT(self):
        return self._t


def pose_refine_batch(scene_depth, scene_K, model_depths, model_Ks, model_Rs, model_ts, detect_xy, device=0,
                      scene_from_scene=False, estimation="point_to_plane", max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """lm_pose_refine_batch: top-K hypotheses of one frame in one ICP launch.  Returns (list of dict, device_ms).  estimation and the
    criteria: see poseRefine; criteria other than the defaults run on an IcpContext of the call's own."""
    lib = load_library()
    flags = _icp_flags(scene_from_scene, estimation)
    if _icp_options(max_iteration, relative_fitness, relative_rmse) is not None:
        ctx = IcpContext(device, scene_from_scene, estimation, max_iteration, relative_fitness, relative_rmse)
        try:
            ctx.set_scene(scene_depth, scene_K)
            ctx.set_models(model_depths)
            return ctx.run(model_Ks, model_Rs, model_ts, detect_xy)
        finally:
            ctx.close()
    sd = _as_depth(scene_depth, "scene_depth")
    n = len(model_depths)
    mds = [_as_depth(m, "model_depth") for m in model_depths]
    ptrs = (ctypes.c_void_p * n)(*[m.ctypes.data for m in mds])
    Ks = np.ascontiguousarray(np.asarray(model_Ks, np.float32).reshape(n, 9))
    Rs = np.ascontiguousarray(np.asarray(model_Rs, np.float32).reshape(n, 9))
    ts = np.ascontiguousarray(np.asarray(model_ts, np.float32).reshape(n, 3))
    xy = np.ascontiguousarray(np.asarray(detect_xy, np.int32).reshape(n, 2))
    sK = np.ascontiguousarray(np.asarray(scene_K, np.float32).reshape(9))
    res = (_CPoseResult * n)()
    ms = ctypes.c_float()
    _check(lib.lm_pose_refine_batch(device, _ptr(sd), sd.shape[1], sd.shape[0], _ptr(sK), n, ptrs, _ptr(Ks), _ptr(Rs), _ptr(ts),
                                    _ptr(xy), flags, res, ctypes.byref(ms)))
    return [_pose_dict(r) for r in res], float(ms.value)


def evaluate_registration(scene_depth, scene_K, model_depths, model_Ks, model_Rs, model_ts, detect_xy, device=0, scene_from_scene=False):
    """open3d EvaluateRegistration of every hypothesis' initial guess (LL.cpp:111-115): pose_refine_batch with max_iteration=0, nothing
    is refined.  Returns (fitness, inlier_rmse), two float arrays with one entry per hypothesis; fitness -1 where the detection window
    leaves the frame (LL.cpp:52-55)."""
    res, _ = pose_refine_batch(scene_depth, scene_K, model_depths, model_Ks, model_Rs, model_ts, detect_xy, device=device,
                               scene_from_scene=scene_from_scene, max_iteration=0)
    return np.array([r["residual"] for r in res], np.float64), np.array([r["rmse"] for r in res], np.float64)


def _pose_dict(r):
    """One lm_pose_result as the result dict; stage: the ICP stage that finished the hypothesis (1 first team launch, 2 large team builds,
    3 sliced launches; 0 not registered)."""
    return {"R": np.array(r.R).reshape(3, 3), "t": np.array(r.t), "residual": float(r.residual), "rmse": float(r.inlier_rmse),
            "iterations": int(r.iterations), "n_source": int(r.n_source), "n_target": int(r.n_target), "stage": int(r.stage)}


class IcpContext:
    """lm_icp (include/amd_linemod.h): batched poseRefine with the depth images resident in HBM.
    set_scene(depth, K) once per frame, set_models(list of depth_ren) into slots, then run(...) any
    number of times; run returns (list of dict like pose_refine_batch, device_ms).  estimation and the criteria: see poseRefine."""

    def __init__(self, device: int = 0, scene_from_scene: bool = False, estimation: str = "point_to_plane", max_iteration: int = 30,
                 relative_fitness: float = 1e-6, relative_rmse: float = 1e-6):
        flags = _icp_flags(scene_from_scene, estimation)
        opt = _icp_options(max_iteration, relative_fitness, relative_rmse)
        lib = load_library()
        self._lib = lib
        self._h = ctypes.c_void_p()
        _check(lib.lm_icp_create(int(device), ctypes.byref(self._h)))
        self.flags = flags
        self.num_models = 0
        if opt is not None:
            _check(lib.lm_icp_set_options(self._h, ctypes.byref(opt)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lm_icp_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def set_scene(self, scene_depth, scene_K):
        sd = _as_depth(scene_depth, "scene_depth")
        sK = np.ascontiguousarray(np.asarray(scene_K, np.float32).reshape(9))
        _check(self._lib.lm_icp_set_scene(self._h, _ptr(sd), sd.shape[1], sd.shape[0], _ptr(sK)))
        self.shape = sd.shape

    def set_models(self, model_depths, first_slot: int = 0):
        mds = [_as_depth(m, "model_depth") for m in model_depths]
        for m in mds:
            if m.shape != self.shape:
                raise RuntimeError("sceneDepth and modelDepth sizes differ")
        ptrs = (ctypes.c_void_p * len(mds))(*[m.ctypes.data for m in mds])
        _check(self._lib.lm_icp_set_models(self._h, int(first_slot), len(mds), ptrs))
        self.num_models = max(self.num_models, first_slot + len(mds))

    def run(self, model_Ks, model_Rs, model_ts, detect_xy, model_slots=None):
        res, ms = self._run_raw(model_Ks, model_Rs, model_ts, detect_xy, model_slots)
        return [_pose_dict(r) for r in res], ms

    def _run_raw(self, model_Ks, model_Rs, model_ts, detect_xy, model_slots=None):
        n = len(detect_xy)
        Ks = np.ascontiguousarray(np.asarray(model_Ks, np.float32).reshape(n, 9))
        Rs = np.ascontiguousarray(np.asarray(model_Rs, np.float32).reshape(n, 9))
        ts = np.ascontiguousarray(np.asarray(model_ts, np.float32).reshape(n, 3))
        xy = np.ascontiguousarray(np.asarray(detect_xy, np.int32).reshape(n, 2))
        slots = None if model_slots is None else np.ascontiguousarray(np.asarray(model_slots, np.int32).reshape(n))
        res = (_CPoseResult * n)()
        ms = ctypes.c_float()
        _check(self._lib.lm_icp_run(self._h, n, None if slots is None else _ptr(slots), _ptr(Ks), _ptr(Rs), _ptr(ts), _ptr(xy),
                                    self.flags, res, ctypes.byref(ms)))
        return res, float(ms.value)

    def read_debug(self, hypothesis: int, kind: int):
        n = self._lib.lm_icp_read_debug(self._h, int(hypothesis), int(kind), None, 0)
        if n < 0:
            _check(int(n))
        out = np.zeros(int(n), np.float64)
        if n:
            self._lib.lm_icp_read_debug(self._h, int(hypothesis), int(kind), _ptr(out), int(n))
        return out if kind >= 3 else out.reshape(-1, 3)


class Pipeline:
    """lm_pipeline (include/amd_linemod.h): the per-frame loop of linemod_and_levelup_test.py:324-372 — match, boxes,
    nms, poseRefine on the first top_k kept matches — as one stream of device work on the detector's resident frame.
    set_views(class_id, depth_rens, Ks, Rs, ts) uploads what the driver renders per matched template; run(...) returns
    (list of dict(x, y, similarity, class_index, template_id, width, height, status, R, t, residual, iterations...),
    timings dict).  estimation and the criteria of its poseRefine: see poseRefine."""

    def __init__(self, detector: "Detector", width: int, height: int, scene_from_scene: bool = False, estimation: str = "point_to_plane",
                 max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6):
        flags = _icp_flags(scene_from_scene, estimation)
        opt = _icp_options(max_iteration, relative_fitness, relative_rmse)
        self._lib = load_library()
        self._det = detector
        self._h = ctypes.c_void_p()
        _check(self._lib.lm_pipeline_create(detector._h, int(width), int(height), ctypes.byref(self._h)))
        self.flags = flags
        if opt is not None:
            _check(self._lib.lm_pipeline_set_icp_options(self._h, ctypes.byref(opt)))
        self.shape = (int(height), int(width))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lm_pipeline_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def set_views(self, class_id: str, depth_rens, Ks, Rs, ts, first_template: int = 0, box_wh=None):
        mds = [_as_depth(m, "depth_ren") for m in depth_rens]
        for m in mds:
            if m.shape != self.shape:
                raise RuntimeError("depth rendering size differs from the pipeline's frame size")
        n = len(mds)
        ptrs = (ctypes.c_void_p * n)(*[m.ctypes.data for m in mds])
        Ks = np.ascontiguousarray(np.asarray(Ks, np.float32).reshape(n, 9))
        Rs = np.ascontiguousarray(np.asarray(Rs, np.float32).reshape(n, 9))
        ts = np.ascontiguousarray(np.asarray(ts, np.float32).reshape(n, 3))
        wh = None if box_wh is None else np.ascontiguousarray(np.asarray(box_wh, np.int32).reshape(n, 2))
        _check(self._lib.lm_pipeline_set_views(self._h, class_id.encode(), int(first_template), n, ptrs, _ptr(Ks), _ptr(Rs), _ptr(ts),
                                               None if wh is None else _ptr(wh)))

    def set_views_rendered(self, class_id: str, mesh: "Mesh", Ks, Rs, ts, first_template: int = 0, clip_near=10.0, clip_far=10000.0, box_wh=None):
        """depth_ren of every template view rendered on the device straight into the resident slots."""
        n, Ks, Rs, ts = Mesh._views(Ks, Rs, ts)
        wh = None if box_wh is None else np.ascontiguousarray(np.asarray(box_wh, np.int32).reshape(n, 2))
        _check(self._lib.lm_pipeline_set_views_rendered(self._h, mesh._h, class_id.encode(), int(first_template), n, _ptr(Ks), _ptr(Rs), _ptr(ts),
                                                        float(clip_near), float(clip_far), None if wh is None else _ptr(wh)))

    def read_icp_debug(self, hypothesis: int, kind: int):
        """IcpContext.read_debug for the hypotheses of the last run()."""
        f = self._lib.lm_pipeline_read_icp_debug
        n = f(self._h, int(hypothesis), int(kind), None, 0)
        if n < 0:
            _check(int(n))
        out = np.zeros(int(n), np.float64)
        if n:
            f(self._h, int(hypothesis), int(kind), _ptr(out), int(n))
        return out if kind >= 3 else out.reshape(-1, 3)

    def run(self, threshold: float, class_ids: Sequence[str], scene_K, top_k: int = 16, nms_iou: float = 0.5,
            norms_thresh: Optional[float] = None):
        """One frame of the driver loop on the device.  norms_thresh (mm): additionally the translation NMS the ROS node applies
        to the refined poses (linemod_ros/detect.py:128, `nms_norms(ts, ts_scores, 40.0)` with score = -residual): the refined
        detections are returned in its keep order, the suppressed ones dropped.  Deliberate difference: a detection whose
        refinement failed (status != 0: window outside the frame, LL.cpp:52-55, or no rendered view) is left out here, whereas the
        node's shared `poseRefine` object would hand `nms_norms` residual -1 (score +1, ranked first) together with the STALE R / t of
        the previous detection — a reference defect this does not reproduce.  Tie order among equal scores: see lm_nms_norms."""
        ids = [c.encode() for c in class_ids]
        arr = (ctypes.c_char_p * len(ids))(*ids) if ids else None
        sK = np.ascontiguousarray(np.asarray(scene_K, np.float32).reshape(9))
        out = (_CDetection * int(top_k))()
        n = ctypes.c_int()
        tm = PipelineTimings()
        _check(self._lib.lm_pipeline_run(self._h, float(threshold), arr, len(ids), _ptr(sK), int(top_k), float(nms_iou), self.flags, out,
                                         ctypes.byref(n), ctypes.byref(tm)))
        res = []
        for i in range(n.value):
            o = out[i]
            res.append({"x": int(o.match.x), "y": int(o.match.y), "similarity": float(o.match.similarity),
                        "class_index": int(o.match.class_index), "template_id": int(o.match.template_id),
                        "width": int(o.width), "height": int(o.height), "status": int(o.status), **_pose_dict(o.pose)})
        if norms_thresh is not None:
            posed = [r for r in res if r["status"] == 0]
            keep = nms_norms(np.array([r["t"] for r in posed], np.float64).reshape(-1, 3), np.array([-r["residual"] for r in posed], np.float64),
                             float(norms_thresh)) if posed else []
            res = [posed[i] for i in keep]
        return res, tm.as_dict()
