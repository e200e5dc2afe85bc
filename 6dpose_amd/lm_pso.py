"""Pose refinement by particle swarm over rendered depth (lm_pso_*): the refiner the reference's author left as a todo
(linemodLevelup/readme.md:41-46).  Correspondence-free, so it needs neither a start inside ICP's correspondence radius nor the
depth rendering of the matched template view: a Mesh, the scene depth and the hypotheses are enough.  For a camera without depth the
same swarm scores the rendered contour against the scene's edges instead (set_scene_edges, run(cost="edges"), pso_refine_edges), or
against its quantised gradient orientations, so that an edge of another direction is far away (set_scene_orientations,
run(cost="oriented"), pso_refine_oriented)."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from lm_abi import PsoOptions, _as_depth, _check, _CPsoResult, _ptr, load_library
from lm_render import Mesh

PSO_DEBUG_KINDS = {"x": 0, "cost": 1, "sum_n_r": 2, "best": 3}


def pso_options(particles=64, generations=30, tau=20, trans_range_mm=20.0, rot_range_deg=10.0, seed=0, inertia=0.7298, c1=1.49618, c2=1.49618,
                clip_near=10.0, clip_far=10000.0, cover_pixels=0, rot_range=None) -> PsoOptions:
    """lm_pso_options.  rot_range_deg: the largest rotation about an axis; the library takes rot_range = tan(radians(rot_range_deg) / 2),
    the bound on a Cayley component (rot_range= passes that number itself).  The limits are checked by lm_pso_run."""
    for name, v in (("particles", particles), ("generations", generations), ("tau", tau), ("cover_pixels", cover_pixels), ("seed", seed)):
        if int(v) != v:
            raise RuntimeError("%s must be an integer (got %r)" % (name, v))
    if not 0 <= int(seed) < 2 ** 64:
        raise RuntimeError("seed must be in 0..2**64 - 1 (got %r)" % (seed,))
    for name, v in (("particles", particles), ("generations", generations), ("tau", tau), ("cover_pixels", cover_pixels)):
        if not -2 ** 31 <= int(v) < 2 ** 31:
            raise RuntimeError("%s out of range (got %r)" % (name, v))
    o = PsoOptions()
    load_library().lm_pso_options_init(ctypes.byref(o))
    o.particles, o.generations, o.tau, o.cover_pixels, o.seed = int(particles), int(generations), int(tau), int(cover_pixels), int(seed)
    o.trans_range_mm = float(trans_range_mm)
    o.rot_range = float(rot_range) if rot_range is not None else math.tan(math.radians(float(rot_range_deg)) / 2.0)
    o.inertia, o.c1, o.c2, o.clip_near, o.clip_far = float(inertia), float(c1), float(c2), float(clip_near), float(clip_far)
    return o


def _result_dict(r):
    return {"R": np.array(r.R, np.float64).reshape(3, 3), "t": np.array(r.t, np.float64), "cost": float(r.cost), "initial_cost": float(r.initial_cost),
            "n_rendered": int(r.n_rendered), "n_initial": int(r.n_initial), "best_particle": int(r.best_particle),
            "best_generation": int(r.best_generation)}


def derive_windows(K, ts, radius_mm, window_size=None):
    """The windows of pso_refine(windows=None): per hypothesis the projection of the sphere of radius_mm around t0, rounded outwards to
    whole pixels; one size for the call, the largest extent rounded up to a multiple of 8 and clamped to 8..256 (or window_size), every
    window centred on its sphere.  Returns (int32 [n][2] origins, (w, h))."""
    K = np.asarray(K, np.float64).reshape(3, 3); ts = np.asarray(ts, np.float64).reshape(-1, 3)
    boxes = []
    for t in ts:
        z = max(float(t[2]) - float(radius_mm), 1.0)                     # the sphere's nearest point bounds its image
        cu, cv = K[0, 0] * t[0] / t[2] + K[0, 2], K[1, 1] * t[1] / t[2] + K[1, 2]
        ru, rv = K[0, 0] * radius_mm / z, K[1, 1] * radius_mm / z
        boxes.append((math.floor(cu - ru), math.ceil(cu + ru), math.floor(cv - rv), math.ceil(cv + rv)))
    if window_size is None:
        w = max(b[1] - b[0] + 1 for b in boxes); h = max(b[3] - b[2] + 1 for b in boxes)
        w, h = (min(max(-(-int(v) // 8) * 8, 8), 256) for v in (w, h))
    else:
        w, h = int(window_size[0]), int(window_size[1])
    xy = np.array([[(b[0] + b[1] + 1 - w) // 2, (b[2] + b[3] + 1 - h) // 2] for b in boxes], np.int32).reshape(-1, 2)
    return xy, (w, h)


class PsoContext:
    """lm_pso (include/amd_linemod.h): set_scene(depth, K) once per frame, then run(mesh, Rs, ts, windows, window_size, **options) any
    number of times; set_scene_edges(edges, K) and run(..., cost="edges") score against an edge map instead, set_scene_orientations(Q, K)
    and run(..., cost="oriented") against an orientation map, and a context may hold all three scenes.  run returns (list of dict(R, t, cost, initial_cost, n_rendered, n_initial, best_particle, best_generation),
    device_ms); options: see pso_options."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        _check(self._lib.lm_pso_create(int(device), ctypes.byref(self._h)))
        self.K = self.edge_K = self.orient_K = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lm_pso_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def set_scene(self, scene_depth, scene_K):
        sd = _as_depth(scene_depth, "scene_depth")
        K = np.ascontiguousarray(np.asarray(scene_K, np.float64).reshape(9))
        _check(self._lib.lm_pso_set_scene(self._h, _ptr(sd), sd.shape[1], sd.shape[0], _ptr(K)))
        self.K, self.shape = K.reshape(3, 3), sd.shape

    def set_scene_edges(self, edges, K, max_dist=32):
        """The edge scene of run(cost="edges"): a uint8 or bool H x W array (an edge where it is not 0) and its camera.  Computes the
        squared distance to the nearest edge, truncated at max_dist pixels (1..255), once; independent of set_scene's depth."""
        e = np.asarray(edges)
        if e.dtype not in (np.uint8, np.bool_) or e.ndim != 2 or e.size == 0:
            raise RuntimeError("edges must be a uint8 or bool HxW edge map (got %s %s)" % (e.dtype, e.shape))
        if int(max_dist) != max_dist or not -2 ** 31 <= int(max_dist) < 2 ** 31:
            raise RuntimeError("max_dist must be an integer in 1..255 (got %r)" % (max_dist,))
        e = np.ascontiguousarray(e).view(np.uint8)
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        self.edge_K = None
        _check(self._lib.lm_pso_set_scene_edges(self._h, _ptr(e), e.shape[1], e.shape[0], _ptr(K), int(max_dist)))
        self.edge_K, self.edge_shape = K.reshape(3, 3), e.shape

    @staticmethod
    def _orient_args(max_dist, orient_penalty):
        for name, v in (("max_dist", max_dist), ("orient_penalty", orient_penalty)):
            if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
                raise RuntimeError("%s must be an integer (got %r)" % (name, v))
        return int(max_dist), int(orient_penalty)

    def set_scene_orientations(self, Q, K, max_dist=32, orient_penalty=16):
        """The oriented scene of run(cost="oriented"): a uint8 H x W array whose bit k (0..7) says "an edge of orientation bin k here"
        (LINE-MOD's quantised colour gradients, det.readStage(level, 0); several bits may be set, 0 = no edge) and its camera.  Computes,
        once, the truncated squared distance in (x, y, orientation) to the nearest oriented edge for each of the eight bins, and the
        undirected distance of set_scene_edges(Q != 0); max_dist 1..255, orient_penalty 0..4096 in px^2 per bin^2.  The default
        orient_penalty=16 is a choice, not a measurement: an edge one bin off counts as 4 px further away, the opposite bin as 16 px.
        Independent of set_scene's depth and of set_scene_edges' map."""
        q = np.asarray(Q)
        if q.dtype != np.uint8 or q.ndim != 2 or q.size == 0:
            raise RuntimeError("Q must be a uint8 HxW orientation map (got %s %s)" % (q.dtype, q.shape))
        M, P = self._orient_args(max_dist, orient_penalty)
        q = np.ascontiguousarray(q)
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        self.orient_K = None
        _check(self._lib.lm_pso_set_scene_orientations(self._h, _ptr(q), q.shape[1], q.shape[0], _ptr(K), M, P))
        self.orient_K, self.orient_shape = K.reshape(3, 3), q.shape

    def orient_distance(self, plane: int) -> np.ndarray:
        """One of the nine uint16 H x W planes set_scene_orientations computed (tests): 0..7 the bins, 8 the undirected distance."""
        n = self._lib.lm_pso_read_orient_distance(self._h, int(plane), None, 0)
        if n < 0:
            _check(int(n))
        out = np.zeros(self.orient_shape, np.uint16)
        assert out.size == n
        self._lib.lm_pso_read_orient_distance(self._h, int(plane), _ptr(out), int(n))
        return out

    def set_scene_from_detector(self, det, K, size, level=0, max_dist=32, directional=False, orient_penalty=16):
        """directional=False: set_scene_edges with LINE-MOD's own edge pixels of the detector's last front end run: det.readStage(level, 0) != 0, i.e. the
        colour gradients that survived blur, Sobel, the strongest channel and the hysteresis vote, the very pixels the templates were
        matched on.  size: (width, height) of the source frame of that run (the detector does not report it); the map has
        det.alignedSize(width, height) >> level, and K is the camera of that pyramid level.  The map makes a host round trip of one
        byte per pixel (device -> host in readStage, host -> device here).
        directional=True: set_scene_orientations with that map itself, its bins kept, handed over on the device
        (lm_pso_set_scene_from_detector): no byte of it crosses PCIe.  Refused while the detector has frames in flight, before its first
        front end, without the colour modality, and across devices."""
        w, h = (int(v) >> int(level) for v in det.alignedSize(int(size[0]), int(size[1])))
        if directional:
            M, P = self._orient_args(max_dist, orient_penalty)
            K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
            n = int(self._lib.lm_detector_read_stage(det._h, int(level), 0, None, 0))    # the stage's size; < 0: the hand-over refuses with its own message
            if n >= 0 and n != w * h:                                                    # before anything is replaced, as on the host path
                raise RuntimeError("the detector's stage has %d pixels, a %dx%d frame has %dx%d at level %d" % (n, size[0], size[1], w, h, level))
            self.orient_K = None
            _check(self._lib.lm_pso_set_scene_from_detector(self._h, det._h, int(level), _ptr(K), M, P))
            self.orient_K, self.orient_shape = K.reshape(3, 3), (h, w)
            return
        q = det.readStage(int(level), 0)
        if q.size != w * h:
            raise RuntimeError("the detector's stage has %d pixels, a %dx%d frame has %dx%d at level %d" % (q.size, size[0], size[1], w, h, level))
        self.set_scene_edges((q != 0).reshape(h, w), K, max_dist)

    def edge_distance(self) -> np.ndarray:
        """The uint16 H x W truncated squared distance set_scene_edges computed (tests)."""
        n = self._lib.lm_pso_read_edge_distance(self._h, None, 0)
        if n < 0:
            _check(int(n))
        out = np.zeros(self.edge_shape, np.uint16)
        assert out.size == n
        self._lib.lm_pso_read_edge_distance(self._h, _ptr(out), int(n))
        return out

    def run(self, mesh: Mesh, Rs, ts, windows=None, window_size=None, **options):
        """cost="depth" (the default) scores against set_scene's depth; cost="edges" against set_scene_edges' map, tau in pixels
        (<= max_dist), with edge_step_mm (0..65535; 0 = the silhouette only) the depth jump of the rendered model that counts as a
        contour; cost="oriented" against set_scene_orientations' planes, the same contour with each pixel reading the plane of its own
        orientation.  The other keywords: pso_options."""
        cost, edge_step_mm = options.pop("cost", "depth"), options.pop("edge_step_mm", 0)
        if cost not in ("depth", "edges", "oriented"):
            raise RuntimeError("cost must be 'depth' or 'edges' or 'oriented' (got %r)" % (cost,))
        if int(edge_step_mm) != edge_step_mm or not 0 <= int(edge_step_mm) <= 65535:
            raise RuntimeError("edge_step_mm must be an integer in 0..65535 (got %r)" % (edge_step_mm,))
        scene_K = {"depth": self.K, "edges": self.edge_K, "oriented": self.orient_K}[cost]
        opts = pso_options(**options)
        Rs = np.ascontiguousarray(np.asarray(Rs, np.float64).reshape(-1, 9))
        n = len(Rs)
        ts = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(n, 3))
        if windows is None:
            if scene_K is None:
                raise RuntimeError({"depth": "no scene depth set (set_scene)", "edges": "no scene edges set (set_scene_edges)",
                                    "oriented": "no scene orientations set (set_scene_orientations)"}[cost])
            windows, window_size = derive_windows(scene_K, ts, mesh.diameter() / 2.0 + opts.trans_range_mm, window_size)
        elif window_size is None:
            raise RuntimeError("windows need a window_size")
        xy = np.ascontiguousarray(np.asarray(windows, np.int32).reshape(n, 2))
        res = (_CPsoResult * max(n, 1))()
        ms = ctypes.c_float()
        head = (self._h, mesh._h, n, _ptr(Rs), _ptr(ts), _ptr(xy), int(window_size[0]), int(window_size[1]), ctypes.byref(opts))
        if cost == "edges":
            _check(self._lib.lm_pso_run_edges(*head, int(edge_step_mm), res, ctypes.byref(ms)))
        elif cost == "oriented":
            _check(self._lib.lm_pso_run_oriented(*head, int(edge_step_mm), res, ctypes.byref(ms)))
        else:
            _check(self._lib.lm_pso_run(*head, res, ctypes.byref(ms)))
        return [_result_dict(res[i]) for i in range(n)], float(ms.value)

    def read_debug(self, hypothesis: int, kind):
        """The record of the last run for one hypothesis, generation 0 (the initial swarm) to `generations`.  kind 'x': float64 (G+1, P, 6)
        positions evaluated; 'cost': (G+1, P); 'sum_n_r': int64 (G+1, P, 2); 'best': int64 (G+1, 2) particle and generation of the global
        best after each generation."""
        k = PSO_DEBUG_KINDS[kind] if isinstance(kind, str) else int(kind)
        f = self._lib.lm_pso_read_debug
        n = f(self._h, int(hypothesis), k, None, 0)
        if n < 0:
            _check(int(n))
        out = np.zeros(int(n), np.float64)
        if n:
            f(self._h, int(hypothesis), k, _ptr(out), int(n))
        gens = int(f(self._h, int(hypothesis), 3, None, 0)) // 2         # kind 3 is [G + 1][2]
        if k == 0:
            return out.reshape(gens, -1, 6)
        if k == 1:
            return out.reshape(gens, -1)
        if k == 2:
            return out.astype(np.int64).reshape(gens, -1, 2)
        return out.astype(np.int64).reshape(gens, 2)


def pso_refine(mesh: Mesh, scene_depth, K, Rs, ts, windows=None, window_size=None, device: int = 0, **options):
    """One call: a context of its own, set_scene, run.  Returns (list of dict, device_ms) like PsoContext.run.  With windows=None the
    window of each hypothesis is derived on the host (derive_windows) from the sphere around t0 of radius Mesh.diameter() / 2 +
    trans_range_mm."""
    ctx = PsoContext(device)
    try:
        ctx.set_scene(scene_depth, K)
        return ctx.run(mesh, Rs, ts, windows, window_size, **options)
    finally:
        ctx.close()


def pso_refine_edges(mesh: Mesh, edges, K, Rs, ts, windows=None, window_size=None, device: int = 0, max_dist=32, edge_step_mm=0, **options):
    """pso_refine for a camera without depth: a context of its own, set_scene_edges(edges, K, max_dist), run(cost="edges").  tau is in
    pixels here (<= max_dist); the cost is the mean squared distance in px^2 from the rendered contour to the nearest scene edge."""
    ctx = PsoContext(device)
    try:
        ctx.set_scene_edges(edges, K, max_dist)
        return ctx.run(mesh, Rs, ts, windows, window_size, cost="edges", edge_step_mm=edge_step_mm, **options)
    finally:
        ctx.close()


def pso_refine_oriented(mesh: Mesh, Q, K, Rs, ts, windows=None, window_size=None, device: int = 0, max_dist=32, orient_penalty=16, edge_step_mm=0,
                        **options):
    """pso_refine_edges with orientations: a context of its own, set_scene_orientations(Q, K, max_dist, orient_penalty),
    run(cost="oriented").  Q is LINE-MOD's quantised orientation map (bit k = an edge of bin k); the cost is the mean squared distance
    in px^2 from the rendered contour to the nearest scene edge in (x, y, orientation).  orient_penalty=16 is a choice, not a measurement."""
    ctx = PsoContext(device)
    try:
        ctx.set_scene_orientations(Q, K, max_dist, orient_penalty)
        return ctx.run(mesh, Rs, ts, windows, window_size, cost="oriented", edge_step_mm=edge_step_mm, **options)
    finally:
        ctx.close()
