"""The rasteriser of the drop-in: Mesh (render, overlay, diameter), its options and training from rendered views
(lm_mesh_*, lm_detector_add_templates_rendered*)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from lm_abi import RenderOptions, _as_depth, _as_rgb, _check, _ptr, load_library


SHADINGS = {"phong": 0, "flat": 1}                                 # LM_SHADING_*
OVERLAY_MODES = {"painter": 0, "nearest": 1}                       # LM_OVERLAY_*


def _colour(c, name, sizes):
    c = np.asarray(c, np.float64).ravel()
    if c.size not in sizes or not np.all((c >= 0) & (c <= 1)):     # NaN fails too
        raise RuntimeError("%s must be %s values in [0, 1], got %r" % (name, " or ".join(map(str, sizes)), c.tolist()))
    return c


def render_options(shading="phong", texture=False, surf_color=None, bg_color=(0, 0, 0, 0), ambient_weight=0.8, ssaa=4, clip_near=10.0,
                   clip_far=10000.0) -> RenderOptions:
    """renderer.render's keywords (renderer.py:306) as an lm_render_options."""
    if shading not in SHADINGS:
        raise RuntimeError("unknown shading %r (known: %s)" % (shading, ", ".join(SHADINGS)))
    o = RenderOptions()
    o.size = ctypes.sizeof(RenderOptions)
    o.shading, o.use_texture, o.ambient, o.ssaa, o.clip_near, o.clip_far = SHADINGS[shading], int(bool(texture)), float(ambient_weight), int(ssaa), \
        float(clip_near), float(clip_far)
    if surf_color is not None:
        o.has_surf_color = 1
        o.surf_color[:] = _colour(surf_color, "surf_color", (3,)).tolist()
    bg = _colour(bg_color, "bg_color", (3, 4))
    o.bg_color[:] = (bg.tolist() + [0.0])[:4]
    return o


class Mesh:
    """lm_mesh (include/amd_linemod.h): a triangle mesh resident in HBM and its rasteriser — what the reference driver
    gets from pysixd (inout.load_ply + renderer.render).  Mesh(path) loads a PLY (with texture_u / texture_v when the file
    has them); Mesh(pts, faces, normals=, colors=, texture_uv=) takes arrays (model dict keys of pysixd: 'pts', 'faces',
    'normals', 'colors', 'texture_uv').  set_texture(image) attaches the texture image."""

    def __init__(self, pts_or_path, faces=None, normals=None, colors=None, device: int = 0, texture_uv=None):
        lib = load_library()
        self._lib = lib
        self._h = ctypes.c_void_p()
        if isinstance(pts_or_path, (str, bytes, os.PathLike)):
            _check(lib.lm_mesh_load_ply(int(device), os.fspath(pts_or_path).encode(), ctypes.byref(self._h)))
        else:
            V = np.ascontiguousarray(np.asarray(pts_or_path, np.float32).reshape(-1, 3))
            Fc = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
            Nn = None if normals is None else np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
            Cc = None if colors is None else np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(-1, 3))
            _check(lib.lm_mesh_create(int(device), _ptr(V), None if Nn is None else _ptr(Nn), None if Cc is None else _ptr(Cc), len(V),
                                      _ptr(Fc), len(Fc), ctypes.byref(self._h)))
        nv, nf = ctypes.c_int(), ctypes.c_int()
        _check(lib.lm_mesh_counts(self._h, ctypes.byref(nv), ctypes.byref(nf)))
        self.num_vertices, self.num_faces = nv.value, nf.value
        if texture_uv is not None:
            uv = np.ascontiguousarray(np.asarray(texture_uv, np.float32).reshape(-1, 2))
            _check(lib.lm_mesh_set_texcoords(self._h, _ptr(uv), len(uv)))

    def set_texture(self, image):
        """Attaches the texture image (H_t, W_t, 3): uint8, or float in [0, 1] which is quantised with rint(x * 255) — pysixd keeps
        float textures as floats (renderer.py:316-321), this library stores 8-bit texels.  Row 0 is the top of the image, as loaded;
        the flip pysixd applies before the upload is part of the lookup rule (render.hip)."""
        img = np.asarray(image)
        if img.ndim != 3 or img.shape[2] != 3 or img.size == 0:
            raise RuntimeError("a texture is an (H, W, 3) image, got shape %r" % (img.shape,))
        if img.dtype != np.uint8:
            if not np.issubdtype(img.dtype, np.floating) or not np.all((img >= 0) & (img <= 1)):
                raise RuntimeError("a texture is uint8 or float in [0, 1]")
            img = np.rint(img.astype(np.float64) * 255.0).astype(np.uint8)
        img = np.ascontiguousarray(img)
        _check(self._lib.lm_mesh_set_texture(self._h, _ptr(img), img.shape[1], img.shape[0]))

    @property
    def has_texture(self) -> bool:
        uv, w, h = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self._lib.lm_mesh_texture_info(self._h, ctypes.byref(uv), ctypes.byref(w), ctypes.byref(h)))
        return bool(uv.value) and w.value > 0 and h.value > 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lm_mesh_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    @staticmethod
    def _views(Ks, Rs, ts):
        Rs = np.ascontiguousarray(np.asarray(Rs, np.float32).reshape(-1, 9))
        n = len(Rs)
        Ks = np.asarray(Ks, np.float32)
        Ks = np.ascontiguousarray(np.tile(Ks.reshape(1, 9), (n, 1)) if Ks.size == 9 else Ks.reshape(n, 9))
        ts = np.ascontiguousarray(np.asarray(ts, np.float32).reshape(n, 3))
        return n, Ks, Rs, ts

    def render(self, im_size, Ks, Rs, ts, clip_near=10.0, clip_far=10000.0, ambient_weight=0.8, ssaa=4, mode="rgb+depth", shading="phong",
               texture=False, surf_color=None, bg_color=(0, 0, 0, 0)):
        """renderer.render for a batch of views; im_size = (width, height).  Returns depth uint16 (n,H,W) and / or rgb uint8 (n,H,W,3).
        shading, texture, surf_color and bg_color are pysixd's keywords (renderer.py:306); texture=True uses the image attached with
        set_texture (pysixd passes the image itself).  The defaults here stay this library's: shading='phong', ambient_weight=0.8 —
        pysixd's own defaults are shading='flat' and ambient_weight=0.5, so a call that relied on those passes them explicitly."""
        W, H = int(im_size[0]), int(im_size[1])
        n, Ks, Rs, ts = self._views(Ks, Rs, ts)
        opts = render_options(shading, texture, surf_color, bg_color, ambient_weight, ssaa, clip_near, clip_far)
        depth = np.zeros((n, H, W), np.uint16) if "depth" in mode else None
        rgb = np.zeros((n, H, W, 3), np.uint8) if "rgb" in mode else None
        if shading == "phong" and not texture and surf_color is None and not any(opts.bg_color[:3]):    # the call as it always was
            _check(self._lib.lm_mesh_render(self._h, n, W, H, _ptr(Ks), _ptr(Rs), _ptr(ts), float(clip_near), float(clip_far), float(ambient_weight),
                                            int(ssaa), None if depth is None else _ptr(depth), None if rgb is None else _ptr(rgb)))
        else:
            _check(self._lib.lm_mesh_render_ex(self._h, n, W, H, _ptr(Ks), _ptr(Rs), _ptr(ts), ctypes.byref(opts), None if depth is None else _ptr(depth),
                                               None if rgb is None else _ptr(rgb)))
        if mode == "depth":
            return depth
        if mode == "rgb":
            return rgb
        return rgb, depth

    def overlay(self, rgb, K, Rs, ts, surf_colors=None, scene_depth=None, mode="painter", hide_occluded=False, meshes=None, clip_near=100.0,
                clip_far=2000.0, ambient_weight=0.5, shading="flat", texture=False):
        """Pose overlays on the device (linemod_and_levelup_test.py:377-383, tools/vis_gt_poses.py:120-145): every pose rendered at the
        frame's size with pysixd's defaults (flat, ambient 0.5, clip 100 / 2000, no supersampling) and composed into a copy of rgb
        (H,W,3 uint8).  surf_colors (n,3) in [0,1]: one colour per pose (the driver's color_list).  meshes: one Mesh per pose where
        the poses belong to different objects (default: this mesh for all).  mode='painter' pastes the poses in order, later over
        earlier, where render_depth > 0; mode='nearest' shows the pose with the smallest rendered depth per pixel.  With scene_depth
        (H,W uint16 mm) and hide_occluded=True a pose shows only where scene_depth == 0 or render_depth < scene_depth.
        Returns (composed image, int8 (H,W) index of the pose that shows, -1 where none).  draw_axis is not part of this."""
        if mode not in OVERLAY_MODES:
            raise RuntimeError("unknown overlay mode %r (known: %s)" % (mode, ", ".join(OVERLAY_MODES)))
        frame = _as_rgb(rgb)
        H, W = frame.shape[:2]
        n, Ks, Rs, ts = self._views(K, Rs, ts)
        ms = [self] * n if meshes is None else list(meshes)
        if len(ms) != n:
            raise RuntimeError("%d meshes for %d poses" % (len(ms), n))
        handles = (ctypes.c_void_p * n)(*[m._h.value for m in ms])
        sc = None
        if surf_colors is not None:
            sc = np.ascontiguousarray(np.asarray(surf_colors, np.float32).reshape(-1, 3))
            if len(sc) != n:
                raise RuntimeError("%d surf_colors for %d poses" % (len(sc), n))
        scene = None
        if hide_occluded:
            if scene_depth is None:
                raise RuntimeError("hide_occluded needs scene_depth")
            scene = _as_depth(scene_depth)
            if scene.shape != (H, W):
                raise RuntimeError("scene_depth size differs from the frame's")
        opts = render_options(shading, texture, None, (0, 0, 0, 0), ambient_weight, 1, clip_near, clip_far)
        out = np.zeros((H, W, 3), np.uint8)
        index = np.zeros((H, W), np.int8)
        _check(self._lib.lm_mesh_overlay(handles, n, W, H, _ptr(frame), _ptr(Ks), _ptr(Rs), _ptr(ts), None if sc is None else _ptr(sc),
                                         ctypes.byref(opts), None if scene is None else _ptr(scene), OVERLAY_MODES[mode], _ptr(out), _ptr(index)))
        return out, index

    def diameter(self) -> float:
        """misc.calc_pts_diameter: the largest vertex-to-vertex distance (mm), on the device (k_pose_pts)."""
        d = ctypes.c_double()
        _check(self._lib.lm_mesh_diameter(self._h, ctypes.byref(d)))
        return d.value


def add_templates_rendered(detector: "Detector", mesh: Mesh, class_id: str, im_size, Ks, Rs, ts, clip_near=10.0, clip_far=10000.0,
                           ambient_weight=0.8, ssaa=4, shading="phong", texture=False, bg_color=(0, 0, 0, 0)):
    """The render_train loop of the driver (linemod_and_levelup_test.py:170-252) on the device.  Returns (template ids (n,),
    -1 where addTemplate failed; box_wh (n,2) = aTemplateInfo 'width','height').  shading / texture / bg_color as Mesh.render:
    texture=True trains a textured model from its texture, as the driver does (:193-227)."""
    n, Ks, Rs, ts = Mesh._views(Ks, Rs, ts)
    ids = np.zeros(n, np.int32)
    wh = np.zeros((n, 2), np.int32)
    opts = render_options(shading, texture, None, bg_color, ambient_weight, ssaa, clip_near, clip_far)
    if shading == "phong" and not texture and not any(opts.bg_color[:3]):
        _check(load_library().lm_detector_add_templates_rendered(detector._h, mesh._h, class_id.encode(), n, int(im_size[0]), int(im_size[1]), _ptr(Ks),
                                                                 _ptr(Rs), _ptr(ts), float(clip_near), float(clip_far), float(ambient_weight), int(ssaa),
                                                                 _ptr(ids), _ptr(wh)))
    else:
        _check(load_library().lm_detector_add_templates_rendered_ex(detector._h, mesh._h, class_id.encode(), n, int(im_size[0]), int(im_size[1]),
                                                                    _ptr(Ks), _ptr(Rs), _ptr(ts), ctypes.byref(opts), _ptr(ids), _ptr(wh)))
    return ids, wh
