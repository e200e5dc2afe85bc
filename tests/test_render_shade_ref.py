"""CPU tests of the shading restatement (tests/render_shade_ref.py: flat, texture, surf_color, bg_color, overlays), evaluated
in software through the restatement alone, and of the public surface the shading options add."""
import inspect
import os
import re

import numpy as np

import render_oracle as ro
import render_shade_ref as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
K = np.array([500.0, 0, 32, 0, 500.0, 24, 0, 0, 1]).reshape(3, 3)          # the principal point is pixel (32, 24)
R0, T0 = np.eye(3), np.array([0.0, 0.0, 500.0])
# a fronto-parallel quad of 100 mm: 100 px wide at 500 mm, so it overhangs the 64 x 48 frame; QUAD_S is one that fits
QUAD = np.array([[-50, -50, 0], [50, -50, 0], [50, 50, 0], [-50, 50, 0]], np.float64)
QUAD_S = QUAD * 0.2                                                        # 20 x 20 px around the principal point
QF = np.array([[0, 1, 2], [0, 2, 3]])
QUV = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], np.float32)               # vertex 0 = the image's top-left corner of the quad


def test_defaults_restate_the_render_oracle():
    from synth import icosphere
    V, F, N, C = icosphere(1, seed=3)
    Rm = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]]); t = np.array([5.0, -3.0, 600.0])
    Kc = np.array([572.4, 0, 80, 0, 573.6, 60, 0, 0, 1]).reshape(3, 3)
    want = ro.render_rgb(V.astype(np.float64), N.astype(np.float64), C.astype(np.float64), F, Kc, Rm, t, 160, 120, ambient=0.5, ssaa=2)
    got = rs.render_shaded(V, F, Kc, Rm, t, 160, 120, ambient=0.5, ssaa=2, N=N, C=C)
    assert (want.sum(2) > 0).sum() > 300 and np.array_equal(got, want)


def test_flat_quad_has_one_colour_per_triangle_and_full_light_on_the_axis():
    colour = (0.2, 0.6, 0.9)
    img, tri = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=0.5, ssaa=1, shading="flat", surf_color=colour, return_samples=True)
    want = np.rint(min(1.0, 0.5 + 1.0) * rs.quantise_colour(colour))      # at the principal point e is parallel to the face normal
    assert tri[24, 32] >= 0 and np.array_equal(img[24, 32], want)
    for f in (0, 1):                                                       # |cos| > 0.5 over the whole quad, so the light saturates: one colour
        px = img[tri == f]
        assert len(px) > 100 and len(np.unique(px, axis=0)) == 1
    # without ambient light the colour at the principal point is still the full colour (diffuse = 1) and falls off away from it
    dark, _ = rs.render_shaded(QUAD, QF, K, R0, T0, W, H, ambient=0.0, ssaa=1, shading="flat", surf_color=colour, return_samples=True)
    assert np.array_equal(dark[24, 32], want) and dark[0, 0, 2] < dark[24, 32, 2]
    # tilted by 60 degrees about x: diffuse = cos 60 on the axis, the same for both windings (flat is two-sided) ...
    a = np.radians(60.0)
    Rt = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    lit = [rs.render_shaded(QUAD_S, faces, K, Rt, T0, W, H, ambient=0.2, ssaa=1, shading="flat", surf_color=colour, return_samples=True)[0]
           for faces in (QF, QF[:, ::-1])]
    assert np.array_equal(lit[0], lit[1])
    assert np.abs(lit[0][24, 32] - (0.2 + 0.5) * rs.quantise_colour(colour)).max() <= 1
    # ... whereas phong with normals that point away from the camera leaves the ambient term only
    Naway = np.tile([0.0, 0.0, 1.0], (4, 1))
    ph = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=0.2, ssaa=1, shading="phong", N=Naway, surf_color=colour, return_samples=True)[0]
    assert np.array_equal(ph[24, 32], np.rint(0.2 * rs.quantise_colour(colour)))
    # a degenerate face (zero normal) has diffuse 0 by rule; it covers no pixel, so the rule shows in the formula only
    assert np.array_equal(np.cross(QUAD[1] - QUAD[0], QUAD[1] - QUAD[0]), np.zeros(3))


def test_texture_lands_with_the_image_top_left_at_uv_0_1():
    tex = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8)   # top: red green, bottom: blue white
    img = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=1.0, ssaa=1, uv=QUV, texture=tex)
    # the quad covers pixels 22..42 x 14..34; its corner with uv = (0, 1) is the top-left one in the image
    assert np.array_equal(img[16, 24], tex[0, 0]) and np.array_equal(img[16, 40], tex[0, 1])
    assert np.array_equal(img[32, 24], tex[1, 0]) and np.array_equal(img[32, 40], tex[1, 1])
    assert np.array_equal(img[2, 2], [0, 0, 0])
    # the lookup rule itself: nearest, clamp to edge, rows counted from the bottom
    row, col = rs.texel_index(np.array([0.0, 0.49, 0.5, 1.0, 1.7, -0.2]), np.array([1.0, 0.51, 0.49, 0.0, -3.0, 2.0]), 2, 2)
    assert col.tolist() == [0, 0, 1, 1, 1, 0] and row.tolist() == [0, 0, 1, 1, 1, 0]


def test_bg_colour_fills_and_blends_on_the_silhouette():
    bg, colour = (0.0, 1.0, 0.4), (1.0, 0.0, 0.0)
    one = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=1.0, ssaa=1, surf_color=colour, bg_color=bg + (0.3,))   # alpha: accepted, ignored
    assert np.array_equal(one[2, 2], rs.quantise_colour(bg)) and np.array_equal(one[24, 32], [255, 0, 0])
    assert set(map(tuple, one.reshape(-1, 3))) == {(0, 255, 102), (255, 0, 0)}
    # a quad whose edges fall inside pixels: at ssaa 4 the silhouette pixels are a mix of the two colours, nothing else changes
    V = QUAD_S + np.array([0.3, 0.25, 0.0])
    four = rs.render_shaded(V, QF, K, R0, T0, W, H, ambient=1.0, ssaa=4, surf_color=colour, bg_color=bg)
    mixed = [p for p in set(map(tuple, four.reshape(-1, 3))) if p not in ((0, 255, 102), (255, 0, 0))]
    assert mixed and all(0 < p[0] < 255 and 0 < p[1] < 255 and 0 < p[2] < 102 for p in mixed)
    samples, tri = rs.render_shaded(V, QF, K, R0, T0, W, H, ambient=1.0, ssaa=4, surf_color=colour, bg_color=bg, return_samples=True)
    y, x = next((y, x) for y in range(H) for x in range(W) if tuple(four[y, x]) in mixed)
    cov = (tri[4 * y:4 * y + 4, 4 * x:4 * x + 4] >= 0).sum()
    want = np.floor((2 * (cov * np.array([255, 0, 0]) + (16 - cov) * np.array([0, 255, 102])) + 16) / 32)
    assert 0 < cov < 16 and np.array_equal(four[y, x], want)


def test_surf_colour_overrides_vertex_colours_and_texture_overrides_both():
    C = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]], np.float64)
    tex = np.full((2, 2, 3), 77, np.uint8)
    vert = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=1.0, ssaa=1, C=C)
    surf = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=1.0, ssaa=1, C=C, surf_color=(0.4, 0.4, 1.0))
    both = rs.render_shaded(QUAD_S, QF, K, R0, T0, W, H, ambient=1.0, ssaa=1, C=C, surf_color=(0.4, 0.4, 1.0), uv=QUV, texture=tex)
    cov = vert.sum(2) > 0
    assert cov.sum() > 300 and len(np.unique(vert[cov], axis=0)) > 50
    assert np.array_equal(np.unique(surf[cov], axis=0), [[102, 102, 255]]) and np.array_equal(surf[~cov], vert[~cov])
    assert np.array_equal(np.unique(both[cov], axis=0), [[77, 77, 77]])


def test_overlay_modes():
    frame = np.random.default_rng(0).integers(0, 256, (4, 6, 3)).astype(np.uint8)
    d0 = np.zeros((4, 6), np.uint16); d0[:, :4] = 500
    d1 = np.zeros((4, 6), np.uint16); d1[:, 2:] = 700
    d2 = np.zeros((4, 6), np.uint16); d2[1:3, 3:5] = 500                   # ties with pose 0 at column 3
    layers = [(np.full((4, 6, 3), 10 * (p + 1), np.uint8), d) for p, d in enumerate((d0, d1, d2))]
    out, idx = rs.overlay(frame, layers, mode="painter")
    assert idx[0].tolist() == [0, 0, 1, 1, 1, 1] and idx[1].tolist() == [0, 0, 1, 2, 2, 1]
    out, idx = rs.overlay(frame, layers, mode="nearest")
    assert idx[0].tolist() == [0, 0, 0, 0, 1, 1] and idx[1].tolist() == [0, 0, 0, 0, 2, 1]
    assert np.array_equal(out[idx == 2], np.full(((idx == 2).sum(), 3), 30)) and idx.dtype == np.int8
    scene = np.full((4, 6), 600, np.uint16); scene[3] = 0                  # hides pose 1 (700 mm) except where the scene has no depth
    out, idx = rs.overlay(frame, layers, scene_depth=scene, mode="painter")
    assert idx[0].tolist() == [0, 0, 0, 0, -1, -1] and idx[1].tolist() == [0, 0, 0, 2, 2, -1] and idx[3].tolist() == [0, 0, 1, 1, 1, 1]
    assert np.array_equal(out[idx < 0], frame[idx < 0])


def test_public_surface_carries_the_shading_options():
    """Fails before the shading options exist: the keywords and the C entry points are the feature's interface."""
    import linemodLevelup_pybind as lm
    render = inspect.signature(lm.Mesh.render).parameters
    for name, default in (("shading", "phong"), ("texture", False), ("surf_color", None), ("bg_color", (0, 0, 0, 0)), ("ambient_weight", 0.8),
                          ("ssaa", 4), ("clip_near", 10.0), ("clip_far", 10000.0), ("mode", "rgb+depth")):
        assert name in render and render[name].default == default, name
    assert "pysixd" in lm.Mesh.render.__doc__ and "'flat'" in lm.Mesh.render.__doc__ and "0.5" in lm.Mesh.render.__doc__
    ov = inspect.signature(lm.Mesh.overlay).parameters
    assert list(ov)[:5] == ["self", "rgb", "K", "Rs", "ts"]
    for name, default in (("surf_colors", None), ("scene_depth", None), ("mode", "painter"), ("hide_occluded", False), ("shading", "flat"),
                          ("ambient_weight", 0.5), ("clip_near", 100.0), ("clip_far", 2000.0)):
        assert name in ov and ov[name].default == default, name
    train = inspect.signature(lm.add_templates_rendered).parameters
    for name, default in (("shading", "phong"), ("texture", False), ("bg_color", (0, 0, 0, 0)), ("ambient_weight", 0.8), ("ssaa", 4)):
        assert name in train and train[name].default == default, name
    assert "texture_uv" in inspect.signature(lm.Mesh.__init__).parameters and callable(lm.Mesh.set_texture)
    assert "rint" in lm.Mesh.set_texture.__doc__ and "pysixd" in lm.Mesh.set_texture.__doc__
    hdr = open(os.path.join(ROOT, "include", "amd_linemod.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("lm_mesh_set_texcoords", "lm_mesh_set_texture", "lm_mesh_render_ex", "lm_mesh_overlay", "lm_detector_add_templates_rendered_ex",
                "lm_render_options_init"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert "typedef struct lm_render_options" in hdr and re.search(r"lm_render_options\s*\{\s*uint32_t size;", hdr)
    # the old entry points keep their signatures
    assert re.search(r"int lm_mesh_render\(lm_mesh \*m, int count, int width, int height, const float \*Ks, const float \*Rs, const float \*ts,\s*"
                     r"float clip_near, float clip_far, float ambient, int ssaa, uint16_t \*depth_out, uint8_t \*rgb_out\);", hdr)


def test_bad_options_raise_before_any_device_call():
    import pytest

    import linemodLevelup_pybind as lm
    for bad in (dict(shading="gouraud"), dict(surf_color=(0.1, 1.2, 0.0)), dict(bg_color=(0.0, -0.1, 0.0)), dict(bg_color=(0.0, 0.0)),
                dict(surf_color=(float("nan"), 0, 0))):
        with pytest.raises(RuntimeError):
            lm.render_options(**bad)
