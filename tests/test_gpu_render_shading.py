"""GPU tests of the rasteriser's shading options (flat shading, textures, surf_color, bg_color), of the pose overlays and of
textured render_train against the numpy restatement tests/render_shade_ref.py.

Exact legs: with ambient_weight = 1 the light is 1 and the colour arithmetic has no rounding freedom, so at ssaa = 1 the
render equals the restatement byte for byte — this pins the texel index and the flip.  Lit legs: the tolerance of the
existing colour test (test_gpu_render.py: max <= 2 grey levels, mean < 0.05, equal coverage), which here covers the
rounding of the lighting product only, the texel being exact."""
import ctypes
import os
import struct

import numpy as np
import pytest

import render_oracle as ro
import render_shade_ref as rs

pytestmark = pytest.mark.gpu

K_CAM = np.array([572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1], np.float32).reshape(3, 3)
K_HALF = K_CAM * np.array([[.5], [.5], [1]], np.float32)


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


from synth import icosphere  # noqa: E402


def look_at_views(n, dist=600.0, seed=1):
    import views
    vs, _ = views.sample_views(42, dist, tilt_step=0.7 * np.pi)
    idx = np.random.default_rng(seed).choice(len(vs), n, replace=False)
    Rs = np.stack([vs[i]["R"] for i in idx]).astype(np.float32)
    ts = np.stack([vs[i]["t"].ravel() for i in idx]).astype(np.float32)
    ts[:, 0] += np.linspace(-40, 40, n); ts[:, 1] += np.linspace(25, -25, n)
    return Rs, ts


def spherical_uv(V):
    d = V / np.linalg.norm(V, axis=1, keepdims=True)
    return np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], 1).astype(np.float32)


def random_texture(seed, block=1):
    """64 x 48 texels in 30..255 (never black, so colour coverage can be compared); block > 1 gives patches with edges between them."""
    rng = np.random.default_rng(seed)
    t = rng.integers(30, 256, (48 // block, 64 // block, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(t, block, 0), block, 1))


def sphere_case():
    """Subdivision-2 icosphere with spherical uv; the second view is cut by the right edge of the frame."""
    V, F, N, C = icosphere(2, seed=3)
    Rs, ts = look_at_views(2, seed=5)
    ts[1, 0] += 290.0
    return dict(V=V, F=F, N=N, C=C, uv=spherical_uv(V), Rs=Rs, ts=ts, near=10.0, far=10000.0)


def cube_case():
    """The close-up cube of test_large_triangles_and_frame_edges (both views leave the frame), with per-vertex uv beyond [0, 1]."""
    s = 80.0
    V = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], np.float32)
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    a, b = np.radians(33.0), np.radians(-21.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]); Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rs = np.stack([Rx @ Ry, Ry @ Rx]).astype(np.float32)
    ts = np.array([[150, -90, 420], [-260, 140, 380]], np.float32)
    uv = np.random.default_rng(8).uniform(-0.2, 1.2, (8, 2)).astype(np.float32)
    C = np.random.default_rng(9).integers(40, 256, (8, 3)).astype(np.uint8)
    return dict(V=V, F=F, N=None, C=C, uv=uv, Rs=Rs, ts=ts, near=100.0, far=2000.0)


CASES = {"icosphere": sphere_case, "cube": cube_case}


def make_mesh(lm, c, tex=None):
    mesh = lm.Mesh(c["V"], c["F"], normals=c["N"], colors=c["C"], texture_uv=c["uv"])
    if tex is not None:
        mesh.set_texture(tex)
    return mesh


def ref(c, i, K, W, H, **kw):
    return rs.render_shaded(c["V"], c["F"], K, c["Rs"][i], c["ts"][i], W, H, c["near"], c["far"], N=c["N"], C=c["C"], **kw)


def assert_lit_close(got, want, cover=None, min_cover=500):
    """cover = (got, want) coverage masks; by default the pixels that are not black, as in test_gpu_render.py."""
    diff = np.abs(got.astype(int) - want.astype(int))
    print("lit: max %d mean %.5f" % (diff.max(), diff.mean()))
    assert diff.max() <= 2 and diff.mean() < 0.05, (diff.max(), diff.mean())
    cov_g, cov_w = cover if cover is not None else (got.sum(2) > 0, want.sum(2) > 0)
    assert cov_w.sum() > min_cover and np.array_equal(cov_g, cov_w)


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_texture_surf_colour_and_background(lm, case):
    c = CASES[case]()
    tex = random_texture(4)
    mesh = make_mesh(lm, c, tex)
    W, H = 640, 480
    surf, bg = (0.2, 0.7, 0.45), (0.1, 0.3, 0.9, 0.5)
    kw = dict(clip_near=c["near"], clip_far=c["far"], ambient_weight=1.0, ssaa=1, mode="rgb")
    got_tex = mesh.render((W, H), K_CAM, c["Rs"], c["ts"], texture=True, surf_color=surf, **kw)          # the texture wins over surf_color
    got_surf = mesh.render((W, H), K_CAM, c["Rs"], c["ts"], surf_color=surf, **kw)
    got_bg = mesh.render((W, H), K_CAM, c["Rs"], c["ts"], surf_color=surf, bg_color=bg, **kw)
    got_tbg = mesh.render((W, H), K_CAM, c["Rs"], c["ts"], texture=True, bg_color=bg[:3], shading="flat", **kw)
    edge = False
    for i in range(2):
        cov = ro.render_depth(c["V"], c["F"], K_CAM, c["Rs"][i], c["ts"][i], W, H, c["near"], c["far"])[0] > 0
        assert cov.sum() > 3000
        edge |= bool(cov[0].any() or cov[-1].any() or cov[:, 0].any() or cov[:, -1].any())
        want = ref(c, i, K_CAM, W, H, ambient=1.0, ssaa=1, uv=c["uv"], texture=tex)
        assert len(np.unique(want[cov], axis=0)) > 50                                                       # many texels are in view
        assert np.array_equal(got_tex[i], want), (case, i, "texture")
        assert np.array_equal(got_surf[i], ref(c, i, K_CAM, W, H, ambient=1.0, ssaa=1, surf_color=surf)), (case, i, "surf_color")
        want = ref(c, i, K_CAM, W, H, ambient=1.0, ssaa=1, surf_color=surf, bg_color=bg)
        assert np.array_equal(want[~cov], np.tile(rs.quantise_colour(bg).astype(np.uint8), ((~cov).sum(), 1)))
        assert np.array_equal(got_bg[i], want), (case, i, "bg_color")
        assert np.array_equal(got_tbg[i], ref(c, i, K_CAM, W, H, ambient=1.0, ssaa=1, shading="flat", uv=c["uv"], texture=tex, bg_color=bg)), (case, i)
    assert edge                                                                                              # a view clipped by the frame edge


@pytest.mark.parametrize("case", sorted(CASES))
def test_lit_flat_and_textured_within_a_rounding_step(lm, case):
    c = CASES[case]()
    tex = random_texture(6)
    mesh = make_mesh(lm, c, tex)
    W, H = 320, 240
    kw = dict(clip_near=c["near"], clip_far=c["far"], mode="rgb")
    flat = mesh.render((W, H), K_HALF, c["Rs"], c["ts"], shading="flat", ambient_weight=0.3, ssaa=2, **kw)
    flat_tex = mesh.render((W, H), K_HALF, c["Rs"], c["ts"], shading="flat", texture=True, ambient_weight=0.5, ssaa=1, **kw)
    phong_tex = mesh.render((W, H), K_HALF, c["Rs"], c["ts"], shading="phong", texture=True, ambient_weight=0.5, ssaa=2, **kw)
    for i in range(2):
        assert_lit_close(flat[i], ref(c, i, K_HALF, W, H, ambient=0.3, ssaa=2, shading="flat"))
        assert_lit_close(flat_tex[i], ref(c, i, K_HALF, W, H, ambient=0.5, ssaa=1, shading="flat", uv=c["uv"], texture=tex))
        assert_lit_close(phong_tex[i], ref(c, i, K_HALF, W, H, ambient=0.5, ssaa=2, shading="phong", uv=c["uv"], texture=tex))
    # flat shading is not the phong image: the icosphere shows its facets, the cube (no normals: phong lights it head-on) its faces
    phong = mesh.render((W, H), K_HALF, c["Rs"], c["ts"], shading="phong", ambient_weight=0.3, ssaa=2, **kw)
    assert np.abs(flat.astype(int) - phong.astype(int)).max() > 8


@pytest.mark.parametrize("ssaa", [2, 4])
def test_lit_background_colour_is_averaged_into_the_silhouette(lm, ssaa):
    c = sphere_case()
    mesh = make_mesh(lm, c)
    W, H = 320, 240
    bg = (0.9, 0.2, 0.6)
    got, depth = mesh.render((W, H), K_HALF, c["Rs"], c["ts"], shading="flat", ambient_weight=0.5, ssaa=ssaa, bg_color=bg)
    bg8 = rs.quantise_colour(bg).astype(np.uint8)
    for i in range(2):
        want = ref(c, i, K_HALF, W, H, ambient=0.5, ssaa=ssaa, shading="flat", bg_color=bg)
        # coverage from the depth image: on a non-black background a colour does not tell covered from uncovered
        assert_lit_close(got[i], want, (depth[i] > 0, ro.render_depth(c["V"], c["F"], K_HALF, c["Rs"][i], c["ts"][i], W, H)[0] > 0))
        assert np.array_equal(got[i][0, 0], bg8)
        mixed = (got[i] != bg8).any(2) & (depth[i] == 0)                                      # silhouette pixels whose centre is not covered
        assert mixed.sum() > 20


def test_defaults_are_unchanged_through_the_new_entry_point(lm):
    """The inputs of test_colour_rendering_matches_within_a_rounding_step: lm_mesh_render_ex with shading = phong and no other
    option (the new resolve kernel) returns the bytes of lm_mesh_render (the resolve kernel as it was)."""
    V, F, N, C = icosphere(2, seed=3)
    Rs, ts = look_at_views(2, seed=5)
    mesh = lm.Mesh(V, F, normals=N, colors=C)
    old_rgb, old_depth = mesh.render((320, 240), K_HALF, Rs, ts, ambient_weight=0.5, ssaa=2)
    n, Ks, Rf, tf = lm.Mesh._views(K_HALF, Rs, ts)
    opts = lm.render_options(shading="phong", ambient_weight=0.5, ssaa=2)
    new_rgb, new_depth = np.zeros_like(old_rgb), np.zeros_like(old_depth)
    rc = lm.load_library().lm_mesh_render_ex(mesh._h, n, 320, 240, Ks.ctypes.data_as(ctypes.c_void_p), Rf.ctypes.data_as(ctypes.c_void_p),
                                             tf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(opts), new_depth.ctypes.data_as(ctypes.c_void_p),
                                             new_rgb.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and (old_rgb.sum(3) > 0).sum() > 1000
    assert np.array_equal(new_rgb, old_rgb) and np.array_equal(new_depth, old_depth)
    # and without normals / colours (grey, head-on normal), at the library's own defaults
    bare = lm.Mesh(V, F)
    old = bare.render((320, 240), K_HALF, Rs, ts, mode="rgb")
    opts = lm.render_options()
    new = np.zeros_like(old)
    rc = lm.load_library().lm_mesh_render_ex(bare._h, n, 320, 240, Ks.ctypes.data_as(ctypes.c_void_p), Rf.ctypes.data_as(ctypes.c_void_p),
                                             tf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(opts), None, new.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(new, old)


def test_overlays_in_both_modes_with_and_without_hiding(lm):
    """Three poses of two meshes over a random frame; poses 0 and 1 overlap in the image, pose 2 lies behind the scene's surface."""
    W, H = 320, 240
    Va, Fa, Na, Ca = icosphere(2, radius=50.0, seed=13)
    cube = cube_case()
    Vb, Fb = cube["V"] * 0.5, cube["F"]
    mesh_a, mesh_b = lm.Mesh(Va, Fa, normals=Na, colors=Ca), lm.Mesh(Vb, Fb)
    Rs = np.stack([np.eye(3), cube["Rs"][0], cube["Rs"][1]]).astype(np.float32)
    ts = np.array([[-30, 0, 480], [35, 10, 450], [-290, -70, 700]], np.float32)
    order = [(Va, Fa, Na, Ca), (Vb, Fb, None, None), (Va, Fa, Na, Ca)]
    meshes = [mesh_a, mesh_b, mesh_a]
    colours = np.array([[1.0, 0.2, 0.1], [0.1, 0.9, 0.3], [0.2, 0.3, 1.0]], np.float32)
    frame = np.random.default_rng(5).integers(0, 256, (H, W, 3)).astype(np.uint8)
    scene = np.full((H, W), 470, np.uint16)
    scene[:, :40] = 0                                                       # no scene measurement: nothing is hidden there
    scene[:50] = 2000
    layers = rs.overlay_layers(order, K_HALF, Rs, ts, W, H, surf_colors=colours)
    masks = [d > 0 for _, d in layers]
    assert all(m.sum() > 1000 for m in masks) and (masks[0] & masks[1]).sum() > 500
    seen = {}
    for mode in ("painter", "nearest"):
        for hide in (False, True):
            got, idx = mesh_a.overlay(frame, K_HALF, Rs, ts, surf_colors=colours, scene_depth=scene, mode=mode, hide_occluded=hide, meshes=meshes)
            want, widx = rs.overlay(frame, layers, scene if hide else None, mode)
            assert idx.dtype == np.int8 and np.array_equal(idx, widx), (mode, hide)
            assert np.array_equal(got[idx < 0], frame[idx < 0])
            diff = np.abs(got[idx >= 0].astype(int) - want[idx >= 0].astype(int))
            assert diff.max() <= 2 and diff.mean() < 0.05, (mode, hide, diff.max(), diff.mean())
            seen[mode, hide] = idx
    assert all((seen["painter", False] == p).sum() > 500 for p in range(3))
    assert not np.array_equal(seen["painter", False], seen["nearest", False])            # the overlap is resolved differently
    for mode in ("painter", "nearest"):
        hidden = (seen[mode, False] >= 0) & (seen[mode, True] < 0)
        assert hidden.sum() > 500 and (seen[mode, True] == 2).sum() > 0                   # pose 2 shows only where the scene allows
    # one mesh, its own colours, defaults: the driver's call for a single object
    got, idx = mesh_a.overlay(frame, K_HALF, Rs[[0, 2]], ts[[0, 2]])
    want, widx = rs.overlay(frame, rs.overlay_layers([order[0], order[2]], K_HALF, Rs[[0, 2]], ts[[0, 2]], W, H))
    assert np.array_equal(idx, widx) and np.abs(got.astype(int) - want.astype(int)).max() <= 2


def test_textured_training_equals_the_host_round_trip(lm):
    """add_templates_rendered(texture=True) adds the templates that Mesh.render(texture=True), downloaded, and Detector.addTemplate per
    view add; and the texture matters: some view's features differ from the untextured training."""
    V, F, N, C = icosphere(3, radius=70.0, seed=11)
    Rs, ts = look_at_views(5, dist=520.0, seed=9)
    mesh = lm.Mesh(V, F, normals=N, colors=C, texture_uv=spherical_uv(V))
    mesh.set_texture(random_texture(12, block=8))
    assert mesh.has_texture
    nfeat, T = 63, [4, 8]
    det_a, det_b, det_c = (lm.Detector(nfeat, T, device=0) for _ in range(3))
    ids, wh = lm.add_templates_rendered(det_a, mesh, "obj", (640, 480), K_CAM, Rs, ts, texture=True)
    rgb, depth = mesh.render((640, 480), K_CAM, Rs, ts, texture=True)
    want_ids = []
    for i in range(len(Rs)):
        want_ids.append(det_b.addTemplate([rgb[i], depth[i]], "obj", (depth[i] > 0).astype(np.uint8) * 255))
        ys, xs = np.nonzero(depth[i])
        assert tuple(wh[i]) == (xs.max() - xs.min(), ys.max() - ys.min())
    assert ids.tolist() == want_ids and max(want_ids) >= 0
    for t in [t for t in want_ids if t >= 0]:
        for a, b in zip(det_a.getTemplates("obj", t), det_b.getTemplates("obj", t)):
            assert (a.width, a.height, a.pyramid_level) == (b.width, b.height, b.pyramid_level) and np.array_equal(a.features, b.features)
    ids_c, _ = lm.add_templates_rendered(det_c, mesh, "obj", (640, 480), K_CAM, Rs, ts)    # the same views from the vertex colours
    differ = [i for i in range(len(Rs)) if (ids[i] >= 0) != (ids_c[i] >= 0) or (ids[i] >= 0 and any(
        not np.array_equal(a.features, b.features) for a, b in zip(det_a.getTemplates("obj", int(ids[i])), det_c.getTemplates("obj", int(ids_c[i])))))]
    assert differ, "the texture changed no template"


def _write_ply_uv(path, V, F, uv, binary):
    with open(path, "wb") as f:
        hdr = "ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float texture_u\n" \
              "property float texture_v\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" \
              % ("binary_little_endian" if binary else "ascii", len(V), len(F))
        f.write(hdr.encode())
        for v, t in zip(V, uv):
            f.write(struct.pack("<5f", *v, *t) if binary else ("%r %r %r %r %r\n" % (*map(float, v), *map(float, t))).encode())
        for t in F:
            f.write(struct.pack("<B3i", 3, *t) if binary else ("3 %d %d %d\n" % tuple(t)).encode())


def test_ply_files_with_texture_coordinates_load_like_arrays(lm, tmp_path):
    V, F, N, C = icosphere(1, seed=7)
    uv = spherical_uv(V)
    tex = random_texture(3)
    Rs, ts = look_at_views(1, seed=2)
    ref_mesh = lm.Mesh(V, F, texture_uv=uv)
    ref_mesh.set_texture(tex)
    want = ref_mesh.render((640, 480), K_CAM, Rs, ts, ssaa=2, texture=True)
    assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 50
    for binary in (False, True):
        path = str(tmp_path / ("uv_%d.ply" % binary))
        _write_ply_uv(path, V, F, uv, binary)
        mesh = lm.Mesh(path)
        assert (mesh.num_vertices, mesh.num_faces) == (len(V), len(F)) and not mesh.has_texture
        mesh.set_texture(tex.astype(np.float32) / 255.0)                                      # float in [0, 1]: rint(x * 255)
        assert mesh.has_texture
        got = mesh.render((640, 480), K_CAM, Rs, ts, ssaa=2, texture=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_bad_arguments_raise(lm):
    V, F, N, C = icosphere(1, seed=7)
    Rs, ts = look_at_views(1, seed=2)
    mesh = lm.Mesh(V, F, normals=N, colors=C)
    view = ((64, 48), K_CAM * np.array([[.1], [.1], [1]], np.float32), Rs, ts)
    with pytest.raises(RuntimeError, match="texture"):
        mesh.render(*view, texture=True)                                                      # neither coordinates nor image
    with pytest.raises(RuntimeError, match="texture"):
        lm.add_templates_rendered(lm.Detector(63, [4, 8], device=0), mesh, "obj", (640, 480), K_CAM, Rs, ts, texture=True)
    with pytest.raises(RuntimeError, match="texture"):
        mesh.overlay(np.zeros((48, 64, 3), np.uint8), K_CAM, Rs, ts, texture=True)
    with_uv = lm.Mesh(V, F, texture_uv=spherical_uv(V))
    with pytest.raises(RuntimeError, match="texture"):
        with_uv.render(*view, texture=True)                                                   # coordinates, no image
    with pytest.raises(RuntimeError, match="vertices"):
        lm.Mesh(V, F, texture_uv=spherical_uv(V)[:-1])                                        # uv count != nv
    with pytest.raises(RuntimeError, match="shading"):
        mesh.render(*view, shading="gouraud")
    with pytest.raises(RuntimeError, match="surf_color"):
        mesh.render(*view, surf_color=(0.5, 1.5, 0.0))
    with pytest.raises(RuntimeError, match="bg_color"):
        mesh.render(*view, bg_color=(-0.1, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="surf_color"):
        mesh.overlay(np.zeros((48, 64, 3), np.uint8), K_CAM, Rs, ts, surf_colors=[[0.0, 0.0, 2.0]])
    with pytest.raises(RuntimeError):
        mesh.overlay(np.zeros((48, 64, 3), np.uint8), K_CAM, Rs, ts, mode="xray")
    with pytest.raises(RuntimeError):
        with_uv.set_texture(np.full((4, 4, 3), 1.5, np.float32))
    # the C entry point validates what the wrapper would not let through
    lib = lm.load_library()
    n, Ks, Rf, tf = lm.Mesh._views(K_CAM, Rs, ts)
    out = np.zeros((1, 48, 64, 3), np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                         # noqa: E731
    for field, value, word in (("shading", 7, "shading"), ("size", 8, "size")):
        opts = lm.render_options()
        setattr(opts, field, value)
        assert lib.lm_mesh_render_ex(mesh._h, n, 64, 48, ptr(Ks), ptr(Rf), ptr(tf), ctypes.byref(opts), None, ptr(out)) < 0
        assert word in lib.lm_last_error().decode()
    opts = lm.render_options()
    opts.surf_color[1], opts.has_surf_color = 1.5, 1
    assert lib.lm_mesh_render_ex(mesh._h, n, 64, 48, ptr(Ks), ptr(Rf), ptr(tf), ctypes.byref(opts), None, ptr(out)) < 0
    assert "surf_color" in lib.lm_last_error().decode()
    # and a valid call still works afterwards
    assert mesh.render(*view, shading="flat", mode="rgb").any()
