"""GPU: the rasteriser's kernels (k_project, k_raster, k_resolve_depth, k_resolve_rgb) at the edges that random views do not
reach — edges through pixel centres, equal depths, vertices at and behind the camera plane, the 1e9 guard, NaN poses,
clip planes inside triangles, uint16 saturation, supersampled borders, a second chunk of views, more views than a
grid's y holds — against the references of tests/render_edges_ref.py, which do not restate the kernel (closed-form
coverage, exact ownership, a float64 ray caster), and bit for bit against oracle/render_oracle.py.
tests/test_render_edges_ref.py checks on the CPU that the oracle itself meets every condition used here."""
import functools
import os

import numpy as np
import pytest

import render_edges_ref as er
import render_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def _clip(c):
    return c.get("clip", (10.0, 10000.0))


def _gpu_depth(lm, c, colors=None):
    near, far = _clip(c)
    return lm.Mesh(c["V"], c["F"], colors=colors).render((c["W"], c["H"]), c["K"], c["R"][None], c["t"][None], clip_near=near, clip_far=far, mode="depth")[0]


def _gpu_owner(lm, c):
    """(owner map decoded from the face-id colours, depth) of an unshared mesh."""
    near, far = _clip(c)
    mesh = lm.Mesh(c["V"], c["F"], colors=er.face_id_colours(len(c["F"])))
    rgb, depth = mesh.render((c["W"], c["H"]), c["K"], c["R"][None], c["t"][None], clip_near=near, clip_far=far, ambient_weight=1.0, ssaa=1)
    return er.decode_owner(rgb[0]), depth[0]


def _oracle(c):
    return ro.render_depth(c["V"], c["F"], c["K"], c["R"], c["t"], c["W"], c["H"], *_clip(c))


@functools.lru_cache(None)
def _ray_case(i):
    c = er.ray_cases()[i]
    return c, er.raycast_depth(c["V"], c["F"], c["K"], c["R"], c["t"], c["W"], c["H"])


@pytest.mark.parametrize("k", range(len(er.LATTICES)))
def test_edges_through_pixel_centres(lm, k):
    """Case 1: covered exactly the half-open rectangle, depth z inside, for every draw of diagonals, windings and face order."""
    for seed in er.LATTICE_SEEDS:
        c = er.lattice_case(k, seed)
        d = _gpu_depth(lm, c)
        assert er.check_lattice_coverage(d, c) is None, (seed, er.check_lattice_coverage(d, c))
        assert np.array_equal(d, _oracle(c)[0])


@pytest.mark.parametrize("k", range(len(er.LATTICES)))
def test_every_pixel_has_one_owner(lm, k):
    """Case 2: the owner the colour image names is the oracle's, contains the pixel centre (exact integers, no fill rule), and
    every face with a pixel centre strictly inside owns one: both triangles of every quad inside the frame."""
    for seed in er.LATTICE_SEEDS:
        c = er.lattice_case(k, seed, unshared=True)
        owner, d = _gpu_owner(lm, c)
        assert er.check_lattice_coverage(d, c) is None
        assert np.array_equal(owner, _oracle(c)[1]), seed
        must = er.check_owners(owner, c)
        if k != 2:
            assert must.all()


def test_depth_ties(lm):
    """Case 3: coincident fragments go to the lower face index, an interpenetrating pair shows the nearer sheet; three renders
    are identical (the order of the atomics does not show)."""
    for c in (er.tie_case(), er.crossing_case()):
        want_d, want_tri = _oracle(c)
        runs = [_gpu_owner(lm, c) for _ in range(3)]
        for owner, d in runs:
            assert np.array_equal(owner, want_tri) and np.array_equal(d, want_d)
        if "twin" in c:
            own = runs[0][0][runs[0][0] >= 0]
            assert len(own) > 500 and (own < c["twin"][own]).all()
        else:
            assert er.check_against_rays(runs[0][1], er.raycast_depth(c["V"], c["F"], c["K"], c["R"], c["t"], c["W"], c["H"])) <= 1


@pytest.mark.parametrize("i", range(4))
def test_depth_agrees_with_the_ray_caster(lm, i):
    """Case 4: coverage equals the rays' hits with no exception and |d - floor(z_ray)| <= 1 on every covered pixel.  The oracle's
    float depth is within 0.126 mm (sphere), 0.061 mm (sphere cut by the right edge), 0.022 and 0.056 mm (the two close
    cubes) of the rays and covers the same pixels; after truncation that is one step of the uint16."""
    c, zr = _ray_case(i)
    d = _gpu_depth(lm, c)
    assert (d > 0).sum() > 800
    err = er.check_against_rays(d, zr)
    print("case 4 %s: max |d - floor(z_ray)| = %d over %d pixels" % (c["name"], err, (d > 0).sum()))
    assert np.array_equal(d, _oracle(c)[0])


def test_vertices_at_and_behind_the_camera_plane(lm):
    """Case 5: a triangle with one, two or three vertices at p_z <= 0 (one at exactly 0) is absent; the rest is the oracle's, and
    what a ray caster sees of the faces wholly in front."""
    c = er.behind_case()
    Vu, Fu = er.unshare(c["V"], c["F"])
    owner, d = _gpu_owner(lm, dict(c, V=Vu, F=Fu))
    want_d, want_tri = _oracle(c)
    assert (d > 0).sum() > 300
    assert np.array_equal(d, want_d) and np.array_equal(owner, want_tri)
    assert c["front"][np.unique(owner[owner >= 0])].all()
    assert np.array_equal(_gpu_depth(lm, c), want_d)                   # shared vertices: the same image
    assert er.check_against_rays(d, er.raycast_depth(c["V"], c["F"][c["front"]], c["K"], c["R"], c["t"], c["W"], c["H"])) <= 1


def test_the_1e9_guard(lm):
    """Case 6: a vertex whose snapped coordinate reaches 1e9 in magnitude is invalid and its triangle is not drawn; at half the
    guard the triangle is drawn (int64 edge functions, bounding box clipped to the frame) and equals the oracle."""
    beyond, half = er.guard_cases()
    assert not _gpu_depth(lm, beyond).any() and not _oracle(beyond)[0].any()
    d = _gpu_depth(lm, half)
    assert (d > 0).sum() > 500 and np.array_equal(d, _oracle(half)[0])
    zr = er.raycast_depth(half["V"], half["F"], half["K"], half["R"], half["t"], half["W"], half["H"])
    assert np.array_equal(d > 0, np.isfinite(zr) & (zr >= 10.0))


def test_nan_and_inf_poses_inside_a_batch(lm):
    """Case 7: the views with a NaN rotation or an infinite translation are empty, their neighbours untouched."""
    c, Rs, ts, bad = er.pose_batch()
    depth = lm.Mesh(c["V"], c["F"]).render((c["W"], c["H"]), c["K"], Rs, ts, mode="depth")
    for i in range(len(Rs)):
        if i in bad:
            assert not depth[i].any(), i
        else:
            want = ro.render_depth(c["V"], c["F"], c["K"], Rs[i], ts[i], c["W"], c["H"])[0]
            assert (want > 0).sum() > 300 and np.array_equal(depth[i], want), i


def test_clip_planes_cut_through_triangles(lm):
    """Case 8: equal to the oracle; against the rays, covered iff 300 <= z_ray <= 600 outside 0.13 mm around either plane (the
    bound of case 4); the pixels inside that band are counted and are fewer than 2 % of the covered ones."""
    c = er.clip_case()
    d = _gpu_depth(lm, c)
    assert np.array_equal(d, _oracle(c)[0])
    zr = er.raycast_depth(c["V"], c["F"], c["K"], c["R"], c["t"], c["W"], c["H"])
    excluded, covered = er.check_clip_against_rays(d, zr, *c["clip"])
    print("case 8: %d pixels excluded of %d covered" % (excluded, covered))
    assert np.abs(d[d > 0].astype(np.int64) - np.floor(zr[d > 0]).astype(np.int64)).max() <= 1


def test_uint16_saturation_and_truncation_to_zero(lm):
    """Case 9: depths saturate at 65535.  A sheet at 0.75 mm inside the clip range is covered (the colour image shows it),
    truncates to 0 and so cannot be told from background in the depth image: depth.astype(np.uint16) of the reference driver
    does the same; this is the format, not a bug."""
    size = (er.U16_W, er.U16_H)
    for z, want in er.U16_Z:
        V, F = er.sheet(z)
        d = lm.Mesh(V, F).render(size, er.K_U16, er.EYE[None], er.ZERO[None], clip_far=1e5, mode="depth")[0]
        assert (d == want).all(), (z, np.unique(d))
    V, F = er.sheet(0.75)
    rgb, d = lm.Mesh(V, F).render(size, er.K_U16, er.EYE[None], er.ZERO[None], clip_near=0.5, clip_far=1e5, ambient_weight=1.0, ssaa=1)
    assert not d.any() and (rgb[0] > 0).all()


@pytest.mark.parametrize("ssaa", er.SSAA_FACTORS)
def test_supersampled_rectangle_is_the_integer_box_average(lm, ssaa):
    """Case 10: every pixel is floor((2 k c + n) / (2 n)) with k of n = ssaa^2 samples inside the half-open rectangle scaled by
    ssaa, k counted in integers."""
    x0, y0, step, _ = er.LATTICES[1]
    c = er.lattice_case(1, 0, unshared=True)
    C = np.tile(np.array(er.SSAA_COLOUR, np.uint8), (len(c["V"]), 1))
    want, k = er.ssaa_expected(x0, y0, er.LATTICE_NX, er.LATTICE_NY, step, c["W"], c["H"], ssaa)
    got = lm.Mesh(c["V"], c["F"], colors=C).render((c["W"], c["H"]), c["K"], c["R"][None], c["t"][None], ambient_weight=1.0, ssaa=ssaa, mode="rgb")[0]
    assert np.array_equal(got, want)
    ref = ro.render_rgb(c["V"], None, C.astype(np.float64), c["F"], c["K"], c["R"], c["t"], c["W"], c["H"], ambient=1.0, ssaa=ssaa)
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 2


def test_second_chunk_of_views(lm):
    """Case 11: 320 x 240 at ssaa 8 is 39 MB of id buffer per view, so lm_mesh_render cuts 55 views after the 54th (2 GB).  The last
    view of the first chunk and the first (= last) of the second equal the same view rendered alone, byte for byte."""
    from synth import icosphere
    V, F, N, C = icosphere(0)
    n = 55
    assert (2 << 30) // (320 * 240 * 64 * 8) == n - 1
    K = np.array([[286.2057, 0, 162.63], [0, 286.78522, 121.02], [0, 0, 1]], np.float32)
    Rs = np.stack([er.rot("y", 0.11 * i) @ er.rot("x", 0.07 * i) for i in range(n)]).astype(np.float32)
    ts = np.stack([[30.0 * np.sin(i), 20.0 * np.cos(i), 2000.0 + 10 * i] for i in range(n)]).astype(np.float32)
    mesh = lm.Mesh(V, F, normals=N, colors=C)
    rgb = mesh.render((320, 240), K, Rs, ts, ssaa=8, mode="rgb")
    for i in (0, n - 2, n - 1):
        alone = mesh.render((320, 240), K, Rs[i:i + 1], ts[i:i + 1], ssaa=8, mode="rgb")[0]
        assert alone.any() and np.array_equal(rgb[i], alone), i
    want = ro.render_rgb(V.astype(np.float64), N.astype(np.float64), C.astype(np.float64), F, K, Rs[n - 1], ts[n - 1], 320, 240, ssaa=8)
    assert (want.sum(2) > 0).sum() > 100 and np.abs(rgb[n - 1].astype(int) - want.astype(int)).max() <= 2


def test_more_views_than_a_grid_is_high(lm):
    """Case 12: 65 537 views of 8 x 6 pixels.  The view is the y of the grids of k_project, k_raster and k_resolve_depth; the call
    returns LM_OK (Mesh.render raises otherwise) and the views at both ends, where a chunk boundary or a wrapped index would
    show, equal the oracle."""
    K = np.array([[256, 0, 4], [0, 256, 3], [0, 0, 1]], np.float32)
    V, F, _ = er.lattice(1, 1, 2, 1, 3, 256, np.random.default_rng(3), K)
    n = 65537
    Rs = np.tile(er.EYE, (n, 1, 1))
    ts = np.zeros((n, 3), np.float32)
    ts[0], ts[n - 2], ts[n - 1] = (1, 0, 0), (0, 1, 0), (2, 1, 0)
    depth = lm.Mesh(V, F).render((8, 6), K, Rs, ts, mode="depth")
    images = {}
    for i in (0, 1, n - 2, n - 1):
        want = ro.render_depth(V, F, K, Rs[i], ts[i], 8, 6)[0]
        assert (want > 0).sum() >= 12 and np.array_equal(depth[i], want), i
        images[i] = want.tobytes()
    assert len(set(images.values())) == 4
    assert (depth[1:n - 2] == depth[1]).all()
