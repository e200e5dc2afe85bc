"""CPU: the numpy restatement of the rasteriser (oracle/render_oracle.py) against references that do not restate it
(tests/render_edges_ref.py): closed-form coverage of lattices whose edges run through pixel centres, exact ownership, a
float64 ray caster.  tests/test_gpu_render_edges.py holds the kernels to the same conditions, and to the oracle bit for
bit; what the oracle meets here, a failure there is a finding about the kernel.  Two mutants of the fill rule show that
the coverage property sees what it is meant to see.  No GPU, no library load."""
import numpy as np
import pytest

import render_edges_ref as er
import render_oracle as ro


def _depth(c, **kw):
    near, far = c.get("clip", (10.0, 10000.0))
    return ro.render_depth(c["V"], c["F"], c["K"], kw.get("R", c["R"]), kw.get("t", c["t"]), c["W"], c["H"], near, far)


def _rays(c, F=None):
    return er.raycast_depth(c["V"], c["F"] if F is None else F, c["K"], c["R"], c["t"], c["W"], c["H"])


LATTICE_RUNS = [(k, s) for k in range(len(er.LATTICES)) for s in er.LATTICE_SEEDS]


@pytest.mark.parametrize("k,seed", LATTICE_RUNS)
def test_lattice_coverage_is_the_half_open_rectangle(k, seed):
    """Case 1: every edge of these sheets passes through pixel centres; any slip of the fill rule or the bounding box leaves a
    hole, a double row or a shifted border."""
    c = er.lattice_case(k, seed)
    assert c["rect"].sum() >= 360
    assert er.check_lattice_coverage(_depth(c)[0], c) is None


@pytest.mark.parametrize("mutant,what", [(lambda ex, ey: False, "holes"), (lambda ex, ey: (ey == 0 and ex < 0) or ey > 0, "extra")])
def test_fill_rule_mutants_fail_the_coverage_property(monkeypatch, mutant, what):
    """"No edge is inside" leaves holes along every edge through pixel centres; the mirrored (bottom-right) rule shifts the
    rectangle by one row and one column.  Case 1 must see both, on every lattice that has edges on pixel centres."""
    monkeypatch.setattr(ro, "_top_left", mutant)
    for k, seed in LATTICE_RUNS:
        c = er.lattice_case(k, seed)
        cov = _depth(c)[0] > 0
        msg = er.check_lattice_coverage(cov * c["z"], c)
        if what == "holes":                                            # every lattice has edges (the diagonals at least) on pixel centres
            assert msg is not None and (c["rect"] & ~cov).any() and not (cov & ~c["rect"]).any()
        elif k in (0, 2):                                              # integer corners: the border itself lies on pixel centres
            assert msg is not None and (cov & ~c["rect"]).any()
            assert (c["rect"] & ~cov).any() == (k == 0)                # lattice 2: the rows and columns that would be lost are outside the frame
        else:                                                          # borders between pixel centres: a mirrored rule covers the same pixels
            assert msg is None


@pytest.mark.parametrize("k,seed", LATTICE_RUNS)
def test_every_pixel_has_one_owner_that_contains_it(k, seed):
    """Case 2: the oracle's owner map on the unshared lattices; containment in exact integers, written without the fill rule."""
    c = er.lattice_case(k, seed, unshared=True)
    d, tri = _depth(c)
    assert er.check_lattice_coverage(d, c) is None
    must = er.check_owners(tri, c)
    if k != 2:                                                         # lattice 2 leaves the frame; the others: both triangles of every quad
        assert must.all() and len(np.unique(c["quad"])) == er.LATTICE_NX * er.LATTICE_NY


@pytest.mark.parametrize("k", range(len(er.LATTICES)))
def test_face_id_colours_name_the_owner(k):
    c = er.lattice_case(k, 0, unshared=True)
    C = er.face_id_colours(len(c["F"]))
    rgb = ro.render_rgb(c["V"], None, C.astype(np.float64), c["F"], c["K"], c["R"], c["t"], c["W"], c["H"], ambient=1.0, ssaa=1)
    assert np.array_equal(er.decode_owner(rgb), _depth(c)[1])
    assert np.array_equal(er.decode_owner(er.face_id_colours(70000)[::3]), np.arange(70000))


def test_depth_ties_go_to_the_lower_face():
    """Case 3."""
    c = er.tie_case()
    d, tri = _depth(c)
    own = tri[tri >= 0]
    assert len(own) > 500 and (own < c["twin"][own]).all()             # of two coincident faces the lower index shows
    assert (np.bincount(own, minlength=len(c["F"])) > 0).sum() >= len(c["F"]) // 2 - 2
    assert er.check_against_rays(d, _rays(c)) <= 1
    x = er.crossing_case()
    d, tri = _depth(x)
    zr = _rays(x)
    assert er.check_against_rays(d, zr) <= 1                           # the nearer sheet shows on either side of the crossing
    z, _ = ro.rasterise(x["V"], x["F"], x["K"], x["R"], x["t"], x["W"], x["H"], 10.0, 10000.0)
    assert np.abs(z[tri >= 0] - zr[tri >= 0]).max() <= er.RAY_BOUND_MM
    assert (zr[:, 4:12] < 255).any() and (zr[:, 20:28] < 255).any()   # nearer than the crossing (z = 256) on both sides: each sheet shows on one


@pytest.mark.parametrize("i", range(4))
def test_depth_agrees_with_the_ray_caster(i):
    """Case 4.  Largest |z_oracle - z_ray| (float): 0.126, 0.061, 0.022, 0.056 mm; coverage differs at no pixel."""
    c = er.ray_cases()[i]
    d, tri = _depth(c)
    zr = _rays(c)
    assert (d > 0).sum() > 800
    if i == 1:
        assert (d > 0)[:, -1].sum() > 50                               # cut by the right edge of the frame
    if i >= 2:
        assert (d > 0)[0].any() or (d > 0)[-1].any() or (d > 0)[:, 0].any() or (d > 0)[:, -1].any()
    assert er.check_against_rays(d, zr) <= 1
    z, _ = ro.rasterise(c["V"], c["F"], c["K"], c["R"], c["t"], c["W"], c["H"], *c["clip"])
    assert np.abs(z[tri >= 0] - zr[tri >= 0]).max() <= er.RAY_BOUND_MM


def test_triangles_with_a_vertex_at_or_behind_the_camera_plane_are_absent():
    """Case 5."""
    c = er.behind_case()
    d, tri = _depth(c)
    assert (d > 0).sum() > 300
    assert c["front"][np.unique(tri[tri >= 0])].all()
    assert er.check_against_rays(d, _rays(c, c["F"][c["front"]])) <= 1   # exactly what the faces wholly in front show
    assert np.isfinite(_rays(c)).sum() > (d > 0).sum() + 100             # the rays do see the dropped triangles' front parts


def test_the_1e9_guard():
    """Case 6."""
    beyond, half = er.guard_cases()
    assert not (_depth(beyond)[0] > 0).any()
    d, _ = _depth(half)
    assert (d > 0).sum() > 500
    zr = _rays(half)
    assert np.array_equal(d > 0, np.isfinite(zr) & (zr >= 10.0))
    assert np.abs(d[d > 0].astype(np.int64) - np.floor(zr[d > 0]).astype(np.int64)).max() <= 1


def test_nan_and_inf_poses_render_nothing():
    """Case 7."""
    c, Rs, ts, bad = er.pose_batch()
    with np.errstate(all="ignore"):
        for i in range(len(Rs)):
            d, _ = _depth(c, R=Rs[i], t=ts[i])
            assert ((d > 0).sum() == 0) == (i in bad), i


def test_clip_planes_cut_through_triangles():
    """Case 8.  14 of 2281 covered pixels lie within 0.13 mm of a plane and are left out."""
    c = er.clip_case()
    d, _ = _depth(c)
    zr = _rays(c)
    assert np.isfinite(zr).all() and zr.min() < 200 and zr.max() > 600
    excluded, covered = er.check_clip_against_rays(d, zr, *c["clip"])
    assert np.abs(d[d > 0].astype(np.int64) - np.floor(zr[d > 0]).astype(np.int64)).max() <= 1


def test_uint16_saturation_and_truncation_to_zero():
    """Case 9.  A sheet at 0.75 mm inside the clip range is covered, truncates to 0 and so cannot be told from background in the
    depth image: depth.astype(np.uint16) of the reference driver does the same; this is the format, not a bug."""
    for z, want in er.U16_Z:
        V, F = er.sheet(z)
        d, tri = ro.render_depth(V, F, er.K_U16, er.EYE, er.ZERO, er.U16_W, er.U16_H, 10.0, 1e5)
        assert (tri >= 0).all() and (d == want).all(), (z, np.unique(d))
    V, F = er.sheet(0.75)
    d, tri = ro.render_depth(V, F, er.K_U16, er.EYE, er.ZERO, er.U16_W, er.U16_H, 0.5, 1e5)
    assert (tri >= 0).all() and (d == 0).all()


@pytest.mark.parametrize("ssaa", er.SSAA_FACTORS)
def test_supersampled_rectangle_is_the_integer_box_average(ssaa):
    """Case 10."""
    x0, y0, step, _ = er.LATTICES[1]
    c = er.lattice_case(1, 0, unshared=True)
    C = np.tile(np.array(er.SSAA_COLOUR, np.float64), (len(c["V"]), 1))
    want, k = er.ssaa_expected(x0, y0, er.LATTICE_NX, er.LATTICE_NY, step, c["W"], c["H"], ssaa)
    if ssaa > 1:
        assert ((k > 0) & (k < ssaa * ssaa)).any()                     # partly covered pixels exist
    got = ro.render_rgb(c["V"], None, C, c["F"], c["K"], c["R"], c["t"], c["W"], c["H"], ambient=1.0, ssaa=ssaa)
    assert np.array_equal(got, want)
