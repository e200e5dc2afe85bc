"""GPU tests of the particle-swarm refiner's directional edge cost (csrc/pso_orient.hip, lm_pso_set_scene_orientations /
lm_pso_set_scene_from_detector / lm_pso_run_oriented) against its numpy statement tests/pso_orient_ref.py: the nine planes as uint16 over
the whole image, the orientation of rendered contours through uniform scenes, (sum, n_c) of hand-placed poses, the whole trajectory bit
for bit, and the device hand-over of the detector's quantised map.  Inputs and the reference's answers: tests/pso_orient_cases.py; what
they have to contain is asserted on the CPU by tests/test_pso_orient_ref.py.

Measured, not asserted: the time of a call; nothing here depends on it."""
import ctypes
import os

import numpy as np
import pytest

import lm_abi
import pso_cases as pc
import pso_edge_cases as ec
import pso_orient_cases as oc
import pso_orient_ref as po
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


@pytest.fixture(scope="module")
def mesh(lm):
    V, F = pc.mesh()
    return lm.Mesh(V, F)


@pytest.fixture(scope="module")
def ctx(lm):
    c = lm.PsoContext(0)
    c.set_scene_orientations(oc.orient_scene(), pc.K, oc.M, oc.P)
    return c


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def assert_equals_reference(ctx, got, ref):
    assert len(got) == len(ref)
    for h, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(ctx.read_debug(h, "sum_n_r"), np.stack([r["sum"], r["n_r"]], -1)), h
        assert np.array_equal(bits(ctx.read_debug(h, "x")), bits(r["x"])), h
        assert np.array_equal(bits(ctx.read_debug(h, "cost")), bits(r["cost"])), h
        assert np.array_equal(ctx.read_debug(h, "best"), r["best"]), h
        assert np.array_equal(bits(g["R"]), bits(r["R"])) and np.array_equal(bits(g["t"]), bits(r["t"])), h
        assert bits(g["cost"]) == bits(r["final_cost"]) and bits(g["initial_cost"]) == bits(r["initial_cost"]), h
        assert (g["n_rendered"], g["n_initial"], g["best_particle"], g["best_generation"]) == \
               (r["n_rendered"], r["n_initial"], r["best_particle"], r["best_generation"]), h


def planes(c):
    return np.stack([c.orient_distance(k) for k in range(9)])


def run(ctx, mesh, **options):
    Rs, ts = pc.hypotheses()
    o = dict(ec.OPTIONS); o.update(options)
    return ctx.run(mesh, Rs[:3], ts[:3], pc.WINDOWS[:3], pc.WIN, cost="oriented", **o)[0]


def record(c, got):
    return b"".join(g[k].tobytes() for g in got for k in ("R", "t")) + bits([g["cost"] for g in got]).tobytes() + \
        b"".join(c.read_debug(h, kind).tobytes() for h in range(len(got)) for kind in ("x", "cost", "sum_n_r", "best"))


# ---- the planes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ec.EDT_FRAMES, ids=["%dx%d" % s for s in ec.EDT_FRAMES])
def test_planes_are_the_reference(lm, size):
    """Every map of pso_orient_cases.plane_maps at M = 1, 2, 5, 32 and P = 0, 1, 16, 4096: all nine planes as uint16."""
    W, H = size
    c = lm.PsoContext(0)
    for name, q in oc.plane_maps(W, H).items():
        for M in oc.PLANE_M:
            for P in oc.PLANE_P:
                c.set_scene_orientations(q, pc.K, M, P)
                got = planes(c)
                assert got.dtype == np.uint16 and got.shape == (9, H, W)
                assert np.array_equal(got, po.orient_distance(q, M, P)), (name, M, P)
    c.close()


def test_planes_at_the_largest_cap_and_a_smaller_frame_after_a_larger_one(lm):
    c = lm.PsoContext(0)
    for name, q in oc.plane_maps(300, 40).items():
        c.set_scene_orientations(q, pc.K, 255, 16)
        assert np.array_equal(planes(c), po.orient_distance(q, 255, 16)), name
    big, small = oc.plane_maps(300, 70)["random"], oc.plane_maps(67, 45)["quadrants"]
    c.set_scene_orientations(big, pc.K, 32, 16)
    assert np.array_equal(planes(c), po.orient_distance(big, 32, 16))
    c.set_scene_orientations(small, pc.K, 5, 1)
    assert c.orient_distance(0).shape == (45, 67) and np.array_equal(planes(c), po.orient_distance(small, 5, 1))
    c.close()


# ---- the orientation of the rendered contour ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steps", "sliver", "cut"])
def test_contour_orientations(lm, name):
    """Evaluate-only under Q = 1 << j everywhere, j = 0..7, with P = 1 and tau = M = 32: a contour pixel of bin k adds d(k, j)^2, one
    without orientation 0, so the eight sums and n_c fix the histogram of the bins on the device."""
    V, F, Rs, ts, wins, win, steps = oc.contour_groups()[name]
    m = lm.Mesh(V, F)
    c = lm.PsoContext(0)
    for j in range(8):
        c.set_scene_orientations(np.full((pc.H, pc.W), 1 << j, np.uint8), pc.K, 32, 1)
        for step in steps:
            c.run(m, Rs, ts, wins, win, cost="oriented", generations=0, tau=oc.H_TAU, edge_step_mm=step)
            got = [tuple(c.read_debug(i, "sum_n_r")[0, 0]) for i in range(len(Rs))]
            assert got == oc.contour_reference(name, step, j), (j, step)
    c.close()


# ---- evaluate-only ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_only(lm, mesh):
    """generations = 0: (sum, n_c) and the cost of the 16 hand-placed poses against pose 0's oriented contour; the cover floor."""
    Rs, ts, wins = ec.eval_poses()
    terms, n_0, costs = oc.eval_reference()
    c = lm.PsoContext(0)
    c.set_scene_orientations(oc.eval_orientations(), pc.K, oc.M, oc.P)
    for cover in (0, n_0):
        got, _ = c.run(mesh, Rs, ts, wins, pc.WIN, cost="oriented", particles=8, generations=0, tau=oc.TAU, cover_pixels=cover)
        for i in range(16):
            assert tuple(c.read_debug(i, "sum_n_r")[0, 0]) == terms[i], (cover, i)
            want = costs[i] if cover else po.cost(terms[i][0], terms[i][1], terms[i][1])
            assert bits(got[i]["cost"]) == bits(want) == bits(got[i]["initial_cost"]) == bits(c.read_debug(i, "cost")[0, 0]), (cover, i)
            assert got[i]["n_rendered"] == terms[i][1] and got[i]["n_initial"] == (cover or terms[i][1])
    c.close()


# ---- the swarm ----------------------------------------------------------------------------------------------------------------------------
def test_trajectory_is_bit_exact_and_repeats(ctx, mesh):
    got = run(ctx, mesh)
    assert_equals_reference(ctx, got, oc.reference())
    first = record(ctx, got)
    assert record(ctx, run(ctx, mesh)) == first


def test_without_a_penalty_the_run_is_the_edge_cost_run(lm, mesh):
    Rs, ts = pc.hypotheses()
    c = lm.PsoContext(0)
    c.set_scene_orientations(oc.orient_scene(), pc.K, oc.M, 0)
    c.set_scene_edges(oc.orient_scene() != 0, pc.K, oc.M)
    args = (mesh, Rs[:3], ts[:3], pc.WINDOWS[:3], pc.WIN)
    oriented = record(c, c.run(*args, cost="oriented", **ec.OPTIONS)[0])
    assert oriented == record(c, c.run(*args, cost="edges", **ec.OPTIONS)[0])
    assert all(np.array_equal(c.orient_distance(k), c.edge_distance()) for k in range(9))
    c.close()


def test_the_helping_scene_is_bit_exact(lm, mesh):
    """oc.HELPS on oc.helps_scene(), through pso_refine_oriented: the numpy statement's own result (what it is worth is asserted of the
    two references on the CPU, tests/test_pso_orient_ref.py; nothing about quality here)."""
    Rs, _ = pc.hypotheses()
    got, ms = lm.pso_refine_oriented(mesh, oc.helps_scene(), pc.K, Rs[:1], ec.REFINE_T0[None], pc.WINDOWS[:1], pc.WIN, max_dist=oc.M,
                                     orient_penalty=oc.P, **oc.HELPS)
    want = oc.helps_references()[0]
    assert ms > 0.0 and np.array_equal(bits(got[0]["t"]), bits(want["t"])) and np.array_equal(bits(got[0]["R"]), bits(want["R"]))
    assert bits(got[0]["cost"]) == bits(want["final_cost"]) and got[0]["n_rendered"] == want["n_rendered"]


# ---- the hand-over ------------------------------------------------------------------------------------------------------------------------
def colour_detector(lm):
    det = lm.Detector(64, [4, 8], device=0, modalities=("ColorGradient",))
    det.addClassPacked("e", np.zeros((0, 3), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
    return det


def test_scene_from_detector_on_the_device(lm, mesh):
    """A colour-only detector after one match on a 160 x 160 frame: the planes and a run equal those of the map read back and set
    through the host, at both pyramid levels."""
    W, H = oc.HAND_SIZE
    rgb, _ = synth.make_frame(5, W, H, 6)
    det = colour_detector(lm)
    det.setFrame([rgb])
    det.matchResident(75.0, ["e"])
    Rs, ts = pc.hypotheses()
    args = (mesh, Rs[:2], ts[:2], pc.WINDOWS[:2], pc.WIN)
    a, b = lm.PsoContext(0), lm.PsoContext(0)
    for level in (0, 1):
        w, h = W >> level, H >> level
        q = det.readStage(level, 0).reshape(h, w)
        assert np.count_nonzero(q) > 50 and len(np.unique(q)) >= 6
        a.set_scene_from_detector(det, oc.HAND_K, (W, H), level=level, max_dist=12, directional=True, orient_penalty=9)
        b.set_scene_orientations(q, oc.HAND_K, 12, 9)
        assert a.orient_distance(0).shape == (h, w)
        assert np.array_equal(planes(a), planes(b)) and np.array_equal(planes(a), po.orient_distance(q, 12, 9)), level
        assert record(a, a.run(*args, cost="oriented", **ec.OPTIONS)[0]) == record(b, b.run(*args, cost="oriented", **ec.OPTIONS)[0]), level
    before = planes(a)
    with pytest.raises(RuntimeError, match="the detector's stage has"):              # a wrong size is refused before the scene is replaced
        a.set_scene_from_detector(det, oc.HAND_K, (W * 2, H), directional=True)
    assert np.array_equal(planes(a), before)
    a.close(); b.close()


def test_scene_from_detector_refusals(lm):
    W, H = oc.HAND_SIZE
    rgb, _ = synth.make_frame(5, W, H, 6)
    c = lm.PsoContext(0)
    det = colour_detector(lm)
    with pytest.raises(RuntimeError, match="no front end has run"):                  # nothing uploaded yet
        c.set_scene_from_detector(det, oc.HAND_K, (W, H), directional=True)
    det.setFrame([rgb])
    with pytest.raises(RuntimeError, match="no front end has run"):                  # a frame, but nothing quantised
        c.set_scene_from_detector(det, oc.HAND_K, (W, H), directional=True)
    det.submit(75.0, ["e"])
    with pytest.raises(RuntimeError, match="frames in flight"):
        c.set_scene_from_detector(det, oc.HAND_K, (W, H), directional=True)
    det.collect()
    c.set_scene_from_detector(det, oc.HAND_K, (W, H), directional=True)              # collected: accepted
    depth_only = lm.Detector(64, [4, 8], device=0, modalities=("DepthNormal",))
    with pytest.raises(RuntimeError, match="no ColorGradient"):
        c.set_scene_from_detector(depth_only, oc.HAND_K, (W, H), directional=True)
    if lm.load_library().lm_device_count() >= 2:                                     # another device exists only on a machine with two
        other = lm.PsoContext(1)
        with pytest.raises(RuntimeError, match="the detector lives on device 0, the context on 1"):
            other.set_scene_from_detector(det, oc.HAND_K, (W, H), directional=True)
        other.close()
    for kw, text in ((dict(level=2), "level 2 out of range"), (dict(max_dist=0), "max_dist must be in 1..255"),
                     (dict(orient_penalty=4097), "orient_penalty must be in 0..4096")):
        with pytest.raises(RuntimeError, match=text):
            c.set_scene_from_detector(det, oc.HAND_K, (W, H), directional=True, **kw)
    c.close()


# ---- neighbours undisturbed -----------------------------------------------------------------------------------------------------------------
def test_depth_and_edges_are_undisturbed_by_an_oriented_scene(lm, mesh):
    Rs, ts = pc.hypotheses()
    args = (mesh, Rs, ts, pc.WINDOWS, pc.WIN)
    plain, both = lm.PsoContext(0), lm.PsoContext(0)
    for c in (plain, both):
        c.set_scene(pc.scene(), pc.K)
        c.set_scene_edges(ec.edge_scene(), pc.K, ec.M)
    both.set_scene_orientations(oc.orient_scene()[:72, :90], pc.K, 16, 7)             # another frame size, cap and penalty
    o0 = record(both, both.run(*args, cost="oriented", **ec.OPTIONS)[0])
    for cost, options in (("depth", pc.OPTIONS), ("edges", ec.OPTIONS)):
        assert record(both, both.run(*args, cost=cost, **options)[0]) == record(plain, plain.run(*args, cost=cost, **options)[0]), cost
    both.set_scene_edges(ec.edge_scene()[:40], pc.K, 8)                              # a new edge scene does not disturb the oriented one
    assert record(both, both.run(*args, cost="oriented", **ec.OPTIONS)[0]) == o0
    assert np.array_equal(planes(both), po.orient_distance(oc.orient_scene()[:72, :90], 16, 7))
    plain.close(); both.close()


def test_refusals(lm, mesh):
    Rs, ts = pc.hypotheses()
    c = lm.PsoContext(0)
    args = (mesh, Rs, ts, pc.WINDOWS, pc.WIN)
    c.set_scene_edges(ec.edge_scene(), pc.K, ec.M)                                   # an edge scene is no oriented scene
    for a in (args, (mesh, Rs, ts)):
        with pytest.raises(RuntimeError, match="no scene orientations set"):
            c.run(*a, cost="oriented", **ec.OPTIONS)
    with pytest.raises(RuntimeError, match="no scene orientations set"):
        c.orient_distance(0)
    q = oc.orient_scene()
    for M in (0, 256):
        with pytest.raises(RuntimeError, match="max_dist must be in 1..255"):
            c.set_scene_orientations(q, pc.K, M)
    for P in (-1, 4097):
        with pytest.raises(RuntimeError, match="orient_penalty must be in 0..4096"):
            c.set_scene_orientations(q, pc.K, 32, P)
    with pytest.raises(RuntimeError, match="orient_penalty must be an integer"):
        c.set_scene_orientations(q, pc.K, 32, 1.5)
    for bad in (q.astype(bool), q.astype(np.uint16), q.ravel(), np.zeros((0, 4), np.uint8)):
        with pytest.raises(RuntimeError, match="uint8 HxW orientation map"):
            c.set_scene_orientations(bad, pc.K)
    c.set_scene_orientations(q, pc.K, 8, 4096)
    for plane in (-1, 9):
        with pytest.raises(RuntimeError, match="plane must be in 0..8"):
            c.orient_distance(plane)
    with pytest.raises(RuntimeError, match="tau must be <= max_dist"):
        c.run(*args, cost="oriented", **dict(ec.OPTIONS, tau=9))
    with pytest.raises(RuntimeError, match="edge_step_mm must be"):
        c.run(*args, cost="oriented", edge_step_mm=65536, **dict(ec.OPTIONS, tau=8))
    with pytest.raises(RuntimeError, match="cost must be 'depth' or 'edges' or 'oriented'"):
        c.run(*args, cost="colour", **ec.OPTIONS)
    lib = lm.load_library()                                                          # the C ABI refuses what the Python layer stops earlier
    res, ms = (lm_abi._CPsoResult * 4)(), ctypes.c_float()
    xy = np.ascontiguousarray(pc.WINDOWS, np.int32)
    R9, t3 = np.ascontiguousarray(Rs.reshape(-1, 9)), np.ascontiguousarray(ts)
    rc = lib.lm_pso_run_oriented(c._h, mesh._h, 4, R9.ctypes.data, t3.ctypes.data, xy.ctypes.data, pc.WIN[0], pc.WIN[1], None, -1, res, ctypes.byref(ms))
    assert rc != 0 and b"edge_step_mm must be in 0..65535" in lib.lm_last_error()
    c.run(*args, cost="oriented", **dict(ec.OPTIONS, tau=8))                         # and the context still works
    c.close()
