"""GPU tests of the particle-swarm refiner's edge cost (csrc/pso_edges.hip, lm_pso_set_scene_edges / lm_pso_run_edges) against its numpy
statement tests/pso_edges_ref.py: the distance transform as uint16 over the whole image, (sum, n_c) of hand-placed poses, and the whole
trajectory bit for bit.  Inputs and the reference's answers: tests/pso_edge_cases.py; what they have to contain is asserted on the CPU
by tests/test_pso_edges_ref.py.

Measured, not asserted: the time of a call; nothing here depends on it."""
import ctypes
import os

import numpy as np
import pytest

import lm_abi
import pso_cases as pc
import pso_edge_cases as ec
import pso_edges_ref as pe
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
    c.set_scene_edges(ec.edge_scene(), pc.K, ec.M)
    return c


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def run(ctx, mesh, window_size=pc.WIN, **options):
    Rs, ts = pc.hypotheses()
    o = dict(ec.OPTIONS); o.update(options)
    return ctx.run(mesh, Rs, ts, pc.WINDOWS, window_size, cost="edges", **o)[0]


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


# ---- the distance transform -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ec.EDT_FRAMES, ids=["%dx%d" % s for s in ec.EDT_FRAMES])
def test_edge_distance_is_the_reference(lm, size):
    """Every map of pso_edge_cases.edt_maps at M = 1, 2, 5, 32: the whole image as uint16.  300 x 70 has rows longer than a workgroup's
    run of 256 columns, more rows than a tile's 32 and sizes that are multiples of nothing; its random map crosses every tile and halo."""
    W, H = size
    c = lm.PsoContext(0)
    for name, e in ec.edt_maps(W, H).items():
        for M in ec.EDT_M:
            c.set_scene_edges(e, pc.K, M)
            got = c.edge_distance()
            assert got.dtype == np.uint16 and got.shape == (H, W)
            assert np.array_equal(got, pe.distance(e, M)), (name, M)
    c.close()


def test_edge_distance_at_the_largest_cap_and_on_the_diagonal(lm):
    """M = 255 on 300 x 40, a frame smaller than the cap in one direction; the (3, 4) diagonal at distance M + 1, M, M - 1; bool maps."""
    c = lm.PsoContext(0)
    for name, e in ec.edt_maps(300, 40).items():
        c.set_scene_edges(e, pc.K, 255)
        assert np.array_equal(c.edge_distance(), pe.distance(e, 255)), name
    e = ec.diagonal_map()
    for M in ec.DIAGONAL_M:
        c.set_scene_edges(e != 0, pc.K, M)
        assert np.array_equal(c.edge_distance(), pe.distance(e, M)), M
    c.close()


def test_a_smaller_frame_after_a_larger_one(lm):
    c = lm.PsoContext(0)
    big, small = ec.edt_maps(300, 70)["random"], ec.edt_maps(67, 45)["corners"]
    c.set_scene_edges(big, pc.K, 32)
    assert np.array_equal(c.edge_distance(), pe.distance(big, 32))
    c.set_scene_edges(small, pc.K, 5)
    assert c.edge_distance().shape == (45, 67) and np.array_equal(c.edge_distance(), pe.distance(small, 5))
    c.close()


# ---- evaluate-only ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_only(lm, mesh):
    """generations = 0: (sum, n_c) and the cost of the 16 hand-placed poses; the cover floor against pose 0's contour count."""
    Rs, ts, wins = ec.eval_poses()
    terms, n_0, costs = ec.eval_reference()
    c = lm.PsoContext(0)
    c.set_scene_edges(ec.eval_edges(), pc.K, ec.M)
    for cover in (0, n_0):
        got, _ = c.run(mesh, Rs, ts, wins, pc.WIN, cost="edges", particles=8, generations=0, tau=ec.TAU, cover_pixels=cover)
        for i in range(16):
            assert tuple(c.read_debug(i, "sum_n_r")[0, 0]) == terms[i], (cover, i)
            want = costs[i] if cover else pe.cost(terms[i][0], terms[i][1], terms[i][1])
            assert bits(got[i]["cost"]) == bits(want) == bits(got[i]["initial_cost"]) == bits(c.read_debug(i, "cost")[0, 0]), (cover, i)
            assert got[i]["n_rendered"] == terms[i][1] and got[i]["n_initial"] == (cover or terms[i][1])
            assert np.array_equal(bits(got[i]["R"]), bits(Rs[i])) and np.array_equal(bits(got[i]["t"]), bits(ts[i]))
    c.close()


def test_depth_jumps_of_the_model(lm):
    """The steps mesh (resolved depths exactly 400, 410, 421) at edge_step_mm 0, 10, 11, 21: a jump counts only when it exceeds the step."""
    V, F = ec.steps_mesh()
    m = lm.Mesh(V, F)
    c = lm.PsoContext(0)
    c.set_scene_edges(ec.edge_scene(), pc.K, ec.M)
    r = ec.steps_render()
    for step in ec.STEPS:
        c.run(m, np.eye(3)[None], ec.STEPS_T[None], [ec.STEPS_WINDOW], ec.STEPS_WIN, cost="edges", generations=0, tau=ec.TAU, edge_step_mm=step)
        want = pe.cost_terms(r, ec.scene_d2(), ec.STEPS_WINDOW[0], ec.STEPS_WINDOW[1], ec.TAU, step)
        assert tuple(c.read_debug(0, "sum_n_r")[0, 0]) == want, step
    c.close()


def test_all_edge_and_empty_scenes(lm, mesh):
    Rs, ts = pc.hypotheses()
    c = lm.PsoContext(0)
    for e, per_pixel in ((np.ones((pc.H, pc.W), np.uint8), 0), (np.zeros((pc.H, pc.W), bool), ec.TAU ** 2)):
        c.set_scene_edges(e, pc.K, ec.M)
        c.run(mesh, Rs[:1], ts[:1], pc.WINDOWS[:1], pc.WIN, cost="edges", generations=0, tau=ec.TAU)
        total, n_c = c.read_debug(0, "sum_n_r")[0, 0]
        assert n_c > 0 and total == n_c * per_pixel
    c.close()


@pytest.mark.parametrize("window_size", [(8, 8), (48, 40), (72, 40), (256, 8), (40, 72)], ids=["8x8", "48x40", "72x40", "256x8", "40x72"])
def test_windows(ctx, mesh, window_size):
    """(sum, n_c) of the four hypotheses in windows of other sizes; 72 x 40 and 256 x 8 take more than one band or more than one pass of
    a band, and 8 x 8 cuts the object on all four sides, where no contour may appear."""
    Rs, ts = pc.hypotheses()
    V, F = pc.mesh()
    ctx.run(mesh, Rs, ts, pc.WINDOWS, window_size, cost="edges", generations=0, tau=ec.TAU)
    for h in range(4):
        x0, y0 = (int(v) for v in pc.WINDOWS[h])
        want = pe.evaluate(V, F, pc.K, ec.scene_d2(), Rs[h], ts[h], x0, y0, window_size[0], window_size[1], ec.TAU)
        assert tuple(ctx.read_debug(h, "sum_n_r")[0, 0]) == want, h


def test_a_window_that_cuts_the_object_adds_no_contour(ctx, mesh):
    """An 8 x 8 window inside object A's image: every pixel rendered, no neighbour inside the window is empty, n_c == 0 and cost +inf."""
    got, _ = ctx.run(mesh, pc.R_A[None], pc.T_A[None], [[22, 18]], (8, 8), cost="edges", generations=0, tau=ec.TAU)
    V, F = pc.mesh()
    assert pe.render_window(V, F, pc.K, pc.R_A, pc.T_A, 22, 18, 8, 8).all()
    assert tuple(ctx.read_debug(0, "sum_n_r")[0, 0]) == (0, 0) and got[0]["cost"] == float("inf") and got[0]["n_rendered"] == 0


# ---- the swarm ----------------------------------------------------------------------------------------------------------------------------
def test_trajectory_is_bit_exact(ctx, mesh):
    got = run(ctx, mesh)
    assert_equals_reference(ctx, got, ec.reference())
    assert ctx.read_debug(0, "x").shape == (pc.G + 1, pc.P, 6)


@pytest.mark.parametrize("options", [dict(particles=1, generations=3), dict(particles=65, generations=2, trans_range_mm=60.0)], ids=["P1", "P65"])
def test_odd_swarms(ctx, mesh, options):
    assert_equals_reference(ctx, run(ctx, mesh, **options), ec.reference(**options))


def test_the_refiner_refines(lm, mesh):
    """ec.REFINE = 16 particles, 6 generations, seed 1, tau 10 px, max_dist 32, from hypothesis (a) displaced by 2 D_T (3.58 px off): for
    these the numpy statement goes to 0.62 px with the cost falling from 5.0 to 0.197 px^2 (tests/test_pso_edges_ref.py asserts it).  The
    device is held to the same inequalities, through pso_refine_edges, the one-call form."""
    Rs, _ = pc.hypotheses()
    got, ms = lm.pso_refine_edges(mesh, ec.edge_scene(), pc.K, Rs[:1], ec.REFINE_T0[None], pc.WINDOWS[:1], pc.WIN, max_dist=ec.M, **ec.REFINE)
    want = ec.centre_px(pc.T_A)
    assert np.linalg.norm(ec.centre_px(ec.REFINE_T0) - want) > 2.0
    assert np.linalg.norm(ec.centre_px(got[0]["t"]) - want) < 1.0
    assert got[0]["cost"] < got[0]["initial_cost"]
    assert ms > 0.0 and np.array_equal(bits(got[0]["t"]), bits(ec.refine_reference()["t"]))


def test_windows_derived_from_the_edge_scene(lm, mesh):
    """windows=None: derive_windows on the edge scene's K, on a context that has no depth scene."""
    Rs, ts = pc.hypotheses()
    c = lm.PsoContext(0)
    c.set_scene_edges(ec.edge_scene(), pc.K, ec.M)
    got, _ = c.run(mesh, Rs[:1], ts[:1], cost="edges", **ec.OPTIONS)
    xy, (w, h) = lm.derive_windows(pc.K, ts[:1], mesh.diameter() / 2.0 + 20.0)
    V, F = pc.mesh()
    want = pe.run(V, F, pc.K, ec.scene_d2(), Rs[:1], ts[:1], xy, w, h, **ec.OPTIONS)[0]
    assert np.array_equal(bits(got[0]["t"]), bits(want["t"])) and bits(got[0]["cost"]) == bits(want["final_cost"])
    c.close()


def test_independent_of_the_depth_scene_and_repeatable(lm, mesh):
    """One context with both scenes, of different sizes: a depth run before and after an edges run returns the same bytes, and the edges
    run the same as on a context without depth; Mesh.render is untouched."""
    Rs, ts = pc.hypotheses()
    before = mesh.render((pc.W, pc.H), pc.K, Rs[:1], ts[:1], mode="depth").tobytes()
    c = lm.PsoContext(0)
    c.set_scene(pc.scene(), pc.K)
    c.set_scene_edges(ec.edge_scene()[:72, :90], pc.K, 16)                           # another frame size and cap than the depth scene's

    def record(got):
        return b"".join(g[k].tobytes() for g in got for k in ("R", "t")) + bits([g["cost"] for g in got]).tobytes() + c.read_debug(1, "x").tobytes()

    def depth_run(**cost):
        return record(c.run(mesh, Rs, ts, pc.WINDOWS, pc.WIN, **cost, **pc.OPTIONS)[0])

    def edges_run():
        return record(c.run(mesh, Rs, ts, pc.WINDOWS, pc.WIN, cost="edges", edge_step_mm=5, **ec.OPTIONS)[0])

    d0 = depth_run(cost="depth")
    assert d0 == depth_run()                                                         # cost="depth" is the path without the keyword
    e0 = edges_run()
    assert depth_run(cost="depth") == d0
    c.set_scene(pc.scene()[:40], pc.K)                                               # a new depth scene does not disturb the edges
    assert edges_run() == e0 and e0 != d0
    d2 = c.edge_distance()
    assert np.array_equal(d2, pe.distance(ec.edge_scene()[:72, :90], 16))
    V, F = pc.mesh()
    want = pe.run(V, F, pc.K, d2, Rs, ts, pc.WINDOWS, *pc.WIN, edge_step_mm=5, **ec.OPTIONS)
    assert np.array_equal(bits(c.read_debug(1, "x")), bits(want[1]["x"]))
    assert mesh.render((pc.W, pc.H), pc.K, Rs[:1], ts[:1], mode="depth").tobytes() == before
    c.close()


def test_refusals(lm, mesh):
    Rs, ts = pc.hypotheses()
    c = lm.PsoContext(0)
    args = (mesh, Rs, ts, pc.WINDOWS, pc.WIN)
    with pytest.raises(RuntimeError, match="no scene edges set"):
        c.run(*args, cost="edges", **ec.OPTIONS)
    with pytest.raises(RuntimeError, match="no scene edges set"):
        c.run(mesh, Rs, ts, cost="edges", **ec.OPTIONS)                              # windows to derive: refused before anything is derived
    with pytest.raises(RuntimeError, match="no scene edges set"):
        c.edge_distance()
    c.set_scene(pc.scene(), pc.K)                                                    # a depth-only context asked for the edge cost
    with pytest.raises(RuntimeError, match="no scene edges set"):
        c.run(*args, cost="edges", **ec.OPTIONS)
    for M in (0, 256):
        with pytest.raises(RuntimeError, match="max_dist must be in 1..255"):
            c.set_scene_edges(ec.edge_scene(), pc.K, M)
    for bad in (ec.edge_scene().astype(np.uint16), ec.edge_scene().astype(np.float32), ec.edge_scene().ravel(), np.zeros((0, 4), np.uint8),
                np.zeros((4, 4, 1), np.uint8)):
        with pytest.raises(RuntimeError, match="uint8 or bool HxW"):
            c.set_scene_edges(bad, pc.K)
    c.set_scene_edges(ec.edge_scene(), pc.K, 8)
    with pytest.raises(RuntimeError, match="tau must be <= max_dist"):
        c.run(*args, cost="edges", **dict(ec.OPTIONS, tau=9))
    with pytest.raises(RuntimeError, match="tau must be in 1..65535"):
        c.run(*args, cost="edges", **dict(ec.OPTIONS, tau=0))
    for step in (-1, 65536, 1.5):
        with pytest.raises(RuntimeError, match="edge_step_mm must be"):
            c.run(*args, cost="edges", edge_step_mm=step, **dict(ec.OPTIONS, tau=8))
    with pytest.raises(RuntimeError, match="cost must be 'depth' or 'edges'"):
        c.run(*args, cost="colour", **ec.OPTIONS)
    with pytest.raises(RuntimeError, match="particles must be in 1..256"):           # lm_pso_run's own checks hold here too
        c.run(*args, cost="edges", **dict(ec.OPTIONS, tau=8, particles=257))
    # the C ABI refuses what the Python layer stops earlier
    lib = lm.load_library()
    res, ms = (lm_abi._CPsoResult * 4)(), ctypes.c_float()
    xy = np.ascontiguousarray(pc.WINDOWS, np.int32)
    R9, t3 = np.ascontiguousarray(Rs.reshape(-1, 9)), np.ascontiguousarray(ts)
    for step in (-1, 65536):
        rc = lib.lm_pso_run_edges(c._h, mesh._h, 4, R9.ctypes.data, t3.ctypes.data, xy.ctypes.data, pc.WIN[0], pc.WIN[1], None, step, res, ctypes.byref(ms))
        assert rc != 0 and b"edge_step_mm must be in 0..65535" in lib.lm_last_error()
    c.run(*args, cost="edges", **dict(ec.OPTIONS, tau=8))                            # and the context still works
    c.close()


def test_scene_from_detector(lm):
    """A colour-only detector after one match on a 96 x 80 frame: the edge scene is its level-0 orientation map != 0."""
    rgb, _ = synth.make_frame(5, pc.W, pc.H, 6)
    det = lm.Detector(64, [4, 8], device=0, modalities=("ColorGradient",))
    det.addClassPacked("e", np.zeros((0, 3), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
    det.setFrame([rgb])
    det.matchResident(75.0, ["e"])
    e = (det.readStage(0, 0) != 0).reshape(pc.H, pc.W)
    assert np.count_nonzero(e) > 50 and not e.all()
    c = lm.PsoContext(0)
    c.set_scene_from_detector(det, pc.K, (pc.W, pc.H), max_dist=12)
    assert np.array_equal(c.edge_distance(), pe.distance(e, 12))
    c.set_scene_from_detector(det, pc.K, (pc.W, pc.H), level=1, max_dist=5)
    e1 = (det.readStage(1, 0) != 0).reshape(pc.H // 2, pc.W // 2)
    assert np.array_equal(c.edge_distance(), pe.distance(e1, 5))
    with pytest.raises(RuntimeError, match="the detector's stage has"):
        c.set_scene_from_detector(det, pc.K, (pc.W * 2, pc.H))
    c.close()
