"""GPU tests of the particle-swarm pose refiner (csrc/pso.hip, lm_pso_*) against its numpy statement tests/pso_ref.py: the whole
trajectory bit for bit.  Inputs and the reference's answers: tests/pso_cases.py; what they have to contain is asserted on the CPU by
tests/test_pso_ref.py.

Measured, not asserted: the time of a call; nothing here depends on it."""
import os

import numpy as np
import pytest

import pso_cases as pc
import pso_ref

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
    c.set_scene(pc.scene(), pc.K)
    return c


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def run(ctx, mesh, window_size=pc.WIN, **options):
    Rs, ts = pc.hypotheses()
    o = dict(pc.OPTIONS); o.update(options)
    return ctx.run(mesh, Rs, ts, pc.WINDOWS, window_size, **o)[0]


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


def test_trajectory_is_bit_exact(ctx, mesh):
    """Every hypothesis and generation: x, (sum, n_r), cost and the best index, and the returned R, t, cost, as uint64."""
    got = run(ctx, mesh)
    assert_equals_reference(ctx, got, pc.reference())
    assert ctx.read_debug(0, "x").shape == (pc.G + 1, pc.P, 6)
    assert np.array_equal(bits(ctx.read_debug(0, "x")), bits(ctx.read_debug(3, "x")))       # (d) is (a): the tie rule across identical swarms
    assert np.array_equal(ctx.read_debug(0, "best"), ctx.read_debug(3, "best"))


def test_evaluate_only(lm, mesh):
    """generations = 0: (sum, n_r) and the cost of 16 hand-placed poses; the cover floor against pose 0's count (cover_pixels)."""
    Rs, ts, wins = pc.eval_poses()
    terms, n_0, costs = pc.eval_reference()
    c = lm.PsoContext(0)
    c.set_scene(pc.eval_scene(), pc.K)
    for cover in (0, n_0):
        got, _ = c.run(mesh, Rs, ts, wins, pc.WIN, particles=8, generations=0, tau=pc.TAU, cover_pixels=cover)
        for i in range(16):
            assert tuple(c.read_debug(i, "sum_n_r")[0, 0]) == terms[i], (cover, i)
            want = costs[i] if cover else pso_ref.cost(terms[i][0], terms[i][1], terms[i][1])
            assert bits(got[i]["cost"]) == bits(want) == bits(got[i]["initial_cost"]) == bits(c.read_debug(i, "cost")[0, 0]), (cover, i)
            assert got[i]["n_rendered"] == terms[i][1] and got[i]["n_initial"] == (cover or terms[i][1])
            assert np.array_equal(bits(got[i]["R"]), bits(Rs[i])) and np.array_equal(bits(got[i]["t"]), bits(ts[i]))   # the pose is left as given
            assert c.read_debug(i, "x").shape == (1, 1, 6)
    c.close()


@pytest.mark.parametrize("options", [dict(particles=1, generations=3), dict(particles=65, generations=2, trans_range_mm=60.0),
                                     dict(window_size=(8, 8), generations=2), dict(window_size=(72, 40), generations=2)],
                         ids=["P1", "P65", "8x8", "72x40"])
def test_odd_shapes(ctx, mesh, options):
    o = dict(options)
    got = run(ctx, mesh, o.pop("window_size", pc.WIN), **o)
    assert_equals_reference(ctx, got, pc.reference(**options))


def test_repeatable_and_leaves_the_mesh_alone(ctx, mesh):
    Rv, tv = pc.hypotheses()
    before = mesh.render((pc.W, pc.H), pc.K, Rv[:1], tv[:1], mode="depth").tobytes()
    a = run(ctx, mesh)
    xa = ctx.read_debug(2, "x")
    b = run(ctx, mesh)
    assert np.array_equal(bits(xa), bits(ctx.read_debug(2, "x")))
    for ga, gb in zip(a, b):
        assert all(np.array_equal(bits(ga[k]), bits(gb[k])) for k in ("R", "t", "cost"))
    run(ctx, mesh, seed=pc.SEED + 1)
    xs = ctx.read_debug(2, "x")
    assert not np.array_equal(bits(xa), bits(xs)) and np.array_equal(bits(xs), bits(pc.reference(seed=pc.SEED + 1)[2]["x"]))
    assert mesh.render((pc.W, pc.H), pc.K, Rv[:1], tv[:1], mode="depth").tobytes() == before


def test_the_refiner_refines(lm, mesh):
    """(a) and (c): the cost does not rise, the translation error falls; through pso_refine, the one-call form."""
    Rs, ts = pc.hypotheses()
    got, ms = lm.pso_refine(mesh, pc.scene(), pc.K, Rs, ts, pc.WINDOWS, pc.WIN, **pc.OPTIONS)
    ref = pc.reference()
    for h in (0, 2):
        assert got[h]["cost"] <= got[h]["initial_cost"]
        assert np.linalg.norm(got[h]["t"] - pc.PLANTED_T[h]) < np.linalg.norm(ts[h] - pc.PLANTED_T[h])
        assert np.array_equal(bits(got[h]["t"]), bits(ref[h]["t"]))
    assert ms > 0.0
    # windows derived on the host: multiples of 8 that hold the sphere around t0
    got2, _ = lm.pso_refine(mesh, pc.scene(), pc.K, Rs[:1], ts[:1], **pc.OPTIONS)
    xy, (w, h) = lm.derive_windows(pc.K, ts[:1], mesh.diameter() / 2.0 + 20.0)
    assert w % 8 == 0 and h % 8 == 0 and 8 <= w <= 256 and 8 <= h <= 256
    V, F = pc.mesh()
    want = pso_ref.run(V, F, pc.K, pc.scene(), Rs[:1], ts[:1], xy, w, h, **pc.OPTIONS)[0]
    assert np.array_equal(bits(got2[0]["t"]), bits(want["t"])) and bits(got2[0]["cost"]) == bits(want["final_cost"])


def test_refusals(lm, mesh):
    Rs, ts = pc.hypotheses()
    c = lm.PsoContext(0)
    with pytest.raises(RuntimeError, match="no scene depth set"):
        c.run(mesh, Rs, ts, pc.WINDOWS, pc.WIN, **pc.OPTIONS)
    c.set_scene(pc.scene(), pc.K)
    bad = [(dict(particles=0), "particles must be in 1..256"), (dict(particles=257), "particles must be in 1..256"),
           (dict(particles=256, count=17), "hypotheses x particles must be in 1..4096"),
           (dict(window_size=(7, 40)), "the window must be 8..256"), (dict(window_size=(48, 257)), "the window must be 8..256"),
           (dict(generations=-1), "generations must be in 0..256"), (dict(generations=257), "generations must be in 0..256"),
           (dict(tau=0), "tau must be in 1..65535"), (dict(tau=65536), "tau must be in 1..65535"),
           (dict(trans_range_mm=0.0), "trans_range_mm must be finite and > 0"), (dict(trans_range_mm=float("inf")), "trans_range_mm must be finite and > 0"),
           (dict(rot_range=float("nan")), "rot_range must be finite and > 0"), (dict(rot_range_deg=-1.0), "rot_range must be finite and > 0")]
    for options, message in bad:
        o = dict(pc.OPTIONS); o.update(options)
        n = o.pop("count", 4)
        win = o.pop("window_size", pc.WIN)
        with pytest.raises(RuntimeError, match=message):
            c.run(mesh, np.tile(Rs[:1], (n, 1, 1)), np.tile(ts[:1], (n, 1)), np.tile(pc.WINDOWS[:1], (n, 1)), win, **o)
    with pytest.raises(RuntimeError, match="no run to read back"):
        c.read_debug(0, "x")
    c.run(mesh, Rs, ts, pc.WINDOWS, pc.WIN, **pc.OPTIONS)                                # and the context still works
    with pytest.raises(RuntimeError, match="hypothesis 4 out of range"):
        c.read_debug(4, "x")
    c.close()
