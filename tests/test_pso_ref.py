"""tests/pso_ref.py, the numpy statement of the particle-swarm refiner, checked on its own (CPU): the random numbers against known
answers, the Cayley rotation, the cost against a per-pixel statement in Python integers, and the conditions the GPU test's inputs
(tests/pso_cases.py) have to meet for tests/test_gpu_pso.py to mean what it says."""
import numpy as np

import pso_cases as pc
import pso_ref


def test_random_numbers_match_the_known_answers():
    for seed, counter, want in pso_ref.KNOWN_ANSWERS:
        assert pso_ref.mix(seed, counter) == want
    # counter c at seed s is counter 0 at seed s + GOLDEN c: the sequence is splitmix64's
    assert pso_ref.mix(12345, 7) == pso_ref.mix((12345 + 7 * pso_ref.GOLDEN) & pso_ref.MASK, 0)
    u = [pso_ref.uniform(3, c) for c in range(2000)]
    assert all(0.0 <= v < 1.0 for v in u) and 0.45 < np.mean(u) < 0.55
    assert pso_ref.uniform(0, 0) == float(0xE220A8397B1DCDAF >> 11) / 2.0 ** 53
    assert len({pso_ref.counter(g, 5, p, d, k) for g in range(3) for p in range(5) for d in range(6) for k in range(2)}) == 3 * 5 * 6 * 2


def test_cayley_rotation_is_orthonormal():
    assert np.array_equal(pso_ref.cayley([0.0, 0.0, 0.0]), np.eye(3))
    rng = np.random.default_rng(1)
    for a in list(rng.uniform(-0.2, 0.2, (50, 3))) + [[1.0, 0, 0], [0.3, -0.9, 0.5], [0, 0, pso_ref.DEFAULTS["rot_range"]]]:
        R = pso_ref.cayley(a)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
    # tan(angle / 2) about an axis is that angle
    R = pso_ref.cayley([0, 0, np.tan(np.radians(10.0) / 2)])
    assert np.allclose(R, pc.rot((0, 0, 1), 10.0), atol=1e-15)
    R, t = pso_ref.particle_pose(pc.R_A, pc.T_A, np.zeros(6))
    assert np.array_equal(R, pc.R_A) and np.array_equal(t, pc.T_A)


def test_cost_agrees_with_a_per_pixel_statement():
    rng = np.random.default_rng(2)
    r = rng.integers(380, 440, (8, 16)).astype(np.uint16); r[rng.random((8, 16)) < 0.3] = 0
    s = (r.astype(np.int64) + rng.integers(-30, 31, (8, 16))).astype(np.uint16); s[rng.random((8, 16)) < 0.2] = 0
    s[0, 0], r[0, 0], s[1, 1], r[1, 1] = 65535, 400, 5, 65535
    for tau in (1, 20, 65535):
        total = n_r = 0
        for y in range(8):
            for x in range(16):
                if int(r[y, x]) > 0:
                    n_r += 1
                    total += tau if int(s[y, x]) == 0 else min(abs(int(r[y, x]) - int(s[y, x])), tau)
        assert pso_ref.cost_terms(r, s, tau) == (total, n_r)
    assert pso_ref.cost(30, 4, 8) == 7.5 and pso_ref.cost(30, 4, 7) == 7.5 and pso_ref.cost(30, 3, 7) == float("inf")
    assert pso_ref.cost(0, 0, 0) == float("inf") and pso_ref.cost(0, 1, 0) == 0.0
    # the window: the frame's content where it lies inside, 0 outside
    frame = np.arange(1, 31, dtype=np.uint16).reshape(5, 6)
    win = pso_ref.window_scene(frame, 4, -1, 4, 3)
    assert np.array_equal(win, [[0, 0, 0, 0], [5, 6, 0, 0], [11, 12, 0, 0]])


def test_the_evaluate_only_inputs_hold_every_edge():
    V, F = pc.mesh()
    Rs, ts, wins = pc.eval_poses()
    scene = pc.eval_scene()
    terms, n_0, costs = pc.eval_reference()
    r = pso_ref.render_window(V, F, pc.K, Rs[0], ts[0], int(wins[0][0]), int(wins[0][1]), *pc.WIN).astype(np.int64)
    s = pso_ref.window_scene(scene, int(wins[0][0]), int(wins[0][1]), *pc.WIN).astype(np.int64)
    diff = np.abs(r - s)[(r > 0) & (s > 0)]
    for want in (pc.TAU, pc.TAU - 1, pc.TAU + 1):
        assert (diff == want).any(), want
    assert ((s == 65535) & (r > 0)).any() and ((s == 0) & (r > 0)).any()
    assert terms[10] == (0, 0) and costs[10] == float("inf")                     # renders nothing
    assert terms[11][1] == (n_0 + 1) // 2 and np.isfinite(costs[11])             # exactly on the cover floor
    assert terms[12][1] == (n_0 + 1) // 2 - 1 and costs[12] == float("inf")      # one below it
    for i in (13, 14, 15):                                                       # rendered pixels beyond the frame's edge
        rr = pso_ref.render_window(V, F, pc.K, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), *pc.WIN)
        ys, xs = np.nonzero(rr)
        assert ((xs + wins[i][0] >= pc.W) | (ys + wins[i][1] >= pc.H)).any(), i
    assert len({t for t in terms}) >= 14                                         # the poses are not copies of one another


def test_the_trajectory_inputs_are_what_they_claim():
    V, F = pc.mesh()
    scene = pc.scene()
    ref = pc.reference()
    Rs, ts = pc.hypotheses()
    # (b): the window leaves the frame on the right and at the bottom, with rendered pixels out there
    x0, y0 = pc.WINDOWS[1]
    assert x0 + pc.WIN[0] > pc.W and y0 + pc.WIN[1] > pc.H
    rr = pso_ref.render_window(V, F, pc.K, Rs[1], ts[1], int(x0), int(y0), *pc.WIN)
    ys, xs = np.nonzero(rr)
    assert (xs + x0 >= pc.W).any() or (ys + y0 >= pc.H).any()
    # (c): holes and an occluder about 100 mm in front, each over part of the object
    x0, y0 = pc.WINDOWS[2]
    rr = pso_ref.render_window(V, F, pc.K, pc.R_C, pc.T_C, int(x0), int(y0), *pc.WIN).astype(np.int64)
    sw = pso_ref.window_scene(scene, int(x0), int(y0), *pc.WIN).astype(np.int64)
    on = rr > 0
    assert ((sw == 0) & on).sum() > 20
    occluded = on & (sw > 0) & (rr - sw > 60)
    assert 0.2 * on.sum() < occluded.sum() < 0.45 * on.sum()
    # (d) is (a): identical swarms
    for key in ("x", "cost", "sum", "n_r", "best"):
        assert np.array_equal(ref[0][key], ref[3][key])
    # the swarm moves, the global best changes hands, and the start is 4 degrees and 6 mm off
    assert abs(np.linalg.norm(pc.D_T) - 6.0) < 0.05
    for h in range(4):
        assert len({tuple(b) for b in ref[h]["best"]}) >= 2
        assert not np.array_equal(ref[h]["x"][0], ref[h]["x"][pc.G])
        assert np.array_equal(ref[h]["x"][:, 0][0], np.zeros(6))
        assert np.abs(ref[h]["x"][..., :3]).max() <= 20.0 and np.abs(ref[h]["x"][..., 3:]).max() <= pso_ref.DEFAULTS["rot_range"]


def test_the_reference_refines():
    """(a) and (c): the cost does not rise and the translation error falls, strictly, for the chosen inputs and seed."""
    ref = pc.reference()
    _, ts = pc.hypotheses()
    for h in (0, 2):
        assert ref[h]["final_cost"] <= ref[h]["initial_cost"]
        assert np.linalg.norm(ref[h]["t"] - pc.PLANTED_T[h]) < np.linalg.norm(ts[h] - pc.PLANTED_T[h])


def test_the_cover_floor_acts_in_a_swarm():
    """With a range wide enough to leave the window some particles fall under the floor: +inf in the record the GPU test compares."""
    ref = pc.reference(particles=65, generations=2, trans_range_mm=60.0)
    infs = sum(int(np.isinf(r["cost"]).sum()) for r in ref)
    assert infs > 0 and all(np.isfinite(r["final_cost"]) for r in ref)


def test_another_seed_is_another_trajectory():
    a, b = pc.reference(), pc.reference(seed=pc.SEED + 1)
    assert not np.array_equal(a[0]["x"][0], b[0]["x"][0]) and np.array_equal(a[0]["x"][0, 0], b[0]["x"][0, 0])
