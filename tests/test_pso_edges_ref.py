"""tests/pso_edges_ref.py, the numpy statement of the refiner's edge cost, checked on its own (CPU): the separable distance transform
against the definition, the contour against a per-pixel statement in Python integers, and the conditions the GPU test's inputs
(tests/pso_edge_cases.py) have to meet for tests/test_gpu_pso_edges.py to mean what it says."""
import numpy as np

import pso_cases as pc
import pso_edge_cases as ec
import pso_edges_ref as pe
import pso_ref


def test_the_separable_distance_is_the_definition():
    rng = np.random.default_rng(0)
    for _ in range(40):
        H, W = (int(v) for v in rng.integers(1, 14, 2))
        M = int(rng.integers(1, 9))
        E = (rng.random((H, W)) < rng.choice([0.0, 0.05, 0.3])).astype(np.uint8) * 200
        d2 = pe.distance(E, M)
        assert d2.dtype == np.uint16 and np.array_equal(d2, pe.distance_brute(E, M)), (H, W, M)
        assert np.array_equal(d2, np.minimum(ec.exact_d2(E), M * M))
    assert np.array_equal(pe.distance(np.zeros((3, 4), np.uint8), 255), np.full((3, 4), 65025, np.uint16))
    assert np.array_equal(pe.row_distance(np.array([[0, 0, 1, 0, 0, 0, 0]], np.uint8), 3), [[2, 1, 0, 1, 2, 3, 3]])
    assert pe.distance(np.array([[True, False]]), 1).tolist() == [[0, 1]]            # bool maps, M = 1


def test_the_contour_agrees_with_a_per_pixel_statement():
    rng = np.random.default_rng(1)
    r = rng.integers(395, 425, (9, 13)).astype(np.uint16); r[rng.random((9, 13)) < 0.3] = 0
    r[0, 0], r[0, 1], r[8, 12] = 65535, 1, 400
    for step in (0, 1, 10, 65535):
        want = np.zeros((9, 13), bool)
        for y in range(9):
            for x in range(13):
                c = int(r[y, x])
                if c == 0:
                    continue
                for ny, nx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= ny < 9 and 0 <= nx < 13:
                        n = int(r[ny, nx])
                        if n == 0 or (step > 0 and n - c > step):
                            want[y, x] = True
        assert np.array_equal(pe.contour(r, step), want), step
    # a window filled to its border has no contour: neighbours outside the window are ignored
    assert not pe.contour(np.full((5, 6), 400, np.uint16), 0).any()
    # the terms: D2 under the contour, tau^2 past the frame
    D2 = np.arange(20, dtype=np.uint16).reshape(4, 5) * 3
    w = np.zeros((3, 3), np.uint16); w[1, 1] = 400                                   # one rendered pixel: a contour pixel at window (1, 1)
    assert pe.cost_terms(w, D2, 2, 1, 4) == (min(int(D2[2, 3]), 16), 1) == (16, 1)
    assert pe.cost_terms(w, D2, 0, 0, 5) == (int(D2[1, 1]), 1) == (18, 1)
    assert pe.cost_terms(w, D2, 4, 0, 4) == (16, 1) and pe.cost_terms(w, D2, -2, 0, 4) == (16, 1) and pe.cost_terms(w, D2, 0, 3, 4) == (16, 1)
    assert pe.cost_terms(np.zeros((3, 3), np.uint16), D2, 0, 0, 4) == (0, 0)


def test_the_distance_cases_sit_on_the_cap():
    """Pixels at distance exactly M - 1, M and M + 1 from the nearest edge: along a row and a column ('one'), and on the (3, 4) diagonal."""
    for (W, H), M in (((67, 45), 32), ((67, 45), 5), ((300, 70), 32), ((300, 70), 2)):
        exact = ec.exact_d2(ec.edt_maps(W, H)["one"])
        for d in (M - 1, M, M + 1):
            assert exact[0, d] == d * d and exact[d, 0] == d * d, (W, H, M, d)
        counts = [int((exact == d * d).sum()) for d in (M - 1, M, M + 1)]
        assert min(counts) >= 2, counts
    exact = ec.exact_d2(ec.edt_maps(300, 40)["one"])
    assert [int(exact[0, d]) for d in (254, 255, 256)] == [254 ** 2, 255 ** 2, 256 ** 2]          # M = 255: along the row only
    e = ec.diagonal_map()
    assert ec.exact_d2(e)[2 + 4, 3 + 3] == 25 and ec.DIAGONAL_M == (4, 5, 6)
    assert [int(pe.distance(e, M)[6, 6]) for M in ec.DIAGONAL_M] == [16, 25, 25]
    p = ec.edt_maps(67, 45)["pair"]
    assert np.count_nonzero(p) == 2 and pe.distance(p, 5)[45 // 2, 67 // 2] == 9
    rnd = ec.edt_maps(300, 70)["random"]
    assert 60 < np.count_nonzero(rnd) < 160 and np.count_nonzero(rnd[:, 250:]) > 0 and np.count_nonzero(rnd[40:]) > 0


def test_the_steps_mesh_has_jumps_of_exactly_10_and_11():
    r = ec.steps_render().astype(np.int64)
    assert sorted(np.unique(r)) == [0, 400, 410, 421]
    jumps = set()
    for a, b in ((r[:, 1:], r[:, :-1]), (r[1:, :], r[:-1, :])):
        on = (a > 0) & (b > 0)
        jumps |= set(np.abs(a - b)[on].tolist())
    assert jumps == {0, 10, 11, 21}
    n = [int(pe.contour(r, s).sum()) for s in ec.STEPS]                              # 0, 10, 11, 21
    assert n[0] == n[3] < n[2] < n[1]                                                # silhouette; + jumps 11 and 21; + jump 21; silhouette
    assert int(pe.contour(r, 9).sum()) > n[1]


def test_the_evaluate_only_inputs_hold_every_edge():
    V, F = pc.mesh()
    Rs, ts, wins = ec.eval_poses()
    terms, n_0, costs = ec.eval_reference()
    assert terms[10] == (0, 0) and costs[10] == float("inf")                         # renders nothing
    assert terms[11][1] == (n_0 + 1) // 2 and np.isfinite(costs[11])                 # exactly on the cover floor
    assert terms[12][1] == (n_0 + 1) // 2 - 1 and costs[12] == float("inf")          # one below it
    assert terms[0][0] < terms[0][1]                                                 # the scene's own pose lies on its edges
    outside = []
    for i in (13, 14, 15):                                                           # contour pixels beyond the frame's edge
        c = pe.contour(pso_ref.render_window(V, F, pc.K, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), *pc.WIN))
        ys, xs = np.nonzero(c)
        outside.append(int(((xs + wins[i][0] >= pc.W) | (ys + wins[i][1] >= pc.H)).sum()))
    assert outside == [3, 4, 23], outside
    # 11 and 12 are cut by the window's left border: rendered pixels in column 0, none of them a contour pixel because of the cut
    for i in (11, 12):
        r = pso_ref.render_window(V, F, pc.K, Rs[i], ts[i], int(wins[i][0]), int(wins[i][1]), *pc.WIN)
        col = np.nonzero(r[:, 0])[0]
        assert len(col) > 10 and not pe.contour(r)[col[1:-1], 0].any()
    assert len({t for t in terms}) >= 14


def test_the_trajectory_inputs_are_what_they_claim():
    e = ec.edge_scene()
    assert e.dtype == np.uint8 and e.shape == (pc.H, pc.W) and not e[14:20, 48:96].any() and e[30, 4:60].all()
    d2 = ec.scene_d2()
    assert d2.max() == ec.M ** 2 and (d2 > ec.TAU ** 2).any() and (d2 == 0).sum() == np.count_nonzero(e)
    ref = ec.reference()
    for key in ("x", "cost", "sum", "n_r", "best"):                                  # (d) is (a): identical swarms
        assert np.array_equal(ref[0][key], ref[3][key])
    for h in range(4):
        assert len({tuple(b) for b in ref[h]["best"]}) >= 2
        assert not np.array_equal(ref[h]["x"][0], ref[h]["x"][pc.G])
        assert ref[h]["n_r"].min() > 0 and ref[h]["sum"].max() <= ref[h]["n_r"].max() * ec.TAU ** 2
    # the swarm is pso_ref's: the same positions in generation 0 as the depth cost's run, another trajectory afterwards
    assert np.array_equal(ref[0]["x"][0], pc.reference()[0]["x"][0]) and not np.array_equal(ref[0]["x"][pc.G], pc.reference()[0]["x"][pc.G])
    assert pso_ref.cost_terms.__module__ == "pso_ref" and pso_ref.window_scene.__module__ == "pso_ref"       # the hooks are put back


def test_the_cover_floor_acts_in_a_swarm():
    ref = ec.reference(particles=65, generations=2, trans_range_mm=60.0)
    infs = sum(int(np.isinf(r["cost"]).sum()) for r in ref)
    assert infs > 0 and all(np.isfinite(r["final_cost"]) for r in ref)


def test_the_reference_refines():
    """The conditions tests/test_gpu_pso_edges.py asserts of the device, met by the numpy statement for ec.REFINE: the projected centre
    of the start is more than 2 px off and ends less than 1 px off, and the cost falls."""
    r = ec.refine_reference()
    want = ec.centre_px(pc.T_A)
    assert np.linalg.norm(ec.centre_px(ec.REFINE_T0) - want) > 2.0
    assert np.linalg.norm(ec.centre_px(r["t"]) - want) < 1.0
    assert r["final_cost"] < r["initial_cost"]
