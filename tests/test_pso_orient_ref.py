"""tests/pso_orient_ref.py, the numpy statement of the refiner's directional edge cost, checked on its own (CPU): the nine planes against
the definition in (x, y, orientation), the bin table, and the conditions the GPU test's inputs (tests/pso_orient_cases.py) have to meet
for tests/test_gpu_pso_orient.py to mean what it says."""
import os
import re

import numpy as np

import pso_cases as pc
import pso_edge_cases as ec
import pso_edges_ref as pe
import pso_orient_cases as oc
import pso_orient_ref as po
import pso_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRUTE_M, BRUTE_P = (1, 5, 32), (0, 1, 16, 4096)


def _brute_maps():
    maps = {"1x1 edge": np.array([[1 << 3]], np.uint8), "1x1 empty": np.zeros((1, 1), np.uint8)}
    q = np.zeros((16, 16), np.uint8)
    for k in range(8):
        q[2 * k + 1, (5 * k + 2) % 16] = 1 << k
    maps["one per bin"] = q
    for seed in (11, 12):
        rng = np.random.default_rng(seed)
        maps["random %d" % seed] = np.where(rng.random((45, 67)) < 1.0 / 200.0, 1 << rng.integers(0, 8, (45, 67)), 0).astype(np.uint8)
    q = np.zeros((16, 16), np.uint8); q[7, 8] = 0x25; q[3, 2] = 0xFF
    maps["multibit"] = q
    maps["tie"] = oc.tie_map(16, 16)[0]
    return maps


def test_the_planes_are_the_definition():
    for name, q in _brute_maps().items():
        for M in BRUTE_M:
            for P in BRUTE_P:
                dd2 = po.orient_distance(q, M, P)
                assert dd2.dtype == np.uint16 and dd2.shape == (9,) + q.shape
                assert np.array_equal(dd2, po.orient_distance_brute(q, M, P)), (name, M, P)
                assert np.array_equal(dd2[8], pe.distance(q != 0, M)), (name, M, P)
                if P == 0:
                    assert all(np.array_equal(dd2[k], dd2[8]) for k in range(8)), (name, M)
    for seed in (11, 12):
        q = _brute_maps()["random %d" % seed]
        assert q.shape == (45, 67) and 5 < np.count_nonzero(q) < 30 and len(np.unique(q)) >= 5


def test_the_tie_and_the_wrap():
    """3^2 + 16 x 1^2 == 5^2: the wrong-bin edge and the right-bin edge are equally far from q in bin 2; one pixel towards either, it wins."""
    q, (cy, cx) = oc.tie_map(16, 16)
    dd2 = po.orient_distance(q, 32, 16)
    assert [int(dd2[2, cy, cx + d]) for d in (-1, 0, 1)] == [16, 25, 20]
    assert [int(dd2[3, cy, cx + d]) for d in (-1, 0, 1)] == [16, 9, 4] and [int(dd2[8, cy, cx + d]) for d in (-1, 0, 1)] == [16, 9, 4]
    assert int(po.orient_distance(q, 32, 17)[2, cy, cx]) == 25 and int(po.orient_distance(q, 32, 15)[2, cy, cx]) == 24
    t, (ty, tx) = oc.tie_map(1, 300)                                                 # the same along y on a frame one pixel wide
    assert [int(po.orient_distance(t, 32, 16)[2, ty + d, tx]) for d in (-1, 0, 1)] == [16, 25, 20] and oc.tie_map(1, 1) == (None, None)
    assert po.bin_distance(0, 7) == 1 and po.bin_distance(0, 4) == 4 and po.bin_distance(7, 0) == 1 and po.bin_distance(6, 1) == 3
    one = np.zeros((5, 5), np.uint8); one[2, 2] = 1 << 7
    dd2 = po.orient_distance(one, 32, 16)
    assert [int(dd2[k, 2, 2]) for k in range(9)] == [16, 64, 144, 256, 144, 64, 16, 0, 0]


def test_the_bin_table():
    """81 entries from float64 atan2, every one at least 0.05 degrees from a bin boundary; the kernel's literal is this table."""
    assert po.BIN_OF.shape == (9, 9) and po.BIN_OF[4, 4] == 8 and (np.delete(po.BIN_OF.ravel(), 40) < 8).all()
    assert po.MARGIN_DEG == 0.05 and 0.0599 < po.BIN_MARGIN_DEG < 0.06
    assert [int(po.BIN_OF[gy + 4, gx + 4]) for gx, gy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))] == [0, 0, 4, 4, 2, 2, 6, 6]
    assert [int(po.BIN_OF[gy + 4, gx + 4]) for gx, gy in ((3, 2), (2, 3), (4, 1), (1, 4), (-4, 1), (4, -1))] == [1, 3, 1, 3, 7, 7]
    assert np.array_equal(po.BIN_OF, po.BIN_OF[::-1, ::-1])                          # the polarity of a gradient does not matter
    text = open(os.path.join(ROOT, "6dpose_amd", "csrc", "pso_orient.hip")).read()
    literal = re.search(r"kBinOf\[81\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", literal)] == po.BIN_OF.ravel().tolist()


def test_the_sobel_sums_agree_with_a_per_pixel_statement():
    rng = np.random.default_rng(2)
    r = rng.integers(395, 425, (9, 13)).astype(np.uint16); r[rng.random((9, 13)) < 0.3] = 0
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    for step in (0, 10, 65535):
        gx, gy = po.sobel_of_outside(r, step)
        for y in range(9):
            for x in range(13):
                o = np.zeros((3, 3), np.int64)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ny, nx = y + dy, x + dx
                        if (dx or dy) and 0 <= ny < 9 and 0 <= nx < 13:
                            n, c = int(r[ny, nx]), int(r[y, x])
                            o[dy + 1, dx + 1] = n == 0 or (step > 0 and n - c > step)
                assert (gx[y, x], gy[y, x]) == ((o * kx).sum(), (o * kx.T).sum()), (step, y, x)
        assert np.abs(gx).max() <= 4 and np.abs(gy).max() <= 4
    # one rendered pixel has no orientation and reads plane 8; outside the frame tau^2
    w = np.zeros((3, 3), np.uint16); w[1, 1] = 400
    dd2 = np.arange(9 * 20, dtype=np.uint16).reshape(9, 4, 5)
    assert po.cost_terms(w, dd2, 0, 0, 32) == (int(dd2[8, 1, 1]), 1)
    w = np.array([[400, 400, 0]], np.uint16)                                          # (0, 1) is the contour: gx = 2, bin 0; transposed gy = 2, bin 4
    assert po.cost_terms(w, dd2, 0, 0, 32) == (int(dd2[0, 0, 1]), 1) and po.cost_terms(w.T, dd2, 0, 0, 32) == (int(dd2[4, 1, 0]), 1)
    assert po.cost_terms(w, dd2, 5, 0, 7) == (49, 1)


def test_the_contour_cases_contain_what_they_claim():
    hist = {(n, i, s): oc.histogram(oc.contour_render(n, i), s) for n, g in oc.contour_groups().items() for i in range(len(g[2])) for s in g[6]}
    h = hist["steps", 0, 0]                                                          # axis-aligned squares: bins 0 and 4, corners in 2 and 6
    assert h[0] > 20 and h[4] > 20 and h[2] > 0 and h[6] > 0 and h[[1, 3, 5, 7, 8]].sum() == 0
    assert np.array_equal(hist["steps", 0, 21], h) and hist["steps", 0, 10].sum() > hist["steps", 0, 11].sum() > h.sum()   # depth-jump contours
    h = hist["steps", 1, 0]                                                          # by 45 degrees: bins 2 and 6
    assert h[2] > 20 and h[6] > 20 and h[[1, 3, 5, 7, 8]].sum() == 0
    h = hist["steps", 2, 0]                                                          # by 22.5 degrees: bins 1 and 5
    assert h[1] > 20 and h[5] > 20 and h[8] == 0
    h = hist["sliver", 0, 0]                                                         # one pixel wide: its ends in bin 4, the rest without orientation
    r = oc.contour_render("sliver", 0)
    assert (np.count_nonzero(r, axis=1) <= 1).all() and h[8] == np.count_nonzero(r) - 2 >= 10 and h[4] == 2 and h[:4].sum() + h[5:8].sum() == 0
    for i in range(4):                                                               # rendered pixels on the border the window cuts at
        r = oc.contour_render("cut", i)
        side = (r[:, 0], r[:, -1], r[0, :], r[-1, :])[i]
        assert np.count_nonzero(side) > 5 and hist["cut", i, 0].sum() > 15 and hist["cut", i, 0][8] == 0
    # together the eight uniform scenes fix the histogram: sum_j = sum over k of h[k] d(k, j)^2 is an invertible system, n_c gives h[8]
    assert np.linalg.matrix_rank(np.array([[po.bin_distance(k, j) ** 2 for k in range(8)] for j in range(8)])) == 8
    h = hist["steps", 0, 0]
    assert oc.contour_reference("steps", 0, 0)[0] == (int(sum(h[k] * po.bin_distance(k, 0) ** 2 for k in range(8))), int(h.sum()))
    assert np.array_equal(oc.uniform_planes(3)[:, 5, 7], [9, 4, 1, 0, 1, 4, 9, 16, 0])


def test_the_scenes_are_what_they_claim():
    q = oc.orient_scene()
    assert q.dtype == np.uint8 and np.array_equal(q != 0, ec.edge_scene() != 0) and set(np.unique(q)) == {0, 1, 2, 4, 8, 16, 32, 64, 128}
    dd2 = oc.scene_planes()
    assert np.array_equal(dd2[8], ec.scene_d2()) and all((dd2[k] >= dd2[8]).all() and (dd2[k] > dd2[8]).any() for k in range(8))
    e = oc.eval_orientations()
    assert (e[40:60, 70] == 16).all() and not e[60].any() and len(np.unique(e)) == 9
    terms, n_0, costs = oc.eval_reference()
    plain = ec.eval_reference()[0]
    assert [t[1] for t in terms] == [t[1] for t in plain] and all(a[0] >= b[0] for a, b in zip(terms, plain))    # the same contours, further away
    assert sum(a[0] > b[0] for a, b in zip(terms, plain)) >= 10 and terms[10] == (0, 0)
    assert terms[11][1] == (n_0 + 1) // 2 and np.isfinite(costs[11]) and costs[12] == float("inf")


def test_without_a_penalty_the_run_is_the_edge_cost_run():
    ref0, plain = oc.reference(orient_penalty=0), ec.reference()
    for h in range(3):
        for key in ("x", "cost", "sum", "n_r", "best", "R", "t"):
            assert np.array_equal(ref0[h][key], plain[h][key]), (h, key)
    ref = oc.reference()
    assert any(not np.array_equal(ref[h]["sum"], plain[h]["sum"]) for h in range(3))                   # P = 16 is another run
    assert all(np.array_equal(ref[h]["n_r"][0], plain[h]["n_r"][0]) for h in range(3))
    assert pso_ref.cost_terms.__module__ == "pso_ref" and pso_ref.window_scene.__module__ == "pso_ref"       # the hooks are put back


def test_orientations_help_against_a_foreign_clutter_line():
    """oc.HELPS on oc.helps_scene(): the oriented reference ends nearer the planted pose than the edges reference, which the clutter
    line of a foreign bin pulls aside.  Asserted of the two numpy references only; the device is held to the oriented one bit for bit."""
    oriented, edges = oc.helps_references()
    want = ec.centre_px(pc.T_A)
    err_o, err_e = (float(np.linalg.norm(ec.centre_px(r["t"]) - want)) for r in (oriented, edges))
    print("centre_px error: oriented %.3f px, edges %.3f px" % (err_o, err_e))
    assert err_o < err_e
    assert (oc.helps_scene()[2:44, oc.HELPS_COLUMN] == 16).all()
