"""CPU tests of the host side of the symmetry-aware evaluation: symmetry_transforms against the numpy restatement
(tests/pose_sym_ref.py) and geometric facts, match_poses against the reference's own pysixd/pose_matching.py recorded in
tests/golden/pose_matching_golden.json, recall and bop19_thresholds on hand-built cases."""
import json
import math
import os

import numpy as np
import pytest

import pose_sym_ref as psr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lm():
    import linemodLevelup_pybind as mod
    return mod


def rot(axis, deg):
    return psr.rodrigues(axis, math.radians(deg))


@pytest.mark.parametrize("step,n", [(0.01, 315), (0.3, 11), (1.0, 4)])
def test_continuous_symmetry_counts(lm, step, n):
    assert psr.disc_count(step) == n
    Rs, ts = lm.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_sym_disc_step=step)
    assert Rs.shape == (n - 1, 3, 3) and ts.shape == (n - 1, 3) and Rs.dtype == np.float64 and ts.dtype == np.float64
    # two discrete symmetries (D = 3 with the identity) and two axes: S = 3 * 2 (n - 1)
    Rs, ts = lm.symmetry_transforms([psr.as4x4(rot([1, 0, 0], 180)), psr.as4x4(rot([0, 1, 0], 180)).ravel().tolist()],
                                    [((0, 0, 1), (0, 0, 0)), ((1, 1, 0), (3, 4, 5))], step)
    assert Rs.shape == (3 * 2 * (n - 1), 3, 3)
    want = psr.symmetry_transforms([psr.as4x4(rot([1, 0, 0], 180)), psr.as4x4(rot([0, 1, 0], 180))],
                                   [((0, 0, 1), (0, 0, 0)), ((1, 1, 0), (3, 4, 5))], step)
    assert np.abs(Rs - want[0]).max() <= 1e-15 and np.abs(ts - want[1]).max() <= 1e-13
    for R in Rs:
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12


def test_no_symmetry_is_the_identity(lm):
    Rs, ts = lm.symmetry_transforms()
    assert Rs.shape == (1, 3, 3) and np.array_equal(Rs[0], np.eye(3)) and np.array_equal(ts, np.zeros((1, 3)))


def test_cube_rotations_map_the_vertex_set_onto_itself(lm):
    V = np.array([[x, y, z] for x in (-40.0, 40.0) for y in (-40.0, 40.0) for z in (-40.0, 40.0)])
    rots = psr.cube_rotations()
    Rs, ts = lm.symmetry_transforms([psr.as4x4(R) for R in rots[1:]])
    assert Rs.shape == (24, 3, 3) and np.array_equal(ts, np.zeros((24, 3)))
    assert np.array_equal(Rs[0], np.eye(3))
    want = sorted(map(tuple, V.tolist()))
    for R, t in zip(Rs, ts):
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
        assert sorted(map(tuple, psr.transform(R, t, V).tolist())) == want


def test_cylinder_axis_with_offset_keeps_the_axis_fixed(lm):
    axis, off = np.array([1.0, 2.0, -0.5]), np.array([12.0, -7.0, 30.0])
    Rs, ts = lm.symmetry_transforms(continuous=[(axis, off)], max_sym_disc_step=0.3)
    u = axis / np.linalg.norm(axis)
    on_axis = off[None] + np.array([-50.0, 0.0, 13.0, 200.0])[:, None] * u[None]
    away = off + np.array([5.0, 0.0, 0.0])
    moved = 0.0
    for R, t in zip(Rs, ts):
        assert np.abs(psr.transform(R, t, on_axis) - on_axis).max() <= 1e-12
        q = psr.transform(R, t, away[None])[0]
        assert abs(np.linalg.norm(q - off) - 5.0) <= 1e-12             # a rotation about the offset point
        moved = max(moved, np.linalg.norm(q - away))
    assert moved > 5.0


def test_composition_order_of_discrete_and_continuous(lm):
    """One generic discrete symmetry and one continuous one: D = [I, d], C = [c_1 .. c_(n-1)]; the result lists, for d in D
    (outer) and c in C (inner), x -> c(d(x)) = R_c (R_d x + t_d) + t_c, i.e. R = R_c R_d, t = R_c t_d + t_c.  The other
    order, d(c(x)), gives R_d R_c and R_d t_c + t_d, which differs for a generic d."""
    Rd, td = rot([0.3, -1.0, 0.2], 50.0), np.array([4.0, -9.0, 2.5])
    axis, off = np.array([0.2, 0.1, 1.0]), np.array([-3.0, 8.0, 1.0])
    n = 4                                                              # step 1.0: angles 90, 180, 270 degrees
    Rs, ts = lm.symmetry_transforms([psr.as4x4(Rd, td)], [(axis, off)], 1.0)
    assert Rs.shape == (2 * (n - 1), 3, 3)
    x = np.array([10.0, -20.0, 35.0])
    k = 0
    for R_d, t_d in ((np.eye(3), np.zeros(3)), (Rd, td)):
        for i in range(1, n):
            Rc = rot(axis, 90.0 * i)
            tc = off - Rc @ off
            assert np.abs(Rs[k] - Rc @ R_d).max() <= 1e-14, k
            assert np.abs(ts[k] - (Rc @ t_d + tc)).max() <= 1e-13, k
            assert np.abs((Rs[k] @ x + ts[k]) - (Rc @ (R_d @ x + t_d) + tc)).max() <= 1e-12
            if k >= n - 1:                                              # the other order is a different transformation
                assert np.abs(Rs[k] - R_d @ Rc).max() > 1e-2
            k += 1
    # S = 1 x (n - 1) when the only discrete entry is the identity
    assert lm.symmetry_transforms((), [(axis, off)], 1.0)[0].shape == (n - 1, 3, 3)


def test_bad_symmetries_raise(lm):
    with pytest.raises(RuntimeError, match="axis"):
        lm.symmetry_transforms(continuous=[((0, 0, 0), (1, 2, 3))])
    bad = psr.as4x4(np.eye(3))
    bad[3, 0] = 0.5
    with pytest.raises(RuntimeError, match="bottom row"):
        lm.symmetry_transforms([bad])
    with pytest.raises(RuntimeError):
        lm.symmetry_transforms([np.eye(3)])


def test_match_poses_equals_the_reference(lm):
    cases = json.load(open(os.path.join(HERE, "golden", "pose_matching_golden.json")))
    assert len(cases) >= 30
    seen = {"ties": 0, "masked": 0, "all_false": 0, "capped": 0, "empty": 0, "matched": 0}
    for i, c in enumerate(cases):
        errs = np.asarray(c["errs"], np.float64).reshape(len(c["scores"]), c["G"])
        kw = {}
        if c["max_ests"] is not None:
            kw["max_ests_count"] = c["max_ests"]
        if c["mask"] is not None:
            kw["gt_valid_mask"] = c["mask"]
        got = lm.match_poses(errs, c["scores"], c["thresh"], **kw)
        want = c["matches"]
        assert len(got) == len(want), (i, got, want)
        for a, b in zip(got, want):
            assert sorted(a) == ["error", "error_norm", "est_id", "gt_id", "score"]
            assert (a["est_id"], a["gt_id"]) == (b["est_id"], b["gt_id"]), (i, got, want)
            for k in ("score", "error", "error_norm"):                  # bit for bit
                assert isinstance(a[k], float) and np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (i, k, a, b)
        seen["ties"] += len(set(c["scores"])) < len(c["scores"])
        seen["masked"] += bool(c["mask"]) and any(c["mask"])
        seen["all_false"] += bool(c["mask"]) and not any(c["mask"])
        seen["capped"] += c["max_ests"] is not None and 0 < c["max_ests"] < len(c["scores"])
        seen["empty"] += len(c["scores"]) == 0
        seen["matched"] += len(want) > 0
    assert all(v > 0 for v in seen.values()), seen


def test_match_poses_accepts_arrays_and_rejects_bad_shapes(lm):
    errs = np.array([[1.0, 2.0], [0.5, 3.0]])
    a = lm.match_poses(errs, np.array([0.25, 0.75]), 2.5, gt_valid_mask=np.array([True, True]))
    assert [(m["est_id"], m["gt_id"]) for m in a] == [(1, 0), (0, 1)]
    with pytest.raises(ValueError):
        lm.match_poses(errs, [1.0], 2.5)
    with pytest.raises(ValueError):
        lm.match_poses(errs, [1.0, 2.0], 2.5, gt_valid_mask=[1])


def test_recall_on_two_images(lm):
    """Image 0: 3 GTs, GT 2 invalid; estimate 0 (score 0.9) is 4 from GT 0, estimate 1 (0.8) is 12 from GT 1 and 1 from the
    invalid GT 2, estimate 2 (0.1) is 2 from GT 0, which estimate 0 has taken already.  Image 1: 1 GT, one estimate at 7.
    Valid targets: 2 + 1 = 3.
      threshold  5: image 0 matches (0 -> GT 0); estimate 1: 12 >= 5; estimate 2: GT 1 at 30.  Image 1: 7 >= 5.  1 / 3
      threshold 10: as above, and image 1 matches (7 < 10).                                              2 / 3
      threshold 12: 12 < 12 is false, as above.                                                          2 / 3
      threshold 20: estimate 1 -> GT 1 as well.                                                          3 / 3"""
    e0 = np.array([[4.0, 50.0, 60.0], [40.0, 12.0, 1.0], [2.0, 30.0, 70.0]])
    e1 = np.array([[7.0]])
    errs, scores, masks = [e0, e1], [[0.9, 0.8, 0.1], [0.5]], [[1, 1, 0], None]
    for th, want in ((5.0, 1 / 3.0), (10.0, 2 / 3.0), (12.0, 2 / 3.0), (20.0, 1.0)):
        assert lm.recall(errs, scores, th, gt_valid_masks=masks) == want, th
    assert lm.recall(errs, scores, [5.0, 10.0, 12.0, 20.0], gt_valid_masks=masks) == np.mean([1 / 3.0, 2 / 3.0, 2 / 3.0, 1.0])
    # without the masks GT 2 is a target too, and estimate 1 takes it at 1: targets 4
    assert lm.recall(errs, scores, 5.0) == 2 / 4.0
    # the best estimate per image only (n_top = 1): one target per image; at 5 image 0 is found, image 1 is not
    assert lm.recall(errs, scores, 5.0, max_ests_count=1, gt_valid_masks=masks) == 1 / 2.0
    # no targets at all
    assert lm.recall([np.zeros((2, 0))], [[0.5, 0.4]], 5.0) == 0.0
    assert lm.recall([e1], [[0.5]], 10.0, gt_valid_masks=[[0]]) == 0.0


def test_bop19_thresholds(lm):
    ssd, spd = lm.bop19_thresholds(200.0, 1280)
    assert len(ssd) == 10 and len(spd) == 10
    assert np.allclose(ssd, [10, 20, 30, 40, 50, 60, 70, 80, 90, 100], rtol=1e-15, atol=0)
    assert spd == [10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0, 90.0, 100.0]
    assert lm.bop19_thresholds(1.0, 640)[1] == [5.0 * k for k in range(1, 11)]


def test_restated_errors_on_a_symmetric_cube():
    """The restatement itself: a cube rotated by one of its symmetries is at distance 0 with the full set, far with the identity."""
    V = np.array([[x, y, z] for x in (-40.0, 40.0) for y in (-40.0, 40.0) for z in (-40.0, 40.0)])
    rots = psr.cube_rotations()
    Rs, ts = np.stack(rots), np.zeros((24, 3))
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1.0]])
    Rg, tg = rot([0.2, 0.7, 0.1], 25.0), np.array([-60.0, 40.0, 750.0])
    for S in rots[1:]:
        assert psr.mssd(Rg @ S, tg, Rg, tg, V, Rs, ts) <= 1e-9
        assert psr.mspd(Rg @ S, tg, Rg, tg, K, V, Rs, ts) <= 1e-9
        assert psr.mssd(Rg @ S, tg, Rg, tg, V, Rs[:1], ts[:1]) > 10.0
