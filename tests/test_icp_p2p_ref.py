"""The point-to-point restatement (tests/icp_p2p_ref.py) on its own, on the CPU: the Kabsch update, the loop's EvaluateRegistration
corner, and that every case the GPU test (tests/test_gpu_icp_p2p.py) compares is well-posed on the restatement's own evidence, so
that the GPU test has nothing to skip."""
import numpy as np
import pytest

import icp_p2p_ref as ref


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(deg)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * K @ K


def _sums(p, q):
    d2 = ((p - q) ** 2).sum(1)
    return np.concatenate([[len(p)], [d2.sum()], p.sum(0), q.sum(0), (q[:, :, None] * p[:, None, :]).sum(0).reshape(9)])


@pytest.mark.parametrize("n,deg", [(3, 20.0), (4, 179.0), (50, 2.0), (500, 75.0)])
def test_kabsch_recovers_a_rigid_motion(n, deg):
    rng = np.random.default_rng(n)
    p = rng.normal(size=(n, 3))
    R, t = _rot(rng.normal(size=3), deg), rng.normal(size=3)
    T = ref.kabsch(_sums(p, p @ R.T + t))
    assert np.abs(T[:3, :3] - R).max() < 1e-12 and np.abs(T[:3, 3] - t).max() < 1e-12
    assert np.array_equal(T[3], [0, 0, 0, 1])


def test_kabsch_gives_a_proper_rotation_for_a_mirror_image():
    rng = np.random.default_rng(7)
    p = rng.normal(size=(40, 3))
    q = p * np.array([1.0, 1.0, -1.0]) + 0.3                  # no rotation maps p to q
    T = ref.kabsch(_sums(p, q))
    R = T[:3, :3]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    # and it is the best one: no worse than the identity and than random rotations about the centroids
    pc, qc = p - p.mean(0), q - q.mean(0)
    cost = lambda M: ((pc @ M.T - qc) ** 2).sum()
    assert all(cost(R) <= cost(_rot(rng.normal(size=3), rng.uniform(0, 180))) + 1e-9 for _ in range(200)) and cost(R) <= cost(np.eye(3)) + 1e-9


def test_kabsch_identity_rule():
    rng = np.random.default_rng(9)
    p = rng.normal(size=(2, 3))
    assert np.array_equal(ref.kabsch(_sums(p, p + 0.5)), np.eye(4))                 # n = 2
    s = _sums(rng.normal(size=(10, 3)), rng.normal(size=(10, 3)))
    s[2:] = np.nan
    assert np.array_equal(ref.kabsch(s), np.eye(4))                                 # NaN sums
    assert np.array_equal(ref.kabsch(np.zeros(17)), np.eye(4))                      # no correspondences


def test_sums_are_the_correspondences_of_the_oracle_search():
    rng = np.random.default_rng(11)
    tgt = rng.uniform(0, 0.05, (300, 3))
    src = tgt[rng.permutation(300)[:200]] + rng.normal(0, 0.002, (200, 3))
    fit, rmse, s = ref.icp_eval_p2p(src, tgt, 0.003)
    d2 = ref._sqdist(src, tgt)
    j = d2.argmin(1)
    ok = d2.min(1) < 0.003 ** 2
    assert 0 < ok.sum() < 200 and s[0] == ok.sum() and fit == ok.sum() / 200.0
    assert np.allclose(s, _sums(src[ok], tgt[j[ok]]), rtol=1e-12, atol=0) and abs(rmse - np.sqrt(d2.min(1)[ok].mean())) < 1e-15


def test_max_iter_0_is_evaluate_registration():
    rng = np.random.default_rng(13)
    tgt = rng.uniform(0, 0.05, (400, 3))
    src = tgt[:250] + rng.normal(0, 0.001, (250, 3))
    init = np.eye(4)
    init[:3, :3] = _rot((1, 2, 3), 1.0)
    init[:3, 3] = (0.001, -0.002, 0.0015)
    hist = []
    T, fit, rmse, it = ref.icp_point_to_point(src, tgt, init, 0.01, max_iter=0, history=hist)
    f0, r0, _ = ref.icp_eval_p2p(src @ init[:3, :3].T + init[:3, 3], tgt, 0.01)
    assert np.array_equal(T, init) and it == 0 and (fit, rmse) == (f0, r0) and len(hist) == 1
    # ... and the loop goes somewhere from there: a full run ends closer
    T2, fit2, rmse2, it2 = ref.icp_point_to_point(src, tgt, init, 0.01)
    assert it2 >= 1 and rmse2 < rmse and fit2 >= fit


@pytest.mark.parametrize("name,estimation,max_iter,rel", ref.RUNS, ids=["%s-%s-%d-%g" % r for r in ref.RUNS])
def test_gpu_cases_are_well_posed(name, estimation, max_iter, rel):
    """Every run tests/test_gpu_icp_p2p.py compares with the restatement: well-posed by ill_posed_p2p (or the oracle's ill_posed for
    the point-to-plane runs), and of the kind its case claims."""
    case, sfs = ref.cases()[name]
    for i, nm in enumerate(case.names):
        r = ref.reference(case, sfs, i, estimation, max_iter, rel)
        if nm == "out of frame":
            assert r["residual"] == -1.0
            continue
        assert r["residual"] != -1.0 and np.all(np.isfinite(r["R"])) and np.all(np.isfinite(r["t"])), nm
        assert ref.ill_posed_run(r, rel, rel, estimation) == "", (name, nm, ref.ill_posed_run(r, rel, rel, estimation))
        assert r["iterations"] <= max_iter
        if nm in ("no correspondences", "verbatim, 0.3 m"):
            assert r["residual"] == 0.0 and np.array_equal(r["T_icp"], r["init_guess"]), nm
        elif max_iter == 30:
            assert r["residual"] > 0.5, (nm, r["residual"])
            if nm == "verbatim, 3 mm":                         # back to the identity: the unrefined pose, fitness 1
                assert r["residual"] == 1.0 and np.abs(r["T_icp"] - np.eye(4)).max() < 1e-6


def test_case_sizes():
    """The shapes the GPU test is about: a few hundred points, and more than 256 per slice of 64."""
    c = ref.cases()
    small = ref.reference(*c["small"], 0, "point_to_point", 0, ref.ICP_REL)
    large = ref.reference(*c["large"], 0, "point_to_point", 0, ref.ICP_REL)
    assert small["n_source"] < 512 and large["n_source"] > 64 * 256, (small["n_source"], large["n_source"])
