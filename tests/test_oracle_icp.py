"""The ICP oracle's neighbour modes against its plain brute force (CPU only).

oracle.estimate_normals / icp_point_to_plane work through the distance matrix in blocks of rows (bounded memory) or, with
nn="kdtree", through candidates from scipy's cKDTree whose squared distances are recomputed by the oracle's own formula and
ordered by (d^2, index).  Both must give exactly what the whole n x m matrix gives (the restatement below): the same ordered
neighbour lists, normals, transformation, fitness and iteration count, bit for bit — on clouds built to have exact distance
ties (a regular grid, duplicated points) as well as on sensor-like ones.
"""
import numpy as np
import pytest

import linemod_oracle as lo


def _full_knn(pts, k):
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2)
    d2 = d2[..., 0] + d2[..., 1] + d2[..., 2]
    n = len(pts)
    return np.array([np.lexsort((np.arange(n), d2[i]))[:k] for i in range(n)])


def _full_normals(pts, knn=lo.KNN):
    n = len(pts)
    k = min(knn, n)
    out = np.zeros((n, 3))
    for i, nb in enumerate(_full_knn(pts, k)):
        q = pts[nb]
        mean = lo._seq_sum(q) / k
        cov = lo._seq_sum(q[:, :, None] * q[:, None, :]) / k - np.outer(mean, mean)
        w, v = np.linalg.eigh(cov)
        out[i] = v[:, 0] if np.linalg.norm(v[:, 0]) > 0 else (0, 0, 1)
    return out


def _full_eval(src, tgt, nrm, max_dist):
    d2 = ((src[:, None, :] - tgt[None, :, :]) ** 2)
    d2 = d2[..., 0] + d2[..., 1] + d2[..., 2]
    j = d2.argmin(1)
    best = d2[np.arange(len(src)), j]
    ok = best < max_dist * max_dist
    n = int(ok.sum())
    if n == 0:
        return 0.0, 0.0, 0, None, None
    p, q, nt = src[ok], tgt[j[ok]], nrm[j[ok]]
    r = ((p - q) * nt).sum(1)
    J = np.concatenate([np.cross(p, nt), nt], 1)
    return n / float(len(src)), float(np.sqrt(lo._seq_sum(best[ok][:, None])[0] / n)), n, lo._seq_sum(J[:, :, None] * J[:, None, :]), lo._seq_sum(J * r[:, None])


def _full_icp(src, tgt, nrm, init, max_dist=lo.ICP_MAX_DIST, max_iter=lo.ICP_MAX_ITER):
    T = np.array(init, np.float64)
    pts = src @ T[:3, :3].T + T[:3, 3]
    fit, rmse, n, JTJ, JTr = _full_eval(pts, tgt, nrm, max_dist)
    iters = 0
    for _ in range(max_iter):
        iters += 1
        upd = np.eye(4)
        if n >= 6:
            try:
                x = np.linalg.solve(JTJ, -JTr)
                if np.all(np.isfinite(x)):
                    upd = lo._rot_xyz(x)
            except np.linalg.LinAlgError:
                pass
        T = upd @ T
        pts = pts @ upd[:3, :3].T + upd[:3, 3]
        bfit, brmse = fit, rmse
        fit, rmse, n, JTJ, JTr = _full_eval(pts, tgt, nrm, max_dist)
        if abs(bfit - fit) < lo.ICP_REL and abs(brmse - rmse) < lo.ICP_REL:
            break
    return T, fit, rmse, iters


def _cloud(kind):
    rng = np.random.default_rng({"surface": 1, "grid": 2, "dup": 3, "sparse": 4}[kind])
    if kind == "surface":        # a rippled bump as a depth sensor sees it: ~2.5 mm spacing, 1 m away, noise
        u, v = np.meshgrid(np.arange(-18, 18) * 0.0025, np.arange(-15, 15) * 0.0025)
        z = 1.0 - 0.03 * np.exp(-(u ** 2 + v ** 2) / 0.002) + 0.002 * np.sin(u * 300) * np.cos(v * 200)
        pts = np.stack([u.ravel(), v.ravel(), z.ravel()], 1) + rng.normal(0, 2e-4, (u.size, 3))
    elif kind == "grid":         # exact ties everywhere: integer millimetres on a 3-D lattice (many equidistant neighbours)
        g = np.mgrid[0:12, 0:10, 0:5].reshape(3, -1).T.astype(np.float64)
        pts = g * 0.002 + np.array([0.1, -0.05, 0.9])
    elif kind == "dup":          # duplicated points (d^2 = 0 ties) on a curved sheet
        u, v = np.meshgrid(np.arange(24) * 0.003, np.arange(20) * 0.003)
        base = np.stack([u.ravel(), v.ravel(), 0.8 + 2.0 * (u.ravel() - 0.03) ** 2 + 1.5 * (v.ravel() - 0.03) ** 2], 1)
        pts = np.concatenate([base, base[rng.choice(len(base), 150, replace=False)]], 0)
        pts = pts[rng.permutation(len(pts))]
    else:                        # a sparse cloud with far outliers (their neighbours are across the cloud)
        pts = rng.uniform(-0.05, 0.05, (300, 3)) + np.array([0, 0, 1.0])
        pts[:7] += rng.uniform(0.3, 0.6, (7, 3))
    return np.ascontiguousarray(pts)


CLOUDS = ["surface", "grid", "dup", "sparse"]


@pytest.mark.parametrize("kind", CLOUDS)
def test_neighbour_lists_and_normals_equal_the_full_matrix(kind):
    pts = _cloud(kind)
    assert len(pts) > lo._ROWS                                  # (more rows than one block: the blocks are exercised)
    want = _full_knn(pts, lo.KNN)
    for nn in ("brute", "kdtree"):
        got = lo.knn_lists(pts, nn=nn)
        assert np.array_equal(got, want), nn
    if kind in ("grid", "dup"):                                 # (the cloud really has ties at the k-th neighbour)
        d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
        kth = np.sort(d2, 1)[:, lo.KNN - 1:lo.KNN + 1]
        assert (kth[:, 0] == kth[:, 1]).any()
    nrm = _full_normals(pts)
    for nn in ("brute", "kdtree"):
        assert np.array_equal(lo.estimate_normals(pts, nn=nn), nrm), nn


@pytest.mark.parametrize("kind", CLOUDS)
def test_icp_modes_equal_the_full_matrix(kind):
    rng = np.random.default_rng(7)
    tgt = _cloud(kind)
    nrm = _full_normals(tgt)
    a = np.radians(1.5)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = tgt.mean(0)
    src = (tgt - c) @ Rz.T + c + np.array([0.002, -0.0015, 0.001])
    if kind == "grid":
        src = tgt + np.array([0.001, 0.0, 0.0])                 # half a lattice step: every source point ties between two targets
    src = src[rng.permutation(len(src))[: int(0.8 * len(src))]]
    init = np.eye(4)
    init[:3, 3] = rng.normal(0, 0.001, 3)
    T0, fit0, rmse0, it0 = _full_icp(src, tgt, nrm, init)
    for nn in ("brute", "kdtree"):
        hist = []
        T, fit, rmse, it = lo.icp_point_to_plane(src, tgt, nrm, init, nn=nn, history=hist)
        assert np.array_equal(T, T0) and fit == fit0 and rmse == rmse0 and it == it0, nn
        assert len(hist) == it + 1 and hist[-1]["fitness"] == fit and hist[-1]["rmse"] == rmse
    j_b, d_b = lo.nearest(src, tgt, "brute")
    j_k, d_k = lo.nearest(src, tgt, "kdtree")
    assert np.array_equal(j_b, j_k) and np.array_equal(d_b, d_k)


class _CountingTree:
    """A cKDTree that records the neighbour counts it is asked for."""

    def __init__(self, pts):
        from scipy.spatial import cKDTree
        self.tree, self.asked = cKDTree(pts), []

    def query(self, x, k):
        self.asked.append(k)
        return self.tree.query(x, k=k)


def test_kdtree_widens_past_a_cluster_of_ties():
    """More points tied with the k-th neighbour than the first query holds (2k + 8): a cluster of 121 duplicates.  Its first
    candidates are all at d^2 = 0, so their farthest is not beyond the k-th and the query must be widened; the neighbour
    lists, normals and nearest targets still equal the full matrix's."""
    rng = np.random.default_rng(11)
    base = _cloud("surface")
    pts = np.concatenate([base, np.repeat(base[200:201], 120, 0)], 0)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    dup = np.nonzero(np.all(pts == base[200], 1))[0]
    assert len(dup) == 121
    tree = _CountingTree(pts)
    got = lo._kd_take(tree, pts, pts[dup[0]], lo.KNN)
    assert tree.asked[0] == 2 * lo.KNN + 8 and max(tree.asked) > len(dup), tree.asked        # (widened until beyond the cluster)
    assert np.array_equal(got, _full_knn(pts, lo.KNN)[dup[0]])
    tree = _CountingTree(pts)
    assert lo._kd_take(tree, pts, pts[dup[5]], 1)[0] == dup[0] and max(tree.asked) > len(dup), tree.asked
    assert np.array_equal(lo.knn_lists(pts, nn="kdtree"), _full_knn(pts, lo.KNN))
    assert np.array_equal(lo.estimate_normals(pts, nn="kdtree"), _full_normals(pts))
    src = pts[dup[:10]] + np.array([1e-4, 0.0, 0.0])
    j_b, d_b = lo.nearest(src, pts, "brute")
    j_k, d_k = lo.nearest(src, pts, "kdtree")
    assert np.array_equal(j_b, j_k) and np.array_equal(d_b, d_k) and (j_k == dup[0]).all()


def test_pose_refine_kdtree_mode_is_bit_identical():
    import synth
    md = synth.synth_model_depth(5, 320, 240)
    sd = np.where(md > 0, md + 3, 0).astype(np.uint16)
    K = np.array([572.4114, 0, 160, 0, 573.57043, 120, 0, 0, 1], np.float32).reshape(3, 3)
    R, t = np.eye(3, dtype=np.float32), np.array([0, 0, 1000], np.float32)
    ys, xs = np.nonzero(md)
    a = lo.pose_refine(sd, md, K, K, R, t, int(xs.min()), int(ys.min()), scene_from_scene=True)
    b = lo.pose_refine(sd, md, K, K, R, t, int(xs.min()), int(ys.min()), scene_from_scene=True, nn="kdtree")
    assert np.array_equal(a["normals"], b["normals"]) and np.array_equal(a["T_icp"], b["T_icp"])
    assert a["iterations"] == b["iterations"] and a["residual"] == b["residual"] and a["history"] == b["history"]
    assert lo.ill_posed(a["history"]) == ""


def test_ill_posed_reads_the_oracles_evidence():
    ok = [{"fitness": 0.9, "rmse": 0.003, "eig_ratio": 1e-3}, {"fitness": 0.95, "rmse": 0.002, "eig_ratio": 1e-3}]
    assert lo.ill_posed(ok) == ""
    near = ok + [{"fitness": 0.95, "rmse": 0.002 - lo.ICP_REL - 1e-10, "eig_ratio": 1e-3}]
    assert "rmse" in lo.ill_posed(near)
    flat = ok[:1] + [{"fitness": 0.95, "rmse": 0.002, "eig_ratio": 1e-10}]
    assert "eigenvalue" in lo.ill_posed(flat)
