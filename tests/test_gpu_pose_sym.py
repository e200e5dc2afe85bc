"""GPU tests of the symmetry-aware pose errors on the device (lm_mesh_pose_errors_sym: MSSD, MSPD) against the numpy
restatement tests/pose_sym_ref.py, and of the chain errors -> match_poses -> recall.

Tolerance against the restatement: 1e-9 mm (MSSD) and 1e-9 px (MSPD), derived rather than measured: every quantity is f64
(unit roundoff 1.1e-16), coordinates are at most 2e3 mm, and a result is about 20 rounded operations deep, which bounds the
absolute error by about 20 * 2e3 * 1.1e-16 * (a small factor for the division by z >= 300) ~ 1e-11; 1e-9 leaves a factor of
100.  Which vertex or symmetry attains an extremum may differ between near-ties, the value may not differ beyond that.
Every test pose keeps all vertices at z >= 300 mm."""
import ctypes
import math
import os

import numpy as np
import pytest

import pose_sym_ref as psr
import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-9
K_CAM = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float64)
VERTEX_COUNTS = [1, 63, 64, 65, 255, 256, 257, 4097]                    # wave and chunk edges, more than one block
SYM_COUNTS = [1, 2, 24, 37, 315]                                         # 315 spans several LDS tiles (asserted)
LM_ERR_INVALID = -2


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "pose_error_golden.npz")))


@pytest.fixture(scope="module")
def ico5():
    return synth.icosphere(5, radius=80.0, seed=2)[0]                   # 10242 vertices


def rot(axis, deg):
    return psr.rodrigues(axis, math.radians(deg))


def poses(seed, n_est, n_gt):
    """GTs around z = 800 mm (objects are at most ~100 mm in radius: every vertex at z >= 300), estimates that are
    perturbations of the GTs, from a fraction of a degree to a wrong pose."""
    rng = np.random.default_rng(seed)
    gR = np.stack([rot(rng.normal(size=3), rng.uniform(0, 180)) for _ in range(n_gt)])
    gt = np.array([0.0, 0.0, 800.0]) + rng.uniform(-150, 150, (n_gt, 3))
    eR = np.stack([rot(rng.normal(size=3), [0.5, 8.0, 90.0][e % 3]) @ gR[e % n_gt] for e in range(n_est)])
    et = gt[np.arange(n_est) % n_gt] + rng.uniform(-1, 1, (n_est, 3)) * np.array([2.0, 15.0, 60.0])[np.arange(n_est) % 3, None]
    return eR, et, gR, gt


def sym_set(lm, count):
    """A symmetry set of exactly `count` transformations, generic enough that every entry gives another error."""
    if count == 1:
        return None
    if count == 2:
        return lm.symmetry_transforms([psr.as4x4(rot([0, 0, 1], 180.0), [1.0, -2.0, 0.5])])
    if count == 24:
        return lm.symmetry_transforms([psr.as4x4(R) for R in psr.cube_rotations()[1:]])
    rng = np.random.default_rng(count)
    if count == 37:
        return lm.symmetry_transforms([psr.as4x4(rot(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-5, 5, 3)) for _ in range(36)])
    axis, off = np.array([0.3, -0.2, 1.0]), np.array([4.0, 2.0, -6.0])    # the identity and count - 1 turns about an offset axis
    turns = [psr.rodrigues(axis, 2.0 * math.pi * i / count) for i in range(1, count)]
    return lm.symmetry_transforms([psr.as4x4(R, off - R @ off) for R in turns])


def mesh_of(lm, V):
    n = len(V)
    return lm.Mesh(np.ascontiguousarray(V, np.float32), np.array([[0, min(1, n - 1), min(2, n - 1)]], np.int32))


def check(lm, V, eR, et, gR, gt, syms):
    mesh = mesh_of(lm, V)
    got = lm.pose_errors(mesh, eR, et, gR, gt, K_CAM, metrics=("mssd", "mspd"), symmetries=syms)
    again = lm.pose_errors(mesh, eR, et, gR, gt, K_CAM, metrics=("mspd", "mssd"), symmetries=syms)
    one = {k: lm.pose_errors(mesh, eR, et, gR, gt, K_CAM, metrics=(k,), symmetries=syms)[k] for k in ("mssd", "mspd")}
    mesh.close()
    Rs, ts = (np.eye(3)[None], np.zeros((1, 3))) if syms is None else syms
    want = psr.errors(eR, et, gR, gt, K_CAM, V.astype(np.float64), Rs, ts)
    for k in ("mssd", "mspd"):
        assert got[k].shape == (len(eR), len(gR)) and got[k].dtype == np.float64
        d = np.abs(got[k] - want[k]).max()
        print("%s: nv %d, S %d, %dx%d: max |device - numpy| = %.3e (values up to %.1f)" % (k, len(V), len(Rs), len(eR), len(gR), d, want[k].max()))
        assert d <= TOL, (k, d)
        assert got[k].tobytes() == again[k].tobytes(), k                # two calls are bit-identical
        assert got[k].tobytes() == one[k].tobytes(), k                  # a metric alone equals the same metric of the joint pass
    return got


@pytest.mark.parametrize("nv", VERTEX_COUNTS)
def test_any_vertex_count(lm, ico5, nv):
    eR, et, gR, gt = poses(nv, 3, 2)
    check(lm, ico5[:nv], eR, et, gR, gt, sym_set(lm, 37))
    check(lm, ico5[:nv], eR, et, gR, gt, None)


@pytest.mark.parametrize("count", SYM_COUNTS)
def test_any_symmetry_count(lm, ico5, count):
    tile = lm.load_library().lm_pose_sym_tile()
    assert 37 < tile < 315 and 315 % tile != 0, "315 must span several LDS tiles with a partial last one, 37 must fit one"
    syms = sym_set(lm, count)
    assert (1 if syms is None else len(syms[0])) == count
    eR, et, gR, gt = poses(100 + count, 3, 2)
    check(lm, ico5[:257], eR, et, gR, gt, syms)


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (16, 1)])
def test_batch_shapes(lm, shape):
    V = synth.icosphere(2, radius=50.0, seed=3)[0]                      # 162 vertices
    eR, et, gR, gt = poses(7, *shape)
    check(lm, V, eR, et, gR, gt, sym_set(lm, 24))


def test_cube_symmetries(lm, gold):
    """An estimate equal to GT . S_k is a perfect estimate for the full set of the cube's rotations, and a bad one without."""
    V = gold["B_pts"]
    rots = psr.cube_rotations()
    syms = lm.symmetry_transforms([psr.as4x4(R) for R in rots[1:]])
    Rg, tg = gold["cgt_R"][0], gold["cgt_t"][0]
    eR = np.stack([Rg @ S for S in rots])
    et = np.repeat(tg[None], 24, 0)
    cube = lm.Mesh(V, gold["B_faces"])
    full = lm.pose_errors(cube, eR, et, Rg, tg, K_CAM, metrics=("mssd", "mspd"), symmetries=syms)
    ident = lm.pose_errors(cube, eR, et, Rg, tg, K_CAM, metrics=("mssd", "mspd"))
    cube.close()
    assert full["mssd"].shape == (24, 1)
    assert full["mssd"].max() < 1e-9 and full["mspd"].max() < 1e-9
    assert ident["mssd"][0, 0] < 1e-9 and ident["mssd"][1:].min() > 10.0
    assert ident["mspd"][1:].min() > 1.0


def test_bounds_without_symmetries(lm, ico5):
    """S = 1: the largest vertex distance is at least their mean (ADD) and at most ||R_e - R_g||_2 max|v| + |t_e - t_g|; the
    largest pixel distance is at most the diagonal of the box that holds both projections of the vertices (project_pts)."""
    V = ico5[:4097]
    V64 = V.astype(np.float64)
    eR, et, gR, gt = poses(11, 3, 2)
    mesh = mesh_of(lm, V)
    r = lm.pose_errors(mesh, eR, et, gR, gt, K_CAM, metrics=("add", "mssd", "mspd"))
    mesh.close()
    rmax = np.linalg.norm(V64, axis=1).max()
    for e in range(3):
        for g in range(2):
            assert r["add"][e, g] <= r["mssd"][e, g] + TOL
            assert r["mssd"][e, g] <= np.linalg.norm(eR[e] - gR[g], 2) * rmax + np.linalg.norm(et[e] - gt[g]) + TOL
            both = np.concatenate([psr.project(K_CAM, psr.transform(eR[e], et[e], V64)), psr.project(K_CAM, psr.transform(gR[g], gt[g], V64))])
            assert r["mspd"][e, g] <= np.linalg.norm(both.max(0) - both.min(0)) + TOL
    assert r["mssd"].min() > 0.1 and r["mspd"].min() > 0.1


@pytest.mark.parametrize("max_step", [0.3, 0.01])
def test_continuous_symmetry_discretisation_bound(lm, max_step):
    """An estimate turned about the model's z axis by theta, scored with the continuous z symmetry.  The set samples the turns
    i * step, step = 2 pi / n, i = 1 .. n-1 (not 0), so for theta in [step, 2 pi - step] a sample lies within step / 2 of it.
    The residual turn delta <= step / 2 moves a vertex at distance r from the axis by the chord 2 r sin(delta / 2)
    <= 2 r_max sin(step / 4).  The axis passes through the inside of the blob, so r_max <= diameter cos(step / 4), and with
    sin(step / 2) = 2 sin(step / 4) cos(step / 4) the chord is at most diameter * sin(step / 2)."""
    V = synth.icosphere(3, radius=55.0, seed=1)[0]
    V64 = V.astype(np.float64)
    syms = lm.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_sym_disc_step=max_step)
    n = psr.disc_count(max_step)
    step = 2 * math.pi / n
    assert len(syms[0]) == n - 1
    Rg, tg = rot([0.4, 1.0, -0.3], 65.0), np.array([40.0, -30.0, 700.0])
    thetas = [step, 1.5 * step, 1.2345, math.pi, 2 * math.pi - 1.5 * step]
    eR = np.stack([Rg @ psr.rodrigues([0, 0, 1], th) for th in thetas])
    et = np.repeat(tg[None], len(thetas), 0)
    mesh = mesh_of(lm, V)
    diameter = mesh.diameter()
    got = lm.pose_errors(mesh, eR, et, Rg, tg, metrics=("mssd",), symmetries=syms)["mssd"][:, 0]
    plain = lm.pose_errors(mesh, eR, et, Rg, tg, metrics=("mssd",))["mssd"][:, 0]
    mesh.close()
    chord = 2.0 * np.linalg.norm(V64[:, :2], axis=1).max() * math.sin(step / 4.0)
    bound = diameter * math.sin(step / 2.0)
    assert chord <= bound
    assert got.max() <= chord + TOL and got.max() <= bound, (got, chord, bound)
    assert got[0] <= TOL                                                # theta is a sample itself
    assert got[1] > 0.25 * chord                                         # halfway between two samples
    assert plain[3] > 50.0                                               # half a turn without the symmetry: a wrong pose


def test_old_metrics_are_untouched_by_the_new_ones(lm, gold):
    V, F, K, scene = gold["A_pts"], gold["A_faces"], gold["K"], gold["scene"]
    old = ("vsd", "cou", "add", "adi", "re", "te")
    mesh = lm.Mesh(V, F)
    a = lm.pose_errors(mesh, gold["est_R"], gold["est_t"], gold["gt_R"], gold["gt_t"], K, scene)
    b = lm.pose_errors(mesh, gold["est_R"], gold["est_t"], gold["gt_R"], gold["gt_t"], K, scene, metrics=old + ("mssd", "mspd"),
                       symmetries=sym_set(lm, 24))
    mesh.close()
    assert sorted(a) == sorted(old) and sorted(b) == sorted(old + ("mssd", "mspd"))
    for k in old:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert b["mssd"].shape == a["add"].shape == (6, 3)


def test_error_cases(lm, gold):
    lib = lm.load_library()
    mesh = lm.Mesh(gold["B_pts"], gold["B_faces"])
    R, t = np.ascontiguousarray(np.eye(3).reshape(1, 9)), np.array([[0.0, 0.0, 800.0]])
    K = np.ascontiguousarray(K_CAM.reshape(9))
    out = np.zeros(4)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.lm_last_error.restype = ctypes.c_char_p
    for bits in (64, 128, 4 | 64):
        rc = lib.lm_mesh_pose_errors(mesh._h, 1, p(R), p(t), 1, p(R), p(t), p(K), 640, 480, None, bits, 15.0, 20.0, 0, 100.0, 10000.0, p(out))
        assert rc == LM_ERR_INVALID and b"lm_mesh_pose_errors_sym" in lib.lm_last_error()
    sym = lambda n_sym, Kp, bits: lib.lm_mesh_pose_errors_sym(mesh._h, 1, p(R), p(t), 1, p(R), p(t), n_sym, p(R), p(np.zeros((1, 3))), Kp, bits, p(out))  # noqa: E731
    assert sym(1, p(K), 64 | 128) == 0 and out[0] == 0.0 and out[1] == 0.0
    assert sym(0, p(K), 64) == LM_ERR_INVALID
    assert sym(-1, p(K), 64) == LM_ERR_INVALID
    assert sym(1, None, 128) == LM_ERR_INVALID
    assert sym(1, None, 64 | 128) == LM_ERR_INVALID
    assert sym(1, None, 64) == 0                                         # MSSD needs no K
    assert sym(1, p(K), 0) == LM_ERR_INVALID and sym(1, p(K), 4) == LM_ERR_INVALID
    with pytest.raises(RuntimeError, match="K"):
        lm.pose_errors(mesh, R.reshape(3, 3), t[0], R.reshape(3, 3), t[0], metrics=("mspd",))
    with pytest.raises(RuntimeError):
        lm.pose_errors(mesh, R.reshape(3, 3), t[0], R.reshape(3, 3), t[0], metrics=("mssd",), symmetries=(np.zeros((0, 3, 3)), np.zeros((0, 3))))
    with pytest.raises(ValueError):
        lm.pose_errors(mesh, R.reshape(3, 3), t[0], R.reshape(3, 3), t[0], metrics=("mssd",), symmetries=(np.eye(3), np.zeros(3)))
    with pytest.raises(ValueError, match="unknown metric"):
        lm.pose_errors(mesh, R.reshape(3, 3), t[0], R.reshape(3, 3), t[0], metrics=("msd",))
    r = lm.pose_errors(mesh, np.zeros((0, 3, 3)), np.zeros((0, 3)), R.reshape(3, 3), t[0], K_CAM, metrics=("mssd", "mspd"))
    assert r["mssd"].shape == (0, 1) and r["mspd"].shape == (0, 1)
    mesh.close()


def test_errors_to_recall_on_a_three_instance_scene(lm):
    """Three instances, three estimates with the GT's rotation, so that an estimate moved by d along the camera's x has
    MSSD = d exactly and MSPD = max_v fx d / z_v.  Estimate 0: 1 mm off (found at every threshold).  Estimate 1: 0.22 diameters
    off, i.e. found at the MSSD thresholds 0.25 .. 0.50 (6 of 10) and at the MSPD thresholds above fx d / z_min.  Estimate 2:
    one whole diameter off, beyond the largest thresholds (0.5 diameters; 50 px).  The instances are far apart, so an
    estimate can only match its own.  MSSD recall = (10 + 6 + 0) / (3 * 10)."""
    V = synth.icosphere(2, radius=50.0, seed=3)[0]
    V64 = V.astype(np.float64)
    mesh = mesh_of(lm, V)
    diameter = mesh.diameter()
    gR = np.stack([rot([0.3, 1.0, 0.2], 35.0), rot([1.0, 0.2, 0.1], 120.0), rot([0.0, 0.4, 1.0], -70.0)])
    gt = np.array([[10.0, 5.0, 800.0], [-300.0, 20.0, 900.0], [250.0, -120.0, 950.0]])
    d = np.array([1.0, 0.22 * diameter, diameter])
    et = gt + np.stack([d, np.zeros(3), np.zeros(3)], 1)
    errs = lm.pose_errors(mesh, gR, et, gR, gt, K_CAM, metrics=("mssd", "mspd"))
    mesh.close()
    assert np.abs(np.diag(errs["mssd"]) - d).max() <= TOL
    th_ssd, th_spd = lm.bop19_thresholds(diameter, 640)
    scores = [0.5, 0.9, 0.7]
    m = lm.match_poses(errs["mssd"], scores, th_ssd[-1])
    assert [(x["est_id"], x["gt_id"]) for x in m] == [(1, 1), (0, 0)]
    # per threshold: 1 of 3 found at the four thresholds below 0.22 diameters, 2 of 3 at the six above
    assert lm.recall([errs["mssd"]], [scores], th_ssd) == np.mean([1 / 3.0] * 4 + [2 / 3.0] * 6)
    assert abs(lm.recall([errs["mssd"]], [scores], th_ssd) - (10 + 6 + 0) / 30.0) <= 1e-15
    # MSPD: the pixel shift of a vertex is fx d / z_v, the largest at the nearest vertex
    found = 0
    for g in range(3):
        z = psr.transform(gR[g], gt[g], V64)[:, 2]
        lo, hi = K_CAM[0, 0] * d[g] / z.max(), K_CAM[0, 0] * d[g] / z.min()
        assert lo - TOL <= errs["mspd"][g, g] <= hi + TOL
        assert abs(errs["mspd"][g, g] - hi) <= TOL
        assert all(abs(th - hi) > 1e-6 for th in th_spd), "a threshold at the largest shift: the count would not be by hand"
        found += sum(th > hi for th in th_spd)
    assert found == 10 + 7 + 0                                            # 1 mm: < 5 px; 0.22 d: between 15 and 20 px; d: > 50 px
    assert abs(lm.recall([errs["mspd"]], [scores], th_spd) - found / 30.0) <= 1e-15
    # an image without estimates halves the recall
    assert abs(lm.recall([errs["mssd"], np.zeros((0, 3))], [scores, []], th_ssd) - 16 / 60.0) <= 1e-15
