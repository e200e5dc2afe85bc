"""GPU tests of the pose errors on the device (lm_mesh_pose_errors / lm_mesh_gt_stats / lm_mesh_diameter) against pysixd's own
numbers recorded in tests/golden/pose_error_golden.npz and against the numpy restatement (tests/pose_error_ref.py) fed with the
rasteriser's numpy twin (oracle/render_oracle.py)."""
import math
import os

import numpy as np
import pytest

import pose_error_ref as per
import render_oracle as ro
import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = ("vsd", "cou", "add", "adi", "re", "te")
K_CAM = np.array([572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1], np.float32).reshape(3, 3)


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


def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def oracle_depth(V, F, K, R, t, W, H, near=100.0, far=10000.0):
    """What lm_mesh_pose_errors renders: float32 eye depth of the rasteriser with R, t, K cast to float32, background 0."""
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    z, tri = ro.rasterise(V, F, f32(K), f32(R), f32(t).ravel(), W, H, near, far)
    return np.where(tri >= 0, z, 0).astype(np.float32)


def restate(V, F, K, scene, eR, et, gR, gt, W, H, delta=15.0, tau=20.0):
    ed = [oracle_depth(V, F, K, R, t, W, H) for R, t in zip(eR, et)]
    gd = [oracle_depth(V, F, K, R, t, W, H) for R, t in zip(gR, gt)]
    out = {k: np.zeros((len(eR), len(gR))) for k in ("vsd", "vsd_tlinear", "cou", "add", "adi", "re", "te")}
    for e in range(len(eR)):
        for g in range(len(gR)):
            if scene is not None:
                out["vsd"][e, g] = per.vsd(ed[e], gd[g], scene, K, delta, tau, "step")
                out["vsd_tlinear"][e, g] = per.vsd(ed[e], gd[g], scene, K, delta, tau, "tlinear")
            out["cou"][e, g] = per.cou(ed[e], gd[g])
            out["add"][e, g] = per.add(eR[e], et[e], gR[g], gt[g], V)
            out["adi"][e, g] = per.adi(eR[e], et[e], gR[g], gt[g], V)
            out["re"][e, g] = per.re(eR[e], gR[g])
            out["te"][e, g] = per.te(et[e], gt[g])
    return out


def assert_criteria(got, want, vsd=True):
    """The parity bar: step VSD and COU exact, tlinear VSD 1e-12, ADD / ADI 1e-4 mm, TE 1e-9 mm, RE 1e-5 deg."""
    if vsd:
        assert np.array_equal(got["vsd"], want["vsd"]), (got["vsd"], want["vsd"])
        if "vsd_tlinear" in got:
            assert np.allclose(got["vsd_tlinear"], want["vsd_tlinear"], rtol=0, atol=1e-12)
    assert np.array_equal(got["cou"], want["cou"]), (got["cou"], want["cou"])
    for k, tol in (("add", 1e-4), ("adi", 1e-4), ("te", 1e-9), ("re", 1e-5)):
        d = np.abs(got[k] - want[k]).max() if got[k].size else 0.0
        assert d <= tol, (k, d)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_device_equals_recorded_pysixd_and_restatement(lm, gold, tag):
    V, F = gold[tag + "_pts"], gold[tag + "_faces"]
    eR, et = (gold["est_R"], gold["est_t"]) if tag == "A" else (gold["cest_R"], gold["cest_t"])
    gR, gt = (gold["gt_R"], gold["gt_t"]) if tag == "A" else (gold["cgt_R"], gold["cgt_t"])
    K, scene = gold["K"], gold["scene"]
    mesh = lm.Mesh(V, F)
    got = lm.pose_errors(mesh, eR, et, gR, gt, K, scene)
    got["vsd_tlinear"] = lm.pose_errors(mesh, eR, et, gR, gt, K, scene, metrics=("vsd",), cost="tlinear")["vsd"]
    rec = {k: gold["%s_%s" % (tag, k)] for k in ("vsd_tlinear", "cou", "add", "adi", "re", "te")}
    rec["vsd"] = gold[tag + "_vsd_step"]
    assert_criteria(got, rec)
    H, W = scene.shape
    assert_criteria(got, restate(V, F, K, scene, eR, et, gR, gt, W, H))
    # the counts behind the errors: restatement on the device's own render rules
    ed = [oracle_depth(V, F, K, R, t, W, H) for R, t in zip(eR, et)]
    gd = [oracle_depth(V, F, K, R, t, W, H) for R, t in zip(gR, gt)]
    for e in range(len(eR)):
        for g in range(len(gR)):
            c = per.vsd_counts(ed[e], gd[g], scene, K, 15.0, 20.0)
            want = (c["step"] + c["union"] - c["inter"]) / float(c["union"]) if c["union"] else 1.0
            assert got["vsd"][e, g] == want
    mesh.close()


def test_gt_stats_equal_recorded(lm, gold):
    mesh = lm.Mesh(gold["A_pts"], gold["A_faces"])
    st = lm.gt_stats(mesh, gold["gt_R"], gold["gt_t"], gold["K"], gold["scene"])
    for g, s in enumerate(st):
        row = [s["px_count_all"], s["px_count_valid"], s["px_count_visib"]] + s["bbox_obj"] + s["bbox_visib"]
        assert row == gold["gts_int"][g].tolist(), (g, row)
        assert s["visib_fract"] == gold["gts_visib_fract"][g]
    # uint16 scene depth is converted exactly
    st16 = lm.gt_stats(mesh, gold["gt_R"], gold["gt_t"], gold["K"], gold["scene"].astype(np.uint16))
    assert st16 == st
    mesh.close()


def random_poses(rng, n, around_t, spread_deg, spread_mm):
    R = np.stack([rot(rng.normal(size=3), rng.uniform(0, spread_deg)) for _ in range(n)])
    t = np.asarray(around_t, np.float64) + rng.uniform(-spread_mm, spread_mm, (n, 3))
    return R, t


def test_batch_16_by_3_and_repeatability(lm, gold):
    V, F, K, scene = gold["A_pts"], gold["A_faces"], gold["K"], gold["scene"]
    rng = np.random.default_rng(5)
    gR, gt = gold["gt_R"], gold["gt_t"]
    eR = np.concatenate([rot([0.2, 1, 0], d)[None] @ gR[i % 3] for i, d in enumerate(np.linspace(0, 40, 16))])
    et = gt[np.arange(16) % 3] + rng.uniform(-30, 30, (16, 3))
    mesh = lm.Mesh(V, F)
    a = lm.pose_errors(mesh, eR, et, gR, gt, K, scene)
    b = lm.pose_errors(mesh, eR, et, gR, gt, K, scene)
    for k in ALL:
        assert a[k].shape == (16, 3) and a[k].dtype == np.float64
        assert a[k].tobytes() == b[k].tobytes(), k                      # bit-identical
    H, W = scene.shape
    assert_criteria(a, restate(V, F, K, scene, eR, et, gR, gt, W, H))
    # a subset of metrics lands in the same place; cou needs no scene, only the image size
    c = lm.pose_errors(mesh, eR, et, gR, gt, K, None, metrics=("te", "cou", "adi"), im_size=(W, H))
    assert sorted(c) == ["adi", "cou", "te"]
    for k in c:
        assert c[k].tobytes() == a[k].tobytes(), k
    mesh.close()


def test_empty_batches_and_missing_scene(lm, gold):
    mesh = lm.Mesh(gold["A_pts"], gold["A_faces"])
    K, scene = gold["K"], gold["scene"]
    r = lm.pose_errors(mesh, np.zeros((0, 3, 3)), np.zeros((0, 3)), gold["gt_R"], gold["gt_t"], K, scene)
    assert all(r[k].shape == (0, 3) for k in ALL)
    r = lm.pose_errors(mesh, gold["est_R"], gold["est_t"], np.zeros((0, 3, 3)), np.zeros((0, 3)), K, scene)
    assert all(r[k].shape == (6, 0) for k in ALL)
    with pytest.raises(RuntimeError, match="scene"):
        lm.pose_errors(mesh, gold["est_R"], gold["est_t"], gold["gt_R"], gold["gt_t"], K, None)
    with pytest.raises(ValueError):
        lm.gt_stats(mesh, gold["gt_R"], gold["gt_t"], K, None)
    # a single pose is a batch of one
    r = lm.pose_errors(mesh, gold["est_R"][1], gold["est_t"][1], gold["gt_R"][0], gold["gt_t"][0], K, scene)
    assert r["vsd"].shape == (1, 1) and r["vsd"][0, 0] == gold["A_vsd_step"][1, 0]
    mesh.close()


@pytest.mark.parametrize("nv", [1, 63, 64, 4097, 20011, "ico5"])
def test_point_metrics_any_vertex_count(lm, nv):
    rng = np.random.default_rng(7)
    if nv == "ico5":
        V, F, _, _ = synth.icosphere(5, radius=80.0, seed=2)           # 10242 vertices, a subdivided mesh
    else:
        V = (rng.normal(size=(nv, 3)) * [60.0, 40.0, 25.0]).astype(np.float32)
        F = np.array([[0, min(1, nv - 1), min(2, nv - 1)]], np.int32)
    mesh = lm.Mesh(V, F)
    gR, gt = random_poses(rng, 2, [0, 0, 900], 180, 100)
    eR = np.concatenate([rot(rng.normal(size=3), 3.0)[None] @ gR[0][None], rot(rng.normal(size=3), 60.0)[None] @ gR[1][None], gR[:1]])
    et = np.concatenate([gt[:1] + [2.0, -1.0, 3.0], gt[1:] + [30.0, 10.0, -40.0], gt[:1]])
    got = lm.pose_errors(mesh, eR, et, gR, gt, metrics=("add", "adi", "re", "te"))
    V64 = V.astype(np.float64)
    for e in range(3):
        for g in range(2):
            assert abs(got["add"][e, g] - per.add(eR[e], et[e], gR[g], gt[g], V64)) <= 1e-4
            assert abs(got["adi"][e, g] - per.adi(eR[e], et[e], gR[g], gt[g], V64)) <= 1e-4
            assert abs(got["re"][e, g] - per.re(eR[e], gR[g])) <= 1e-5
            assert abs(got["te"][e, g] - per.te(et[e], gt[g])) <= 1e-9
    assert got["add"][2, 0] == 0.0 and got["adi"][2, 0] == 0.0
    if nv != 20011:                                                      # the brute-force numpy diameter is O(n^2)
        assert abs(mesh.diameter() - per.diameter(V64)) <= 1e-4
    mesh.close()


def test_diameter_of_the_bumpy_icosphere(lm):
    V, F, _, _ = synth.icosphere(3, radius=55.0, seed=1)
    mesh = lm.Mesh(V, F)
    d = mesh.diameter()
    assert abs(d - per.diameter(V)) <= 1e-4
    assert mesh.diameter() == d
    mesh.close()


def test_invariances(lm, gold):
    K, scene = gold["K"], gold["scene"]
    mesh = lm.Mesh(gold["A_pts"], gold["A_faces"])
    gR, gt = gold["gt_R"], gold["gt_t"]
    r = lm.pose_errors(mesh, gR, gt, gR, gt, K, scene)
    d = np.arange(3)
    for k in ("add", "adi", "te", "cou"):
        assert np.all(r[k][d, d] == 0.0), k
    assert np.all(r["re"][d, d] <= 1e-5)
    # VSD of a pose against itself is 0 only where something is visible (GT 2 is fully occluded: 1.0)
    assert r["vsd"][0, 0] == 0.0 and r["vsd"][1, 1] == 0.0 and r["vsd"][2, 2] == 1.0
    mesh.close()
    # the exactly symmetric cube: a rotation mapping its vertex set to itself leaves ADI at 0, not ADD
    cube = lm.Mesh(gold["B_pts"], gold["B_faces"])
    R0, t0 = gold["cgt_R"][0], gold["cgt_t"][0]
    for S in (rot([0, 0, 1], 90.0), rot([1, 0, 0], 180.0), rot([1, 1, 1], 120.0)):
        r = lm.pose_errors(cube, R0 @ S, t0, R0, t0, metrics=("add", "adi"))
        assert r["adi"][0, 0] <= 1e-9 and r["add"][0, 0] > 10.0
    assert abs(cube.diameter() - 80.0 * math.sqrt(3.0)) <= 1e-4
    cube.close()


def test_pipeline_pose_of_a_planted_view_passes_sixd_criteria(lm):
    """End to end: a scene rendered at a training view, match + NMS + ICP on the device, then the errors of the top detection."""
    import linemod_oracle  # noqa: F401  (oracle/ on the path, as the other GPU tests)
    import views
    W, H = 640, 480
    V, F, N, C = synth.icosphere(2, radius=60.0, seed=13)
    C[:] = (C // 64) * 64 + 30
    mesh = lm.Mesh(V, F, normals=N, colors=C)
    vs, _ = views.sample_views(42, 600.0, tilt_step=0.7 * np.pi)
    idx = np.random.default_rng(3).choice(len(vs), 8, replace=False)
    Rs = np.stack([vs[i]["R"] for i in idx]).astype(np.float32)
    ts = np.stack([vs[i]["t"].ravel() for i in idx]).astype(np.float32)
    R_gt, t_gt = Rs[2].astype(np.float64), ts[2].astype(np.float64)
    rgb_o, dep_o = mesh.render((W, H), K_CAM, Rs[2:3], ts[2:3])
    rgb, dep = synth.make_frame(17, W, H)
    obj = dep_o[0] > 0
    rgb[obj], dep[obj] = rgb_o[0][obj], dep_o[0][obj]
    det = lm.Detector(63, [4, 8], device=0)
    ids, wh = lm.add_templates_rendered(det, mesh, "obj", (W, H), K_CAM, Rs, ts)
    assert ids[2] >= 0
    pipe = lm.Pipeline(det, W, H, scene_from_scene=True)
    pipe.set_views_rendered("obj", mesh, K_CAM, Rs, ts, box_wh=wh)
    det.setFrame([rgb, dep])
    res, _ = pipe.run(70.0, ["obj"], K_CAM, top_k=4)
    pipe.close()
    assert len(res) > 0 and res[0]["status"] == 0, res[:1]
    R_e, t_e = np.asarray(res[0]["R"], np.float64), np.asarray(res[0]["t"], np.float64).ravel()
    got = lm.pose_errors(mesh, R_e, t_e, R_gt, t_gt, K_CAM, dep)
    want = restate(V, F, K_CAM.astype(np.float64), dep.astype(np.float32), R_e[None], t_e[None], R_gt[None], t_gt[None], W, H)
    assert_criteria(got, want)
    diam = mesh.diameter()
    print("planted view: template %d, adi %.3f mm (diameter %.1f), vsd %.4f, add %.3f, re %.3f deg, te %.3f mm"
          % (res[0]["template_id"], got["adi"][0, 0], diam, got["vsd"][0, 0], got["add"][0, 0], got["re"][0, 0], got["te"][0, 0]))
    assert got["adi"][0, 0] < 0.1 * diam
    assert got["vsd"][0, 0] < 0.3
    mesh.close()
