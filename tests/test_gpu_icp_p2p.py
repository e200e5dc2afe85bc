"""Point-to-point estimation, the convergence criteria and evaluate-only (max_iteration = 0) of poseRefine on the device against the
numpy restatement tests/icp_p2p_ref.py (point-to-point; UNPINNED, see there) and the oracle's icp_point_to_plane (criteria).

Bar, per hypothesis, the one tests/test_gpu_icp_oracle.py applies to the point-to-plane path: equal iterations, n_source and n_target,
|residual - reference| < 1e-6, R entries within 1e-4, t within 1e-4 m; and |inlier RMSE - reference| < 1e-6 (the tolerance of the
fitness: both are what the convergence test compares at 1e-6; the float the result carries rounds an RMSE <= 0.01 m by < 1e-9).
Every compared run is well-posed by the restatement's own evidence (tests/test_icp_p2p_ref.py asserts that on the CPU), so nothing
is exempt.  The cases (tests/icp_p2p_ref.py: cases): a cloud of a few hundred points, one of ~19k (64 slices of ~295 points: more than a
workgroup's 256 threads), a batch of three with a window out of frame and a hypothesis without correspondences, and the two verbatim
regimes of SURVEY C.6."""
import numpy as np
import pytest

import icp_p2p_ref as ref
from helpers import K_CAM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import os
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def run(lm, case, sfs, **kw):
    Ks, Rs, ts, xy = case.arrays()
    res, _ = lm.pose_refine_batch(case.scene, K_CAM, case.mds, Ks, Rs, ts, xy, device=0, scene_from_scene=sfs, **kw)
    return res


def kwargs(estimation, max_iter, rel):
    return dict(estimation=estimation, max_iteration=max_iter, relative_fitness=rel, relative_rmse=rel)


def compare(case, sfs, got, estimation, max_iter, rel, label):
    """Every hypothesis of a run against the restatement (the bar in the module docstring); returns the largest differences seen."""
    worst = {"R": 0.0, "t_m": 0.0, "fitness": 0.0, "rmse": 0.0}
    assert len(got) == len(case.mds)
    for i, g in enumerate(got):
        r = ref.reference(case, sfs, i, estimation, max_iter, rel)
        ctx = "%s / %s" % (label, case.names[i])
        if r["residual"] == -1.0:                                   # the window leaves the frame (LL.cpp:52-55): nothing touched
            assert g["residual"] == -1.0 and g["stage"] == 0 and g["iterations"] == 0 and not np.any(g["R"]) and not np.any(g["t"]), (ctx, g)
            continue
        d = {"R": float(np.abs(g["R"] - r["R"]).max()), "t_m": float(np.abs(g["t"] - r["t"]).max() / 1000.0),
             "fitness": abs(g["residual"] - r["residual"]), "rmse": abs(g["rmse"] - r["rmse"])}
        print("%-40s it %2d / %2d  stage %d  n %d/%d  dR %.2e dt %.2e m dfit %.2e drmse %.2e" % (
            ctx, g["iterations"], r["iterations"], g["stage"], g["n_source"], g["n_target"], d["R"], d["t_m"], d["fitness"], d["rmse"]))
        assert g["n_source"] == r["n_source"] and g["n_target"] == r["n_target"], (ctx, r["n_source"], r["n_target"])
        assert g["iterations"] == r["iterations"], (ctx, g["iterations"], r["iterations"])
        assert d["fitness"] < 1e-6 and d["rmse"] < 1e-6, (ctx, d)
        assert d["R"] < 1e-4 and d["t_m"] < 1e-4, (ctx, d)
        for k in worst:
            worst[k] = max(worst[k], d[k])
    return worst


SIZES = ("small", "large", "batch3")


# ---- 1: the estimator itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SIZES)
def test_one_point_to_point_update(lm, name):
    """max_iteration = 1: the pose after one point-to-point update is the restatement's; one point-to-plane update from the same
    inputs is another pose."""
    case, sfs = ref.cases()[name]
    got = run(lm, case, sfs, **kwargs("point_to_point", 1, ref.ICP_REL))
    compare(case, sfs, got, "point_to_point", 1, ref.ICP_REL, "%s, one point-to-point update" % name)
    plane = run(lm, case, sfs, estimation="point_to_plane", max_iteration=1)
    i = 0                                                           # (the ordinary hypothesis of every case)
    r = ref.reference(case, sfs, i, "point_to_point", 1, ref.ICP_REL)
    assert got[i]["iterations"] == plane[i]["iterations"] == 1 and got[i]["stage"] == plane[i]["stage"] == 3
    assert max(np.abs(plane[i]["R"] - r["R"]).max(), np.abs(plane[i]["t"] - r["t"]).max() / 1000.0) > 1e-6


# ---- 2: full runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SIZES + ("verbatim_near", "verbatim_far"))
def test_point_to_point_full_run(lm, name):
    case, sfs = ref.cases()[name]
    got = run(lm, case, sfs, estimation="point_to_point")
    worst = compare(case, sfs, got, "point_to_point", 30, ref.ICP_REL, "%s, point-to-point" % name)
    print("largest differences:", worst)
    assert all(g["stage"] == 3 for g in got if g["residual"] != -1.0)
    if name == "batch3":                                            # no correspondences: T = init guess, fitness 0
        g, r = got[2], ref.reference(case, sfs, 2, "point_to_point", 30, ref.ICP_REL)
        assert case.names[2] == "no correspondences" and g["residual"] == 0.0 and g["rmse"] == 0.0 and g["iterations"] == r["iterations"]
    if name == "verbatim_near":
        assert got[0]["residual"] == 1.0
    if name == "verbatim_far":
        assert got[0]["residual"] == 0.0


def test_point_to_point_on_the_other_entry_points(lm):
    """poseRefine.process and IcpContext.run give what pose_refine_batch gives (one kernel path, three doors); the build that finished
    the hypothesis is the sliced launches' (IcpState.build 0)."""
    from helpers import DBG3_BUILD
    case, sfs = ref.cases()["small"]
    want = run(lm, case, sfs, estimation="point_to_point")[0]
    pr = lm.poseRefine(device=0, scene_from_scene=sfs, estimation="point_to_point")
    pr.process(case.scene, case.mds[0], K_CAM, case.Ks[0], case.Rs[0], case.ts[0], case.xy[0][0], case.xy[0][1])
    assert np.array_equal(pr.getR(), want["R"]) and np.array_equal(pr.getT().ravel(), want["t"]) and pr.info["stage"] == 3
    Ks, Rs, ts, xy = case.arrays()
    ctx = lm.IcpContext(device=0, scene_from_scene=sfs, estimation="point_to_point")
    try:
        ctx.set_scene(case.scene, K_CAM)
        ctx.set_models(case.mds)
        res, _ = ctx.run(Ks, Rs, ts, xy)
        assert np.array_equal(res[0]["R"], want["R"]) and np.array_equal(res[0]["t"], want["t"]) and res[0]["iterations"] == want["iterations"]
        assert int(ctx.read_debug(0, 3)[DBG3_BUILD]) == 0
    finally:
        ctx.close()
    # the criteria on a poseRefine object (a context of its own): evaluate-only leaves the guess alone
    pr0 = lm.poseRefine(device=0, scene_from_scene=sfs, max_iteration=0)
    pr0.process(case.scene, case.mds[0], K_CAM, case.Ks[0], case.Rs[0], case.ts[0], case.xy[0][0], case.xy[0][1])
    e = run(lm, case, sfs, max_iteration=0)[0]
    assert pr0.info["iterations"] == 0 and np.array_equal(pr0.getR(), e["R"]) and np.array_equal(pr0.getT().ravel(), e["t"])
    assert pr0.getResidual() == e["residual"]


# ---- 3: evaluate-only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimation", ["point_to_point", "point_to_plane"])
@pytest.mark.parametrize("name", SIZES)
def test_max_iteration_0_is_evaluate_registration(lm, name, estimation):
    case, sfs = ref.cases()[name]
    Ks, Rs, ts, xy = case.arrays()
    ctx = lm.IcpContext(device=0, scene_from_scene=sfs, estimation=estimation, max_iteration=0)
    try:
        ctx.set_scene(case.scene, K_CAM)
        ctx.set_models(case.mds)
        got, _ = ctx.run(Ks, Rs, ts, xy)
        dbg = [ctx.read_debug(h, 3) for h in range(len(got))]
    finally:
        ctx.close()
    compare(case, sfs, got, estimation, 0, ref.ICP_REL, "%s, %s, evaluate-only" % (name, estimation))
    fit, rmse = lm.evaluate_registration(case.scene, K_CAM, case.mds, Ks, Rs, ts, xy, device=0, scene_from_scene=sfs)
    for i, (g, d) in enumerate(zip(got, dbg)):
        assert fit[i] == g["residual"]
        if g["residual"] == -1.0:
            continue
        assert rmse[i] == g["rmse"] and g["iterations"] == 0 and g["stage"] == 3
        # transformation_ = init_guess, exactly: the identity with the device's own centroid translation ...
        init, T = d[0:3], d[3:19].reshape(4, 4)
        want = np.eye(4)
        want[:3, 3] = init
        assert np.array_equal(T, want), (case.names[i], T)
        # ... which is the restatement's up to the order of two sums of <= 2 * 10^4 terms of magnitude <= 2 (bound 2e4 * 2 * 2^-53 < 1e-11)
        r = ref.reference(case, sfs, i, estimation, 0, ref.ICP_REL)
        assert np.abs(init - r["init_guess"][:3, 3]).max() < 1e-9
        # ... and the pose returned is init_guess * init_base, exactly (the product of lm_icp_compose_result, term by term)
        base = ref.init_base(case.Rs[i], case.ts[i])
        M = np.zeros((4, 4))
        for a in range(4):
            for b in range(4):
                v = 0.0
                for k in range(4):
                    v += want[a, k] * base[k, b]
                M[a, b] = v
        assert np.array_equal(g["R"], M[:3, :3]) and np.array_equal(g["t"], M[:3, 3] * 1000.0), case.names[i]


# ---- 4: the criteria at point-to-plane -----------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [2, 5])
@pytest.mark.parametrize("name", SIZES)
def test_criteria_against_the_oracle_loop(lm, name, max_iter):
    """max_iteration in {2, 5} with relative_fitness = relative_rmse = 1e-3 against the oracle's icp_point_to_plane at those values."""
    case, sfs = ref.cases()[name]
    got = run(lm, case, sfs, **kwargs("point_to_plane", max_iter, 1e-3))
    compare(case, sfs, got, "point_to_plane", max_iter, 1e-3, "%s, point-to-plane, max_iteration %d, 1e-3" % (name, max_iter))
    assert all(g["stage"] == 3 and g["iterations"] <= max_iter for g in got if g["residual"] != -1.0)


def test_the_two_tolerances_are_carried_separately(lm):
    """relative_fitness alone loose, relative_rmse alone loose, both loose: three different iteration counts on the restatement (the
    run ends when BOTH tests hold), and the same three on the device."""
    full, sfs = ref.cases()["batch3"]
    case = full.subset([0])
    c = ref.clouds(case.scene, case.mds[0], K_CAM, case.Ks[0], case.xy[0][0], case.xy[0][1], sfs)
    its = {}
    for rf, rr in ((1.0, 1e-6), (1e-6, 1.0), (1.0, 1.0)):
        hist = []
        _, fit, rmse, it = ref.icp_point_to_point(c["src"], c["tgt"], c["init_guess"], rel_fitness=rf, rel_rmse=rr, history=hist)
        assert ref.ill_posed_p2p(hist, rf, rr) == ""
        g = run(lm, case, sfs, estimation="point_to_point", relative_fitness=rf, relative_rmse=rr)[0]
        assert g["iterations"] == it and abs(g["residual"] - fit) < 1e-6 and abs(g["rmse"] - rmse) < 1e-6, (rf, rr, g["iterations"], it)
        its[(rf, rr)] = it
    assert its[(1.0, 1.0)] == 1 and len(set(its.values())) == 3, its


# ---- 5: defaults and determinism ------------------------------------------------------------------------------------
def _bits(res):
    return [(r["R"].tobytes(), r["t"].tobytes(), r["residual"], r["rmse"], r["iterations"], r["stage"]) for r in res]


@pytest.mark.parametrize("name", ["small", "batch3"])
def test_defaults_are_the_run_without_the_new_arguments(lm, name):
    case, sfs = ref.cases()[name]
    plain = run(lm, case, sfs)
    named = run(lm, case, sfs, **kwargs("point_to_plane", 30, 1e-6))
    assert _bits(plain) == _bits(named) and all(r["stage"] == 1 for r in plain if r["residual"] != -1.0)
    a, b = run(lm, case, sfs, estimation="point_to_point"), run(lm, case, sfs, estimation="point_to_point")
    assert _bits(a) == _bits(b)


# ---- 6: the pipeline -----------------------------------------------------------------------------------------------
def test_pipeline_point_to_point_equals_match_nms_pose_refine(lm):
    """Pipeline(estimation="point_to_point") on a small bank = Detector.match + nms + pose_refine_batch(estimation="point_to_point"),
    detection by detection (as tests/test_gpu_parity.py does for the default)."""
    import linemod_oracle as lo
    import synth
    W, H, T, nfeat, n, thr, top_k = 640, 480, [4, 8], (64, 32), 60, 70.0, 8
    rgb, dep = synth.make_frame(11, W, H)
    od = lo.OracleDetector(nfeat[0], T)
    pyr = od.quantize_pyramid(rgb, dep)
    feat, offs, wh = synth.make_planted_bank(77, n, [(p[0], p[1]) for p in pyr], T, nfeat)
    E = 2 * len(T)
    det = lm.Detector(nfeat[0], T, device=0)
    det.addClassPacked("obj", feat, offs, wh)
    rng = np.random.default_rng(5)
    shapes = [synth.synth_model_depth(200 + k, W, H) for k in range(4)]
    views = [(shapes[t % 4], K_CAM.copy(), np.eye(3, dtype=np.float32),
              np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), 1000 + rng.uniform(-20, 20)], np.float32)) for t in range(n)]
    pipe = lm.Pipeline(det, W, H, scene_from_scene=True, estimation="point_to_point")
    try:
        pipe.set_views("obj", [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views])
        det.setFrame([rgb, dep])
        got, _ = pipe.run(thr, ["obj"], K_CAM, top_k=top_k, nms_iou=0.5)
    finally:
        pipe.close()
    m = det.matchArray([rgb, dep], thr, ["obj"])
    dets = np.zeros((len(m), 5))
    for i, r in enumerate(m):
        w, h = wh[int(r["template_id"]) * E]
        dets[i] = (r["x"], r["y"], r["x"] + w, r["y"] + h, r["similarity"])
    sel = [m[i] for i in lm.nms(dets, 0.5)[:top_k]]
    tid = [int(r["template_id"]) for r in sel]
    poses, _ = lm.pose_refine_batch(dep, K_CAM, [views[t][0] for t in tid], np.stack([views[t][1] for t in tid]), np.stack([views[t][2] for t in tid]),
                                    np.stack([views[t][3] for t in tid]), [(int(r["x"]), int(r["y"])) for r in sel], device=0, scene_from_scene=True,
                                    estimation="point_to_point")
    assert len(got) == len(sel) > 0
    refined = 0
    for g, r, p in zip(got, sel, poses):
        assert (g["x"], g["y"], g["template_id"], g["similarity"]) == (int(r["x"]), int(r["y"]), int(r["template_id"]), float(r["similarity"]))
        if p["residual"] == -1.0:
            assert g["status"] == 1 and g["residual"] == -1.0 and g["stage"] == 0
            continue
        refined += 1
        assert g["status"] == 0 and g["iterations"] == p["iterations"] and abs(g["residual"] - p["residual"]) < 1e-6 and g["stage"] == p["stage"] == 3
        if len(got) == top_k:                                       # same hypothesis count = same slicing: identical sums
            assert np.allclose(g["R"], p["R"], atol=1e-9, equal_nan=True) and np.allclose(g["t"], p["t"], atol=1e-6, equal_nan=True)
        else:
            assert np.allclose(g["R"], p["R"], atol=1e-6, equal_nan=True) and np.allclose(g["t"], p["t"], atol=1e-3, equal_nan=True)
    assert refined > 0


# ---- 7: bad values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(estimation="point_to_line"), dict(max_iteration=-1), dict(relative_rmse=0.0)])
def test_bad_values_raise_before_anything_runs(lm, kw):
    case, sfs = ref.cases()["small"]
    for make in (lambda: run(lm, case, sfs, **kw), lambda: lm.poseRefine(device=0, **kw), lambda: lm.IcpContext(device=0, **kw)):
        with pytest.raises(RuntimeError) as e:
            make()
        if "estimation" in kw:
            assert "point_to_plane" in str(e.value) and "point_to_point" in str(e.value)


def test_c_abi_checks_the_options(lm):
    """lm_icp_set_options: LM_ERR_INVALID with a message, the context keeps its options; NULL restores the defaults."""
    import ctypes
    lib = lm.load_library()
    case, sfs = ref.cases()["small"]
    ctx = lm.IcpContext(device=0, scene_from_scene=sfs, max_iteration=0)
    try:
        o = lm.IcpOptions()
        lib.lm_icp_options_init(ctypes.byref(o))
        assert (o.max_iteration, o.reserved, o.relative_fitness, o.relative_rmse) == (30, 0, 1e-6, 1e-6)
        for field, bad in (("max_iteration", -1), ("relative_fitness", float("nan")), ("relative_rmse", 0.0), ("relative_rmse", float("inf"))):
            b = lm.IcpOptions(30, 0, 1e-6, 1e-6)
            setattr(b, field, bad)
            assert lib.lm_icp_set_options(ctx._h, ctypes.byref(b)) != 0
            assert field in lib.lm_last_error().decode()
        ctx.set_scene(case.scene, K_CAM)
        ctx.set_models(case.mds)
        Ks, Rs, ts, xy = case.arrays()
        assert ctx.run(Ks, Rs, ts, xy)[0][0]["iterations"] == 0                   # still evaluate-only
        assert lib.lm_icp_set_options(ctx._h, None) == 0
        res = ctx.run(Ks, Rs, ts, xy)[0][0]
        assert res["iterations"] >= 1 and res["stage"] == 1                       # the defaults again: the team kernel
    finally:
        ctx.close()
