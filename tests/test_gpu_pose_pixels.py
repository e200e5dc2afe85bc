"""GPU tests of the pixel passes of the pose errors (k_vsd, k_gt_stats) on chosen pixels, and of every chunked path of csrc/pose_error.cpp,
against the numpy statement (tests/pose_error_ref.py, tests/pose_sym_ref.py) on the inputs of tests/pose_pixel_cases.py, which
tests/test_pose_pixel_cases.py proves on the CPU.

The bars are the project's own (tests/test_gpu_pose_error.py::assert_criteria, tests/test_gpu_pose_sym.py): step VSD, COU and the GT statistics
equal, tlinear VSD within 1e-12, ADD / ADI within 1e-4 mm, MSSD / MSPD within 1e-9.  Every call is made twice and compared byte for byte."""
import os

import numpy as np
import pytest

import pose_pixel_cases as pc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
SYM_TOL = 1e-9                                                           # tests/test_gpu_pose_sym.py::TOL


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
def blob(lm):
    m = lm.Mesh(*pc.mesh())
    yield m
    m.close()


def twice(fn):
    """fn() twice; dicts of arrays and lists of dicts must repeat byte for byte."""
    a, b = fn(), fn()
    if isinstance(a, dict):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    else:
        assert a == b
    return a


def device_pixels(lm, mesh, c, scene=None, **opt):
    """{"vsd", "vsd_tlinear", "cou"} of a case's poses, each call repeated."""
    scene = c["scene"] if scene is None else scene
    args = (mesh, c["eR"], c["et"], c["gR"], c["gt"], c["K"], scene)
    got = twice(lambda: lm.pose_errors(*args, metrics=("vsd", "cou"), **opt))
    tl = twice(lambda: lm.pose_errors(*args, metrics=("vsd",), cost="tlinear", **opt))
    assert got["vsd"].shape == got["cou"].shape == tl["vsd"].shape == (len(c["eR"]), len(c["gR"]))
    got["vsd_tlinear"] = tl["vsd"]
    return got


def assert_pixels(got, want):
    """assert_criteria's bars for the rendered metrics: step VSD and COU equal as floats, tlinear VSD within 1e-12."""
    for k in ("vsd", "cou"):
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (k, len(bad), bad[:4].tolist(), [(got[k][tuple(i)], want[k][tuple(i)]) for i in bad[:4]])
    d = np.abs(got["vsd_tlinear"] - want["vsd_tlinear"]).max() if got["vsd_tlinear"].size else 0.0
    print("tlinear vsd: max |device - numpy| = %.3e" % d)
    assert np.allclose(got["vsd_tlinear"], want["vsd_tlinear"], rtol=0, atol=1e-12), d


def assert_stats(got, want):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert a == b, (g, a, b)                                         # counts, boxes and visib_fract equal


def device_stats(lm, mesh, c, scene=None, **opt):
    return twice(lambda: lm.gt_stats(mesh, c["gR"], c["gt"], c["K"], c["scene"] if scene is None else scene, **opt))


# ---- the pixel passes on chosen pixels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.FRAME_NAMES)
def test_frame_sizes(lm, blob, name):
    c, want = pc.frame_case(name), pc.frame_expected(name)
    assert_pixels(device_pixels(lm, blob, c), want)
    assert_stats(device_stats(lm, blob, c), want["stats"])
    cou = lm.pose_errors(blob, c["eR"], c["et"], c["gR"], c["gt"], c["K"], None, metrics=("cou",), im_size=(c["W"], c["H"]))["cou"]
    assert np.array_equal(cou, want["cou"])                              # scene == nullptr: the same pass, COU counts only


@pytest.mark.parametrize("side", pc.DELTA_SIDES)
def test_delta_at_equality(lm, blob, side):
    c, want = pc.delta_case(side), pc.delta_expected(side)
    for delta, w in zip(c["deltas"], want):
        assert_pixels(device_pixels(lm, blob, c, delta=delta), w)
        assert_stats(device_stats(lm, blob, c, delta=delta, clip_far=10000.0), w["stats"])


def test_tau_at_equality(lm, blob):
    c, want = pc.tau_case(), pc.tau_expected()
    for tau, w in zip(c["taus"], want):
        assert_pixels(device_pixels(lm, blob, c, tau=tau), w)


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_hostile_scenes(lm, blob, dtype):
    c, want = pc.hostile_case(dtype), pc.hostile_expected(dtype)
    got = device_pixels(lm, blob, c)
    assert_pixels(got, want)
    st = device_stats(lm, blob, c)
    assert_stats(st, want["stats"])
    if dtype == "uint16":                                                # the uint16 scene equals its float32 conversion
        as_f32 = device_pixels(lm, blob, c, scene=c["scene"].astype(F32))
        for k in got:
            assert got[k].tobytes() == as_f32[k].tobytes(), k
        assert device_stats(lm, blob, c, scene=c["scene"].astype(F32)) == st


def test_empty_results(lm, blob):
    c, want = pc.empty_case(), pc.empty_expected()
    clip = dict(clip_near=pc.EMPTY_NEAR, clip_far=pc.EMPTY_FAR)
    got = device_pixels(lm, blob, c, **clip)
    assert_pixels(got, want)
    st = device_stats(lm, blob, c, **clip)
    assert_stats(st, want["stats"])
    g, e = pc.EMPTY_GT.index, pc.EMPTY_EST.index
    for k in ("beyond_far", "outside"):
        s = st[g(k)]
        assert s["px_count_all"] == 0 and s["visib_fract"] == 0.0 and s["bbox_visib"] == [-1, -1, -1, -1]
    assert st[g("occluded")]["px_count_visib"] == 0 and st[g("occluded")]["bbox_visib"] == [-1, -1, -1, -1]
    assert st[g("one_pixel")]["px_count_visib"] == 1 and st[g("one_pixel")]["bbox_visib"] == [c["one"][1], c["one"][0], 0, 0]
    for k in ("vsd", "vsd_tlinear", "cou"):
        assert got[k][e("before_near"), g("visible")] == 1.0 and got[k][e("before_near"), g("beyond_far")] == 1.0 and got[k][e("outside"), g("outside")] == 1.0


@pytest.mark.parametrize("delta", pc.OPTION_DELTAS)
def test_delta_and_tau_off_their_defaults(lm, blob, delta):
    c = pc.frame_case("100x77")
    for tau in pc.OPTION_TAUS:
        assert_pixels(device_pixels(lm, blob, c, delta=delta, tau=tau), pc.option_expected(delta=delta, tau=tau))
    assert_stats(device_stats(lm, blob, c, delta=delta, clip_far=10000.0), pc.option_expected(delta=delta)["stats"])


@pytest.mark.parametrize("near,far", pc.OPTION_CLIPS)
def test_clip_planes_through_the_blob(lm, blob, near, far):
    c, want = pc.frame_case("100x77"), pc.option_expected(near=near, far=far)
    assert_pixels(device_pixels(lm, blob, c, clip_near=near, clip_far=far), want)
    assert_stats(device_stats(lm, blob, c, clip_near=near, clip_far=far), want["stats"])


# ---- chunked paths -----------------------------------------------------------------------------------------------------------------------------
def in_pieces(lm, mesh, c, e_piece, g_piece, **kw):
    """The same poses in pieces small enough not to chunk, assembled into the (E, G) tables."""
    n_est, n_gt = len(c["eR"]), len(c["gR"])
    out = None
    for e0 in range(0, n_est, e_piece):
        for g0 in range(0, n_gt, g_piece):
            r = lm.pose_errors(mesh, c["eR"][e0:e0 + e_piece], c["et"][e0:e0 + e_piece], c["gR"][g0:g0 + g_piece], c["gt"][g0:g0 + g_piece], **kw)
            if out is None:
                out = {k: np.zeros((n_est, n_gt)) for k in r}
            for k in r:
                out[k][e0:e0 + e_piece, g0:g0 + g_piece] = r[k]
    return out


PIECES = {"a_200x60": (100, 60), "b_5x300": (5, 150), "c_140x140": (70, 70), "e_2048x1024": (15, 4)}


@pytest.mark.parametrize("name", pc.CHUNKED_VSD_NAMES)
def test_chunked_renders(lm, blob, name):
    c, T = pc.chunked_vsd_case(name), pc.chunked_vsd_distinct(name)
    assert len(c["eR"]) + len(c["gR"]) > pc.views_per_render(c["W"], c["H"])
    se, sg, _ = pc.vsd_sources(c["n_est"], c["n_gt"], *pc.vsd_chunking(c["n_est"], c["n_gt"], c["W"], c["H"]))
    want = {k: pc.expand(T[k], se, sg, c["pe"], c["pg"]) for k in ("vsd", "vsd_tlinear", "cou")}
    got = device_pixels(lm, blob, c)
    assert_pixels(got, want)
    ep, gp = PIECES[name]
    assert ep + gp <= pc.views_per_render(c["W"], c["H"])
    pieces = in_pieces(lm, blob, c, ep, gp, K=c["K"], scene_depth=c["scene"], metrics=("vsd", "cou"))
    tl = in_pieces(lm, blob, c, ep, gp, K=c["K"], scene_depth=c["scene"], metrics=("vsd",), cost="tlinear")
    assert got["vsd"].tobytes() == pieces["vsd"].tobytes() and got["cou"].tobytes() == pieces["cou"].tobytes()
    assert got["vsd_tlinear"].tobytes() == tl["vsd"].tobytes()


def test_chunked_gt_stats(lm, blob):
    c = pc.gt_stats_case()
    assert len(c["gR"]) == pc.GT_STATS_N > pc.views_per_render(c["W"], c["H"])
    st = device_stats(lm, blob, c)
    assert_stats(st, [c["stats"][g % pc.PERIOD_GT] for g in range(pc.GT_STATS_N)])
    halves = sum((lm.gt_stats(blob, c["gR"][g0:g0 + 150], c["gt"][g0:g0 + 150], c["K"], c["scene"]) for g0 in (0, 150)), [])
    assert st == halves


def test_chunked_point_metrics(lm):
    c = pc.pts_case()
    n_est, n_gt = pc.PTS_SHAPE
    assert n_est * n_gt > pc.MAX_PTS_PAIRS
    mesh = lm.Mesh(c["V"], c["F"])
    got = twice(lambda: lm.pose_errors(mesh, c["eR"], c["et"], c["gR"], c["gt"], metrics=("add", "adi")))
    src = pc.flat_sources(n_est * n_gt, pc.MAX_PTS_PAIRS)
    for k in ("add", "adi"):
        d = np.abs(got[k].ravel() - pc.flat_expand(c[k], src, n_gt)).max()
        print("%s: max |device - numpy| = %.3e mm" % (k, d))
        assert d <= 1e-4, (k, d)
    pieces = in_pieces(lm, mesh, c, 100, n_gt, metrics=("add", "adi"))
    add_only = lm.pose_errors(mesh, c["eR"], c["et"], c["gR"], c["gt"], metrics=("add",))["add"]
    mesh.close()
    assert 100 * n_gt <= pc.MAX_PTS_PAIRS
    for k in ("add", "adi"):
        assert got[k].tobytes() == pieces[k].tobytes(), k
    assert add_only.tobytes() == got["add"].tobytes()                    # kPtsAddOnly through the same loop


def test_chunked_symmetry_batches(lm):
    c = pc.sym_case()
    n_est, n_gt = pc.SYM_SHAPE
    syms = lm.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_sym_disc_step=pc.SYM_STEP)
    assert len(syms[0]) == c["n_sym"] and n_est * n_gt > pc.sym_batch(len(c["V"]), 2, c["n_sym"])
    assert np.abs(syms[0] - c["Rs"]).max() <= 1e-15 and np.abs(syms[1] - c["ts"]).max() <= 1e-12
    mesh = lm.Mesh(c["V"], c["F"])
    kw = dict(K=pc.SYM_K, metrics=("mssd", "mspd"), symmetries=syms)
    got = twice(lambda: lm.pose_errors(mesh, c["eR"], c["et"], c["gR"], c["gt"], **kw))
    src = pc.flat_sources(n_est * n_gt, pc.sym_batch(len(c["V"]), 2, c["n_sym"]))
    for k in ("mssd", "mspd"):
        d = np.abs(got[k].ravel() - pc.flat_expand(c[k], src, n_gt)).max()
        print("%s: max |device - numpy| = %.3e" % (k, d))
        assert d <= SYM_TOL, (k, d)
    pieces = in_pieces(lm, mesh, c, 50, n_gt, **kw)
    mesh.close()
    assert 50 * n_gt <= pc.sym_batch(len(c["V"]), 2, c["n_sym"])
    for k in ("mssd", "mspd"):
        assert got[k].tobytes() == pieces[k].tobytes(), k


def test_a_default_call_after_chunked_calls_returns_the_recorded_values(lm, gold):
    """The scratch buffers shrink and grow with the calls: the recorded pysixd numbers before, between and after chunked calls on the same Mesh."""
    import test_gpu_pose_error as tpe
    V, F, K, scene = gold["A_pts"], gold["A_faces"], gold["K"], gold["scene"]
    rec = {k: gold["A_" + k] for k in ("vsd_tlinear", "cou", "add", "adi", "re", "te")}
    rec["vsd"] = gold["A_vsd_step"]
    mesh = lm.Mesh(V, F)

    def golden():
        got = lm.pose_errors(mesh, gold["est_R"], gold["est_t"], gold["gt_R"], gold["gt_t"], K, scene)
        got["vsd_tlinear"] = lm.pose_errors(mesh, gold["est_R"], gold["est_t"], gold["gt_R"], gold["gt_t"], K, scene, metrics=("vsd",), cost="tlinear")["vsd"]
        tpe.assert_criteria(got, rec)
        st = lm.gt_stats(mesh, gold["gt_R"], gold["gt_t"], K, scene)
        for g, s in enumerate(st):
            assert [s["px_count_all"], s["px_count_valid"], s["px_count_visib"]] + s["bbox_obj"] + s["bbox_visib"] == gold["gts_int"][g].tolist()
        return got

    first = golden()
    c = pc.chunked_vsd_case("c_140x140")
    big = lm.pose_errors(mesh, c["eR"], c["et"], c["gR"], c["gt"], c["K"], c["scene"], metrics=("vsd", "cou", "add", "adi"))
    assert big["vsd"].shape == (140, 140)
    after = golden()
    g = pc.gt_stats_case()
    assert len(lm.gt_stats(mesh, g["gR"], g["gt"], g["K"], g["scene"])) == pc.GT_STATS_N
    s = pc.sym_case()
    syms = lm.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_sym_disc_step=0.01)
    lm.pose_errors(mesh, s["eR"], s["et"], s["gR"], s["gt"], pc.SYM_K, metrics=("mssd", "mspd"), symmetries=syms)
    last = golden()
    mesh.close()
    for k in first:
        assert first[k].tobytes() == after[k].tobytes() == last[k].tobytes(), k
