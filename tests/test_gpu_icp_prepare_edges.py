"""The kernels that prepare the ICP clouds (icp.hip: k_icp_voxel_wide / k_icp_voxel, k_icp_grid_wide / k_icp_grid, k_icp_knn /
k_icp_knn_far, k_icp_normals) on inputs that leave their usual route, against the CPU oracle.

The inputs are tests/icp_prepare_cases.py; each proves on the CPU that it sits on its edge (tests/test_icp_prepare_cases.py).  All of
them but mid_cloud are the hypotheses of ONE batch on one frame, so a cloud the one-workgroup kernels redo sits next to clouds the
eight-workgroup kernels finish; the batch runs with the target taken from the model (verbatim, LL.cpp:109) and from the scene.

Per case and mode:
  path        read_debug kind 3 (helpers.DBG3_VOX_DONE_MODEL ...): the eight groups of the wide sorts finished the cloud, or did not, as
              icp_prepare_cases.voxel_groups / grid_groups say they must; the points handed to k_icp_knn_far (all that need it: its list refuses none).
  clouds      kinds 0 and 1 equal the oracle's in shape and to 1e-12; n_source, n_target, init_guess.
  neighbours  kind 5 (rows in sorted order, kind 6 = their original indices): the neighbour count is k = min(30, n_target) and each of
              the nine cumulants is within (k - 1) * eps * sum|term| of the sum over the oracle's ordered list (terms rounded to
              double, added in np.longdouble).  The bound is the sequential-summation bound: any order of adding k terms errs by at most
              (k - 1) * u * sum|term|, a product fused into the sum differs from its rounding by u * |term|, u = eps / 2, so k * u <=
              (k - 1) * eps for k >= 2; for k = 1 nothing is rounded and the bound is 0.  A wrong neighbour moves a sum by millimetres.
  normals     1 - |cos| < 1e-9 against the oracle where the relative eigenvalue gap is at least icp_prepare_cases.NORMAL_GAP_MIN (how
              it was measured: there); below it a unit vector orthogonal to the oracle's largest eigenvector within the same angle.  At
              most a quarter of a case is below the gap, and only in wire and tiny_3 (three collinear points: all of it); exactly (0, 0, 1)
              for k < 3.
  pose        the bar of test_gpu_icp_oracle.py (iterations, |residual| < 1e-6, R within 1e-4, t within 1e-4 m; NaN exactly where the
              oracle has NaN: every case but lattice_ties, the two near ones and deep_range has a NaN init guess, the frame's centre
              pixel is not theirs), exempt only by lo.ill_posed on the oracle's history.
A second run of the batch repeats bit for bit, and a process under LM_ICP_WIDE_SORT=0 (one workgroup per cloud) returns the same clouds
bit for bit and does mid_cloud, whose radix keys stay in HBM."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linemod_oracle as lo
import icp_prepare_cases as pc
from helpers import (DBG3_GRID_DONE, DBG3_KNN_FAR, DBG3_KNN_FAR_REFUSED, DBG3_VOX_DONE_MODEL, DBG3_VOX_DONE_SCENE, SORT_GROUPS)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for n, _ in pc.FRAME]
MODES = {"verbatim": False, "scene": True}
EPS = np.finfo(np.float64).eps


def run_batch(cases, scene_mode, reps=1):
    """IcpContext.run on the cases as one batch, `reps` times: per repetition and hypothesis the result and the read-backs."""
    import linemodLevelup_pybind as mod
    n = len(cases)
    Ks = np.tile(pc.K512.reshape(1, 9), (n, 1))
    Rs = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    ts = np.tile(np.array([[0, 0, 1000]], np.float32), (n, 1))
    ctx = mod.IcpContext(device=0, scene_from_scene=scene_mode)
    try:
        ctx.set_scene(cases[0].scene, pc.K512)
        ctx.set_models([c.md for c in cases])
        out = []
        for _ in range(reps):
            res, _ = ctx.run(Ks, Rs, ts, [c.xy for c in cases])
            out.append([dict(res=res[h], src=ctx.read_debug(h, 0), tgt=ctx.read_debug(h, 1), nrm=ctx.read_debug(h, 2), dbg=ctx.read_debug(h, 3),
                             cum=ctx.read_debug(h, 5).reshape(-1, 12), orig=ctx.read_debug(h, 6).astype(np.int64)) for h in range(n)])
        return out
    finally:
        ctx.close()


_WORKER = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [root, os.path.join(root, "6dpose_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")]
import icp_prepare_cases as pc
import test_gpu_icp_prepare_edges as T
z = {}
frame = list(pc.frame_cases().values())
for label, cases, mode in (("verbatim", frame, False), ("scene", frame, True), ("mid", [pc.mid_case()], False)):
    for c, g in zip(cases, T.run_batch(cases, mode)[0]):
        z["%s/%s/src" % (label, c.name)] = g["src"]; z["%s/%s/tgt" % (label, c.name)] = g["tgt"]; z["%s/%s/dbg" % (label, c.name)] = g["dbg"]
        z["%s/%s/pose" % (label, c.name)] = np.concatenate([g["res"]["R"].ravel(), g["res"]["t"].ravel(), [g["res"]["iterations"], g["res"]["residual"]]])
np.savez(out, **z)
print("RESULT ok")
"""


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


@pytest.fixture(scope="module")
def batches(lm):
    """{mode: [first run, second run]}, each a list of per-hypothesis dicts in the order of NAMES."""
    cases = [pc.frame_cases()[n] for n in NAMES]
    return {label: run_batch(cases, mode, reps=2) for label, mode in MODES.items()}


@pytest.fixture(scope="module")
def one_workgroup(lm, tmp_path_factory):
    """The frame's two batches and mid_cloud in a process of its own under LM_ICP_WIDE_SORT=0 (the knob is read once per process)."""
    d = tmp_path_factory.mktemp("icp_prepare")
    script = d / "worker.py"
    script.write_text(_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT, str(d / "out.npz")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, LM_ICP_WIDE_SORT="0"))
    text = r.stdout.decode()
    assert r.returncode == 0 and "RESULT ok" in text, text[-3000:]
    return dict(np.load(d / "out.npz"))


def got_of(batches, name, label, rep=0):
    return batches[label][rep][NAMES.index(name)]


CASES = [(n, m) for n in NAMES for m in MODES]


@pytest.mark.parametrize("name,label", CASES)
def test_path(batches, name, label):
    """The case was prepared by the kernels its edge sends it to."""
    c, g = pc.frame_cases()[name], got_of(batches, name, label)
    o = c.oracle(MODES[label])
    d = g["dbg"]
    clouds = [(DBG3_VOX_DONE_MODEL, o["model_pts"])] + ([(DBG3_VOX_DONE_SCENE, o["scene_pts"])] if MODES[label] else [])
    for idx, pts in clouds:
        vg = pc.voxel_groups(pts)
        done = int(d[idx])
        print("\n%s %s: vox_done %d (groups %s, %d index bits)" % (name, label, done, vg["counts"].tolist(), vg["bits"]))
        if vg["wide"]:
            assert done == SORT_GROUPS, (name, label, done)
        elif vg["bits"] > 32:
            assert done == 0, (name, label, done)                     # every group leaves the cloud alike
        else:
            assert 0 <= done < SORT_GROUPS, (name, label, done)       # a group over the cap, the groups behind it give up
    gg = pc.grid_groups(o["raw_tgt"], o["tgt"])
    grid_done, far, refused = int(d[DBG3_GRID_DONE]), int(d[DBG3_KNN_FAR]), int(d[DBG3_KNN_FAR_REFUSED])
    print("%s %s: grid_done %d (groups %s), far %d, refused %d" % (name, label, grid_done, gg["counts"].tolist(), far, refused))
    assert (grid_done == SORT_GROUPS) if gg["wide"] else (0 <= grid_done < SORT_GROUPS), (name, label, grid_done)
    # the edges themselves: cap_8193 leaves both wide kernels, deep_range the voxel one, every other case stays on them
    want_vox, want_grid = {"cap_8193": (False, False), "deep_range": (False, True)}.get(name, (True, True))
    assert all(pc.voxel_groups(p)["wide"] == want_vox for _, p in clouds) and gg["wide"] == want_grid, (name, label)
    sure = pc.surely_far(o, gg["wide"])
    # every point that k_icp_knn cannot finish is k_icp_knn_far's (its list holds every target): none is refused, so none is summed another way
    assert refused == 0 and sure <= far <= len(o["tgt"]), (name, label, far, refused, sure)
    if name == "many_far":
        assert far >= sure > pc.FAR_MAX, (far, sure)                  # more than the 256 the list once stopped at
    if name.startswith("cap") or name == "deep_range":
        assert far >= 9, (name, far)                                  # the blob: fewer than k points, metres from the rest


@pytest.mark.parametrize("name,label", CASES)
def test_clouds(batches, name, label):
    c, g = pc.frame_cases()[name], got_of(batches, name, label)
    o = c.oracle(MODES[label])
    assert g["src"].shape == o["src"].shape and g["tgt"].shape == o["tgt"].shape, (name, label, g["src"].shape, o["src"].shape, g["tgt"].shape, o["tgt"].shape)
    assert np.abs(g["src"] - o["src"]).max() < 1e-12 and np.abs(g["tgt"] - o["tgt"]).max() < 1e-12, (name, label)
    assert g["res"]["n_source"] == len(o["src"]) and g["res"]["n_target"] == len(o["tgt"])
    init = g["dbg"][:3]
    assert np.array_equal(np.isnan(init), np.isnan(o["init"])), (name, label, init, o["init"])
    if np.isfinite(o["init"]).all():
        assert np.abs(init - o["init"]).max() < 1e-12, (name, label)
    # (the model depth at the frame's centre is lattice_ties' or 0, and only the near patches lie within 0.4 m of depth 0)
    assert np.isfinite(o["init"]).all() == (name in ("lattice_ties", "near_many", "near_few", "deep_range")), name


@pytest.mark.parametrize("name,label", CASES)
def test_neighbours(batches, name, label):
    c, g = pc.frame_cases()[name], got_of(batches, name, label)
    o = c.oracle(MODES[label])
    n, k = len(o["tgt"]), o["k"]
    assert g["cum"].shape == (n, 12) and sorted(g["orig"].tolist()) == list(range(n)), (name, label)
    cum = np.zeros((n, 12))
    cum[g["orig"]] = g["cum"]                                         # rows by original index
    assert (cum[:, 9] == k).all(), (name, label, np.unique(cum[:, 9]))
    q = o["tgt"][o["lists"]]                                          # (n, k, 3)
    iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    terms = np.concatenate([q, np.stack([q[..., a] * q[..., b] for a, b in iu], -1)], -1)      # (n, k, 9), rounded to double
    ref = terms.astype(np.longdouble).sum(1)
    bound = (k - 1) * EPS * np.abs(terms).sum(1)
    err = np.abs(cum[:, :9].astype(np.longdouble) - ref).astype(np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if k > 1 else float(err.max())
    print("\n%s %s: k %d, largest error / bound %.3g" % (name, label, k, worst))
    bad = np.nonzero((err > bound).any(1))[0]
    assert len(bad) == 0, (name, label, len(bad), bad[:5].tolist(), err[bad[:5]].max(1).tolist(), bound[bad[:5]].max(1).tolist())
    # the separation: squared distance to the nearest other point
    if n > 1:
        assert np.array_equal(cum[:, 10], o["d2"][:, 1]), (name, label)


@pytest.mark.parametrize("name,label", CASES)
def test_normals(batches, name, label):
    c, g = pc.frame_cases()[name], got_of(batches, name, label)
    o = c.oracle(MODES[label])
    if o["k"] < 3:
        assert np.array_equal(g["nrm"], np.tile([0.0, 0.0, 1.0], (len(o["tgt"]), 1))), (name, label, g["nrm"])
        return
    _, big, gap = pc.exact_normals(o["tgt"], o["lists"])
    firm = gap >= pc.NORMAL_GAP_MIN
    assert 4 * int((~firm).sum()) <= len(gap) or name == "tiny_3", (name, label, int((~firm).sum()))
    assert firm.all() or name in ("wire", "tiny_3"), (name, label, int((~firm).sum()), float(gap.min()))
    dis = 1 - np.abs((g["nrm"] * o["normals"]).sum(1))
    print("\n%s %s: %d normals, %d below the gap, smallest gap above %.3g, largest 1 - |cos| %.3g" % (
        name, label, len(gap), int((~firm).sum()), gap[firm].min() if firm.any() else np.nan, dis[firm].max() if firm.any() else np.nan))
    assert (dis[firm] < 1e-9).all(), (name, label, float(dis[firm].max()), int(np.argmax(np.where(firm, dis, 0))))
    loose = g["nrm"][~firm]
    assert (np.abs(np.linalg.norm(loose, axis=1) - 1) < 1e-9).all(), (name, label)
    assert (0.5 * (loose * big[~firm]).sum(1) ** 2 < 1e-9).all(), (name, label)


def expected_pose(o):
    """lo.pose_refine's R, t (mm) for model R = I, t = (0, 0, 1000): T_icp * [I | (0, 0, 1)], all four columns of the product (a NaN
    translation makes the whole row NaN, as in the reference's matrix product)."""
    base = np.eye(4, dtype=np.float32)
    base[2, 3] = np.float32(1000.0) / np.float32(1000.0)
    result = o["T"] @ base.astype(np.float64)
    return result[:3, :3].copy(), result[:3, 3] * 1000.0


def check_pose(name, label, res, o, ill):
    R, t = np.asarray(res["R"], np.float64), np.asarray(res["t"], np.float64).ravel()
    wR, wt = expected_pose(o)
    assert res["stage"] in (1, 2, 3), (name, label, res["stage"])
    if not np.isfinite(wR).all() or not np.isfinite(wt).all():
        assert np.array_equal(np.isnan(R), np.isnan(wR)) and np.array_equal(np.isnan(t), np.isnan(wt)), (name, label)
        assert res["residual"] == o["fitness"] and res["iterations"] == o["iterations"], (name, label, res["residual"], res["iterations"])
        return
    why = lo.ill_posed(o["history"])
    if why:
        ill.append("%s %s: %s" % (name, label, why))
        return
    assert res["iterations"] == o["iterations"], (name, label, res["iterations"], o["iterations"])
    assert abs(res["residual"] - o["fitness"]) < 1e-6, (name, label, res["residual"], o["fitness"])
    assert np.abs(R - wR).max() < 1e-4 and np.abs(t - wt).max() / 1000.0 < 1e-4, (name, label, np.abs(R - wR).max(), np.abs(t - wt).max())


@pytest.mark.parametrize("label", list(MODES))
def test_registration(batches, label):
    ill = []
    for name in NAMES:
        check_pose(name, label, got_of(batches, name, label)["res"], pc.frame_cases()[name].oracle(MODES[label]), ill)
    print("\n%s: ill-posed by the oracle's evidence: %s" % (label, ill))
    assert 4 * len(ill) <= len(NAMES), ill


@pytest.mark.parametrize("name,label", CASES)
def test_second_run_repeats_bit_for_bit(batches, name, label):
    """The same batch run again on the same context: clouds, neighbour sums, normals, poses and paths bit for bit.

    many_far found a run that did not: k_icp_knn handed the points it could not finish to k_icp_knn_far through an atomic counter, the
    list stopped at 256 entries and the points beyond it (85 of 341 here) were summed by their own wave, 64 lanes instead of 512
    threads.  Which points those were depended on the order the waves arrived, so the cumulants of 36-64 of the 2080 targets differed
    between two runs by up to 4.5e-13 (the last place of sums near 1e3).  The list now holds every target."""
    a, b = got_of(batches, name, label, 0), got_of(batches, name, label, 1)
    diff = {}
    for key in ("src", "tgt", "orig", "cum", "nrm"):
        if not np.array_equal(a[key], b[key], equal_nan=True):
            diff[key] = (int((a[key] != b[key]).any(-1).sum()) if a[key].ndim > 1 else int((a[key] != b[key]).sum()), float(np.nanmax(np.abs(a[key] - b[key]))))
    for key in ("R", "t"):
        if not np.array_equal(a["res"][key], b["res"][key], equal_nan=True):
            diff[key] = float(np.nanmax(np.abs(a["res"][key] - b["res"][key])))
    print("\n%s %s: differing between two runs (rows, largest difference): %s" % (name, label, diff or "nothing"))
    assert not diff, (name, label, diff)
    assert a["res"]["iterations"] == b["res"]["iterations"] and a["res"]["residual"] == b["res"]["residual"], (name, label)
    for idx in (DBG3_VOX_DONE_MODEL, DBG3_VOX_DONE_SCENE, DBG3_GRID_DONE, DBG3_KNN_FAR, DBG3_KNN_FAR_REFUSED):
        assert a["dbg"][idx] == b["dbg"][idx], (name, label, idx)


def test_one_workgroup_kernels_return_the_same_clouds(batches, one_workgroup):
    """LM_ICP_WIDE_SORT=0: k_icp_voxel and k_icp_grid alone did every cloud (no group of the wide kernels finished any), and the clouds
    equal the default run's bit for bit."""
    z = one_workgroup
    for label in MODES:
        for name in NAMES:
            g, d = got_of(batches, name, label), z["%s/%s/dbg" % (label, name)]
            assert d[DBG3_VOX_DONE_MODEL] == 0 and d[DBG3_VOX_DONE_SCENE] == 0 and d[DBG3_GRID_DONE] == 0, (name, label)
            assert np.array_equal(z["%s/%s/src" % (label, name)], g["src"]) and np.array_equal(z["%s/%s/tgt" % (label, name)], g["tgt"]), (name, label)


def test_mid_cloud_radix_keys_in_hbm(one_workgroup):
    """19200 points under LM_ICP_WIDE_SORT=0: k_icp_voxel sorts them by radix with the keys in HBM (16384 < n <= 32768), k_icp_grid
    the 19200 voxels likewise.  The clouds against the oracle, the pose to the bar."""
    z, c = one_workgroup, pc.mid_case()
    o = c.oracle(False)
    assert 16384 < len(o["model_pts"]) <= 32768 and pc.voxel_groups(o["model_pts"])["bits"] <= 32 and 16384 < len(o["tgt"]) <= 32768
    d = z["mid/mid_cloud/dbg"]
    assert d[DBG3_VOX_DONE_MODEL] == 0 and d[DBG3_GRID_DONE] == 0
    for key in ("src", "tgt"):
        got = z["mid/mid_cloud/" + key]
        assert got.shape == o[key].shape and np.abs(got - o[key]).max() < 1e-12, key
    pose = z["mid/mid_cloud/pose"]
    wR, wt = expected_pose(o)
    assert not lo.ill_posed(o["history"])
    assert pose[12] == o["iterations"] and abs(pose[13] - o["fitness"]) < 1e-6
    assert np.abs(pose[:9].reshape(3, 3) - wR).max() < 1e-4 and np.abs(pose[9:12] - wt).max() / 1000.0 < 1e-4
