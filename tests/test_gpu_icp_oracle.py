"""Every registration path of poseRefine against the CPU oracle (oracle/linemod_oracle.py:pose_refine).

k_icp_team has four builds (one point per thread with the whole target cloud in LDS, one / two / five points per thread
with a slab of it), a cut and relaunch that resumes hypotheses from IcpState, a global-memory mode for a slab that
overflows, and behind it the large builds (stage 2) and the sliced launches (stage 3).  Each test here reaches one of them
on purpose, asserts that it did — by lm_pose_result.stage, IcpState.build and team_note (read_debug kind 3) — and compares
the poses with the oracle.  A row that does not reach its path fails; it never compares another path quietly.

Bar (per hypothesis): equal iterations, n_source and n_target, |residual - oracle| < 1e-6, R entries within 1e-4 and t
within 1e-4 m.  A hypothesis is exempt from the pose bar only when the ORACLE's own history calls it ill-posed
(oracle.ill_posed: a convergence test within 1e-9 of its threshold, or a final JtJ eigenvalue ratio below 1e-8); at most a
quarter of a case may be.  The LM_ICP_* knobs are read once per process, so knob settings run in processes of their own.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import linemod_oracle as lo
import synth
from synth import bump
from helpers import DBG3_BUILD, DBG3_RESUME_IT, DBG3_TEAM_NOTE, DBG3_TEAM_SIZE, K_CAM, h16, pipeline_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
BUILD_NAMES = {0: "sliced", 4: "<1,false>", 6: "<1,true> whole", 7: "<1,true> slab", 10: "<2,true> whole", 11: "<2,true> slab",
               22: "<5,true> whole", 23: "<5,true> slab"}


# ---- inputs --------------------------------------------------------------------------------------
def surface(half_w, half_h, z0=2000.0):
    """A large curved, rippled depth patch (every pixel its own voxel at 2 m): a registration no sliding can satisfy."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xx - W // 2, yy - H // 2
    inside = (np.abs(dx) < half_w) & (np.abs(dy) < half_h)
    depth = z0 - 0.004 * (dx ** 2 + 0.7 * dy ** 2) + 6.0 * np.sin(dx / 9.0) * np.cos(dy / 11.0) + 0.002 * dx * dy
    return np.where(inside, depth, 0).astype(np.uint16)


def rand_rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def model_K(rng):
    """A model camera unlike the scene's: fx, fy, cx and cy each differ."""
    K = K_CAM.copy()
    K[0, 0] *= 1 + rng.uniform(-0.04, 0.04); K[1, 1] *= 1 + rng.uniform(-0.04, 0.04)
    K[0, 2] += rng.uniform(-8, 8); K[1, 2] += rng.uniform(-8, 8)
    return K


def place(md, mK, shift_px, seed, rot_deg=None, t_mm=None):
    """The model surface as the scene sees it elsewhere: back-projected with the model camera, moved by a small rigid motion
    (1-3 degrees about a random axis through its centroid, a few mm) plus the translation that moves it `shift_px` pixels
    in the image, projected with the scene camera (forward splatting, the nearest point wins) + 1 mm noise.  Float depth."""
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(md)
    z = md[ys, xs].astype(np.float64)
    mK = np.asarray(mK, np.float64); sK = K_CAM.astype(np.float64)
    P = np.stack([(xs - mK[0, 2]) / mK[0, 0] * z, (ys - mK[1, 2]) / mK[1, 1] * z, z], 1)
    c = P.mean(0)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = np.radians(rot_deg if rot_deg is not None else rng.uniform(1, 3) * rng.choice([-1, 1]))
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    t = np.asarray(t_mm if t_mm is not None else rng.uniform(-4, 4, 3), np.float64)
    t = t + np.array([shift_px[0] * c[2] / sK[0, 0], shift_px[1] * c[2] / sK[1, 1], 0.0])
    Q = (P - c) @ R.T + c + t
    u = np.rint(Q[:, 0] / Q[:, 2] * sK[0, 0] + sK[0, 2]).astype(int)
    v = np.rint(Q[:, 1] / Q[:, 2] * sK[1, 1] + sK[1, 2]).astype(int)
    out = np.zeros((H, W), np.float64)
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    order = np.argsort(-Q[ok, 2])                                 # far first: the nearest point is written last
    zz = Q[ok, 2] + rng.normal(0, 1.0, int(ok.sum()))
    out[v[ok][order], u[ok][order]] = zz[order]
    return out


def shift_layer(L, dx, dy):
    """The layer moved by whole pixels; what leaves the frame is cut off."""
    out = np.zeros_like(L)
    ys, xs = np.nonzero(L)
    u, v = xs + dx, ys + dy
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    out[v[ok], u[ok]] = L[ys[ok], xs[ok]]
    return out


CORNER_OVERHANG = 2             # pixels of the top-left object beyond column 0 and row 0 (edge_case)


def compose(layers):
    sd = np.zeros((H, W), np.float64)
    for L in layers:
        sd = np.where(L > 0, L, sd)
    return np.clip(np.rint(sd), 0, 65535).astype(np.uint16)


def window_of(md, layer):
    """detect (x, y) that puts the model's dilated window over the layer: the scene pixel of model pixel (x, y) is
    (x - min x + detect_x, y - min y + detect_y) (LL.cpp:64-66 with the 4-pixel dilation)."""
    ys, xs = np.nonzero(layer)
    return int(xs.min()), int(ys.min())


def clamped_reads_with_depth(md, scene, dx, dy):
    """Scene pixels with depth that the window at (dx, dy) reads through the clamp max(. - 4, 0) (LL.cpp:64-66): pixels of the
    model's dilated mask whose scene row or column would lie above or left of the frame."""
    from scipy.ndimage import maximum_filter
    mask = maximum_filter((md > 0).astype(np.uint8), size=9, mode="constant", cval=0)
    ys, xs = np.nonzero(mask)
    bx, by = int(xs.min()), int(ys.min())
    r, c = np.mgrid[0:int(ys.max()) - by + 1, 0:int(xs.max()) - bx + 1]
    sr, sc = r + dy - 4, c + dx - 4
    clamped = (mask[r + by, c + bx] > 0) & ((sr < 0) | (sc < 0))
    return int((scene[np.maximum(sr, 0), np.maximum(sc, 0)][clamped] > 0).sum())


def dilated_box(md):
    from scipy.ndimage import maximum_filter
    ys, xs = np.nonzero(maximum_filter((md > 0).astype(np.uint8), size=9, mode="constant", cval=0))
    return int(xs.max()) - int(xs.min()) + 1, int(ys.max()) - int(ys.min()) + 1


class Case:
    """One scene and its hypotheses (model images, cameras, poses, windows)."""

    def __init__(self, scene):
        self.scene = scene
        self.mds, self.Ks, self.Rs, self.ts, self.xy, self.names = [], [], [], [], [], []

    def add(self, name, md, mK, R, t, xy):
        self.names.append(name); self.mds.append(md); self.Ks.append(np.asarray(mK, np.float32))
        self.Rs.append(np.asarray(R, np.float32)); self.ts.append(np.asarray(t, np.float32)); self.xy.append((int(xy[0]), int(xy[1])))

    def subset(self, idx):
        c = Case(self.scene)
        for i in idx:
            c.add(self.names[i], self.mds[i], self.Ks[i], self.Rs[i], self.ts[i], self.xy[i])
        return c

    def arrays(self):
        n = len(self.mds)
        return (np.stack(self.Ks).reshape(n, 9), np.stack(self.Rs).reshape(n, 9), np.stack(self.ts).reshape(n, 3), self.xy)


def _pose(rng):
    return rand_rot(rng), np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), 1000 + rng.uniform(-30, 30)], np.float32)


def main_case():
    """One frame, nine objects: four small (whole target cloud in LDS), three medium (~2k source points: more than 704
    per member of a team of two), one large (a 4-8k point target cloud: the slab build), and one striped model whose scene
    window holds about twice its points (a slab that overflows when one workgroup serves it: global mode)."""
    rng = np.random.default_rng(100)
    layers, hyps = [], []
    specs = [("small%d" % k, dict(a=22 + 2 * k, b=18 + k), (-250 + 120 * k, 150)) for k in range(4)]
    specs += [("medium%d" % k, dict(a=34 - k, b=28), (-230 + 150 * k, 20)) for k in range(3)]
    specs += [("large", dict(a=56, b=46), (-200, -140)), ("striped", dict(a=54, b=45, stripes=True), (150, -140))]
    for k, (name, kw, shift) in enumerate(specs):
        md = bump(300 + k, **kw)
        mK = model_K(rng)
        full = bump(300 + k, **{q: v for q, v in kw.items() if q != "stripes"})   # the object itself: the stripes are holes of the model only
        L = place(full, mK, shift, 500 + k)
        layers.append(L)
        R, t = _pose(rng)
        ys, xs = np.nonzero(md)
        fy, fx = np.nonzero(full)
        # window: the model's mask box over the layer (the stripes do not move the box: its first column is a full one or within the dilation)
        dx, dy = window_of(full, L)
        dx += int(xs.min()) - int(fx.min()); dy += int(ys.min()) - int(fy.min())
        hyps.append((name, md, mK, R, t, (dx, dy)))
    c = Case(compose(layers))
    for h in hyps:
        c.add(*h)
    return c


def edge_case():
    """Inputs the other tests never vary, in one batch with ordinary hypotheses: windows at the frame's edges (the clamp of
    scene pixels at x, y < 4, over an object that overhangs column 0 and row 0; at the right and bottom edges the last window
    taken, detect_x + bw = W - 1, and the first rejected, detect_x + bw >= W with bw the width of the dilated box, LL.cpp:52-55;
    the same in y), a model whose centre pixel is off the object and one more than 0.4 m from every scene point (both: a NaN
    init guess, as the reference has)."""
    rng = np.random.default_rng(200)
    md_a = bump(400, 26, 21)
    bw, bh = dilated_box(md_a)
    ys, xs = np.nonzero(md_a)
    ow, oh = int(xs.max()) - int(xs.min()), int(ys.max()) - int(ys.min())
    x0, y0 = int(xs.min()), int(ys.min())
    mKs = [model_K(rng) for _ in range(4)]
    # top-left corner: the object overhangs column 0 and row 0 of the scene by CORNER_OVERHANG pixels, so that the scene pixels a
    # window at detect (0..3, 0) reads through the clamp max(. - 4, 0) carry depth
    L_tl = place(md_a, mKs[0], (-x0, -y0), 600)
    ly, lx = np.nonzero(L_tl)
    L_tl = shift_layer(L_tl, -int(lx.min()) - CORNER_OVERHANG, -int(ly.min()) - CORNER_OVERHANG)
    # right edge: a window at detect_x = W - 1 - bw (the last one taken; detect_x + bw >= W is rejected) puts the object's right
    # end near column W - 10
    L_r = place(md_a, mKs[1], (W - 10 - ow - x0 - (bw - 9 - ow), 0), 601)
    # bottom edge
    L_b = place(md_a, mKs[2], (-150, H - 10 - oh - y0 - (bh - 9 - oh)), 602)
    # an ordinary one in the middle
    L_m = place(md_a, mKs[3], (120, 60), 603)
    c = Case(compose([L_tl, L_r, L_b, L_m]))
    for dxx in (0, 1, 3):
        c.add("corner x=%d" % dxx, md_a, mKs[0], *_pose(rng), (dxx, 0))
    ly = np.nonzero(L_r)[0]
    c.add("right, last taken", md_a, mKs[1], *_pose(rng), (W - 1 - bw, int(ly.min())))        # detect_x + bw = W - 1
    c.add("right, rejected", md_a, mKs[1], *_pose(rng), (W - bw, int(ly.min())))              # detect_x + bw = W
    lx = np.nonzero(L_b)[1]
    c.add("bottom, last taken", md_a, mKs[2], *_pose(rng), (int(lx.min()), H - 1 - bh))
    c.add("bottom, rejected", md_a, mKs[2], *_pose(rng), (int(lx.min()), H - bh))
    c.add("middle", md_a, mKs[3], *_pose(rng), window_of(md_a, L_m))
    off = bump(401, 24, 20, centre=(150, 40))                     # centre pixel off the object
    c.add("centre off object", off, mKs[3], *_pose(rng), window_of(md_a, L_m))
    far = bump(402, 26, 21, z0=1600.0)                            # > 0.4 m behind every scene point of its window
    c.add("model 0.6 m away", far, mKs[3], *_pose(rng), window_of(md_a, L_m))
    c.add("middle again", md_a, mKs[3], *_pose(rng), window_of(md_a, L_m))
    return c


def surface_case(half_w, half_h, seed):
    md = surface(half_w, half_h)
    L = place(md, K_CAM, (0, 0), seed, rot_deg=1.5, t_mm=(3.0, -2.0, 4.0))
    c = Case(compose([L]))
    ys, xs = np.nonzero(md)
    c.add("surface %dx%d" % (2 * half_w - 1, 2 * half_h - 1), md, K_CAM, *_pose(np.random.default_rng(seed)), (int(xs.min()), int(ys.min())))
    return c


# ---- the oracle, once per distinct hypothesis ------------------------------------------------------
_ORACLE = {}


def oracle(case, i):
    key = (h16(case.scene), h16(case.mds[i]), case.Ks[i].tobytes(), case.Rs[i].tobytes(), case.ts[i].tobytes(), case.xy[i])
    if key not in _ORACLE:
        x, y = case.xy[i]
        big = max(int((case.mds[i] > 0).sum()), int((case.scene[y:y + 200, x:x + 200] > 0).sum())) > 3000
        nn = "kdtree" if big else "brute"                             # (exact either way: tests/test_oracle_icp.py)
        _ORACLE[key] = lo.pose_refine(case.scene, case.mds[i], K_CAM, case.Ks[i], case.Rs[i], case.ts[i], case.xy[i][0], case.xy[i][1],
                                      scene_from_scene=True, nn=nn)
    return _ORACLE[key]


# ---- the product, in this process or in one of its own (knobs) ------------------------------------
def run_icp(case, slots=None, reps=1):
    """IcpContext.run on the case: result dicts with build, team_note, team_size and resume_it of every hypothesis."""
    import linemodLevelup_pybind as mod
    Ks, Rs, ts, xy = case.arrays()
    ctx = mod.IcpContext(device=0, scene_from_scene=True)
    try:
        ctx.set_scene(case.scene, K_CAM)
        if slots is None:
            ctx.set_models(case.mds)
        else:
            ctx.set_models(case.mds[:max(slots) + 1])
        for _ in range(reps):
            res, _ = ctx.run(Ks, Rs, ts, xy, model_slots=slots)
        out = []
        for h, r in enumerate(res):
            d = ctx.read_debug(h, 3)
            out.append({"R": None if r["R"] is None else np.asarray(r["R"], np.float64).tolist(),
                        "t": None if r["t"] is None else np.asarray(r["t"], np.float64).ravel().tolist(),
                        "residual": float(r["residual"]), "iterations": int(r["iterations"]), "n_source": int(r["n_source"]),
                        "n_target": int(r["n_target"]), "stage": int(r["stage"]), "build": int(d[DBG3_BUILD]),
                        "team_note": [int(v) for v in d[DBG3_TEAM_NOTE:DBG3_TEAM_NOTE + 4]], "team_size": int(d[DBG3_TEAM_SIZE]),
                        "resume_it": int(d[DBG3_RESUME_IT])})
        return out
    finally:
        ctx.close()


_WORKER = r"""
import json, os, sys
import numpy as np
root, case_file = sys.argv[1], sys.argv[2]
sys.path[:0] = [root, os.path.join(root, "6dpose_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")]
import test_gpu_icp_oracle as T
z = np.load(case_file)
c = T.Case(z["scene"])
for i in range(len(z["mds"])):
    c.add(str(i), z["mds"][i], z["Ks"][i], z["Rs"][i], z["ts"][i], tuple(z["xy"][i]))
print("RESULT " + json.dumps(T.run_icp(c)))
"""


def run_icp_env(case, env, tmp_path):
    """run_icp in a process of its own with the given LM_ICP_* knobs (read once per process)."""
    f = tmp_path / ("case_%s.npz" % "_".join("%s%s" % kv for kv in sorted(env.items())))
    np.savez(f, scene=case.scene, mds=np.stack(case.mds), Ks=np.stack(case.Ks), Rs=np.stack(case.Rs), ts=np.stack(case.ts), xy=np.array(case.xy))
    script = tmp_path / "icp_worker.py"
    script.write_text(_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT, str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, **env))
    text = r.stdout.decode()
    assert r.returncode == 0, text[-3000:]
    return json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])


# ---- the bar -----------------------------------------------------------------------------------------
def describe(name, g):
    return "%-22s stage %d build %-2d (%s) team %2d note %s resume %d it %2d n %d/%d" % (
        name, g["stage"], g["build"], BUILD_NAMES.get(g["build"], "?"), g["team_size"], g["team_note"], g["resume_it"], g["iterations"],
        g["n_source"], g["n_target"])


def compare(case, got, label):
    """Every hypothesis against the oracle (the bar in the module docstring); prints the served path of each."""
    assert len(got) == len(case.mds)
    ill, lines = [], []
    for i, g in enumerate(got):
        ref = oracle(case, i)
        name = case.names[i]
        lines.append(describe(name, g))
        if ref["residual"] == -1.0:                                   # the window leaves the frame (LL.cpp:52-55)
            assert g["residual"] == -1.0 and g["stage"] == 0, (label, name, g)
            continue
        ctx = "%s / %s: %s" % (label, name, lines[-1])
        assert g["n_source"] == ref["n_source"] and g["n_target"] == ref["n_target"], (ctx, ref["n_source"], ref["n_target"])
        R, t = np.array(g["R"]), np.array(g["t"])
        if not np.all(np.isfinite(ref["R"])) or not np.all(np.isfinite(ref["t"])):   # a NaN init guess: NaN exactly where the oracle has it
            assert np.array_equal(np.isnan(R), np.isnan(ref["R"])) and np.array_equal(np.isnan(t), np.isnan(ref["t"])), ctx
            assert g["residual"] == ref["residual"] and g["iterations"] == ref["iterations"], (ctx, ref["residual"], ref["iterations"])
            continue
        why = lo.ill_posed(ref["history"])
        if why:
            ill.append("%s: %s" % (name, why))
            continue
        assert g["iterations"] == ref["iterations"], (ctx, ref["iterations"])
        assert abs(g["residual"] - ref["residual"]) < 1e-6, (ctx, g["residual"], ref["residual"])
        assert np.abs(R - ref["R"]).max() < 1e-4, (ctx, np.abs(R - ref["R"]).max())
        assert np.abs(t - ref["t"]).max() / 1000.0 < 1e-4, (ctx, np.abs(t - ref["t"]).max())
    print("\n[%s]\n  " % label + "\n  ".join(lines))
    if ill:
        print("  ill-posed by the oracle's evidence: " + "; ".join(ill))
    assert 4 * len(ill) <= len(got), (label, ill)
    return lines


@pytest.fixture(scope="module")
def main():
    return main_case()


def _idx(case, prefix):
    return [i for i, n in enumerate(case.names) if n.startswith(prefix)]


# ---- §3: each build against the oracle ---------------------------------------------------------------------
def test_one_point_whole_cloud(lm, main):
    c = main.subset(_idx(main, "small"))
    got = run_icp(c)
    compare(c, got, "1-point, whole")
    assert all(g["stage"] == 1 and g["build"] == 4 for g in got), [describe(n, g) for n, g in zip(c.names, got)]


def test_one_point_slab(lm, main):
    c = main.subset(_idx(main, "large"))
    got = run_icp(c)
    compare(c, got, "1-point, slab")
    assert got[0]["stage"] == 1 and got[0]["build"] == 7 and 4000 <= got[0]["n_target"] <= 8000, describe("large", got[0])


def test_mixed_batch_takes_the_slab_build_for_all(lm, main):
    """One slab-sized cloud among whole ones: the build without a slab takes a batch only whole (__ballot(big) in k_icp_team)."""
    c = main.subset(_idx(main, "small")[:3] + _idx(main, "large"))
    got = run_icp(c)
    compare(c, got, "mixed batch")
    assert all(g["stage"] == 1 and g["build"] in (6, 7) for g in got), [describe(n, g) for n, g in zip(c.names, got)]
    assert got[-1]["build"] == 7 and all(g["build"] == 6 for g in got[:-1])


def test_two_point_build(lm, main, tmp_path):
    c = main.subset(_idx(main, "medium"))
    got = run_icp_env(c, {"LM_ICP_BUILDS": "4", "LM_ICP_TEAM": "2"}, tmp_path)
    compare(c, got, "2-point (LM_ICP_BUILDS=4 LM_ICP_TEAM=2)")
    assert all(g["stage"] == 1 and g["build"] in (10, 11) and g["team_size"] == 2 for g in got), [describe(n, g) for n, g in zip(c.names, got)]
    assert all(g["n_source"] > 2 * 704 for g in got)                  # (more than the one-point builds hold per member)


def test_five_point_build_and_global_mode(lm, main, tmp_path):
    """LM_ICP_BUILDS=8 LM_ICP_TEAM=1: the five-point build, one workgroup per hypothesis.  The striped model has at most 3520
    source points but its window holds more targets than the slab holds (C): its workgroup reads them from global memory
    (team_note 3: member, targets needed, capacity)."""
    c = main.subset(_idx(main, "medium") + _idx(main, "striped"))
    got = run_icp_env(c, {"LM_ICP_BUILDS": "8", "LM_ICP_TEAM": "1"}, tmp_path)
    compare(c, got, "5-point (LM_ICP_BUILDS=8 LM_ICP_TEAM=1)")
    assert all(g["stage"] == 1 and g["build"] in (22, 23) and g["team_size"] == 1 for g in got), [describe(n, g) for n, g in zip(c.names, got)]
    s = got[-1]
    assert s["n_source"] <= 5 * 704 and s["team_note"][0] == 3 and s["build"] == 23 and s["team_note"][2] > s["team_note"][3], describe("striped", s)


def test_cut_and_relaunch(lm, main):
    """40 hypotheses of the frame (each object five times, windows as found): a cramped batch that leaves the first launch
    after evaluation 3 and resumes in the second from IcpState; every hypothesis against the oracle, the resumed ones counted."""
    n = 40
    base = _idx(main, "small") + _idx(main, "medium") + _idx(main, "large")
    c = main.subset([base[h % len(base)] for h in range(n)])
    got = run_icp(c)
    compare(c, got, "cut and relaunch (40 hypotheses)")
    resumed = [g for g in got if g["resume_it"] > 0]
    assert all(g["stage"] == 1 for g in got) and len(resumed) >= 8, [describe(nm, g) for nm, g in zip(c.names, got)]
    assert all(g["build"] in (6, 7) for g in resumed)                 # (the relaunch is the slab build alone)


def test_sliced_launches_knob(lm, main, tmp_path):
    c = main.subset(_idx(main, "small")[:2] + _idx(main, "medium")[:1] + _idx(main, "large"))
    got = run_icp_env(c, {"LM_ICP_SLICED": "1"}, tmp_path)
    compare(c, got, "sliced (LM_ICP_SLICED=1)")
    assert all(g["stage"] == 3 and g["build"] == 0 for g in got)


@pytest.mark.parametrize("half_w,half_h,stage", [(130, 110, 2), (150, 120, 3)])
def test_large_curved_clouds(lm, half_w, half_h, stage):
    """56.7k points (more than 704 per member of a team of 64: the large builds, stage 2) and 71k (more targets than the
    16-bit cell table of k_icp_team addresses: the sliced launches, stage 3), registered non-identically on a curved,
    rippled surface; the oracle in its exact KD-tree mode."""
    c = surface_case(half_w, half_h, 700 + half_w)
    got = run_icp(c)
    compare(c, got, "large cloud, stage %d" % stage)
    g = got[0]
    assert g["stage"] == stage, describe(c.names[0], g)
    if stage == 2:
        assert g["build"] in (10, 11, 22, 23) and g["n_source"] > 64 * 704, describe(c.names[0], g)
    else:
        assert g["build"] == 0 and g["n_target"] > 65535, describe(c.names[0], g)


# ---- §4: the inputs the suite never varied --------------------------------------------------------------
def test_cameras_poses_windows_and_nan_guesses(lm):
    """One batch through IcpContext.run and the same hypotheses one by one through poseRefine.process: model cameras unlike
    the scene's, random model R with t.x, t.y != 0 (only t.z is divided by 1000, LL.cpp:37), windows at the frame's edges,
    NaN init guesses."""
    import linemodLevelup_pybind as mod
    c = edge_case()
    # the corner windows reach the clamp of scene pixels at x, y < 4 over depth, so a kernel that skipped, shifted or disagreed
    # about those reads would change the target cloud
    bw, bh = dilated_box(c.mds[0])
    assert (c.scene[0:bh, 0] > 0).any() and (c.scene[0, 0:bw] > 0).any()
    for i in range(3):
        assert c.names[i].startswith("corner") and clamped_reads_with_depth(c.mds[i], c.scene, *c.xy[i]) > 0, c.names[i]
    got = run_icp(c)
    compare(c, got, "cameras, poses, windows, NaN guesses (batch)")
    rejected = [n for n, g in zip(c.names, got) if g["residual"] == -1.0]
    assert rejected == ["right, rejected", "bottom, rejected"], rejected
    nan = [n for n, g in zip(c.names, got) if np.isnan(np.array(g["R"])).any()]
    assert nan == ["centre off object", "model 0.6 m away"], nan
    assert all(np.isfinite(oracle(c, i)["init_guess"]).all() == (c.names[i] not in nan) for i in range(len(c.names)) if c.names[i] not in rejected)
    one = []
    for i in range(len(c.mds)):
        pr = mod.poseRefine(device=0, scene_from_scene=True)          # (a rejected window leaves a poseRefine's outputs untouched)
        pr.process(c.scene, c.mds[i], K_CAM, c.Ks[i], c.Rs[i], c.ts[i], c.xy[i][0], c.xy[i][1])
        inf = pr.info
        one.append({"R": None if pr.getR() is None else np.asarray(pr.getR(), np.float64).tolist(),
                    "t": None if pr.getT() is None else np.asarray(pr.getT(), np.float64).ravel().tolist(),
                    "residual": float(pr.getResidual()), "iterations": int(inf.get("iterations", 0)), "n_source": int(inf.get("n_source", 0)),
                    "n_target": int(inf.get("n_target", 0)), "stage": int(inf.get("stage", 0)), "build": -1, "team_note": [], "team_size": 0,
                    "resume_it": 0})
    compare(c, one, "cameras, poses, windows, NaN guesses (poseRefine.process)")
    for n, g, o in zip(c.names, got, one):                            # the batch and the lone calls: the same hypothesis, the same path
        assert g["residual"] == o["residual"] and (g["residual"] == -1.0 or (g["iterations"] == o["iterations"] and g["stage"] == o["stage"])), n


# ---- §5: BASELINE configs[2] at size: 2000 templates -> NMS 0.5 -> top-16 -> poseRefine --------------------
def config2_frame(n_templates=2000, n_bumps=24, seed=17):
    """A 640x480 frame whose depth holds n_bumps objects (each a bump of its own model image, moved rigidly and seen through
    the scene camera), and a bank of templates cut out of the frame at the objects' boxes.  View of template i: the model
    image of its object (a camera unlike the scene's), a random R and t."""
    rng = np.random.default_rng(seed)
    rgb, dep = synth.make_frame(seed, W, H)
    layers, mds, mKs, boxes = [], [], [], []
    cols, rows = 6, 4
    for b in range(n_bumps):
        md = bump(800 + b, rng.uniform(20, 27), rng.uniform(17, 22))
        mK = model_K(rng)
        cx = 60 + (b % cols) * 104 + rng.uniform(-4, 4)
        cy = 62 + (b // cols) * 118 + rng.uniform(-4, 4)
        L = place(md, mK, (cx - W / 2, cy - H / 2), 900 + b)
        ys, xs = np.nonzero(L)
        layers.append(L); mds.append(md); mKs.append(mK)
        boxes.append((int(xs.min()), int(ys.min()), int(xs.max()) - int(xs.min()) + 1, int(ys.max()) - int(ys.min()) + 1))
    scene = compose(layers)
    # the background 0.8 m further back: more than the 0.4 m of the reference's centroid test (LL.cpp:92) behind the objects
    dep = np.where(scene > 0, scene, np.where(dep > 0, dep.astype(np.int64) + 800, 0)).astype(np.uint16)
    rgb = rgb.copy()                                                    # a painted object: colour edges all over it (the colour features)
    for (x0, y0, w, h) in boxes:
        cells = rng.integers(30, 226, ((h + 5) // 6, (w + 5) // 6, 3)).astype(np.uint8)
        rgb[y0:y0 + h, x0:x0 + w] = np.repeat(np.repeat(cells, 6, 0), 6, 1)[:h, :w]
    views = []
    for i in range(n_templates):
        views.append((mds[i % n_bumps], mKs[i % n_bumps].astype(np.float32), *_pose(rng)))
    return rgb, dep, views, [boxes[i % n_bumps] for i in range(n_templates)]


def test_config2_2k_templates_nms_top16_pose_refine(lm):
    """BASELINE configs[2]: Pipeline.run (match 2000 templates, NMS 0.5, top 16, poseRefine on the device) against the
    oracle-only chain (match_oracle.c, canonical sort / unique, the driver's nms, oracle pose_refine): the 16 detections
    exact, the poses to the ICP bar, at least 12 of the 16 well-posed by the oracle's evidence."""
    T, nfeat, thr, top_k = [4, 8], (150, 75), 75.0, 16
    rgb, dep, views, windows = config2_frame()
    od = lo.OracleDetector(nfeat[0], T)
    pyr = od.quantize_pyramid(rgb, dep)
    feat, offs, wh = synth.make_planted_bank(2024, len(views), [(p[0], p[1]) for p in pyr], T, nfeat, windows=windows)
    E = 2 * len(T)
    det = lm.Detector(nfeat[0], T, device=0)
    det.addClassPacked("obj", feat, offs, wh)
    pipe = lm.Pipeline(det, W, H, scene_from_scene=True)
    try:
        pipe.set_views("obj", [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views])
        det.setFrame([rgb, dep])
        got, _ = pipe.run(thr, ["obj"], K_CAM, top_k=top_k, nms_iou=0.5)
        dbg = [pipe.read_icp_debug(h, 3) for h in range(len(got))]
    finally:
        pipe.close()
    osel, oposes = pipeline_oracle(od, rgb, dep, (feat, offs, wh), T, wh, E, views, thr, top_k, 0.5)
    assert len(got) == len(osel) == top_k
    for g, r in zip(got, osel):
        assert (g["x"], g["y"], g["template_id"], g["similarity"]) == (int(r["x"]), int(r["y"]), int(r["tid"]), float(r["sim"]))
    # the poses: the same bar as every other case, hypothesis by hypothesis (Case = the frame and the 16 detections' views)
    c = Case(dep)
    for g in got:
        md, K, R, t = views[g["template_id"]]
        c.add("tid %d at (%d, %d)" % (g["template_id"], g["x"], g["y"]), md, K, R, t, (g["x"], g["y"]))
    for i, p in enumerate(oposes):                                     # (the oracle chain's poses are the cache's)
        _ORACLE.setdefault((h16(c.scene), h16(c.mds[i]), c.Ks[i].tobytes(), c.Rs[i].tobytes(), c.ts[i].tobytes(), c.xy[i]), p)
    rows = []
    for g, d in zip(got, dbg):
        rows.append({"R": np.asarray(g["R"], np.float64).tolist(), "t": np.asarray(g["t"], np.float64).ravel().tolist(), "residual": g["residual"],
                     "iterations": g["iterations"], "n_source": g["n_source"], "n_target": g["n_target"], "stage": g["stage"],
                     "build": int(d[DBG3_BUILD]), "team_note": [int(v) for v in d[DBG3_TEAM_NOTE:DBG3_TEAM_NOTE + 4]],
                     "team_size": int(d[DBG3_TEAM_SIZE]), "resume_it": int(d[DBG3_RESUME_IT])})
        assert g["status"] == 0, describe("status %d" % g["status"], rows[-1])
    compare(c, rows, "configs[2]: 2000 templates, NMS 0.5, top-16")
    well = sum(1 for i in range(top_k) if not lo.ill_posed(oracle(c, i)["history"]))
    assert well >= 12, well
