"""Who owns device and pinned host memory (csrc/dev_buf.h): lm_mesh, its pose-error scratch, lm_pso, lm_icp, lm_pipeline and the
detector's staging buffer, ingest ring and result slots (`-m gpu`).

DevBuf<T> and PinBuf<T> alone are checked by the stand-alone program tests/cpp/dev_buf_cases.cpp, built here next to the header it tests;
DevStream and DevEvent, which own every stream and event of the same contexts, by tests/cpp/dev_handle_cases.cpp.  The lifecycle tests at
the end open and close every context several times in one process, close a detector with frames in flight and after its lazily created
handles have been made, and compare what the next context answers with what the first one did.

The grow-and-reuse tests make ONE context serve a small call, then a larger call under which every scratch buffer of that path has to be
replaced by a larger one, then the small call again, and compare each answer with the same call on a context that has served nothing else.
A buffer that kept its old capacity, its old pointer in a kernel argument, or a stale capacity after it was replaced shows as a difference
(or as a fault).  The comparisons are exact: these paths use integer atomics and sums in a fixed order, and two fresh contexts agree bit for
bit."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pso_cases as pc
import pso_edge_cases as ec
import synth
from synth import icosphere

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def run_alone(name, tmp_path):
    """Builds tests/cpp/<name>.cpp next to the header it tests, with the library's flags and -Werror, and runs it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "6dpose_amd", "csrc"), "-x", "hip", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe],
                          timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"ok:" in r.stdout, r.stdout.decode()[-2000:]


def test_dev_buf_alone(lm, tmp_path):
    """ensure(0) allocates nothing; ensure(m <= n) keeps pointer and cap; growth gives cap == n; release() twice; both moves leave the
    source {nullptr, 0}; a std::vector<DevBuf> that reallocates keeps every pointer and what was written through it.  The same for
    PinBuf, written and read through the host pointer."""
    run_alone("dev_buf_cases", tmp_path)


def test_dev_handles_alone(lm, tmp_path):
    """DevStream and DevEvent: no copies, nothrow moves; a default-constructed handle is null; ensure() creates one and a second ensure()
    keeps it; release() twice; both moves leave the source null; a std::vector<DevEvent> that reallocates keeps every handle.  A stream
    of each creation form takes a 256-byte memset and has the priority it was created with; two default events time the memset; an
    event of each of the three flag kinds is recorded, waited on from a second stream and synchronised."""
    run_alone("dev_handle_cases", tmp_path)


# ---- the shared scene: the 80-triangle icosphere of radius 40 mm, about 400 mm from the camera ----------------------------------
def cam(W, H):
    """A camera under which the sphere is a third of a W x H frame high."""
    f = H * 400.0 / 240.0
    return np.array([f, 0, W / 2.0 - 0.3, 0, f, H / 2.0 + 0.2, 0, 0, 1], np.float64).reshape(3, 3)


def poses(n, seed):
    """n poses side by side, 50 mm from the first to the last (the spheres overlap, each shows), each 3 mm behind the one before."""
    rng = np.random.RandomState(seed)
    Rs = np.stack([pc.rot(rng.uniform(-1, 1, 3), rng.uniform(-80, 80)) for _ in range(n)])
    ts = np.array([[-25.0 + 50.0 * i / max(n - 1, 1), -10.0 + 5.0 * i, 400.0 + 3.0 * i] for i in range(n)])
    return Rs, ts


def estimates(Rg, tg, n):
    """The first n ground truths, 2 degrees and a few mm off."""
    return np.stack([pc.rot((1, -2, 1), 2.0) @ R for R in Rg[:n]]), tg[:n] + np.array([2.0, -1.0, 3.0])


def full_mesh(lm):
    V, F, N, C = icosphere(1, radius=40.0, seed=5)
    return lm.Mesh(V, F, normals=N, colors=C)


def same(a, b):
    """Bit-equal, for arrays, scalars and the containers the wrappers return."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def grow_and_reuse(make, small, large):
    """small, large, small on one context; each against the same call on a fresh one."""
    used, want_small, want_large = make(), small(make()), large(make())
    assert same(small(used), want_small), "first call"
    assert same(large(used), want_large), "the call under which every buffer grows"
    assert same(small(used), want_small), "the small call again, in the grown buffers"
    assert same(large(used), want_large), "and the large one, now without growth"


# ---- lm_mesh -----------------------------------------------------------------------------------------------------------------
def test_render_grows_and_reuses(lm):
    """2 views at 32 x 24 and ssaa 1, then 5 views at 64 x 48 and ssaa 3: views, projected vertices, depth and colour grow with the
    call, the z-buffer by another factor of 9."""
    def call(n, W, H, ssaa):
        Rs, ts = poses(n, 11)
        return lambda m: m.render((W, H), cam(W, H), Rs, ts, clip_near=100.0, clip_far=2000.0, ssaa=ssaa)
    small, large = call(2, 32, 24, 1), call(5, 64, 48, 3)
    grow_and_reuse(lambda: full_mesh(lm), small, large)
    rgb, depth = large(full_mesh(lm))
    assert all((depth[i] > 0).sum() > 100 and rgb[i].any() for i in range(5))            # the comparison is not one of empty images


def test_overlay_grows_and_reuses(lm):
    """1 layer on a 32 x 24 frame, then 3 layers on 64 x 48, both with per-pose colours and a scene depth that hides part of a pose:
    the layer table, the frame, the scene, both outputs and the per-view colours grow."""
    def call(n, W, H):
        Rs, ts = poses(n, 23)
        rng = np.random.RandomState(n)
        frame = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        scene = np.full((H, W), 2000, np.uint16); scene[:, : W // 2] = 390
        colours = rng.uniform(0, 1, (n, 3))
        return lambda m: m.overlay(frame, cam(W, H), Rs, ts, surf_colors=colours, scene_depth=scene, mode="nearest", hide_occluded=True)
    small, large = call(1, 32, 24), call(3, 64, 48)
    grow_and_reuse(lambda: full_mesh(lm), small, large)
    _, index = large(full_mesh(lm))
    assert set(np.unique(index)) == {-1, 0, 1, 2}


def test_pose_errors_grow_and_reuse(lm):
    """1 pair on a 32 x 24 scene, then 9 pairs on 64 x 48 with VSD on, then MSSD / MSPD — under 2 symmetries in the pair buffer as the
    point metrics left it, under 8 in one that has to grow once more (other records in the same bytes) — and the GT statistics, which
    keep a third record type in the partials."""
    def scene(W, H, Rs, ts):
        d = full_mesh(lm).render((W, H), cam(W, H), Rs[:1], ts[:1], clip_near=100.0, clip_far=2000.0, mode="depth")[0].astype(np.float32)
        d[d > 0] += 3.0
        d[::5] = 0.0
        return d

    def call(ne, ng, W, H):
        Rg, tg = poses(ng, 37)
        Re, te = estimates(Rg, tg, ne)
        s = scene(W, H, Rg, tg)
        return lambda m: lm.pose_errors(m, Re, te, Rg, tg, K=cam(W, H), scene_depth=s, cost="tlinear")

    def sym(n_sym):
        Rg, tg = poses(3, 37)
        Re, te = estimates(Rg, tg, 3)
        S = (np.stack([pc.rot((0, 0, 1), 360.0 * k / n_sym) for k in range(n_sym)]), np.zeros((n_sym, 3)))
        return lambda m: lm.pose_errors(m, Re, te, Rg, tg, K=cam(64, 48), metrics=("mssd", "mspd"), symmetries=S)

    def stats(ng, W, H):
        Rg, tg = poses(ng, 37)
        s = scene(W, H, Rg, tg)
        return lambda m: lm.gt_stats(m, Rg, tg, cam(W, H), s)

    small, large, sym2, sym8, gt1, gt4 = call(1, 1, 32, 24), call(3, 3, 64, 48), sym(2), sym(8), stats(1, 32, 24), stats(4, 64, 48)
    fresh = lambda: lm.Mesh(*pc.mesh())
    used = fresh()
    for name, f in (("1 pair", small), ("9 pairs", large), ("2 symmetries", sym2), ("8 symmetries", sym8), ("1 pair again", small), ("1 GT", gt1),
                    ("4 GTs", gt4), ("9 pairs again", large), ("2 symmetries again", sym2), ("1 GT again", gt1)):
        assert same(f(used), f(fresh())), name
    e = large(fresh())
    assert sorted(e) == ["add", "adi", "cou", "re", "te", "vsd"] and all(v.shape == (3, 3) for v in e.values())
    assert 0.0 < e["vsd"].min() < 1.0 and e["add"].min() > 0.0                            # rendered, and compared with a scene that is there


# ---- lm_pso ------------------------------------------------------------------------------------------------------------------
def swarm(ctx, mesh, n, window, **options):
    Rs, ts = pc.hypotheses()
    got, _ = ctx.run(mesh, Rs[:n], ts[:n], pc.WINDOWS[:n], window, seed=pc.SEED, tau=options.pop("tau", pc.TAU), **options)
    return got, [[ctx.read_debug(h, k) for k in ("x", "cost", "sum_n_r", "best")] for h in range(n)]


def test_pso_grows_and_reuses(lm):
    """1 hypothesis x 8 particles x 2 generations in a 32 x 32 window on a 72 x 60 scene, then 3 x 16 x 3 in 48 x 40 on the whole
    96 x 80 scene: the scene, the swarm's state, its render scratch and the record of every generation grow; what read_debug returns
    comes from the buffers of the last run."""
    mesh = lm.Mesh(*pc.mesh())

    def call(n, P, G, window, crop):
        def f(ctx):
            ctx.set_scene(pc.scene()[:crop[1], :crop[0]], pc.K)
            return swarm(ctx, mesh, n, window, particles=P, generations=G)
        return f
    grow_and_reuse(lambda: lm.PsoContext(0), call(1, 8, 2, (32, 32), (72, 60)), call(3, 16, 3, pc.WIN, (pc.W, pc.H)))
    got, _ = call(3, 16, 3, pc.WIN, (pc.W, pc.H))(lm.PsoContext(0))
    assert all(g["n_rendered"] > 100 and g["cost"] <= g["initial_cost"] for g in got)


def test_pso_edge_scene_grows_and_reuses(lm):
    """The edge scene at 72 x 60, then at 96 x 80: the map, its row distances and the squared distance grow; the distance read back and
    a swarm scored against it."""
    mesh = lm.Mesh(*pc.mesh())

    def call(n, crop):
        def f(ctx):
            ctx.set_scene_edges(ec.edge_scene()[:crop[1], :crop[0]], pc.K, ec.M)
            return ctx.edge_distance(), swarm(ctx, mesh, n, (32, 32), particles=8, generations=2, tau=ec.TAU, cost="edges")
        return f
    grow_and_reuse(lambda: lm.PsoContext(0), call(1, (72, 60)), call(3, (pc.W, pc.H)))
    d2, _ = call(3, (pc.W, pc.H))(lm.PsoContext(0))
    assert np.array_equal(d2, ec.scene_d2())


# ---- lm_icp ------------------------------------------------------------------------------------------------------------------
DBG3_NO_CLOCKS = list(range(0, 25)) + list(range(33, 39)) + [47, 48] + list(range(65, 73))   # kind 3 without clk, knn_clk, vox_clk, sort_clk


def icp_scene(seed, n_models, W, H):
    """n_models rendered-object stand-ins on a W x H frame, the scene = the first one 3 mm further away and a pixel to the right, and a
    camera with its principal point in the middle of the frame."""
    models = [synth.synth_model_depth(seed + s, W, H) for s in range(n_models)]
    scene = np.roll(np.where(models[0] > 0, models[0] + 3, 0).astype(np.uint16), 1, axis=1)
    K = np.array([572.4114, 0, W / 2, 0, 573.57043, H / 2, 0, 0, 1], np.float32).reshape(3, 3)
    return models, scene, K


def icp_run(ctx, models, K, slots):
    """One hypothesis per entry of slots, each a pixel or two off its model's corner: R, t, iterations and stage of every hypothesis, and
    of the last one the source and target clouds, the state words that are no clocks and the cumulants of the normals."""
    n = len(slots)
    xy = []
    for h, s in enumerate(slots):
        ys, xs = np.nonzero(models[s])
        xy.append((int(xs.min()) + h % 3 - 1 + h // 6, int(ys.min()) + h % 2))
    Ks = np.tile(K.reshape(1, 9), (n, 1)); Rs = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    ts = np.array([[0.5 * h, -0.25 * h, 1000 + h] for h in range(n)], np.float32)
    res, _ = ctx.run(Ks, Rs, ts, xy, model_slots=slots)
    assert all(r["residual"] >= 0 and r["iterations"] > 0 and r["n_source"] > 1000 for r in res)   # every window inside the frame: registered (a residual of -1 says it was not)
    return ([(r["R"], r["t"], r["iterations"], r["stage"]) for r in res],
            [ctx.read_debug(n - 1, 0), ctx.read_debug(n - 1, 1), ctx.read_debug(n - 1, 3)[DBG3_NO_CLOCKS], ctx.read_debug(n - 1, 5)])


def icp_context(lm, models, scene, K):
    ctx = lm.IcpContext(device=0, scene_from_scene=True)
    ctx.set_scene(scene, K)
    ctx.set_models(models)
    return ctx


def test_icp_grows_and_reuses(lm):
    """160 x 120.  3 models in slots 0-2 and 3 hypotheses; then models up to slot 19, past the 16 slots the first upload made room for,
    and 18 hypotheses, past the 16 the arenas were sized for, on slots 0-2 and 17-19: the used context uploads only slots 3-19, so what it
    answers for 0-2 comes from the images and boxes that the growth of the slot arrays carried over.  Then both again."""
    W, H = 160, 120
    models, scene, K = icp_scene(300, 20, W, H)
    small, large = [0, 1, 2], [0, 1, 2, 17, 18, 19] * 3
    want_small = icp_run(icp_context(lm, models[:3], scene, K), models, K, small)
    want_large = icp_run(icp_context(lm, models, scene, K), models, K, large)
    used = icp_context(lm, models[:3], scene, K)
    assert same(icp_run(used, models, K, small), want_small), "first call"
    used.set_models(models[3:], first_slot=3)
    assert same(icp_run(used, models, K, large), want_large), "the call under which the slot arrays and every arena grow"
    assert same(icp_run(used, models, K, small), want_small), "the small call again, in the grown buffers"
    assert same(icp_run(used, models, K, large), want_large), "and the large one, now without growth"
    assert len(want_large[1][0]) > 100 and len(want_large[1][3]) > 100                    # the clouds compared are there


def test_icp_changes_geometry(lm):
    """One context at 160 x 120, at 320 x 240 with other models, and at 160 x 120 again: a new frame size drops the arenas, the slots
    and the scene, so a run before the models are uploaded again is refused — its slots are not resident —, and after the upload the
    context answers what a fresh one does."""
    used = lm.IcpContext(device=0, scene_from_scene=True)
    for W, H, seed in ((160, 120, 340), (320, 240, 350), (160, 120, 340)):
        models, scene, K = icp_scene(seed, 3, W, H)
        used.set_scene(scene, K)
        with pytest.raises(RuntimeError, match="model slot 0 of hypothesis 0 is not resident"):
            icp_run(used, models, K, [0])
        used.set_models(models)
        assert same(icp_run(used, models, K, [0, 1, 2]), icp_run(icp_context(lm, models, scene, K), models, K, [0, 1, 2])), (W, H)


# ---- lm_pipeline -------------------------------------------------------------------------------------------------------------
PIPE_W, PIPE_H, PIPE_T, PIPE_NF, PIPE_THR = 320, 240, [4, 8], (64, 32), 70.0
PIPE_CLASSES = ["n%d" % i for i in range(9)]
PIPE_K = np.array([286.2057, 0, 162.63055, 0, 286.785215, 121.024495, 0, 0, 1], np.float32).reshape(3, 3)


@pytest.fixture(scope="module")
def pipe_scene():
    """A 320 x 240 frame and nine classes of five templates planted in it, each at places of its own well inside the frame (the window of
    a detection there stays in it, so its pose is refined); the first two with few labels changed, so that their matches score highest
    and lead the NMS.  Per template a view: one of two rendered-object stand-ins, a pose near 1 m."""
    import linemod_oracle as lo
    rgb, dep = synth.make_frame(21, PIPE_W, PIPE_H, n_poly=16)
    pyr = lo.OracleDetector(PIPE_NF[0], PIPE_T).quantize_pyramid(rgb, dep)
    banks = {}
    for i, c in enumerate(PIPE_CLASSES):
        windows = [(40 + 36 * k + 4 * i, 36 + 22 * k + 2 * (i % 4), 56, 60) for k in range(5)]
        banks[c] = synth.make_planted_bank(100 + i, 5, [(p[0], p[1]) for p in pyr], PIPE_T, PIPE_NF, label_noise=0.02 if i < 2 else 0.12, windows=windows)
    shapes = [synth.synth_model_depth(200 + k, PIPE_W, PIPE_H) for k in range(2)]
    rng = np.random.default_rng(5)
    views = {c: [(shapes[(t + i) % 2], PIPE_K, np.eye(3, dtype=np.float32), np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), 1000 + rng.uniform(-20, 20)], np.float32))
                 for t in range(5)] for i, c in enumerate(PIPE_CLASSES)}
    return dict(frame=[rgb, dep], banks=banks, views=views)


def pipeline(lm, sc):
    det = lm.Detector(PIPE_NF[0], PIPE_T, device=0)
    for c in PIPE_CLASSES:
        det.addClassPacked(c, *sc["banks"][c])
    return det, lm.Pipeline(det, PIPE_W, PIPE_H, scene_from_scene=True)


def pipe_views(pipe, sc, c):
    v = sc["views"][c]
    pipe.set_views(c, [x[0] for x in v], [x[1] for x in v], [x[2] for x in v], [x[3] for x in v])


def pipe_run(det, pipe, sc, class_ids, top_k):
    det.setFrame(sc["frame"])
    return pipe.run(PIPE_THR, class_ids, PIPE_K, top_k=top_k, nms_iou=0.5)[0]


def test_pipeline_grows_and_reuses(lm, pipe_scene):
    """One pipeline: class n0 alone with top_k 2; top_k 8 (the selection and its pinned copy grow); the views of a second class (the view
    tables are replaced and uploaded again); nine class ids, past the eight the class table starts with, and top_k 18, past the 16
    hypotheses the ICP arenas were sized for; the first call again.  Each against a fresh pipeline on a fresh detector with the same
    bank and the views set so far."""
    sc = pipe_scene

    def fresh(classes_with_views, class_ids, top_k):
        det, pipe = pipeline(lm, sc)
        for c in classes_with_views:
            pipe_views(pipe, sc, c)
        got = pipe_run(det, pipe, sc, class_ids, top_k)
        pipe.close()
        return got
    det, used = pipeline(lm, sc)
    pipe_views(used, sc, "n0")
    first = fresh(["n0"], ["n0"], 2)
    assert len(first) == 2
    assert same(pipe_run(det, used, sc, ["n0"], 2), first), "first call"
    assert same(pipe_run(det, used, sc, ["n0"], 8), fresh(["n0"], ["n0"], 8)), "top_k 8"
    pipe_views(used, sc, "n1")
    assert same(pipe_run(det, used, sc, ["n0", "n1"], 8), fresh(["n0", "n1"], ["n0", "n1"], 8)), "a second class's views"
    large = fresh(["n0", "n1"], PIPE_CLASSES, 18)
    assert same(pipe_run(det, used, sc, PIPE_CLASSES, 18), large), "nine class ids, top_k 18"
    assert len(large) > 8 and any(r["status"] == 0 and r["iterations"] > 0 for r in large)    # the comparison is not one of empty lists
    assert len({r["class_index"] for r in large}) > 2
    assert same(pipe_run(det, used, sc, ["n0"], 2), first), "the first call again, in the grown buffers"
    assert same(pipe_run(det, used, sc, PIPE_CLASSES, 18), large), "and the large one, now without growth"
    used.close()


# ---- lm_detector: the staging buffer, the ingest ring and the result slots ---------------------------------------------------------
def test_detector_frames_grow_and_shrink(lm):
    """One detector matches a 320 x 240 frame, a 640 x 480 frame and the first again, each through matchArray (the staging buffer) and
    as two frames in flight through submitFrame / collect (the ingest ring's pinned entries, the result slots): the lists are those of a
    fresh detector with the same bank."""
    import linemod_oracle as lo
    T, nf = [4, 8], (64, 32)
    frames = [synth.make_frame(3, 320, 240, n_poly=16), synth.make_frame(4, 640, 480)]
    banks = {}
    for c, (rgb, dep) in zip(("small", "large"), frames):
        pyr = lo.OracleDetector(nf[0], T).quantize_pyramid(rgb, dep)
        banks[c] = synth.make_planted_bank(11, 24, [(p[0], p[1]) for p in pyr], T, nfeat=nf)

    def detector():
        det = lm.Detector(nf[0], T, device=0)
        for c in banks:
            det.addClassPacked(c, *banks[c])
        return det

    def lists(det, frame):
        got = [det.matchArray(list(frame), 70.0, ["small", "large"])]
        det.submitFrame(list(frame), 70.0, ["small", "large"]); det.submitFrame(list(frame), 70.0, ["small", "large"])
        return got + [det.collect(), det.collect()]
    used = detector()
    for name, frame in (("small", frames[0]), ("large", frames[1]), ("small again", frames[0]), ("large again", frames[1])):
        got, want = lists(used, frame), lists(detector(), frame)
        assert len(want[0]) > 0 and want[1].tobytes() == want[0].tobytes() == want[2].tobytes(), name
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)), name


# ---- lifecycles: every stream and event is created with its context and dies with it (DevStream / DevEvent) -----------------------------
LIFE_W, LIFE_H, LIFE_T, LIFE_NF, LIFE_THR = 64, 48, [2, 2], (32, 16), 70.0
LIFE_MODES = dict(min_pixels=200)                                                          # of the 3072 pixels of the frame


def close(ctx):
    """Destroys the context now: its close(), or for the detector, which has none, what dropping the last reference runs."""
    ctx.close() if hasattr(ctx, "close") else ctx.__del__()


@pytest.fixture(scope="module")
def life_scene(lm):
    """A 64 x 48 frame, four templates planted where the refinement reaches them (T = 2: a border of 16 pixels), and what a detector that
    has done nothing else answers: the records of the frame, and its depth-slab pass."""
    import linemod_oracle as lo
    rgb, dep = synth.make_frame(3, LIFE_W, LIFE_H, n_poly=6)
    pyr = lo.OracleDetector(LIFE_NF[0], LIFE_T).quantize_pyramid(rgb, dep)
    windows = [(18 + 2 * k, 16 + 2 * (k % 2), 24, 14) for k in range(4)]
    bank = synth.make_planted_bank(11, 4, [(p[0], p[1]) for p in pyr], LIFE_T, nfeat=LIFE_NF, label_noise=0.05, windows=windows)
    sc = dict(frame=[rgb, dep], bank=bank)
    det = life_detector(lm, sc)
    sc["records"] = det.matchArray(sc["frame"], LIFE_THR, ["obj"])
    sc["slabs"] = det.matchSlabs(sc["frame"], LIFE_THR, ["obj"], **LIFE_MODES)
    close(det)
    assert len(sc["records"]) > 0 and len(set(sc["records"]["template_id"])) == 4           # the comparisons are not ones of empty lists
    assert sc["slabs"][1][0]["depth_mm"] is not None and len(sc["slabs"][0]) > 0           # at least one mode, and records under its slab
    return sc


def life_detector(lm, sc):
    det = lm.Detector(LIFE_NF[0], LIFE_T, device=0)
    det.addClassPacked("obj", *sc["bank"])
    det.setClassDepthRange("obj", 300, 4000)
    return det


def life_case(lm, kind, life_scene, pipe_scene):
    """(open, call, close) of one kind of context: open() gives what close() takes, call() one small call on it."""
    if kind == "detector":
        return (lambda: life_detector(lm, life_scene)), (lambda d: d.matchArray(life_scene["frame"], LIFE_THR, ["obj"])), close
    if kind == "mesh":
        Rs, ts = poses(2, 11)
        return (lambda: full_mesh(lm)), (lambda m: m.render((32, 24), cam(32, 24), Rs, ts, clip_near=100.0, clip_far=2000.0, ssaa=1)), close
    if kind == "pso":
        mesh = lm.Mesh(*pc.mesh())

        def run(ctx):
            ctx.set_scene(pc.scene()[:60, :72], pc.K)
            return swarm(ctx, mesh, 1, (32, 32), particles=8, generations=2)
        return (lambda: lm.PsoContext(0)), run, close
    if kind == "icp":
        models, scene, K = icp_scene(300, 1, 160, 120)
        return (lambda: icp_context(lm, models, scene, K)), (lambda c: icp_run(c, models, K, [0])), close

    def open_pipeline():
        det, pipe = pipeline(lm, pipe_scene)
        pipe_views(pipe, pipe_scene, "n0")
        return det, pipe

    def close_pipeline(both):
        close(both[1])                                                                     # the pipeline, then the detector it was made on
        close(both[0])
    return open_pipeline, (lambda both: pipe_run(both[0], both[1], pipe_scene, ["n0"], 2)), close_pipeline


@pytest.mark.parametrize("kind", ["detector", "mesh", "pso", "icp", "pipeline"])
def test_context_opens_and_closes_three_times(lm, life_scene, pipe_scene, kind):
    """Created and closed three times in one process: once without having run anything, twice after one small call, whose answer is both
    times the same, bit for bit.  The pipeline is closed before its detector."""
    make, call, shut = life_case(lm, kind, life_scene, pipe_scene)
    shut(make())
    answers = []
    for _ in range(2):
        ctx = make()
        answers.append(call(ctx))
        shut(ctx)
    assert same(answers[1], answers[0])
    if kind == "detector":
        assert same(answers[0], life_scene["records"])
    if kind == "pipeline":
        assert len(answers[0]) == 2


def test_detector_closes_with_frames_in_flight(lm, life_scene):
    """Two streamed frames launched and never collected, a third still waiting for its batch: destroying the detector launches and flushes
    them.  The next detector in the process matches the frame to the same records."""
    sc = life_scene
    det = life_detector(lm, sc)
    det.setBatch(2); det.setBatchQueue(0)                                                  # a batch goes out when it is full, not before
    for _ in range(3):
        det.submitFrame(sc["frame"], LIFE_THR, ["obj"])
    assert (det.framesSubmitted(), det.framesLaunched(), det.framesCollected()) == (3, 2, 0)
    close(det)
    det = life_detector(lm, sc)
    assert same(det.matchArray(sc["frame"], LIFE_THR, ["obj"]), sc["records"])
    close(det)


def test_detector_closes_after_its_lazy_handles(lm, life_scene):
    """A detector that has been through every site that creates a handle on first use — a frame streamed through the ingest ring (its copy
    stream and timing events are made with the detector, or there), a depth-slab pass (modes_ready) and one exchange group of world 1,
    packed and merged in place (the exchange's done events) — answers what a fresh detector does, and so does the next one after it."""
    sc = life_scene
    det = life_detector(lm, sc)
    det.submitFrame(sc["frame"], LIFE_THR, ["obj"])
    assert same(det.collect(), sc["records"]), "ingest ring"
    assert same(det.matchSlabs(sc["frame"], LIFE_THR, ["obj"], **LIFE_MODES), sc["slabs"]), "depth slabs"
    lib = lm.load_library()                                                                # (its handle also resolves the HIP runtime it is bound to)
    block, nbytes = ctypes.c_void_p(), ctypes.c_size_t(lib.lm_exchange_block_bytes(256))
    assert lib.hipMalloc(ctypes.byref(block), nbytes) == 0 and lib.hipMemset(block, 0, nbytes) == 0 and lib.hipDeviceSynchronize() == 0
    try:
        first = det.framesSubmitted()
        det.submit(LIFE_THR, ["obj"]); det.flush()
        det.exchangePackGroup(first, 1, block.value, 256)
        det.exchangeMergeGroup(first, 1, block.value, 1, 256)
        got, failed = det.exchangeCollect()
        assert failed == 0 and same(got, sc["records"]), "exchange of world 1"
        close(det)
    finally:
        lib.hipFree(block)
    det = life_detector(lm, sc)
    assert same(det.matchArray(sc["frame"], LIFE_THR, ["obj"]), sc["records"])
    close(det)
