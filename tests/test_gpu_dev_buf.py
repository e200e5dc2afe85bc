"""Who owns device memory (csrc/dev_buf.h) in the mesh family: lm_mesh, its pose-error scratch and lm_pso (`-m gpu`).

DevBuf<T> alone is checked by the stand-alone program tests/cpp/dev_buf_cases.cpp, built here next to the header it tests.

The grow-and-reuse tests make ONE context serve a small call, then a larger call under which every scratch buffer of that path has to be
replaced by a larger one, then the small call again, and compare each answer with the same call on a context that has served nothing else.
A buffer that kept its old capacity, its old pointer in a kernel argument, or a stale capacity after it was replaced shows as a difference
(or as a fault).  The comparisons are exact: these paths use integer atomics and sums in a fixed order, and two fresh contexts agree bit for
bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pso_cases as pc
import pso_edge_cases as ec
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


def test_dev_buf_alone(lm, tmp_path):
    """ensure(0) allocates nothing; ensure(m <= n) keeps pointer and cap; growth gives cap == n; release() twice; both moves leave the
    source {nullptr, 0}; a std::vector<DevBuf> that reallocates keeps every pointer and what was written through it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "dev_buf_cases")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "6dpose_amd", "csrc"), "-x", "hip", os.path.join(ROOT, "tests", "cpp", "dev_buf_cases.cpp"), "-o", exe],
                          timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"ok:" in r.stdout, r.stdout.decode()[-2000:]


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
