"""GPU tests of the device feature selection (csrc/train.hip) at its edges: the frames of tests/train_cases.py (whose edges
tests/test_train_cases.py asserts on the CPU) through Detector.addTemplate on the device, through the host selection
(LM_TRAIN_HOST=1) and through the oracle — integer equality — with Detector.trainStats() saying which selection served;
batches of rendered views that mix ok, too-few, empty and host-path views; the refusal of num_features >> (levels - 1) == 0."""
import os
import re

import numpy as np
import pytest

import linemod_oracle as lo
import train_cases as tc
from synth import icosphere

pytestmark = pytest.mark.gpu

K_CAM = np.array([572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1], np.float32).reshape(3, 3)


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def make_detector(lm, p, tmp_path):
    """The product's way to non-default modality parameters: write(), edit the YAML, read()."""
    det = lm.Detector(p["num_features"], p["T"], device=0)
    path = str(tmp_path / "params.yaml")
    det.write(path)
    text = open(path).read()
    for key, val in (("strong_threshold", "%r" % float(p["strong_threshold"])), ("weak_threshold", "%r" % float(p["weak_threshold"])),
                     ("extract_threshold", "%d" % p["extract_threshold"]), ("distance_threshold", "%d" % p["distance_threshold"]),
                     ("difference_threshold", "%d" % p["difference_threshold"]), ("num_features", "%d" % p["num_features"])):
        text, n = re.subn(r"(\b%s:) *\S+" % key, r"\1 " + val, text)
        assert n == (2 if key == "num_features" else 1), key
    open(path, "w").write(text)
    det.read(path)
    assert det.trainStats() == (0, 0, 0, 0)
    return det


def train(lm, p, tmp_path, frame, host):
    rgb, depth, mask = frame
    if host:
        os.environ["LM_TRAIN_HOST"] = "1"
    try:
        det = make_detector(lm, p, tmp_path)
        rc = det.addTemplate([rgb, depth], "obj", mask)
    finally:
        if host:
            del os.environ["LM_TRAIN_HOST"]
    return det, rc


def assert_same_templates(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert (a.width, a.height, a.pyramid_level) == (b.width, b.height, b.pyramid_level), what
        assert np.array_equal(a.features, np.asarray(b.features, np.int32).reshape(-1, 3)), what


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_case_device_host_and_oracle_agree(lm, tmp_path, name):
    (rgb, depth, mask, p), _, oid, want = tc.analysed(name)
    _, path, trains = tc.CASES[name]
    det_d, rc_d = train(lm, p, tmp_path, (rgb, depth, mask), host=False)
    det_h, rc_h = train(lm, p, tmp_path, (rgb, depth, mask), host=True)
    print(name, "device", rc_d, det_d.trainStats(), "host", rc_h, det_h.trainStats(), "oracle", oid)
    assert rc_d == rc_h == oid and (oid == 0) == trains
    if trains:
        assert_same_templates(det_d.getTemplates("obj", 0), want, "device")
        assert_same_templates(det_h.getTemplates("obj", 0), want, "host")
    assert det_d.numTemplates("obj") == det_h.numTemplates("obj") == (1 if trains else 0)
    failed = 0 if trains else 1
    assert det_d.trainStats() == ((1, 0, failed, 0) if path == "device" else (0, 1, failed, 0))
    assert det_h.trainStats() == (0, 1, failed, 0)


@pytest.mark.parametrize("name", ["9a_at_cap", "4_ties"])
def test_selection_is_repeatable(lm, tmp_path, name):
    """k_train_prep and k_train_dt append candidates in atomic order; only the sort's key (score, then raster position) orders them."""
    (rgb, depth, mask, p), _, _, _ = tc.analysed(name)
    runs = []
    for _ in range(2):
        det, rc = train(lm, p, tmp_path, (rgb, depth, mask), host=False)
        assert rc == 0 and det.trainStats() == (1, 0, 0, 0)
        runs.append(b"".join(t.features.tobytes() for t in det.getTemplates("obj", 0)))
    assert runs[0] == runs[1] and len(runs[0]) > 0


def test_too_few_features_for_the_levels_are_refused(lm, tmp_path):
    """num_features >> (levels - 1) == 0 made LL.cpp:632 divide by zero (SIGFPE): refused where the state is set.  The smallest
    detectors that are allowed still train like the oracle."""
    with pytest.raises(RuntimeError, match="num_features 1 .* 2 pyramid levels"):
        lm.Detector(1, [4, 8])
    with pytest.raises(RuntimeError, match="num_features 3 .* 3 pyramid levels"):
        lm.Detector(3, [4, 4, 8])
    det = lm.Detector(8, [4, 8], device=0)
    path = str(tmp_path / "p.yaml")
    det.write(path)
    text, n = re.subn(r"num_features: 8", "num_features: 1", open(path).read())
    assert n == 2
    open(path, "w").write(text)
    with pytest.raises(RuntimeError, match="LL.cpp:560"):
        det.read(path)
    (rgb, depth, mask, _), _, _, _ = tc.analysed("4_ties")
    for nf, T in ((2, [4, 8]), (1, [4])):
        od = lo.OracleDetector(nf, T)
        assert od.addTemplate([rgb, depth], "obj", mask) == 0
        d = lm.Detector(nf, T, device=0)
        assert d.addTemplate([rgb, depth], "obj", mask) == 0 and d.trainStats() == (1, 0, 0, 0)
        assert_same_templates(d.getTemplates("obj", 0), od.class_templates["obj"][0], (nf, T))


def _views(n, seed):
    rng = np.random.default_rng(seed)
    Rs = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        Rs.append(q)
    return np.stack(Rs).astype(np.float32)


def _mesh(lm, level):
    V, F, N, C = icosphere(level, radius=70.0, seed=11)
    C[:] = (C // 64) * 64 + 30
    return lm.Mesh(V, F, normals=N, colors=C)


def _host_round_trip(lm, det, rgb, depth):
    ids = []
    for i in range(len(depth)):
        ids.append(det.addTemplate([rgb[i], depth[i]], "obj", (depth[i] > 0).astype(np.uint8) * 255))
    return ids


def test_batch_of_70_views_mixes_ok_few_and_empty(lm):
    """Two chunks (64 + 6) on a 128x96 frame: per-view scratch offsets, the second launch, and every outcome inside one chunk."""
    W, H, n, nf, T = 128, 96, 70, 16, [4, 8]
    K = (K_CAM * np.array([[.2], [.2], [1]], np.float32)).astype(np.float32)
    Rs = _views(n, 5)
    ts = np.tile(np.array([0, 0, 420], np.float32), (n, 1))
    ts[:, 0] += np.linspace(-25, 25, n); ts[:, 1] += np.linspace(15, -15, n)
    kind = np.arange(n) % 7
    ts[kind == 5, 2] = 4000.0                      # a few pixels: too few candidates
    ts[kind == 6, 0] = 2000.0                      # outside the frame: empty
    mesh = _mesh(lm, 2)
    det_a, det_b = lm.Detector(nf, T, device=0), lm.Detector(nf, T, device=0)
    ids, wh = lm.add_templates_rendered(det_a, mesh, "obj", (W, H), K, Rs, ts)
    rgb, depth = mesh.render((W, H), K, Rs, ts)
    px = (depth > 0).reshape(n, -1).sum(1)
    want = _host_round_trip(lm, det_b, rgb, depth)
    empty, few, ok = px == 0, (px > 0) & (np.asarray(want) < 0), np.asarray(want) >= 0
    assert empty[:64].any() and few[:64].any() and ok[:64].any() and ok[64:].any()
    assert np.array_equal(empty, kind == 6) and np.array_equal(few, kind == 5) and px[few].max() < 100
    assert ids.tolist() == want
    for i in range(n):
        ys, xs = np.nonzero(depth[i])
        assert tuple(wh[i]) == ((xs.max() - xs.min(), ys.max() - ys.min()) if len(xs) else (0, 0)), i
    for t in [t for t in want if t >= 0]:
        for a, b in zip(det_a.getTemplates("obj", t), det_b.getTemplates("obj", t)):
            assert (a.width, a.height, a.pyramid_level) == (b.width, b.height, b.pyramid_level) and np.array_equal(a.features, b.features), t
    od = lo.OracleDetector(nf, T)
    for i in np.nonzero(ok)[0][:4]:
        oid = od.addTemplate([rgb[i], depth[i]], "obj", (depth[i] > 0).astype(np.uint8) * 255)
        assert oid >= 0
        for a, b in zip(det_a.getTemplates("obj", want[i]), od.class_templates["obj"][oid]):
            assert (a.width, a.height, a.pyramid_level) == (b.width, b.height, b.pyramid_level), i
            assert np.array_equal(a.features, np.asarray(b.features, np.int32).reshape(-1, 3)), i
    stats = det_a.trainStats()
    print("batch of 70:", stats, "ok", int(ok.sum()), "few", int(few.sum()), "empty", int(empty.sum()))
    assert stats == (int(ok.sum() + few.sum()), 0, int(few.sum()), int(empty.sum()))
    assert stats[0] + stats[1] + stats[3] == n
    assert det_b.trainStats() == (n, 0, int(few.sum() + empty.sum()), 0)       # per view with a mask: the device decides, an all-zero mask is a too-few view


def test_host_path_view_between_device_views_keeps_view_order(lm):
    """640x480, one chunk of three views: the near one (radius ~190 px) has more candidates than the kernel sorts and goes through the
    host selection between its neighbours; the template ids keep view order."""
    Rs = _views(3, 9)
    ts = np.array([[-30, 20, 520], [0, 0, 210], [30, -20, 520]], np.float32)
    mesh = _mesh(lm, 3)
    det_a, det_b = lm.Detector(63, [4, 8], device=0), lm.Detector(63, [4, 8], device=0)
    ids, _ = lm.add_templates_rendered(det_a, mesh, "obj", (640, 480), K_CAM, Rs, ts)
    rgb, depth = mesh.render((640, 480), K_CAM, Rs, ts)
    assert ids.tolist() == [0, 1, 2] == _host_round_trip(lm, det_b, rgb, depth)
    assert det_a.trainStats() == (2, 1, 0, 0) and det_b.trainStats() == (2, 1, 0, 0)
    for t in range(3):
        for a, b in zip(det_a.getTemplates("obj", t), det_b.getTemplates("obj", t)):
            assert (a.width, a.height, a.pyramid_level) == (b.width, b.height, b.pyramid_level) and np.array_equal(a.features, b.features), t
    px = (depth > 0).reshape(3, -1).sum(1)
    assert px[1] > 4 * px[0] and px[1] > 4 * px[2]
