"""GPU tests (`-m gpu`) of grey colour frames: Detector(..., colour_channels=1) takes a uint8 HxW image in the colour slot.

The definition is exact and needs no oracle of its own: quantizedOrientations (LL.cpp:350-425) on a frame whose three channels are equal
takes channel 0 at every pixel, and cv::pyrDown keeps equal channels equal, so a grey frame g must give, byte for byte and at every
level, what the RGB path and the existing oracle give on rep = g replicated to three channels.  Throughout: g = one channel of
synth.make_frame(...), rep = np.repeat(g[..., None], 3, 2), od = lo.OracleDetector; every case checks that the level-0 orientation
map has set pixels, so no equality is one of empty maps."""
import os

import numpy as np
import pytest

import linemod_oracle as lo
import modality_ref as mr
import synth
from helpers import K_CAM, oracle_matches

pytestmark = pytest.mark.gpu

EMPTY = (np.zeros((0, 3), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
# (W, H, T, polygons): the smallest frames at which the grey chain can go wrong
GEOMS = {
    "16x16": (16, 16, [2], 6),              # smaller than one 32 x 16 tile: clamping on all four sides at once
    "50x48": (50, 48, [2], 6),              # a tile hangs over the right edge, rows are not dword-aligned: the vote's four-pixel store falls back to bytes
    "100x96": (100, 96, [2, 2], 10),        # the same at level 1, after one grey pyrDown (REFLECT_101)
    "24x32": (24, 32, [2, 2, 2], 6),        # two pyrDowns: the smallest three-level frame of test_gpu_parity
    "320x240": (320, 240, [4, 8], 12),      # several tiles each way (synth_small_T48)
}


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def grey_frame(seed, W, H, n_poly):
    rgb, dep = synth.make_frame(seed, W, H, n_poly)
    g = np.ascontiguousarray(rgb[..., 1])
    return g, np.repeat(g[..., None], 3, 2), dep


_frames = {}


def frame_of(geom):
    """g, rep, depth and the oracle's pyramid on rep for a geometry: computed once, never modified"""
    if geom not in _frames:
        W, H, T, n_poly = GEOMS[geom]
        g, rep, dep = grey_frame(4, W, H, n_poly)
        pyr = lo.OracleDetector(64, T).quantize_pyramid(rep, dep)
        assert (pyr[0][0] > 0).any(), "the level-0 orientation map must have set pixels"
        _frames[geom] = {"g": g, "rep": rep, "dep": dep, "pyr": pyr, "T": T, "W": W, "H": H}
    return _frames[geom]


_scene = {}


def scene():
    """320 x 240, T = (4, 8): nine frames, a bank of eight templates planted in frame 0, the oracle's answer on rep of frame 0"""
    if not _scene:
        W, H, T, nfeat, thr = 320, 240, [4, 8], (64, 32), 70.0
        frames = [grey_frame(30 + i, W, H, 12) for i in range(9)]
        g, rep, dep = frames[0]
        od = lo.OracleDetector(nfeat[0], T)
        pyr = od.quantize_pyramid(rep, dep)
        assert (pyr[0][0] > 0).any()
        bank = synth.make_planted_bank(11, 8, [(p[0], p[1]) for p in pyr], T, nfeat=nfeat)
        raw, st = oracle_matches(od, rep, dep, bank, T, thr)
        canon = lo.canonical_sort_unique(raw)
        assert len(canon) > 0 and len(set(canon["sim"].tolist())) > 1
        _scene.update(W=W, H=H, T=T, nf=nfeat[0], thr=thr, frames=frames, bank=bank, raw=raw, st=st, canon=canon, od=od)
    return _scene


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for a, b in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("template_id", "tid")):
        assert np.array_equal(got[a], want[b]), a


def same_templates(a, b):
    assert len(a) == len(b) and len(a) > 0
    for s, t in zip(a, b):
        assert (s.width, s.height, s.pyramid_level) == (t.width, t.height, t.pyramid_level)
        assert len(s.features) > 0 and np.array_equal(s.features, t.features)


# ---- 1. stages ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_stages_equal_the_oracle_on_the_replicated_frame(lm, geom):
    f = frame_of(geom)
    T = f["T"]
    det = lm.Detector(64, T, device=0, colour_channels=1)
    assert det.getColourChannels() == 1
    det.addClassPacked("e", *EMPTY)
    det.setFrame([f["g"], f["dep"]])
    det.matchResident(75.0, ["e"])
    for l, (qc, qn, *_r) in enumerate(f["pyr"]):
        n = 8 * qc.size
        assert np.array_equal(det.readStage(l, 0).reshape(qc.shape), qc), "orientations level %d" % l
        assert np.array_equal(det.readStage(l, 2), lo.build_linear_memories(qc, T[l])[:n]), "LM colour level %d" % l
        # the depth image lands behind a W * H byte colour image
        assert np.array_equal(det.readStage(l, 1).reshape(qn.shape), qn), "normals level %d" % l
        assert np.array_equal(det.readStage(l, 3), lo.build_linear_memories(qn, T[l])[:n]), "LM normal level %d" % l
    assert (f["pyr"][0][1] > 0).any()


# ---- 2. colour-only ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["50x48", "320x240"])
def test_colour_only_detector(lm, geom):
    f = frame_of(geom)
    T = f["T"]
    det = lm.Detector(64, T, device=0, modalities=("ColorGradient",), colour_channels=1)
    det.addClassPacked("e", *EMPTY)
    det.setFrame([f["g"]])
    det.matchResident(75.0, ["e"])
    for l, (qc, *_r) in enumerate(f["pyr"]):
        assert np.array_equal(det.readStage(l, 0).reshape(qc.shape), qc), "orientations level %d" % l
        assert np.array_equal(det.readStage(l, 2), lo.build_linear_memories(qc, T[l])[:8 * qc.size]), "LM colour level %d" % l


# ---- 3. training -------------------------------------------------------------------------------------------------------------------------------
def test_add_template_equals_the_rgb_detector_on_the_replicated_view(lm):
    """one synthetic object (tests/modality_ref.view), and a crop of another whose mask touches the image border"""
    T = [4, 8]
    grey, col = lm.Detector(32, T, device=0, colour_channels=1), lm.Detector(32, T, device=0)
    crops = [(slice(None), slice(None)), (slice(48, 176), slice(64, 208))]
    for i, (seed, sl) in enumerate(zip((1, 2), crops)):
        rgb, dep, mask = mr.view(seed)
        g, dep, mask = np.ascontiguousarray(rgb[sl][..., 1]), np.ascontiguousarray(dep[sl]), np.ascontiguousarray(mask[sl])
        rep = np.repeat(g[..., None], 3, 2)
        assert (mask[0].any() or mask[:, 0].any()) == (i == 1)
        assert (lo.OracleDetector(32, T).quantize_pyramid(rep, dep)[0][0] > 0).any()
        assert grey.addTemplate([g, dep], "o", mask) == col.addTemplate([rep, dep], "o", mask) == i
        same_templates(grey.getTemplates("o", i), col.getTemplates("o", i))
        assert len(grey.getTemplates("o", i)) == 2 * len(T)


# ---- 4. match ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [None, ("tiles", "bytes")], ids=["default", "bytes"])
def test_match_equals_the_rgb_detector_and_the_oracle(lm, paths):
    s = scene()
    g, rep, dep = s["frames"][0]
    grey, col = lm.Detector(s["nf"], s["T"], device=0, colour_channels=1), lm.Detector(s["nf"], s["T"], device=0)
    got = []
    for det, src in ((grey, g), (col, rep)):
        if paths:
            det.setPaths(*paths)
        det.addClassPacked("obj", *s["bank"])
        got.append(det.matchArray([src, dep], s["thr"], ["obj"]))
        want = paths or ("bits", "bits")
        assert det.getPaths() == want and det.refinesOnBitPlanes() == (want[0] == "bits")
        tm = det.lastTimings()
        assert tm["coarse_candidates"] == s["st"]["coarse_candidates"] and tm["matches_pre_unique"] == len(s["raw"])
    assert got[0].tobytes() == got[1].tobytes()
    same_records(got[0], s["canon"])


# ---- 5. stream ---------------------------------------------------------------------------------------------------------------------------------
def test_stream_of_nine_frames_three_of_them_filled_in_place(lm):
    s = scene()
    W, H, thr = s["W"], s["H"], 45.0
    det = lm.Detector(s["nf"], s["T"], device=0, colour_channels=1)
    det.addClassPacked("obj", *s["bank"])
    det.setBatch(8)
    det.setBatchQueue(0)                                       # one full batch and a remainder
    for i, (g, _rep, dep) in enumerate(s["frames"]):
        if i in (1, 4, 8):
            bufs = det.ingestBuffers(W, H)
            assert len(bufs) == 2 and bufs[0].shape == (H, W) and bufs[0].dtype == np.uint8 and bufs[1].shape == (H, W)
            bufs[0][:] = g
            bufs[1][:] = dep
            det.submitFrame([bufs[0], bufs[1]], thr, ["obj"])
        else:
            det.submitFrame([g, dep], thr, ["obj"])
    assert det.framesLaunched() == 8
    streamed = [det.collect() for _ in range(9)]
    sync = [det.matchArray([g, dep], thr, ["obj"]) for g, _rep, dep in s["frames"]]
    for a, b in zip(streamed, sync):
        assert a.tobytes() == b.tobytes()
    assert len(sync[0]) > 0 and len(set(x.tobytes() for x in sync)) > 1


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_detector_usable(lm):
    s = scene()
    g, rep, dep = s["frames"][0]
    grey, col = lm.Detector(s["nf"], s["T"], device=0, colour_channels=1), lm.Detector(s["nf"], s["T"], device=0)
    for det in (grey, col):
        det.addClassPacked("obj", *s["bank"])
    with pytest.raises(RuntimeError, match="colour_channels"):
        grey.matchArray([rep, dep], s["thr"], ["obj"])
    with pytest.raises(RuntimeError, match="colour_channels"):
        col.matchArray([g, dep], s["thr"], ["obj"])
    with pytest.raises(RuntimeError, match="colour_channels"):
        lm.Detector(s["nf"], s["T"], device=0, colour_channels=2)
    with pytest.raises(RuntimeError, match="colour_channels"):
        lm.Detector(s["nf"], s["T"], device=0, modalities=("DepthNormal",), colour_channels=1)
    with pytest.raises(RuntimeError, match="colour_channels"):
        col.setColourChannels(2)
    assert col.getColourChannels() == 3
    grey.setFrame([g, dep])
    grey.submit(s["thr"], ["obj"])
    with pytest.raises(RuntimeError, match="in flight"):
        grey.setColourChannels(3)
    assert grey.getColourChannels() == 1
    same_records(grey.collect(), s["canon"])
    same_records(grey.matchArray([g[:, :, None], dep], s["thr"], ["obj"]), s["canon"])     # (HxWx1 is a grey image too)
    same_records(col.matchArray([rep, dep], s["thr"], ["obj"]), s["canon"])


# ---- 7. renders --------------------------------------------------------------------------------------------------------------------------------
def test_rgb_to_grey_is_the_integer_formula(lm):
    rgb = np.random.default_rng(7).integers(0, 256, (37, 5, 3), dtype=np.uint8)
    rgb[0, 0], rgb[36, 4], rgb[5, 2] = 0, 255, (255, 0, 255)
    v = rgb.astype(np.int64)
    want = ((4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14).astype(np.uint8)
    got = lm.rgb_to_grey(rgb)
    assert got.shape == (37, 5) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert got[0, 0] == 0 and got[36, 4] == 255 and np.array_equal(lm.rgb_to_grey_ref(rgb), want)


def test_rendered_views_equal_add_template_on_the_converted_renders(lm):
    W, H, T = 128, 96, [4, 8]
    K = (K_CAM * np.array([[.2], [.2], [1]], np.float32)).astype(np.float32)
    V, F, N, C = synth.icosphere(2, radius=70.0, seed=11)
    C[:] = (C // 64) * 64 + 30
    mesh = lm.Mesh(V, F, normals=N, colors=C)
    Rs = np.stack([np.eye(3, dtype=np.float32), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)])
    ts = np.tile(np.array([0, 0, 300], np.float32), (2, 1))
    a, b = lm.Detector(32, T, device=0, colour_channels=1), lm.Detector(32, T, device=0, colour_channels=1)
    ids, _wh = lm.add_templates_rendered(a, mesh, "obj", (W, H), K, Rs, ts)
    rgb, depth = mesh.render((W, H), K, Rs, ts)
    grey = [lm.rgb_to_grey(rgb[i]) for i in range(2)]
    assert not np.array_equal(rgb[0][..., 0], rgb[0][..., 1]) and not np.array_equal(grey[0], rgb[0][..., 1]), "a colour render: the conversion matters"
    want = [b.addTemplate([grey[i], depth[i]], "obj", (depth[i] > 0).astype(np.uint8) * 255) for i in range(2)]
    assert ids.tolist() == want == [0, 1]
    for t in want:
        same_templates(a.getTemplates("obj", t), b.getTemplates("obj", t))


# ---- 8. pipeline -------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_on_a_grey_and_depth_detector(lm):
    """Only the front end differs between the two detectors, so nothing downstream may: same detections, R and t bit for bit."""
    s = scene()
    W, H, T = s["W"], s["H"], s["T"]
    g, rep, dep = s["frames"][0]
    n = (len(s["bank"][1]) - 1) // (2 * len(T))
    rng = np.random.default_rng(5)
    shapes = [synth.synth_model_depth(200 + k, W, H) for k in range(2)]
    Kv = (K_CAM * np.array([[.5], [.5], [1]], np.float32)).astype(np.float32)
    views = [(shapes[t % 2], Kv, np.eye(3, dtype=np.float32), np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), 1000 + rng.uniform(-20, 20)], np.float32))
             for t in range(n)]
    out = []
    for cch, src in ((1, g), (3, rep)):
        det = lm.Detector(s["nf"], T, device=0, colour_channels=cch)
        det.addClassPacked("obj", *s["bank"])
        pipe = lm.Pipeline(det, W, H, scene_from_scene=True)
        pipe.set_views("obj", [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views])
        det.setFrame([src, dep])
        got, tm = pipe.run(s["thr"], ["obj"], Kv, top_k=8, nms_iou=0.5)
        assert tm["coarse_candidates"] == s["st"]["coarse_candidates"]
        out.append(got)
        pipe.close()
    a, b = out
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k
