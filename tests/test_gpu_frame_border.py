"""GPU tests (`-m gpu`) of the border policies (Detector.setBorder): frames whose size is not aligned to the T grid.

The definition is exact: under "pad" every entry point returns bit for bit what "strict" returns for the frame padded on the host (colour by
edge replication, depth and masks with 0, at the right and bottom), under "crop" what it returns for frame[:Ha, :Wa].  So every case holds
the detector against (a) the CPU oracle on the host-padded / host-cropped frame (tests/frame_border_ref.py, itself checked by hand in
test_frame_border_host.py) and (b) a strict detector fed that frame.  Frames come from synth.make_frame, banks are planted in the oracle's
quantisation of the PADDED frame; every matching case asserts a list that is not empty.

lm_timings counts no launches, so "the same launches as strict" is held through what it does count: candidates, evaluations, bytes read,
records and batch_frames are equal to the strict detector's on the aligned frame (INT_TIMINGS), and getPaths() is the same.
Under "strict", 313 x 229 is refused by the FIRST of the reference's asserts, (rows * cols) % 16 (LL.cpp:1136), as before this policy existed;
the T-grid assert (LL.cpp:1217-1218) is what 312 x 232 meets.  test_policy_surface asserts both."""
import os

import numpy as np
import pytest

import frame_border_ref as fb
import linemod_oracle as lo
import modality_ref as mr
import synth
from helpers import K_CAM, class_raw, det_fields, oracle_matches

pytestmark = pytest.mark.gpu

THR = 70.0
# name: (T, source W, H, features per level, aligned size under "pad")
CASES = {
    "313x229": ([4, 8], 313, 229, (64, 32), (320, 240)),
    "305x225": ([4, 8], 305, 225, (64, 32), (320, 240)),           # pad 15 each way: the most
    "319x239": ([4, 8], 319, 239, (64, 32), (320, 240)),           # pad 1, odd rows
    "320x240": ([4, 8], 320, 240, (64, 32), (320, 240)),           # aligned: the strict path
    "300x200_T58": ([5, 8], 300, 200, (64, 32), (320, 240)),
    "310x230_T448": ([4, 4, 8], 310, 230, (64, 32, 16), (320, 256)),
    "720x540": ([4, 8], 720, 540, (64, 32), (720, 544)),           # the T-LESS frame
}
# 313 x 229: two templates cut so that their boxes end within T = 4 pixels of the source's right / bottom edge (x0, y0, w, h)
EDGE_WINDOWS = [(250, 60, 60, 90), (80, 150, 80, 76)]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def aligned(frame, T, border, masks=()):
    """(colour, depth, masks) as the policy defines them, on the host"""
    colour, dep = frame
    H, W = (colour if colour is not None else dep).shape[:2]
    Wa, Ha = lo_aligned(T, W, H, border)
    return (fb.pad_frame if border == "pad" else fb.crop_frame)(colour, dep, Wa, Ha, masks)


def lo_aligned(T, W, H, border):
    from lm_abi import aligned_size
    return aligned_size(T, W, H, border)


_scenes = {}


def scene(name):
    """frame, bank (planted in the oracle's quantisation of the padded frame) and the oracle's answers of a case: computed once, never modified"""
    if name not in _scenes:
        T, W, H, nfeat, want_pad = CASES[name]
        assert lo_aligned(T, W, H, "pad") == want_pad
        n = 60 if name == "720x540" else 40
        rgb, dep = synth.make_frame(21, W, H, 30 if name == "720x540" else 12)
        od = lo.OracleDetector(nfeat[0], T)
        rgbp, depp, _ = aligned((rgb, dep), T, "pad")
        pyr = od.quantize_pyramid(rgbp, depp)
        windows = None
        if name == "313x229":
            rng = np.random.default_rng(5)
            windows = [(int(rng.integers(34, 200)), int(rng.integers(34, 120)), int(rng.integers(30, 66)), int(rng.integers(30, 70))) for _ in range(n - 2)]
            windows += EDGE_WINDOWS
        bank = synth.make_planted_bank(11, n, [(p[0], p[1]) for p in pyr], T, nfeat=nfeat, windows=windows)
        _scenes[name] = {"T": T, "W": W, "H": H, "nf": nfeat[0], "frame": (rgb, dep), "od": od, "bank": bank, "n": n, "expect": {}}
    return _scenes[name]


def expect(s, border, frame=None, key=0, thr=THR):
    """the oracle on the host-padded / host-cropped frame: (canonical list, statistics, the aligned frame)"""
    k = (border, key, thr)
    if k not in s["expect"]:
        colour, dep, _ = aligned(frame or s["frame"], s["T"], border)
        raw, st = oracle_matches(s["od"], colour, dep, s["bank"], s["T"], thr)
        s["expect"][k] = (lo.canonical_sort_unique(raw), st, (colour, dep), len(raw))
    return s["expect"][k]


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for a, b in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("template_id", "tid")):
        assert np.array_equal(got[a], want[b]), a


def detector(lm, s, border, **kw):
    det = lm.Detector(s["nf"], s["T"], device=0, **kw)
    det.addClassPacked("obj", *s["bank"])
    if border != "strict":
        det.setBorder(border)
        assert det.getBorder() == border
    return det


def masked_memories(od, colour, dep, masks):
    """(linear memories, sizes) of a frame with one mask per modality (None: unmasked): quantize() copies through the mask, LL.cpp:583-587"""
    pc, pn = od.quantize_pyramid(colour, dep, masks[0]), od.quantize_pyramid(colour, dep, masks[1])
    lms = [[lo.build_linear_memories(c[0], T), lo.build_linear_memories(n[1], T)] for c, n, T in zip(pc, pn, od.T_at_level)]
    return lms, [(c[0].shape[1], c[0].shape[0]) for c in pc]


INT_TIMINGS = ("coarse_candidates", "local_evals", "matches_pre_unique", "templates", "coarse_bytes", "local_bytes", "batch_frames")


# ---- 1. source sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ["pad", "crop"])
@pytest.mark.parametrize("name", [c for c in CASES if c != "720x540"])
def test_match_equals_strict_and_the_oracle_on_the_aligned_frame(lm, name, border):
    s = scene(name)
    canon, st, host, nraw = expect(s, border)
    assert len(canon) > 0, "a case with an empty list proves nothing"
    det, strict = detector(lm, s, border), detector(lm, s, "strict")
    got = det.matchArray(list(s["frame"]), THR, ["obj"])
    tm = det.lastTimings()
    ref = strict.matchArray(list(host), THR, ["obj"])
    tm_ref = strict.lastTimings()
    same_records(got, canon)
    assert got.tobytes() == ref.tobytes()
    assert tm["coarse_candidates"] == st["coarse_candidates"] and tm["matches_pre_unique"] == nraw
    assert det.getPaths() == strict.getPaths() == ("bits", "bits")
    assert [tm[k] for k in INT_TIMINGS] == [tm_ref[k] for k in INT_TIMINGS]       # the same work on the aligned geometry
    assert det.alignedSize(s["W"], s["H"]) == host[1].shape[::-1]
    if name == "320x240":                                    # aligned already: both policies are the strict path on the frame itself
        assert np.array_equal(host[0], s["frame"][0]) and np.array_equal(host[1], s["frame"][1])
        assert strict.matchArray(list(s["frame"]), THR, ["obj"]).tobytes() == got.tobytes()


# ---- 2. what is in the margins -----------------------------------------------------------------------------------------------------------------
def test_margins_are_replicated_colour_and_zero_depth_with_nothing_stale(lm):
    s = scene("313x229")
    T, W, H, E = s["T"], s["W"], s["H"], 2 * len(s["T"])
    canon, st, host, nraw = expect(s, "pad")
    wh, n = s["bank"][2], s["n"]
    for tid, (axis, size) in ((n - 2, ("x", W)), (n - 1, ("y", H))):        # the planted edge templates are found where their boxes end in the last T pixels
        hit = canon[canon["tid"] == tid]
        assert len(hit) and (hit[axis] + int(wh[tid * E][0 if axis == "x" else 1]) >= size - T[0]).any(), (tid, axis)
    # a wrong margin changes the records: the oracle on the frame padded with zeros in the colour image answers differently
    rgb0 = np.ascontiguousarray(np.pad(s["frame"][0], ((0, 240 - H), (0, 320 - W), (0, 0))))
    raw0, _st = oracle_matches(s["od"], rgb0, host[1], s["bank"], T, THR)
    canon0 = lo.canonical_sort_unique(raw0)
    assert len(canon0) != len(canon) or canon0.tobytes() != canon.tobytes()
    # the same detector first on a larger aligned frame of noise (everything this frame does not overwrite would be stale), then the odd frame
    det = detector(lm, s, "pad")
    rng = np.random.default_rng(3)
    noise = [rng.integers(0, 256, (288, 384, 3), dtype=np.uint8), rng.integers(300, 4000, (288, 384), dtype=np.uint16)]
    det.matchArray(noise, THR, ["obj"])
    det.submitFrame(noise, THR, ["obj"])                                     # ... and through the ingest ring, whose entries are reused too
    det.collect()
    got = det.matchArray(list(s["frame"]), THR, ["obj"])
    same_records(got, canon)
    assert det.lastTimings()["coarse_candidates"] == st["coarse_candidates"]
    det.submitFrame(list(s["frame"]), THR, ["obj"])
    assert det.collect().tobytes() == got.tobytes()
    det.setBorder("crop")                                                    # the other policy on the same buffers
    same_records(det.matchArray(list(s["frame"]), THR, ["obj"]), expect(s, "crop")[0])


# ---- 3. masks, one modality, grey --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ["pad", "crop"])
def test_masks_come_at_the_source_size(lm, border):
    s = scene("313x229")
    T, W, H = s["T"], s["W"], s["H"]
    rng = np.random.default_rng(9)
    masks = [np.ascontiguousarray(np.kron(rng.integers(0, 4, (H // 16 + 1, W // 16 + 1)) > 0, np.ones((16, 16)))[:H, :W].astype(np.uint8) * 255)
             for _ in range(2)]
    assert all(0 < (m > 0).mean() < 1 for m in masks) and masks[0][:, -1].any() and masks[1][-1].any()
    colour, dep, hm = aligned(s["frame"], T, border, masks)
    raw, st = class_raw(s["od"], masked_memories(s["od"], colour, dep, hm), s["bank"], T, THR, 0)
    canon = lo.canonical_sort_unique(raw)
    unmasked = expect(s, border)[0]
    assert 0 < len(canon) < len(unmasked), "the masks matter"
    det, strict = detector(lm, s, border), detector(lm, s, "strict")
    got = det.matchArray(list(s["frame"]), THR, ["obj"], masks=masks)
    same_records(got, canon)
    assert det.lastTimings()["coarse_candidates"] == st["coarse_candidates"]
    assert got.tobytes() == strict.matchArray([colour, dep], THR, ["obj"], masks=hm).tobytes()
    same_records(det.matchArray(list(s["frame"]), THR, ["obj"], masks=[masks[0], None]),
                 lo.canonical_sort_unique(class_raw(s["od"], masked_memories(s["od"], colour, dep, [hm[0], None]), s["bank"], T, THR, 0)[0]))
    with pytest.raises(RuntimeError, match="LL.cpp:1717"):
        det.matchArray(list(s["frame"]), THR, ["obj"], masks=hm if border == "pad" else [m[:-1] for m in masks])   # not the source size


@pytest.mark.parametrize("border", ["pad", "crop"])
@pytest.mark.parametrize("mods", mr.SETS, ids=lambda m: m[0])
def test_detectors_of_one_modality(lm, mods, border):
    s = scene("313x229")
    T, k = s["T"], mr.KIND[mods[0]]
    colour, dep, _ = aligned(s["frame"], T, border)
    padded = aligned(s["frame"], T, "pad")
    maps = mr.present_maps(s["od"].quantize_pyramid(padded[0], padded[1]), k)
    bank = mr.make_bank(11, 30, 6, maps, T, 63)
    here = mr.present_maps(s["od"].quantize_pyramid(colour, dep), k)
    raw, canon, st = mr.oracle_match(bank, T, *mr.linear_memories(here, T), 62.0)
    assert len(canon) > 0
    det = lm.Detector(63, T, device=0, modalities=mods)
    det.addClassPacked("obj", *mr.pack_single(bank))
    det.setBorder(border)
    src = s["frame"][k]
    got = det.matchArray([src], 62.0, ["obj"])
    assert len(got) == len(canon)
    for g, w in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("template_id", "tid")):
        assert np.array_equal(got[g], canon[w]), g
    assert det.lastTimings()["coarse_candidates"] == st["coarse_candidates"]
    det.submitFrame([src], 62.0, ["obj"])                                   # the ring entry of one image
    assert det.collect().tobytes() == got.tobytes()
    bufs = det.ingestBuffers(s["W"], s["H"])
    assert len(bufs) == 1 and bufs[0].shape[:2] == (s["H"], s["W"])


@pytest.mark.parametrize("border", ["pad", "crop"])
def test_grey_colour_frames(lm, border):
    s = scene("313x229")
    T = s["T"]
    g = np.ascontiguousarray(s["frame"][0][..., 1])
    rep, dep = np.repeat(g[..., None], 3, 2), s["frame"][1]
    colour, depa, _ = aligned((rep, dep), T, border)
    raw, st = oracle_matches(s["od"], colour, depa, s["bank"], T, 50.0)    # (the bank was planted in the colour frame: a lower threshold)
    canon = lo.canonical_sort_unique(raw)
    assert len(canon) > 0
    det = detector(lm, s, border, colour_channels=1)
    got = det.matchArray([g, dep], 50.0, ["obj"])
    same_records(got, canon)
    assert det.lastTimings()["coarse_candidates"] == st["coarse_candidates"]
    det.submitFrame([g, dep], 50.0, ["obj"])                                # rows of 313 bytes: every row starts at another byte offset
    assert det.collect().tobytes() == got.tobytes()


# ---- 4. parked frames and streams --------------------------------------------------------------------------------------------------------------
_stream = {}


def stream_frames():
    """twelve different 313 x 229 frames (frame 0 is the scene's) and the oracle's answer for each under "pad", at a threshold that leaves
    every list non-empty"""
    if not _stream:
        s = scene("313x229")
        frames = [s["frame"]] + [synth.make_frame(40 + i, s["W"], s["H"], 12) for i in range(1, 12)]
        canons = [expect(s, "pad", f, key=("stream", i), thr=45.0)[0] for i, f in enumerate(frames)]
        assert all(len(c) > 0 for c in canons) and len(set(c.tobytes() for c in canons)) == 12
        _stream.update(frames=frames, canons=canons)
    return _stream


def test_parked_frames_have_the_aligned_size(lm):
    s, st = scene("313x229"), stream_frames()
    det = detector(lm, s, "pad")
    for slot in range(3):
        det.storeFrame(slot, list(st["frames"][slot]))
    for slot in (2, 0, 1):
        det.selectFrame(slot)
        same_records(det.matchResident(45.0, ["obj"]), st["canons"][slot])
    crop = detector(lm, s, "crop")
    crop.storeFrame(0, list(s["frame"]))
    crop.selectFrame(0)
    same_records(crop.matchResident(THR, ["obj"]), expect(s, "crop")[0])


def test_a_batch_of_eight_different_frames_is_one_launch(lm):
    s, st = scene("313x229"), stream_frames()
    W, H = s["W"], s["H"]
    det = detector(lm, s, "pad")
    det.setBatch(8)
    det.setBatchQueue(0)                                       # nothing goes out before the batch is full
    for i in range(8):
        rgb, dep = st["frames"][i]
        if i in (1, 6):                                        # filled in place: the pinned entries have the SOURCE size
            bufs = det.ingestBuffers(W, H)
            assert bufs[0].shape == (H, W, 3) and bufs[1].shape == (H, W)
            bufs[0][:], bufs[1][:] = rgb, dep
            det.submitFrame([bufs[0], bufs[1]], 45.0, ["obj"])
        else:
            det.submitFrame([rgb, dep], 45.0, ["obj"])
        assert det.framesLaunched() == (8 if i == 7 else 0)
    with pytest.raises(RuntimeError, match="in flight"):
        det.setBorder("crop")
    assert det.getBorder() == "pad"
    streamed = [det.collect() for _ in range(8)]
    assert det.lastTimings()["batch_frames"] == 8
    for i, got in enumerate(streamed):
        same_records(got, st["canons"][i])
        assert got.tobytes() == det.matchArray(list(st["frames"][i]), 45.0, ["obj"]).tobytes()


def test_match_stream_over_twelve_frames(lm):
    s, st = scene("313x229"), stream_frames()
    det = detector(lm, s, "pad")
    outs = list(det.matchStream([list(f) for f in st["frames"]], 45.0, ["obj"], depth=5))
    assert len(outs) == 12
    for i, got in enumerate(outs):
        same_records(got, st["canons"][i])
        assert got.tobytes() == det.matchArray(list(st["frames"][i]), 45.0, ["obj"]).tobytes()
    crop = detector(lm, s, "crop")
    outs = list(crop.matchStream([list(f) for f in st["frames"][:3]], 45.0, ["obj"]))
    for i, got in enumerate(outs):
        same_records(got, expect(s, "crop", st["frames"][i], key=("stream", i), thr=45.0)[0])
    assert len(outs[0]) > 0


# ---- 5. stages ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["313x229", "310x230_T448"])
def test_read_stage_returns_the_aligned_geometry(lm, name):
    s = scene(name)
    L = len(s["T"])
    host = expect(s, "pad")[2]
    det, strict = detector(lm, s, "pad"), detector(lm, s, "strict")
    for d, src in ((det, s["frame"]), (strict, host)):
        d.setPaths("bits", "bits", 2)                          # (2: the pair stream stays readable after the match)
        d.matchArray(list(src), THR, ["obj"])
    Wa, Ha = host[1].shape[::-1]
    for l in range(L):
        kinds = [0, 1, 2, 3] + ([4] if l < L - 1 else [5])
        for kind in kinds:
            a, b = det.readStage(l, kind), strict.readStage(l, kind)
            assert a.shape == b.shape and a.any() and np.array_equal(a, b), (l, kind)
        assert det.readStage(l, 0).size == (Wa >> l) * (Ha >> l)


# ---- 6. the pipeline ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_equals_the_strict_pipeline_on_the_padded_inputs(lm):
    """60 templates, top_k = 5; R and t bit for bit: the same kernels on the same bytes"""
    s = scene("313x229")
    T, W, H = s["T"], s["W"], s["H"]
    od = s["od"]
    host = expect(s, "pad")[2]
    pyr = od.quantize_pyramid(*host)
    n = 60
    bank = synth.make_planted_bank(13, n, [(p[0], p[1]) for p in pyr], T, nfeat=(64, 32))
    rng = np.random.default_rng(5)
    shapes = [synth.synth_model_depth(200 + k, W, H) for k in range(2)]
    Kv = (K_CAM * np.array([[.5], [.5], [1]], np.float32)).astype(np.float32)
    views = [(shapes[t % 2], Kv, np.eye(3, dtype=np.float32), np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), 1000 + rng.uniform(-20, 20)], np.float32))
             for t in range(n)]
    out = []
    for border in ("pad", "strict"):
        det = lm.Detector(s["nf"], T, device=0)
        det.addClassPacked("obj", *bank)
        det.setBorder(border)
        if border == "pad":
            pipe = lm.Pipeline(det, W, H, scene_from_scene=True)                     # the source size
            pipe.set_views("obj", [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views])
            det.setFrame(list(s["frame"]))
        else:
            pipe = lm.Pipeline(det, 320, 240, scene_from_scene=True)
            pipe.set_views("obj", [fb.pad_zero(v[0], 320, 240) for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views])
            det.setFrame(list(host))
        got, tm = pipe.run(THR, ["obj"], Kv, top_k=5, nms_iou=0.5)
        out.append((got, tm["coarse_candidates"]))
        pipe.close()
    (a, ca), (b, cb) = out
    assert ca == cb and len(a) == len(b) and len(a) > 0
    assert [det_fields(x) for x in a] == [det_fields(y) for y in b]
    assert any(x["status"] == 0 for x in a), "at least one refined pose"
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


# ---- 7. the frame the feature exists for -------------------------------------------------------------------------------------------------------
def test_a_native_t_less_frame(lm):
    s = scene("720x540")
    canon, st, host, nraw = expect(s, "pad")
    assert host[1].shape == (544, 720) and len(canon) > 0
    det = detector(lm, s, "pad")
    got = det.matchArray(list(s["frame"]), THR, ["obj"])
    same_records(got, canon)
    tm = det.lastTimings()
    assert tm["coarse_candidates"] == st["coarse_candidates"] and tm["matches_pre_unique"] == nraw
    assert det.getPaths() == ("bits", "bits")
    det.submitFrame(list(s["frame"]), THR, ["obj"])
    assert det.collect().tobytes() == got.tobytes()


# ---- 8. the policy surface ---------------------------------------------------------------------------------------------------------------------
def test_policy_surface(lm):
    from lm_abi import aligned_size
    s = scene("313x229")
    det = detector(lm, s, "strict")
    assert det.getBorder() == "strict"
    # strict refuses what it refused, in the reference's words.  313 x 229 fails the first of its asserts, (rows * cols) % 16 (LL.cpp:1136), which
    # comes before the T grid's; 312 x 232 passes that one and fails response_map.cols % T at level 1 (LL.cpp:1217-1218).
    near = [np.ascontiguousarray(s["frame"][0][:, :312]), np.ascontiguousarray(np.pad(s["frame"][1], ((0, 3), (0, 0)))[:, :312])]
    near[0] = np.ascontiguousarray(np.pad(near[0], ((0, 3), (0, 0), (0, 0))))
    assert near[0].shape == (232, 312, 3) and near[1].shape == (232, 312)
    for src, line in ((list(s["frame"]), r"LL\.cpp:1136"), (near, r"LL\.cpp:1217-1218")):
        H, W = src[1].shape
        for call in (lambda: det.matchArray(src, THR, ["obj"]), lambda: det.setFrame(src), lambda: det.submitFrame(src, THR, ["obj"]),
                     lambda: det.alignedSize(W, H)):
            with pytest.raises(RuntimeError, match=line):
                call()
    for bad in ("reflect", "", None, 1):
        with pytest.raises(RuntimeError, match="unknown border policy"):
            det.setBorder(bad)
    lib = lm.load_library()
    assert lib.lm_detector_set_border(det._h, 3) < 0 and b"unknown border policy" in lib.lm_last_error()
    assert det.getBorder() == "strict"
    det.setBorder("pad")
    det.setFrame(list(s["frame"]))
    det.submit(THR, ["obj"])
    for other in ("crop", "strict", "pad"):
        with pytest.raises(RuntimeError, match="in flight"):
            det.setBorder(other)
    same_records(det.collect(), expect(s, "pad")[0])
    det.setBorder("strict")                                                 # ... and allowed again, and strict refuses again
    with pytest.raises(RuntimeError, match=r"LL\.cpp:1136"):
        det.matchArray(list(s["frame"]), THR, ["obj"])
    for T in ([4, 8], [5, 8], [4, 4, 8], [5]):
        d = lm.Detector(32, T, device=0)
        for W, H in ((313, 229), (305, 225), (720, 540), (1920, 1080), (848, 480), (320, 240), (640, 480), (17, 16), (100, 75)):
            for border in ("pad", "crop"):
                try:
                    want = aligned_size(T, W, H, border)
                except RuntimeError:
                    with pytest.raises(RuntimeError, match="unsupported frame size"):
                        d.alignedSize(W, H, border)
                    continue
                assert d.alignedSize(W, H, border) == want, (T, W, H, border)
        d.setBorder("crop")
        assert d.alignedSize(720, 540) == aligned_size(T, 720, 540, "crop")   # None: the detector's own policy
    small = lm.Detector(32, [5, 8], device=0)
    small.setBorder("crop")
    with pytest.raises(RuntimeError, match="unsupported frame size"):
        small.setFrame([np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64), np.uint16)])     # nothing of 80 x 80 fits
