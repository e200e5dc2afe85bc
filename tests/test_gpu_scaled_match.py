"""GPU tests (`-m gpu`) of depth-scaled matching (Detector.matchScaled; k_depth_probe / k_coarse_scaled / k_local_scaled, match_scaled.hip)
against scaled_match_ref.py, record for record: all seven fields exact, the similarity bit for bit.  test_scaled_match_ref.py pins that reference
and proves, on the CPU, the conditions on the inputs used here (scaled_cases.py).  Where a variant of the front end has no CPU statement here
(the padded frame, grey colour, the depth-only set, another response table) the reference runs on the byte linear memories the detector built
(readStage kinds 2 and 3, which other suites hold to the oracle)."""
import os

import numpy as np
import pytest

import response_table_ref as rt
import scaled_cases as sc
import scaled_match_ref as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def detector(lm, T, bank, d_train=sc.D_TRAIN, name="planted", **kw):
    det = lm.Detector(150, list(T), device=0, **kw)
    det.addClassPacked(name, *bank)
    if d_train is not None:
        det.setClassTrainDepth(name, d_train)
    return det


def same(got, want_raw):
    want = sm.canonical(want_raw)
    assert got.dtype == lm_dtype() and len(got) == len(want), (len(got), len(want))
    for f in sm.FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert got["similarity"].tobytes() == want["similarity"].tobytes()


def lm_dtype():
    import lm_abi
    return lm_abi.SCALED_MATCH_DTYPE


def device_memories(det, T, depth_only=False):
    """the byte linear memories of the last front end, as the reference takes them"""
    lms = []
    for l in range(len(T)):
        nrm = det.readStage(l, 3)
        lms.append([np.zeros_like(nrm) if depth_only else det.readStage(l, 2), nrm])
    return lms


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", sc.PROBES)
@pytest.mark.parametrize("ladder", sorted(sc.LADDERS))
def test_records_equal_the_reference(lm, ladder, probe):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"])
    lo, hi = sc.PARITY_BOUNDS[ladder]
    want, _ = sc.reference(sc.T2, ladder, probe, sc.THRESHOLD, sc.D_TRAIN, (lo, hi))
    got = det.matchScaled([s["rgb"], s["dep"]], sc.THRESHOLD, ["planted"], scales=sc.LADDERS[ladder], min_scale=lo, max_scale=hi, probe=probe)
    same(got, want)
    assert len(got) > 0


# ---- 2. efficacy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", sc.EFFICACY_Z)
def test_an_object_trained_at_1000_mm_is_found_at_other_depths(lm, z):
    e = sc.efficacy()
    s = e["scenes"][z]
    det = lm.Detector(63, list(sc.EFFICACY_T), device=0)
    det.addClassPacked("obj", *e["bank"])
    det.setClassTrainDepth("obj", e["d_train"])
    assert det.classTrainDepth("obj") == e["d_train"]
    got = det.matchScaled([s["rgb"], s["dep"]], sc.EFFICACY_THRESHOLD, ["obj"], scales=e["scales"])
    same(got, s["want"])
    on = sc.on_object(got, e["box"])
    assert len(on) > 0 and (on["scale_index"] == s["k"]).all()
    x0, y0, w, h = lm.scaled_box(on[0], e["box"], e["scales"])
    assert abs(x0 + w / 2 - 160) <= sc.EFFICACY_RADIUS and abs(w - e["box"][0] * 1000.0 / z) < 0.03 * w
    plain = det.matchResident(sc.EFFICACY_THRESHOLD, ["obj"])
    assert len(sc.on_object(plain, e["box"])) == 0


# ---- 3. the ladder {1024} is matchResident ---------------------------------------------------------------------------------------------------
def test_ladder_1024_equals_match_resident(lm):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"])
    det.setFrame([s["rgb"], s["dep"]])
    got = det.matchScaledResident(sc.THRESHOLD, ["planted"], scales=(1.0,), min_scale=0.25, max_scale=4.0)
    plain = det.matchResident(sc.THRESHOLD, ["planted"])
    assert len(plain) > 0 and (got["scale_index"] == 0).all()
    for f in ("x", "y", "similarity", "class_index", "template_id"):
        assert np.array_equal(np.unique(got[["x", "y", "similarity", "class_index", "template_id"]])[f], np.unique(plain)[f]), f


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bounds", "tie", "double", "half"])
def test_edge_cases_of_the_ladder(lm, case):
    kw = dict(sc.edge_cases()[case])
    s = sc.scene()
    want, _ = sc.reference(**kw)
    det = detector(lm, s["T"], s["bank"], kw.get("d_train", sc.D_TRAIN))
    lo, hi = kw.get("lo_hi", (None, None))
    got = det.matchScaled([s["rgb"], s["dep"]], kw.get("threshold", sc.THRESHOLD), ["planted"], scales=kw["scales"], min_scale=lo, max_scale=hi)
    same(got, want)
    assert len(got) > 0


def test_a_probe_window_of_zeros(lm):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"])
    dep = s["dep"].copy()
    dep[:, :160] = 0                                                                  # the left half has no measurement
    lms, sizes = rt.linear_memories(lm_oracle_pyramid(s, dep), s["T"], rt.DEFAULT)
    want = sm.match_scaled(s["bank"], lms, sizes, s["T"], sc.THRESHOLD, dep, sc.D_TRAIN, sc.ladder_q10(sc.LADDERS[9]))
    got = det.matchScaled([s["rgb"], dep], sc.THRESHOLD, ["planted"])
    same(got, want)
    assert len(got) > 0 and (got["depth_mm"] > 0).all()
    assert len(det.matchScaled([s["rgb"], np.zeros_like(dep)], 10.0, ["planted"])) == 0     # no depth anywhere: nothing is matched


def lm_oracle_pyramid(s, dep):
    import linemod_oracle as lo
    return lo.OracleDetector(150, s["T"]).quantize_pyramid(s["rgb"], dep)


@pytest.mark.parametrize("T", [sc.T1, sc.T3])
def test_one_and_three_level_pyramids(lm, T):
    s = sc.scene(T)
    want, _ = sc.reference(T, 9, 2)
    det = detector(lm, T, s["bank"])
    same(det.matchScaled([s["rgb"], s["dep"]], sc.THRESHOLD, ["planted"]), want)
    assert len(want) > 0


def test_grow_and_rerun_under_a_small_candidate_capacity(lm):
    s = sc.scene()
    want, st = sc.reference(sc.T2, 9, 2, 40.0)
    assert st["candidates"] > 2 * 1024
    det = detector(lm, s["T"], s["bank"])
    det.setCandidateCapacity(1024)
    same(det.matchScaled([s["rgb"], s["dep"]], 40.0, ["planted"]), want)


def variant(lm, det, frame, T, bank, threshold=sc.THRESHOLD, depth_only=False, dep=None):
    got = det.matchScaled(frame, threshold, ["planted"])
    Wa, Ha = det.alignedSize(frame[-1].shape[1], frame[-1].shape[0])
    lms = device_memories(det, T, depth_only)
    sizes = [(Wa >> l, Ha >> l) for l in range(len(T))]
    depth = np.zeros((Ha, Wa), np.uint16)
    d = frame[-1] if dep is None else dep
    depth[:d.shape[0], :d.shape[1]] = d                                                # the padding's depth is 0
    want = sm.match_scaled(bank, lms, sizes, list(T), threshold, depth, sc.D_TRAIN, sc.ladder_q10(sc.LADDERS[9]))
    same(got, want)
    assert len(got) > 0
    return got


def test_a_300_x_200_frame_under_pad(lm):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"])
    det.setBorder("pad")
    assert det.alignedSize(300, 200) == (304, 208)
    variant(lm, det, [np.ascontiguousarray(s["rgb"][:200, :300]), np.ascontiguousarray(s["dep"][:200, :300])], sc.T2, s["bank"])


def test_grey_colour_frames(lm):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"], colour_channels=1)
    grey = np.ascontiguousarray(s["rgb"][..., 1])
    variant(lm, det, [grey, s["dep"]], sc.T2, s["bank"], threshold=60.0)


def test_the_depth_only_modality_set(lm):
    s = sc.scene()
    two, one = sc.normals_only(s["bank"], 2)
    det = detector(lm, s["T"], one, modalities=("DepthNormal",))
    variant(lm, det, [s["dep"]], sc.T2, two, depth_only=True)


def test_the_response_table_linemod(lm):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"])
    det.setResponseTable("linemod")
    got = variant(lm, det, [s["rgb"], s["dep"]], sc.T2, s["bank"], threshold=84.0)
    lms, sizes = rt.linear_memories(s["pyr"], s["T"], rt.NAMED["linemod"])              # ... and against the CPU's memories of that table
    same(got, sm.match_scaled(s["bank"], lms, sizes, s["T"], 84.0, s["dep"], sc.D_TRAIN, sc.ladder_q10(sc.LADDERS[9])))


# ---- 5. repeatability ------------------------------------------------------------------------------------------------------------------------
def test_a_second_call_is_identical_and_plain_matching_is_untouched(lm):
    s = sc.scene()
    det = detector(lm, s["T"], s["bank"])
    det.setFrame([s["rgb"], s["dep"]])
    before = det.matchResident(sc.THRESHOLD, ["planted"])
    a = det.matchScaledResident(sc.THRESHOLD, ["planted"])
    b = det.matchScaledResident(sc.THRESHOLD, ["planted"])
    after = det.matchResident(sc.THRESHOLD, ["planted"])
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    assert len(before) > 0 and before.tobytes() == after.tobytes()
    c = det.matchScaledResident(sc.THRESHOLD, ["planted"], scales=sc.LADDERS[3])      # another ladder: the cached tables are rebuilt
    same(c, sc.reference(sc.T2, 3, 2)[0])
    same(det.matchScaledResident(sc.THRESHOLD, ["planted"]), sc.reference(sc.T2, 9, 2)[0])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(lm):
    s = sc.scene()
    frame = [s["rgb"], s["dep"]]
    det = detector(lm, s["T"], s["bank"], d_train=None)
    with pytest.raises(RuntimeError, match="no frame resident"):
        det.matchScaledResident(sc.THRESHOLD, ["planted"])
    det.setFrame(frame)
    with pytest.raises(RuntimeError, match="has no training depth"):
        det.matchScaledResident(sc.THRESHOLD, ["planted"])
    with pytest.raises(RuntimeError, match="1..65535"):
        det.setClassTrainDepth("planted", 0)
    with pytest.raises(RuntimeError, match="unknown class"):
        det.setClassTrainDepth("nothing", 1000)
    assert det.classTrainDepth("planted") is None
    det.setClassTrainDepth("planted", sc.D_TRAIN)
    for bad, msg in ((dict(scales=()), "1..16 scales"), (dict(scales=tuple(1.0 + 0.01 * i for i in range(17))), "1..16 scales"),
                     (dict(scales=(1.0, 1.0)), "strictly ascending"), (dict(scales=(1.25, 1.0)), "strictly ascending"),
                     (dict(scales=(0.4, 1.0)), r"outside \[512, 2048\]"), (dict(scales=(1.0, 2.1)), r"outside \[512, 2048\]"),
                     (dict(scales=(1.0,), min_scale=1.5, max_scale=1.0), "bad scale bounds"), (dict(probe=5), "probe must be in 0..4"),
                     (dict(probe=-1), "probe must be in 0..4")):
        with pytest.raises(RuntimeError, match=msg):
            det.matchScaledResident(sc.THRESHOLD, ["planted"], **bad)
    det.setPartMatching(2)
    with pytest.raises(RuntimeError, match="not available under part matching"):
        det.matchScaledResident(sc.THRESHOLD, ["planted"])
    det.setPartMatching(0)
    det.submit(sc.THRESHOLD, ["planted"])
    with pytest.raises(RuntimeError, match="frames in flight"):
        det.matchScaledResident(sc.THRESHOLD, ["planted"])
    det.collect()
    assert len(det.matchScaledResident(sc.THRESHOLD, ["planted"])) > 0                  # ... and it still matches
    assert det._lib.lm_detector_exchange_pack(det._h, None, 4096) != 0                  # a scaled match leaves nothing for the exchange
    assert "no frame in flight" in det._lib.lm_last_error().decode()
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    with pytest.raises(RuntimeError, match="serves a pipeline"):
        det.matchScaledResident(sc.THRESHOLD, ["planted"])
    del pipe
    sharded = detector(lm, s["T"], s["bank"])
    sharded.setShard(0, 2)
    sharded.setFrame(frame)
    with pytest.raises(RuntimeError, match="sharded detector"):
        sharded.matchScaledResident(sc.THRESHOLD, ["planted"])
    colour = lm.Detector(150, list(s["T"]), device=0, modalities=("ColorGradient",))
    with pytest.raises(RuntimeError, match="needs the DepthNormal modality"):
        colour.matchScaledResident(sc.THRESHOLD)
