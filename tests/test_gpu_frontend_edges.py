"""GPU tests (`-m gpu`) of the front end (csrc/fe_quant.hip, csrc/fe_bits.hip) away from the default modality parameters and on the frames of frontend_cases.py:
every comparison is exact, against the oracle that test_frontend_cases.py holds to the scalar restatement on the same frames.

The parameters are set the way a user sets them: the detector writes its parameter file, the values are replaced in the text, Detector.read()
takes it.  The oracle gets the same values as attributes.  What is compared: the quantised maps and linear memories of both levels (readStage
0 .. 3), the strip records and the pair stream as the front end's own writers leave them (4, 5), the normals BEFORE the median (8: the 5 x 5
median hides a wrong raw normal at fewer than 13 of 25 taps), the streamed path, grey / one-modality / padded instantiations, a match per
parameter set and addTemplate."""
import os
import re

import numpy as np
import pytest

import frame_border_ref as fb
import frontend_cases as fc
import linemod_oracle as lo
import modality_ref as mr
import synth
from helpers import oracle_matches
from test_gpu_parity import _pair_stream, _strip_records, expect_paths, same_records

pytestmark = pytest.mark.gpu

KEYS = ("weak_threshold", "strong_threshold", "distance_threshold", "difference_threshold")
NAMES = list(fc.all_cases())


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def configure(det, tmp_path, p):
    """det.write() -> the values of p replaced in the text -> det.read(): the file a user would edit.  Clears the classes."""
    path = str(tmp_path / "params.yaml")
    det.write(path)
    text = open(path).read()
    mods = det.getModalities()
    for k in KEYS:
        if k not in p:
            continue
        present = ("ColorGradient" if k in KEYS[:2] else "DepthNormal") in mods
        text, n = re.subn(r"(%s:) \S+" % k, lambda m: "%s %r" % (m.group(1), p[k]), text)
        assert n == (1 if present else 0), (k, n)
    with open(path, "w") as f:
        f.write(text)
    det.read(path)
    assert det.numClasses() == 0


def oracle_for(nf, T, p):
    od = lo.OracleDetector(nf, list(T))
    for k in KEYS:
        if k in p:
            setattr(od, k, p[k])
    return od


_pyr = {}


def oracle_pyramid(c):
    """the oracle's quantised pyramid of a case: computed once, never modified"""
    if c["name"] not in _pyr:
        _pyr[c["name"]] = oracle_for(8, c["T"], c["params"]).quantize_pyramid(c["rgb"], c["dep"])
    return _pyr[c["name"]]


EMPTY = (np.zeros((0, 3), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))


def check_stages(det, c, pyr, sources=None):
    """readStage 0 .. 3 of every level against the oracle's pyramid, as test_frontend_stages_bit_exact compares them, after a synchronous match"""
    T = c["T"]
    det.addClassPacked("e", *EMPTY)
    det.setFrame([c["rgb"], c["dep"]] if sources is None else sources)
    det.matchResident(75.0, ["e"])
    for l, (qc, qn, *_r) in enumerate(pyr):
        n = 8 * qc.size
        assert np.array_equal(det.readStage(l, 0).reshape(qc.shape), qc), (c["name"], "orientations level %d" % l)
        assert np.array_equal(det.readStage(l, 1).reshape(qn.shape), qn), (c["name"], "normals level %d" % l)
        assert np.array_equal(det.readStage(l, 2), lo.build_linear_memories(qc, T[l])[:n]), (c["name"], "LM colour level %d" % l)
        assert np.array_equal(det.readStage(l, 3), lo.build_linear_memories(qn, T[l])[:n]), (c["name"], "LM normal level %d" % l)


def check_raw_normals(det, c):
    p = c["params"]
    want = lo.quantized_normals_raw(c["dep"], p["distance_threshold"], p["difference_threshold"])
    got = det.readStage(0, 8).reshape(want.shape)
    assert np.array_equal(got, want), (c["name"], "normals before the median", int((got != want).sum()))


def check_bit_planes(lm, c, pyr, tmp_path):
    """kinds 4 and 5 as the front end's own writers leave them (direct 2 / 10 / 6), against the numpy packing of the oracle's linear memories"""
    T, (H, W) = c["T"], c["dep"].shape
    L = len(T)
    lms = [[lo.build_linear_memories(p[0], T[l]), lo.build_linear_memories(p[1], T[l])] for l, p in enumerate(pyr)]
    bank = synth.make_random_bank(3, 2, 96, 64, nfeat=(8, 4))                # (templates of 6 .. 19 x 7 .. 21 pixels: they fit the lowest frame, 1280 x 32)
    for direct in (2, 10, 6):
        det = lm.Detector(8, T, device=0)
        configure(det, tmp_path, c["params"])
        det.setPaths("bits", "bits", direct)
        det.addClassPacked("o", *bank)
        det.setFrame([c["rgb"], c["dep"]])
        det.matchResident(70.0, ["o"])
        assert det.getPaths() == ("bits", "bits")
        for l in range(L - 1):
            Wd, Hd = (W >> l) // T[l], (H >> l) // T[l]
            rec = det.readStage(l, 4).view(np.uint64).reshape(2, 8, T[l] * T[l], (Wd + 15) // 16, Hd)
            for m in range(2):
                assert np.array_equal(rec[m], _strip_records(lms[l][m], T[l], Wd, Hd)), (c["name"], direct, "strip records", l, m)
        Wd, Hd = (W >> (L - 1)) // T[-1], (H >> (L - 1)) // T[-1]
        ps = det.readStage(L - 1, 5).view(np.uint32).reshape(-1, 2)
        assert np.array_equal(ps, _pair_stream(lms[L - 1][0], lms[L - 1][1], T[-1], Wd, Hd, len(ps))), (c["name"], direct, "pair stream")


# ---- 1. the parameters take effect ---------------------------------------------------------------------------------------------------------
def test_a_parameter_file_with_other_values_changes_the_stages(lm, tmp_path):
    """Each of weak_threshold, distance_threshold and difference_threshold, changed alone in the file, changes readStage output against the
    defaults on the same frame — and the output is the oracle's under that value."""
    rgb, dep = fc.all_cases()["at_threshold"]["rgb"], fc.all_cases()["steep_planes_diff150"]["dep"]
    base = {"name": "defaults", "rgb": rgb, "dep": dep, "T": [2, 2], "params": fc.params()}
    det = lm.Detector(8, [2, 2], device=0)
    check_stages(det, base, oracle_for(8, [2, 2], base["params"]).quantize_pyramid(rgb, dep))
    default = [det.readStage(0, k).copy() for k in (0, 1)]
    for kw, kind in (({"weak_threshold": 4.0}, 0), ({"distance_threshold": 1500}, 1), ({"difference_threshold": 150}, 1)):
        c = dict(base, name=str(kw), params=fc.params(**kw))
        configure(det, tmp_path, c["params"])
        check_stages(det, c, oracle_for(8, [2, 2], c["params"]).quantize_pyramid(rgb, dep))
        assert not np.array_equal(det.readStage(0, kind), default[kind]), kw
        assert np.array_equal(det.readStage(0, 1 - kind), default[1 - kind]), kw
    configure(det, tmp_path, base["params"])
    check_stages(det, base, oracle_for(8, [2, 2], base["params"]).quantize_pyramid(rgb, dep))
    assert all(np.array_equal(det.readStage(0, k), default[k]) for k in (0, 1))


# ---- 2. every case ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_oracle(lm, name, tmp_path):
    """quantised maps and linear memories of every level, the raw normals, and (two levels, frames of 96 x 64 and larger) the bit planes of
    the three front-end writers"""
    c = fc.all_cases()[name]
    fc.check_conditions(c)
    pyr = oracle_pyramid(c)
    det = lm.Detector(8, c["T"], device=0)
    configure(det, tmp_path, c["params"])
    check_stages(det, c, pyr)
    check_raw_normals(det, c)
    if len(c["T"]) == 2 and c["dep"].shape[1] >= 96:
        check_bit_planes(lm, c, pyr, tmp_path)


def test_raw_normals_read_back(lm):
    """readStage(0, 8): level 0 only, the normals' modality only, after addTemplate too; at default parameters it differs from the median's output"""
    c = fc.all_cases()["near_zero_diff50"]
    det = lm.Detector(8, c["T"], device=0)
    check_stages(det, c, oracle_pyramid(c))
    check_raw_normals(det, c)
    assert not np.array_equal(det.readStage(0, 8), det.readStage(0, 1))
    with pytest.raises(RuntimeError):
        det.readStage(1, 8)
    with pytest.raises(RuntimeError):
        det.readStage(0, 9)
    col = lm.Detector(8, c["T"], device=0, modalities=("ColorGradient",))
    col.addClassPacked("e", *EMPTY)
    col.matchArray([c["rgb"]], 75.0, ["e"])
    with pytest.raises(RuntimeError, match="not in the detector's modality set"):
        col.readStage(0, 8)


# ---- 3. the streamed path --------------------------------------------------------------------------------------------------------------------
STREAM = ("sat_steps", "channel_ties", "vote_edges", "axis_and_diagonal", "at_threshold", "steep_planes_diff150", "near_zero_diff150",
          "extremes_diff150_dist65536", "distance_edge_diff150_dist2000", "collinear_diff150")


@pytest.mark.parametrize("batch", [8, 1])
def test_streamed_frames_under_non_default_parameters(lm, batch, tmp_path):
    """Ten frames of different cases (colour of one, depth of another) through submitFrame under weak 4.0 / distance 40000 / difference 150:
    every frame's records equal the synchronous call's, the synchronous records equal the oracle's, and the stages of the last frame (left by
    the batch's launch, not by a synchronous one) equal the oracle's."""
    p = fc.params(weak_threshold=4.0, distance_threshold=40000, difference_threshold=150)
    cases = fc.all_cases()
    frames = [[cases[STREAM[i % 5]]["rgb"], cases[STREAM[5 + (i + i // 5) % 5]]["dep"]] for i in range(10)]       # ten different pairs
    T, thr = [2, 2], 50.0
    od = oracle_for(8, T, p)
    pyr0 = od.quantize_pyramid(*frames[1])
    bank = synth.make_planted_bank(4, 4, [(q[0], q[1]) for q in pyr0], T, (8, 4), windows=[(10 + 6 * i, 8 + 2 * i, 56, 44) for i in range(4)])
    det = lm.Detector(8, T, device=0)
    configure(det, tmp_path, p)
    det.addClassPacked("o", *bank)
    det.setBatch(batch)
    det.setBatchQueue(0)
    for f in frames:                                                         # (batches of 8: frames 0 .. 7 launch together, 8 and 9 at the first collect that needs them)
        det.submitFrame(f, thr, ["o"])
    streamed = [det.collect() for _ in frames]
    last = {"name": "streamed frame 9", "rgb": frames[9][0], "dep": frames[9][1], "T": T, "params": p}
    pyr = od.quantize_pyramid(*frames[9])
    sync = [det.matchArray(f, thr, ["o"]) for f in frames]
    for i, (a, b) in enumerate(zip(streamed, sync)):
        assert a.tobytes() == b.tobytes(), ("streamed frame", i)
    assert len(set(s.tobytes() for s in sync)) >= 4 and len(sync[1]) > 0 and len(sync[5]) > 0
    for i in (1, 5, 9):
        raw, _ = oracle_matches(od, frames[i][0], frames[i][1], bank, T, thr)
        same_records(sync[i], lo.canonical_sort_unique(raw))
    det2 = lm.Detector(8, T, device=0)                                       # the last frame streamed alone: the stages its launch leaves (a batch that ignored the parameters would leave the default maps)
    configure(det2, tmp_path, p)
    det2.addClassPacked("o", *bank)
    det2.setBatch(batch)
    det2.setBatchQueue(0)
    det2.submitFrame(frames[9], thr, ["o"])
    assert det2.collect().tobytes() == sync[9].tobytes()
    for l, (qc, qn, *_r) in enumerate(pyr):
        n = 8 * qc.size
        assert np.array_equal(det2.readStage(l, 0).reshape(qc.shape), qc), ("streamed orientations", l)
        assert np.array_equal(det2.readStage(l, 1).reshape(qn.shape), qn), ("streamed normals", l)
        assert np.array_equal(det2.readStage(l, 2), lo.build_linear_memories(qc, T[l])[:n]), ("streamed LM colour", l)
        assert np.array_equal(det2.readStage(l, 3), lo.build_linear_memories(qn, T[l])[:n]), ("streamed LM normal", l)
    check_raw_normals(det2, last)
    dflt = oracle_for(8, T, fc.params()).quantize_pyramid(*frames[9])
    assert not np.array_equal(dflt[0][0], pyr[0][0]) and not np.array_equal(dflt[0][1], pyr[0][1]), "the parameters must matter on this frame"


# ---- 4. other instantiations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sat_steps", "at_threshold", "vote_edges"])
def test_grey_detector_on_the_cases(lm, name, tmp_path):
    c = fc.all_cases()[name]
    g = np.ascontiguousarray(c["rgb"][..., 0])
    rep = dict(c, name=name + " (grey)", rgb=np.ascontiguousarray(np.repeat(g[..., None], 3, 2)))
    pyr = oracle_for(8, c["T"], c["params"]).quantize_pyramid(rep["rgb"], rep["dep"])
    assert pyr[0][0].any() and pyr[1][0].any()
    grey, col = lm.Detector(8, c["T"], device=0, colour_channels=1), lm.Detector(8, c["T"], device=0)
    for det in (grey, col):
        configure(det, tmp_path, c["params"])
    check_stages(grey, rep, pyr, sources=[g, c["dep"]])
    check_stages(col, rep, pyr)
    for l in range(2):
        for k in range(4):
            assert np.array_equal(grey.readStage(l, k), col.readStage(l, k)), (name, l, k)


@pytest.mark.parametrize("name,mods", [("extremes_diff70000_dist65536", ("DepthNormal",)), ("extremes_diff150_dist65535", ("DepthNormal",)),
                                       ("near_zero_diff49", ("DepthNormal",)), ("near_zero_diff151", ("DepthNormal",)), ("channel_ties", ("ColorGradient",))])
def test_one_modality_detectors_on_the_cases(lm, name, mods, tmp_path):
    c = fc.all_cases()[name]
    k = mr.KIND[mods[0]]
    pyr = oracle_pyramid(c)
    det = lm.Detector(8, c["T"], device=0, modalities=mods)
    configure(det, tmp_path, c["params"])
    det.addClassPacked("e", *EMPTY)
    det.setFrame([c["rgb"] if k == 0 else c["dep"]])
    det.matchResident(75.0, ["e"])
    for l, p in enumerate(pyr):
        n = 8 * p[k].size
        assert p[k].any() and np.array_equal(det.readStage(l, k).reshape(p[k].shape), p[k]), (name, "quantised map", l)
        assert np.array_equal(det.readStage(l, 2 + k), lo.build_linear_memories(p[k], c["T"][l])[:n]), (name, "linear memory", l)
    if k == 1:
        check_raw_normals(det, c)


@pytest.mark.parametrize("name", ["sat_steps", "steep_planes_diff150"])
def test_padded_crop_of_the_cases(lm, name, tmp_path):
    """setBorder("pad") on the 93 x 61 crop: the stages of the strict detector on the host-padded frame, and the oracle's on it"""
    c = fc.all_cases()[name]
    rgb, dep = np.ascontiguousarray(c["rgb"][:61, :93]), np.ascontiguousarray(c["dep"][:61, :93])
    pad, strict = lm.Detector(8, c["T"], device=0), lm.Detector(8, c["T"], device=0)
    for det in (pad, strict):
        configure(det, tmp_path, c["params"])
    pad.setBorder("pad")
    Wa, Ha = pad.alignedSize(93, 61)
    assert (Wa, Ha) != (93, 61)
    prgb, pdep, _m = fb.pad_frame(rgb, dep, Wa, Ha, ())
    host = dict(c, name=name + " (padded on the host)", rgb=prgb, dep=pdep)
    pyr = oracle_for(8, c["T"], c["params"]).quantize_pyramid(prgb, pdep)
    check_stages(strict, host, pyr)
    check_stages(pad, host, pyr, sources=[rgb, dep])
    check_raw_normals(pad, host)
    for l in range(2):
        for k in range(4):
            a, b = pad.readStage(l, k), strict.readStage(l, k)
            assert a.shape == b.shape and a.any() and np.array_equal(a, b), (name, l, k)


# ---- 5. a match per parameter set --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [("bits", "bits"), ("tiles", "bytes")], ids=["bits-bits", "tiles-bytes"])
@pytest.mark.parametrize("name", ["near_zero_160x128_diff49", "at_threshold_160x128"])
def test_match_under_the_parameters(lm, name, paths, tmp_path):
    """a bank planted from the oracle's maps under the case's parameters; the records equal the oracle's"""
    c = fc.all_cases()[name]
    T, thr = c["T"], 60.0
    od = oracle_for(8, T, c["params"])
    pyr = oracle_pyramid(c)
    bank = synth.make_planted_bank(5, 6, [(p[0], p[1]) for p in pyr], T, (8, 4), windows=[(20 + 6 * i, 20 + 4 * i, 100, 80) for i in range(6)])
    raw, st = oracle_matches(od, c["rgb"], c["dep"], bank, T, thr)
    want = lo.canonical_sort_unique(raw)
    assert len(want) >= 4 and st["local_evals"] > 0
    det = lm.Detector(8, T, device=0)
    configure(det, tmp_path, c["params"])
    det.setPaths(*paths)
    det.addClassPacked("o", *bank)
    same_records(det.matchArray([c["rgb"], c["dep"]], thr, ["o"]), want)
    expect_paths(det, paths)
    tm = det.lastTimings()
    assert tm["coarse_candidates"] == st["coarse_candidates"] and tm["matches_pre_unique"] == len(raw)


# ---- 6. training -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mods", [("at_threshold_160x128", ("ColorGradient",)), ("near_zero_160x128_diff49", ("DepthNormal",)),
                                       ("near_zero_160x128_diff49", ("ColorGradient", "DepthNormal"))], ids=["colour", "normals", "both"])
def test_add_template_under_the_parameters(lm, name, mods, tmp_path):
    """addTemplate runs the same kernels with the magnitude output on: the template equals the oracle's under weak / strong 4.0 and the
    case's depth thresholds (strong_threshold 4.0: at 55 the low-contrast frame has no colour feature)"""
    c = fc.all_cases()[name]
    p = dict(c["params"], strong_threshold=4.0)
    H, W = c["dep"].shape
    mask = np.zeros((H, W), np.uint8)
    mask[8:H - 8, 8:W - 8] = 255
    od = oracle_for(8, c["T"], p)
    det = lm.Detector(8, c["T"], device=0, modalities=mods)
    configure(det, tmp_path, p)
    if len(mods) == 2:
        assert od.addTemplate([c["rgb"], c["dep"]], "o", mask) == 0
        want = od.class_templates["o"][0]
        assert det.addTemplate([c["rgb"], c["dep"]], "o", mask) == 0
    else:
        k = mr.KIND[mods[0]]
        want = mr.train_expect(od, c["rgb"], c["dep"], mask, k)
        assert want is not None
        assert det.addTemplate([c["rgb"] if k == 0 else c["dep"]], "o", mask) == 0
    assert all(len(t.features) > 0 for t in want)
    mr.same_templates(det.getTemplates("o", 0), want)
    if "DepthNormal" in mods:                                                # the training front end leaves the raw normals too
        check_raw_normals(det, dict(c, params=p))
