"""GPU tests (`-m gpu`) of the depth slabs: Detector.depthModes, setClassDepthRange and matchSlabs / matchSlabsResident.

depthModes is held to the numpy statement of its rule (tests/depth_slabs_ref.py, itself checked by hand in test_depth_slabs_ref.py), exactly.
matchSlabs is held to the CPU oracle, field for field: per primary depth the numpy slab mask (ANDed with the user's masks) goes through the
oracle's own masking — quantize() copies through the mask, LL.cpp:583-587, and the mask follows the pyramid by nearest-neighbour halving,
:573-578 — into its linear memories and match_oracle.c, per class of the slab; the classes without a range are matched under the user's masks
alone; everything is merged with lo.canonical_sort_unique.  (lo.OracleDetector.match takes `masks` and ignores them, so the expectation is put
together from the oracle's parts, as test_gpu_frame_border.py does for masked frames.)

The scene is synth.make_frame(21, 320, 240, 12): with min_pixels=500 it has the modes 1187, 912, 762 and 1012 mm (asserted on the CPU in
test_depth_slabs_ref.py).  Three classes of about 40 templates planted in the oracle's quantisation of the frame: "far" holds 1187 only,
"near" holds 762 and 912, "free" has no range; 1012 falls in no range.  The request also names a class that does not exist."""
import os

import numpy as np
import pytest

import depth_slabs_ref as ds
import frame_border_ref as fb
import linemod_oracle as lo
import modality_ref as mr
import response_table_ref as rt
import synth
from helpers import class_raw

pytestmark = pytest.mark.gpu

THR = 70.0
T = [4, 8]
NAMES = ["far", "ghost", "near", "free"]                     # "ghost" is in no detector: skipped, and the positions stay
RANGES = {"far": (1100, 1300), "near": (700, 950)}
MODES = dict(min_pixels=500)
FIXTURE_MODES = [1187, 912, 762, 1012]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def blocky_masks(seed, W, H):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(np.kron(rng.integers(0, 4, (H // 16 + 1, W // 16 + 1)) > 0, np.ones((16, 16)))[:H, :W].astype(np.uint8) * 255)
            for _ in range(2)]


_scenes = {}


def scene(kind):
    """kind: "colour" (both modalities, 320x240), "grey" (the same frame's green channel as a grey image), "pad" (the frame cut to 313x229,
    matched under "pad"), "depth" (a DepthNormal detector).  Frame, aligned frame, unmasked quantised pyramid and the three banks: computed
    once, never modified."""
    if kind not in _scenes:
        rgb, dep = synth.make_frame(21, 320, 240, 12)
        if kind == "pad":
            rgb, dep = np.ascontiguousarray(rgb[:229, :313]), np.ascontiguousarray(dep[:229, :313])
        if kind == "grey":
            g = np.ascontiguousarray(rgb[..., 1])
            rgb = np.ascontiguousarray(np.repeat(g[..., None], 3, 2))
        colour, depa = (rgb, dep) if kind != "pad" else fb.pad_frame(rgb, dep, 320, 240, ())[:2]
        nf = 63 if kind == "depth" else 64
        od = lo.OracleDetector(nf, T)
        pyr = od.quantize_pyramid(colour, depa)
        if kind == "depth":
            maps = mr.present_maps(pyr, 1)
            banks = {n: mr.make_bank(s, 30, 6, maps, T, 63) for n, s in (("far", 11), ("near", 12), ("free", 13))}
        else:
            banks = {n: synth.make_planted_bank(s, 40, [(p[0], p[1]) for p in pyr], T, nfeat=(64, 32)) for n, s in (("far", 11), ("near", 12), ("free", 13))}
        src = [dep] if kind == "depth" else ([np.ascontiguousarray(rgb[..., 1]), dep] if kind == "grey" else [rgb, dep])
        _scenes[kind] = {"kind": kind, "src": src, "host": (colour, depa), "od": od, "pyr": pyr, "banks": banks, "nf": nf, "memo": {}}
    return _scenes[kind]


def memories(sc, masks, table):
    """the oracle's linear memories of the aligned frame under one mask per modality (None: unmasked), for a response table (None: the default)"""
    L = len(T)
    quant = [[], []]
    for m in range(2):
        msk = masks[m] if m < len(masks) else None
        for l in range(L):
            if l > 0 and msk is not None:
                msk = lo.nn_down2(msk)
            q = sc["pyr"][l][3 + m]
            quant[m].append(q if msk is None else np.where(msk > 0, q, 0).astype(np.uint8))
    build = lo.build_linear_memories if table is None else (lambda q, t: rt.linear_memory(q, t, table))
    sizes = [(q.shape[1], q.shape[0]) for q in quant[0]]
    if sc["kind"] == "depth":
        return mr.linear_memories([np.ascontiguousarray(q) for q in quant[1]], T, build), sizes
    return [[build(np.ascontiguousarray(quant[0][l]), T[l]), build(np.ascontiguousarray(quant[1][l]), T[l])] for l in range(L)], sizes


def class_records(sc, name, mem, thr, pos):
    if sc["kind"] == "depth":
        (lms, _sizes), sizes = mem
        raw = mr.oracle_match(sc["banks"][name], T, lms, sizes, thr)[0]
        raw["cls"] = pos
        return raw
    return class_raw(sc["od"], mem, sc["banks"][name], T, thr, pos)[0]


def expect(sc, user=(None, None), thr=THR, table=None, slab_mm=150, ranges=RANGES, names=NAMES, **mode_options):
    """(canonical merged list, the slab dicts) as the header defines matchSlabs, from the numpy rule and the CPU oracle"""
    key = (tuple(id(u) for u in user), thr, table, slab_mm, tuple(sorted(ranges.items())), tuple(names), tuple(sorted(mode_options.items())))
    if key in sc["memo"]:
        return sc["memo"][key]
    dep = sc["host"][1]
    if sc["kind"] == "depth":
        user = (None, user[0])                              # the one mask of a depth-only detector belongs to the normals
    raws, slabs = [np.zeros(0, lo.MATCH_DTYPE)], []
    for m in ds.depth_modes(dep, **mode_options):
        p = int(m["depth_mm"])
        pos = [i for i, n in enumerate(names) if n in sc["banks"] and n in ranges and ranges[n][0] <= p <= ranges[n][1]]
        records = 0
        if pos:
            S = ds.slab_mask(dep, p, slab_mm)
            mem = memories(sc, [S if u is None else (S & u) for u in user], table)
            for i in pos:
                raws.append(class_records(sc, names[i], mem, thr, i))
                records += len(raws[-1])
        slabs.append({"depth_mm": p, "pixels": int(m["pixels"]), "lo_mm": p - slab_mm, "hi_mm": p + slab_mm,
                      "class_ids": [names[i] for i in pos], "records": records})
    free = [i for i, n in enumerate(names) if n in sc["banks"] and n not in ranges]
    if free:
        mem = memories(sc, list(user), table)
        records = 0
        for i in free:
            raws.append(class_records(sc, names[i], mem, thr, i))
            records += len(raws[-1])
        slabs.append({"depth_mm": None, "pixels": None, "lo_mm": None, "hi_mm": None, "class_ids": [names[i] for i in free], "records": records})
    sc["memo"][key] = (lo.canonical_sort_unique(np.concatenate(raws)), slabs)
    return sc["memo"][key]


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for a, b in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("class_index", "cls"), ("template_id", "tid")):
        assert np.array_equal(got[a], want[b]), a


def detector(lm, sc, ranges=RANGES, **kw):
    if sc["kind"] == "depth":
        det = lm.Detector(63, T, device=0, modalities=("DepthNormal",), **kw)
        for n, bank in sc["banks"].items():
            det.addClassPacked(n, *mr.pack_single(bank))
    else:
        det = lm.Detector(sc["nf"], T, device=0, colour_channels=1 if sc["kind"] == "grey" else 3, **kw)
        for n, bank in sc["banks"].items():
            det.addClassPacked(n, *bank)
    if sc["kind"] == "pad":
        det.setBorder("pad")
    for n, (lo_mm, hi_mm) in ranges.items():
        det.setClassDepthRange(n, lo_mm, hi_mm)
    return det


def check_slabs(det, sc, user=(), thr=THR, table=None, paths=("bits", "bits"), modes=FIXTURE_MODES):
    """matchSlabs against the oracle, with everything the issue asks of a case"""
    users = tuple(user) if len(user) else (None, None)
    want, want_slabs = expect(sc, users, thr, table, **MODES)
    got, slabs = det.matchSlabs(sc["src"], thr, NAMES, masks=list(user), **MODES)
    assert [s["depth_mm"] for s in want_slabs] == modes + [None]
    assert len(want) > 0, "the merged list is not empty"
    assert sum(1 for s in want_slabs[:-1] if s["records"] > 0) >= 1, "at least one slab contributes records"
    assert slabs == want_slabs
    assert modes[3] == 1012 and slabs[3]["class_ids"] == [] and slabs[3]["records"] == 0
    assert slabs[0]["class_ids"] == ["far"] and slabs[1]["class_ids"] == slabs[2]["class_ids"] == ["near"] and slabs[4]["class_ids"] == ["free"]
    same_records(got, want)
    assert det.getPaths() == paths
    plain = det.matchArray(sc["src"], thr, NAMES, masks=list(user))
    assert len(plain) != len(got) or plain.tobytes() != got.tobytes(), "the slabs did something"
    return got, slabs


# ---- 1. depthModes ----------------------------------------------------------------------------------------------------------------------------
def modes_detector(lm):
    return lm.Detector(64, T, device=0, modalities=("DepthNormal",))


@pytest.mark.parametrize("frame", [(21, 320, 240, 12), (7, 160, 160, 6), (3, 640, 480, 40)], ids=lambda f: "%dx%d" % f[1:3])
def test_depth_modes_equal_the_rule_on_synthetic_frames(lm, frame):
    _rgb, dep = synth.make_frame(*frame)
    det = modes_detector(lm)
    det.setFrame([dep])
    for opt in (dict(), dict(min_pixels=500), dict(window=0, min_pixels=200, max_modes=16), dict(max_modes=1),
                dict(bin_mm=1, near_mm=300, far_mm=4396, min_pixels=20, max_modes=16), dict(bin_mm=4000, near_mm=1, far_mm=4001),
                dict(bin_mm=7, near_mm=555, far_mm=1234, window=5, min_pixels=1)):
        want = ds.depth_modes(dep, **opt)
        got = det.depthModes(**opt)
        ds.same_modes(got, want)
        ds.same_modes(det.depthModes(**opt), got)                      # the same call twice
    assert len(ds.depth_modes(dep, min_pixels=500)) >= 3
    assert ds.num_bins(1, 300, 4396) == 4096 and ds.num_bins(4000, 1, 4001) == 1


@pytest.mark.parametrize("border", ["pad", "crop"])
def test_depth_modes_of_a_frame_that_is_not_aligned(lm, border):
    rgb, dep = synth.make_frame(21, 313, 229, 12)
    det = lm.Detector(64, T, device=0)
    det.setBorder(border)
    det.setFrame([rgb, dep])
    Wa, Ha = det.alignedSize(313, 229)
    host = fb.pad_frame(rgb, dep, Wa, Ha, ())[1] if border == "pad" else fb.crop_frame(rgb, dep, Wa, Ha, ())[1]
    assert host.shape == (Ha, Wa) and host.shape != dep.shape
    for opt in (dict(min_pixels=500), dict(bin_mm=10, window=3, min_pixels=100, max_modes=16)):
        ds.same_modes(det.depthModes(**opt), ds.depth_modes(host, **opt))
    assert len(ds.depth_modes(host, min_pixels=500)) >= 3


def test_depth_modes_of_degenerate_images(lm):
    det = modes_detector(lm)
    near, far = 300, 4000
    zero = np.zeros((240, 320), np.uint16)
    const = np.full((240, 320), 1234, np.uint16)
    edge = np.tile(np.array([near, far - 1, far, 0, 65535, near - 1, near, far - 1], np.uint16), (240, 40))
    odd = np.zeros((48, 48), np.uint16)                                # a few pixels only, at both ends of a row
    odd[0, 0], odd[0, -1], odd[-1, -1] = 700, 700, 3999
    for dep, n in ((zero, 0), (const, 1), (edge, 2), (odd, 2)):
        det.setFrame([np.ascontiguousarray(dep)])
        for opt in (dict(min_pixels=1), dict(window=0, min_pixels=1, max_modes=16), dict()):
            want = ds.depth_modes(dep, **opt)
            ds.same_modes(det.depthModes(**opt), want)
        assert len(ds.depth_modes(dep, min_pixels=1)) == n
    det.setFrame([const])
    assert det.depthModes()["pixels"].tolist() == [240 * 320] and det.depthModes()["depth_mm"].tolist() == [300 + 37 * 25 + 12]


# ---- 2. matchSlabs against the oracle ------------------------------------------------------------------------------------------------------------
def test_match_slabs_equal_the_oracle(lm):
    sc = scene("colour")
    det = detector(lm, sc)
    got, slabs = check_slabs(det, sc)
    assert set(got["class_index"].tolist()) <= {0, 2, 3} and 3 in got["class_index"]      # positions in the request, "ghost" skipped
    # every class by default: sorted classIds(), and the positions follow
    all_got, all_slabs = det.matchSlabs(sc["src"], THR, (), **MODES)
    want, want_slabs = expect(sc, names=["far", "free", "near"], **MODES)
    same_records(all_got, want)
    assert all_slabs == want_slabs
    # slab_mm and the mode options reach the device: a thin slab, three modes
    thin, thin_slabs = det.matchSlabs(sc["src"], THR, NAMES, slab_mm=40, min_pixels=1000)
    want, want_slabs = expect(sc, slab_mm=40, min_pixels=1000)
    same_records(thin, want)
    assert thin_slabs == want_slabs and [s["depth_mm"] for s in thin_slabs] == [1187, 912, 762, None]


def test_match_slabs_with_a_user_mask_on_each_modality(lm):
    sc = scene("colour")
    masks = sc.setdefault("masks", blocky_masks(9, 320, 240))
    assert all(0 < (m > 0).mean() < 1 for m in masks)
    det = detector(lm, sc)
    got, slabs = check_slabs(det, sc, user=masks)
    unmasked = expect(sc, **MODES)[0]
    assert len(got) < len(unmasked), "the user's masks matter"
    one = [masks[0], None]                                               # a mask on one modality: the other reads the slab alone
    same_records(det.matchSlabs(sc["src"], THR, NAMES, masks=one, **MODES)[0], expect(sc, (masks[0], None), **MODES)[0])


def test_match_slabs_on_a_depth_only_detector(lm):
    sc = scene("depth")
    det = detector(lm, sc)
    check_slabs(det, sc, thr=62.0)
    mask = sc.setdefault("masks", blocky_masks(9, 320, 240))[:1]        # a depth-only detector takes one mask
    got, _slabs = det.matchSlabs(sc["src"], 62.0, NAMES, masks=mask, **MODES)
    want = expect(sc, (mask[0], None), 62.0, **MODES)[0]
    assert 0 < len(want) < len(expect(sc, (None, None), 62.0, **MODES)[0])
    same_records(got, want)


def test_match_slabs_with_a_grey_colour_image(lm):
    sc = scene("grey")
    det = detector(lm, sc)
    assert det.getColourChannels() == 1
    check_slabs(det, sc)


def test_match_slabs_of_a_padded_frame(lm):
    sc = scene("pad")
    assert sc["src"][1].shape == (229, 313) and sc["host"][1].shape == (240, 320)
    det = detector(lm, sc)
    check_slabs(det, sc, modes=[1212, 912, 762, 1012])       # (the cut moves the background's peak one bin up; "far" still holds it)


def test_match_slabs_on_the_wide_paths_under_the_linemod_table(lm):
    sc = scene("colour")
    det = detector(lm, sc)
    det.setPaths("wide", "wide")
    det.setResponseTable("linemod")
    check_slabs(det, sc, thr=84.0, table=rt.NAMED["linemod"], paths=("wide", "wide"))


# ---- 3. nothing of a slab call stays behind -----------------------------------------------------------------------------------------------------
def test_the_resident_call_and_what_follows_it(lm):
    sc = scene("colour")
    masks = sc.setdefault("masks", blocky_masks(9, 320, 240))
    det = detector(lm, sc)
    plain = det.matchArray(sc["src"], THR, NAMES)
    det.setFrame(sc["src"], masks)
    before = det.matchResident(THR, NAMES)
    assert len(before) > 0 and before.tobytes() != plain.tobytes()
    got, slabs = det.matchSlabsResident(THR, NAMES, **MODES)
    same_records(got, expect(sc, tuple(masks), **MODES)[0])
    assert det.matchResident(THR, NAMES).tobytes() == before.tobytes()          # the frame's own masks are what they were
    again, again_slabs = det.matchSlabsResident(THR, NAMES, **MODES)
    assert again.tobytes() == got.tobytes() and again_slabs == slabs
    both, both_slabs = det.matchSlabs(sc["src"], THR, NAMES, masks=masks, **MODES)
    assert both.tobytes() == got.tobytes() and both_slabs == slabs
    assert det.matchArray(sc["src"], THR, NAMES).tobytes() == plain.tobytes()   # no slab mask in a plain match
    det.submitFrame(sc["src"], THR, NAMES)                                      # ... nor in a streamed one
    assert det.collect().tobytes() == plain.tobytes()
    with pytest.raises(RuntimeError, match="setFrame"):
        det.matchSlabsResident(THR, NAMES, masks=masks)


# ---- 4. refusals and the surface -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_ranges(lm, tmp_path):
    sc = scene("colour")
    det = detector(lm, sc)
    assert det.getClassDepthRange("far") == (1100, 1300) and det.getClassDepthRange("free") is None
    det.setClassDepthRange("far", None, None)
    assert det.getClassDepthRange("far") is None
    det.setClassDepthRange("far", 1187, 1187)                                    # lo == hi is a range
    assert det.getClassDepthRange("far") == (1187, 1187)
    with pytest.raises(RuntimeError, match="above hi_mm"):
        det.setClassDepthRange("far", 1301, 1300)
    assert det.getClassDepthRange("far") == (1187, 1187)                         # a refused set changes nothing
    for call in (lambda: det.setClassDepthRange("ghost", 1, 2), lambda: det.getClassDepthRange("ghost"), lambda: det.setClassDepthRange("ghost", None, None)):
        with pytest.raises(RuntimeError, match="unknown class"):
            call()
    with pytest.raises(RuntimeError, match="integers"):
        det.setClassDepthRange("far", 1.5, 2)
    det.setFrame(sc["src"])
    for bad, words in ((dict(bin_mm=1, near_mm=300, far_mm=4397), "nbins"), (dict(near_mm=4000), "nbins"), (dict(bin_mm=0), "bin_mm"),
                       (dict(near_mm=0), "near_mm"), (dict(far_mm=65537), "far_mm"), (dict(window=-1), "window"), (dict(max_modes=0), "max_modes"),
                       (dict(max_modes=17), "max_modes"), (dict(min_pixels=0), "min_pixels")):
        for call in (lambda: det.depthModes(**bad), lambda: det.matchSlabsResident(THR, NAMES, **bad), lambda: det.matchSlabs(sc["src"], THR, NAMES, **bad)):
            with pytest.raises(RuntimeError, match=words):
                call()
    with pytest.raises(RuntimeError, match="slab_mm"):
        det.matchSlabsResident(THR, NAMES, slab_mm=-1)
    with pytest.raises(TypeError):
        det.depthModes(bins=3)
    # ranges are in no file
    fmt = str(tmp_path / "%s_templ.yaml")
    det.writeClasses(fmt)
    back = lm.Detector(sc["nf"], T, device=0)
    back.readClasses(["far", "near", "free"], fmt)
    assert [back.getClassDepthRange(n) for n in ("far", "near", "free")] == [None, None, None]
    bank = str(tmp_path / "bank.bin")
    det.writeBank(bank)
    back = lm.Detector(sc["nf"], T, device=0)
    back.readBank(bank)
    assert back.classIds() == ["far", "free", "near"] and [back.getClassDepthRange(n) for n in back.classIds()] == [None, None, None]
    # without ranges a slab call is a plain match, reported as the one pass without a slab
    got, slabs = back.matchSlabs(sc["src"], THR, NAMES, **MODES)
    assert got.tobytes() == back.matchArray(sc["src"], THR, NAMES).tobytes() and len(got) > 0
    assert [s["class_ids"] for s in slabs] == [[], [], [], [], ["far", "near", "free"]] and slabs[-1]["depth_mm"] is None
    # a detector without a depth image
    col = lm.Detector(sc["nf"], T, device=0, modalities=("ColorGradient",))
    col.setFrame([sc["src"][0]])
    for call in (lambda: col.depthModes(), lambda: col.matchSlabsResident(THR), lambda: col.matchSlabs([sc["src"][0]], THR)):
        with pytest.raises(RuntimeError, match="no depth image"):
            call()
    # a sharded detector
    det.setShard(0, 2)
    with pytest.raises(RuntimeError, match="sharded"):
        det.matchSlabs(sc["src"], THR, NAMES, **MODES)
    det.setShard(0, 1)
    # no resident frame
    fresh = detector(lm, sc)
    with pytest.raises(RuntimeError, match="no frame resident"):
        fresh.depthModes()
    with pytest.raises(RuntimeError, match="no frame resident"):
        fresh.matchSlabsResident(THR, NAMES)
