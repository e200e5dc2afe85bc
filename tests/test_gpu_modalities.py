"""GPU tests (`-m gpu`) of detectors with ONE modality — Detector(..., modalities=("ColorGradient",)) and ("DepthNormal",) — against the
unchanged two-slot oracle through tests/modality_ref.py (present modality in slot 0, an empty slot 1; test_modality_ref.py pins that
construction to a brute-force scorer and to the reference's own lines)."""
import os

import numpy as np
import pytest

import linemod_oracle as lo
import modality_ref as mr
import response_table_ref as rt
from helpers import K_CAM
from synth import icosphere

pytestmark = pytest.mark.gpu

SETS = mr.SETS
ids_of = lambda m: m[0]                                                                     # noqa: E731
PATHS = [("bits", "bits"), ("bits", "bytes"), ("tiles", "bytes"), ("single", "bytes")]
# (W, H, T, feature counts at level 0): VGA once; 208 x 176 = 52 columns at level 0 (no multiple of 16), 13 at level 1 (bytes, no dwords),
# with the oracle's 8-bit (63) and 16-bit (150) mode; three levels; T = (5, 8)
GEOMS = {"vga": (640, 480, (4, 8), (150,)), "small": (208, 176, (4, 8), (63, 150)), "three": (256, 192, (4, 4, 8), (150,)),
         "t58": (240, 160, (5, 8), (63,))}
THR = 62.0


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def source(sc, mods):
    return [sc["rgb"] if mods[0] == "ColorGradient" else sc["dep"]]


_cases = {}


def case(geom, mods, nf0):
    """scene, bank (planted + random, 48 templates) and the oracle's answer of a (geometry, set, feature count): computed once, never modified"""
    key = (geom, mods, nf0)
    if key not in _cases:
        W, H, T, _ = GEOMS[geom]
        sc = mr.scene(W, H, T)
        maps = mr.present_maps(sc["pyr"], mr.KIND[mods[0]])
        bank = mr.make_bank(11, 36, 12, maps, T, nf0)
        lms, sizes = mr.linear_memories(maps, T)
        raw, canon, st = mr.oracle_match(bank, T, lms, sizes, THR)
        assert len(canon) > 0 and len(set(canon["sim"].tolist())) > 1, "the reference alone: a list with more than one score"
        _cases[key] = {"sc": sc, "bank": bank, "raw": raw, "canon": canon, "st": st, "T": list(T)}
    return _cases[key]


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("class_index", "cls"), ("template_id", "tid")):
        assert np.array_equal(got[g], want[w]), g


def expected_paths(paths, levels):
    return ("single" if paths[0] == "tiles" and levels != 2 else paths[0], paths[1])


# ---- 1. match parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", PATHS, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("geom,nf0", [(g, nf) for g, v in GEOMS.items() for nf in v[3]])
@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_match_equals_the_oracle_on_every_path(lm, mods, geom, nf0, paths):
    c = case(geom, mods, nf0)
    det = lm.Detector(nf0, c["T"], device=0, modalities=mods)
    det.setPaths(*paths)
    det.addClassPacked("obj", *mr.pack_single(c["bank"]))
    got = det.matchArray(source(c["sc"], mods), THR, ["obj"])
    assert det.getPaths() == expected_paths(paths, len(c["T"]))
    same_records(got, c["canon"])
    tm = det.lastTimings()
    assert tm["coarse_candidates"] == c["st"]["coarse_candidates"] and tm["matches_pre_unique"] == len(c["raw"])
    pre = det.matchResident(THR, ["obj"], sort_unique=False)
    assert mr.gpu_multiset(pre) == mr.multiset(c["raw"])


# ---- 2. the front end of the present modality is the default detector's ---------------------------------------------------------------------
@pytest.mark.parametrize("direct", [2, False], ids=["direct", "packed"])
@pytest.mark.parametrize("geom", ["small", "three"])
@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_stages_equal_the_default_detectors(lm, mods, geom, direct):
    c = case(geom, mods, 150)
    sc, T, k = c["sc"], c["T"], mr.KIND[mods[0]]
    L = len(T)
    one, both = lm.Detector(150, T, device=0, modalities=mods), lm.Detector(150, T, device=0)
    one.addClassPacked("obj", *mr.pack_single(c["bank"]))
    if k == 0:                                               # the default detector gets the same features, in the present modality's slot
        packed = lo.pack_bank(mr.two_slot(c["bank"]), L)
    else:
        packed = lo.pack_bank([[s for t in tp for s in (mr.empty_like(t), t)] for tp in c["bank"]], L)
    both.addClassPacked("obj", packed.feat, packed.tmpl_off, packed.tmpl_wh)
    for d in (one, both):
        d.setPaths("bits", "bits", direct)
    one.matchArray(source(sc, mods), THR, ["obj"])
    both.matchArray([sc["rgb"], sc["dep"]], THR, ["obj"])
    assert one.getPaths() == both.getPaths() == ("bits", "bits")
    for l in range(L):
        if l < L - 1:                                        # strip records: the default detector's are [colour block, normal block]
            assert np.array_equal(one.readStage(l, 4), both.readStage(l, 4).reshape(2, -1)[k]), ("strip records", l)
        elif direct:                                         # pair stream (kept readable by direct = 2): the present block's half, zeros in the other
            a, b = one.readStage(l, 5).reshape(2, -1), both.readStage(l, 5).reshape(2, -1)
            assert np.array_equal(a[k], b[k]) and not a[1 - k].any() and a[k].any(), "pair stream"
        assert np.array_equal(one.readStage(l, k), both.readStage(l, k)), ("quantised map", l)
        assert np.array_equal(one.readStage(l, 2 + k), both.readStage(l, 2 + k)) and one.readStage(l, 2 + k).any(), ("linear memory", l)
        for kind in (1 - k, 3 - k):                          # the absent modality's stages
            with pytest.raises(RuntimeError, match="not in the detector's modality set"):
                one.readStage(l, kind)


# ---- 3. masks --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_mask_of_the_present_modality(lm, mods):
    W, H, T, _ = GEOMS["small"]
    c = case("small", mods, 150)
    sc = c["sc"]
    mask = np.zeros((H, W), np.uint8)
    mask[20:150, 30:190] = 255
    pyr = sc["od"].quantize_pyramid(sc["rgb"], sc["dep"], mask)
    lms, sizes = mr.linear_memories(mr.present_maps(pyr, mr.KIND[mods[0]], masked=True), T)
    raw, canon, st = mr.oracle_match(c["bank"], T, lms, sizes, THR)
    assert 0 < len(canon) and mr.multiset(raw) != mr.multiset(c["raw"])
    det = lm.Detector(150, list(T), device=0, modalities=mods)
    det.addClassPacked("obj", *mr.pack_single(c["bank"]))
    same_records(det.matchArray(source(sc, mods), THR, ["obj"], masks=[mask]), canon)
    assert det.lastTimings()["coarse_candidates"] == st["coarse_candidates"]
    with pytest.raises(RuntimeError, match="1714"):
        det.matchArray(source(sc, mods), THR, ["obj"], masks=[mask, mask])


# ---- 4. training -----------------------------------------------------------------------------------------------------------------------------
def train_views(kind):
    """three ordinary views (one of them with colour in one quadrant only: the crop of test_modality_ref), one on which only the PRESENT
    modality finds features, one on which it finds none"""
    views = [mr.view(1), mr.view(2), mr.view(3, colour_quadrant=True)]
    views.append(mr.view(4, flat_depth=True) if kind == 0 else mr.view(4, flat_colour=True))
    return views, (mr.view(5, flat_colour=True) if kind == 0 else mr.view(5, flat_depth=True))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_add_template_equals_the_helper(lm, mods, host, monkeypatch):
    if host:
        monkeypatch.setenv("LM_TRAIN_HOST", "1")
    kind, T = mr.KIND[mods[0]], [4, 8]
    od = lo.OracleDetector(32, T)
    det = lm.Detector(32, T, device=0, modalities=mods)
    views, failing = train_views(kind)
    for i, (rgb, dep, mask) in enumerate(views):
        want = mr.train_expect(od, rgb, dep, mask, kind)
        assert want is not None
        assert det.addTemplate([rgb if kind == 0 else dep], "obj", mask) == i
        mr.same_templates(det.getTemplates("obj", i), want)
    rgb, dep, mask = failing
    assert det.addTemplate([rgb if kind == 0 else dep], "obj", mask) == -1 and det.numTemplates("obj") == len(views)
    assert det.trainStats()[0 if not host else 1] == len(views) + 1


def _rotations(n, seed):
    rng = np.random.default_rng(seed)
    Rs = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        Rs.append(q)
    return np.stack(Rs).astype(np.float32)


@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_rendered_views_equal_add_template_on_the_rendered_images(lm, mods):
    W, H, n, T, kind = 208, 176, 4, [4, 8], mr.KIND[mods[0]]
    K = (K_CAM * np.array([[.325], [.3667], [1]], np.float32)).astype(np.float32)
    V, F, N, C = icosphere(2, radius=70.0, seed=11)
    C[:] = (C // 64) * 64 + 30
    mesh = lm.Mesh(V, F, normals=N, colors=C)
    Rs, ts = _rotations(n, 3), np.tile(np.array([0, 0, 520], np.float32), (n, 1))
    a, b = lm.Detector(32, T, device=0, modalities=mods), lm.Detector(32, T, device=0, modalities=mods)
    ids, wh = lm.add_templates_rendered(a, mesh, "obj", (W, H), K, Rs, ts)
    rgb, depth = mesh.render((W, H), K, Rs, ts)
    want = [b.addTemplate([rgb[i] if kind == 0 else depth[i]], "obj", (depth[i] > 0).astype(np.uint8) * 255) for i in range(n)]
    assert ids.tolist() == want and min(want) >= 0
    for t in want:
        mr.same_templates(a.getTemplates("obj", t), b.getTemplates("obj", t))
        assert len(a.getTemplates("obj", t)) == len(T)


# ---- 5. files --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_class_files_parameters_and_packed_bank(lm, mods, tmp_path):
    kind, T = mr.KIND[mods[0]], [4, 8]
    det = lm.Detector(32, T, device=0, modalities=mods)
    for rgb, dep, mask in train_views(kind)[0][:2]:
        assert det.addTemplate([rgb if kind == 0 else dep], "obj", mask) >= 0
    fmt = str(tmp_path / "%s_templ.yaml")
    det.writeClasses(fmt)
    text = open(fmt % "obj").read()
    assert "modalities: [ %s ]\n" % mods[0] in text and text.count("pyramid_level:") == 2 * len(T)
    again, default, other = lm.Detector(32, T, device=0, modalities=mods), lm.Detector(32, T, device=0), lm.Detector(32, T, device=0, modalities=SETS[1 - kind])
    again.readClasses(["obj"], fmt)
    for t in range(2):
        mr.same_templates(again.getTemplates("obj", t), det.getTemplates("obj", t))
    for d in (default, other):                              # a one-modality file into another set
        with pytest.raises(RuntimeError, match="2047"):
            d.readClasses(["obj"], fmt)
    rgb, dep, mask = mr.view(1)
    assert default.addTemplate([rgb, dep], "pair", mask) == 0
    default.writeClasses(fmt)
    with pytest.raises(RuntimeError, match="2047"):          # ... and the default's file into a one-modality detector
        again.readClasses(["pair"], fmt)
    # Detector.write / read
    det.write(tmp_path / "params.yaml")
    ptext = open(tmp_path / "params.yaml").read()
    assert ptext.count("type:") == 1 and "type: %s" % mods[0] in ptext and "num_features: 32" in ptext
    again.read(tmp_path / "params.yaml")
    assert again.numClasses() == 0 and again.getModalities() == mods and again.pyramidLevels() == 2
    with pytest.raises(RuntimeError, match="modalities must be"):
        default.read(tmp_path / "params.yaml")
    # packed bank
    det.writeBank(tmp_path / "one.bank")
    info = lm.bank_file_info(tmp_path / "one.bank")
    assert lm.bank_file_modalities(tmp_path / "one.bank") == mods and info["num_pyramids"] == 2
    again.readBank(tmp_path / "one.bank")
    for t in range(2):
        mr.same_templates(again.getTemplates("obj", t), det.getTemplates("obj", t))
    for d in (lm.Detector(32, T, device=0), other):
        with pytest.raises(RuntimeError, match="bank holds modalities"):
            d.readBank(tmp_path / "one.bank")
    default.writeBank(tmp_path / "pair.bank")
    with pytest.raises(RuntimeError, match="bank holds modalities"):
        lm.Detector(32, T, device=0, modalities=mods).readBank(tmp_path / "pair.bank")


def test_bank_file_of_the_previous_format_still_loads(lm, golden_dir):
    """tests/golden/two_modality_v1.bank: written by writeBank before the header word named a modality set (the word is zero)."""
    path = os.path.join(golden_dir, "two_modality_v1.bank")
    info = lm.bank_file_info(path)
    assert lm.bank_file_modalities(path) == ("ColorGradient", "DepthNormal") and info["class_ids"] == ["obj"] and info["num_pyramids"] == 2
    det = lm.Detector(32, [4, 8], device=0)
    det.readBank(path)
    assert det.numTemplates("obj") == 2 and len(det.getTemplates("obj", 0)) == 4
    with pytest.raises(RuntimeError, match="bank holds modalities"):
        lm.Detector(32, [4, 8], device=0, modalities=("ColorGradient",)).readBank(path)


# ---- 6. the streamed path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods", SETS, ids=ids_of)
def test_stream_of_ten_frames_in_batches_of_eight(lm, mods):
    W, H, T, _ = GEOMS["small"]
    c = case("small", mods, 150)
    kind = mr.KIND[mods[0]]
    scenes = [c["sc"]] + [mr.scene(W, H, T, seed=20 + i) for i in range(9)]
    frames = [source(s, mods) for s in scenes]
    det = lm.Detector(150, list(T), device=0, modalities=mods)
    det.addClassPacked("obj", *mr.pack_single(c["bank"]))
    det.setBatch(8)
    bufs = det.ingestBuffers(W, H)
    assert len(bufs) == 1 and bufs[0].dtype == (np.uint8 if kind == 0 else np.uint16)
    thr = 45.0
    streamed = list(det.matchStream(frames, thr, ["obj"], depth=10))
    assert len(streamed) == 10
    sync = [det.matchArray(f, thr, ["obj"]) for f in frames]
    for a, b in zip(streamed, sync):
        assert a.tobytes() == b.tobytes()
    assert len(set(s.tobytes() for s in sync)) > 1
    for i in (0, 7):
        maps = mr.present_maps(scenes[i]["pyr"], kind)
        raw, canon, st = mr.oracle_match(c["bank"], T, *mr.linear_memories(maps, T), thr)
        assert len(canon) > 0
        same_records(sync[i], canon)
    # setFrame / matchResident and storeFrame / selectFrame
    det.setFrame(frames[3]); assert det.matchResident(thr, ["obj"]).tobytes() == sync[3].tobytes()
    det.storeFrame(0, frames[5]); det.storeFrame(1, frames[0])
    det.selectFrame(0); assert det.matchResident(thr, ["obj"]).tobytes() == sync[5].tobytes()
    det.selectFrame(1); assert det.matchResident(thr, ["obj"]).tobytes() == sync[0].tobytes()


# ---- 7. the response table stays orthogonal --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["levelup2", "linemod"])
def test_response_table_on_a_colour_only_detector(lm, name):
    W, H, T, _ = GEOMS["small"]
    mods = SETS[0]
    c = case("small", mods, 150)
    r = rt.NAMED[name]
    maps = mr.present_maps(c["sc"]["pyr"], 0)
    thr = rt.THRESHOLDS["planted"][name] - 10.0
    raw, canon, st = mr.oracle_match(c["bank"], T, *mr.linear_memories(maps, T, build=lambda q, t: rt.linear_memory(q, t, r)), thr)
    assert len(canon) > 0 and len(set(canon["sim"].tolist())) > 1
    det = lm.Detector(150, list(T), device=0, modalities=mods)
    det.addClassPacked("obj", *mr.pack_single(c["bank"]))
    det.setResponseTable(r)
    same_records(det.matchArray(source(c["sc"], mods), thr, ["obj"]), canon)
    assert det.getPaths() == (("bits", "bits") if rt.distinct_nonzero(r) <= 2 else ("tiles", "bytes"))
    assert det.lastTimings()["coarse_candidates"] == st["coarse_candidates"]


# ---- 8. the interface ------------------------------------------------------------------------------------------------------------------------
def test_interface(lm):
    both = ("ColorGradient", "DepthNormal")
    for mods in SETS + (both,):
        for args in ((), ([4, 8],), (63, [4, 8])):
            assert lm.Detector(*args, device=0, modalities=mods).getModalities() == mods
    for args in ((), ([4, 8],), (63, [4, 8])):
        assert lm.Detector(*args, device=0).getModalities() == both
    for bad in (("Colour",), ("ColorGradient", "ColorGradient"), ("DepthNormal", "ColorGradient"), (), ("ColorGradient", "DepthNormal", "DepthNormal")):
        with pytest.raises(RuntimeError, match="modalities must be"):
            lm.Detector(63, [4, 8], device=0, modalities=bad)
    rgb, dep, mask = mr.view(1)
    default = lm.Detector(32, [4, 8], device=0)
    for call in (lambda: default.matchArray([rgb], 80.0), lambda: default.addTemplate([rgb], "obj", mask)):
        with pytest.raises(RuntimeError, match="1707"):
            call()
    col, nor = lm.Detector(32, [4, 8], device=0, modalities=SETS[0]), lm.Detector(32, [4, 8], device=0, modalities=SETS[1])
    for det, good, wrong in ((col, rgb, dep), (nor, dep, rgb)):
        with pytest.raises(RuntimeError, match="1707"):
            det.matchArray([rgb, dep], 80.0)
        with pytest.raises(RuntimeError, match="1707"):
            det.addTemplate([rgb, dep], "obj", mask)
        with pytest.raises(RuntimeError, match="must be a uint"):
            det.matchArray([wrong], 80.0)
        with pytest.raises(RuntimeError, match="1714"):
            det.setFrame([good], masks=[mask, mask])
        with pytest.raises(RuntimeError, match="needs both modalities"):
            lm.Pipeline(det, 208, 176)
        with pytest.raises(RuntimeError, match="needs both modalities"):
            det.setShard(0, 2)
        assert det.addTemplate([good], "obj", mask) == 0
        with pytest.raises(RuntimeError, match="needs both modalities"):
            det.setFrame([good]); det.submit(80.0); det.exchangePack(0, 256)
        det.collect()
