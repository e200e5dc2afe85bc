"""GPU tests (`-m gpu`) of the "wide" matching paths (Detector.setPaths("wide", "wide"); match_wide.hip): response tables of three or four
distinct non-zero values on two sets of bit planes.  The yardstick is the unchanged CPU oracle fed with the linear memories
response_table_ref.py builds for the table; the plane contents are held to wide_planes_ref.py, the numpy statement of the encoding that
test_wide_planes_ref.py checks on the CPU."""
import functools
import os

import numpy as np
import pytest

import linemod_oracle as lo
import response_table_ref as rt
import synth
import wide_planes_ref as wp
from helpers import K_CAM, det_fields, nms_chain_oracle

pytestmark = pytest.mark.gpu

WIDE = ("wide", "wide")
NAMED_WIDE = [(n, rt.NAMED[n]) for n in ("linemod", "drop1", "drop1_keep3")]
PLANE_TABLES = [rt.NAMED["linemod"], rt.NAMED["drop1"], rt.NAMED["drop1_keep3"], (4, 3, 2, 2, 1), (4, 4, 3, 1, 1)]
FIELDS = ["x", "y", "similarity", "class_index", "template_id"]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("class_index", "cls"), ("template_id", "tid")):
        assert np.array_equal(got[g], want[w]), g


def multiset(rec, names):
    return sorted(zip(*[rec[n].tolist() for n in names]))


@functools.lru_cache(maxsize=None)
def _narrow_scene():
    """104 x 96 at T = 4, 4: 26 and 13 cells per row, whole dwords at neither level; templates of at most 16 x 17 pixels."""
    W, H, T = 104, 96, [4, 4]
    rgb, dep = synth.make_frame(34, W, H, 14)
    pyr = lo.OracleDetector(150, T).quantize_pyramid(rgb, dep)
    bank = synth.make_random_bank(44, 8, W, H, (16, 8))
    assert bank[2].max() <= 32 and bank[0][:, :2].min() >= 0
    return {"W": W, "H": H, "T": T, "rgb": rgb, "dep": dep, "pyr": pyr, "banks": {"planted": bank}}


def scene_and_memories(geom):
    if geom == "narrow":
        sc = _narrow_scene()
        return sc, lambda r: rt.linear_memories(sc["pyr"], sc["T"], tuple(r))[0]
    return rt.scene(geom), lambda r: rt.memories(geom, tuple(r))[0]


def wide_detector(lm, sc, kinds, paths=WIDE, direct=True):
    det = lm.Detector(150, sc["T"], device=0)
    det.setPaths(paths[0], paths[1], direct)
    for k in kinds:
        det.addClassPacked(k, *sc["banks"][k])
    return det


def oracle_raw(geom, kinds, r, thr):
    raws, coarse, evals = [], 0, 0
    for i, kind in enumerate(kinds):
        raw, st = rt.oracle(geom, kind, tuple(r), thr)
        raw = raw.copy()
        raw["cls"] = i
        raws.append(raw)
        coarse += st["coarse_candidates"]; evals += st["local_evals"]
    return np.concatenate(raws), coarse, evals


# ---- 1. plane contents ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["G1", "G2", "G3", "narrow"])
def test_both_sets_of_planes_equal_the_numpy_packing(lm, geom):
    """After a match under ("wide", "wide"): readStage kinds 4 / 6 (strip records, sets 0 / 1) and 5 / 7 (pair streams) equal the numpy packing
    of the table's memories bit for bit, at every level and for both modalities, and kinds 2 / 3 still equal the byte memories."""
    sc, memories = scene_and_memories(geom)
    W, H, T = sc["W"], sc["H"], sc["T"]
    L = len(T)
    det = wide_detector(lm, sc, ["planted"])
    det.setFrame([sc["rgb"], sc["dep"]])
    for r in PLANE_TABLES:
        assert rt.distinct_nonzero(r) > 2
        det.setResponseTable(r)
        det.matchResident(70.0, ["planted"])
        assert det.getPaths() == WIDE and det.refinesOnBitPlanes(), (r, det.getPaths())
        lms = memories(r)
        for l in range(L - 1):
            Wd, Hd = (W >> l) // T[l], (H >> l) // T[l]
            shape = (2, 8, T[l] * T[l], (Wd + 15) // 16, Hd)
            got = [det.readStage(l, k).view(np.uint64).reshape(shape) for k in (4, 6)]
            for m in range(2):
                want = wp.strip_records(lms[l][m], T[l], Wd, Hd, r)
                for s in range(2):
                    assert np.array_equal(got[s][m], want[s]), (r, "strip records", l, m, s)
        Wd, Hd = (W >> (L - 1)) // T[-1], (H >> (L - 1)) // T[-1]
        got = [det.readStage(L - 1, k).view(np.uint32).reshape(-1, 2) for k in (5, 7)]
        want = wp.pair_streams(lms[L - 1][0], lms[L - 1][1], T[-1], Wd, Hd, len(got[0]), r)
        for s in range(2):
            assert np.array_equal(got[s], want[s]), (r, "pair stream", s)
        assert got[1][:, 0].any()                                   # (the table does use the second set)
        for l in range(L):
            n = 8 * (W >> l) * (H >> l)
            for m in range(2):
                assert np.array_equal(det.readStage(l, 2 + m), lms[l][m][:n]), (r, "linear memory", l, m)


# ---- 2. matches ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [WIDE, ("wide", "bytes")], ids=["wide-wide", "wide-bytes"])
@pytest.mark.parametrize("geom", ["G1", "G2", "G3"])
def test_matches_equal_the_oracle(lm, geom, paths):
    """The three named tables of three or four values: canonical list, pre-unique multiset, coarse candidates, refinement evaluations and
    matches_pre_unique equal the oracle's — planted banks (150 and fewer than 64 features) on one detector, the random bank (some of its
    windows leave their planes: the per-candidate launch behind k_local_wide) on another — and getPaths() names the kernels."""
    sc = rt.scene(geom)
    dets = [(wide_detector(lm, sc, kinds, paths), kinds) for kinds in (("planted", "small"), ("random",))]
    for name, r in NAMED_WIDE:
        for det, kinds in dets:
            thr = rt.THRESHOLDS[kinds[0]][name]
            raw, coarse, evals = oracle_raw(geom, kinds, r, thr)
            assert len(raw) > 0
            det.setResponseTable(name)
            got = det.matchArray([sc["rgb"], sc["dep"]], thr, list(kinds))
            assert det.getPaths() == paths and det.refinesOnBitPlanes(), (det.getPaths(), name)
            same_records(got, lo.canonical_sort_unique(raw))
            tm = det.lastTimings()
            assert (tm["coarse_candidates"], tm["local_evals"], tm["matches_pre_unique"]) == (coarse, evals, len(raw)), (name, kinds)
            pre = det.matchResident(thr, list(kinds), sort_unique=False)
            assert multiset(pre, FIELDS) == multiset(raw, ["x", "y", "sim", "cls", "tid"])


# ---- 3. every table that needs the second set, once ----------------------------------------------------------------------------------------
def test_every_wide_table_once(lm):
    """G1, planted bank, threshold 90 (planted templates score near 100 under every table: r[0] = 4): the canonical list equals the oracle's
    for each of the 35 legal tables of three or four distinct non-zero values, none skipped, none with an empty list."""
    geom = "G1"
    sc = rt.scene(geom)
    det = wide_detector(lm, sc, ["planted"])
    det.setFrame([sc["rgb"], sc["dep"]])
    tables = [r for r in rt.legal_tables() if rt.distinct_nonzero(r) > 2]
    assert len(tables) == 35
    for r in tables:
        raw, _ = rt.oracle(geom, "planted", r, 90.0)
        assert len(raw) > 0, r
        det.setResponseTable(r)
        same_records(det.matchResident(90.0, ["planted"]), lo.canonical_sort_unique(raw))
        assert det.getPaths() == WIDE, r


# ---- 4. tables of two planes under "wide" --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,thr", [("levelup", 70.0), ("levelup2", 72.0), ((4, 4, 4, 4, 4), 99.0)], ids=["default", "levelup2", "44444"])
def test_two_plane_tables_run_what_bits_runs(lm, table, thr):
    geom = "G1"
    sc = rt.scene(geom)
    L = len(sc["T"])
    r = rt.NAMED[table] if isinstance(table, str) else table
    out = []
    for paths in (WIDE, ("bits", "bits")):
        det = wide_detector(lm, sc, ["planted", "small"], paths, direct=2)     # (2: the pair stream stays readable after the match)
        det.setResponseTable(r)
        got = det.matchArray([sc["rgb"], sc["dep"]], thr, ["planted", "small"])
        assert det.getPaths() == ("bits", "bits") and det.wideArenaBytes() == (0, 0)
        planes = [det.readStage(l, 4).tobytes() for l in range(L - 1)] + [det.readStage(L - 1, 5).tobytes()]
        with pytest.raises(RuntimeError, match="no second set of strip records"):
            det.readStage(0, 6)
        out.append((got.tobytes(), planes, det.bitArenaBytes()))
    assert out[0] == out[1]
    raw, _, _ = oracle_raw(geom, ("planted", "small"), r, thr)
    assert len(raw) > 0
    same_records(got, lo.canonical_sort_unique(raw))


# ---- 5. memory -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [WIDE, ("wide", "bytes")], ids=["wide-wide", "wide-bytes"])
def test_second_arenas_appear_with_the_first_wide_match(lm, paths):
    geom = "G3"
    sc = rt.scene(geom)
    L = len(sc["T"])
    frame = [sc["rgb"], sc["dep"]]
    det = wide_detector(lm, sc, ["planted"], paths)
    det.matchArray(frame, 70.0, ["planted"])
    assert det.getPaths() == ("bits", paths[1] if paths[1] == "bytes" else "bits")
    first = det.bitArenaBytes()
    assert det.wideArenaBytes() == (0, 0) and min(first) > 0
    det.setResponseTable("linemod")
    assert det.wideArenaBytes() == (0, 0)                           # ... not by selecting the table either
    det.matchArray(frame, 84.0, ["planted"])
    assert det.getPaths() == paths
    strips, pairs = det.wideArenaBytes()
    assert strips >= sum(len(det.readStage(l, 6)) for l in range(L - 1)) > 0
    if paths[1] == "wide":
        assert pairs >= len(det.readStage(L - 1, 7)) > 0
    else:
        assert pairs == 0
        with pytest.raises(RuntimeError, match="no second pair stream"):
            det.readStage(L - 1, 7)
    assert det.bitArenaBytes() == first
    after = det.wideArenaBytes()
    det.setResponseTable("levelup")
    det.matchArray(frame, 70.0, ["planted"])
    assert det.bitArenaBytes() == first and det.wideArenaBytes() == after    # a table of two planes in between adds nothing
    det.setResponseTable("drop1")
    det.matchArray(frame, 74.0, ["planted"])                        # the next result slot serves its first wide match: its second arenas, the same sizes
    assert det.bitArenaBytes() == first and det.wideArenaBytes() == (2 * after[0], 2 * after[1])
    slots = lm.load_library().lm_detector_max_in_flight()
    assert slots * after[0] == first[0] and slots * after[1] in (0, first[1])   # per slot the size of the first set


# ---- 6. switching --------------------------------------------------------------------------------------------------------------------------
def test_switching_tables_on_one_wide_detector(lm):
    geom = "G2"
    sc = rt.scene(geom)
    frame = [sc["rgb"], sc["dep"]]
    det = wide_detector(lm, sc, ["planted"])
    first = det.matchArray(frame, 70.0, ["planted"])
    assert det.getPaths() == ("bits", "bits")
    det.setResponseTable("linemod")
    mid = det.matchResident(84.0, ["planted"])                      # the resident frame, its planes rebuilt under the new table
    assert det.getPaths() == WIDE
    want = lo.canonical_sort_unique(rt.oracle(geom, "planted", rt.NAMED["linemod"], 84.0)[0])
    assert len(want) > 0
    same_records(mid, want)
    det.setResponseTable("levelup")
    third = det.matchResident(70.0, ["planted"])
    assert det.getPaths() == ("bits", "bits")
    assert first.tobytes() == third.tobytes()
    same_records(first, lo.canonical_sort_unique(rt.oracle(geom, "planted", rt.DEFAULT, 70.0)[0]))
    # with a frame in flight both sets are refused, and nothing changes
    det.setResponseTable("linemod")
    det.submit(84.0, ["planted"])
    with pytest.raises(RuntimeError, match="frames in flight"):
        det.setPaths("bits", "bits")
    with pytest.raises(RuntimeError, match="frames in flight: collect them before changing the response table"):
        det.setResponseTable("levelup")
    assert det.getResponseTable() == rt.NAMED["linemod"]
    assert det.collect().tobytes() == mid.tobytes() and det.getPaths() == WIDE
    assert det.matchResident(84.0, ["planted"]).tobytes() == mid.tobytes() and det.getPaths() == WIDE


def test_what_set_paths_refuses(lm):
    det = lm.Detector(63, [4, 8], device=0)
    for refine in ("bits", "tiles", "single"):
        with pytest.raises(RuntimeError, match="plans no tiles"):
            det.setPaths(refine, "wide")
    lib = lm.load_library()                                         # the C ABI's own range check names the new values
    for refine, coarse in ((4, 0), (3, 3)):
        assert lib.lm_detector_set_paths(det._h, refine, coarse) < 0
        msg = lib.lm_last_error().decode()
        assert "3 (wide bit planes)" in msg and "2 (wide bit planes)" in msg, msg
    det.setPaths("wide", "bytes"); det.setPaths("wide", "wide")
    # a sharded detector: refused either way round, with a message
    with pytest.raises(RuntimeError, match="not available on a sharded detector"):
        det.setShard(0, 2)
    det.setPaths("bits", "bits")
    det.setShard(0, 2)
    with pytest.raises(RuntimeError, match="not available on a sharded detector"):
        det.setPaths("wide", "wide")


# ---- 7. streamed path ----------------------------------------------------------------------------------------------------------------------
def test_streamed_frames_on_the_wide_paths(lm):
    """submitFrame / collect of three different frames with setBatch(2) under linemod: the records of the synchronous call and of the oracle."""
    geom = "G1"
    sc = rt.scene(geom)
    W, H, T = sc["W"], sc["H"], sc["T"]
    r, thr = rt.NAMED["linemod"], rt.THRESHOLDS["random"]["linemod"]
    frames = [(sc["rgb"], sc["dep"])] + [synth.make_frame(900 + i, W, H, 14) for i in range(2)]
    feat, offs, wh = sc["banks"]["random"]
    bank = lo.PackedBank((len(offs) - 1) // (2 * len(T)), len(T), feat, offs, wh)
    want = []
    for rgb, dep in frames:
        lms, sizes = rt.linear_memories(sc["od"].quantize_pyramid(rgb, dep), T, r)
        raw, _ = lo.match_bank_c(bank, lms, sizes, T, thr)
        raw["cls"] = 0
        assert len(raw) > 0
        want.append(lo.canonical_sort_unique(raw))
    det = wide_detector(lm, sc, ["random"])
    det.setResponseTable("linemod")
    sync = [det.matchArray(list(f), thr, ["random"]) for f in frames]
    det.setBatch(2)
    for f in frames:
        det.submitFrame(list(f), thr, ["random"])
    for s, w in zip(sync, want):
        got = det.collect()
        same_records(got, w)
        assert got.tobytes() == s.tobytes()
    assert det.getPaths() == WIDE


# ---- 8. pipeline ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_on_the_wide_paths(lm):
    """Pipeline.run takes paths and table from its detector: match, NMS and top-k fields equal the oracle's chain on the table's memories."""
    W, H, T, nfeat, thr = 320, 240, [4, 8], (64, 32), 84.0
    rgb, dep = synth.make_frame(3, W, H)
    od = lo.OracleDetector(nfeat[0], T)
    pyr = od.quantize_pyramid(rgb, dep)
    bank = synth.make_planted_bank(41, 80, [(p[0], p[1]) for p in pyr], T, nfeat)
    lms_sizes = rt.linear_memories(pyr, T, rt.NAMED["linemod"])
    det = lm.Detector(nfeat[0], T, device=0)
    det.setPaths(*WIDE)
    det.addClassPacked("obj", *bank)
    det.setResponseTable("linemod")
    pipe = lm.Pipeline(det, W, H, scene_from_scene=True)
    for iou, k in ((0.5, 16), (0.3, 64)):
        ch = nms_chain_oracle(od, rgb, dep, [{"bank": bank}], T, thr, iou, k, lms_sizes=lms_sizes)
        assert len(ch["sel"]) > 1
        det.setFrame([rgb, dep])
        got, tm = pipe.run(thr, ["obj"], K_CAM, top_k=k, nms_iou=iou)
        assert det.getPaths() == WIDE
        assert tm["nms_records"] == ch["m"]
        assert [det_fields(g) for g in got] == ch["sel"]
    pipe.close()


# ---- 9. the 14-bit counters ----------------------------------------------------------------------------------------------------------------
def test_entries_beyond_511_features_take_the_14_bit_instantiation(lm):
    """Entries of 650 (level 0) and 595 (top level) features under linemod: k_local_wide<10, .> / k_coarse_wide<10, .> — still ("wide", "wide"),
    still the oracle's records and statistics."""
    geom = "G1"
    sc = rt.scene(geom)
    T = sc["T"]
    qp = [(p[0], p[1]) for p in sc["pyr"]]
    windows = [(34 + 2 * i, 34 + 2 * (i % 2), 100, 90) for i in range(12)]       # 100 x 90 pixels: room for 520 normal features at level 1
    feat, offs, wh = bank = synth.make_planted_bank(45, 12, qp, T, ((150, 500), (75, 520)), windows=windows)
    assert (offs[2] - offs[0], offs[4] - offs[2]) == (650, 595)
    r, thr = rt.NAMED["linemod"], 84.0
    lms, sizes = rt.memories(geom, r)
    raw, st = lo.match_bank_c(lo.PackedBank(12, len(T), feat, offs, wh), lms, sizes, T, thr)
    raw["cls"] = 0
    assert len(raw) > 0
    det = lm.Detector(150, T, device=0)
    det.setPaths(*WIDE)
    det.addClassPacked("big", *bank)
    det.setResponseTable("linemod")
    same_records(det.matchArray([sc["rgb"], sc["dep"]], thr, ["big"]), lo.canonical_sort_unique(raw))
    assert det.getPaths() == WIDE
    tm = det.lastTimings()
    assert (tm["coarse_candidates"], tm["local_evals"], tm["matches_pre_unique"]) == (st["coarse_candidates"], st["local_evals"], len(raw))
