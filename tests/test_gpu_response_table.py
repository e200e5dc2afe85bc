"""GPU tests (`-m gpu`) of the selectable response table (Detector.setResponseTable): response memories of every writer, matches on every
kernel path, the streamed path, switching on one detector and the pipeline — against the unchanged CPU oracle fed with linear memories that
response_table_ref.py builds in numpy for the table.  test_response_table_ref.py pins that spec to the oracle and shows that the inputs used
here tell the tables apart."""
import functools
import os

import numpy as np
import pytest

import linemod_oracle as lo
import response_table_ref as rt
import synth
from helpers import K_CAM, det_fields, nms_chain_oracle

pytestmark = pytest.mark.gpu

# every kernel path of the matcher, as in test_gpu_parity.py: (refinement, coarse pass[, bit planes written by the front end itself])
PATHS = [("bits", "bits"), ("bits", "bytes"), ("tiles", "bytes"), ("single", "bytes"), ("bits", "bits", False)]
TABLES = [(n, rt.NAMED[n]) for n in ("levelup", "levelup2", "linemod", "drop1", "drop1_keep3")]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def expected_paths(paths, r, levels):
    """What getPaths() must report: a table with more than two distinct non-zero values does not fit the two bit planes and runs on the
    byte kernels (tiles where the geometry allows them: two levels); the others run where setPaths put them."""
    refine, coarse = paths[:2]
    if refine == "bits" and rt.distinct_nonzero(r) > 2:
        refine, coarse = "tiles", "bytes"
    if refine == "tiles" and levels != 2:
        refine = "single"
    return (refine, coarse)


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("class_index", "cls"), ("template_id", "tid")):
        assert np.array_equal(got[g], want[w]), g


def multiset(rec, names):
    return sorted(zip(*[rec[n].tolist() for n in names]))


def oracle_raw(geom, kinds, r, thr):
    """the oracle's raw records of a request of several banks (class position = index in kinds) and its statistics summed"""
    raws, coarse, evals = [], 0, 0
    for i, kind in enumerate(kinds):
        raw, st = rt.oracle(geom, kind, tuple(r), thr)
        raw = raw.copy()
        raw["cls"] = i
        raws.append(raw)
        coarse += st["coarse_candidates"]; evals += st["local_evals"]
    return np.concatenate(raws), coarse, evals


def check_match(det, sc, geom, kinds, r, thr, paths):
    raw, coarse, evals = oracle_raw(geom, kinds, r, thr)
    assert len(raw) > 0
    got = det.matchArray([sc["rgb"], sc["dep"]], thr, list(kinds))
    assert det.getPaths() == expected_paths(paths, r, len(sc["T"])), (det.getPaths(), paths, r)
    assert det.refinesOnBitPlanes() == (det.getPaths()[0] == "bits")
    same_records(got, lo.canonical_sort_unique(raw))
    tm = det.lastTimings()
    assert tm["coarse_candidates"] == coarse and tm["local_evals"] == evals and tm["matches_pre_unique"] == len(raw)
    pre = det.matchResident(thr, list(kinds), sort_unique=False)
    assert multiset(pre, ["x", "y", "similarity", "class_index", "template_id"]) == multiset(raw, ["x", "y", "sim", "cls", "tid"])


# ---- the bit planes in numpy: two bits per cell, "the response is a" / "the response is 4" (a = the table's second non-zero value) ----------
def low_value(r):
    vals = sorted(set(v for v in r if v and v != 4))
    assert len(vals) <= 1
    return vals[0] if vals else 255                          # no second value: the low plane is empty


def strip_records(lm_flat, T, Wd, Hd, a):
    NS = (Wd + 15) // 16
    planes = lm_flat[:8 * T * T * Wd * Hd].reshape(8, T * T, Hd, Wd)
    pad = np.zeros((8, T * T, Hd, NS * 16 + 32), np.uint8)
    pad[..., :Wd] = planes
    w1 = np.uint64(1) << (2 * np.arange(32, dtype=np.uint64))
    out = np.zeros((8, T * T, NS, Hd), np.uint64)
    for s in range(NS):
        seg = pad[..., 16 * s:16 * s + 32]
        out[:, :, s, :] = ((seg == a).astype(np.uint64) * w1).sum(axis=-1) + ((seg == 4).astype(np.uint64) * (w1 << np.uint64(1))).sum(axis=-1)
    return out


def pair_stream(lm_colour, lm_normal, T, Wd, Hd, npairs, a):
    block = npairs * 16
    flat = np.zeros(2 * block, np.uint8)
    n = 8 * T * T * Wd * Hd
    flat[:n] = lm_colour[:n]; flat[block:block + n] = lm_normal[:n]
    g = flat.reshape(npairs, 32)
    w = np.uint32(1) << np.arange(32, dtype=np.uint32)
    out = np.zeros((npairs, 2), np.uint32)
    out[:, 0] = ((g == a).astype(np.uint32) * w).sum(axis=1); out[:, 1] = ((g == 4).astype(np.uint32) * w).sum(axis=1)
    return out


# ---- 1. response memories ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [2, 10, 6, False], ids=["tiles", "dwords", "ored", "packed"])
@pytest.mark.parametrize("geom", ["G1", "G2"])
def test_response_memories_of_every_writer(lm, geom, direct):
    """readStage(level, 2 / 3) equals the spec's linear memories byte for byte for the five named tables, 4 1 1 0 0 and 4 4 4 4 4, at every
    level and both modalities, with each writer of the bit planes the front end has (pixel tiles, whole dwords, OR-ed ballots, packed from the
    byte planes); where the table fits two planes the strip records and the pair stream equal a numpy packing of the same memories; and the
    default table's bit planes are, after all the switching, the bytes the detector produced before the first setResponseTable."""
    sc = rt.scene(geom)
    W, H, T = sc["W"], sc["H"], sc["T"]
    L = len(T)
    det = lm.Detector(150, T, device=0)
    det.setPaths("bits", "bits", direct)
    det.addClassPacked("planted", *sc["banks"]["planted"])
    det.setFrame([sc["rgb"], sc["dep"]])

    def bit_planes():
        return [det.readStage(l, 4).tobytes() for l in range(L - 1)] + [det.readStage(L - 1, 5).tobytes()]

    assert det.getResponseTable() == rt.DEFAULT
    det.matchResident(70.0, ["planted"])
    assert det.getPaths() == ("bits", "bits")
    before = bit_planes()
    for r in [t for _, t in TABLES] + [(4, 1, 1, 0, 0), (4, 4, 4, 4, 4)] + [rt.DEFAULT]:
        det.setResponseTable(r)
        assert det.getResponseTable() == tuple(r)
        det.matchResident(70.0, ["planted"])
        assert det.getPaths() == expected_paths(("bits", "bits"), r, L), (r, det.getPaths())
        lms, _ = rt.memories(geom, tuple(r))
        if rt.distinct_nonzero(r) <= 2:                       # (read first: building the byte planes on demand does not touch them)
            a = low_value(r)
            for l in range(L - 1):
                Wd, Hd = (W >> l) // T[l], (H >> l) // T[l]
                rec = det.readStage(l, 4).view(np.uint64).reshape(2, 8, T[l] * T[l], (Wd + 15) // 16, Hd)
                for m in range(2):
                    assert np.array_equal(rec[m], strip_records(lms[l][m], T[l], Wd, Hd, a)), (r, "strip records", l, m)
            Wd, Hd = (W >> (L - 1)) // T[-1], (H >> (L - 1)) // T[-1]
            ps = det.readStage(L - 1, 5).view(np.uint32).reshape(-1, 2)
            assert np.array_equal(ps, pair_stream(lms[L - 1][0], lms[L - 1][1], T[-1], Wd, Hd, len(ps), a)), (r, "pair stream")
        for l in range(L):
            n = 8 * (W >> l) * (H >> l)
            for m in range(2):
                assert np.array_equal(det.readStage(l, 2 + m), lms[l][m][:n]), (r, "linear memory", l, m)
    assert bit_planes() == before


# ---- 2. matches on every path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", PATHS, ids=["-".join(map(str, p)) for p in PATHS])
@pytest.mark.parametrize("geom", ["G1", "G2", "G3"])
def test_matches_equal_the_oracle_on_the_tables_memories(lm, geom, paths):
    """For each named table: canonical list, pre-unique multiset, coarse candidates and refinement evaluations equal the oracle's on the
    spec's memories — planted banks (150 and fewer than 64 features: the oracle's 16-bit and 8-bit paths) on one detector, a random bank (some
    of its windows leave their planes: the per-candidate path behind the bit-plane kernel) on another — and getPaths() names the kernels."""
    sc = rt.scene(geom)
    dets = []
    for kinds in (("planted", "small"), ("random",)):
        det = lm.Detector(150, sc["T"], device=0)
        det.setPaths(*paths)
        for k in kinds:
            det.addClassPacked(k, *sc["banks"][k])
        dets.append((det, kinds))
    for name, r in TABLES:
        for det, kinds in dets:
            det.setResponseTable(name)
            check_match(det, sc, geom, kinds, r, rt.THRESHOLDS[kinds[0]][name], paths)


# ---- 3. two-plane tables stay on the two-bit records ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,thr", [("levelup2", 72.0), ((4, 1, 1, 0, 0), 72.0), ((4, 3, 3, 0, 0), 80.0), ((4, 4, 4, 4, 4), 99.0)],
                         ids=["levelup2", "41100", "43300", "44444"])
def test_two_plane_tables_run_on_the_bit_plane_kernels(lm, table, thr):
    """At most two distinct non-zero values (weights 2, 1, 3 of the low plane, and no low plane at all): ("bits", "bits"), exact results, and
    the device memory allocated for the bit planes (bitArenaBytes: the arenas' capacities, not a size derived from the geometry) is what the
    default table needs."""
    geom = "G1"
    sc = rt.scene(geom)
    L = len(sc["T"])
    det = lm.Detector(150, sc["T"], device=0)
    det.setPaths("bits", "bits", 2)
    for k in ("planted", "small"):
        det.addClassPacked(k, *sc["banks"][k])
    det.matchArray([sc["rgb"], sc["dep"]], 70.0, [])
    sizes = [len(det.readStage(l, 4)) for l in range(L - 1)] + [len(det.readStage(L - 1, 5))]
    allocated = det.bitArenaBytes()
    assert allocated[0] >= sum(sizes[:-1]) > 0 and allocated[1] >= sizes[-1] > 0
    det.setResponseTable(table)
    r = rt.NAMED[table] if isinstance(table, str) else table
    check_match(det, sc, geom, ("planted", "small"), r, thr, ("bits", "bits"))
    assert det.getPaths() == ("bits", "bits")
    assert [len(det.readStage(l, 4)) for l in range(L - 1)] + [len(det.readStage(L - 1, 5))] == sizes
    assert det.bitArenaBytes() == allocated
    det.setResponseTable("linemod")                            # ... and a table of the byte kernels allocates nothing for bit planes either
    det.matchArray([sc["rgb"], sc["dep"]], 84.0, [])
    assert det.getPaths() == ("tiles", "bytes") and det.bitArenaBytes() == allocated


# ---- 4. streamed path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linemod", "levelup2"])
def test_streamed_frames_under_a_table(lm, name):
    """submitFrame / collect of three different frames with setBatch(2): the records of the synchronous call per frame and of the oracle."""
    geom = "G1"
    sc = rt.scene(geom)
    W, H, T = sc["W"], sc["H"], sc["T"]
    r, thr = rt.NAMED[name], rt.THRESHOLDS["random"][name]
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
    det = lm.Detector(150, T, device=0)
    det.addClassPacked("random", *sc["banks"]["random"])
    det.setResponseTable(name)
    sync = [det.matchArray(list(f), thr, ["random"]) for f in frames]
    det.setBatch(2)
    for f in frames:
        det.submitFrame(list(f), thr, ["random"])
    for s, w in zip(sync, want):
        got = det.collect()
        same_records(got, w)
        assert got.tobytes() == s.tobytes()
    assert det.getPaths() == expected_paths(("bits", "bits"), r, len(T))


# ---- 5. switching --------------------------------------------------------------------------------------------------------------------------
def test_switching_tables_on_one_detector(lm):
    geom = "G2"
    sc = rt.scene(geom)
    frame = [sc["rgb"], sc["dep"]]

    def fresh():
        det = lm.Detector(150, sc["T"], device=0)
        det.addClassPacked("planted", *sc["banks"]["planted"])
        return det

    det = fresh()
    first = det.matchArray(frame, 70.0, ["planted"])
    assert det.getPaths() == ("bits", "bits")
    det.setResponseTable("linemod")
    assert det.getResponseTable() == (4, 3, 2, 1, 0)
    mid = det.matchResident(84.0, ["planted"])                  # the resident frame: its response memories are rebuilt under the new table
    same_records(mid, lo.canonical_sort_unique(rt.oracle(geom, "planted", rt.NAMED["linemod"], 84.0)[0]))
    assert det.getPaths() == ("tiles", "bytes")
    det.setResponseTable("levelup")
    third = det.matchResident(70.0, ["planted"])
    assert det.getPaths() == ("bits", "bits")
    assert first.tobytes() == third.tobytes() == fresh().matchArray(frame, 70.0, ["planted"]).tobytes()
    same_records(first, lo.canonical_sort_unique(rt.oracle(geom, "planted", rt.DEFAULT, 70.0)[0]))
    assert mid.tobytes() != first.tobytes()
    # refused with a frame in flight, and nothing changes
    det.submit(70.0, ["planted"])
    with pytest.raises(RuntimeError, match="frames in flight: collect them before changing the response table"):
        det.setResponseTable("linemod")
    assert det.getResponseTable() == rt.DEFAULT
    assert det.collect().tobytes() == first.tobytes()
    det.setResponseTable("linemod")                            # ... and accepted once it is collected


@functools.lru_cache(maxsize=None)
def _narrow_scene():
    """104 x 96 at T = 4, 4: 26 and 13 cells per row, whole dwords at neither level (G2 has 48 and 15).  Templates of at most 16 x 17 pixels:
    every window stays inside its planes, so the default paths leave bit planes only at both levels."""
    W, H, T = 104, 96, [4, 4]
    rgb, dep = synth.make_frame(34, W, H, 14)
    pyr = lo.OracleDetector(150, T).quantize_pyramid(rgb, dep)
    bank = synth.make_random_bank(44, 8, W, H, (16, 8))
    assert bank[2].max() <= 32 and bank[0][:, :2].min() >= 0 and W - 32 - 16 * T[0] >= 0 and H - 32 - 16 * T[0] >= 0
    return {"W": W, "H": H, "T": T, "rgb": rgb, "dep": dep, "pyr": pyr, "banks": {"planted": bank}}


@pytest.mark.parametrize("geom,paths,direct", [("G2", ("bits", "bits"), 2), ("G2", ("tiles", "bytes"), 2), ("narrow", ("bits", "bits"), None)],
                         ids=["bits", "bytes", "narrow-bits-default"])
def test_read_stage_between_a_set_and_the_next_match(lm, geom, paths, direct):
    """readStage(level, 2 / 3) answers under the table in force, whether the last front end left byte planes (now stale: rebuilt) or bit
    planes only (built on demand: a linear-memory job of the front end's job table, which takes the table from the launch); the bit planes
    (kinds 4 / 5) stay what the last match read.  G2 rebuilds rows of whole dwords (level 0) and of bytes (level 1); "narrow": rows of bytes
    at both levels, under the detector's default paths."""
    sc = rt.scene(geom) if geom != "narrow" else _narrow_scene()
    W, H, T = sc["W"], sc["H"], sc["T"]
    det = lm.Detector(150, T, device=0)
    if direct is not None:
        det.setPaths(paths[0], paths[1], direct)
    det.addClassPacked("planted", *sc["banks"]["planted"])
    det.matchArray([sc["rgb"], sc["dep"]], 70.0, ["planted"])
    assert det.getPaths() == paths
    bits = [det.readStage(0, 4).tobytes(), det.readStage(1, 5).tobytes()] if paths[0] == "bits" else None
    for name in ("linemod", "levelup2", "levelup"):
        det.setResponseTable(name)
        lms, _ = rt.memories(geom, rt.NAMED[name]) if geom != "narrow" else rt.linear_memories(sc["pyr"], T, rt.NAMED[name])
        for l in range(2):
            for m in range(2):
                assert np.array_equal(det.readStage(l, 2 + m), lms[l][m][:8 * (W >> l) * (H >> l)]), (name, l, m)
        if bits:
            assert [det.readStage(0, 4).tobytes(), det.readStage(1, 5).tobytes()] == bits


def test_legal_and_illegal_tables(lm):
    det = lm.Detector(63, [4, 8], device=0)
    for r in rt.legal_tables():
        det.setResponseTable(r)
        assert det.getResponseTable() == r
    for name, r in rt.NAMED.items():
        det.setResponseTable(name)
        assert det.getResponseTable() == r
    det.setResponseTable("levelup2")
    for bad, msg in (((3, 1, 0, 0, 0), r"r\[0\] must be 4"), ((4, 1, 2, 0, 0), "must not increase"),
                     ((4, 0, 0, 0, 1), "must not increase"), ((4, 1, 0, 0), "five values"),
                     ((4, 1, 0, 0, 0, 0), "five values"), ((4, -1, 0, 0, 0), "integers in 0..4"), ((4, 5, 0, 0, 0), "integers in 0..4"), ((5, 1, 0, 0, 0), "integers in 0..4"),
                     ((4, 1.9, 0, 0, 0), "integers in 0..4"), ((4, True, 0, 0, 0), "integers in 0..4"), ("opencv", "unknown response table")):
        with pytest.raises(RuntimeError, match=msg):
            det.setResponseTable(bad)
        assert det.getResponseTable() == rt.NAMED["levelup2"]  # a refused set changes nothing


# ---- 6. pipeline ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_under_linemod(lm):
    """Pipeline.run takes the table from its detector: match, NMS and top-k fields equal the oracle's chain on the spec's memories."""
    W, H, T, nfeat, thr = 320, 240, [4, 8], (64, 32), 84.0
    rgb, dep = synth.make_frame(3, W, H)
    od = lo.OracleDetector(nfeat[0], T)
    pyr = od.quantize_pyramid(rgb, dep)
    bank = synth.make_planted_bank(41, 80, [(p[0], p[1]) for p in pyr], T, nfeat)
    lms_sizes = rt.linear_memories(pyr, T, rt.NAMED["linemod"])
    det = lm.Detector(nfeat[0], T, device=0)
    det.addClassPacked("obj", *bank)
    det.setResponseTable("linemod")
    pipe = lm.Pipeline(det, W, H, scene_from_scene=True)
    default_chain = nms_chain_oracle(od, rgb, dep, [{"bank": bank}], T, thr, 0.5, 16)
    for iou, k in ((0.5, 16), (0.3, 64)):
        ch = nms_chain_oracle(od, rgb, dep, [{"bank": bank}], T, thr, iou, k, lms_sizes=lms_sizes)
        assert len(ch["sel"]) > 1
        det.setFrame([rgb, dep])
        got, tm = pipe.run(thr, ["obj"], K_CAM, top_k=k, nms_iou=iou)
        assert tm["nms_records"] == ch["m"]
        assert [det_fields(g) for g in got] == ch["sel"]
    assert default_chain["sel"] != nms_chain_oracle(od, rgb, dep, [{"bank": bank}], T, thr, 0.5, 16, lms_sizes=lms_sizes)["sel"]
    pipe.close()
