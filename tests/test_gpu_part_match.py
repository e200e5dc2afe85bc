"""GPU tests (`-m gpu`) of part-based matching (Detector.setPartMatching; k_coarse_parts / k_local_parts, match_parts.hip) against
part_match_ref.py, record for record.  test_part_match_ref.py pins that reference and proves, on the CPU, the conditions on the inputs used here.

The scenes are those of response_table_ref (G1, G2, G3).  Part matching refuses a bank whose refinement windows can leave their planes; the
scenes' banks hold such templates on G2 (random) and G3 (both), so the parity cases run on the templates of each bank that the detector accepts
(test_part_match_ref.fitting_bank: all 40 on G1, at least 10 elsewhere) and the refusal test runs on the banks as they are."""
import functools
import os

import numpy as np
import pytest

import linemod_oracle as lo
import part_match_cases as pc
import part_match_ref as pm
import response_table_ref as rt
import synth
import test_part_match_ref as cpu

pytestmark = pytest.mark.gpu
FIELDS = ["x", "y", "similarity", "template_id"]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def got_multiset(rec):
    return sorted(zip(*[rec[n].tolist() for n in FIELDS]))


def detector(lm, nfeat, T, banks):
    det = lm.Detector(nfeat, list(T), device=0)
    for name, bank in banks.items():
        det.addClassPacked(name, *bank)
    return det


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("geom", ["G1", "G2", "G3"])
def test_records_equal_the_reference(lm, geom, kind):
    """min_parts 1..4 x min_part_features 1, 8 and a value that makes parts ineligible: the pre-unique records are the reference's multiset, the
    canonical list its sorted unique, and with part matching off again the oracle's holistic records."""
    sc = rt.scene(geom)
    bank, keep = cpu.fitting_bank(geom, kind)
    thr = cpu.THRESHOLDS[kind]
    det = detector(lm, 150, sc["T"], {kind: bank})
    det.setFrame([sc["rgb"], sc["dep"]])
    for mpf in cpu.min_part_features(geom):
        for mp in (1, 2, 3, 4):
            det.setPartMatching(mp, mpf)
            assert det.partMatching() == (mp, mpf)
            want = cpu.reference(geom, kind, mp, mpf)
            pre = det.matchResident(thr, [kind], sort_unique=False)
            assert got_multiset(pre) == pm.multiset(want), (mp, mpf)
            fin = det.matchResident(thr, [kind])
            w = lo.canonical_sort_unique(want)
            assert len(fin) == len(w) and all(np.array_equal(fin[a], w[b]) for a, b in zip(FIELDS, ["x", "y", "sim", "tid"])), (mp, mpf)
    det.setPartMatching(0)
    lms, sizes = rt.memories(geom, rt.DEFAULT)
    raw, _ = lo.match_bank_c(lo.PackedBank(len(keep), len(sc["T"]), *bank), lms, sizes, sc["T"], thr)
    assert got_multiset(det.matchResident(thr, [kind], sort_unique=False)) == rt.multiset(raw)


# ---- 2. occlusion ---------------------------------------------------------------------------------------------------------------------------
OCCLUSION_THRESHOLD = 80.0


@functools.lru_cache(maxsize=None)
def occluded_cases():
    """For ten planted templates of G1 (the frame is too small for ten windows that do not overlap: a frame per template; the ten are the first
    of the bank's 40 for which the reference finds the plant again within 2 px, i.e. in the same level-0 cell — chosen on the reference alone):
    the frame with the right half of the template's box at its plant set to a constant colour and depth 0, the template as a bank of its own,
    the holistic oracle's and the part reference's records there.  plant = the template's best record on the frame as it was."""
    sc = rt.scene("G1")
    T = sc["T"]
    clean, _ = rt.oracle("G1", "planted", rt.DEFAULT, 70.0)
    cases = []
    for p in range(40):
        if len(cases) == 10:
            break
        bank = cpu.sub_bank(sc["banks"]["planted"], 2, [p])
        c = clean[clean["tid"] == p]
        plant = c[np.argmax(c["sim"])]
        x0, y0, (w, h) = int(plant["x"]), int(plant["y"]), bank[2][0]
        rgb, dep = sc["rgb"].copy(), sc["dep"].copy()
        rgb[y0:y0 + h + 1, x0 + (w + 1) // 2:x0 + w + 1] = (90, 90, 90)
        dep[y0:y0 + h + 1, x0 + (w + 1) // 2:x0 + w + 1] = 0
        lms, sizes = rt.linear_memories(sc["od"].quantize_pyramid(rgb, dep), T, rt.DEFAULT)
        hol, _ = lo.match_bank_c(lo.PackedBank(1, 2, *bank), lms, sizes, T, OCCLUSION_THRESHOLD)
        want = pm.match_parts(bank, lms, sizes, T, OCCLUSION_THRESHOLD, 2, 8)
        near = lambda r: bool(((np.abs(r["x"] - x0) <= 2) & (np.abs(r["y"] - y0) <= 2)).any())
        if near(want) and not near(hol):
            cases.append({"bank": bank, "rgb": rgb, "dep": dep, "hol": hol, "want": want, "hol_near": near(hol), "want_near": near(want)})
    return cases


def test_half_occluded_plants_are_found_by_two_parts(lm):
    cases = occluded_cases()
    print("holistic / part records near the plant:", [(c["hol_near"], c["want_near"]) for c in cases])
    assert len(cases) == 10 and not any(c["hol_near"] for c in cases) and all(c["want_near"] for c in cases)          # the conditions on the inputs
    sc = rt.scene("G1")
    det = detector(lm, 150, sc["T"], {"t%d" % i: c["bank"] for i, c in enumerate(cases)})
    for i, c in enumerate(cases):
        det.setFrame([c["rgb"], c["dep"]])
        det.setPartMatching(2)
        assert got_multiset(det.matchResident(OCCLUSION_THRESHOLD, ["t%d" % i], sort_unique=False)) == pm.multiset(c["want"])
        det.setPartMatching(0)
        assert got_multiset(det.matchResident(OCCLUSION_THRESHOLD, ["t%d" % i], sort_unique=False)) == rt.multiset(c["hol"])


# ---- 3. the golden half-occluded frame --------------------------------------------------------------------------------------------------------
def test_the_golden_half_occluded_frame(lm):
    case, bank, lms, sizes = cpu.golden_half()
    want = pm.match_parts(bank, lms, sizes, [5, 8], 75.0, 2, 8)
    det = lm.Detector(127, [5, 8], device=0)
    det.readClasses(["06_template"], os.path.join(cpu.GOLDEN, "bank127_%s.yaml.gz"))
    det.setFrame([case["rgb"], case["dep"]])
    assert len(det.matchResident(75.0, ["06_template"], sort_unique=False)) == 0
    det.setPartMatching(2)
    pre = det.matchResident(75.0, ["06_template"], sort_unique=False)
    assert len(pre) == cpu.GOLDEN_HALF_PARTS2 and got_multiset(pre) == pm.multiset(want)


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------------
edge_bank = pc.edge_bank              # (the bank of this section lives in part_match_cases.py, which test_gpu_part_match_edges.py shares)


@pytest.mark.parametrize("levels", [2, 1])
def test_edges(lm, levels):
    sc = rt.scene("G1")
    T = [4, 8][:levels] if levels == 2 else [8]
    bank = edge_bank(levels)
    pyr = lo.OracleDetector(150, T).quantize_pyramid(sc["rgb"], sc["dep"])
    lms, sizes = rt.linear_memories(pyr, T, rt.DEFAULT)
    Wd, Hd = sizes[-1][0] // T[-1], sizes[-1][1] // T[-1]
    F, w, h = pm.entry_of(bank, 4, levels - 1, levels)
    assert (Hd - ((h - 1) // T[-1] + 1)) * Wd + (Wd - ((w - 1) // T[-1] + 1)) + 1 < Wd * Hd         # positions without sums
    assert max(len(pm.entry_of(bank, 3, l, levels)[0]) for l in range(levels)) > 511
    det = detector(lm, 150, T, {"edges": bank})
    det.setFrame([sc["rgb"], sc["dep"]])
    some = 0
    for mp, mpf, thr in ((1, 1, 30.0), (2, 8, 25.0), (1, 9, 30.0), (4, 1, 10.0), (2, 8, 0.0)):
        want = pm.match_parts(bank, lms, sizes, T, thr, mp, mpf)
        det.setPartMatching(mp, mpf)
        assert got_multiset(det.matchResident(thr, ["edges"], sort_unique=False)) == pm.multiset(want), (mp, mpf, thr)
        some += len(want)
    assert some > 0


# ---- 5. machinery -----------------------------------------------------------------------------------------------------------------------------
def test_stream_resident_rerun_and_switching_off(lm):
    sc = rt.scene("G1")
    bank, thr = sc["banks"]["planted"], 70.0
    frames = [(sc["rgb"], sc["dep"])] + [synth.make_frame(950 + i, sc["W"], sc["H"], 14) for i in range(7)]
    det = detector(lm, 150, sc["T"], {"planted": bank})
    before = det.matchArray(list(frames[0]), thr, ["planted"])
    det.setPartMatching(2)
    sync = [det.matchArray(list(f), thr, ["planted"]) for f in frames]
    assert got_multiset(_pre(det, frames[0], thr)) == pm.multiset(cpu.reference("G1", "planted", 2, 8))
    det.setFrame(list(frames[0]))
    assert det.matchResident(thr, ["planted"]).tobytes() == sync[0].tobytes() == det.matchResident(thr, ["planted"]).tobytes()   # resident, and a second run
    det.setBatch(8)
    streamed = list(det.matchStream([list(f) for f in frames], thr, ["planted"]))
    assert len(streamed) == 8 and all(s.tobytes() == m.tobytes() for s, m in zip(streamed, sync))
    assert sum(len(s) for s in sync) > 0 and sync[0].tobytes() != before.tobytes()
    small = detector(lm, 150, sc["T"], {"planted": bank})      # a capacity below the frame's candidates: one grow-and-rerun
    small.setCandidateCapacity(1024)
    small.setPartMatching(1)
    big = detector(lm, 150, sc["T"], {"planted": bank})
    big.setPartMatching(1)
    a, b = small.matchArray(list(frames[0]), 40.0, ["planted"]), big.matchArray(list(frames[0]), 40.0, ["planted"])
    assert big.lastTimings()["coarse_candidates"] > 1024 and a.tobytes() == b.tobytes()
    det.setPartMatching(0)
    assert det.partMatching()[0] == 0 and det.matchArray(list(frames[0]), thr, ["planted"]).tobytes() == before.tobytes()


def _pre(det, frame, thr):
    det.setFrame(list(frame))
    return det.matchResident(thr, ["planted"], sort_unique=False)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(lm):
    sc = rt.scene("G1")
    frame = [sc["rgb"], sc["dep"]]
    det = detector(lm, 150, sc["T"], {"planted": sc["banks"]["planted"]})
    for bad, msg in (((5, 8), "min_parts must be 0"), ((-1, 8), "min_parts must be 0"), ((2, 0), "min_part_features must be at least 1")):
        with pytest.raises(RuntimeError, match=msg):
            det.setPartMatching(*bad)
    assert det.partMatching() == (0, 8)
    det.setPartMatching(2)
    with pytest.raises(RuntimeError, match="threshold >= 0"):
        det.matchArray(frame, -1.0, ["planted"])
    for paths in (("bits", "bytes"), ("tiles", "bytes"), ("single", "bytes"), ("wide", "wide")):
        det.setPaths(*paths)
        with pytest.raises(RuntimeError, match="bit-plane kernels only"):
            det.matchArray(frame, 70.0, ["planted"])
    det.setPaths("bits", "bits")
    det.setResponseTable("linemod")
    with pytest.raises(RuntimeError, match="at most two distinct non-zero values"):
        det.matchArray(frame, 84.0, ["planted"])
    det.setResponseTable("levelup")
    with pytest.raises(RuntimeError, match="sharded detector"):
        det.setShard(0, 2)
    det.setFrame(frame)
    with pytest.raises(RuntimeError, match="not available under part matching"):
        det.matchSlabsResident(70.0, ["planted"])
    with pytest.raises(RuntimeError, match="not available under part matching"):
        lm.Pipeline(det, sc["W"], sc["H"], scene_from_scene=True)
    det.submit(70.0, ["planted"])
    assert det._lib.lm_detector_exchange_pack(det._h, None, 4096) != 0
    assert "the multi-GPU exchange is not available under part matching" in det._lib.lm_last_error().decode()
    with pytest.raises(RuntimeError, match="frames in flight"):
        det.setPartMatching(0)
    det.collect()
    assert len(det.matchArray(frame, 70.0, ["planted"])) > 0                        # ... and it still matches
    sharded = detector(lm, 150, sc["T"], {"planted": sc["banks"]["planted"]})
    sharded.setShard(0, 2)
    with pytest.raises(RuntimeError, match="sharded detector"):
        sharded.setPartMatching(2)
    g3 = rt.scene("G3")                                                             # G3's banks hold templates whose windows leave their planes
    outside = detector(lm, 150, g3["T"], {"planted": g3["banks"]["planted"]})
    outside.setPartMatching(2)
    with pytest.raises(RuntimeError, match="every refinement window inside its planes"):
        outside.matchArray([g3["rgb"], g3["dep"]], 70.0, ["planted"])
    outside.setPartMatching(0)
    assert len(outside.matchArray([g3["rgb"], g3["dep"]], 70.0, ["planted"])) > 0
