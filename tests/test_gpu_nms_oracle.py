"""The middle of Pipeline.run — k_nms_pack, k_topk_nms (csrc/nms.hip) and k_icp_bind (csrc/icp_clouds.hip): which matches are kept, in
which order, with which box, and which rendered view each is bound to — against the ORACLE's own chain (helpers.nms_chain_oracle:
match_oracle.c per class -> canonical sort / unique -> boxes -> numpy nms, stable; no product call on the expected side).

Every detection field and the count are compared with ==; the only tolerances are those of the poses in the binding case (the ones
of test_pipeline_equals_match_nms_pose_refine).  Each case first asserts, on the oracle's numbers alone, that it contains what it
claims (enough survivors, a tie, a boundary IoU, several classes ...), then asserts the witness of the path the device took:
timings["nms_records"], the number of distinct records the greedy loop ran over, against the oracle's count of distinct (x, y,
template, class) among the raw matches, and with it the side of the LDS limit (kNmsLds = 8192 records).  A line per run is printed
(`NMS-WITNESS ...`) for the record.  Most cases give the classes no views: every kept detection then has status 5 and no pose, and
the oracle side needs no poseRefine."""
import os

import numpy as np
import pytest

import linemod_oracle as lo
import synth
from helpers import K_CAM, det_fields, nms_chain_oracle

pytestmark = pytest.mark.gpu

NMS_LDS = 8192            # kNmsLds (csrc/nms.hip): up to this many distinct records the greedy loop runs in LDS, above it in HBM
CAND_CAP = 1 << 18        # lm_detector::cand_cap of a fresh detector (csrc/detector_internal.h)


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


# ---- inputs and the comparison ---------------------------------------------------------------------
class Scene:
    """A frame, the oracle's view of it, and planted banks cut from it."""

    def __init__(self, frame_seed, W=640, H=480, T=(4, 8), nfeat=(64, 32)):
        self.W, self.H, self.T, self.nfeat = W, H, list(T), tuple(nfeat)
        self.E = 2 * len(self.T)
        self.rgb, self.dep = synth.make_frame(frame_seed, W, H)
        self.od = lo.OracleDetector(self.nfeat[0], self.T)
        self.pyr = [(p[0], p[1]) for p in self.od.quantize_pyramid(self.rgb, self.dep)]
        self.lms_sizes = self.od.linear_memories(self.rgb, self.dep)

    def bank(self, seed, n, **kw):
        return synth.make_planted_bank(seed, n, self.pyr, self.T, self.nfeat, **kw)

    def chain(self, classes, thr, iou, top_k, raws=None):
        return nms_chain_oracle(self.od, self.rgb, self.dep, classes, self.T, thr, iou, top_k, lms_sizes=self.lms_sizes, raws=raws)

    def detector(self, lm, named_banks):
        det = lm.Detector(self.nfeat[0], self.T, device=0)
        for name, b in named_banks:
            det.addClassPacked(name, *b)
        return det


def take_templates(bank, E, ids):
    """A packed bank made of the pyramids `ids` of another (repeats allowed): the same templates under new ids."""
    feat, offs, wh = bank
    fs, ws, lens = [], [], []
    for t in ids:
        for e in range(t * E, (t + 1) * E):
            fs.append(feat[offs[e]:offs[e + 1]])
            lens.append(offs[e + 1] - offs[e])
            ws.append(wh[e])
    o = np.zeros(len(lens) + 1, np.int32)
    o[1:] = np.cumsum(lens)
    return np.ascontiguousarray(np.concatenate(fs)), o, np.asarray(ws, np.int32).reshape(-1, 2)


def run(sc, det, pipe, thr, ids, top_k, iou):
    det.setFrame([sc.rgb, sc.dep])
    return pipe.run(thr, ids, K_CAM, top_k=top_k, nms_iou=iou)


def check(case, got, tm, ch, path=None):
    """Witness first (the path is the oracle's count's), then count and every field of every detection, exactly."""
    n_cls = len(set(s[3] for s in ch["sel"]))
    print("NMS-WITNESS %s: m=%d (oracle %d) %s kept=%d (oracle %d of %d survivors) tied=%d removed=%d apart_class=%d apart_entry=%d classes_in_topk=%d"
          % (case, tm["nms_records"], ch["m"], "HBM" if tm["nms_records"] > NMS_LDS else "LDS", len(got), len(ch["sel"]), ch["survivors"],
             ch["tied"], ch["removed"], ch["apart_class"], ch["apart_entry"], n_cls))
    assert tm["nms_records"] == ch["m"], case
    if path is not None:
        assert ("HBM" if tm["nms_records"] > NMS_LDS else "LDS") == path, case
    assert len(got) == len(ch["sel"]), case
    for i, (g, s) in enumerate(zip(got, ch["sel"])):
        assert det_fields(g) == s, (case, i)


def no_view_status(got):
    for g in got:
        assert g["status"] == 5 and g["residual"] == -1.0


# ---- LDS path, general -----------------------------------------------------------------------------
IOUS = (0.0, 0.3, 0.5, 0.75, 1.0, 1.5)
TOPKS = (1, 16, 64)


@pytest.mark.parametrize("frame_seed,bank_seed,n,W,H,T,nfeat,thr", [
    (11, 77, 60, 640, 480, (4, 8), (64, 32), 60.0),
    (5, 17, 150, 640, 480, (4, 8), (150, 75), 70.0),
    (23, 31, 90, 640, 480, (4, 4, 8), (64, 32, 16), 50.0),         # three pyramid levels
    (3, 41, 80, 320, 240, (4, 8), (64, 32), 62.0),                 # not VGA
    (11, 77, 60, 640, 480, (4, 8), (64, 32), 88.0),                # a handful of matches: fewer survivors than top_k
], ids=["f11", "f5-nf150", "f23-L3", "f3-qvga", "f11-sparse"])
def test_lds_path_thresholds_and_top_k(lm, frame_seed, bank_seed, n, W, H, T, nfeat, thr):
    """iou in {0, 0.3, 0.5, 0.75, 1, 1.5} x top_k in {1, 16, 64} on one class without views.  Over the grid of a row the oracle must
    keep fewer than top_k somewhere (the loop runs out of records: n_out < top_k) and, except in the sparse row, >= 10 x top_k
    somewhere (the loop stops at top_k with most records still alive)."""
    sc = Scene(frame_seed, W, H, T, nfeat)
    bank = sc.bank(bank_seed, n)
    cls = [{"bank": bank}]
    chains = {}
    raws = None
    for iou in IOUS:
        for k in TOPKS:
            chains[(iou, k)] = sc.chain(cls, thr, iou, k, raws=raws)
            raws = chains[(iou, k)]["raws"]
    m = chains[(0.5, 16)]["m"]
    assert 0 < m <= NMS_LDS
    assert any(c["survivors"] < k for (iou, k), c in chains.items())
    if thr < 80:
        assert any(c["survivors"] >= 10 * k for (iou, k), c in chains.items() if k >= 16)
    # iou >= 1 suppresses nothing but what the unique pass removed: the survivors are the whole list
    assert chains[(1.5, 64)]["survivors"] == len(chains[(1.5, 64)]["unique"])
    det = sc.detector(lm, [("obj", bank)])
    pipe = lm.Pipeline(det, W, H, scene_from_scene=True)
    for (iou, k), ch in chains.items():
        got, tm = run(sc, det, pipe, thr, ["obj"], k, iou)
        check("lds f%d iou=%.2f top_k=%d" % (frame_seed, iou, k), got, tm, ch, "LDS")
        no_view_status(got)
        assert len(got) == min(k, ch["survivors"])
    pipe.close()


# ---- HBM path and repeatability --------------------------------------------------------------------
def test_hbm_path_and_its_lds_twin_and_repeatability(lm):
    """A 500-template planted bank at threshold 50: more than 8192 distinct records, so nms_rounds runs over the HBM scratch; the
    same bank at 60 stays in LDS.  Both exact; the kept lists differ (at iou 0, top_k 64); five runs of each return identical bytes (k_nms_pack appends
    the records in whatever order its atomics resolve)."""
    sc = Scene(11)
    bank = sc.bank(77, 500)
    cls = [{"bank": bank}]
    lo_ch = {(iou, k): sc.chain(cls, 50.0, iou, k) for iou, k in ((0.5, 16), (0.0, 64))}
    hi_ch = {(iou, k): sc.chain(cls, 60.0, iou, k) for iou, k in ((0.5, 16), (0.0, 64))}
    assert lo_ch[(0.5, 16)]["m"] > NMS_LDS and 0 < hi_ch[(0.5, 16)]["m"] <= NMS_LDS
    assert lo_ch[(0.5, 16)]["coarse"] < CAND_CAP // 2                    # far from the candidate capacity: no re-run here
    # the first 16 of iou 0.5 are the best-scoring boxes at either threshold; at iou 0 fewer than 64 survive and the records the
    # lower threshold adds are among them: there the two lists differ, and the HBM loop runs out of records (n_out < top_k)
    assert lo_ch[(0.0, 64)]["sel"] != hi_ch[(0.0, 64)]["sel"] and lo_ch[(0.0, 64)]["survivors"] < 64
    assert lo_ch[(0.5, 16)]["removed"] >= 1                              # the predecessor test has work to do in HBM too
    det = sc.detector(lm, [("obj", bank)])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    for thr, chains, path in ((50.0, lo_ch, "HBM"), (60.0, hi_ch, "LDS"), (50.0, lo_ch, "HBM")):
        for (iou, k), ch in chains.items():
            first = None
            for rep in range(5 if k == 16 else 1):
                got, tm = run(sc, det, pipe, thr, ["obj"], k, iou)
                if rep == 0:
                    check("%s twin thr=%.0f iou=%.2f top_k=%d" % (path.lower(), thr, iou, k), got, tm, ch, path)
                    no_view_status(got)
                    first = (repr(got), tm["nms_records"])
                assert (repr(got), tm["nms_records"]) == first, (path, rep)
    pipe.close()


# ---- thresholds on the boundary --------------------------------------------------------------------
def test_threshold_equal_to_an_occurring_iou(lm):
    """thresh = an IoU that occurs between a kept box and a later one (numpy, f64), one ulp below it and one above: `!(ovr <=
    thresh)` with __ddiv_rn against numpy's divide.  Only values for which the oracle's first 64 kept differ between the three
    thresholds are used (the boundary decides something), four of them."""
    sc = Scene(11)
    bank = sc.bank(77, 60)
    cls = [{"bank": bank}]
    base = sc.chain(cls, 60.0, 0.5, 64)
    d, keep = base["dets"], base["keep"]
    area = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
    picked = []
    for k in keep[:12]:
        w = np.maximum(0.0, np.minimum(d[k, 2], d[:, 2]) - np.maximum(d[k, 0], d[:, 0]) + 1)
        h = np.maximum(0.0, np.minimum(d[k, 3], d[:, 3]) - np.maximum(d[k, 1], d[:, 1]) + 1)
        ovr = (w * h) / (area[k] + area - w * h)
        for v in sorted(set(float(x) for x in ovr if 0.2 < x < 0.8)):
            three = [v, float(np.nextafter(v, 0.0)), float(np.nextafter(v, 1.0))]
            chains = [sc.chain(cls, 60.0, t, 64, raws=base["raws"]) for t in three]
            if chains[0]["sel"] != chains[1]["sel"] and len(picked) < 4 and all(abs(v - p[0][0]) > 0.02 for p in picked):
                assert chains[0]["sel"] == chains[2]["sel"]             # IoU == thresh is not suppressed; one ulp up changes nothing
                picked.append((three, chains))
            if len(picked) == 4:
                break
        if len(picked) == 4:
            break
    assert len(picked) == 4
    det = sc.detector(lm, [("obj", bank)])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    for three, chains in picked:
        for t, ch in zip(three, chains):
            got, tm = run(sc, det, pipe, 60.0, ["obj"], 64, t)
            check("boundary iou=%r" % t, got, tm, ch, "LDS")
    pipe.close()


# ---- ties and duplicates ---------------------------------------------------------------------------
def small_view(sc):
    """One small rendered shape for every template of a case whose subject is the box, not the pose (box_wh comes with views)."""
    md = synth.bump(900, 9, 7, W=sc.W, H=sc.H)
    return md, K_CAM.copy(), np.eye(3, dtype=np.float32), np.array([0, 0, 1000], np.float32)


def set_same_views(pipe, name, view, n, box, first=0):
    pipe.set_views(name, [view[0]] * n, [view[1]] * n, [view[2]] * n, [view[3]] * n, first_template=first, box_wh=box)


def test_ties_and_duplicates_within_and_across_classes(lm):
    """Templates repeated under new ids, inside a class (ids 40..59 of `a` are its 0..19 again) and in another class (`b` = 10..29
    of `a`, then ten of its own), the repeats with other boxes than the originals.  Equal (x, y, similarity) then occurs across
    template ids of a class — adjacent in the canonical order: dropped, suppressing nothing; with another entry between: kept — and
    across classes: kept.  The visit order among the many equal similarities is 'the later canonical entry first'."""
    sc = Scene(11)
    base = sc.bank(77, 40)
    a = take_templates(base, sc.E, list(range(40)) + list(range(20)))
    b_own = sc.bank(78, 10)
    b_rep = take_templates(base, sc.E, list(range(10, 30)))
    b = (np.concatenate([b_rep[0], b_own[0]]), np.concatenate([b_rep[1], b_own[1][1:] + b_rep[1][-1]]).astype(np.int32), np.concatenate([b_rep[2], b_own[2]]))
    box_a = [(int(a[2][t * sc.E][0]) + (0 if t < 40 else 9 - t % 4), int(a[2][t * sc.E][1]) + (0 if t < 40 else t % 5 - 6)) for t in range(60)]
    box_b = [(int(b[2][t * sc.E][0]) - 5 + t % 3, int(b[2][t * sc.E][1]) + 4) for t in range(30)]
    cls = [{"bank": a, "box": box_a}, {"bank": b, "box": box_b}]
    det = sc.detector(lm, [("a", a), ("b", b)])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    view = small_view(sc)
    set_same_views(pipe, "a", view, 60, box_a)
    set_same_views(pipe, "b", view, 30, box_b)
    for thr, iou, k in ((70.0, 0.5, 16), (60.0, 0.5, 16), (60.0, 0.3, 8), (80.0, 1.0, 16)):
        ch = sc.chain(cls, thr, iou, k)
        if thr == 60.0:
            assert ch["tied"] >= 100 and ch["removed"] >= 1 and ch["apart_class"] >= 1
        got, tm = run(sc, det, pipe, thr, ["a", "b"], k, iou)
        check("ties thr=%.0f iou=%.2f top_k=%d" % (thr, iou, k), got, tm, ch, "LDS")
    ch = sc.chain(cls, 60.0, 0.5, 16)
    assert len(set(s[3] for s in ch["sel"])) == 2 and any(s[4] >= 40 for s in ch["sel"] if s[3] == 0)     # both classes and a repeat are among the kept
    pipe.close()


# ---- box extremes ----------------------------------------------------------------------------------
def test_box_extremes(lm):
    """box_wh of (0, 0) (a box of one pixel), negative (the template's own size), larger than the frame, mixed within one class, and
    given for a part of the class only (the rest: own size).  Detection fields only — the views are one small shape."""
    sc = Scene(5)
    bank = sc.bank(17, 60)
    own = lambda t: (int(bank[2][t * sc.E][0]), int(bank[2][t * sc.E][1]))
    mixed = [[(0, 0), (-1, -1), (3000, 2000), (own(t)[0] + 3, own(t)[1] - 2), (-7, -3)][t % 5] for t in range(60)]
    part = {t: (own(t)[0] // 2, own(t)[1] * 2) for t in range(20, 45)}
    view = small_view(sc)
    for name, box, first, n in (("mixed", mixed, 0, 60), ("part", part, 20, 25)):
        det = sc.detector(lm, [("obj", bank)])
        pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
        set_same_views(pipe, "obj", view, n, [box[t] for t in range(first, first + n)], first=first)
        cls = [{"bank": bank, "box": box}]
        for thr, iou, k in ((65.0, 0.5, 16), (65.0, 0.05, 16), (75.0, 0.0, 16)):
            ch = sc.chain(cls, thr, iou, k)
            if name == "mixed" and iou == 0.5:
                ws = [s[5] for s in ch["sel"]]
                assert 0 in ws and 3000 in ws and any(s[4] % 5 in (1, 4) and (s[5], s[6]) == own(s[4]) for s in ch["sel"])
            if name == "part" and iou == 0.5:
                assert any(s[4] in part for s in ch["sel"]) and any(s[4] not in part for s in ch["sel"])
            got, tm = run(sc, det, pipe, thr, ["obj"], k, iou)
            check("box %s thr=%.0f iou=%.2f" % (name, thr, iou), got, tm, ch, "LDS")
            for g in got:
                assert (g["status"] == 5) == (not (first <= g["template_id"] < first + n))
        pipe.close()


# ---- no matches ------------------------------------------------------------------------------------
def test_no_match_at_all(lm):
    sc = Scene(11)
    bank = sc.bank(77, 60)
    ch = sc.chain([{"bank": bank}], 100.0, 0.5, 16)
    assert ch["m"] == 0 and ch["sel"] == []
    det = sc.detector(lm, [("obj", bank)])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    for k in (1, 16):
        got, tm = run(sc, det, pipe, 100.0, ["obj"], k, 0.5)
        check("no match top_k=%d" % k, got, tm, ch, "LDS")
        assert got == [] and tm["nms_records"] == 0
    ch = sc.chain([{"bank": bank}], 70.0, 0.5, 16)                           # and the pipeline goes on
    got, tm = run(sc, det, pipe, 70.0, ["obj"], 16, 0.5)
    check("after no match", got, tm, ch, "LDS")
    pipe.close()


# ---- several classes and the view binding ----------------------------------------------------------
POSE_CACHE = {}


def test_several_classes_orders_and_view_binding(lm):
    """Three classes of 40, 25 and 30 templates, added as zeta, alpha, mid (so the sorted order an empty request uses differs from
    the order added).  zeta has views and boxes for all templates, alpha from template 10 on, mid none.  One pipeline serves, in
    sequence: the full list before any view exists, the same list after the views were set (the cached class_base changes under an
    unchanged list), another order, a subset, the empty list, and the first list again.  class_index, template_id and box per
    detection against the oracle; status 5 exactly where the view table has no view, else the oracle's poseRefine against THAT class's
    rendering (status 1 where the oracle's window leaves the frame).  The classes' shapes and view poses differ by far more than the
    tolerance — asserted on the oracle side by refining one detection against the other class's view."""
    sc = Scene(11)
    banks = {"zeta": sc.bank(77, 40), "alpha": sc.bank(78, 25), "mid": sc.bank(79, 30)}
    rng = np.random.default_rng(9)
    shapes = {"zeta": [synth.bump(500 + k, 34, 20, z0=950.0) for k in range(2)], "alpha": [synth.bump(510 + k, 18, 30, z0=1180.0, amp=35.0) for k in range(2)]}
    views = {"zeta": {}, "alpha": {}, "mid": {}}
    for name, lo_t, n in (("zeta", 0, 40), ("alpha", 10, 25)):
        for t in range(lo_t, n):
            tt = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), (950 if name == "zeta" else 1180) + rng.uniform(-20, 20)], np.float32)
            views[name][t] = (shapes[name][t % 2], K_CAM.copy(), np.eye(3, dtype=np.float32), tt)
    own = lambda name, t: (int(banks[name][2][t * sc.E][0]), int(banks[name][2][t * sc.E][1]))
    boxes = {"zeta": {t: (own("zeta", t)[0] + 6 - t % 4, own("zeta", t)[1] - 3 + t % 3) for t in range(40)},
             "alpha": {t: (own("alpha", t)[0] - 4, own("alpha", t)[1] + 5) for t in range(10, 25)}, "mid": None}
    det = sc.detector(lm, [(n, banks[n]) for n in ("zeta", "alpha", "mid")])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    thr, k, iou = 70.0, 16, 0.5
    full = ["zeta", "alpha", "mid"]

    def one(tag, ids, with_views):
        order = ids if ids else sorted(banks)                           # an empty request: every class, in sorted order
        cls = [{"bank": banks[n], "box": boxes[n] if with_views else None} for n in order]
        ch = sc.chain(cls, thr, iou, k)
        assert len(set(s[3] for s in ch["sel"])) >= 2, tag              # the top-K holds detections of at least two classes
        want_status = []
        for s in ch["sel"]:
            name, t = order[s[3]], s[4]
            if not with_views or t not in views[name]:
                want_status.append((5, None))
                continue
            key = (name, t, s[0], s[1])
            if key not in POSE_CACHE:
                md, K, R, tt = views[name][t]
                POSE_CACHE[key] = lo.pose_refine(sc.dep, md, K_CAM, K, R, tt, s[0], s[1], scene_from_scene=True)
            p = POSE_CACHE[key]
            want_status.append((1 if p["residual"] == -1.0 else 0, p))
        if with_views:
            assert any(w[0] == 0 for w in want_status) and any(w[0] == 5 for w in want_status), tag
        got, tm = run(sc, det, pipe, thr, ids, k, iou)
        check("classes %s" % tag, got, tm, ch, "LDS")
        for g, (st, p) in zip(got, want_status):
            assert g["status"] == st, (tag, g, st)
            if st == 0:
                assert abs(g["residual"] - p["residual"]) < 1e-6
                assert np.allclose(g["R"], p["R"], atol=1e-4) and np.allclose(np.ravel(g["t"]) / 1000.0, np.ravel(p["t"]) / 1000.0, atol=1e-4)
        return ch, want_status

    one("before views", full, False)
    pipe.set_views("zeta", *[[views["zeta"][t][q] for t in range(40)] for q in range(4)], box_wh=[boxes["zeta"][t] for t in range(40)])
    pipe.set_views("alpha", *[[views["alpha"][t][q] for t in range(10, 25)] for q in range(4)], first_template=10, box_wh=[boxes["alpha"][t] for t in range(10, 25)])
    ch, ws = one("order added", full, True)
    # a view of the other class at the same detection is a different pose by far more than the tolerance
    i = next(i for i, (st, p) in enumerate(ws) if st == 0)
    s = ch["sel"][i]
    other = "alpha" if full[s[3]] == "zeta" else "zeta"
    md, K, R, tt = views[other][max(10, min(s[4], 24))]
    wrong = lo.pose_refine(sc.dep, md, K_CAM, K, R, tt, s[0], s[1], scene_from_scene=True)
    assert wrong["residual"] == -1.0 or not np.allclose(np.ravel(wrong["t"]) / 1000.0, np.ravel(ws[i][1]["t"]) / 1000.0, atol=1e-2)
    one("another order", ["mid", "zeta", "alpha"], True)
    one("subset", ["alpha", "mid"], True)
    one("empty list = sorted", [], True)
    one("order added again", full, True)
    # what Detector.match reports as class_index for the empty request is the same position
    det.setFrame([sc.rgb, sc.dep])
    ms = det.matchResident(thr, [])
    ch = sc.chain([{"bank": banks[n]} for n in sorted(banks)], thr, iou, k)
    assert [(int(r["x"]), int(r["y"]), int(r["class_index"]), int(r["template_id"])) for r in ms] == \
           [(int(r["x"]), int(r["y"]), int(r["cls"]), int(r["tid"])) for r in ch["unique"]]
    pipe.close()


# ---- class position at the packing limit -----------------------------------------------------------
def test_class_position_128_is_the_limit(lm):
    """128 classes (one small bank under 128 names): positions 0..127 fit the packed record, the results are exact and hold a
    detection of class 127 (among equal entries the later canonical one is visited first).  A 129th class that matches is refused with
    LM_ERR_INVALID and the documented message — an argument check, nothing is written out of range — and the pipeline stays usable."""
    sc = Scene(3, 320, 240)
    bank = sc.bank(41, 6)
    names = ["c%03d" % i for i in range(129)]
    thr, k, iou = 72.0, 16, 0.5
    one = sc.chain([{"bank": bank}], thr, iou, k)
    assert one["m"] > 0
    cls = [{"bank": bank}] * 128
    ch = sc.chain(cls, thr, iou, k, raws=one["raws"] * 128)
    assert ch["m"] == 128 * one["m"] and any(s[3] == 127 for s in ch["sel"]) and ch["apart_class"] >= 128
    det = sc.detector(lm, [(n, bank) for n in names[:128]])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    got, tm = run(sc, det, pipe, thr, names[:128], k, iou)
    check("128 classes", got, tm, ch, "LDS")
    ch1 = sc.chain(cls, thr, 1.0, 64, raws=one["raws"] * 128)              # nothing suppressed: the visit order over all classes
    got, tm = run(sc, det, pipe, thr, names[:128], 64, 1.0)
    check("128 classes iou=1", got, tm, ch1, "LDS")
    det.addClassPacked(names[128], *bank)
    with pytest.raises(RuntimeError, match="a match field exceeds the packed record"):
        run(sc, det, pipe, thr, names, k, iou)
    with pytest.raises(RuntimeError, match="a match field exceeds the packed record"):
        run(sc, det, pipe, thr, [], k, iou)                                 # the empty request is all 129 too
    got, tm = run(sc, det, pipe, thr, names[:128], k, iou)
    check("128 classes after the refusal", got, tm, ch, "LDS")
    ch2 = sc.chain([{"bank": bank}] * 2, thr, iou, k, raws=one["raws"] * 2)
    got, tm = run(sc, det, pipe, thr, [names[128], names[5]], k, iou)        # the 129th class itself is fine at a position below 128
    check("two of the 129", got, tm, ch2, "LDS")
    pipe.close()


# ---- the re-run after a candidate-buffer overflow ---------------------------------------------------
def test_rerun_after_candidate_overflow(lm):
    """A fresh detector holds 2^18 candidates; 1500 planted templates at threshold 50 give more coarse candidates than that, so the
    first pass of lm_pipeline_run overflows, the buffers grow and the frame runs again — hash table and counters preset anew.  The
    result is the oracle's, and a second run (which does not overflow any more) returns the same bytes."""
    sc = Scene(11)
    bank = sc.bank(77, 1500)
    ch = sc.chain([{"bank": bank}], 50.0, 0.5, 16)
    assert ch["coarse"] > CAND_CAP and ch["m"] > NMS_LDS
    det = sc.detector(lm, [("obj", bank)])
    pipe = lm.Pipeline(det, sc.W, sc.H, scene_from_scene=True)
    got, tm = run(sc, det, pipe, 50.0, ["obj"], 16, 0.5)
    assert tm["coarse_candidates"] == ch["coarse"]
    check("overflow first run", got, tm, ch, "HBM")
    got2, tm2 = run(sc, det, pipe, 50.0, ["obj"], 16, 0.5)
    check("overflow second run", got2, tm2, ch, "HBM")
    assert repr(got2) == repr(got)
    pipe.close()
