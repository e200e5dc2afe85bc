"""The edge-case inputs of depth-scaled matching shared by test_scaled_edge_cases.py (which proves the conditions on them, on the CPU, on the
reference alone) and test_gpu_scaled_edges.py (which holds the kernels to the reference on them).  scaled_cases.py keeps to one corner: one
class, one training depth, equal feature counts, boxes away from the right and bottom edges, thresholds of 25 and more.  Here: several classes
with their own training depths and feature counts, K-row tables above 64 KB, entries without features, boxes at and beyond the edges of a level,
thresholds at and below zero, and a geometry whose probe tiles are partial in both axes.  All frames are 320 x 240 or smaller but for the
328 x 200 one; every bank is a few pyramids.

A case is a dict: frame (frame()), classes (name -> packed bank, in the order they are ADDED to a detector, which is not the order of the
names), d_train (name -> mm), selection, threshold, scales (floats), lo_hi, probe, expect ("records", "empty" or "refused")."""
import functools

import numpy as np

import linemod_oracle as lo
import response_table_ref as rt
import scaled_cases as sc
import scaled_match_ref as sm
import synth

W, H = 320, 240
T2 = (4, 8)
TRAIN = {"a": 700, "b": 1000, "c": 1400, "d": 850}
SELECTIONS = {"all": (), "c_a": ("c", "a"), "c_nope_a": ("c", "nope", "a"), "a_a": ("a", "a")}
CLASS_THRESHOLD = 62.0


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame(seed=53, size=(W, H), T=T2, crop=None, mask_left=False):
    """frame, quantised maps and byte linear memories (default table).  crop = (w, h): the top left corner of the frame of `size`.
    mask_left: the quantised maps of the left half are empty, as under masks that hide it, while the depth image stays measured (the CPU's
    stand-in for setFrame(sources, masks): the GPU test takes the detector's own memories)."""
    rgb, dep = synth.make_frame(seed, size[0], size[1], 14)
    if crop is not None:
        rgb, dep = np.ascontiguousarray(rgb[:crop[1], :crop[0]]), np.ascontiguousarray(dep[:crop[1], :crop[0]])
    od = lo.OracleDetector(150, list(T))
    qp = [(p[0].copy(), p[1].copy()) for p in od.quantize_pyramid(rgb, dep)]
    if mask_left:
        for qc, qn in qp:
            qc[:, :qc.shape[1] // 2] = 0
            qn[:, :qn.shape[1] // 2] = 0
    lms, sizes = rt.linear_memories(qp, list(T), rt.DEFAULT)
    h0, w0 = dep.shape
    masks = ()
    if mask_left:
        m = np.full((h0, w0), 255, np.uint8)
        m[:, :w0 // 2] = 0
        masks = (m, m)
    return {"T": list(T), "rgb": rgb, "dep": dep, "qp": qp, "lms": lms, "sizes": sizes, "size": (w0, h0), "masks": masks}


# ---- banks (features (F, 3), offsets, (width, height) per entry; entry = (pyramid * levels + level) * 2 + modality) ---------------------------------
def windows(seed, n, size=(W, H), T0=4, lo_px=32, hi_px=65):
    rng = np.random.default_rng(seed)
    border = 8 * T0 + 2
    out = []
    for _ in range(n):
        w, h = int(rng.integers(lo_px, hi_px)), int(rng.integers(lo_px, hi_px))
        out.append((int(rng.integers(border, size[0] - w - border - 16)), int(rng.integers(border, size[1] - h - border - 16)), w, h))
    return out


def planted(fr, seed, nfeat, wins):
    return synth.make_planted_bank(seed, len(wins), fr["qp"], fr["T"], nfeat, windows=wins)


def entries(bank):
    feat, offs, wh = bank
    return [feat[offs[e]:offs[e + 1]] for e in range(len(offs) - 1)], [tuple(int(v) for v in w) for w in wh]


def concat(*banks):
    fs, ws = [], []
    for b in banks:
        f, w = entries(b)
        fs += f
        ws += w
    return synth._finish(fs, ws)


def pyramids(bank, L, which):
    f, w = entries(bank)
    fs, ws = [], []
    for p in which:
        fs += f[p * 2 * L:(p + 1) * 2 * L]
        ws += w[p * 2 * L:(p + 1) * 2 * L]
    return synth._finish(fs, ws)


def strip(bank, L, pyramid, level):
    """the bank with both modalities of one entry emptied (its box stays)"""
    f, w = entries(bank)
    for m in range(2):
        f[(pyramid * L + level) * 2 + m] = np.zeros((0, 3), np.int32)
    return synth._finish(f, w)


def hand(seed, box, counts):
    """one pyramid of box (w, h) at level 0 whose features are drawn at random inside the box of each level (coinciding features allowed);
    counts[level] = (colour, normals)"""
    rng = np.random.default_rng(seed)
    fs, ws = [], []
    for l, cn in enumerate(counts):
        wl, hl = box[0] >> l, box[1] >> l
        for n in cn:
            fs.append(np.stack([rng.integers(0, wl + 1, n), rng.integers(0, hl + 1, n), rng.integers(0, 8, n)], 1).astype(np.int32).reshape(-1, 3))
            ws.append((wl, hl))
    return synth._finish(fs, ws)


def top_nf(bank, L):
    f, _ = entries(bank)
    return [len(f[(p * L + L - 1) * 2]) + len(f[(p * L + L - 1) * 2 + 1]) for p in range(len(f) // (2 * L))]


# ---- the reference on a case ------------------------------------------------------------------------------------------------------------------------
def reference(case, lms=None, sizes=None, stats=None, **over):
    """raw records of the reference on a case; lms / sizes: other memories than the frame's (the detector's own); over: fields replaced"""
    c = dict(case, **over)
    fr = c["frame"]
    lo_, hi_ = c.get("lo_hi", (None, None))
    return sm.match_classes(c["classes"], c["d_train"], c["selection"], fr["lms"] if lms is None else lms, fr["sizes"] if sizes is None else sizes,
                            fr["T"], c["threshold"], fr["dep"], sc.ladder_q10(c["scales"]), None if lo_ is None else sm.q10(lo_),
                            None if hi_ is None else sm.q10(hi_), c.get("probe", 2), stats=stats)


def make(fr, classes, threshold, selection=(), scales=sc.LADDERS[9], lo_hi=(None, None), probe=2, expect="records", d_train=None):
    return {"frame": fr, "classes": classes, "d_train": dict(TRAIN) if d_train is None else d_train, "selection": tuple(selection),
            "threshold": threshold, "scales": tuple(scales), "lo_hi": lo_hi, "probe": probe, "expect": expect}


def first_threshold_with_records(case, candidates=(70.0, 60.0, 50.0, 40.0, 30.0, 25.0, 20.0, 15.0, 10.0, 5.0), per_template=False):
    """the largest of `candidates` at which the reference returns a record (per_template: one of every template of class 0)"""
    for t in candidates:
        rec = reference(case, threshold=t)
        want = sum(len(b[1]) - 1 for b in case["classes"].values()) // (2 * len(case["frame"]["T"])) if per_template else 1
        if len(np.unique(rec[["class_index", "template_id"]])) >= want:
            return t
    raise AssertionError("the reference returns nothing at any threshold tried")


# ---- a. several classes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def class_banks():
    """a: 1 pyramid, b: 5 (two feature layouts inside the class), c: 3, and d (2), the class added later; ADDED in the order c, a, b"""
    fr = frame()
    a = planted(fr, 11, ((30, 20), 24), windows(1, 1))
    b = concat(planted(fr, 12, (60, 30), windows(2, 2)), planted(fr, 13, ((40, 20), (12, 30)), windows(3, 3)))
    c = planted(fr, 14, (36, (10, 8)), windows(4, 3))
    d = planted(fr, 15, (44, 22), windows(5, 2))
    return {"c": c, "a": a, "b": b}, d


@functools.lru_cache(maxsize=None)
def class_case(selection="all"):
    return make(frame(), class_banks()[0], CLASS_THRESHOLD, SELECTIONS[selection])


# ---- b. big tables --------------------------------------------------------------------------------------------------------------------------------
BIG_BOX = (96, 80)


@functools.lru_cache(maxsize=None)
def big_case(name):
    """`mixed`: top-level entries of 600 and 40 features under the 16-scale ladder (76,800 bytes of table for the launch, 5,120 for the small
    one); `limit`: 1280 features, 163,840 bytes, the most the matcher accepts; `over`: 1281 features, refused."""
    fr = frame()
    if name == "mixed":
        bank = concat(hand(21, (64, 48), ((20, 20), (20, 20))), hand(22, BIG_BOX, ((30, 30), (300, 300))))
    elif name == "limit":
        bank = hand(23, BIG_BOX, ((30, 30), (640, 640)))
    else:
        bank = hand(24, BIG_BOX, ((30, 30), (641, 640)))
    c = make(fr, {"big": bank}, 0.0, scales=sc.LADDERS[16], d_train={"big": 1000}, expect="refused" if name == "over" else "records")
    if name != "over":
        c["threshold"] = first_threshold_with_records(c, per_template=True)
    return c


# ---- c. entries without features ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zero_case(threshold=CLASS_THRESHOLD):
    """pyramid 0: no features at the top level; pyramid 1: ordinary; pyramid 2: no features at level 0"""
    fr = frame()
    bank = planted(fr, 31, (60, 30), windows(6, 3))
    bank = strip(strip(bank, 2, 0, 1), 2, 2, 0)
    return make(fr, {"z": bank}, threshold, d_train={"z": 1000})


# ---- d. edges of the level ----------------------------------------------------------------------------------------------------------------------------
EDGE_LADDERS = {"double": dict(scales=(2.0,), lo_hi=(0.5, 8.0), d_train=2400), "both": dict(scales=(0.5, 2.0), lo_hi=(None, None), d_train=1500)}
EDGE_THRESHOLD = 25.0


@functools.lru_cache(maxsize=None)
def flush_case(ladder):
    """boxes of 96 x 80 planted flush with the right edge, with the bottom edge, and in the bottom right corner"""
    fr = frame()
    wins = [(W - 96, 60, 96, 80), (100, H - 80, 96, 80), (W - 96, H - 80, 96, 80)]
    kw = EDGE_LADDERS[ladder]
    return make(fr, {"edge": planted(fr, 41, (60, 30), wins)}, EDGE_THRESHOLD, scales=kw["scales"], lo_hi=kw["lo_hi"], d_train={"edge": kw["d_train"]})


@functools.lru_cache(maxsize=None)
def wide_case():
    """a box of 272 x 64: at level 0 the clamp's upper end W - w - 8 T = 16 lies below its lower end 8 T = 32"""
    fr = frame()
    c = make(fr, {"wide": planted(fr, 42, (60, 30), [(24, 88, 272, 64)])}, 0.0, d_train={"wide": 1000})
    c["threshold"] = first_threshold_with_records(c)
    return c


@functools.lru_cache(maxsize=None)
def huge_case():
    """a box of 400 x 300: larger than the top level (and than the frame); no position, no candidate, no error"""
    return make(frame(), {"huge": hand(43, (400, 300), ((30, 30), (20, 20)))}, 1.0, d_train={"huge": 1000}, expect="empty")


def outside(case, rec, level=0):
    """(features sampled at a cell column >= Wd, at a cell row >= Hd, at a column < 0, at a row < 0) of one record at its position of `level`
    (the record's own position for level 0)"""
    fr = case["frame"]
    name = (case["selection"] or sorted(case["classes"]))[int(rec["class_index"])]
    L, Tl = len(fr["T"]), fr["T"][level]
    F, w, h = sm.pm.entry_of(case["classes"][name], int(rec["template_id"]), level, L)
    sx, sy = sm.scaled_features(w, h, F[:, 0], F[:, 1], sc.ladder_q10(case["scales"])[int(rec["scale_index"])])
    off = Tl // 2 + (Tl % 2 - 1)
    cx, cy = (int(rec["x"]) - off + sx) // Tl, (int(rec["y"]) - off + sy) // Tl
    Wd, Hd = fr["sizes"][level][0] // Tl, fr["sizes"][level][1] // Tl
    return int((cx >= Wd).sum()), int((cy >= Hd).sum()), int((cx < 0).sum()), int((cy < 0).sum())


# ---- e. thresholds at and below zero ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked_case(threshold):
    """three pyramids on a frame whose left half is masked out while its depth stays measured"""
    fr = frame(mask_left=True)
    plain = frame()
    wins = [(180, 40, 48, 40), (200, 120, 56, 48), (230, 80, 40, 64)]
    return make(fr, {"m": planted(plain, 51, (60, 30), wins)}, threshold, d_train={"m": 1000})


def top_level(case, name):
    """[(positions, k, d, raw, nf)] per pyramid of class `name`: what the top level looks at (scaled_match_ref.coarse)"""
    fr = case["frame"]
    bank = case["classes"][name]
    q = sc.ladder_q10(case["scales"])
    lo_, hi_ = case.get("lo_hi", (None, None))
    P0 = sm.probe_map(fr["dep"], case.get("probe", 2))
    NP = (len(bank[1]) - 1) // (2 * len(fr["T"]))
    return [sm.coarse(bank, p, fr["lms"], fr["sizes"], fr["T"], P0, case["d_train"][name], q, q[0] if lo_ is None else sm.q10(lo_),
                      q[-1] if hi_ is None else sm.q10(hi_)) for p in range(NP)]


@functools.lru_cache(maxsize=None)
def exact_thresholds():
    """(t_top, t_low) on class b of the class scene.  t_top: a similarity some top-level cell has exactly, chosen so that a cell with exactly that
    score would go on to a record ABOVE it at level 0: `score > threshold` keeps it out, `>=` would let it in.  t_low: a similarity some record
    has exactly at level 0 whose top-level score lay above it: `sim < threshold` keeps it, `<=` would drop it."""
    base = make(frame(), {"b": class_banks()[0]["b"]}, 60.0, d_train={"b": 1000})
    tops = np.unique(np.concatenate([sm.pm.score_of(raw, nf) for _, _, _, raw, nf in top_level(base, "b")]))
    t_top = None
    for t in tops[(tops >= 60) & (tops < 90)][::-1]:
        below = np.nextafter(np.float32(t), np.float32(0))
        with_it, without = sm.canonical(reference(base, threshold=float(below))), sm.canonical(reference(base, threshold=float(t)))
        extra = set(sm.rows(with_it)) - set(sm.rows(without))
        if any(r[2] > t for r in extra):
            t_top = float(t)
            break
    rec = sm.canonical(reference(base))
    t_low = None
    for t in np.unique(rec["similarity"])[::-1]:
        if (sm.canonical(reference(base, threshold=float(t)))["similarity"] == t).any():
            t_low = float(t)
            break
    assert t_top is not None and t_low is not None
    return base, t_top, t_low


# ---- f. geometry ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_case():
    """T = (8,) on 328 x 200: 5 probe tiles and 8 px in x, 12 and 8 px in y"""
    fr = frame(seed=57, size=(328, 200), T=(8,))
    c = make(fr, {"g": planted(fr, 61, (40,), windows(7, 6, (328, 200)))}, 0.0, d_train={"g": 1000})
    c["threshold"] = first_threshold_with_records(c, (70.0, 65.0, 60.0, 55.0, 50.0))
    return c


# ---- the one-detector sequence ------------------------------------------------------------------------------------------------------------------------------
SMALL = (256, 192)
GROW_CAPACITY = 1024               # the smallest capacity lm_detector_set_candidate_capacity accepts
GROW_THRESHOLD = 20.0              # the reference has more than 2 x GROW_CAPACITY candidates there (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def small_frame():
    return frame(crop=SMALL)


def case(name):
    """the parity cases the GPU test runs through Detector.matchScaled, by name (PARITY_NAMES)"""
    if name.startswith("classes_"):
        return class_case(name[len("classes_"):])
    if name.startswith("big_"):
        return big_case(name[len("big_"):])
    if name.startswith("flush_"):
        return flush_case(name[len("flush_"):])
    return {"zero_62": zero_case, "zero_minus_1": lambda: zero_case(-1.0), "wide": wide_case, "huge": huge_case, "geometry": geometry_case}[name]()


PARITY_NAMES = ("classes_all", "classes_c_a", "classes_c_nope_a", "classes_a_a", "big_mixed", "big_limit", "big_over", "zero_62", "zero_minus_1",
                "flush_double", "flush_both", "wide", "huge", "geometry")
