"""The inputs of test_gpu_part_match_edges.py and the reference's answers on them (part_match_ref.py), computed once per process and never
modified.  Every threshold here was chosen on the CPU from the reference alone; test_part_match_cases.py proves, again on the reference alone,
the condition that justifies each of them, so that no case of the GPU file passes on an empty or an indifferent list.

Groups: 1. every build of k_coarse_parts / k_local_parts (the table's low weight 1, 2, 3 x counters of 9 and 14 bits); 2. top-level maps of
more than 2048 positions (the second pass of the coarse loop); 3. several classes in one request; 4. thresholds that a part's score attains
exactly, 100 and beyond, and 0; 5. detectors of one modality, grey frames and frames padded or cropped to the T grid."""
import functools

import numpy as np

import linemod_oracle as lo
import part_match_ref as pm
import response_table_ref as rt
import synth
import test_part_match_ref as cpu

F32 = np.float32


# ---- banks ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_bank(levels):
    """One bank on G1's frame: a template with all its features in one part; parts of 7, 8, 9, 16 and 17 features (padding); an entry of 600
    features (the 14-bit counters); a template as wide as the refinement allows, whose position count lies below the map's."""
    rng = np.random.default_rng(77)
    feats, whs = [], []

    def entry(per_part, w, h, l):
        quad = [(0, w // 2, 0, h // 2), ((w + 1) // 2, w + 1, 0, h // 2), (0, w // 2, (h + 1) // 2, h + 1), ((w + 1) // 2, w + 1, (h + 1) // 2, h + 1)]
        rows = [(int(rng.integers(a, b)), int(rng.integers(c, d)), int(rng.integers(0, 8)), k % 2) for (a, b, c, d), n in zip(quad, per_part) for k in range(n)]
        for m in range(2):
            feats.append(np.array([r[:3] for r in rows if r[3] == m], np.int32).reshape(-1, 3)); whs.append((w >> 0, h >> 0))

    shapes = [((40, 0, 0, 0), 60, 48), ((7, 8, 9, 16), 60, 48), ((17, 16, 8, 7), 50, 40), ((150, 150, 150, 150), 64, 48), ((20, 20, 20, 20), 120, 90)]
    for per_part, w, h in shapes:
        for l in range(levels):
            entry(per_part, w >> l, h >> l, l)
    offs = np.zeros(len(feats) + 1, np.int32)
    offs[1:] = np.cumsum([len(f) for f in feats])
    return np.ascontiguousarray(np.concatenate(feats), np.int32), offs, np.array(whs, np.int32).reshape(-1, 2)


def concat_banks(*banks):
    """packed banks of the same level count, one after the other"""
    feat = np.ascontiguousarray(np.concatenate([b[0] for b in banks]), np.int32)
    offs = [np.asarray(banks[0][1], np.int64)]
    for b in banks[1:]:
        offs.append(np.asarray(b[1][1:], np.int64) + offs[-1][-1])
    return feat, np.concatenate(offs).astype(np.int32), np.concatenate([np.asarray(b[2], np.int32).reshape(-1, 2) for b in banks])


def pyramids(bank, L):
    return (len(bank[1]) - 1) // (2 * L)


def max_entry(bank, L):
    """the largest feature count of an entry (both modalities), what chooses the counter width: <= 511 -> 9 bits, beyond -> 14"""
    return max(len(pm.entry_of(bank, p, l, L)[0]) for p in range(pyramids(bank, L)) for l in range(L))


def two_slot(single, L):
    """a packed bank of levels x 1 templates (a one-modality detector's) -> the levels x 2 layout of part_match_ref: the present modality in
    slot 0, an empty slot 1 (modality_ref.py)"""
    feat, offs, wh = single
    o, whs = [0], []
    for e in range(len(offs) - 1):
        o += [int(offs[e + 1]), int(offs[e + 1])]
        whs += [tuple(wh[e]), tuple(wh[e])]
    return np.ascontiguousarray(feat, np.int32), np.array(o, np.int32), np.array(whs, np.int32).reshape(-1, 2)


def one_slot(double, L):
    """the inverse of two_slot for a bank whose second slots are empty"""
    feat, offs, wh = double
    assert all(offs[e + 1] == offs[e] for e in range(1, len(offs) - 1, 2))
    return np.ascontiguousarray(feat, np.int32), np.ascontiguousarray(offs[::2], np.int32), np.ascontiguousarray(wh[::2], np.int32)


def fitting(bank, W, H, T):
    """the pyramids of a bank that part matching accepts on a W x H frame, as a bank (test_part_match_ref.fitting_bank for any bank)"""
    keep = [p for p in range(pyramids(bank, len(T))) if cpu.windows_stay_inside(bank, W, H, T, p)]
    return cpu.sub_bank(bank, len(T), keep), keep


def multiset5(raw):
    """(x, y, similarity, class, template) of reference records, sorted"""
    return sorted(zip(raw["x"].tolist(), raw["y"].tolist(), raw["sim"].tolist(), raw["cls"].tolist(), raw["tid"].tolist()))


def canonical(raw):
    """the canonical list of reference records as the same tuples"""
    c = lo.canonical_sort_unique(raw)
    return list(zip(c["x"].tolist(), c["y"].tolist(), c["sim"].tolist(), c["cls"].tolist(), c["tid"].tolist()))


# ---- 1. every kernel build: tables x counter widths --------------------------------------------------------------------------------------------
# The low plane of a two-plane table carries its smaller non-zero value: weight 2 under 4 2 0 0 0, 3 under 4 3 0 0 0, and 1 (an empty low plane
# resp. the code of the default table) under the one-value tables 4 4 0 0 0 and 4 0 0 0 0.  The banks choose the counters: G1's planted bank
# (entries of 300 features: 9 bits) and edge_bank (an entry of 600: 14 bits).
TABLES = {"levelup2": (4, 2, 0, 0, 0), "4_3": (4, 3, 0, 0, 0), "4_4": (4, 4, 0, 0, 0), "4_0": (4, 0, 0, 0, 0)}
BUILD_BANKS = ("planted", "edge")
# Scores of different tables are not comparable, so every table x bank has its own threshold: the highest of a 4-point grid at which the
# reference still has records for three of the four min_parts under both min_part_features (a higher threshold = fewer candidates = a
# quicker reference); test_part_match_cases.py asserts that, and that the lists differ from the default table's and from the holistic one.
BUILD_THRESHOLDS = {"planted": {"levelup2": 84.0, "4_3": 88.0, "4_4": 92.0, "4_0": 82.0},
                    "edge": {"levelup2": 40.0, "4_3": 45.0, "4_4": 50.0, "4_0": 30.0}}
BUILD_RULES = tuple((mp, mpf) for mpf in (1, 8) for mp in (1, 2, 3, 4))


def build_bank(bank):
    return cpu.fitting_bank("G1", "planted")[0] if bank == "planted" else edge_bank(2)


@functools.lru_cache(maxsize=None)
def build_reference(table, bank, min_parts, mpf, memories=None):
    """the reference on G1's frame at the threshold of table x bank, on the memories of `memories` (a name of TABLES or "levelup", the default
    table; None: `table` itself); min_parts = 0: the holistic list"""
    lms, sizes = rt.memories("G1", TABLES.get(memories or table, rt.DEFAULT))
    return pm.match_parts(build_bank(bank), lms, sizes, rt.scene("G1")["T"], BUILD_THRESHOLDS[bank][table], min_parts, mpf)


# ---- 2. maps of more than 2048 top-level positions ---------------------------------------------------------------------------------------------
# 256 x 160 at T = 4 is a map of 64 x 40 = 2560 positions: position 2048 is the first of row 32, y = 128.  A template has sums at positions
# beyond 2047 iff it is at most 32 pixels high there (limit = (40 - hf) 64 + 64 - wf + 1), so six windows are 20..30 pixels high and lie at
# y = 120..132, on both sides of row 32, and four are higher (limit < 2048).  "one": the map is the only level; "two": it is the top of
# 512 x 320 under T = (4, 4), the windows doubled.
_WINDOWS = [(20, 130, 60, 24), (100, 132, 50, 20), (170, 128, 70, 28), (40, 120, 48, 30), (120, 124, 56, 26), (200, 126, 40, 24),
            (30, 30, 80, 60), (120, 40, 90, 70), (60, 60, 64, 48), (150, 20, 70, 90)]
BIG = {"one": {"W": 256, "H": 160, "T": (4,), "seed": 34, "nfeat": (40,), "windows": _WINDOWS},
       "two": {"W": 512, "H": 320, "T": (4, 4), "seed": 35, "nfeat": (80, 40), "windows": [tuple(2 * v for v in w) for w in _WINDOWS]}}
BIG_RULES = ((2, 8, 70.0), (1, 1, 60.0))                       # (min_parts, min_part_features, threshold)
BIG_STREAM_RULE = (1, 1, 60.0)
BIG_STREAM_SEEDS = (134, 234)                                  # the two further frames of the batch of 3


@functools.lru_cache(maxsize=None)
def big_scene(name):
    g = BIG[name]
    T = list(g["T"])
    od = lo.OracleDetector(150, T)
    frames = [synth.make_frame(s, g["W"], g["H"], 14) for s in (g["seed"],) + BIG_STREAM_SEEDS]
    pyrs = [od.quantize_pyramid(*f) for f in frames]
    bank = synth.make_planted_bank(41, len(g["windows"]), [(p[0], p[1]) for p in pyrs[0]], T, g["nfeat"], windows=g["windows"])
    mems = [rt.linear_memories(p, T, rt.DEFAULT) for p in pyrs]
    return {"W": g["W"], "H": g["H"], "T": T, "frames": frames, "bank": bank, "mems": mems, "npos": (g["W"] >> (len(T) - 1)) // T[-1] * ((g["H"] >> (len(T) - 1)) // T[-1])}


@functools.lru_cache(maxsize=None)
def big_reference(name, frame, min_parts, mpf, thr):
    """(records, trace) of frame `frame` of a big scene"""
    s = big_scene(name)
    tr = []
    rec = pm.match_parts(s["bank"], *s["mems"][frame], s["T"], thr, min_parts, mpf, trace=tr)
    return rec, tr


# ---- 3. several classes in one request ----------------------------------------------------------------------------------------------------------
# Three classes on G1's frame, 7, 10 and 5 templates, added under names whose sorted order (the order of the detector's bank) is not the order
# they are added in.  The first two planted templates are in all of them under the same template ids, so their records differ in the class
# alone; the others are random templates, different ones per class, and "m" ends with the 600-feature entry of edge_bank (the 14-bit build
# for the whole request).  The threshold is one at which the random templates have records too.
CLASS_ORDER = ("z", "b", "m")
CLASS_REQUESTS = (("z", "b", "m"), ("m", "z", "b"), ("b", "m"), ("z", "b", "z"), ("b", "unknown", "z"))
CLASS_RULE = (1, 8, 33.0)


@functools.lru_cache(maxsize=None)
def class_banks():
    planted, rnd = cpu.fitting_bank("G1", "planted")[0], cpu.fitting_bank("G1", "random")[0]
    two = cpu.sub_bank(planted, 2, range(2))
    return {"z": concat_banks(two, cpu.sub_bank(rnd, 2, range(0, 5))),
            "b": concat_banks(two, cpu.sub_bank(rnd, 2, range(5, 13))),
            "m": concat_banks(two, cpu.sub_bank(rnd, 2, range(13, 15)), cpu.sub_bank(edge_bank(2), 2, [3]))}


@functools.lru_cache(maxsize=None)
def _class_reference(name):
    lms, sizes = rt.memories("G1", rt.DEFAULT)
    mp, mpf, thr = CLASS_RULE
    return pm.match_parts(class_banks()[name], lms, sizes, rt.scene("G1")["T"], thr, mp, mpf)


def request_reference(request):
    """the reference per class, the class column = the class's place in the request (an unknown class keeps its place and has no records)"""
    out = []
    for i, name in enumerate(request):
        if name in CLASS_ORDER:
            r = _class_reference(name).copy()
            r["cls"] = i
            out.append(r)
    return np.concatenate(out)


# ---- 4. ties, 100 and beyond, 0 ------------------------------------------------------------------------------------------------------------------
# A candidate's fate hangs on ONE score: its critical score = the min_parts-th largest score among its eligible parts.  At the top it must be
# > threshold, below >= threshold.  The thresholds below are float32 values that, on G1's fitting planted bank, are the critical score of top-level
# positions AND of refined candidates (found by searching the reference's attained scores; counted again by test_part_match_cases.py):
# between nextafter(t, -inf) and t the top-level candidates change, between t and nextafter(t, +inf) the candidates dropped below the top.
TIES = {("levelup", 1): float(F32(67.85713958740234)), ("levelup", 2): 67.5,
        ("levelup2", 1): float(F32(80.55555725097656)), ("levelup2", 2): float(F32(80.95237731933594))}


def around(t):
    return (float(np.nextafter(F32(t), F32(-np.inf))), float(F32(t)), float(np.nextafter(F32(t), F32(np.inf))))


def critical(raw, n, min_parts, mpf):
    """the min_parts-th largest score among the eligible parts of raw [candidates][4] (-1 where fewer parts are eligible)"""
    sc = np.stack([pm.score_of(raw[:, k], n[k]) if n[k] >= mpf else np.full(len(raw), -1, F32) for k in range(4)], 1)
    return np.sort(sc, 1)[:, 4 - min_parts]


@functools.lru_cache(maxsize=None)
def tie_reference(table, min_parts, thr):
    """(records, trace) on G1's fitting planted bank under a named table, min_part_features 8"""
    lms, sizes = rt.memories("G1", rt.NAMED[table])
    tr = []
    rec = pm.match_parts(cpu.fitting_bank("G1", "planted")[0], lms, sizes, rt.scene("G1")["T"], thr, min_parts, 8, trace=tr)
    return rec, tr


def level_counts(trace, top):
    """(candidates that left the top level, candidates dropped below it) of a trace"""
    return (sum(t["left"] for t in trace if t["level"] == top), sum(t["entered"] - t["left"] for t in trace if t["level"] != top))


# 100 and beyond: six templates of G1 planted without label noise, so at their plants every feature scores 4 and every part exactly 100.
HUNDRED = (float(np.nextafter(F32(100), F32(0))), 100.0, 100.5, float("inf"))


@functools.lru_cache(maxsize=None)
def perfect_bank():
    sc = rt.scene("G1")
    windows = [(40, 40, 60, 50), (90, 36, 70, 60), (36, 70, 80, 48), (100, 80, 50, 44), (60, 50, 64, 64), (44, 60, 90, 56)]
    bank = synth.make_planted_bank(45, len(windows), [(p[0], p[1]) for p in sc["pyr"]], sc["T"], (150, 75), label_noise=0.0, windows=windows)
    return fitting(bank, sc["W"], sc["H"], sc["T"])[0]


@functools.lru_cache(maxsize=None)
def perfect_reference(thr, min_parts):
    lms, sizes = rt.memories("G1", rt.DEFAULT)
    tr = []
    rec = pm.match_parts(perfect_bank(), lms, sizes, rt.scene("G1")["T"], thr, min_parts, 8, trace=tr)
    return rec, tr


# 0: two planted templates of G1 whose level-0 entries keep part 0 and, of every other part, 8 features that point the other way (label + 4: no
# response where the plant responds), so that eligible parts have a sum of 0 at refined positions — and pass `>= 0`.
ZERO_RULE = (4, 8, 0.0)                                     # all four parts must pass: a part with a sum of 0 decides


@functools.lru_cache(maxsize=None)
def zero_bank():
    feat, offs, wh = cpu.sub_bank(cpu.fitting_bank("G1", "planted")[0], 2, [0, 1])
    out = []
    for e in range(len(offs) - 1):
        f = feat[offs[e]:offs[e + 1]].copy()
        if e % 4 < 2:                                                         # level 0, either modality
            part = pm.part_of(f[:, 0], f[:, 1], int(wh[e][0]), int(wh[e][1]))
            rows = [f[part == 0]]
            for k in (1, 2, 3):                                               # 4 per modality = 8 per part: just eligible
                t = f[part == k][:4]
                t[:, 2] = (t[:, 2] + 4) % 8
                rows.append(t)
            f = np.concatenate(rows)
        out.append(f)
    o = np.zeros(len(out) + 1, np.int32)
    o[1:] = np.cumsum([len(f) for f in out])
    return np.ascontiguousarray(np.concatenate(out), np.int32), o, wh


@functools.lru_cache(maxsize=None)
def zero_reference():
    lms, sizes = rt.memories("G1", rt.DEFAULT)
    mp, mpf, thr = ZERO_RULE
    tr = []
    rec = pm.match_parts(zero_bank(), lms, sizes, rt.scene("G1")["T"], thr, mp, mpf, trace=tr)
    return rec, tr


# ---- 5. detectors of other kinds -----------------------------------------------------------------------------------------------------------------
# Each on the smallest geometry its own GPU test matches on, its memories from that test's reference; the bank = what part matching accepts of
# that test's bank (a few templates of it: the reference is a loop per candidate).  -> kwargs of the Detector, its border, the sources, the bank
# as addClassPacked takes it, and (bank, memories, sizes) as part_match_ref takes them.
KINDS = ("colour", "depth", "grey", "pad", "crop")
KIND_RULES = ((2, 1), (1, 1))                                   # (min_parts, min_part_features)
KIND_THRESHOLD = {"colour": 62.0, "depth": 62.0, "grey": 70.0, "pad": 75.0, "crop": 75.0}


@functools.lru_cache(maxsize=None)
def kind_case(kind):
    import modality_ref as mr
    if kind in ("colour", "depth"):
        W, H, T = 208, 176, [4, 8]                                               # test_gpu_modalities.GEOMS["small"]
        k = KINDS.index(kind)
        sc = mr.scene(W, H, tuple(T))
        maps = mr.present_maps(sc["pyr"], k)
        whole = two_slot(mr.pack_single(mr.make_bank(11, 36, 12, maps, T, 63)), 2)
        keep = [p for p in list(range(10)) + list(range(36, 40)) if cpu.windows_stay_inside(whole, W, H, T, p)]      # planted and random ones
        bank = cpu.sub_bank(whole, 2, keep)
        lms, sizes = mr.linear_memories(maps, T)
        return {"nf": 63, "T": T, "kwargs": {"modalities": mr.SETS[k]}, "border": None, "sources": [sc["rgb"] if k == 0 else sc["dep"]],
                "packed": one_slot(bank, 2), "bank": bank, "lms": lms, "sizes": sizes}
    if kind == "grey":
        import test_gpu_grey as gg
        s = gg.scene()                                                            # 320 x 240, T = (4, 8)
        g, rep, dep = s["frames"][0]
        bank = fitting(s["bank"], s["W"], s["H"], s["T"])[0]
        lms, sizes = s["od"].linear_memories(rep, dep)
        return {"nf": s["nf"], "T": s["T"], "kwargs": {"colour_channels": 1}, "border": None, "sources": [g, dep], "packed": bank, "bank": bank, "lms": lms, "sizes": sizes}
    import test_gpu_frame_border as fbt
    s = fbt.scene("313x229")                                                      # -> 320 x 240 padded, 304 x 224 cropped
    colour, dep, _ = fbt.aligned(s["frame"], s["T"], kind)
    Ha, Wa = dep.shape
    assert (Wa, Ha) != (s["W"], s["H"])
    bank = cpu.sub_bank(s["bank"], 2, [p for p in range(s["n"] - 14, s["n"]) if cpu.windows_stay_inside(s["bank"], Wa, Ha, s["T"], p)])   # the last ones: the two at the source's edges among them
    lms, sizes = s["od"].linear_memories(colour, dep)
    return {"nf": s["nf"], "T": s["T"], "kwargs": {}, "border": kind, "sources": list(s["frame"]), "packed": bank, "bank": bank, "lms": lms, "sizes": sizes}


@functools.lru_cache(maxsize=None)
def kind_reference(kind, min_parts, mpf):
    """min_parts = 0: the holistic list"""
    c = kind_case(kind)
    return pm.match_parts(c["bank"], c["lms"], c["sizes"], c["T"], KIND_THRESHOLD[kind], min_parts, mpf)
