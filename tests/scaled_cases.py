"""The inputs shared by test_scaled_match_ref.py (which proves the conditions on them, on the CPU) and test_gpu_scaled_match.py.

Frames of 320 x 240 with T = (4, 8): the smallest VGA-like geometry at which both levels keep a non-empty clamp range for boxes up to 64 px.
Banks of 24 templates planted in the frame's own quantised maps (synth.make_planted_bank), boxes of 32..64 px, away from the right and bottom
edges so that no holistic candidate sits on a cell whose reads wrap."""
import functools

import numpy as np

import linemod_oracle as lo
import part_match_ref as pm
import response_table_ref as rt
import scaled_match_ref as sm
import synth

W, H = 320, 240
T2, T1, T3 = (4, 8), (8,), (4, 4, 4)
NFEAT = {2: (60, 30), 1: (40,), 3: (60, 30, 16)}
D_TRAIN = 1000
THRESHOLD = 70.0
LADDERS = {1: (1.0,), 3: (0.75, 1.0, 1.25), 9: tuple(2.0 ** (i / 4.0 - 1.0) for i in range(9)),
           16: tuple(0.5 + 0.1 * i for i in range(16))}
PROBES = (0, 2, 4)
PARITY_BOUNDS = {1: (0.5, 2.0), 3: (None, None), 9: (None, None), 16: (None, None)}    # (min_scale, max_scale): a ladder of one needs room around it


def ladder_q10(scales):
    return [sm.q10(s) for s in scales]


@functools.lru_cache(maxsize=None)
def scene(T=T2, seed=53, size=(W, H)):   # (seed: the first from 51 on at which no holistic candidate of any of the three pyramids sits on a cell whose reads wrap)
    """frame, quantised pyramid, linear memories (default table) and a planted bank of 24 for the pyramid T"""
    w0, h0 = size
    rgb, dep = synth.make_frame(seed, w0, h0, 14)
    return scene_of(rgb, dep, T)


def scene_of(rgb, dep, T):
    h0, w0 = dep.shape
    od = lo.OracleDetector(150, list(T))
    pyr = od.quantize_pyramid(rgb, dep)
    qp = [(p[0], p[1]) for p in pyr]
    rng = np.random.default_rng(77)
    border = 8 * T[0] + 2
    windows = []
    for _ in range(24):
        w, h = int(rng.integers(32, 65)), int(rng.integers(32, 65))
        windows.append((int(rng.integers(border, w0 - w - border - 16)), int(rng.integers(border, h0 - h - border - 16)), w, h))
    bank = synth.make_planted_bank(61, 24, qp, list(T), NFEAT[len(T)], windows=windows)
    lms, sizes = rt.linear_memories(pyr, list(T), rt.DEFAULT)
    return {"T": list(T), "rgb": rgb, "dep": dep, "pyr": pyr, "bank": bank, "lms": lms, "sizes": sizes, "windows": windows}


@functools.lru_cache(maxsize=None)
def reference(T=T2, ladder=9, probe=2, threshold=THRESHOLD, d_train=D_TRAIN, lo_hi=(None, None), scales=None):
    """(raw records, statistics) of the reference on scene(T); ladder: a key of LADDERS, or `scales` as floats"""
    sc = scene(T)
    q = ladder_q10(scales if scales is not None else LADDERS[ladder])
    st = {}
    raw = sm.match_scaled(sc["bank"], sc["lms"], sc["sizes"], sc["T"], threshold, sc["dep"], d_train, q,
                          None if lo_hi[0] is None else sm.q10(lo_hi[0]), None if lo_hi[1] is None else sm.q10(lo_hi[1]), probe, stats=st)
    return raw, st


@functools.lru_cache(maxsize=None)
def anchor_depth():
    """the probed depth under the best record of the ladder {1024} with open bounds: the d_train of the `bounds` and `tie` cases"""
    raw, _ = reference(T2, 1, 2, THRESHOLD, D_TRAIN, (0.25, 4.0))
    best = sm.canonical(raw)[0]
    return int(best["depth_mm"])


# the edge cases: name -> keyword arguments of reference() / Detector.matchScaledResident
def edge_cases():
    d0 = anchor_depth()
    return {
        "bounds": dict(scales=(1.0,), d_train=d0, lo_hi=(1.0, 1.0)),                   # only cells with d == d_train: both bounds inclusive
        "tie": dict(scales=(0.75, 1.25), d_train=d0),                                  # d == d_train: |768 d - 1024 d| == |1280 d - 1024 d|, k = 0
        "double": dict(scales=(2.0,), d_train=2400, lo_hi=(0.5, 8.0), threshold=25.0),  # scale 2048 everywhere: cdx < 0 at the left and top
        "half": dict(scales=(0.5,), d_train=450, lo_hi=(0.25, 1.0), threshold=60.0),   # scale 512: features coincide
    }


def holistic(T=T2, threshold=THRESHOLD):
    sc = scene(T)
    return pm.match_parts(sc["bank"], sc["lms"], sc["sizes"], sc["T"], threshold, 0)


def as_holistic(rec):
    """(x, y, similarity, template_id) rows of scaled or MATCH records"""
    sim = rec["similarity"] if "similarity" in rec.dtype.names else rec["sim"]
    tid = rec["template_id"] if "template_id" in rec.dtype.names else rec["tid"]
    return sorted(zip(rec["x"].tolist(), rec["y"].tolist(), sim.tolist(), tid.tolist()))


def normals_only(bank, L):
    """(the bank with its colour features removed — two slots per level, for the reference —, the same as a bank of one modality per level)"""
    feat, offs, wh = bank
    f2, w2, f1, w1 = [], [], [], []
    for e in range(len(offs) - 1):
        f = feat[offs[e]:offs[e + 1]]
        if e % 2 == 0:
            f2.append(f[:0]); w2.append(wh[e])
        else:
            f2.append(f); w2.append(wh[e]); f1.append(f); w1.append(wh[e])
    return synth._finish(f2, w2), synth._finish(f1, w1)


# ---- efficacy: one object trained at 1000 mm, seen at 700 mm and at 1400 mm ---------------------------------------------------------------------
EFFICACY_T = (4, 8)
EFFICACY_Z = (700, 1400)
EFFICACY_THRESHOLD = 80.0          # asserted on the CPU (test_scaled_match_ref): the reference finds the object there, the holistic oracle does not
EFFICACY_RADIUS = 8                # px between the record's box centre and the object's: two level-0 cells


def blob_view(z, centre=(160.0, 120.0)):
    """An ellipsoidal cap with ripples, 40 x 30 px half axes at 1000 mm, whose front stands z mm away: its image scales by 1000 / z, its relief
    (60 mm behind the front) stays.  Colour follows the relief, the background is flat (depth 0 = no measurement).  An analytic stand-in for a
    rendered mesh: the same view at every distance, to the pixel, which the CPU assertions need."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    s = 1000.0 / z
    u, v = (xx - centre[0]) / s, (yy - centre[1]) / s
    th = 0.6
    u, v = u * np.cos(th) + v * np.sin(th), -u * np.sin(th) + v * np.cos(th)
    r2 = (u / 40.0) ** 2 + (v / 30.0) ** 2
    inside = r2 < 1
    relief = 60.0 * np.sqrt(np.clip(1 - r2, 0, None)) + 8.0 * np.sin(u / 5.0) * np.cos(v / 7.0)
    dep = np.where(inside, z + 60.0 - relief, 0).astype(np.uint16)
    shade = np.clip(60 + 2.5 * relief + 30 * np.sin(u / 4.0), 0, 255)
    rgb = np.where(inside[..., None], np.stack([shade, 0.8 * shade, 255 - shade], -1), 90.0).astype(np.uint8)
    return np.ascontiguousarray(rgb), np.ascontiguousarray(dep)


@functools.lru_cache(maxsize=None)
def efficacy():
    """the trained bank (one template, the oracle's addTemplate of the view at 1000 mm), its training depth (1000 mm: where the view was made)
    and per scene depth: frame, memories, the reference's and the holistic oracle's records, the expected scale index"""
    T = list(EFFICACY_T)
    od = lo.OracleDetector(63, T)
    rgb, dep = blob_view(1000)
    assert od.addTemplate([rgb, dep], "obj", ((dep > 0) * 255).astype(np.uint8)) == 0
    pb = lo.pack_bank(od.class_templates["obj"], 2)
    bank = (pb.feat, pb.tmpl_off, pb.tmpl_wh)
    d_train = 1000
    scales = LADDERS[9]
    out = {"bank": bank, "d_train": d_train, "scales": scales, "train": (rgb, dep), "box": tuple(int(v) for v in pb.tmpl_wh[0]), "scenes": {}}
    for z in EFFICACY_Z:
        rgb, dep = blob_view(z)
        lms, sizes = rt.linear_memories(od.quantize_pyramid(rgb, dep), T, rt.DEFAULT)
        want = sm.match_scaled(bank, lms, sizes, T, EFFICACY_THRESHOLD, dep, d_train, ladder_q10(scales))
        hol = pm.match_parts(bank, lms, sizes, T, EFFICACY_THRESHOLD, 0)
        k = int(np.argmin([abs(s - 1000.0 / z) for s in scales]))
        out["scenes"][z] = {"rgb": rgb, "dep": dep, "want": want, "hol": hol, "k": k}
    return out


def on_object(rec, box, radius=EFFICACY_RADIUS, centre=(160, 120)):
    """the records whose box centre (x + w0 // 2, y + h0 // 2) lies within `radius` px (each axis) of the object's centre"""
    cx, cy = rec["x"] + box[0] // 2, rec["y"] + box[1] // 2
    return rec[(np.abs(cx - centre[0]) <= radius) & (np.abs(cy - centre[1]) <= radius)]
