"""Adversarial training frames for Detector.addTemplate (csrc/train.hip and its host twin), plain numpy, no GPU.

Every case is `(rgb, depth, mask, params)`: a small frame whose depth is piecewise planar (a normal label covers a region the case
controls) and whose colour image puts gradients where the case wants rim candidates.  `oracle_candidates` returns what the oracle
feeds to selectScatteredFeatures for such a frame, per level and modality; tests/test_train_cases.py asserts from it, on the CPU, that
every case really sits on the edge it is named after, and tests/test_gpu_train.py runs the cases on the device.

Levers the cases use:
  * the mask of level l is mask[::2^l, ::2^l] (nearest neighbour, LL.cpp:576): mask pixels at odd coordinates exist at level 0 only;
  * a colour ramp of slope s per pixel has a Sobel response of 8 s at level 0 and 16 s at level 1: candidates at level 1 only;
  * a depth jump of more than difference_threshold keeps the normals of two planes apart (LL.cpp:760).
The quantised normals are 0 in the outer 5 pixels of the frame (LL.cpp:745: the 5-pixel stencil), so a labelled run never reaches
the frame border itself: it ends at that margin.  test_train_cases.py asserts this for every case (the `kInf` run ends of
k_train_runs are out of reach of any frame), and case 6 asserts the nearest thing, a run that ends at the margin under a mask that
touches the border."""
import functools

import numpy as np

import linemod_oracle as lo

K_TRAIN_CAP = 16384            # csrc/lm_kernels.h: candidates per list the selection kernel sorts
K_TRAIN_MAX_FEATURES = 1024    # csrc/lm_kernels.h: features per template the selection kernel keeps

DEFAULTS = dict(num_features=63, T=[4, 8], strong_threshold=55.0, extract_threshold=2, weak_threshold=10.0, distance_threshold=2000,
                difference_threshold=50)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    p["T"] = list(p["T"])
    return p


_MODALITY_KEYS = ("strong_threshold", "extract_threshold", "weak_threshold", "distance_threshold", "difference_threshold")


def make_oracle(p):
    od = lo.OracleDetector(p["num_features"], p["T"])
    for k in _MODALITY_KEYS:
        setattr(od, k, p[k])
    return od


def oracle_candidates(od, rgb, depth, mask):
    """Per level {"color": stats, "normal": stats, "mask": level mask}; stats as linemod_oracle.extract_*_template fill them (n, cands
    in sorted order, scores, distance = the start distance, passes, last_distance) plus nf, the level's feature count."""
    probe, out = make_oracle(dict(DEFAULTS, num_features=od.num_features, T=od.T_at_level, **{k: getattr(od, k) for k in _MODALITY_KEYS})), []
    if probe.addTemplate([rgb, depth], "probe", mask, out) >= 0:
        return out
    out = []                                       # the view fails: addTemplate stops at the failing level, so walk the levels here
    nf, ext = od.num_features, od.extract_threshold
    for l, (_, _, mag, ang, normal, msk) in enumerate(od.quantize_pyramid(rgb, depth, mask)):
        if l > 0:
            nf //= 2
            ext //= 2
        c, n = {"nf": nf}, {"nf": nf, "extract_threshold": ext}
        lo.extract_color_template(mag, ang, msk, nf, od.strong_threshold, l, c)
        lo.extract_normal_template(normal, msk, nf, ext, l, n)
        out.append({"color": c, "normal": n, "mask": msk})
    return out


# ---- building blocks --------------------------------------------------------------------------------------------------------------

def plane(W, H, base, theta_deg, slope=1.0):
    """Depth of a plane tilted towards theta: with ~1 mm per pixel at ~1 m its normal falls well inside one LUT sector."""
    yy, xx = np.mgrid[0:H, 0:W]
    t = np.radians(theta_deg)
    return base + slope * (np.cos(t) * (xx - W / 2.0) + np.sin(t) * (yy - H / 2.0))


def finish_depth(d):
    return np.clip(np.rint(d), 1, 65535).astype(np.uint16)


def mosaic_depth(W, H, cell, x0=0, y0=0):
    """Cells of `cell` pixels, each its own plane: all eight tilt directions, neighbouring cells more than difference_threshold apart."""
    d = np.zeros((H, W))
    for j in range((H - y0 + cell - 1) // cell):
        for i in range((W - x0 + cell - 1) // cell):
            ys, xs = slice(y0 + j * cell, min(H, y0 + (j + 1) * cell)), slice(x0 + i * cell, min(W, x0 + (i + 1) * cell))
            d[ys, xs] = plane(W, H, 700 + 150 * ((i + 2 * j) % 4), 45 * ((i + 3 * j) % 8))[ys, xs]
    if y0:
        d[:y0] = plane(W, H, 1400, 90)[:y0]
    if x0:
        d[:, :x0] = plane(W, H, 1400, 0)[:, :x0]
    return d


def blocks(W, H, seed, cell=8):
    """Blocky colours: every block edge is a strong gradient."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, ((H + cell - 1) // cell, (W + cell - 1) // cell, 3)) * 64 + 30
    return np.repeat(np.repeat(g, cell, 0), cell, 1)[:H, :W].astype(np.uint8)


def object_on_dark(rgb, mask):
    out = rgb.copy()
    out[mask == 0] //= 5
    return out


def rect_mask(W, H, x0, y0, x1, y1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def _painted(W, H, rect, k, top, ramp_rows=0):
    """A flat grey frame; inside `rect` the rows from `top` on are painted bright, k half rows of them (a half row reaches the left
    edge only), in bands of four rows of different brightness: vertical steps on the rim's left and right side, as many as k says.
    ramp_rows > 0: the top of the frame carries a horizontal triangle ramp of slope 5 — rim candidates at level 1 only."""
    x0, y0, x1, y1 = rect
    img = np.full((H, W), 60, np.int32)
    if ramp_rows:
        xx = np.arange(W)
        img[:ramp_rows] = 40 + 5 * np.abs((xx % 80) - 40)
    for r in range((k + 1) // 2):
        y = top + r
        if y >= y1:
            break
        xe = x1 if (2 * r + 1 < k) else (x0 + x1) // 2
        img[y, x0:xe] = (150, 240, 180, 210)[(r // 4) % 4]
    return np.repeat(img[:, :, None], 3, 2).astype(np.uint8)


def _tune(build, od, target, ks, level=0, modality="color"):
    """The first k whose frame has exactly `target` candidates in the oracle's list of (level, modality)."""
    for k in ks:
        rgb, depth, mask = build(k)
        pyr = od.quantize_pyramid(rgb, depth, mask)
        _, _, mag, ang, normal, msk = pyr[level]
        s = {}
        lo.extract_color_template(mag, ang, msk, 1 << 30, od.strong_threshold, level, s)
        if s["n"] == target:
            return rgb, depth, mask
    raise AssertionError("no frame with %d candidates" % target)


# ---- the cases --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_fill(short):
    """1. n == nf at level 0 of the colour modality (short = 0), n == nf - 1 (short = 1: -1, decided on the device)."""
    W, H, rect = 96, 80, (20, 12, 76, 68)
    p = params(num_features=24)
    od = make_oracle(p)
    depth = finish_depth(plane(W, H, 900, 135))
    mask = rect_mask(W, H, *rect)
    return _tune(lambda k: (_painted(W, H, rect, k, rect[1] + 22, ramp_rows=rect[1] + 10), depth, mask), od, 24 - short, range(1, 70)) + (p,)


CHUNK_EDGES = {63: 8, 64: 16, 65: 16, 127: 24, 128: 32, 129: 32}     # n of the colour list -> num_features


@functools.lru_cache(maxsize=None)
def chunk_edge(n):
    """2. n around the 64-lane chunks of the selection loop."""
    W, H, rect = 96, 80, (12, 10, 84, 70)
    p = params(num_features=CHUNK_EDGES[n])
    od = make_oracle(p)
    depth = finish_depth(plane(W, H, 900, 45))
    mask = rect_mask(W, H, *rect)
    top = rect[1] + (4 if n < 100 else 0)          # the short lists come from the rim's sides alone, the long ones add its top
    return _tune(lambda k: (_painted(W, H, rect, k, top), depth, mask), od, n, range(1, 125)) + (p,)


@functools.lru_cache(maxsize=None)
def many_passes():
    """3. The normal list of level 1 is barely longer than nf: the schedule runs 2.7 -> 1.7 -> 0.7."""
    W, H = 96, 80
    p = params(num_features=32)
    mask = rect_mask(W, H, 40, 30, 60, 46)
    rgb = np.full((H, W, 3), 40, np.uint8)
    rgb[mask > 0] = (200, 120, 220)
    return rgb, finish_depth(plane(W, H, 900, 0)), mask, p


@functools.lru_cache(maxsize=None)
def ties():
    """4. A flat two-colour step image: the rim's straight sides share one magnitude each; the normal scores tie by construction."""
    W, H = 96, 80
    p = params(num_features=32)
    mask = rect_mask(W, H, 18, 14, 80, 66)
    rgb = np.full((H, W, 3), 40, np.uint8)
    rgb[mask > 0] = 200
    return rgb, finish_depth(plane(W, H, 900, 90)), mask, p


@functools.lru_cache(maxsize=None)
def mask_shapes():
    """5. A hole, a one-pixel spur, a three-pixel bar (erode^2 removes it) and a band that touches three frame borders."""
    W, H = 128, 96
    p = params(num_features=32)
    mask = rect_mask(W, H, 30, 30, 100, 82)
    mask[46:62, 55:71] = 0                       # hole
    mask[50, 100:116] = 255                      # spur
    mask[30:72, 14:17] = 255                     # bar
    mask[0:13, :] = 255                          # band: top, left and right border
    rgb = object_on_dark(blocks(W, H, 5), mask)
    return rgb, finish_depth(mosaic_depth(W, H, 32)), mask, p


@functools.lru_cache(maxsize=None)
def label_mosaic(ext):
    """6. Many small regions of all eight labels; a finger of the mask too narrow for a candidate; the mask touches the left border."""
    W, H = 128, 96
    p = params(num_features=16, extract_threshold=ext)
    mask = rect_mask(W, H, 0, 8, 112, 72)
    fw = {1: 6, 2: 6, 5: 10}[ext]                # erode^2 leaves fw - 4 columns: every distance below ext (ext >= 2)
    mask[72:90, 40:40 + fw] = 255
    rgb = object_on_dark(blocks(W, H, 7), mask)
    return rgb, finish_depth(mosaic_depth(W, H, 14, x0=6, y0=6)), mask, p


@functools.lru_cache(maxsize=None)
def thresholds(strong):
    """7. A body whose rim has a medium step (between 55 and 90) and mask lines at odd columns on strong steps: at 90 level 0 still
    fills, level 1 (which never sees the odd columns) does not."""
    W, H = 128, 96
    p = params(num_features=32, strong_threshold=float(strong))
    mask = rect_mask(W, H, 24, 40, 104, 84)
    img = np.full((H, W), 50, np.int32)
    img[mask > 0] = 84
    for x in range(31, 100, 10):
        mask[18:40, x] = 255
        img[16:38, x:x + 3] = 235
    rgb = np.repeat(img[:, :, None], 3, 2).astype(np.uint8)
    return rgb, finish_depth(plane(W, H, 900, 225)), mask, p


@functools.lru_cache(maxsize=None)
def odd_levels():
    """8. 150x110 with three levels: 75x55 and 37x27; the mask reaches the last column and row of every level."""
    W, H = 150, 110
    p = params(num_features=32, T=[4, 4, 8])
    mask = rect_mask(W, H, 50, 30, W, H)
    rgb = object_on_dark(blocks(W, H, 9), mask)
    rgb[:, 100:] = blocks(W, H, 10, cell=6)[:, 100:]      # gradients next to the right border, inside the mask
    return rgb, finish_depth(mosaic_depth(W, H, 40)), mask, p


@functools.lru_cache(maxsize=None)
def cap_boundary(over):
    """9. One label under a square mask: 128 x 128 normal candidates == kTrainCap (9a); one more column -> host (9b)."""
    W, H = 192, 160
    p = params()
    mask = rect_mask(W, H, 20, 13, 154 + over, 147)
    rgb = object_on_dark(blocks(W, H, 11), mask)
    return rgb, finish_depth(plane(W, H, 1000, 45)), mask, p


@functools.lru_cache(maxsize=None)
def feature_ceiling(nf):
    """10. 1024 features (kTrainMaxFeatures: device) and 1025 (host): an object full of small holes, a long rim."""
    W, H = 224, 176
    p = params(num_features=nf, extract_threshold=3)
    mask = rect_mask(W, H, 8, 8, 216, 168)
    for y in range(14, 160, 16):
        for x in range(14, 208, 16):
            mask[y:y + 4, x:x + 4] = 0
    rgb = object_on_dark(blocks(W, H, 13, cell=16), mask)
    return rgb, finish_depth(plane(W, H, 1000, 315)), mask, p


# name -> (builder, expected path, the view trains)
CASES = {
    "1_exact_fill": (lambda: exact_fill(0), "device", True),
    "1_one_short": (lambda: exact_fill(1), "device", False),
    "3_many_passes": (many_passes, "device", True),
    "4_ties": (ties, "device", True),
    "5_mask_shapes": (mask_shapes, "device", True),
    "7_strong_20": (lambda: thresholds(20), "device", True),
    "7_strong_55": (lambda: thresholds(55), "device", True),
    "7_strong_90": (lambda: thresholds(90), "device", False),
    "8_odd_levels": (odd_levels, "device", True),
    "9a_at_cap": (lambda: cap_boundary(0), "device", True),
    "9b_over_cap": (lambda: cap_boundary(1), "host", True),
    "10a_1024_features": (lambda: feature_ceiling(1024), "device", True),
    "10b_1025_features": (lambda: feature_ceiling(1025), "host", True),
}
for _n in CHUNK_EDGES:
    CASES["2_chunk_n%d" % _n] = (functools.partial(chunk_edge, _n), "device", True)
for _e in (1, 2, 5):
    CASES["6_mosaic_ext%d" % _e] = (functools.partial(label_mosaic, _e), "device", True)


@functools.lru_cache(maxsize=None)
def analysed(name):
    """(frame, oracle candidates, oracle addTemplate result, oracle templates or None), computed once per process."""
    rgb, depth, mask, p = CASES[name][0]()
    od, cand = make_oracle(p), []
    oid = od.addTemplate([rgb, depth], "obj", mask, cand)
    if oid < 0:
        cand = oracle_candidates(od, rgb, depth, mask)
    return (rgb, depth, mask, p), cand, oid, (od.class_templates["obj"][oid] if oid >= 0 else None)
