"""Seeded frames that put the front end (csrc/fe_quant.hip, csrc/fe_bits.hip) on its edges, each with the modality parameters it needs and a CONDITION
function: given the oracle's intermediates (the `parts` of quantized_orientations / quantized_normals_raw) it counts the pixels that sit on
the edge the case is about.  tests/test_frontend_cases.py asserts those counts and holds the oracle to the scalar restatement
(frontend_scalar_ref.py) on every frame; tests/test_gpu_frontend_edges.py runs the same frames through the kernels.

A case is a dict: name, rgb (H, W, 3) u8, dep (H, W) u16, T, params (weak_threshold, distance_threshold, difference_threshold; what is
not named keeps the default), about ("colour" / "depth": the modality whose chain the case is built for — the other source is a benign
filler), need {count name: minimum} and cond(parts) -> {count name: value}.  Nothing here is random at run time: every seed is fixed and
was chosen on the CPU so that the conditions hold.

Sizes: 96 x 64 spans 3 x 4 colour tiles of 32 x 16 (halos 5, 2, 1) and has a 48 x 32 level 1; 100 x 96 under T = (2, 2) has rows that are no
multiple of a dword at level 1; 1280 x 32 makes the decimated raster index of the linear memories (n of fast_div) span many rows; 320 x 240 is
the largest (the tap lattice needs 512 centres 11 apart).  The smallest frame a detector takes is 16 x 16; 24 x 16 under T = (2, 2) has a
12 x 8 level 1, smaller than a colour tile's halo."""
import numpy as np

import linemod_oracle as lo

DEFAULTS = {"weak_threshold": 10.0, "strong_threshold": 55.0, "distance_threshold": 2000, "difference_threshold": 50}
DIFFS = (1, 49, 50, 150, 151, 70000)
TAPS = ((-5, -5), (0, -5), (5, -5), (-5, 0), (5, 0), (-5, 5), (0, 5), (5, 5))          # (i, j) = (x, y) offsets, the reference's order


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def filler_depth(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return (900 + 3 * xx + 2 * yy).astype(np.uint16)


def filler_rgb(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(np.stack([(40 + 2 * xx) % 256, (30 + 3 * yy) % 256, (200 - xx - yy) % 256], 2).astype(np.uint8))


def colour_parts(rgb, weak):
    parts = {}
    mag, out = lo.quantized_orientations(rgb, weak, parts)
    parts.update(mag=mag, out=out)
    return parts


def depth_parts(dep, dist, diff):
    parts = {}
    raw = lo.quantized_normals_raw(dep, dist, diff, parts)
    parts.update(raw=raw)
    return parts


def case_parts(c):
    """the oracle's intermediates of the chain the case is about"""
    p = c["params"]
    if c["about"] == "colour":
        return colour_parts(c["rgb"], p["weak_threshold"])
    return depth_parts(c["dep"], p["distance_threshold"], p["difference_threshold"])


def _colour(name, rgb, cond, need, T=(2, 2), **kw):
    H, W = rgb.shape[:2]
    return {"name": name, "about": "colour", "rgb": np.ascontiguousarray(rgb.astype(np.uint8)), "dep": filler_depth(W, H), "T": list(T),
            "params": params(**kw), "cond": cond, "need": need}


def _depth(name, dep, cond, need, T=(2, 2), **kw):
    H, W = dep.shape
    return {"name": name, "about": "depth", "rgb": filler_rgb(W, H), "dep": np.ascontiguousarray(dep.astype(np.uint16)), "T": list(T),
            "params": params(**kw), "cond": cond, "need": need}


# ------------------------------------------------------------------------------------------------------------------------------------------
# colour
# ------------------------------------------------------------------------------------------------------------------------------------------
def _half_plane_patch(theta, size=15):
    """0 / 255 half plane through the centre of a size x size patch whose normal points at angle theta"""
    r = size // 2
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return np.where(np.cos(theta) * xx + np.sin(theta) * yy > 1e-9, 255, 0).astype(np.uint8)


_sat = {}


def saturated_magnitude():
    """The largest squared gradient magnitude blurred 0 / 255 data gives, MEASURED on the oracle: blur and Sobel are linear, so the image that
    maximises the gradient along a direction is a half plane; all half planes through a pixel (720 directions, 15 x 15 patches: the support of
    Sobel after the 7 x 7 blur is 9 x 9) go through quantized_orientations and the largest magnitude at the centre is taken.  Returns (value,
    patch)."""
    if not _sat:
        best = (-1, None)
        for k in range(720):
            patch = _half_plane_patch(2 * np.pi * k / 720)
            parts = colour_parts(np.repeat(patch[..., None], 3, 2), 10.0)
            m = int(parts["mag3"][7, 7, 0])
            if m > best[0]:
                best = (m, patch)
        _sat["v"] = best
    return _sat["v"]


def sat_steps(W=96, H=64, T=(2, 2)):
    """0 / 255 only.  R: a grid of 24 x 16 blocks of bars (vertical, horizontal) and checkerboards of periods 1, 2, 5 and 7; G: step edges at
    x = 31, 32, 33 (the seam of the first two tile columns), one per band of rows, the polarity alternating; B: step edges at y = 15, 16, 17
    by band of columns.  The half plane of saturated_magnitude() is pasted once per channel, at three tile seams, with the other two
    channels saturated around it (R and B share a 32-bit lane in the kernel)."""
    yy, xx = np.mgrid[0:H, 0:W]
    R = np.zeros((H, W), np.int64)
    for by in range((H + 15) // 16):
        for bx in range((W + 23) // 24):
            p = (1, 2, 5, 7)[bx % 4]
            kind = by % 4
            sel = (yy // 16 == by) & (xx // 24 == bx)
            pat = ((xx // p) % 2, (yy // p) % 2, (xx // p + yy // p) % 2, ((xx + yy) // p) % 2)[kind]
            R = np.where(sel, 255 * pat, R)
    band = (yy * 3) // H
    G = np.where(xx >= 31 + band, 255, 0) ^ np.where(band == 1, 255, 0)
    cband = (xx * 3) // W
    B = np.where(yy >= 15 + cband, 255, 0) ^ np.where(cband == 2, 255, 0)
    rgb = np.stack([R, G, B], 2).astype(np.uint8)
    sat, patch = saturated_magnitude()
    for ch, (cx, cy) in enumerate(((32, 16), (64, 32), (48, 47))):       # centres on tile seams (x = 32, 64; y = 16, 32) and inside a tile
        if cx + 8 <= W and cy + 8 <= H:
            rgb[cy - 7:cy + 8, cx - 7:cx + 8, ch] = patch
            for other in range(3):
                if other != ch:
                    rgb[cy - 7:cy + 8, cx - 7:cx + 8, other] = 255 * ((xx[cy - 7:cy + 8, cx - 7:cx + 8] + other) % 2)

    def cond(parts):
        m3 = parts["mag3"]
        return {"saturated_pixels": int((m3.max(axis=2) == sat).sum()), "max_magnitude": int(m3.max()), "saturated_value": sat,
                "channels_saturated": int(sum((m3[..., c] == sat).any() for c in range(3)))}
    return _colour("sat_steps" if (W, H) == (96, 64) else "sat_steps_%dx%d" % (W, H), rgb, cond,
                   {"saturated_pixels": 3, "saturated_value": 200000, "channels_saturated": 3}, T)


def _tie_counts(parts):
    m3, dx3, dy3 = parts["mag3"], parts["dx3"], parts["dy3"]
    top = m3.max(axis=2)
    tied = np.zeros(top.shape, bool)
    is_top = m3 == top[..., None]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        differ = (dx3[..., a] != dx3[..., b]) | (dy3[..., a] != dy3[..., b])
        tied |= is_top[..., a] & is_top[..., b] & differ & (top > 0)
    three = is_top.all(axis=2) & tied
    inner = np.zeros(top.shape, bool)
    inner[1:-1, 1:-1] = True
    return {"tied_pixels": int((tied & inner).sum()), "three_way": int((three & inner).sum()), "two_way": int((tied & ~three & inner).sum())}


def channel_ties(W=96, H=64):
    """R a ramp in +x, G the same ramp in +y, B in -x: equal magnitudes, different (dx, dy).  Four bands of rows: all three tie; R = G with B
    flat; G = B with R flat (G must win: the first of the two); R = B with G flat."""
    yy, xx = np.mgrid[0:H, 0:W]
    ly = yy % 16
    R, G, B = 20 + 2 * xx, 20 + 2 * ly, 230 - 2 * xx
    band = yy // 16
    R = np.where(band == 2, 77, R)
    G = np.where(band == 3, 77, G)
    B = np.where(band == 1, 77, B)
    return _colour("channel_ties", np.stack([R, G, B], 2), _tie_counts, {"tied_pixels": 256, "three_way": 64, "two_way": 192}, weak_threshold=10.0)


def _at_threshold_counts(parts):
    mag, thr = parts["mag"][1:-1, 1:-1], parts["thr_sq"]
    sums = sorted({a * a + b * b for a in range(64) for b in range(a % 2, 64, 2)})       # a magnitude is dx^2 + dy^2 with dx = dy (mod 2): both are p00 + p02 + p20 + p22 plus an even number
    lo_, hi_ = np.float32(max(s for s in sums if s <= thr)), np.float32(min(s for s in sums if s > thr))
    return {"at_equality": int((mag == thr).sum()), "just_below": int((mag == lo_).sum()), "just_above": int((mag == hi_).sum()),
            "zero_magnitude": int((mag == 0).sum())}


def at_threshold(weak=4.0, seed=3, W=96, H=64, T=(2, 2)):
    """128 + U{-6 .. 6}: independent channels in the left half, one grey value in the right (so that the magnitude 0 occurs too).  weak 4.0
    puts hundreds of pixels at mag == 16 exactly; 0.0 asks for mag > 0 with pixels at 0; 3.5 (12.25) sits between the magnitudes 10 = 9 + 1 and 16 (Sobel's dx and dy have the same parity: 13 = 9 + 4 does not occur)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(-6, 7, (H, W, 3))
    n[:, W // 2:, 1] = n[:, W // 2:, 0]
    n[:, W // 2:, 2] = n[:, W // 2:, 0]
    need = {4.0: {"at_equality": 256}, 0.0: {"at_equality": 64, "zero_magnitude": 64}, 3.5: {"just_below": 64, "just_above": 64}}[weak]
    name = ("at_threshold" if weak == 4.0 else "at_threshold_weak%g" % weak) + ("" if (W, H) == (96, 64) else "_%dx%d" % (W, H))
    return _colour(name, 128 + n, _at_threshold_counts, need, T, weak_threshold=weak)


def _vote_counts(parts):
    above = parts["mag"][1:-1, 1:-1] > parts["thr_sq"]
    mv = parts["max_votes"]
    return {"four_votes": int((above & (mv == 4)).sum()), "five_votes": int((above & (mv == 5)).sum())}


def vote_edges(seed=1, W=96, H=64, T=(2, 2)):
    rng = np.random.default_rng(seed)
    name = "vote_edges" if (W, H) == (96, 64) else "vote_edges_%dx%d" % (W, H)
    return _colour(name, rng.integers(0, 256, (H, W, 3)), _vote_counts, {"four_votes": 64, "five_votes": 64}, T)


_SLOPES = ((2, 0), (-2, 0), (0, 2), (0, -2), (1, 1), (1, -1), (-1, 1), (-1, -1),          # dy == 0, dx == 0, |dx| == |dy|: the eight octant borders
           (2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (1, -2),                             # the odd labels
           (3, -1 / 3.0), (3, 1 / 3.0))                                                     # just below 360 degrees (code 16) and just above 0


def _axis_counts(parts):
    dx, dy, out = parts["dx"][1:-1, 1:-1], parts["dy"][1:-1, 1:-1], parts["out"]
    code = np.rint((parts["angle"] * np.float32(16.0 / 360.0)).astype(np.float32))[1:-1, 1:-1]
    res = {"labels": int(sum(bool((out == (1 << b)).any()) for b in range(8))), "code_16": int((code == 16).sum())}
    octants = 0
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        octants += bool(((np.sign(dx) == sx) & (np.sign(dy) == sy)).any())
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        octants += bool(((np.sign(dx) == sx) & (np.sign(dy) == sy) & (np.abs(dx) == np.abs(dy))).any())
    res["octant_borders"] = octants
    return res


def axis_and_diagonal(W=96, H=64):
    """Sixteen 24 x 16 blocks, a grey ramp a x + b y in each: Sobel after the blur gives (8 a, 8 b) exactly inside a block."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W), np.float64)
    for k, (a, b) in enumerate(_SLOPES):
        by, bx = divmod(k, 4)
        sel = (yy // 16 == by) & (xx // 24 == bx)
        img = np.where(sel, 128 + a * (xx % 24 - 12) + np.floor(b * (yy % 16 - 8)), img)
    return _colour("axis_and_diagonal", np.repeat(img[..., None], 3, 2), _axis_counts, {"labels": 8, "code_16": 16, "octant_borders": 8})


def _all_zero(parts):
    return {"nonzero_outputs": int((parts["out"] != 0).sum()), "nonzero_magnitudes": int((parts["mag"] != 0).sum())}


def constant(value, W=96, H=64):
    c = _colour("constant_%d" % value, np.full((H, W, 3), value), _all_zero, {})
    c["exact"] = {"nonzero_outputs": 0, "nonzero_magnitudes": 0}
    return c


def tiny(W, H, T, seed=5):
    """the smallest frames: uniform noise over a steep depth plane (the normals' interior is [5, W - 6] x [5, H - 6]: 5 x 5 pixels at 16 x 16)"""
    rng = np.random.default_rng(seed)
    c = _colour("tiny_%dx%d" % (W, H), rng.integers(0, 256, (H, W, 3)), lambda parts: {"outputs": int((parts["out"] != 0).sum())}, {"outputs": 1}, T)
    yy, xx = np.mgrid[0:H, 0:W]
    c["dep"] = (500 + 7 * xx - 3 * yy + rng.integers(0, 3, (H, W))).astype(np.uint16)
    return c


def colour_cases():
    return [sat_steps(), sat_steps(100, 96), channel_ties(), at_threshold(4.0), at_threshold(0.0), at_threshold(3.5), vote_edges(),
            vote_edges(2, 1280, 32), axis_and_diagonal(), constant(0), constant(255), constant(128),
            tiny(16, 16, (2,)), tiny(24, 16, (2, 2)), tiny(32, 16, (2, 2)), at_threshold(4.0, 3, 160, 128, (4, 8))]


# ------------------------------------------------------------------------------------------------------------------------------------------
# depth
# ------------------------------------------------------------------------------------------------------------------------------------------
def _steep_counts(diff):
    def cond(parts):
        ad = np.abs(parts["deltas"])
        cnt = parts["counted"].astype(bool)
        return {"largest_counted_is_diff_minus_1": int(((np.where(cnt, ad, -1).max(axis=0) == diff - 1) & cnt.all(axis=0)).sum()),
                "a_delta_equal_to_diff": int((ad == diff).any(axis=0).sum()), "all_eight_taps": int(cnt.all(axis=0).sum())}
    return cond


def steep_planes(diff, W=96, H=64, T=(2, 2)):
    """Four quadrants, the four sign combinations of a plane over the 5-pixel grid the taps sample: depth = m1 sx (x // 5) + m2 sy (y // 5), so
    that a tap's delta is exactly +-m1, +-m2, +-(m1 + m2) or +-(m1 - m2) at every pixel.  In the left half of a quadrant m1 + m2 = diff - 1
    (all eight taps count, the largest |delta| one below the threshold), in the right half m1 + m2 = diff (the two diagonal taps fall out
    at equality).  A 16-bit frame cannot reach diff = 70000: there the slope is capped and every tap counts."""
    yy, xx = np.mgrid[0:H, 0:W]
    gx, gy = xx // 5, yy // 5
    dep = np.zeros((H, W), np.int64)
    for qy in range(2):
        for qx in range(2):
            for half in range(2):
                tot = min(diff - 1 + half, 600 + half)
                m1 = tot // 2
                m2 = tot - m1
                sel = (yy * 2 // H == qy) & (xx * 2 // W == qx) & (((xx % (W // 2)) * 2 // (W // 2)) == half)
                plane = (1 - 2 * qx) * m1 * gx + (1 - 2 * qy) * m2 * gy
                dep = np.where(sel, plane - plane[sel].min() + 1000, dep)
    need = {"all_eight_taps": 64}
    if diff <= 601:
        need.update({"largest_counted_is_diff_minus_1": 64, "a_delta_equal_to_diff": 64})
    name = "steep_planes" if (W, H) == (96, 64) else "steep_planes_%dx%d" % (W, H)
    return _depth("%s_diff%d" % (name, diff), dep, _steep_counts(diff), need, T, difference_threshold=diff, distance_threshold=65536)


def steep_planes_29(diff):
    """1000 + 29 x + 29 y and the three other sign combinations, one per quadrant: the axis taps differ by +-145, the diagonal ones by 0 or
    +-290."""
    W, H = 96, 64
    yy, xx = np.mgrid[0:H, 0:W]
    dep = np.zeros((H, W), np.int64)
    for qy in range(2):
        for qx in range(2):
            sel = (yy * 2 // H == qy) & (xx * 2 // W == qx)
            plane = (1 - 2 * qx) * 29 * xx + (1 - 2 * qy) * 29 * yy
            dep = np.where(sel, plane - plane[sel].min() + 1000, dep)

    def cond(parts):
        ad, cnt = np.abs(parts["deltas"]), parts["counted"].astype(bool)
        return {"counted_145": int(((ad == 145) & cnt).any(axis=0).sum()), "deltas_145": int((ad == 145).any(axis=0).sum())}
    need = {"deltas_145": 256}
    if diff > 145:
        need["counted_145"] = 256
    return _depth("steep_planes_29_diff%d" % diff, dep, cond, need, difference_threshold=diff, distance_threshold=65536)


def tap_extremes(diff):
    """Brute force over the 256 subsets of counted taps and the signs of their deltas (+-(diff - 1): ddx and ddy are linear in the deltas, so
    their extremes lie there).  Python integers.  Returns {"ddx": (max |1150 ddx|, subset mask, deltas), "ddy": ...}."""
    best = {"ddx": (-1, 0, None), "ddy": (-1, 0, None)}
    for mask in range(256):
        S = [k for k in range(8) if mask >> k & 1]
        A0 = sum(TAPS[k][0] * TAPS[k][0] for k in S)
        A1 = sum(TAPS[k][0] * TAPS[k][1] for k in S)
        A3 = sum(TAPS[k][1] * TAPS[k][1] for k in S)
        for key, coef in (("ddx", [A3 * TAPS[k][0] - A1 * TAPS[k][1] for k in range(8)]), ("ddy", [-A1 * TAPS[k][0] + A0 * TAPS[k][1] for k in range(8)])):
            deltas = [((diff - 1) if coef[k] >= 0 else -(diff - 1)) if k in S else None for k in range(8)]
            v = 1150 * sum(coef[k] * deltas[k] for k in S)
            assert v >= 0
            if v > best[key][0]:
                best[key] = (v, mask, deltas)
    return best


def tap_subsets(diff):
    """320 x 240, centre depth 30000.  A lattice of centres 11 pixels apart (their taps, 5 away, never coincide with another centre or its
    taps): centre n < 256 has exactly the taps of subset n counted, at +-(diff - 1) with the signs that maximise |ddx|, centre 256 + n the same
    for |ddy|; a tap outside the subset lies 1000 deeper.  Below the lattice, a band of straight depth steps of diff - 1 every 7 columns
    and every 3 rows (the subsets half planes reach)."""
    W, H = 320, 240
    assert diff - 1 < 1000
    dep = np.full((H, W), 30000, np.int64)
    centres = [(5 + 11 * cx, 5 + 11 * cy) for cy in range(20) for cx in range(28)]
    for n in range(512):
        x, y = centres[n]
        mask = n & 255
        S = [k for k in range(8) if mask >> k & 1]
        A0 = sum(TAPS[k][0] ** 2 for k in S); A1 = sum(TAPS[k][0] * TAPS[k][1] for k in S); A3 = sum(TAPS[k][1] ** 2 for k in S)
        for k, (i, j) in enumerate(TAPS):
            coef = (A3 * i - A1 * j) if n < 256 else (-A1 * i + A0 * j)
            dep[y + j, x + i] = 30000 + (((diff - 1) if coef >= 0 else -(diff - 1)) if k in S else 1000)
    yy, xx = np.mgrid[0:H, 0:W]
    dep = np.where(yy >= 221, 30000 + (diff - 1) * (xx // 7) + (diff - 1) * ((yy - 221) // 3), dep)
    ext = tap_extremes(diff)

    def cond(parts):
        subsets = set()
        cnt = parts["counted"]
        code = sum(cnt[k] << k for k in range(8))
        for n in range(512):
            x, y = centres[n]
            subsets.add(int(code[y - 5, x - 5]) if n < 256 else -1)
        return {"max_1150_ddx": int(np.abs(1150 * parts["ddx"]).max()), "max_1150_ddy": int(np.abs(1150 * parts["ddy"]).max()),
                "brute_force_ddx": ext["ddx"][0], "brute_force_ddy": ext["ddy"][0], "subsets_planted": len(subsets - {-1}),
                "max_det_times_depth": int(np.abs(parts["det"] * parts["c"]).max())}
    c = _depth("tap_subsets_diff%d" % diff, dep, cond, {"subsets_planted": 256}, (4, 8), difference_threshold=diff, distance_threshold=65536)
    c["equal"] = (("max_1150_ddx", "brute_force_ddx"), ("max_1150_ddy", "brute_force_ddy"))
    return c


def _near_zero_counts(parts):
    c, cnt, valid = parts["c"], parts["counted"].astype(bool), parts["valid"]
    return {"zero_centres_with_a_counted_tap": int(((c == 0) & cnt.any(axis=0)).sum()),
            "index_of_20": int((valid & ((parts["v1"] == 20) | (parts["v2"] == 20))).sum()),
            "zero_centres_with_a_normal": int(((c == 0) & (parts["raw"][5:-6, 5:-6] != 0)).sum())}


def near_zero(diff, W=96, H=64, T=(2, 2)):
    """depths 0 .. 49: (3 x + 2 y) % 50 in the upper half, a seeded draw from 0 .. 49 with every fifth pixel 0 in the lower.  A centre of depth
    0 has nz = 0, so nx or ny reaches +-1 where the other vanishes and the table index becomes 20 (the next row of the flat table)."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    dep = (3 * xx + 2 * yy) % 50
    noise = rng.integers(0, 50, (H, W)) * (rng.integers(0, 5, (H, W)) > 0)
    dep = np.where(yy >= H // 2, noise, dep)
    dep = np.where((yy >= 3 * H // 4) & (xx % 5 != 0), 7 * (xx // 5) % 50, dep)            # columns of constant depth: ddy == 0 exactly ...
    dep = np.where((yy >= 3 * H // 4) & (xx % 10 == 0), 0, dep)                            # ... around centres of depth 0
    need = {"zero_centres_with_a_counted_tap": 64}
    if diff >= 49:
        need.update({"index_of_20": 1, "zero_centres_with_a_normal": 16})
    name = "near_zero" if (W, H) == (96, 64) else "near_zero_%dx%d" % (W, H)
    return _depth("%s_diff%d" % (name, diff), dep, _near_zero_counts, need, T, difference_threshold=diff)


def extremes(diff, dist):
    """{0, 1, 30000, 65534, 65535} drawn per pixel (columns 32 ..), and a block that is 65535 with one pixel in ten 65534 (columns .. 31: all
    taps count at the largest centre depth, det * d = 22500 * 65535).  At diff = 70000 every tap counts and 1150 ddx leaves 32 bits."""
    W, H = 96, 64
    rng = np.random.default_rng(21)
    dep = np.array([0, 1, 30000, 65534, 65535])[rng.integers(0, 5, (H, W))]
    block = np.where(rng.integers(0, 10, (H, W)) == 0, 65534, 65535)
    dep = np.where(np.mgrid[0:H, 0:W][1] < 32, block, dep)

    def cond(parts):
        proc = parts["c"] < dist
        return {"max_1150_ddx": int(np.abs(1150 * parts["ddx"]).max()), "max_det_times_depth": int(np.abs(parts["det"] * parts["c"]).max()),
                "processed": int(proc.sum()), "normals": int((parts["raw"] != 0).sum())}
    need = {}
    if diff == 70000:
        need["max_1150_ddx"] = 2 ** 31 + 1
    if diff >= 49 and diff <= 151:
        need["max_det_times_depth"] = 2 ** 30                # (22500 * 65535 = 1 474 537 500: inside 32 bits, past 2^30)
    c = _depth("extremes_diff%d_dist%d" % (diff, dist), dep, cond, need, difference_threshold=diff, distance_threshold=dist)
    if dist == 0:
        c["exact"] = {"processed": 0, "normals": 0}
    return c


def distance_edge(diff, dist=2000):
    """a plane across distance_threshold: column 47 is dist - 1 (processed), column 48 is dist (not)"""
    W, H = 96, 64
    yy, xx = np.mgrid[0:H, 0:W]
    dep = dist - 48 + xx + (yy % 2)
    dep = np.where(yy % 2 == 1, dep - 1, dep)

    def cond(parts):
        c, raw = parts["c"], parts["raw"][5:-6, 5:-6]
        return {"at_dist_minus_1": int((c == dist - 1).sum()), "at_dist": int((c == dist).sum()),
                "normals_at_dist_minus_1": int(((c == dist - 1) & (raw != 0)).sum()), "normals_at_dist": int(((c >= dist) & (raw != 0)).sum())}
    c = _depth("distance_edge_diff%d_dist%d" % (diff, dist), dep, cond, {"at_dist_minus_1": 32, "at_dist": 32, "normals_at_dist_minus_1": 32 if diff > 1 else 0},
               difference_threshold=diff, distance_threshold=dist)
    c["exact"] = {"normals_at_dist": 0}
    return c


def collinear(diff):
    """Upper half: depth jumps by 1000 every 3 columns and slopes 7 per row — only the taps (0, +-5) count, A0 = A1 = 0, det = 0.  Lower half:
    the same with rows and columns exchanged — only (+-5, 0) count."""
    W, H = 96, 64
    yy, xx = np.mgrid[0:H, 0:W]
    dep = np.where(yy < H // 2, 1000 + 1000 * (xx // 3) + 7 * yy, 1000 + 1000 * (yy // 3) + 7 * xx)

    def cond(parts):
        cnt = parts["counted"].astype(bool)
        only_v = cnt[1] & cnt[6] & ~(cnt[0] | cnt[2] | cnt[3] | cnt[4] | cnt[5] | cnt[7])
        only_h = cnt[3] & cnt[4] & ~(cnt[0] | cnt[1] | cnt[2] | cnt[5] | cnt[6] | cnt[7])
        return {"only_vertical_taps": int(only_v.sum()), "only_horizontal_taps": int(only_h.sum()),
                "det_zero_with_taps": int(((parts["det"] == 0) & cnt.any(axis=0)).sum()), "normals_there": int(((only_v | only_h) & (parts["raw"][5:-6, 5:-6] != 0)).sum())}
    need = {"only_vertical_taps": 64, "only_horizontal_taps": 64, "det_zero_with_taps": 128} if 36 <= diff <= 1000 else {}
    c = _depth("collinear_diff%d" % diff, dep, cond, need, difference_threshold=diff, distance_threshold=65536)
    c["exact"] = {"normals_there": 0}
    return c


def depth_cases():
    out = []
    for diff in DIFFS:
        out += [steep_planes(diff), steep_planes_29(diff), near_zero(diff), distance_edge(diff), collinear(diff)]
        out += [extremes(diff, dist) for dist in (65536, 65535, 1, 0)]
    out += [tap_subsets(150), tap_subsets(151), steep_planes(150, 100, 96), near_zero(50, 100, 96), distance_edge(50, 1000),
            near_zero(49, 160, 128, (4, 8))]
    return out


_all = {}


def all_cases():
    """name -> case, built once per process and never modified"""
    if not _all:
        for c in colour_cases() + depth_cases():
            assert c["name"] not in _all, c["name"]
            _all[c["name"]] = c
    return _all


def check_conditions(c, parts=None):
    """the case's counts, asserted: need = minimum, exact = the value itself, equal = pairs of counts that must agree"""
    counts = c["cond"](case_parts(c) if parts is None else parts)
    for k, v in c["need"].items():
        assert counts[k] >= v, (c["name"], k, counts[k], ">=", v)
    for k, v in c.get("exact", {}).items():
        assert counts[k] == v, (c["name"], k, counts[k], "==", v)
    for a, b in c.get("equal", ()):
        assert counts[a] == counts[b], (c["name"], a, counts[a], b, counts[b])
    return counts
