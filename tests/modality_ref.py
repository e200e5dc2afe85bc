"""A detector with ONE modality, stated through the two-slot oracle (oracle/linemod_oracle.py, unchanged): the present modality sits in
slot 0, slot 1 is empty — an all-zero quantised map and templates without features.  match_oracle.c sums nf over both slots for the
denominator, takes its 8-/16-bit mode and the clamp sizes from slot 0 and adds zeros for a slot without features, which is what the reference's
matchClass does over a modality list of one (LL.cpp:1788-1941).  Only public functions of the oracle are used."""
import functools

import numpy as np

import linemod_oracle as lo
import synth

SETS = (("ColorGradient",), ("DepthNormal",))
KIND = {"ColorGradient": 0, "DepthNormal": 1}


def present_maps(pyr, kind, masked=False):
    """Per level the quantised map of modality `kind` out of OracleDetector.quantize_pyramid's tuples (qc, qn, mag, ang, normal, msk)."""
    return [np.ascontiguousarray(p[kind] if masked else p[3 + kind]) for p in pyr]


def linear_memories(maps, T, build=lo.build_linear_memories):
    """(lms[level] = [present, empty], sizes[level] = (W, H)); `build(map, T)` may be another table's builder (response_table_ref)."""
    lms = [[build(m, T[l]), build(np.zeros_like(m), T[l])] for l, m in enumerate(maps)]
    return lms, [(m.shape[1], m.shape[0]) for m in maps]


def empty_like(t):
    return lo.Template(t.width, t.height, t.pyramid_level, np.zeros((0, 3), np.int32))


def two_slot(pyramids):
    """[t_l0, t_l1, ...] per pyramid -> [t_l0, empty, t_l1, empty, ...]: the oracle's levels x 2 layout."""
    return [[s for t in tp for s in (t, empty_like(t))] for tp in pyramids]


def pack_single(pyramids):
    """(features, tmpl_offsets, tmpl_wh) of levels x 1 templates per pyramid: what addClassPacked of a one-modality detector takes."""
    feats = [np.asarray(t.features, np.int32).reshape(-1, 3) for tp in pyramids for t in tp]
    offs = np.zeros(len(feats) + 1, np.int32)
    offs[1:] = np.cumsum([len(f) for f in feats])
    wh = np.asarray([(t.width, t.height) for tp in pyramids for t in tp], np.int32).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate(feats, 0), np.int32), offs, wh


def oracle_match(pyramids, T, lms, sizes, threshold):
    """(raw records, canonical list, statistics) of the single class "obj" through OracleDetector.match_raw."""
    od = lo.OracleDetector(63, list(T))
    od.class_templates["obj"] = two_slot(pyramids)
    raw = od.match_raw(lms, sizes, threshold, ["obj"])
    return raw, lo.canonical_sort_unique(raw), dict(od.last_stats)


def multiset(raw):
    return sorted(zip(raw["x"].tolist(), raw["y"].tolist(), raw["sim"].tolist(), raw["tid"].tolist()))


def gpu_multiset(recs):
    return sorted(zip(recs["x"].tolist(), recs["y"].tolist(), recs["similarity"].tolist(), recs["template_id"].tolist()))


def crop(levels_feats):
    """cropTemplates over the templates of ONE modality: levels_feats[l] = (n, 3) absolute x, y, label at level l."""
    tp = [lo.Template(-1, -1, l, np.asarray(f, np.int32).reshape(-1, 3)) for l, f in enumerate(levels_feats)]
    lo.crop_templates(tp)
    return tp


def make_bank(seed, n_planted, n_random, maps, T, nf0, label_noise=0.12):
    """n_planted templates cut out of the present modality's quantised maps (a fraction of the labels re-drawn) and n_random ones with uniform
    features, nf0 >> l features at level l.  cropTemplates leaves one feature at x == width and one at y == height (max - min is the size),
    the positions whose 16-byte reads run past their phase row; asserted below."""
    rng = np.random.default_rng(seed)
    H0, W0 = maps[0].shape
    L = len(maps)
    labs = [np.where(q > 0, np.log2(np.maximum(q, 1)).astype(np.int32), -1) for q in maps]
    border = 8 * T[0] + 2
    out, guard = [], 0
    while len(out) < n_planted:
        guard += 1
        if guard > 200 * n_planted + 1000:
            raise RuntimeError("could not plant templates: quantised maps too sparse")
        w = int(rng.integers(40, max(41, min(100, W0 - 2 * border - 2))))
        h = int(rng.integers(40, max(41, min(100, H0 - 2 * border - 2))))
        x0 = int(rng.integers(border, max(border + 1, W0 - w - border))) & ~1
        y0 = int(rng.integers(border, max(border + 1, H0 - h - border))) & ~1
        lv = []
        for l in range(L):
            nf = nf0 >> l
            xl, yl, wl, hl = x0 >> l, y0 >> l, max(2, w >> l), max(2, h >> l)
            box = labs[l][yl:yl + hl + 1, xl:xl + wl + 1]
            ys, xs = np.nonzero(box >= 0)
            if len(ys) < nf:
                break
            sel = rng.choice(len(ys), nf, replace=False)
            lab = box[ys[sel], xs[sel]].copy()
            flip = rng.uniform(0, 1, nf) < label_noise
            lab[flip] = rng.integers(0, 8, int(flip.sum()))
            lv.append(np.stack([xs[sel] + xl, ys[sel] + yl, lab], 1))
        if len(lv) == L:
            out.append(crop(lv))
    for _ in range(n_random):
        w, h = int(rng.integers(24, 90)), int(rng.integers(24, 90))
        lv = []
        for l in range(L):
            nf, wl, hl = nf0 >> l, max(2, w >> l), max(2, h >> l)
            lv.append(np.stack([rng.integers(0, wl + 1, nf), rng.integers(0, hl + 1, nf), rng.integers(0, 8, nf)], 1))
        out.append(crop(lv))
    for tp in out:                                           # (the extreme feature may sit at any level: the box spans the whole pyramid)
        assert any(t.features[:, 0].max() == t.width for t in tp) and any(t.features[:, 1].max() == t.height for t in tp), "cropTemplates invariant"
    return out


def train_expect(od, rgb, depth, mask, kind):
    """Detector::addTemplate of a one-modality detector (LL.cpp:1943-1975): quantize_pyramid, the present modality's extractTemplate per level
    with num_features (and the normals' extract_threshold) halved per level, cropTemplates over the present templates only.  None = -1."""
    pyr = od.quantize_pyramid(rgb, depth, mask)
    nf, ext = od.num_features, od.extract_threshold
    tp = []
    for l, (qc, qn, mag, ang, normal, msk) in enumerate(pyr):
        if l > 0:
            nf //= 2
            ext //= 2
        t = lo.extract_color_template(mag, ang, msk, nf, od.strong_threshold, l) if kind == 0 else \
            lo.extract_normal_template(normal, msk, nf, ext, l)
        if t is None:
            return None
        tp.append(t)
    lo.crop_templates(tp)
    return tp


def same_templates(got, want):
    """getTemplates of the detector against a list of oracle Templates, element for element."""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert (g.width, g.height, g.pyramid_level) == (w.width, w.height, w.pyramid_level), ((g.width, g.height), (w.width, w.height))
        assert np.array_equal(np.asarray(g.features, np.int32).reshape(-1, 3), np.asarray(w.features, np.int32).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def scene(W, H, T, seed=7, n_poly=14):
    """frame, oracle detector and quantised pyramid of a geometry (computed once per process, never modified)."""
    rgb, dep = synth.make_frame(seed, W, H, n_poly)
    od = lo.OracleDetector(63, list(T))
    return {"rgb": rgb, "dep": dep, "od": od, "pyr": od.quantize_pyramid(rgb, dep), "T": list(T)}


def view(seed, W=208, H=176, flat_depth=False, flat_colour=False, colour_quadrant=False):
    """A synthetic training view: a textured, bumpy ellipse on a plain background, its depth and its two-valued mask.  flat_depth: no depth
    anywhere, what a colour camera delivers (no normals: DepthNormal finds no features); flat_colour: a uniform image (ColorGradient finds none);
    colour_quadrant: only the lower right quarter of the object differs from the background in colour, so the colour features (on the
    mask's rim, where the gradient is strong) cover a quarter of the box the normal features span."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy, a, b = W / 2 + rng.uniform(-6, 6), H / 2 + rng.uniform(-6, 6), rng.uniform(44, 60), rng.uniform(36, 50)
    r2 = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2
    inside = r2 < 1
    depth = 900.0 - 140.0 * np.sqrt(np.clip(1 - r2, 0, None)) + 10.0 * np.sin(xx / 6.0) * np.cos(yy / 5.0)
    depth = np.where(inside & (not flat_depth), depth, 0).astype(np.uint16)
    rgb = np.full((H, W, 3), 30, np.uint8)
    if not flat_colour:
        tex = np.stack([128 + 90 * np.sin(xx / (5 + c) + seed) * np.cos(yy / (7 - c)) for c in range(3)], 2)
        shown = inside & (xx > cx) & (yy > cy) if colour_quadrant else inside
        rgb = np.where(shown[..., None], tex, 30).clip(0, 255).astype(np.uint8)
    return np.ascontiguousarray(rgb), np.ascontiguousarray(depth), (inside * 255).astype(np.uint8)
