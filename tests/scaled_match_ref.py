"""Depth-scaled matching (Detector.matchScaled; match_scaled.hip) stated in numpy.  This file is the definition; the
kernels are held to it record for record.

It is the holistic rule of part_match_ref.match_parts(min_parts=0) — the same positions, thresholds, windows, clamps, first-maximum arg-max and
position updates, which that file pins to LL.cpp:1835-1938 — with one change: where a feature is sampled.
  1. Probe.  P = the smallest non-zero depth of the (2 probe + 1)^2 window of level-0 pixels around a pixel, clipped to the frame; 0 if none.
  2. Top level, entry (pyramid, L - 1) of box (w, h), step T, Wd = W / T: every cell (i, j) whose raster position lies below the template's
     position count (`limit` of part_match_ref.coarse_parts, of the unscaled box) is looked at; d = P at the level-0 pixel
     ((i T + w // 2) << (L - 1), (j T + h // 2) << (L - 1)) clamped into the frame; no candidate if d = 0, d_train 1024 < min d or
     d_train 1024 > max d; else k = argmin |s_k d - d_train 1024| (integers; a tie to the lower k), carried unchanged through the lower levels.
  3. Scaled features of an entry with centre c = (w // 2, h // 2): sx = cx + sign(fx - cx) ((|fx - cx| s_k + 512) >> 10), sy alike; labels,
     count and denominator unchanged; coinciding features count twice.  The response at a position origin (ox, oy), a multiple of T, is
     LM[label][(py mod T) T + px mod T][(py // T) Wd + px // T] at (px, py) = (ox + sx, oy + sy), floor mod and //, and 0 when px // T lies outside
     [0, Wd) or py // T outside [0, Hd): no wrap into the next row or memory (the one departure from the reference's reads).
  4. Candidates iff (raw 100.f) / (4 nf) > threshold in float32; the levels below as match_parts(min_parts=0) with the level's own entry scaled by k.
  5. Records (x, y, similarity, class_index, template_id, scale_index, depth_mm), x, y, similarity of the unscaled convention; exact duplicates
     removed; ordered by similarity descending, then class_index, template_id, y, x, scale_index (and depth_mm) ascending."""
import numpy as np

import part_match_ref as pm

F32 = np.float32
DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("similarity", np.float32), ("class_index", np.int32), ("template_id", np.int32),
                  ("scale_index", np.int32), ("depth_mm", np.int32)])
FIELDS = list(DTYPE.names)


def q10(scale):
    """floor(1024 scale + 0.5): the rounding of lm_detector.scale_q10"""
    return int(np.floor(1024.0 * float(scale) + 0.5))


def scale_coord(v, c, s):
    dv = np.asarray(v, np.int64) - int(c)
    return int(c) + np.sign(dv) * ((np.abs(dv) * int(s) + 512) >> 10)


def scaled_features(width, height, xs, ys, s):
    """what lm_scaled_features returns"""
    return scale_coord(xs, width // 2, s), scale_coord(ys, height // 2, s)


def probe_map(depth, probe):
    """min non-zero over the clipped (2 probe + 1)^2 window; 0 where the window holds none"""
    H, W = depth.shape
    big = np.where(depth == 0, 1 << 20, depth.astype(np.int64))
    pad = np.full((H + 2 * probe, W + 2 * probe), 1 << 20, np.int64)
    pad[probe:probe + H, probe:probe + W] = big
    out = np.full((H, W), 1 << 20, np.int64)
    for dy in range(2 * probe + 1):
        for dx in range(2 * probe + 1):
            out = np.minimum(out, pad[dy:dy + H, dx:dx + W])
    return np.where(out == 1 << 20, 0, out).astype(np.int64)


def select_scale(d, d_train, scales, lo=None, hi=None):
    """k per probed depth (int64 array), -1: no candidate.  Python-int exact for the ranges used (|s d - 1024 d_train| < 2^63)."""
    d = np.asarray(d, np.int64)
    lo = scales[0] if lo is None else lo
    hi = scales[-1] if hi is None else hi
    t = int(d_train) * 1024
    err = np.stack([np.abs(int(s) * d - t) for s in scales], 0)
    k = err.argmin(0)                                                                   # the first minimum: a tie goes to the lower entry
    ok = (d != 0) & ~(t < lo * d) & ~(t > hi * d)
    return np.where(ok, k, -1)


def sample(lms, F, sx, sy, T, Wd, Hd, ci, cj):
    """sum over the features of the responses at the position cells (ci, cj) (arrays of one shape): LM of step 3"""
    ci, cj = np.asarray(ci, np.int64), np.asarray(cj, np.int64)
    total = np.zeros(ci.shape, np.int64)
    for f in range(len(F)):
        px, py = ci * T + int(sx[f]), cj * T + int(sy[f])
        cx, cy = px // T, py // T
        ok = (cx >= 0) & (cx < Wd) & (cy >= 0) & (cy < Hd)
        idx = (int(F[f, 2]) * T * T + (py % T) * T + px % T) * (Wd * Hd) + cy * Wd + cx
        total += np.where(ok, lms[int(F[f, 3])][np.where(ok, idx, 0)], 0)
    return total


def coarse(bank, p, lms, sizes, T, P0, d_train, scales, lo, hi):
    """top level of pyramid p: (positions, k, d, raw) of every cell looked at with a scale (k >= 0)"""
    L = len(T)
    F, w, h = pm.entry_of(bank, p, L - 1, L)
    Wt, Ht = sizes[L - 1]
    Tt = T[L - 1]
    Wd, Hd = Wt // Tt, Ht // Tt
    wf, hf = (w - 1) // Tt + 1, (h - 1) // Tt + 1
    limit = max(0, min((Hd - hf) * Wd + (Wd - wf) + 1, Wd * Hd))
    pos = np.arange(limit, dtype=np.int64)
    i, j = pos % Wd, pos // Wd
    H0, W0 = P0.shape
    px = np.clip((i * Tt + w // 2) << (L - 1), 0, W0 - 1)
    py = np.clip((j * Tt + h // 2) << (L - 1), 0, H0 - 1)
    d = P0[py, px]
    k = select_scale(d, d_train, scales, lo, hi)
    raw = np.zeros(limit, np.int64)
    for q in range(len(scales)):
        sel = np.nonzero(k == q)[0]
        if len(sel):
            sx, sy = scaled_features(w, h, F[:, 0], F[:, 1], scales[q])
            raw[sel] = sample(lms[L - 1], F, sx, sy, Tt, Wd, Hd, i[sel], j[sel])
    keep = k >= 0
    return pos[keep], k[keep], d[keep], raw[keep], len(F)


def match_scaled(bank, lms, sizes, T, threshold, depth0, d_train, scales, lo=None, hi=None, probe=2, cls=0, stats=None):
    """Raw records (DTYPE, before duplicate removal and ordering) of a packed bank on a frame whose level-0 depth image is depth0."""
    feat, offs, wh = bank
    L = len(T)
    NP = (len(offs) - 1) // (2 * L)
    thr = F32(threshold)
    P0 = probe_map(np.asarray(depth0), probe)
    out = []
    ncand = 0
    for p in range(NP):
        pos, k, d, raw, nf = coarse(bank, p, lms, sizes, T, P0, d_train, scales, lo, hi)
        Tt = T[L - 1]
        Wd = sizes[L - 1][0] // Tt
        sim = pm.score_of(raw, nf)
        hit = sim > thr
        pos, k, d, sim = pos[hit], k[hit], d[hit], sim[hit]
        ncand += len(pos)
        off = Tt // 2 + (Tt % 2 - 1)
        cx, cy = (pos % Wd) * Tt + off, (pos // Wd) * Tt + off
        for l in range(L - 2, -1, -1):
            if len(cx) == 0:
                break
            F, w, h = pm.entry_of(bank, p, l, L)
            Wl, Hl = sizes[l]
            Tl = T[l]
            Wdl, Hdl = Wl // Tl, Hl // Tl
            border, offset = 8 * Tl, Tl // 2 + (Tl % 2 - 1)
            x = np.minimum(np.maximum(cx * 2 + 1, border), Wl - w - border)
            y = np.minimum(np.maximum(cy * 2 + 1, border), Hl - h - border)
            gx, gy = x // Tl - 8, y // Tl - 8
            total = np.zeros((len(x), 256), np.int64)
            wr, wc = np.divmod(np.arange(256), 16)
            for q in range(len(scales)):
                sel = np.nonzero(k == q)[0]
                if len(sel) == 0:
                    continue
                sx, sy = scaled_features(w, h, F[:, 0], F[:, 1], scales[q])
                total[sel] = sample(lms[l], F, sx, sy, Tl, Wdl, Hdl, gx[sel, None] + wc[None, :], gy[sel, None] + wr[None, :])
            best = total.argmax(1)
            rawmax = total[np.arange(len(x)), best]
            br, bc = np.where(rawmax > 0, best // 16, -1), np.where(rawmax > 0, best % 16, -1)
            sim = np.where(rawmax > 0, pm.score_of(rawmax, len(F)), F32(0)).astype(F32)
            cx, cy = (gx + bc) * Tl + offset, (gy + br) * Tl + offset
            keep = ~(sim < thr)
            cx, cy, sim, k, d = cx[keep], cy[keep], sim[keep], k[keep], d[keep]
        rec = np.zeros(len(cx), DTYPE)
        rec["x"], rec["y"], rec["similarity"], rec["class_index"], rec["template_id"], rec["scale_index"], rec["depth_mm"] = cx, cy, sim, cls, p, k, d
        out.append(rec)
    if stats is not None:
        stats["candidates"] = stats.get("candidates", 0) + ncand
    return np.concatenate(out) if out else np.zeros(0, DTYPE)


def match_classes(banks, d_train, selection, lms, sizes, T, threshold, depth0, scales, lo=None, hi=None, probe=2, stats=None):
    """match_scaled once per listed class — `selection` as the caller gives it: unknown names are skipped and keep their position, a repeated
    name is matched again; an empty selection is every class in the order of its name — with class_index = the position in the list and that
    class's own training depth; the raw records concatenated.  banks and d_train: name -> packed bank / mm."""
    out = []
    for pos, name in enumerate(selection if len(selection) else sorted(banks)):
        if name in banks:
            out.append(match_scaled(banks[name], lms, sizes, T, threshold, depth0, d_train[name], scales, lo, hi, probe, cls=pos, stats=stats))
    return np.concatenate(out) if out else np.zeros(0, DTYPE)


def canonical(rec):
    """exact duplicates removed; similarity descending, then class_index, template_id, y, x, scale_index, depth_mm ascending"""
    if len(rec) == 0:
        return rec.copy()
    rec = np.unique(rec)
    order = np.lexsort((rec["depth_mm"], rec["scale_index"], rec["x"], rec["y"], rec["template_id"], rec["class_index"], -rec["similarity"].astype(np.float64)))
    return rec[order]


def rows(rec):
    return [tuple(r) for r in rec[FIELDS].tolist()]
