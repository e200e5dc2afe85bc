"""Part-based matching (Detector.setPartMatching; match_parts.hip) stated in numpy.  This file is the definition;
the kernels are held to it record for record.

An entry is one (template pyramid, level): width, height and the nf features of both modalities.
  1. Parts.  A feature at (x, y) belongs to part p = (2x >= width) + 2 (2y >= height); both modalities are pooled; n_p = the part's feature
     count; a part is eligible iff n_p >= min_part_features.
  2. Top level.  For a position below the template's position count (LL.cpp:1299-1309): raw_p = the part's response sum; a part passes iff it
     is eligible and (raw_p * 100.f) / (4 * n_p) > threshold (float32, LL.cpp:1842-1844); the position is a candidate iff at least min_parts
     parts pass; its score is the holistic (sum_p raw_p * 100.f) / (4 * nf); positions in raster order.
  3. Levels below.  Window, clamp, arg-max (first maximum of the holistic sum in raster order) and position update as the reference
     (LL.cpp:1871-1931); sim = the holistic score; the candidate stays iff at least min_parts eligible parts have
     (raw_p at the arg-max position * 100.f) / (4 * n_p) >= threshold.  With raw <= 0 the part sums are 0 (they are: sums are not negative).
  4. Records: (x, y, holistic score at level 0, class, template).
min_parts = 0 states the holistic rule with the same machinery (score > threshold at the top, sim < threshold drops below): the tests hold
that to the oracle (match_oracle.c), which pins windows, clamps and arg-max of this file to the reference's lines."""
import numpy as np

import linemod_oracle as lo

F32 = np.float32


def part_of(x, y, width, height):
    return (2 * np.asarray(x) >= width).astype(np.int64) + 2 * (2 * np.asarray(y) >= height).astype(np.int64)


def part_table(width, height, xs, ys, min_part_features):
    """What lm_part_table returns: start[4], n[4], npad[4] (a multiple of 8), eligible[4], and per slot the feature's index (-1: padding)."""
    p = part_of(xs, ys, width, height) if len(xs) else np.zeros(0, np.int64)
    n = np.array([(p == k).sum() for k in range(4)], np.int64)
    npad = (n + 7) // 8 * 8
    start = np.concatenate([[0], np.cumsum(npad)[:-1]])
    order = -np.ones(int(npad.sum()), np.int64)
    for k in range(4):
        idx = np.nonzero(p == k)[0]
        order[start[k]:start[k] + len(idx)] = idx
    return {"start": start, "n": n, "npad": npad, "eligible": (n >= min_part_features).astype(np.int64), "order": order}


def score_of(raw, n):
    """(raw * 100.f) / (4 * n) in float32, elementwise (n = 0: nan, which passes no comparison)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(raw).astype(F32) * F32(100.0)) / F32(4 * int(n))


def entry_of(bank, pyramid, level, L):
    """bank = (features (F, 3), offsets, (width, height) per template) as synth packs it, L levels -> (x, y, label, modality) rows, width, height"""
    feat, offs, wh = bank
    rows = []
    for m in range(2):
        e = (pyramid * L + level) * 2 + m
        f = feat[offs[e]:offs[e + 1]]
        rows.append(np.concatenate([f, np.full((len(f), 1), m, f.dtype)], 1))
    e0 = (pyramid * L + level) * 2
    return np.concatenate(rows, 0).astype(np.int64), int(wh[e0][0]), int(wh[e0][1])


def _offsets(F, T, Wd, Hd):
    """accessLinearMemory (LL.cpp:1248-1271): flat offset of a feature's run inside its modality's block"""
    x, y, lab = F[:, 0], F[:, 1], F[:, 2]
    return (lab * T * T + (y % T) * T + (x % T)) * (Wd * Hd) + (y // T) * Wd + x // T


def coarse_parts(F, width, height, lms, W, H, T):
    """(raw_p [4][limit], n_p [4]) of one top-level entry: limit = the template's position count, at most the map's"""
    Wd, Hd = W // T, H // T
    wf, hf = (width - 1) // T + 1, (height - 1) // T + 1
    limit = max(0, min((Hd - hf) * Wd + (Wd - wf) + 1, Wd * Hd))
    part = part_of(F[:, 0], F[:, 1], width, height)
    n = np.array([(part == k).sum() for k in range(4)], np.int64)
    raw = np.zeros((4, limit), np.int64)
    inside = (F[:, 0] >= 0) & (F[:, 0] < W) & (F[:, 1] >= 0) & (F[:, 1] < H)          # LL.cpp:1330
    off = _offsets(F, T, Wd, Hd)
    for i in np.nonzero(inside)[0]:
        raw[part[i]] += lms[F[i, 3]][off[i]:off[i] + limit]
    return raw, n


def local_parts(F, width, height, lms, W, H, T, xs, ys):
    """(raw_p [candidates][4][256], n_p [4]) of one entry below the top for candidates whose clamped positions on this level are (xs, ys)"""
    Wd = W // T
    part = part_of(F[:, 0], F[:, 1], width, height)
    n = np.array([(part == k).sum() for k in range(4)], np.int64)
    raw = np.zeros((len(xs), 4, 256), np.int64)
    win = (np.arange(16)[:, None] * Wd + np.arange(16)[None, :]).reshape(-1)
    for c, (x, y) in enumerate(zip(xs, ys)):
        G = F.copy()
        G[:, 0] += (x // T - 8) * T; G[:, 1] += (y // T - 8) * T                          # LL.cpp:1380-1381
        inside = (G[:, 0] >= 0) & (G[:, 1] >= 0) & (G[:, 0] < W) & (G[:, 1] < H)          # LL.cpp:1394
        off = _offsets(G, T, Wd, H // T)
        for m in range(2):
            sel = np.nonzero(inside & (F[:, 3] == m))[0]
            if len(sel) == 0:
                continue
            vals = lms[m][off[sel][:, None] + win[None, :]].astype(np.int64)             # 16 rows of 16 bytes, row stride W / T
            np.add.at(raw[c], part[sel], vals)
    return raw, n


def match_parts(bank, lms, sizes, T, threshold, min_parts, min_part_features=8, cls=0, trace=None):
    """Raw records (lo.MATCH_DTYPE) of a packed bank under the part rule; min_parts = 0: the holistic rule.  cls: the class column of the
    records (a multi-class request is this function per class, cls = the class's place in the request).  trace: a list that receives, per
    template and level from the top down, {"tid", "level", "entered", "left", "pos", "raw", "n", "hit"} — the candidates that entered and left the
    level, and for those that entered the top-level position index resp. a zero, the part sums [entered][4] there (below the top: at the
    arg-max position) the parts' feature counts and who left; it observes the rule and takes no part in it."""
    feat, offs, wh = bank
    L = len(T)
    P = (len(offs) - 1) // (2 * L)
    thr = F32(threshold)
    assert min_parts == 0 or thr >= 0, "threshold < 0 is refused in part mode"
    out = []
    for p in range(P):
        F, w, h = entry_of(bank, p, L - 1, L)
        Wt, Ht = sizes[L - 1]
        Tt = T[L - 1]
        raw, n = coarse_parts(F, w, h, lms[L - 1], Wt, Ht, Tt)
        total = raw.sum(0)
        nf = len(F)
        if min_parts == 0:
            hit = score_of(total, nf) > thr
        else:
            passes = np.zeros(raw.shape[1], np.int64)
            for k in range(4):
                if n[k] >= min_part_features:
                    passes += score_of(raw[k], n[k]) > thr
            hit = passes >= min_parts
        pos = np.nonzero(hit)[0]                                                        # raster order
        if trace is not None:
            trace.append({"tid": p, "level": L - 1, "entered": raw.shape[1], "left": len(pos), "pos": np.arange(raw.shape[1]), "raw": raw.T.copy(), "n": n, "hit": hit.copy()})
        off = Tt // 2 + (Tt % 2 - 1)
        Wd = Wt // Tt
        cx, cy = (pos % Wd) * Tt + off, (pos // Wd) * Tt + off
        sim = score_of(total[pos], nf)
        for l in range(L - 2, -1, -1):
            if len(cx) == 0:
                break
            F, w, h = entry_of(bank, p, l, L)
            Wl, Hl = sizes[l]
            Tl = T[l]
            border, offset = 8 * Tl, Tl // 2 + (Tl % 2 - 1)
            x = np.minimum(np.maximum(cx * 2 + 1, border), Wl - w - border)             # LL.cpp:1871-1880 (the lower clamp first)
            y = np.minimum(np.maximum(cy * 2 + 1, border), Hl - h - border)
            raw, n = local_parts(F, w, h, lms[l], Wl, Hl, Tl, x, y)
            total = raw.sum(1)
            best = total.argmax(1)                                                      # the first maximum in raster order
            rawmax = total[np.arange(len(x)), best]
            br, bc = np.where(rawmax > 0, best // 16, -1), np.where(rawmax > 0, best % 16, -1)      # LL.cpp:1910-1911
            sim = np.where(rawmax > 0, score_of(rawmax, len(F)), F32(0)).astype(F32)
            cx, cy = (x // Tl - 8 + bc) * Tl + offset, (y // Tl - 8 + br) * Tl + offset
            if min_parts == 0:
                keep = ~(sim < thr)
            else:
                passes = np.zeros(len(x), np.int64)
                at = np.where(rawmax > 0, best, 0)
                for k in range(4):
                    if n[k] >= min_part_features:
                        passes += score_of(raw[np.arange(len(x)), k, at], n[k]) >= thr
                keep = passes >= min_parts
            if trace is not None:
                trace.append({"tid": p, "level": l, "entered": len(x), "left": int(keep.sum()), "pos": np.zeros(len(x), np.int64),
                              "raw": raw[np.arange(len(x)), :, np.where(rawmax > 0, best, 0)], "n": n, "hit": keep.copy()})
            cx, cy, sim = cx[keep], cy[keep], sim[keep]
        rec = np.zeros(len(cx), lo.MATCH_DTYPE)
        rec["x"], rec["y"], rec["sim"], rec["tid"], rec["cls"] = cx, cy, sim, p, cls
        out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, lo.MATCH_DTYPE)


def multiset(raw):
    return sorted(zip(raw["x"].tolist(), raw["y"].tolist(), raw["sim"].tolist(), raw["tid"].tolist()))
