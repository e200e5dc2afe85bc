"""CPU tests of the statement of depth-scaled matching (scaled_match_ref.py) and of the conditions that test_gpu_scaled_match.py relies on
(scaled_cases.py): lm_scaled_features against numpy, the ladder selection against Python integers, a per-pixel restatement in plain loops, the
ladder {1024} against part_match_ref.match_parts(min_parts=0) — which the suite holds to the oracle —, and the edge conditions."""
import os

import numpy as np
import pytest

import lm_abi
import part_match_ref as pm
import scaled_cases as sc
import scaled_match_ref as sm


# ---- 1. lm_scaled_features ------------------------------------------------------------------------------------------------------------------
def test_scale_coord_by_hand():
    # centre 10: dx = 0 stays; 512 halves with the half-way case away from the centre (|dx| = 1 -> (512 + 512) >> 10 = 1); 2048 doubles
    assert sm.scale_coord([10, 11, 9, 13, 7, 20, 0], 10, 512).tolist() == [10, 11, 9, 12, 8, 15, 5]
    assert sm.scale_coord([10, 11, 9, 20, 0], 10, 2048).tolist() == [10, 12, 8, 30, -10]
    assert sm.scale_coord([10, 11, 9, 20, 0], 10, 1024).tolist() == [10, 11, 9, 20, 0]
    assert sm.scale_coord([12], 10, 768).tolist() == [12] and sm.scale_coord([8], 10, 768).tolist() == [8]     # 1.5 rounds away, on both sides
    assert [sm.q10(s) for s in (0.5, 1.0, 2.0, 0.75, 2.0 ** 0.25)] == [512, 1024, 2048, 768, 1218]


def test_lm_scaled_features_equals_the_statement():
    if not os.path.exists(lm_abi.library_path()):
        import __graft_entry__ as g
        g.build()
    import lm_detector
    rng = np.random.default_rng(5)
    used = sorted({q for lad in sc.LADDERS.values() for q in sc.ladder_q10(lad)} | {512, 1024, 2048, 768, 1280})
    for w, h in ((64, 48), (33, 57), (2, 2), (75, 1)):
        xs = np.concatenate([rng.integers(-20, w + 20, 200), [w // 2, 0, w, w // 2 + 1, w // 2 - 1]]).astype(np.int32)
        ys = np.concatenate([rng.integers(-20, h + 20, 200), [h // 2, 0, h, h // 2 + 1, h // 2 - 1]]).astype(np.int32)
        for s in used:
            gx, gy = lm_detector.scaled_features(w, h, xs, ys, s)
            wx, wy = sm.scaled_features(w, h, xs, ys, s)
            assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (w, h, s)
    with pytest.raises(RuntimeError, match=r"\[512, 2048\]"):
        lm_detector.scaled_features(10, 10, [1], [1], 511)


# ---- 2. ladder selection and bounds -----------------------------------------------------------------------------------------------------------
def pick(d, d_train, scales, lo, hi):
    """plain Python integers"""
    t = d_train * 1024
    if d == 0 or t < lo * d or t > hi * d:
        return -1
    best, k = None, -1
    for q, s in enumerate(scales):
        e = abs(s * d - t)
        if best is None or e < best:
            best, k = e, q
    return k


def test_ladder_selection_by_hand():
    lad = [768, 1280]
    assert sm.select_scale([1000], 1000, lad).tolist() == [0]                          # an exact tie goes to the lower entry
    assert sm.select_scale([999], 1000, lad).tolist() == [1] and sm.select_scale([1001], 1000, lad).tolist() == [0]
    assert sm.select_scale([0], 1000, lad).tolist() == [-1]                            # no measurement
    lad = [512, 1024, 2048]
    assert sm.select_scale([2000, 2001, 500, 499], 1000, lad).tolist() == [0, -1, 2, -1]    # d exactly on min and on max is inside
    assert sm.select_scale([1000, 1001, 999], 1000, [1024], 1024, 1024).tolist() == [0, -1, -1]
    rng = np.random.default_rng(9)
    for _ in range(40):
        K = int(rng.integers(1, 17))
        lad = sorted(rng.choice(np.arange(512, 2049), K, replace=False).tolist())
        d = rng.integers(0, 65536, 64)
        d[:4] = [0, 1, 65535, 1000]
        dt = int(rng.integers(1, 65536))
        lo, hi = int(rng.integers(256, 1025)), int(rng.integers(1024, 4097))
        assert sm.select_scale(d, dt, lad, lo, hi).tolist() == [pick(int(v), dt, lad, lo, hi) for v in d]


def test_probe_map_by_hand():
    d = np.array([[0, 0, 0, 0], [0, 7, 0, 0], [0, 0, 0, 0], [0, 0, 0, 3]], np.uint16)
    assert sm.probe_map(d, 0).tolist() == d.tolist()
    assert sm.probe_map(d, 1).tolist() == [[7, 7, 7, 0], [7, 7, 7, 0], [7, 7, 3, 3], [0, 0, 3, 3]]
    assert (sm.probe_map(np.zeros((5, 5), np.uint16), 2) == 0).all()


# ---- 3. a per-pixel statement in plain loops ----------------------------------------------------------------------------------------------------
def loops(bank, lms, sizes, T, threshold, depth0, d_train, scales, lo, hi, probe):
    L = len(T)
    H0, W0 = depth0.shape
    out = []
    for p in range((len(bank[1]) - 1) // (2 * L)):
        def resp(l, F, w, h, k, ox, oy):
            Tl = T[l]
            Wd, Hd = sizes[l][0] // Tl, sizes[l][1] // Tl
            raw = 0
            for fx, fy, lab, m in F.tolist():
                dx, dy = fx - w // 2, fy - h // 2
                sx = w // 2 + (1 if dx > 0 else -1 if dx < 0 else 0) * ((abs(dx) * scales[k] + 512) >> 10)
                sy = h // 2 + (1 if dy > 0 else -1 if dy < 0 else 0) * ((abs(dy) * scales[k] + 512) >> 10)
                px, py = ox + sx, oy + sy
                if 0 <= px // Tl < Wd and 0 <= py // Tl < Hd:
                    raw += int(lms[l][m][(lab * Tl * Tl + (py % Tl) * Tl + px % Tl) * Wd * Hd + (py // Tl) * Wd + px // Tl])
            return raw
        F, w, h = pm.entry_of(bank, p, L - 1, L)
        Tt = T[L - 1]
        Wd, Hd = sizes[L - 1][0] // Tt, sizes[L - 1][1] // Tt
        limit = max(0, min((Hd - ((h - 1) // Tt + 1)) * Wd + (Wd - ((w - 1) // Tt + 1)) + 1, Wd * Hd))
        for pos in range(limit):
            i, j = pos % Wd, pos // Wd
            px, py = min(max((i * Tt + w // 2) << (L - 1), 0), W0 - 1), min(max((j * Tt + h // 2) << (L - 1), 0), H0 - 1)
            win = depth0[max(0, py - probe):py + probe + 1, max(0, px - probe):px + probe + 1]
            d = int(win[win > 0].min()) if (win > 0).any() else 0
            k = pick(d, d_train, scales, lo, hi)
            if k < 0:
                continue
            sim = pm.score_of(resp(L - 1, F, w, h, k, i * Tt, j * Tt), len(F))
            if not sim > np.float32(threshold):
                continue
            off = Tt // 2 + (Tt % 2 - 1)
            cx, cy, alive = i * Tt + off, j * Tt + off, True
            for l in range(L - 2, -1, -1):
                Fl, wl, hl = pm.entry_of(bank, p, l, L)
                Tl = T[l]
                x = min(max(cx * 2 + 1, 8 * Tl), sizes[l][0] - wl - 8 * Tl)
                y = min(max(cy * 2 + 1, 8 * Tl), sizes[l][1] - hl - 8 * Tl)
                best, br, bc = 0, -1, -1
                for r in range(16):
                    for c in range(16):
                        v = resp(l, Fl, wl, hl, k, (x // Tl - 8 + c) * Tl, (y // Tl - 8 + r) * Tl)
                        if v > best:
                            best, br, bc = v, r, c
                sim = pm.score_of(best, len(Fl)) if best > 0 else np.float32(0)
                o = Tl // 2 + (Tl % 2 - 1)
                cx, cy = (x // Tl - 8 + bc) * Tl + o, (y // Tl - 8 + br) * Tl + o
                if sim < np.float32(threshold):
                    alive = False
                    break
            if alive:
                out.append((cx, cy, float(sim), 0, p, k, d))
    return out


def test_plain_loops_equal_the_vectorised_reference():
    """on a tiny frame (96 x 80, T = (4, 8)) with 3 small templates: every step of the rule once more, pixel by pixel"""
    import response_table_ref as rt
    import synth
    rgb, dep = synth.make_frame(17, 96, 80, 6)
    import linemod_oracle as lo
    T = [4, 8]
    pyr = lo.OracleDetector(150, T).quantize_pyramid(rgb, dep)
    bank = synth.make_planted_bank(5, 3, [(q[0], q[1]) for q in pyr], T, (12, 6), windows=[(34, 34, 20, 10), (40, 36, 14, 8), (36, 34, 10, 10)])
    lms, sizes = rt.linear_memories(pyr, T, rt.DEFAULT)
    scales = [512, 724, 1024, 1448, 2048]
    for probe, thr, lo_hi in ((0, 40.0, (None, None)), (2, 55.0, (700, 1500)), (4, 30.0, (256, 4096))):
        got = sm.match_scaled(bank, lms, sizes, T, thr, dep, 900, scales, lo_hi[0], lo_hi[1], probe)
        want = loops(bank, lms, sizes, T, thr, dep, 900, scales, scales[0] if lo_hi[0] is None else lo_hi[0],
                     scales[-1] if lo_hi[1] is None else lo_hi[1], probe)
        assert len(want) > 0 and sorted(sm.rows(got)) == sorted(want), (probe, thr)
        assert len(set(r[5] for r in want)) > 1                                           # more than one ladder entry in play


# ---- 4. the ladder {1024} is the holistic rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [sc.T2, sc.T1, sc.T3])
def test_ladder_1024_equals_the_holistic_rule_where_nothing_wraps(T):
    s = sc.scene(T)
    L = len(T)
    Tt = T[-1]
    Wd = s["sizes"][-1][0] // Tt
    for p in range(24):                                                                  # no holistic candidate sits on a cell whose reads wrap
        F, w, h = pm.entry_of(s["bank"], p, L - 1, L)
        raw, _ = pm.coarse_parts(F, w, h, s["lms"][L - 1], s["sizes"][L - 1][0], s["sizes"][L - 1][1], Tt)
        hits = np.nonzero(pm.score_of(raw.sum(0), len(F)) > np.float32(sc.THRESHOLD))[0]
        assert ((hits % Wd) + (w - 1) // Tt + 1 <= Wd).all(), p
    raw, _ = sc.reference(T, 1, 2, sc.THRESHOLD, sc.D_TRAIN, (0.25, 4.0))
    hol = sc.holistic(T)
    assert len(hol) > 0 and sc.as_holistic(raw) == sc.as_holistic(hol)
    assert (raw["scale_index"] == 0).all() and (raw["depth_mm"] > 0).all()


# ---- 5. the conditions the GPU cases rely on ------------------------------------------------------------------------------------------------------
def test_conditions_of_the_parity_cases():
    for ladder in sc.LADDERS:
        for probe in sc.PROBES:
            raw, st = sc.reference(sc.T2, ladder, probe, sc.THRESHOLD, sc.D_TRAIN, sc.PARITY_BOUNDS[ladder])
            assert len(raw) > 0, (ladder, probe)
    assert len(set(sc.reference(sc.T2, 9, 2)[0]["scale_index"].tolist())) >= 3            # several ladder entries are in play
    assert len(set(sc.reference(sc.T2, 16, 2)[0]["scale_index"].tolist())) >= 5
    rows = [sorted(sm.rows(sc.reference(sc.T2, 9, p)[0])) for p in sc.PROBES]
    assert rows[0] != rows[1] and rows[1] != rows[2]                                    # the probe radius matters
    assert sc.reference(sc.T2, 9, 2, 40.0)[1]["candidates"] > 2 * 1024                  # overflows a capacity of 1024, twice over
    for T in (sc.T1, sc.T3):
        assert len(sc.reference(T, 9, 2)[0]) > 0


def test_conditions_of_the_edge_cases():
    cases = sc.edge_cases()
    s = sc.scene()
    d0 = sc.anchor_depth()
    raw, _ = sc.reference(**cases["bounds"])
    assert len(raw) > 0 and (raw["depth_mm"] == d0).all()                               # exclusive bounds would leave nothing
    raw, _ = sc.reference(**cases["tie"])
    tied = raw[raw["depth_mm"] == d0]
    assert len(tied) > 0 and (tied["scale_index"] == 0).all() and (raw["scale_index"] == 1).any()
    # "double": at cell (0, 0) a feature left of / above the centre is sampled outside the level; "half": features coincide
    L, outside, coincide = 2, 0, 0
    for p in range(24):
        F, w, h = pm.entry_of(s["bank"], p, L - 1, L)
        sx, sy = sm.scaled_features(w, h, F[:, 0], F[:, 1], 2048)
        outside += int(((sx < 0) | (sy < 0)).sum())
        hx, hy = sm.scaled_features(w, h, F[:, 0], F[:, 1], 512)
        coincide += len(F) - len(set(zip(hx.tolist(), hy.tolist(), F[:, 2].tolist(), F[:, 3].tolist())))
    assert outside > 0 and coincide > 0
    raw, _ = sc.reference(**cases["double"])
    assert len(raw) > 0 and (raw["x"] < 16).any() and (raw["y"] < 16).any()              # records at the frame's left and top
    # ... and top-level candidates in column 0 and in row 0 of templates that sample left of / above the level there (cdx < 0, cdy < 0)
    kw = cases["double"]
    P0 = sm.probe_map(s["dep"], 2)
    left = top = 0
    Wd = s["sizes"][1][0] // s["T"][1]
    for p in range(24):
        F, w, h = pm.entry_of(s["bank"], p, L - 1, L)
        sx, sy = sm.scaled_features(w, h, F[:, 0], F[:, 1], 2048)
        pos, k, d, rawsum, nf = sm.coarse(s["bank"], p, s["lms"], s["sizes"], s["T"], P0, kw["d_train"], [2048], sm.q10(kw["lo_hi"][0]), sm.q10(kw["lo_hi"][1]))
        hit = pos[pm.score_of(rawsum, nf) > np.float32(kw["threshold"])]
        left += int((hit % Wd == 0).sum()) * int((sx < 0).any())
        top += int((hit // Wd == 0).sum()) * int((sy < 0).any())
    assert left > 0 and top > 0
    assert len(sc.reference(**cases["half"])[0]) > 0


def test_conditions_of_the_efficacy_case():
    e = sc.efficacy()
    assert e["d_train"] == 1000 and abs(int(sm.probe_map(e["train"][1], 2)[120, 160]) - 1000) <= 5     # the cap's front stands at the stated distance
    for z, s in e["scenes"].items():
        on = sc.on_object(sm.canonical(s["want"]), e["box"])
        assert len(on) > 0 and (on["scale_index"] == s["k"]).all(), z                   # found, with the ladder entry nearest to 1000 / z
        assert len(sc.on_object(s["hol"], e["box"])) == 0, z                             # the holistic rule finds nothing there at this threshold
    assert [e["scenes"][z]["k"] for z in sc.EFFICACY_Z] == [6, 2]
