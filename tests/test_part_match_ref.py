"""CPU tests of part-based matching: part_match_ref.py (the definition) against a per-position, per-feature statement in Python integers, the
host's part table (lm_part_table) against it, the holistic mode of the same machinery against the oracle, and the conditions on the inputs
that test_gpu_part_match.py relies on — proven here on the reference alone."""
import ctypes
import functools
import os

import numpy as np
import pytest

import linemod_oracle as lo
import lm_abi
import part_match_ref as pm
import response_table_ref as rt
from helpers import GOLDEN

# the third value lies above the smallest parts of the scene's entries (G1, G2: 22..24 features at the top level; G3: 8..10 — 16 there, the first value at which the min_parts = 2 lists of both banks change), so some parts are ineligible
INELIGIBLE = {"G1": 26, "G2": 26, "G3": 16}


def min_part_features(geom):
    return (1, 8, INELIGIBLE[geom])


THRESHOLDS = {"planted": 70.0, "random": 30.0}
GOLDEN_HALF_PARTS2 = 48                 # records of bank 127 on the half-occluded golden frame at threshold 75, min_parts = 2 (holistic: 0)


# ---- the rule, feature by feature -----------------------------------------------------------------------------------------------------------
def slow_match(bank, lms, sizes, T, thr, min_parts, mpf):
    feat, offs, wh = bank
    L = len(T)
    thr = np.float32(thr)
    out = []

    def score(raw, n):
        return (np.float32(raw) * np.float32(100.0)) / np.float32(4 * n) if n else np.float32("nan")

    for p in range((len(offs) - 1) // (2 * L)):
        def entry(l):
            F, w, h = pm.entry_of(bank, p, l, L)
            return [tuple(int(v) for v in f) for f in F], w, h
        F, w, h = entry(L - 1)
        (W, H), Tt = sizes[L - 1], T[L - 1]
        Wd, Hd = W // Tt, H // Tt
        limit = min((Hd - ((h - 1) // Tt + 1)) * Wd + (Wd - ((w - 1) // Tt + 1)) + 1, Wd * Hd)
        n = [0] * 4
        for x, y, _, _ in F:
            n[(2 * x >= w) + 2 * (2 * y >= h)] += 1
        cands = []
        for j in range(max(0, limit)):
            raw = [0] * 4
            for x, y, lab, m in F:
                if 0 <= x < W and 0 <= y < H:
                    raw[(2 * x >= w) + 2 * (2 * y >= h)] += int(lms[L - 1][m][(lab * Tt * Tt + (y % Tt) * Tt + x % Tt) * Wd * Hd + (y // Tt) * Wd + x // Tt + j])
            if sum(1 for k in range(4) if n[k] >= mpf and score(raw[k], n[k]) > thr) >= min_parts:
                o = Tt // 2 + (Tt % 2 - 1)
                cands.append(((j % Wd) * Tt + o, (j // Wd) * Tt + o, score(sum(raw), len(F))))
        for l in range(L - 2, -1, -1):
            F, w, h = entry(l)
            (W, H), Tl = sizes[l], T[l]
            Wd = W // Tl
            n = [0] * 4
            for x, y, _, _ in F:
                n[(2 * x >= w) + 2 * (2 * y >= h)] += 1
            kept = []
            for cx, cy, _ in cands:
                x0 = min(max(cx * 2 + 1, 8 * Tl), W - w - 8 * Tl)
                y0 = min(max(cy * 2 + 1, 8 * Tl), H - h - 8 * Tl)
                best, bat, braw = 0, (-1, -1), [0] * 4
                for r in range(16):
                    for c in range(16):
                        raw = [0] * 4
                        for x, y, lab, m in F:
                            fx, fy = x + (x0 // Tl - 8) * Tl, y + (y0 // Tl - 8) * Tl
                            if 0 <= fx < W and 0 <= fy < H:
                                raw[(2 * x >= w) + 2 * (2 * y >= h)] += int(lms[l][m][(lab * Tl * Tl + (fy % Tl) * Tl + fx % Tl) * Wd * (H // Tl) + (fy // Tl) * Wd + fx // Tl + r * Wd + c])
                        if sum(raw) > best:
                            best, bat, braw = sum(raw), (r, c), raw
                o = Tl // 2 + (Tl % 2 - 1)
                rec = ((x0 // Tl - 8 + bat[1]) * Tl + o, (y0 // Tl - 8 + bat[0]) * Tl + o, score(best, len(F)) if best > 0 else np.float32(0))
                if sum(1 for k in range(4) if n[k] >= mpf and score(braw[k], n[k]) >= thr) >= min_parts:
                    kept.append(rec)
            cands = kept
        out += [(x, y, float(s), p) for x, y, s in cands]
    return sorted(out)


def tiny_case(seed):
    """112 x 96, T = 4, 4 with random response bytes, and hand-made entries of 1..40 features that hold the edge cases: 2x == width on an even
    and on an odd width (the odd one cannot attain it: 2x > width), an empty part, n_p == 8 and n_p == 7 for min_part_features = 8."""
    rng = np.random.default_rng(seed)
    sizes, T = [(112, 96), (56, 48)], [4, 4]
    lms = []
    for W, H in sizes:
        n = 8 * W * H
        lms.append([np.concatenate([rng.choice(np.array([0, 0, 1, 4], np.uint8), n), np.zeros(lo.lm_tail_pad(W // 4, H // 4), np.uint8)]) for _ in range(2)])
    feats, offs, whs = [], [0], []

    def add(entry_feats, w, h):
        for m in range(2):
            f = np.array([e[:3] for e in entry_feats if e[3] == m], np.int32).reshape(-1, 3)
            feats.append(f); offs.append(offs[-1] + len(f)); whs.append((w, h))

    def rand_entry(nf, w, h):
        return [(int(rng.integers(0, w + 1)), int(rng.integers(0, h + 1)), int(rng.integers(0, 8)), int(rng.integers(0, 2))) for _ in range(nf)]

    # pyramid 0: even width 20 with features at x = 10 (2x == width: right parts); level 1 of 1 feature
    add([(10, 3, 1, 0), (9, 3, 2, 1), (10, 12, 3, 0), (0, 0, 4, 1)] + rand_entry(20, 20, 16), 20, 16); add([(2, 2, 5, 0)], 10, 8)
    # pyramid 1: odd width 21 (x = 10: 20 < 21 left, x = 11 right), an empty part (nothing with 2y >= height on the left)
    add([(10, 2, 1, 0), (11, 2, 2, 1), (11, 12, 3, 0)] + [(int(rng.integers(11, 22)), int(rng.integers(0, 18)), int(rng.integers(0, 8)), 1) for _ in range(12)], 21, 17)
    add(rand_entry(6, 10, 8), 10, 8)
    # pyramid 2: parts of exactly 8 and 7 features (min_part_features = 8: eligible / not), 40 features in all
    e = [(1 + k, 1, k % 8, k % 2) for k in range(8)] + [(14 + (k % 5), 1 + k // 5, k % 8, 0) for k in range(7)]
    e += [(int(rng.integers(0, 12)), int(rng.integers(10, 21)), int(rng.integers(0, 8)), 1) for _ in range(12)] + [(int(rng.integers(12, 25)), int(rng.integers(10, 21)), int(rng.integers(0, 8)), 0) for _ in range(13)]
    add(e, 24, 20); add(rand_entry(40, 12, 10), 12, 10)
    bank = (np.concatenate(feats).astype(np.int32), np.array(offs, np.int32), np.array(whs, np.int32))
    return bank, lms, sizes, T


@pytest.mark.parametrize("min_parts,mpf", [(1, 1), (2, 1), (2, 8), (3, 4), (4, 1)])
def test_the_reference_equals_the_statement_in_python_integers(min_parts, mpf):
    bank, lms, sizes, T = tiny_case(5)
    F, w, h = pm.entry_of(bank, 2, 0, 2)
    assert sorted(pm.part_table(w, h, F[:, 0], F[:, 1], 8)["n"].tolist())[:2] == [7, 8] and len(F) == 40
    F1, w1, h1 = pm.entry_of(bank, 1, 0, 2)
    assert 0 in pm.part_table(w1, h1, F1[:, 0], F1[:, 1], 1)["n"].tolist()
    assert pm.part_of(10, 0, 20, 16) == 1 and pm.part_of(10, 0, 21, 17) == 0 and pm.part_of(11, 0, 21, 17) == 1 and pm.part_of(0, 8, 20, 16) == 2
    for thr in (20.0, 35.0):
        want = slow_match(bank, lms, sizes, T, thr, min_parts, mpf)
        got = pm.multiset(pm.match_parts(bank, lms, sizes, T, thr, min_parts, mpf))
        assert got == want
    assert len(slow_match(bank, lms, sizes, T, 20.0, min_parts, mpf)) > 0


def test_the_host_part_table_equals_the_reference():
    if not os.path.exists(lm_abi.library_path()):
        import __graft_entry__ as g
        g.build()
    lib = lm_abi.load_library()
    rng = np.random.default_rng(9)
    cases = [(20, 16, [10, 9, 10, 0], [3, 3, 12, 0]), (21, 17, [10, 11], [2, 2]), (8, 8, [], []), (30, 30, [1] * 7, [1] * 7), (30, 30, [1] * 8, [1] * 8),
             (30, 30, [1] * 9 + [20] * 16 + [1] * 17, [1] * 9 + [1] * 16 + [20] * 17)]
    for _ in range(30):
        w, h, n = int(rng.integers(1, 60)), int(rng.integers(1, 60)), int(rng.integers(0, 41))
        cases.append((w, h, rng.integers(-3, w + 4, n).tolist(), rng.integers(-3, h + 4, n).tolist()))
    for w, h, xs, ys in cases:
        for mpf in (1, 8, 9):
            xa, ya = np.array(xs, np.int32), np.array(ys, np.int32)
            out, order = np.zeros(16, np.int32), np.full(len(xs) + 28, -7, np.int32)
            assert lib.lm_part_table(w, h, xa.ctypes.data_as(ctypes.c_void_p), ya.ctypes.data_as(ctypes.c_void_p), len(xs), mpf, out.ctypes.data_as(ctypes.c_void_p),
                                     order.ctypes.data_as(ctypes.c_void_p)) == 0
            ref = pm.part_table(w, h, xa.astype(np.int64), ya.astype(np.int64), mpf)
            assert out[0:4].tolist() == ref["start"].tolist() and out[4:8].tolist() == ref["n"].tolist()
            assert out[8:12].tolist() == ref["npad"].tolist() and out[12:16].tolist() == ref["eligible"].tolist()
            assert order[:len(ref["order"])].tolist() == ref["order"].tolist() and (order[len(ref["order"]):] == -7).all()
    assert lib.lm_part_table(4, 4, None, None, 0, 0, np.zeros(16, np.int32).ctypes.data_as(ctypes.c_void_p), None) != 0       # min_part_features >= 1


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------------------
def windows_stay_inside(bank, W, H, T, pyramid):
    """the detector's condition for part matching (bits_all_in) on one pyramid: every refinement window inside its planes"""
    L = len(T)
    for l in range(L - 1):
        F, w, h = pm.entry_of(bank, pyramid, l, L)
        if not (F[:, 0].min() >= 0 and F[:, 1].min() >= 0 and F[:, 0].max() <= w and F[:, 1].max() <= h and (W >> l) - w - 16 * T[l] >= 0 and (H >> l) - h - 16 * T[l] >= 0):
            return False
    return True


def sub_bank(bank, L, keep):
    feat, offs, wh = bank
    fs, o, whs = [], [0], []
    for p in keep:
        for e in range(2 * L * p, 2 * L * (p + 1)):
            fs.append(feat[offs[e]:offs[e + 1]]); o.append(o[-1] + offs[e + 1] - offs[e]); whs.append(wh[e])
    return np.ascontiguousarray(np.concatenate(fs), np.int32), np.array(o, np.int32), np.array(whs, np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def fitting_bank(geom, kind):
    """The templates of a scene's bank that part matching accepts (the others have refinement windows that leave their planes, which the
    detector refuses under part matching): all 40 on G1 and of G2's planted bank, fewer elsewhere.  -> (bank, kept pyramids)"""
    sc = rt.scene(geom)
    bank = sc["banks"][kind]
    keep = [p for p in range(40) if windows_stay_inside(bank, sc["W"], sc["H"], sc["T"], p)]
    return sub_bank(bank, len(sc["T"]), keep), keep


@functools.lru_cache(maxsize=None)
def reference(geom, kind, min_parts, mpf, thr=None):
    sc = rt.scene(geom)
    lms, sizes = rt.memories(geom, rt.DEFAULT)
    return pm.match_parts(fitting_bank(geom, kind)[0], lms, sizes, sc["T"], THRESHOLDS[kind] if thr is None else thr, min_parts, mpf)


@pytest.mark.parametrize("geom", ["G1", "G2", "G3"])
def test_conditions_on_the_parity_inputs(geom):
    sc = rt.scene(geom)
    lms, sizes = rt.memories(geom, rt.DEFAULT)
    differ = False
    for kind in ("planted", "random"):
        bank, keep = fitting_bank(geom, kind)
        assert len(keep) >= 10 and (geom != "G1" or len(keep) == 40)
        # the holistic mode of this file's machinery is the oracle
        hol = pm.match_parts(bank, lms, sizes, sc["T"], THRESHOLDS[kind], 0)
        raw, _ = lo.match_bank_c(lo.PackedBank(len(keep), len(sc["T"]), *bank), lms, sizes, sc["T"], THRESHOLDS[kind])
        assert pm.multiset(hol) == rt.multiset(raw)
        for mpf in min_part_features(geom):
            lists = [pm.multiset(reference(geom, kind, mp, mpf)) for mp in (1, 2, 3, 4)]
            assert all(len(l) > 0 for l in lists) and all(l != pm.multiset(hol) for l in lists)
            differ = differ or len(set(map(tuple, lists))) == 4
        assert pm.multiset(reference(geom, kind, 2, INELIGIBLE[geom])) != pm.multiset(reference(geom, kind, 2, 8))     # ... and the lists show it
    assert differ


def golden_half():
    import ref_cases as rc
    case = rc.fixture_case("_half", "127")
    q = rc.quantized_of(case)
    lms = [[lo.build_linear_memories(q[l][m], case["T"][l]) for m in range(2)] for l in range(2)]
    sizes = [(q[l][0].shape[1], q[l][0].shape[0]) for l in range(2)]
    b = case["banks"]["06_template"]
    return case, (b.feat, b.tmpl_off, b.tmpl_wh), lms, sizes


def test_the_golden_half_occluded_frame():
    case, bank, lms, sizes = golden_half()
    P = (len(bank[1]) - 1) // 4
    assert all(windows_stay_inside(bank, 640, 480, [5, 8], p) for p in range(P))
    assert len(pm.match_parts(bank, lms, sizes, [5, 8], 75.0, 0)) == 0                      # nothing at the driver's threshold
    assert len(lo.match_bank_c(lo.PackedBank(P, 2, *bank), lms, sizes, [5, 8], 75.0)[0]) == 0
    n = len(pm.match_parts(bank, lms, sizes, [5, 8], 75.0, 2, 8))
    print("part records on the half-occluded frame:", n)
    assert n == GOLDEN_HALF_PARTS2 and n > 0
