"""CPU checks of wide_planes_ref.py, the numpy statement of the "wide" bit planes (two sets of strip records / pair streams) and of the
lane-level sum of k_local_wide, for all 70 legal response tables on G1's memories (response_table_ref.py).

One point where this file follows the detector rather than the letter of "c0 + 2 c1 + 4 c2 for every table": a table of two planes whose
second value a is 2 or 3 (4 2 0 0 0, 4 3 3 0 0, ...) keeps today's packing under "wide" — bit 2c = "is a", set 1 empty —, and that packing
sums to a c0 + 4 c2, as k_local_bits<., ., a> does.  Demanding both "set 0 equals the existing packing, set 1 is zero" and weight 1 for c0
is impossible for such a table (a cell of value 2 would count 1).  So the weights are wide_planes_ref.weights(r): (1, 2, 4) for every table
of three or four values and for a = 1, (a, 2, 4) with c1 = 0 otherwise; every other check is as stated, for all 70 tables."""
import numpy as np
import pytest

import linemod_oracle as lo
import response_table_ref as rt
import wide_planes_ref as wp

GEOM = "G1"


# ---- the existing packing of the two-plane tables, restated from the GPU test of the response tables (bit 2c = "is a", 2c + 1 = "is 4") ----
def old_strip_records(lm_flat, T, Wd, Hd, a):
    NS = (Wd + 15) // 16
    planes = lm_flat[:8 * T * T * Wd * Hd].reshape(8, T * T, Hd, Wd)
    pad = np.zeros((8, T * T, Hd, NS * 16 + 32), np.uint8)
    pad[..., :Wd] = planes
    w1 = np.uint64(1) << (2 * np.arange(32, dtype=np.uint64))
    out = np.zeros((8, T * T, NS, Hd), np.uint64)
    for s in range(NS):
        seg = pad[..., 16 * s:16 * s + 32]
        out[:, :, s, :] = ((seg == a).astype(np.uint64) * w1).sum(axis=-1) + ((seg == 4).astype(np.uint64) * (w1 << np.uint64(1))).sum(axis=-1)
    return out


def old_pair_stream(lm_colour, lm_normal, T, Wd, Hd, npairs, a):
    block = npairs * 16
    flat = np.zeros(2 * block, np.uint8)
    n = 8 * T * T * Wd * Hd
    flat[:n] = lm_colour[:n]; flat[block:block + n] = lm_normal[:n]
    g = flat.reshape(npairs, 32)
    w = np.uint32(1) << np.arange(32, dtype=np.uint32)
    out = np.zeros((npairs, 2), np.uint32)
    out[:, 0] = ((g == a).astype(np.uint32) * w).sum(axis=1); out[:, 1] = ((g == 4).astype(np.uint32) * w).sum(axis=1)
    return out


def _level(sc, l):
    T = sc["T"][l]
    return T, (sc["W"] >> l) // T, (sc["H"] >> l) // T


def _features(sc, t, l):
    """level-l features of planted template t as rows (x, y, label, modality)"""
    feat, offs, _ = sc["banks"]["planted"]
    L = len(sc["T"])
    rows = []
    for m in range(2):
        k = (t * L + l) * 2 + m
        f = feat[offs[k]:offs[k + 1]]
        rows.append(np.column_stack([f[:, :3], np.full(len(f), m)]))
    return np.concatenate(rows).astype(np.int64)


def _origins(sc, F, t):
    """two window origins of template t at level 0 with every window inside its planes: the one the refinement takes at the oracle's best match
    (the sums there reach the template's score), and one beside it at an odd column (another shift, another strip carry)"""
    T, Wd, Hd = _level(sc, 0)
    raw, _ = rt.oracle(GEOM, "planted", rt.DEFAULT, 70.0)
    mine = raw[raw["tid"] == t]
    assert len(mine) > 0
    best = mine[np.argmax(mine["sim"])]
    cx, cy = int(F[:, 0].max()) // T, int(F[:, 1].max()) // T
    out = []
    for dx, dy in ((0, 0), (3, 1)):
        gx = min(max(int(best["x"]) // T - 8 + dx, 0), Wd - 16 - cx)
        gy = min(max(int(best["y"]) // T - 8 + dy, 0), Hd - 17 - cy)
        assert gx >= 0 and gy >= 0
        out.append((gx, gy))
    return out


TABLES = rt.legal_tables()


def test_seventy_tables_of_which_thirty_five_need_the_second_set():
    assert len(TABLES) == 70
    assert sum(rt.distinct_nonzero(r) > 2 for r in TABLES) == 35
    for name in ("linemod", "drop1", "drop1_keep3"):
        assert wp.weights(rt.NAMED[name]) == (1, 2, 4)
    assert wp.weights(rt.DEFAULT) == (1, 2, 4) and wp.weights(rt.NAMED["levelup2"]) == (2, 2, 4) and wp.weights((4, 4, 4, 4, 4)) == (1, 2, 4)


@pytest.mark.parametrize("r", TABLES, ids=["".join(map(str, r)) for r in TABLES])
def test_both_sets_give_back_the_bytes_and_the_lane_sum_is_the_byte_sum(r):
    sc = rt.scene(GEOM)
    lms, _ = rt.memories(GEOM, r)
    L = len(sc["T"])
    two = rt.distinct_nonzero(r) <= 2
    # levels below the top: strip records
    T, Wd, Hd = _level(sc, 0)
    n = 8 * T * T * Wd * Hd
    recs = [wp.strip_records(lms[0][m], T, Wd, Hd, r) for m in range(2)]
    planes = [lms[0][m][:n].reshape(8, T * T, Hd, Wd) for m in range(2)]
    for m in range(2):
        assert np.array_equal(wp.unpack_strip_records(recs[m][0], recs[m][1], Wd, r), planes[m])
        assert wp.strip_overlap_ok(recs[m][0], Wd) and wp.strip_overlap_ok(recs[m][1], Wd)
        if two:
            assert np.array_equal(recs[m][0], old_strip_records(lms[0][m], T, Wd, Hd, wp.low_value(r) or 255)) and not recs[m][1].any()
    # the top level: pair streams (the detector's stream starts at the colour block; blocks of whole pairs as laid out here)
    Tt, Wdt, Hdt = _level(sc, L - 1)
    nt = 8 * Tt * Tt * Wdt * Hdt
    npairs = 2 * ((nt + lo.lm_tail_pad(Wdt, Hdt) + 31) // 32)
    ps = wp.pair_streams(lms[L - 1][0], lms[L - 1][1], Tt, Wdt, Hdt, npairs, r)
    flat = wp.unpack_pair_streams(ps[0], ps[1], r)
    block = npairs * 16
    assert np.array_equal(flat[:nt], lms[L - 1][0][:nt]) and np.array_equal(flat[block:block + nt], lms[L - 1][1][:nt])
    assert not flat[nt:block].any() and not flat[block + nt:].any()
    if two:
        assert np.array_equal(ps[0], old_pair_stream(lms[L - 1][0], lms[L - 1][1], Tt, Wdt, Hdt, npairs, wp.low_value(r) or 255)) and not ps[1].any()
    # the lane-level sum of the refinement at every position of the windows of a planted template
    w = wp.weights(r)
    rec0, rec1 = np.stack([recs[0][0], recs[1][0]]), np.stack([recs[0][1], recs[1][1]])
    t = 3
    F = _features(sc, t, 0)
    for gx, gy in _origins(sc, F, t):
        n1, n2, n4 = wp.lane_counts(rec0, rec1, F, T, Hd, gx, gy)
        c0, c1, c2 = wp.positions(n1), wp.positions(n2), wp.positions(n4)
        want = wp.byte_window_sums(planes, F, T, gx, gy)
        assert max(c0.max(), c1.max(), c2.max()) <= len(F) and want.max() <= 4 * len(F)
        assert np.array_equal(w[0] * c0 + w[1] * c1 + w[2] * c2, want)
        if two:
            assert not c1.any()
        if w[0] == 1:                                            # the kernel's own bit-sliced sum, 12 bits per position
            assert np.array_equal(wp.positions(wp.weighted_sum_wide(n1, n2, n4)), want)
    # ... and of the coarse pass: a lane's 32 positions are 32 consecutive bits of the streams, a feature shifts them by its offset
    Ft = _features(sc, t, L - 1)
    d = [[((s[:, k][:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(-1).astype(np.int64) for k in range(2)] for s in ps]
    npos = Wdt * Hdt
    c = [np.zeros(npos, np.int64) for _ in range(3)]
    want = np.zeros(npos, np.int64)
    for x, y, lab, m in Ft:
        off = (lab * Tt * Tt + (y % Tt) * Tt + (x % Tt)) * npos + (y // Tt) * Wdt + (x // Tt)
        c[0] += d[0][0][m * block + off:m * block + off + npos]; c[1] += d[1][0][m * block + off:m * block + off + npos]
        c[2] += d[0][1][m * block + off:m * block + off + npos]
        want += lms[L - 1][m][off:off + npos]
    assert np.array_equal(w[0] * c[0] + w[1] * c[1] + w[2] * c[2], want) and want.max() > 0
