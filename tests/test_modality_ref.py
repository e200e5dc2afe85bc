"""tests/modality_ref.py against an independent statement: the empty-slot construction on the two-slot oracle equals a brute-force numpy
scorer of ONE modality, in the oracle's 8-bit mode (63 features) and its 16-bit mode (64 and more); through the reference's own match lines
where they were built; and cropTemplates over the present templates gives other coordinates than the colour half of the pair's template."""
import numpy as np
import pytest

import linemod_oracle as lo
import ll_ref
import modality_ref as mr

W, H, T = 208, 176, (4, 8)


def brute(maps, T, pyramids, thr):
    """matchClass over one modality (LL.cpp:1788-1941) in numpy: the sum of the features' responses at every top-level template position,
    then per level below the 16 x 16 window around each surviving candidate.  Returns the raw records (x, y, sim, tid)."""
    mem, geo = [], []
    for l, q in enumerate(maps):
        t, (h, w) = T[l], q.shape
        resp = lo.response_np(lo.spread_np(q, t))
        planes = [lo.linearize_np(resp[o], t).reshape(-1) for o in range(8)]
        mem.append(np.concatenate(planes + [np.zeros(lo.lm_tail_pad(w // t, h // t), np.uint8)]).astype(np.int64))
        geo.append((w, h, t, w // t, h // t))

    def run(l, x, y, lab):                                  # accessLinearMemory (LL.cpp:1248-1271)
        w, h, t, wd, hd = geo[l]
        return (lab * t * t + (y % t) * t + x % t) * wd * hd + (y // t) * wd + x // t

    out, L = [], len(T)
    for tid, tp in enumerate(pyramids):
        w, h, t, wd, hd = geo[L - 1]
        top = tp[L - 1]
        npos = (hd - ((top.height - 1) // t + 1)) * wd + (wd - ((top.width - 1) // t + 1)) + 1
        tot = np.zeros(wd * hd, np.int64)
        for x, y, lab in top.features.tolist():
            if 0 <= x < w and 0 <= y < h:
                tot[:npos] += mem[L - 1][run(L - 1, x, y, lab):][:npos]
        score = (tot.astype(np.float32) * np.float32(100)) / np.float32(4 * len(top.features))
        off = t // 2 + (t % 2 - 1)
        cands = [[(j % wd) * t + off, (j // wd) * t + off, score[j]] for j in np.nonzero(score > np.float32(thr))[0]]
        for l in range(L - 2, -1, -1):
            w, h, t, wd, hd = geo[l]
            tl, border, off = tp[l], 8 * t, t // 2 + (t % 2 - 1)
            kept = []
            for cx, cy, _ in cands:
                x = min(max(cx * 2 + 1, border), w - tl.width - border)
                y = min(max(cy * 2 + 1, border), h - tl.height - border)
                ox, oy = (x // t - 8) * t, (y // t - 8) * t
                win = np.zeros((16, 16), np.int64)
                for fx, fy, lab in tl.features.tolist():
                    fx, fy = fx + ox, fy + oy
                    if 0 <= fx < w and 0 <= fy < h:
                        p = run(l, fx, fy, lab)
                        win += np.stack([mem[l][p + r * wd:p + r * wd + 16] for r in range(16)])
                sc = (win.astype(np.float32) * np.float32(100)) / np.float32(4 * len(tl.features))
                k = int(np.argmax(sc))                       # the first maximum in raster order (strict > in LL.cpp:1919)
                if sc.flat[k] > 0 and not sc.flat[k] < np.float32(thr):
                    kept.append([(x // t - 8 + k % 16) * t + off, (y // t - 8 + k // 16) * t + off, sc.flat[k]])
            cands = kept
        out += [(int(x), int(y), float(s), tid) for x, y, s in cands]
    return sorted(out)


@pytest.fixture(scope="module")
def sc():
    return mr.scene(W, H, T)


@pytest.mark.parametrize("nf0", [63, 64, 150])
@pytest.mark.parametrize("mods", mr.SETS, ids=lambda m: m[0])
def test_empty_slot_construction_equals_brute_force(sc, mods, nf0):
    maps = mr.present_maps(sc["pyr"], mr.KIND[mods[0]])
    bank = mr.make_bank(5, 3, 0, maps, T, nf0)
    lms, sizes = mr.linear_memories(maps, T)
    raw, canon, st = mr.oracle_match(bank, T, lms, sizes, 60.0)
    assert len(raw) > 0 and len(set(raw["sim"].tolist())) > 1 and st["coarse_candidates"] > 0
    assert mr.multiset(raw) == brute(maps, T, bank, 60.0)


@pytest.mark.skipif(not ll_ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("nf0", [63, 150])
@pytest.mark.parametrize("mods", mr.SETS, ids=lambda m: m[0])
def test_empty_slot_construction_through_the_reference(mods, nf0):
    """The same construction through the reference's own match lines: quantised maps (present, zeros), templates (present, no features).
    At 640 x 480: the reference reads past the last phase row of a label's memory, and on the small frame its heap blocks are
    small enough for that read to leave them — the two-modality bank crashes it there just the same."""
    s = mr.scene(640, 480, T)
    maps = mr.present_maps(s["pyr"], mr.KIND[mods[0]])
    bank = mr.make_bank(6, 6, 2, maps, T, nf0)
    lms, sizes = mr.linear_memories(maps, T)
    raw, canon, st = mr.oracle_match(bank, T, lms, sizes, 60.0)
    assert len(raw) > 0
    quant = [(m, np.zeros_like(m)) for m in maps]
    got = ll_ref.match(quant, list(T), {"obj": lo.pack_bank(mr.two_slot(bank), len(T))}, 60.0, ["obj"], pre_unique=True)
    assert mr.multiset(got) == mr.multiset(raw)


def test_the_geometry_passes_the_oracles_asserts(sc):
    """208 x 176 with T = (4, 8): 52 columns at level 0 (no multiple of 16), 13 at level 1 (whole bytes, no whole dwords)."""
    maps = mr.present_maps(sc["pyr"], 0)
    assert [m.shape[1] // t for m, t in zip(maps, T)] == [52, 13]
    mr.linear_memories(maps, T)                              # raises on (rows * cols) % 16 and on rows / cols % T


def test_crop_over_present_templates_differs_from_the_pairs_colour_half():
    """On a view whose normal features reach further out than its colour features, the colour-only template has other coordinates (and
    another size) than the colour templates of the two-modality pyramid: the comparison of test_gpu_modalities' training test can fail."""
    rgb, dep, mask = mr.view(3, colour_quadrant=True)
    od = lo.OracleDetector(32, list(T))
    single = mr.train_expect(od, rgb, dep, mask, 0)
    assert single is not None and od.addTemplate([rgb, dep], "pair", mask) == 0
    pair = od.class_templates["pair"][0]
    for l in range(len(T)):
        assert len(single[l].features) == len(pair[2 * l].features) == 32 >> l
        assert (single[l].width, single[l].height) != (pair[2 * l].width, pair[2 * l].height)
        assert not np.array_equal(single[l].features, pair[2 * l].features)
        d = pair[2 * l].features[:, :2] - single[l].features[:, :2]          # the same features, shifted by the difference of the two boxes' origins
        assert (d == d[0]).all() and d[0].any() and np.array_equal(single[l].features[:, 2], pair[2 * l].features[:, 2])


@pytest.mark.parametrize("mods", mr.SETS, ids=lambda m: m[0])
def test_training_views_succeed_and_fail_where_the_gpu_tests_expect(mods):
    kind = mr.KIND[mods[0]]
    od = lo.OracleDetector(32, list(T))
    for seed in (1, 2, 3):
        assert mr.train_expect(od, *mr.view(seed), kind) is not None
    easy = mr.view(4, flat_depth=True) if kind == 0 else mr.view(4, flat_colour=True)      # the ABSENT modality finds nothing here
    assert mr.train_expect(od, *easy, kind) is not None and mr.train_expect(od, *easy, 1 - kind) is None
    hard = mr.view(5, flat_colour=True) if kind == 0 else mr.view(5, flat_depth=True)      # the present one finds nothing
    assert mr.train_expect(od, *hard, kind) is None
