"""tests/pose_pixel_cases.py proved on the oracle alone (CPU): every case holds the pixels, the empty renders and the chunk counts it claims,
so that tests/test_gpu_pose_pixels.py means what it says; and the chunked tables tell a wrong index map from the right one.

Run time of this file: 4.5 s on one core (the 2048 x 1024 case: 1.6 s of it, for 9 renders and 20 pairs of 2 Mpixel distance images; its blob
is 100 pixels across, so the renders themselves cost milliseconds)."""
import os
import re

import numpy as np
import pytest

import pose_error_ref as per
import pose_pixel_cases as pc
import pose_sym_ref as psr

F32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "6dpose_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_quoted_constants_are_the_sources():
    cpp, hip, hdr = source("pose_error.cpp"), source("pose_error.hip"), source("pose_error_kernels.h")
    assert re.search(r"kZbufBudget = \(size_t\)512 << 20;", cpp) and pc.ZBUF_BUDGET == 512 << 20
    assert re.search(r"kMaxViewsPerRender = 256;", cpp) and pc.MAX_VIEWS_PER_RENDER == 256
    assert re.search(r"kMaxPtsPairs = 16384;", cpp) and pc.MAX_PTS_PAIRS == 16384
    assert re.search(r"kSymPartialBudget = \(size_t\)256 << 20;", cpp) and pc.SYM_PARTIAL_BUDGET == 256 << 20
    assert re.search(r"std::max<size_t>\(2, std::min<size_t>\(kMaxViewsPerRender, kZbufBudget / per\)\)", cpp)
    assert re.search(r"gch = std::min\(n_gt, std::max\(1, cap / 2\)\); ech = std::min\(n_est, cap - gch\);", cpp)
    assert re.search(r"kSymThreads = 256,", hdr) and pc.SYM_THREADS == 256
    assert re.search(r"kPixThreads = 256;", hdr) and pc.PIX_THREADS == 256
    assert re.search(r"\(npx \+ 4 \* kPixThreads - 1\) / \(4 \* kPixThreads\)", hip) and pc.PIX_PER_LANE == 4
    assert re.search(r"b > 128 \? 128 : b", hip) and pc.MAX_PIX_BLOCKS == 128


# ---- frame sizes -----------------------------------------------------------------------------------------------------------------------------
def test_frame_sizes_sit_on_the_grid_edges():
    blocks = {n: pc.pix_blocks(W * H) for n, (W, H, _) in pc.FRAMES.items()}
    assert blocks == {"1x1": 1, "7x5": 1, "32x32": 1, "41x25": 2, "257x3": 1, "100x77": 8, "512x256": 128, "513x256": 128}
    assert 32 * 32 == 1024 and 41 * 25 == 1025                           # the last frame of one block and the first of two
    assert 512 * 256 == pc.MAX_PIX_BLOCKS * pc.PIX_PER_LANE * pc.PIX_THREADS and 513 * 256 > 512 * 256   # 4 pixels per lane, then a fifth
    assert 1 * 1 < pc.PIX_THREADS and 7 * 5 < pc.PIX_THREADS and 257 * 3 < 4 * pc.PIX_THREADS   # lanes that idle
    assert all(W % 64 for W in (1, 7, 41, 257, 100, 513))
    K = pc.FRAMES["257x3"][2]
    assert K[0, 0] != K[1, 1]
    for name, (W, H, K) in pc.FRAMES.items():
        on_column = K[0, 2] == int(K[0, 2]) and 0 <= K[0, 2] < W
        assert on_column == (name == "100x77"), name
        if name != "100x77":
            assert K[0, 2] != int(K[0, 2]) and K[1, 2] != int(K[1, 2])


@pytest.mark.parametrize("name", pc.FRAME_NAMES)
def test_frame_cases_decide_something(name):
    c, x = pc.frame_case(name), pc.frame_expected(name)
    assert x["gd"][1][-1, -1] > 0, "the last pixel of the frame must be rendered: it is the one a strided lane reaches last"
    assert x["gd"][0][(c["H"] - 1) // 2, (c["W"] - 1) // 2] > 0
    assert c["scene"].dtype == F32 and c["scene"].shape == (c["H"], c["W"])
    if name == "1x1":
        return
    st = x["stats"]
    assert all(0 < s["px_count_visib"] < s["px_count_valid"] < s["px_count_all"] for s in st), st    # holes, occluded and visible pixels
    assert 0.0 < x["vsd"][0, 0] < 1.0 and x["vsd"][3, 0] == 0.0 and 0.0 < x["cou"][0, 0] < 1.0
    assert x["vsd_tlinear"][0, 0] != x["vsd"][0, 0]
    if name == "100x77":                                                 # the rendered column on which (u - cx) == 0
        assert (x["gd"][0][:, 50] > 0).any()


# ---- delta at equality -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", pc.DELTA_SIDES)
def test_delta_cases_hold_a_pixel_on_the_boundary_and_one_on_each_side(side):
    c = pc.delta_case(side)
    lo, v, hi = (F32(d) for d in c["deltas"])
    assert float(lo) == c["deltas"][0] and float(v) == c["deltas"][1] and float(hi) == c["deltas"][2]     # float32 values, passed exactly
    assert lo == np.nextafter(v, F32(-np.inf)) and hi == np.nextafter(v, F32(np.inf)) and lo < v < hi
    Dm, Dt = per.dist_image(c["model_depth"], c["K"]), per.dist_image(c["scene"], c["K"])
    valid = (Dm > 0) & (Dt > 0)
    d32 = Dm.astype(F32) - Dt.astype(F32)
    px = c["pixels"]
    assert d32[px["occurs"]] == v and d32[px["at"]] == v and d32[px["below"]] == lo and d32[px["above"]] == hi
    assert all(valid[p] for p in px.values()) and len(set(px.values())) == 4
    # the model's render is the GT's for "gt" and the estimate's for "est"; the other pose renders nothing on the four pixels
    V, F = pc.mesh()
    mine = (c["gR"], c["gt"]) if side == "gt" else (c["eR"], c["et"])
    other = (c["eR"], c["et"]) if side == "gt" else (c["gR"], c["gt"])
    assert np.array_equal(pc.render(V, F, c["K"], mine[0][0], mine[1][0], c["W"], c["H"]), c["model_depth"])
    od = pc.render(V, F, c["K"], other[0][0], other[1][0], c["W"], c["H"])
    assert all(od[p] == 0 for p in px.values()) and (od > 0).any() and ((od > 0) & (c["model_depth"] > 0)).any()
    # a `<` for `<=` and a difference taken in float64 each change the count at delta = v
    n_le = int((valid & (d32 <= v)).sum())
    assert int((valid & (d32 < v)).sum()) <= n_le - 2
    assert (Dm - Dt)[px["at"]] > np.float64(v)
    assert int((valid & ((Dm - Dt) <= np.float64(v))).sum()) != n_le
    # differences on both sides of the boundary are plentiful
    assert int((valid & (d32 < lo)).sum()) > 50 and int((valid & (d32 > hi)).sum()) > 50
    # the three neighbouring deltas give three different unions
    x = pc.delta_expected(side)
    unions = [t["counts"][0][0]["union"] for t in x]
    assert unions[0] + 2 == unions[1] and unions[1] + 1 == unions[2], unions
    if side == "gt":
        vis = [t["stats"][0]["px_count_visib"] for t in x]
        assert vis[0] + 2 == vis[1] and vis[1] + 1 == vis[2], vis


# ---- tau at equality ---------------------------------------------------------------------------------------------------------------------------
def test_tau_case_holds_a_cost_on_the_threshold():
    c, x = pc.tau_case(), pc.tau_expected()
    below, at, above = c["taus"]
    assert c["inter"][c["pixel"]] and c["cost"][c["pixel"]] == at and abs(at - 20.0) < 0.05
    assert below == np.nextafter(at, 0.0) and above == np.nextafter(at, np.inf)          # the same pixel: one ulp above, at, one ulp below tau
    counts = [t["counts"][0][0] for t in x]
    assert counts[0]["union"] == counts[2]["union"] and counts[0]["inter"] == counts[2]["inter"] > 500
    assert counts[1]["step"] == counts[2]["step"] + 1, counts              # cost >= tau: true at tau = cost, false one ulp above
    assert counts[0]["step"] == counts[1]["step"]
    assert counts[0] != counts[1]                                         # the tlinear sum moves with 1 / tau
    assert at * (1.0 / below) >= 1.0 and at * (1.0 / above) < 1.0         # the clamp of min(cost / tau, 1) acts at one tau and not at the other
    assert 0 < counts[1]["step"] < counts[1]["inter"]
    assert x[1]["vsd"][0, 0] != x[2]["vsd"][0, 0] and x[1]["vsd_tlinear"][0, 0] != x[1]["vsd"][0, 0]


# ---- hostile scenes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_every_hostile_value_lands_on_a_rendered_pixel(dtype):
    c, x = pc.hostile_case(dtype), pc.hostile_expected(dtype)
    assert c["scene"].dtype == np.dtype(dtype)
    dg, de = x["gd"][0], x["ed"][0]
    rows = np.array([str(k) for k in c["kind_of_row"]])
    for k in c["kinds"]:
        ys = np.flatnonzero(rows == str(k))
        for d in (dg, de):                                               # each kind of row crosses both silhouettes
            on, off = (d[ys] > 0).any(1), (d[ys] == 0).any(1)
            assert (on & off).any(), (k, ys)
        if not isinstance(k, str):
            got = c["scene"][ys]
            assert np.isnan(got).all() if k != k else (got == F32(k)).all(), k
    if dtype == "uint16":
        assert set(np.unique(c["scene"])) >= {0, 1, 65535}
        return
    s = c["scene"]
    Dt = pc.quiet(per.dist_image, s, c["K"])
    with np.errstate(all="ignore"):
        Dt32 = Dt.astype(F32)
    inf_rows, neg_rows, max_rows, den_rows = (np.flatnonzero(rows == str(k)) for k in (float("inf"), "neg", pc.FLT_MAX, pc.DENORMAL))
    assert (s[neg_rows] < 0).all() and (Dt[neg_rows] > 0).all()          # negative depth, positive distance: valid for pysixd
    y = next(int(y) for y in inf_rows if dg[y, 24] > 0)
    assert np.isnan(Dt[y, 24]) and np.isinf(Dt[y, 23]) and np.isinf(Dt[y, 25])     # (u - cx) == 0 times inf
    assert np.isfinite(Dt[max_rows]).all() and np.isinf(Dt32[max_rows]).any()     # finite in float64, beyond float32 after the cast
    assert (s[den_rows] > 0).all() and (s[den_rows] < np.finfo(F32).tiny).all() and (Dt[den_rows] > 0).all()
    # a mirrored negative scene is visible where it mirrors the render; the union counts those pixels
    vis_g = pc.quiet(per.visib_mask, Dt, per.dist_image(dg, c["K"]), 15.0)
    assert vis_g[neg_rows].any() and vis_g[inf_rows].any() and not vis_g[np.flatnonzero(rows == "0.0")].any()
    assert np.isfinite(x["vsd"]).all() and np.isfinite(x["vsd_tlinear"]).all()


# ---- empty results -----------------------------------------------------------------------------------------------------------------------------
def test_empty_cases_are_empty_for_the_stated_reason():
    c, x = pc.empty_case(), pc.empty_expected()
    V, F = pc.mesh()
    W, H, K = c["W"], c["H"], c["K"]
    g, e = pc.EMPTY_GT.index, pc.EMPTY_EST.index
    st = x["stats"]
    # beyond clip_far: nothing at 2000, something at 10000
    assert not x["gd"][g("beyond_far")].any() and pc.render(V, F, K, c["gR"][1], c["gt"][1], W, H, 100.0, 10000.0).any()
    # in front of clip_near: nothing at 100, something at 1; every vertex in front of the camera (no triangle is dropped for that)
    assert not x["ed"][e("before_near")].any() and pc.render(V, F, K, c["eR"][1], c["et"][1], W, H, 1.0, 2000.0).any()
    z = (V.astype(np.float64) @ c["eR"][1].T + c["et"][1])[:, 2]
    assert 0.0 < z.min() and z.max() < pc.EMPTY_NEAR
    # outside the frame: the projected box ends left of column 0
    assert not x["gd"][g("outside")].any() and st[g("outside")]["bbox_obj"][0] + st[g("outside")]["bbox_obj"][2] < 0
    assert not x["ed"][e("outside")].any()
    for k in ("beyond_far", "outside"):
        assert st[g(k)]["px_count_all"] == 0 and st[g(k)]["visib_fract"] == 0.0 and st[g(k)]["bbox_visib"] == [-1, -1, -1, -1]
    # fully occluded: rendered, every pixel valid, none visible
    s = st[g("occluded")]
    assert s["px_count_all"] == s["px_count_valid"] > 100 and s["px_count_visib"] == 0 and s["bbox_visib"] == [-1, -1, -1, -1]
    # one pixel: the one the scene leaves uncovered
    s = st[g("one_pixel")]
    assert s["px_count_visib"] == 1 and s["px_count_all"] > 100 and s["bbox_visib"] == [c["one"][1], c["one"][0], 0, 0]
    assert c["scene"][c["one"]] > x["gd"][g("one_pixel")][c["one"]]
    # an empty estimate against a visible GT; both empty; the one-pixel pose against itself
    assert x["counts"][e("before_near")][g("visible")]["union"] > 100 and x["counts"][e("before_near")][g("visible")]["inter"] == 0
    assert x["vsd"][e("before_near"), g("visible")] == 1.0 and x["cou"][e("before_near"), g("visible")] == 1.0
    assert x["counts"][e("before_near")][g("beyond_far")]["union"] == 0
    assert x["vsd"][e("before_near"), g("beyond_far")] == 1.0 and x["cou"][e("before_near"), g("beyond_far")] == 1.0
    assert x["counts"][e("one_pixel")][g("one_pixel")]["union"] == 1 and x["vsd"][e("one_pixel"), g("one_pixel")] == 0.0
    assert 0.0 < x["vsd"][e("visible"), g("visible")] < 1.0


# ---- options -----------------------------------------------------------------------------------------------------------------------------------
def test_options_change_the_answers():
    unions = [pc.option_expected(delta=d)["counts"][0][0]["union"] for d in pc.OPTION_DELTAS]
    order = np.argsort(pc.OPTION_DELTAS)
    assert all(unions[a] < unions[b] for a, b in zip(order[:-1], order[1:])), unions       # -5 < 0 < 15 < 1e9: strictly more visible pixels
    steps = [pc.option_expected(tau=t)["counts"][0][0]["step"] for t in pc.OPTION_TAUS]
    inter = pc.option_expected()["counts"][0][0]["inter"]
    assert steps[0] > steps[1] > steps[2] == 0 and steps[0] <= inter, steps
    whole = pc.option_expected()["gd"][0]
    z = whole[whole > 0]
    for near, far in pc.OPTION_CLIPS:
        assert F32(near) == near and F32(far) == far
        cut = pc.option_expected(near=near, far=far)["gd"][0]
        assert 0 < (cut > 0).sum() < (whole > 0).sum()                   # the planes cut through the blob
        assert z.min() < max(near, z.min()) or z.max() > far
        assert ((cut > 0) & (cut != whole)).any() or near == 100.0      # behind the near plane the far side of the blob shows


# ---- chunked paths -----------------------------------------------------------------------------------------------------------------------------
def check_periods(chunks, period):
    """The period divides no size and no offset of a loop that runs more than once."""
    if len(chunks) > 1:
        assert all(n % period for _, n in chunks) and all(o % period for o, _ in chunks[1:]), (chunks, period)


def test_the_counts_exceed_the_caps_and_the_chunks_are_as_stated():
    assert pc.views_per_render(48, 40) == 256 and pc.views_per_render(2048, 1024) == 32 and pc.views_per_render(320, 240) == 256
    want = {"a_200x60": ((60, 196), [(0, 60)], [(0, 196), (196, 4)]),
            "b_5x300": ((128, 5), [(0, 128), (128, 128), (256, 44)], [(0, 5)]),
            "c_140x140": ((128, 128), [(0, 128), (128, 12)], [(0, 128), (128, 12)]),
            "e_2048x1024": ((4, 28), [(0, 4)], [(0, 28), (28, 2)])}
    for name, (W, H, n_est, n_gt, pe, pg) in pc.CHUNKED_VSD.items():
        assert n_est + n_gt > pc.views_per_render(W, H), name
        gch, ech = pc.vsd_chunking(n_est, n_gt, W, H)
        gc, ec = pc.chunks_of(n_gt, gch), pc.chunks_of(n_est, ech)
        assert ((gch, ech), gc, ec) == want[name], name
        assert max(ng for _, ng in gc) + max(ne for _, ne in ec) <= pc.views_per_render(W, H)
        check_periods(gc, pg)
        check_periods(ec, pe)
    assert pc.chunks_of(pc.GT_STATS_N, pc.views_per_render(48, 40)) == [(0, 256), (256, 44)]
    check_periods(pc.chunks_of(pc.GT_STATS_N, 256), pc.PERIOD_GT)
    n = pc.PTS_SHAPE[0] * pc.PTS_SHAPE[1]
    assert n == 18000 and pc.chunks_of(n, pc.MAX_PTS_PAIRS) == [(0, 16384), (16384, 1616)] and len(pc.pts_case()["V"]) == 12
    s = pc.sym_case()
    assert s["n_sym"] == psr.disc_count(pc.SYM_STEP) - 1 == 3141 and len(s["V"]) == 8
    batch = pc.sym_batch(8, 2, s["n_sym"])
    assert batch == (256 << 20) // 8 // (2 * 3141) == 5341 < pc.MAX_PTS_PAIRS               # the partial budget binds, not the pair limit
    assert pc.chunks_of(pc.SYM_SHAPE[0] * pc.SYM_SHAPE[1], batch) == [(0, 5341), (5341, 1659)]
    for small in (pc.sym_batch(8, 1, s["n_sym"]), pc.sym_batch(8, 2, 24)):
        assert small > 7000                                              # one metric alone, or a small set: one batch


APPLICABLE = {"a_200x60": ("drop_e0", "swap_div_mod", "ech_for_short_ne"), "b_5x300": ("drop_g0", "swap_div_mod"),
              "c_140x140": pc.VSD_MISTAKES, "e_2048x1024": ("drop_e0", "swap_div_mod", "ech_for_short_ne")}


@pytest.mark.parametrize("name", pc.CHUNKED_VSD_NAMES)
def test_chunked_tables_tell_a_wrong_index_map(name):
    W, H, n_est, n_gt, pe, pg = pc.CHUNKED_VSD[name]
    gch, ech = pc.vsd_chunking(n_est, n_gt, W, H)
    se, sg, written = pc.vsd_sources(n_est, n_gt, gch, ech)
    assert written.all() and np.array_equal(se, np.arange(n_est)[:, None].repeat(n_gt, 1)) and np.array_equal(sg, np.arange(n_gt)[None].repeat(n_est, 0))
    T = pc.chunked_vsd_distinct(name)
    assert {m for m in pc.VSD_MISTAKES if m not in APPLICABLE[name]} == {m for m in pc.VSD_MISTAKES
                                                                         if all(np.array_equal(a, b) for a, b in zip(pc.vsd_sources(n_est, n_gt, gch, ech, m), (se, sg, written)))}
    for key in ("vsd", "vsd_tlinear", "cou"):
        want = pc.expand(T[key], se, sg, pe, pg)
        assert len(np.unique(T[key])) >= min(pe, pg), key
        for m in APPLICABLE[name]:
            me, mg, mw = pc.vsd_sources(n_est, n_gt, gch, ech, m)
            wrong = pc.expand(T[key], me, mg, pe, pg)
            if (name, m) == ("e_2048x1024", "ech_for_short_ne"):       # 4 GTs x 2 estimates read as rows of 28: the two pairs that stay in
                assert (want[~mw] != 0.0).all() and (~mw).sum() == 6       # bounds are right, the six others are never written and read 0.0
                continue
            assert mw.any() and (wrong != want)[mw].any(), (name, key, m)   # not only the cells a mistake leaves unwritten


def test_the_2048_frame_renders_its_last_pixel():
    T = pc.chunked_vsd_distinct("e_2048x1024")
    assert T["gd"][3][-1, -1] > 0 and all(0.0 < T["vsd"][i, i % 4] < 1.0 for i in range(5))
    assert pc.pix_blocks(2048 * 1024) == 128


def test_chunked_gt_stats_pts_and_sym_tell_a_dropped_offset():
    g = pc.gt_stats_case()
    rows = np.array([[s["px_count_all"], s["px_count_valid"], s["px_count_visib"]] + s["bbox_obj"] + s["bbox_visib"] for s in g["stats"]])
    assert len({tuple(r) for r in rows}) == pc.PERIOD_GT and all(0 < s["px_count_visib"] < s["px_count_all"] for s in g["stats"])
    ok, bad = pc.gt_sources(pc.GT_STATS_N, 256), pc.gt_sources(pc.GT_STATS_N, 256, "drop_g0")
    assert np.array_equal(ok, np.arange(pc.GT_STATS_N))
    assert (rows[bad[bad >= 0] % pc.PERIOD_GT] != rows[ok[bad >= 0] % pc.PERIOD_GT]).any()
    p, s = pc.pts_case(), pc.sym_case()
    for shape, batch, tables in ((pc.PTS_SHAPE, pc.MAX_PTS_PAIRS, (p["add"], p["adi"])), (pc.SYM_SHAPE, pc.sym_batch(8, 2, s["n_sym"]), (s["mssd"], s["mspd"]))):
        n = shape[0] * shape[1]
        ok, bad = pc.flat_sources(n, batch), pc.flat_sources(n, batch, "drop_p0")
        assert np.array_equal(ok, np.arange(n))
        for T in tables:
            assert T.shape == (pc.PERIOD_EST, pc.PERIOD_GT) and len(np.unique(T)) == T.size
            w = bad >= 0
            assert np.abs(pc.flat_expand(T, bad, shape[1]) - pc.flat_expand(T, ok, shape[1]))[w].max() > 1.0     # far beyond the 1e-4 / 1e-9 bars


def test_the_batched_symmetry_oracle_is_the_loop():
    s = pc.sym_case()
    a = psr.errors(s["eR"][:2], s["et"][:2], s["gR"][:2], s["gt"][:2], pc.SYM_K, s["V"].astype(np.float64), s["Rs"][::97], s["ts"][::97])
    b = psr.errors_batched(s["eR"][:2], s["et"][:2], s["gR"][:2], s["gt"][:2], pc.SYM_K, s["V"].astype(np.float64), s["Rs"][::97], s["ts"][::97])
    for k in ("mssd", "mspd"):
        assert np.abs(a[k] - b[k]).max() <= 1e-11 and a[k].min() > 0.0
