"""GPU tests (`-m gpu`) of the batched coarse kernel, k_coarse_bits_batch: every case runs the same frames and bank
through a detector forced onto the batched kernel and one forced onto k_coarse_bits (Detector.setCoarseBatch) and compares, per frame, the
coarse candidates as sets of (x, y, score bits, work), the candidate counters, the layout of a template's candidates in the frame's buffer
(one contiguous slot range, raster order: what k_local_bits's L2 locality rests on) and the final records byte for byte; the small cases also
against the CPU oracle.  Frames and banks are synthetic (synth.py); the shapes are the smallest that reach every edge of the kernel: 300
positions (10 lanes: several frames in one wave), VGA's 1200 (38 lanes: a wave straddles up to three frames), 4800 (150 lanes: a frame
spans waves, eight frames are two groups of four), batches of 1, 2, 3, 5 and 8 frames, 23 templates (no multiple of a workgroup's), a template
as large as the map, one whose sums cover the whole map, a threshold below zero (every position a hit), a buffer smaller than the hits, 511
and 512 features per entry (both counter widths) and the low weights 1, 2 and 3.

The layout check holds for k_coarse_bits too wherever the map fits its one pass of 2048 positions; beyond (the 4800-position case) its passes
reserve their slots one after the other, other workgroups in between, so there it is asserted for the batched kernel alone."""
import functools
import os

import numpy as np
import pytest

import linemod_oracle as lo
import response_table_ref as rt
import synth

pytestmark = pytest.mark.gpu

T2 = [4, 8]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


@functools.lru_cache(maxsize=None)
def frames_of(W, H, distinct):
    return [synth.make_frame(500 + 7 * i, W, H, n_poly=max(8, 40 * W // 640)) for i in range(distinct)]


def boxed_bank(seed, boxes, nfeat):
    """One random-feature pyramid per (w, h) box at level 0 (synth.make_random_bank with chosen sizes); nfeat[l] = (colour, normals) counts."""
    rng = np.random.default_rng(seed)
    feats, whs = [], []
    for w, h in boxes:
        lv = []
        for l, nf in enumerate(nfeat):
            wl, hl = max(2, w >> l), max(2, h >> l)
            lv.append([np.stack([rng.integers(0, wl + 1, n), rng.integers(0, hl + 1, n), rng.integers(0, 8, n)], 1) for n in nf])
        f, wh = synth._crop_pack(lv)
        feats += f
        whs += wh
    return synth._finish(feats, whs)


def concat_banks(*banks):
    feat = np.concatenate([b[0] for b in banks], 0)
    lens = np.concatenate([np.diff(b[1]) for b in banks])
    offs = np.zeros(len(lens) + 1, np.int32)
    offs[1:] = np.cumsum(lens)
    return np.ascontiguousarray(feat), offs, np.concatenate([b[2] for b in banks], 0)


@functools.lru_cache(maxsize=None)
def small_bank():
    """23 templates on 320 x 240 (top level 20 x 15 = 300 positions): 20 cut out of the first frame, a template as large as the map (its sums
    cover 22 positions), one of a single top-level cell (sums at every position: limit == positions) and one in between."""
    rgb, dep = frames_of(320, 240, 8)[0]
    pyr = lo.OracleDetector(64, T2).quantize_pyramid(rgb, dep)
    planted = synth.make_planted_bank(11, 20, [(p[0], p[1]) for p in pyr], T2, nfeat=(64, 32))
    odd = boxed_bank(12, [(300, 220), (14, 14), (120, 90)], ((64, 64), (32, 32)))
    return concat_banks(planted, odd)


@functools.lru_cache(maxsize=None)
def wide_counter_bank(nf_top):
    """five random templates whose top-level entries have nf_top features: 511 = the 9-bit counters' last, 512 = the 14-bit instantiation's first"""
    return boxed_bank(13, [(150, 110), (90, 140), (200, 60), (64, 64), (130, 131)], ((48, 48), (nf_top - nf_top // 2, nf_top // 2)))


@functools.lru_cache(maxsize=None)
def vga_bank():
    rgb, dep = frames_of(640, 480, 3)[0]
    pyr = lo.OracleDetector(64, T2).quantize_pyramid(rgb, dep)
    return concat_banks(synth.make_planted_bank(21, 24, [(p[0], p[1]) for p in pyr], T2, nfeat=(64, 32)),
                        boxed_bank(22, [(600, 440), (15, 15), (200, 300)], ((64, 64), (32, 32))))


@functools.lru_cache(maxsize=None)
def big_bank():
    return boxed_bank(31, [(300, 200), (15, 15), (1200, 900), (500, 640), (90, 70)], ((64, 64), (32, 32)))


def run(lm, W, H, bank, nb, thr, mode, table=None, capacity=None, distinct=8):
    """nb frames as ONE batch launch on a fresh detector: per frame (records or None after an overflow, candidates produced, candidate
    records in slot order); whether the batched kernel ran."""
    src = frames_of(W, H, distinct)
    frames = [src[i % len(src)] for i in range(nb)]
    det = lm.Detector(64, T2, device=0)
    det.addClassPacked("obj", *bank)
    if table is not None:
        det.setResponseTable(table)
    if capacity is not None:
        det.setCandidateCapacity(capacity)
    det.setCoarseBatch(mode)
    det.setBatch(nb)
    det.setBatchQueue(0)                                  # full batches only: all nb frames in one launch
    first = det.framesSubmitted()
    for f in frames:
        det.submitFrame(list(f), thr, ["obj"])
    out = []
    for i in range(nb):
        try:
            rec = det.collect()
        except RuntimeError as e:
            assert "overflow" in str(e), e
            rec = None
        assert det.lastTimings()["batch_frames"] == nb or rec is None
        out.append(rec)
    assert det.getPaths() == ("bits", "bits")
    cands = [det.readCandidates(first + i) for i in range(nb)]
    return [(out[i],) + cands[i] for i in range(nb)], det.coarseBatched()


def cand_set(c):
    return sorted(zip(c["x"].tolist(), c["y"].tolist(), c["score"].view(np.uint32).tolist(), c["work"].tolist()))


def assert_templates_contiguous(c, what):
    """in slot order: the records of a work item are consecutive and ascend in (y, x)"""
    work = c["work"]
    change = np.flatnonzero(np.diff(work) != 0) + 1
    runs = np.split(np.arange(len(c)), change)
    seen = [int(work[r[0]]) for r in runs if len(r)]
    assert len(seen) == len(set(seen)), "%s: a template's candidates lie in more than one slot range" % what
    key = c["y"].astype(np.int64) * 65536 + c["x"]
    same = np.diff(work) == 0
    assert np.all(np.diff(key)[same] > 0), "%s: a template's candidates are not in raster order" % what


def compare(lm, W, H, bank, nb, thr, table=None, capacity=None, distinct=8, oracle=False):
    a, a_batched = run(lm, W, H, bank, nb, thr, True, table, capacity, distinct)
    b, b_batched = run(lm, W, H, bank, nb, thr, False, table, capacity, distinct)
    assert a_batched and not b_batched
    one_pass = (W // 2 // T2[1]) * (H // 2 // T2[1]) <= 2048
    hits = 0
    for i, ((ra, na, ca), (rb, nb_, cb)) in enumerate(zip(a, b)):
        print("frame %d: %d candidates, %d records" % (i, na, -1 if ra is None else len(ra)))
        assert na == nb_, "frame %d: counters %d (batched) and %d (per frame)" % (i, na, nb_)
        hits += na
        assert_templates_contiguous(ca, "batched, frame %d" % i)
        if one_pass:
            assert_templates_contiguous(cb, "per frame, frame %d" % i)
        if capacity is not None and na > capacity:
            assert ra is None and rb is None and len(ca) == len(cb) == capacity       # nothing beyond the buffer, everything inside it
            continue
        assert len(ca) == na and cand_set(ca) == cand_set(cb), "frame %d" % i
        assert ra is not None and rb is not None and ra.tobytes() == rb.tobytes(), "frame %d" % i
    assert hits > 0
    if oracle:
        od = lo.OracleDetector(64, T2)
        pb = lo.PackedBank((len(bank[1]) - 1) // (2 * len(T2)), len(T2), *bank)
        src = frames_of(W, H, distinct)
        for i in range(nb):
            rgb, dep = src[i % len(src)]
            lms, sizes = rt.linear_memories(od.quantize_pyramid(rgb, dep), T2, tuple(table or rt.DEFAULT))
            raw, _ = lo.match_bank_c(pb, lms, sizes, T2, thr)
            want = lo.canonical_sort_unique(raw)
            got = a[i][0]
            assert len(got) == len(want), (i, len(got), len(want))
            for g, w in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("template_id", "tid")):
                assert np.array_equal(got[g], want[w]), (i, g)


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8])
def test_small_map_every_batch_size(lm, nb):
    """300 positions = 10 lanes per frame: up to 6.4 frames per wave; 23 templates; the oracle on the batch of three"""
    compare(lm, 320, 240, small_bank(), nb, 60.0, oracle=(nb == 3))


@pytest.mark.parametrize("table", [(4, 2, 0, 0, 0), (4, 3, 3, 0, 0)], ids=["a2", "a3"])
def test_low_weights_two_and_three(lm, table):
    compare(lm, 320, 240, small_bank(), 3, 66.0, table=table, oracle=True)


def test_a_threshold_that_zero_passes(lm):
    """threshold < 0: every position of the map is a hit of every template, the positions without sums included"""
    compare(lm, 320, 240, small_bank(), 5, -1.0)


def test_a_buffer_smaller_than_the_hits(lm):
    """23 x 300 hits per frame into buffers of 2048: the counters count on, nothing is written past the buffer"""
    compare(lm, 320, 240, small_bank(), 5, -1.0, capacity=2048)


@pytest.mark.parametrize("nf_top", [511, 512])
def test_both_counter_widths(lm, nf_top):
    compare(lm, 320, 240, wide_counter_bank(nf_top), 3, 40.0, oracle=True)


@pytest.mark.parametrize("nb", [3, 8])
def test_vga(lm, nb):
    """1200 positions = 38 lanes: 8 frames are 304 lanes in 5 waves, a wave straddles up to three frames; 27 templates"""
    compare(lm, 640, 480, vga_bank(), nb, 60.0, distinct=3)


@pytest.mark.parametrize("nb", [2, 5, 8])
def test_a_frame_wider_than_a_wave(lm, nb):
    """1280 x 960: 4800 positions = 150 lanes, a frame spans three waves; five frames are one group of 750 lanes, eight are two of 600"""
    compare(lm, 1280, 960, big_bank(), nb, 30.0, distinct=2)


def test_the_launcher_rule(lm):
    """under the rule (setCoarseBatch(None)): a lone frame runs k_coarse_bits, two frames of 10 lanes share one wave and run the batched kernel"""
    for nb, want in ((1, False), (2, True)):
        _, batched = run(lm, 320, 240, small_bank(), nb, 60.0, None)
        assert batched == want, nb
