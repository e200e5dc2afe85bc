"""GPU tests (`-m gpu`) that drive k_coarse_wide (Detector.setPaths("wide", "wide"), table 4 3 2 1 0) to the edges of the coarse stages it shares
with k_coarse_bits / k_coarse_bits_batch (match_planes.h: template head, hit mask, slot reservation, emission): a threshold that zero passes
(every position of the map a hit, the positions without sums included), a candidate buffer smaller than the hits, a map of three passes whose
last pass lies partly beyond a template's sums, and the 14-bit instantiation of the hit mask (kS = 17).  test_gpu_coarse_batch.py drives the
same edges through the two-plane kernels only; its banks and frames are reused.  Expected values come from the CPU oracle on the linear
memories of this table (response_table_ref), never from another GPU path; the candidate count where it follows from the shapes."""
import numpy as np
import pytest

import linemod_oracle as lo
import response_table_ref as rt
from test_gpu_coarse_batch import T2, big_bank, frames_of, lm, small_bank, wide_counter_bank  # noqa: F401  (lm: the module's detector fixture)

pytestmark = pytest.mark.gpu

LINEMOD = (4, 3, 2, 1, 0)
WIDE = ("wide", "wide")


def run_wide(lm, W, H, bank, nb, thr, capacity=None, distinct=8):
    """nb frames as one batch launch on the wide paths: per frame (records, or None after an overflow; candidate counter; candidate records)"""
    frames = frames_of(W, H, distinct)[:nb]
    det = lm.Detector(64, T2, device=0)
    det.addClassPacked("obj", *bank)
    det.setPaths(*WIDE)
    det.setResponseTable(LINEMOD)
    if capacity is not None:
        det.setCandidateCapacity(capacity)
    det.setBatch(nb)
    det.setBatchQueue(0)
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
        out.append(rec)
    assert det.getPaths() == WIDE
    return [(out[i],) + tuple(det.readCandidates(first + i)) for i in range(nb)]


def oracle_records(W, H, bank, i, thr, distinct=8):
    od = lo.OracleDetector(64, T2)
    pb = lo.PackedBank((len(bank[1]) - 1) // (2 * len(T2)), len(T2), *bank)
    rgb, dep = frames_of(W, H, distinct)[i]
    lms, sizes = rt.linear_memories(od.quantize_pyramid(rgb, dep), T2, LINEMOD)
    raw, _ = lo.match_bank_c(pb, lms, sizes, T2, thr)
    return lo.canonical_sort_unique(raw)


def assert_equals_oracle(got, want, what):
    assert got is not None and len(got) == len(want), (what, None if got is None else len(got), len(want))
    for g, w in (("x", "x"), ("y", "y"), ("similarity", "sim"), ("template_id", "tid")):
        assert np.array_equal(got[g], want[w]), (what, g)


def test_a_threshold_that_zero_passes(lm):
    """320 x 240 (top level 20 x 15), threshold -1: every frame's counter is 23 x 300, every cell of the map once per template"""
    T, Wd, Hd = T2[1], 20, 15
    offset = T // 2 + (T % 2 - 1)
    cells = sorted((cx * T + offset, cy * T + offset) for cy in range(Hd) for cx in range(Wd))
    for i, (rec, n, c) in enumerate(run_wide(lm, 320, 240, small_bank(), 3, -1.0)):
        print("frame %d: %d candidates, %d records" % (i, n, len(rec)))
        assert n == 23 * 300 and len(c) == n, (i, n, len(c))
        for work in range(23):
            mine = c[c["work"] == work]
            assert sorted(zip(mine["x"].tolist(), mine["y"].tolist())) == cells, (i, work)
        assert_equals_oracle(rec, oracle_records(320, 240, small_bank(), i, -1.0), "frame %d" % i)


def test_a_buffer_smaller_than_the_hits(lm):
    """23 x 300 hits per frame into buffers of 2048: the counter counts on, exactly the buffer is written, collect reports the overflow"""
    for i, (rec, n, c) in enumerate(run_wide(lm, 320, 240, small_bank(), 3, -1.0, capacity=2048)):
        print("frame %d: %d candidates, %d in the buffer" % (i, n, len(c)))
        assert n == 23 * 300 and len(c) == 2048 and rec is None, (i, n, len(c))


def test_three_passes_and_a_last_pass_beyond_the_sums(lm):
    """1280 x 960: 4800 positions are three passes of 2048; the templates' sums end inside the last (the 1200 x 900 one's inside the first).
    Threshold 30: the oracle's list under this table is not empty (asserted)."""
    (rec, n, c), = run_wide(lm, 1280, 960, big_bank(), 1, 30.0, distinct=2)
    want = oracle_records(1280, 960, big_bank(), 0, 30.0, distinct=2)
    print("%d candidates, %d records, oracle %d" % (n, len(rec), len(want)))
    assert len(want) > 0 and len(c) == n
    assert_equals_oracle(rec, want, "1280 x 960")


def test_the_14_bit_hit_mask(lm):
    """512 features per top-level entry: k_coarse_wide<10, .>, sums of 17 bits"""
    (rec, n, c), = run_wide(lm, 320, 240, wide_counter_bank(512), 1, 40.0)
    want = oracle_records(320, 240, wide_counter_bank(512), 0, 40.0)
    print("%d candidates, %d records, oracle %d" % (n, len(rec), len(want)))
    assert len(want) > 0 and len(c) == n
    assert_equals_oracle(rec, want, "512 features")
