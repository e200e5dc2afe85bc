"""The two oracle functions the on-device NMS tests (tests/test_gpu_nms_oracle.py) take their verdicts from, checked on the CPU
against slow restatements that share no code with them: lo.nms_boxes against an O(n^2) greedy loop with rational IoU, and
lo.canonical_sort_unique against sorted() and a loop."""
from fractions import Fraction

import numpy as np
import pytest

import linemod_oracle as lo


def iou_exact(a, b):
    """IoU of two integer boxes x1, y1, x2, y2 with the driver's +1 pixel convention, as a rational number."""
    w = max(0, min(a[2], b[2]) - max(a[0], b[0]) + 1)
    h = max(0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    inter = w * h
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return Fraction(inter, union)


def suppresses(q, thresh):
    """The driver's rule `not (inter / union <= thresh)` in f64, stated exactly on the rational IoU q: the f64 quotient is rn(q),
    the correctly rounded q, and rn(q) <= thresh holds iff q does not lie beyond the point half way from thresh to the next double
    above it.  (q is never that half-way point itself: it would need 54 significant bits, and q = p / u with p, u < 2^34 and u a
    power of two has at most 34.)"""
    up = float(np.nextafter(np.float64(thresh), np.inf))
    return q > (Fraction(thresh) + Fraction(up)) / 2


def nms_brute(boxes, scores, thresh):
    """Greedy NMS restated: visit by score descending, among equal scores the HIGHER index first; a visited box that no kept box
    suppresses is kept.  thresh is the double the caller passes, taken exactly (Fraction(float) is exact).  Returns (keep, f64_bad,
    naive_bad): the pairs whose verdict by numpy's f64 quotient differs from `suppresses`, and from the naive rational rule q > thresh."""
    th = Fraction(thresh)
    order = sorted(range(len(boxes)), key=lambda i: (-scores[i], -i))
    keep, f64_bad, naive_bad = [], [], []
    for i in order:
        ok = True
        for k in keep:
            q = iou_exact(boxes[k], boxes[i])
            f = np.float64(q.numerator) / np.float64(q.denominator)
            sup = suppresses(q, thresh)
            if (not (f <= np.float64(thresh))) != sup:
                f64_bad.append((k, i, q, thresh))
            if (q > th) != sup:
                naive_bad.append((k, i, q, thresh))
            if sup:
                ok = False
                break
        if ok:
            keep.append(i)
    return keep, f64_bad, naive_bad


def random_boxes(rng, n, span, n_scores):
    x1 = rng.integers(-20, span, n); y1 = rng.integers(-20, span, n)
    w = rng.integers(0, 90, n); h = rng.integers(0, 90, n)
    boxes = np.stack([x1, y1, x1 + w, y1 + h], 1)
    scores = rng.integers(0, n_scores, n).astype(np.float32) / np.float32(7.0) + np.float32(50.0)
    return boxes, scores


@pytest.mark.parametrize("seed", range(6))
def test_nms_boxes_stable_equals_rational_greedy_loop(seed):
    """Heavy score ties (a handful of distinct scores), thresholds that occur exactly as an IoU among the boxes, their f64
    neighbours, 0, 1 and beyond.

    f64 against the exact rational, for integer boxes below 2^16: inter and union are integers below 2^34, exact in f64, so numpy's
    quotient is rn(p/u), the correctly rounded rational, and `suppresses` states rn(p/u) <= t exactly.  The two can only agree: the
    test asserts that no pair disagrees.  The NAIVE rule p/u > t is the same rule whenever t is a double with few bits (0, 1/4, 1/2,
    3/4, 1, 3/2): p/u > k/4 means p/u - k/4 >= 1/(4u) > 2^-36, far beyond half an ulp of t, so rn(p/u) > t as well; and p/u == t
    is exact on both sides — asserted too.  It is NOT the same rule for a threshold that is itself a rounded quotient t = rn(p'/u')
    != p'/u' (IoU 20/3381 and thresh = rn(20/3381), rounded down: the driver keeps the box, p/u > t would drop it): there the
    driver's f64 rule is the specification, and the naive rule's departures are counted and printed, not asserted."""
    rng = np.random.default_rng(seed)
    n = 140
    boxes, scores = random_boxes(rng, n, 160, 5)
    if seed % 2:                                               # exact copies and nested boxes: IoU 1 and simple fractions
        boxes[n // 2:] = boxes[:n - n // 2]
        boxes[n // 2::3, 2:] += 1
    dets = np.concatenate([boxes.astype(np.float64), scores.astype(np.float64)[:, None]], 1)
    occurring = sorted({float(np.float64(q.numerator) / np.float64(q.denominator))
                        for q in (iou_exact(boxes[i], boxes[j]) for i in range(0, n, 7) for j in range(i + 1, n, 5)) if 0 < q < 1})
    pick = [occurring[k] for k in range(0, len(occurring), max(1, len(occurring) // 6))][:6]
    threshes = [0.0, 0.25, 0.5, 0.75, 1.0, 1.5]
    for t in pick:
        threshes += [t, float(np.nextafter(t, 0.0)), float(np.nextafter(t, 2.0))]
    f64_bad, naive_plain, naive_rounded = [], [], 0
    for k, t in enumerate(threshes):
        want, fb, nb = nms_brute(boxes.tolist(), scores.tolist(), t)
        f64_bad += fb
        if k < 6:
            naive_plain += nb
        else:
            naive_rounded += len(nb)
        assert lo.nms_boxes(dets, t, stable=True) == want, t
    print("pairs where q > thresh and the f64 rule part, at thresholds that are rounded quotients: %d" % naive_rounded)
    assert not f64_bad, f64_bad[:5]
    assert not naive_plain, naive_plain[:5]


def test_nms_boxes_threshold_equal_to_an_iou_keeps_the_box():
    """IoU == thresh exactly (1/3, not a double: the rule is on the rounded quotient; and 1/2, a double) does not suppress."""
    boxes = [[0, 0, 9, 9], [5, 0, 14, 9], [0, 20, 9, 29], [0, 25, 9, 39]]       # IoU 50/150 = 1/3, and 50/200 = 1/4
    assert iou_exact(boxes[0], boxes[1]) == Fraction(1, 3) and iou_exact(boxes[2], boxes[3]) == Fraction(1, 4)
    dets = np.array([b + [s] for b, s in zip(boxes, [4.0, 3.0, 2.0, 1.0])], np.float64)
    third = float(np.float64(1.0) / np.float64(3.0))
    assert lo.nms_boxes(dets, third, stable=True) == [0, 1, 2, 3]
    assert lo.nms_boxes(dets, float(np.nextafter(third, 0.0)), stable=True) == [0, 2, 3]
    assert lo.nms_boxes(dets, 0.25, stable=True) == [0, 2, 3]
    assert lo.nms_boxes(dets, float(np.nextafter(0.25, 0.0)), stable=True) == [0, 2]


@pytest.mark.parametrize("seed", range(4))
def test_nms_boxes_unstable_equals_stable_without_ties(seed):
    rng = np.random.default_rng(100 + seed)
    boxes, _ = random_boxes(rng, 300, 200, 5)
    scores = rng.permutation(300).astype(np.float64) / 3.0                       # all distinct
    dets = np.concatenate([boxes.astype(np.float64), scores[:, None]], 1)
    for t in (0.0, 0.3, 0.5, 1.0):
        assert lo.nms_boxes(dets, t, stable=False) == lo.nms_boxes(dets, t, stable=True)


@pytest.mark.parametrize("seed", range(4))
def test_canonical_sort_unique_equals_sorted_and_loop(seed):
    """Several classes, few distinct values per field: equal (x, y, similarity) within a class across template ids (dropped when
    adjacent), across classes (kept), and with an entry of another position in between (kept)."""
    rng = np.random.default_rng(200 + seed)
    n = 3000
    m = np.zeros(n, lo.MATCH_DTYPE)
    m["x"] = rng.integers(-2, 4, n); m["y"] = rng.integers(-2, 4, n)
    m["sim"] = (rng.integers(0, 4, n).astype(np.float32) / np.float32(3.0) + np.float32(70.0))
    m["cls"] = rng.integers(0, 3, n); m["tid"] = rng.integers(0, 6, n)
    # similarities of their own, so that the neighbours in the order are known: template t and t + 1 at one position (the second is
    # dropped), and the same with another position of template t in between (the order is ..., (t, A), (t, B), (t + 1, A): kept)
    extra = []
    for k in range(40):
        t, c, sim = k % 5, k % 3, 80.0 + k
        extra += [(1, 2, sim, c, t), (1, 2, sim, c, t + 1)]
        if k % 2:
            extra.append((3, 2, sim, c, t))
    m = np.concatenate([m, np.array(extra, lo.MATCH_DTYPE)])
    m = m[rng.permutation(len(m))]
    rows = sorted(((-float(r["sim"]), int(r["tid"]), int(r["cls"]), int(r["y"]), int(r["x"])) for r in m))
    want = []
    for r in rows:
        if want and (want[-1][4], want[-1][3], want[-1][0], want[-1][2]) == (r[4], r[3], r[0], r[2]):
            continue
        want.append(r)
    got = lo.canonical_sort_unique(m)
    assert [(-float(r["sim"]), int(r["tid"]), int(r["cls"]), int(r["y"]), int(r["x"])) for r in got] == want
    assert len(set(rows)) - len(want) == 20 and len(set(rows)) < len(m)                                    # adjacent-unique removed across template ids too
    assert len(lo.canonical_sort_unique(m[:0])) == 0
