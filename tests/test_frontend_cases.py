"""CPU: the frames of frontend_cases.py sit on the edges they are built for (every condition count asserted), and on each of them the oracle
equals the per-pixel scalar restatement in Python integers (frontend_scalar_ref.py) — the raw normals, their median, the magnitudes and the
quantised orientations.  The oracle is pinned to the reference by one golden vector at default parameters; this holds it to an independent
statement at the other parameters and on hostile frames before a GPU run is compared with it.  Three mutants of the scalar statement
(`<=` for `<` twice, `>=` for `>`) must each change the result on the case built for that comparison."""
import operator

import numpy as np
import pytest

import frontend_cases as fc
import frontend_scalar_ref as sr
import linemod_oracle as lo

NAMES = list(fc.all_cases())


@pytest.mark.parametrize("name", NAMES)
def test_condition_counts_and_oracle_equals_the_scalar_restatement(name):
    c = fc.all_cases()[name]
    p = c["params"]
    cparts = fc.colour_parts(c["rgb"], p["weak_threshold"])
    dparts = fc.depth_parts(c["dep"], p["distance_threshold"], p["difference_threshold"])
    counts = fc.check_conditions(c, cparts if c["about"] == "colour" else dparts)
    print(name, counts)
    mag, out = sr.orientations(cparts["dx3"], cparts["dy3"], p["weak_threshold"])
    assert np.array_equal(mag, cparts["mag"]) and np.array_equal(out, cparts["out"]), "colour chain"
    raw = sr.raw_normals(c["dep"], p["distance_threshold"], p["difference_threshold"])
    assert np.array_equal(raw, dparts["raw"]), "normals before the median"
    med = lo.quantized_normals(c["dep"], p["distance_threshold"], p["difference_threshold"])
    assert np.array_equal(sr.median5(raw), med), "median"


def test_the_two_overflow_figures():
    """The kernel's 32-bit body (difference_threshold <= 150) relies on 1150 |ddx| < 2^31 and det * d < 2^31.  Brute force over the 256 tap
    subsets at diff = 150, deltas of +-149: the largest |1150 ddx| is 771 075 000 (all eight taps; = |1150 ddy|), and the oracle reaches exactly
    that on the tap lattice — below 2^31 = 2 147 483 648, the comment holds.  det * d peaks at 22500 * 65535 = 1 474 537 500 (extremes).  At
    diff = 70000 the oracle's largest |1150 ddx| on `extremes` is 169 571 812 500 > 2^31: a 64-bit body that truncated would differ."""
    ext = fc.tap_extremes(150)
    assert ext["ddx"][0] == ext["ddy"][0] == 771075000 < 2 ** 31
    counts = fc.check_conditions(fc.all_cases()["tap_subsets_diff150"])
    assert counts["max_1150_ddx"] == counts["max_1150_ddy"] == 771075000
    assert fc.tap_extremes(151)["ddx"][0] == 776250000
    big = fc.check_conditions(fc.all_cases()["extremes_diff70000_dist65536"])
    assert big["max_1150_ddx"] == 169571812500 > 2 ** 31
    assert fc.check_conditions(fc.all_cases()["extremes_diff150_dist65536"])["max_det_times_depth"] == 22500 * 65535 < 2 ** 31


def test_saturated_magnitude():
    """the largest magnitude of blurred 0 / 255 data, measured on the oracle over all half planes: 276 660 (>= 200 000), reached in every channel
    of sat_steps; the R | B lane bounds of the kernel hold with room (a + 2 b + c <= 1020, 7 taps <= 65280)"""
    sat, patch = fc.saturated_magnitude()
    assert sat == 276660 and set(np.unique(patch)) == {0, 255}
    c = fc.all_cases()["sat_steps"]
    assert set(np.unique(c["rgb"])) == {0, 255}
    assert int(fc.case_parts(c)["smoothed"].max()) == 255 and int(fc.case_parts(c)["smoothed"].min()) == 0


@pytest.mark.parametrize("mutant,name", [("difference", "steep_planes_diff150"), ("difference", "steep_planes_diff50"), ("distance", "distance_edge_diff50_dist2000"),
                                         ("weak", "at_threshold")])
def test_mutants_of_the_strict_comparisons_are_detected(mutant, name):
    c = fc.all_cases()[name]
    p = c["params"]
    if mutant == "weak":
        parts = fc.colour_parts(c["rgb"], p["weak_threshold"])
        _, good = sr.orientations(parts["dx3"], parts["dy3"], p["weak_threshold"])
        _, bad = sr.orientations(parts["dx3"], parts["dy3"], p["weak_threshold"], gt=operator.ge)
        want = parts["out"]
    else:
        kw = {"lt": operator.le} if mutant == "difference" else {"dist_lt": operator.le}
        good = sr.raw_normals(c["dep"], p["distance_threshold"], p["difference_threshold"])
        bad = sr.raw_normals(c["dep"], p["distance_threshold"], p["difference_threshold"], **kw)
        want = lo.quantized_normals_raw(c["dep"], p["distance_threshold"], p["difference_threshold"])
        assert not np.array_equal(sr.median5(bad), sr.median5(good)), "the mutant must survive the median too"
    assert np.array_equal(good, want)
    assert int((bad != good).sum()) >= 16, (mutant, name, int((bad != good).sum()))


def test_tiny_below_the_detectors_minimum():
    """12 x 12 (no frame a detector takes; a level 1 can be that small): the normals' interior is the one pixel (5, 5)"""
    rng = np.random.default_rng(9)
    rgb = rng.integers(0, 256, (12, 12, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:12, 0:12]
    dep = (500 + 7 * xx - 3 * yy).astype(np.uint16)
    parts = fc.colour_parts(rgb, 10.0)
    mag, out = sr.orientations(parts["dx3"], parts["dy3"], 10.0)
    assert np.array_equal(mag, parts["mag"]) and np.array_equal(out, parts["out"])
    raw = lo.quantized_normals_raw(dep, 2000, 50)
    assert np.array_equal(sr.raw_normals(dep, 2000, 50), raw) and np.count_nonzero(raw) == 1 and raw[5, 5] != 0
    assert np.array_equal(sr.median5(raw), lo.quantized_normals(dep, 2000, 50))
