"""Depth slabs in numpy: the rule of Detector.depthModes (the histogram of a depth image and its 1-D non-maximum suppression) and the slab
mask of Detector.matchSlabs, restated from include/amd_linemod.h with plain loops.  Integers only: the device has to agree exactly."""
import numpy as np

MODE_DTYPE = np.dtype([("bin", np.int32), ("depth_mm", np.int32), ("pixels", np.uint32)])
DEFAULTS = dict(bin_mm=25, near_mm=300, far_mm=4000, window=2, min_pixels=1000, max_modes=8)


def num_bins(bin_mm, near_mm, far_mm):
    """ceil((far_mm - near_mm) / bin_mm), ValueError for what the library refuses"""
    if bin_mm < 1 or near_mm < 1 or far_mm > 65536:
        raise ValueError("bin_mm >= 1, near_mm >= 1, far_mm <= 65536")
    nbins = -((near_mm - far_mm) // bin_mm)
    if nbins < 1 or nbins > 4096:
        raise ValueError("nbins in 1..4096")
    return nbins


def histogram(depth, bin_mm, near_mm, far_mm):
    """h[b] = pixels with near_mm <= d < far_mm and (d - near_mm) // bin_mm == b; depth 0 and everything else count nowhere"""
    nbins = num_bins(bin_mm, near_mm, far_mm)
    d = np.asarray(depth).astype(np.int64).ravel()
    d = d[(d >= near_mm) & (d < far_mm)]
    return np.bincount((d - near_mm) // bin_mm, minlength=nbins).astype(np.int64)


def modes_of(h, bin_mm, near_mm, window, min_pixels, max_modes):
    """the modes of a histogram, most pixels first, ties towards the smaller depth, at most max_modes"""
    if window < 0 or not 1 <= max_modes <= 16 or min_pixels < 1:
        raise ValueError("window >= 0, max_modes in 1..16, min_pixels >= 1")
    n = len(h)
    found = []
    for b in range(n):
        if h[b] < min_pixels:
            continue
        if any(not h[b] > h[j] for j in range(max(0, b - window), b)):
            continue
        if any(not h[b] >= h[j] for j in range(b + 1, min(n - 1, b + window) + 1)):
            continue
        found.append((-int(h[b]), near_mm + b * bin_mm + bin_mm // 2, b))
    found.sort()
    out = np.zeros(min(len(found), max_modes), MODE_DTYPE)
    for k in range(len(out)):
        out[k] = (found[k][2], found[k][1], -found[k][0])
    return out


def depth_modes(depth, bin_mm=25, near_mm=300, far_mm=4000, window=2, min_pixels=1000, max_modes=8):
    return modes_of(histogram(depth, bin_mm, near_mm, far_mm), bin_mm, near_mm, window, min_pixels, max_modes)


def slab_mask(depth, p, slab_mm):
    """255 where d != 0 and p - slab_mm <= d <= p + slab_mm, 0 elsewhere"""
    d = np.asarray(depth).astype(np.int64)
    return np.ascontiguousarray(np.where((d != 0) & (d >= p - slab_mm) & (d <= p + slab_mm), 255, 0).astype(np.uint8))


def same_modes(got, want):
    assert len(got) == len(want), (got, want)
    for f in ("bin", "depth_mm", "pixels"):
        assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), (f, got, want)
