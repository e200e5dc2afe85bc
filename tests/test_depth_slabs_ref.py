"""The numpy statement of the depth-mode rule and of the slab mask (tests/depth_slabs_ref.py) on cases worked by hand, the fixture scene of
test_gpu_depth_slabs.py held to the modes its tests rely on, and the ctypes mirrors of the structures of include/amd_linemod_depth.h held to
that header.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import depth_slabs_ref as ds
import lm_abi
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def modes(h, bin_mm=10, near_mm=100, window=2, min_pixels=1, max_modes=8):
    return [(int(m["bin"]), int(m["depth_mm"]), int(m["pixels"])) for m in ds.modes_of(np.asarray(h), bin_mm, near_mm, window, min_pixels, max_modes)]


def test_an_empty_histogram_has_no_modes():
    assert modes([0] * 12) == []
    assert len(ds.depth_modes(np.zeros((8, 8), np.uint16))) == 0


def test_one_populated_bin():
    assert modes([0, 0, 0, 7, 0, 0]) == [(3, 135, 7)]                  # 100 + 3 * 10 + 5
    assert modes([0, 0, 0, 7, 0, 0], min_pixels=8) == []


def test_on_a_plateau_the_lowest_bin_wins():
    assert modes([0, 5, 5, 5, 0, 0]) == [(1, 115, 5)]
    assert modes([0, 5, 5, 0, 0, 5, 5]) == [(1, 115, 5), (5, 155, 5)]   # the second plateau starts beyond the first one's window


def test_two_equal_peaks_further_apart_than_the_window_come_in_depth_order():
    assert modes([0, 9, 0, 0, 9, 0]) == [(1, 115, 9), (4, 145, 9)]
    assert modes([0, 9, 0, 9, 0, 0]) == [(1, 115, 9)]                   # within the window: the lower bin suppresses the higher
    assert modes([0, 9, 0, 9, 0, 0], window=1) == [(1, 115, 9), (3, 135, 9)]
    assert modes([0, 8, 0, 0, 9, 0]) == [(4, 145, 9), (1, 115, 8)]     # most pixels first


def test_peaks_at_the_first_and_the_last_bin_with_the_window_clipped():
    assert modes([6, 1, 0, 0, 2, 4]) == [(0, 105, 6), (5, 155, 4)]
    assert modes([6, 1, 0, 0, 2, 4], window=0) == [(0, 105, 6), (5, 155, 4), (4, 145, 2), (1, 115, 1)]
    assert modes([6, 1, 0, 0, 2, 4], window=100) == [(0, 105, 6)]


def test_boundary_values_of_the_depth():
    near, far = 300, 4000
    d = np.array([[near, far - 1, far, 0, 65535, near - 1]], np.uint16)
    h = ds.histogram(d, 25, near, far)
    assert h.sum() == 2 and h[0] == 1 and h[-1] == 1 and len(h) == 148
    assert (far - 1 - near) // 25 == 147
    got = ds.depth_modes(d, min_pixels=1)
    assert [(int(m["bin"]), int(m["depth_mm"])) for m in got] == [(0, 312), (147, 3987)]


def test_one_bin_and_4096_bins():
    d = np.array([[1, 2, 4096, 4097, 0, 700]], np.uint16)
    assert ds.num_bins(4096, 1, 4097) == 1
    one = ds.depth_modes(d, bin_mm=4096, near_mm=1, far_mm=4097, min_pixels=1)
    assert [(int(m["bin"]), int(m["depth_mm"]), int(m["pixels"])) for m in one] == [(0, 1 + 2048, 4)]
    assert ds.num_bins(1, 1, 4097) == 4096
    many = ds.depth_modes(d, bin_mm=1, near_mm=1, far_mm=4097, window=0, min_pixels=1, max_modes=16)
    assert [(int(m["bin"]), int(m["depth_mm"])) for m in many] == [(0, 1), (1, 2), (699, 700), (4095, 4096)]
    for bad in (dict(bin_mm=1, near_mm=1, far_mm=4098), dict(bin_mm=25, near_mm=4000, far_mm=4000), dict(bin_mm=0, near_mm=1, far_mm=10),
                dict(bin_mm=1, near_mm=0, far_mm=10), dict(bin_mm=100, near_mm=1, far_mm=65537)):
        with pytest.raises(ValueError):
            ds.num_bins(**bad)


def test_more_modes_than_max_modes():
    h = [0, 3, 0, 0, 9, 0, 0, 5, 0, 0, 7, 0]
    assert modes(h) == [(4, 145, 9), (10, 205, 7), (7, 175, 5), (1, 115, 3)]
    assert modes(h, max_modes=2) == [(4, 145, 9), (10, 205, 7)]
    assert modes(h, max_modes=1) == [(4, 145, 9)]
    for bad in (dict(max_modes=0), dict(max_modes=17), dict(window=-1), dict(min_pixels=0)):
        with pytest.raises(ValueError):
            modes(h, **bad)


def test_the_slab_mask():
    d = np.array([[0, 849, 850, 1000, 1150, 1151, 65535]], np.uint16)
    assert ds.slab_mask(d, 1000, 150).tolist() == [[0, 0, 255, 255, 255, 0, 0]]
    assert ds.slab_mask(d, 1000, 0).tolist() == [[0, 0, 0, 255, 0, 0, 0]]
    assert ds.slab_mask(d, 100, 150).tolist() == [[0, 0, 0, 0, 0, 0, 0]]          # the slab reaches below 0: depth 0 stays outside


def test_the_fixture_scene_has_the_modes_the_gpu_tests_rely_on():
    _rgb, dep = synth.make_frame(21, 320, 240, 12)
    got = ds.depth_modes(dep, min_pixels=500)
    assert [int(m["depth_mm"]) for m in got] == [1187, 912, 762, 1012]
    assert all(int(a) > int(b) for a, b in zip(got["pixels"][:-1], got["pixels"][1:]))
    for p in got["depth_mm"]:                                 # every slab masks something and leaves something
        assert 0 < (ds.slab_mask(dep, int(p), 150) > 0).mean() < 1


def test_the_structures_follow_their_header():
    text = open(os.path.join(ROOT, "include", "amd_linemod_depth.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    scalars = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}
    mirrors = {"lm_depth_mode_options": lm_abi.DepthModeOptions, "lm_depth_mode": lm_abi._CDepthMode, "lm_slab": lm_abi._CSlab}
    found = re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S)
    assert sorted(n for _t, _b, n in found) == sorted(mirrors)
    for _tag, body, name in found:
        members = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            ctype, first = stmt.split(",")[0].rsplit(None, 1)
            members += [(ctype, d.strip()) for d in [first] + stmt.split(",")[1:]]
        ours = mirrors[name]
        assert [(n, t) for n, t in ours._fields_] == [(m, scalars[c]) for c, m in members], name
    assert lm_abi.DEPTH_MODE_DTYPE.itemsize == ctypes.sizeof(lm_abi._CDepthMode) == 12
    assert list(lm_abi.DEPTH_MODE_DTYPE.names) == [n for n, _ in lm_abi._CDepthMode._fields_] == list(ds.MODE_DTYPE.names)
