"""CPU tests of the border policies' host side: the size rule (aligned_size, plain Python, no library) against a search of its four
conditions, and the numpy padding / cropping helpers the GPU tests use as their reference, against arrays written by hand."""
import numpy as np
import pytest

import frame_border_ref as fb
from lm_abi import aligned_size

TS = [[4, 8], [5, 8], [4, 4, 8], [8], [5], [2, 4], [6, 8]]
LO, HI = 16, 200


@pytest.mark.parametrize("T", TS, ids=lambda T: "T" + "_".join(map(str, T)))
def test_aligned_size_equals_a_search_of_the_four_conditions(T):
    """every W and H in 16..200, both policies"""
    ok = fb.aligned_table(T, 640)                      # (pads stay far below: the longest period of a side here is 80)
    n_none = n_same = 0
    for W in range(LO, HI + 1):
        pad_rows = ok[:, W:].any(1)                    # heights that have an aligned width >= W
        crop_rows = ok[:, 16:W + 1].any(1)             # ... an aligned width in 16..W
        for H in range(LO, HI + 1):
            want = fb.brute_aligned_size(ok, W, H, "pad", pad_rows)
            assert aligned_size(T, W, H, "pad") == want, (T, W, H)
            assert want[0] >= W and want[1] >= H
            want = fb.brute_aligned_size(ok, W, H, "crop", crop_rows)
            if want is None:
                n_none += 1
                with pytest.raises(RuntimeError, match="unsupported frame size"):
                    aligned_size(T, W, H, "crop")
            else:
                assert aligned_size(T, W, H, "crop") == want, (T, W, H)
                assert 16 <= want[0] <= W and 16 <= want[1] <= H
            if ok[H, W]:                               # an aligned size passes through both policies (and strict) unchanged
                n_same += 1
                assert aligned_size(T, W, H, "pad") == aligned_size(T, W, H, "crop") == aligned_size(T, W, H, "strict") == (W, H)
    assert n_same > 0
    assert (n_none > 0) == (T in ([5, 8], [4, 4, 8], [6, 8], [5]))       # their smallest aligned side is above 16


def test_the_sizes_the_feature_exists_for():
    assert aligned_size([4, 8], 720, 540, "pad") == (720, 544) and aligned_size([4, 8], 720, 540, "crop") == (720, 528)
    assert aligned_size([4, 8], 1920, 1080, "pad") == (1920, 1088) and aligned_size([4, 8], 1920, 1080, "crop") == (1920, 1072)
    assert aligned_size([5, 8], 848, 480, "pad") == (880, 480) and aligned_size([5, 8], 848, 480, "crop") == (800, 480)
    assert aligned_size([4, 8], 313, 229, "pad") == aligned_size([4, 8], 305, 225, "pad") == aligned_size([4, 8], 319, 239, "pad") == (320, 240)
    assert aligned_size([5, 8], 300, 200, "pad") == (320, 240) and aligned_size([4, 4, 8], 310, 230, "pad") == (320, 256)
    assert aligned_size([4, 8], 640, 480, "pad") == aligned_size([4, 8], 640, 480, "crop") == aligned_size([4, 8], 640, 480, "strict") == (640, 480)


def test_refusals():
    with pytest.raises(RuntimeError, match="unsupported frame size"):
        aligned_size([5, 8], 79, 200, "crop")              # the smallest aligned width is 80
    with pytest.raises(RuntimeError, match="unsupported frame size"):
        aligned_size([5, 8], 200, 79, "crop")
    with pytest.raises(RuntimeError, match="unsupported frame size"):
        aligned_size([4, 8], 15, 64, "pad")
    with pytest.raises(RuntimeError, match="LL.cpp:1136, 1217-1218"):
        aligned_size([4, 8], 313, 229, "strict")
    with pytest.raises(RuntimeError, match="unknown border policy"):
        aligned_size([4, 8], 320, 240, "reflect")
    with pytest.raises(RuntimeError, match="unknown border policy"):
        aligned_size([4, 8], 320, 240, None)


def test_pad_and_crop_helpers_on_a_5x3_image_by_hand():
    rgb = np.arange(45, dtype=np.uint8).reshape(3, 5, 3) + 1
    grey = np.array([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15]], np.uint8)
    dep = grey.astype(np.uint16) * 100
    mask = np.array([[255, 0, 255, 0, 255], [0, 255, 0, 255, 0], [255, 255, 0, 0, 255]], np.uint8)
    c, d, (m, none) = fb.pad_frame(grey, dep, 7, 5, [mask, None])
    assert none is None and c.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"]
    assert c.tolist() == [[1, 2, 3, 4, 5, 5, 5],
                          [6, 7, 8, 9, 10, 10, 10],
                          [11, 12, 13, 14, 15, 15, 15],
                          [11, 12, 13, 14, 15, 15, 15],          # the bottom row repeats, the corner repeats the last pixel
                          [11, 12, 13, 14, 15, 15, 15]]
    assert d.tolist() == [[100, 200, 300, 400, 500, 0, 0],
                          [600, 700, 800, 900, 1000, 0, 0],
                          [1100, 1200, 1300, 1400, 1500, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0]] and d.dtype == np.uint16
    assert m.tolist() == [[255, 0, 255, 0, 255, 0, 0],
                          [0, 255, 0, 255, 0, 0, 0],
                          [255, 255, 0, 0, 255, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0]] and m.dtype == np.uint8
    c3, _d, _m = fb.pad_frame(rgb, dep, 6, 4)
    assert c3.shape == (4, 6, 3) and np.array_equal(c3[:3, :5], rgb)
    assert c3[0, 5].tolist() == rgb[0, 4].tolist() == [13, 14, 15]                     # replicated column: the whole pixel
    assert c3[3, 2].tolist() == rgb[2, 2].tolist() and c3[3, 5].tolist() == rgb[2, 4].tolist() == [43, 44, 45]   # row, corner
    c, d, (m,) = fb.crop_frame(rgb, dep, 4, 2, [mask])
    assert np.array_equal(c, rgb[:2, :4]) and c.flags["C_CONTIGUOUS"]
    assert d.tolist() == [[100, 200, 300, 400], [600, 700, 800, 900]] and m.tolist() == [[255, 0, 255, 0], [0, 255, 0, 255]]
    c, d, _m = fb.pad_frame(None, dep, 5, 3)
    assert c is None and np.array_equal(d, dep)                                        # nothing to add: unchanged
