"""The host side of grey colour frames (Detector(..., colour_channels=1)) as far as it runs without a device: the shape validation of
the colour source in both modes and rgb_to_grey's numpy restatement against pixels worked out by hand.  CPU only."""
import numpy as np
import pytest

import linemodLevelup_pybind as lm
import lm_abi


def bare_detector(mods, channels):
    """a Detector without a handle: what _sources needs is the modality set and the channel count"""
    d = lm.Detector.__new__(lm.Detector)
    d._mods, d._cch = tuple(mods), channels
    return d


G = np.arange(16 * 20, dtype=np.uint8).reshape(16, 20)
REP = np.repeat(G[..., None], 3, 2)
DEP = np.zeros((16, 20), np.uint16)


def test_grey_sources_are_hxw():
    d = bare_detector(("ColorGradient", "DepthNormal"), 1)
    rgb, dep, shape = d._sources([G, DEP], True)
    assert rgb.shape == (16, 20) and rgb.flags.c_contiguous and shape == (16, 20) and np.array_equal(rgb, G)
    rgb, _, _ = d._sources([G[:, :, None], DEP])                       # HxWx1 is the same image
    assert rgb.shape == (16, 20) and np.array_equal(rgb, G)
    rgb, _, _ = d._sources([G[:, ::2], DEP[:, ::2]])                   # a strided view is made contiguous
    assert rgb.flags.c_contiguous and np.array_equal(rgb, G[:, ::2])
    one = bare_detector(("ColorGradient",), 1)
    rgb, dep, shape = one._sources([G], True)
    assert dep is None and shape == (16, 20)
    with pytest.raises(RuntimeError, match="colour_channels=1"):
        d._sources([REP, DEP])
    with pytest.raises(RuntimeError, match="uint8 HxW grey"):
        d._sources([G.astype(np.uint16), DEP])
    with pytest.raises(RuntimeError, match="sizes differ"):
        d._sources([G[:8], DEP])


def test_rgb_sources_name_the_setting_for_a_grey_image():
    d = bare_detector(("ColorGradient", "DepthNormal"), 3)
    assert d._sources([REP, DEP])[0].shape == (16, 20, 3)
    for grey in (G, G[:, :, None]):
        with pytest.raises(RuntimeError, match="colour_channels=1"):
            d._sources([grey, DEP])
    with pytest.raises(RuntimeError, match="HxWx3") as e:               # another wrong shape: the old message, no hint
        d._sources([np.zeros((16, 20, 4), np.uint8), DEP])
    assert "colour_channels" not in str(e.value)


def test_rgb_to_grey_ref_on_pixels_worked_out_by_hand():
    # (4899 R + 9617 G + 1868 B + 8192) >> 14; 4899 + 9617 + 1868 = 16384 = 2^14, so equal channels stay what they are
    px = {(0, 0, 0): 0, (255, 255, 255): 255, (1, 1, 1): 1, (200, 200, 200): 200,
          (255, 0, 0): 76,       # 1249245 + 8192 = 1257437 -> 76.7
          (0, 255, 0): 150,      # 2452335 + 8192 = 2460527 -> 150.2
          (0, 0, 255): 29,       # 476340 + 8192 = 484532 -> 29.6
          (10, 20, 30): 18,      # 48990 + 192340 + 56040 + 8192 = 305562 -> 18.6
          (255, 255, 0): 226}    # 3701580 + 8192 = 3709772 -> 226.4
    img = np.array(list(px), np.uint8).reshape(3, 3, 3)
    got = lm.rgb_to_grey_ref(img)
    assert got.shape == (3, 3) and got.dtype == np.uint8 and got.ravel().tolist() == list(px.values())
    assert lm.rgb_to_grey_ref(np.array([255, 0, 0], np.uint8)).tolist() == 76                  # any leading shape, none included
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(RuntimeError, match="R, G, B"):
            lm.rgb_to_grey_ref(bad)
        with pytest.raises(RuntimeError, match="R, G, B"):              # the device version checks its argument before it needs the library
            lm.rgb_to_grey(bad)


def test_the_setting_is_in_the_abi_table():
    assert lm_abi.PROTOTYPES["lm_detector_set_colour_channels"][1] == [lm_abi.P, lm_abi.I]
    assert lm_abi.PROTOTYPES["lm_detector_get_colour_channels"][1] == [lm_abi.P]
    assert len(lm_abi.PROTOTYPES["lm_rgb_to_grey"][1]) == 4
