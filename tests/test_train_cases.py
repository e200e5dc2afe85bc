"""CPU checks of tests/train_cases.py: every adversarial training frame sits on the edge it is named after, asserted from what the
oracle itself feeds to selectScatteredFeatures (no GPU).  tests/test_gpu_train.py runs the same frames on the device."""
import numpy as np
import pytest
from scipy import ndimage

import train_cases as tc


def _lists(cand):
    return [(l, m, c[m]) for l, c in enumerate(cand) for m in ("color", "normal")]


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_case_takes_the_path_its_row_names(name):
    """What decides the path: a list longer than kTrainCap or more than kTrainMaxFeatures features mean host, a short list means -1."""
    (rgb, depth, mask, p), cand, oid, _ = tc.analysed(name)
    _, path, trains = tc.CASES[name]
    H, W = mask.shape
    assert 96 <= W <= 224 and 80 <= H <= 176 and rgb.shape == (H, W, 3) and depth.shape == (H, W) and set(np.unique(mask)) == {0, 255}
    assert (oid >= 0) == trains
    over = any(s["n"] > tc.K_TRAIN_CAP for _, _, s in _lists(cand)) or p["num_features"] > tc.K_TRAIN_MAX_FEATURES
    assert over == (path == "host")
    assert any(s["n"] < s["nf"] for _, _, s in _lists(cand)) == (not trains)
    assert p["num_features"] >> (len(p["T"]) - 1) >= 1
    for l, c in enumerate(cand):                   # no label in the frame's outer pixels: a labelled run never ends at the frame border
        lab = c["normal"]["labelled"]
        assert not (lab[0].any() or lab[-1].any() or lab[:, 0].any() or lab[:, -1].any()), l


def test_1_exact_fill():
    for name, n in (("1_exact_fill", 24), ("1_one_short", 23)):
        _, cand, oid, _ = tc.analysed(name)
        assert cand[0]["color"]["nf"] == 24 and cand[0]["color"]["n"] == n
        assert all(s["n"] >= s["nf"] for l, m, s in _lists(cand) if (l, m) != (0, "color"))
        assert (oid >= 0) == (n == 24)


@pytest.mark.parametrize("n", sorted(tc.CHUNK_EDGES))
def test_2_chunk_edges(n):
    _, cand, oid, _ = tc.analysed("2_chunk_n%d" % n)
    assert cand[0]["color"]["n"] == n and 8 <= cand[0]["color"]["nf"] <= 32 and oid >= 0


def test_3_many_passes():
    _, cand, oid, _ = tc.analysed("3_many_passes")
    assert oid >= 0
    assert any(s["passes"] >= 3 and s["last_distance"] < 1 for _, _, s in _lists(cand))


def test_4_ties():
    _, cand, oid, _ = tc.analysed("4_ties")
    assert oid >= 0
    for l, c in enumerate(cand):
        for m in ("color", "normal"):
            _, inv, cnt = np.unique(c[m]["scores"], return_inverse=True, return_counts=True)
            assert (cnt[inv] > 1).mean() >= 0.5, (l, m)


def test_5_mask_shapes():
    (_, _, mask, _), cand, oid, _ = tc.analysed("5_mask_shapes")
    assert oid >= 0
    on = mask > 0
    H, W = on.shape
    bg, nb = ndimage.label(~on)
    border = set(bg[0]) | set(bg[-1]) | set(bg[:, 0]) | set(bg[:, -1])
    assert any(k not in border for k in range(1, nb + 1))                                      # a hole
    spur = on[1:-1] & ~on[:-2] & ~on[2:]
    assert max(len(r) for row in spur for r in "".join("x" if v else " " for v in row).split()) >= 8   # a one-pixel-wide part
    e1 = ndimage.minimum_filter(mask, 3, mode="nearest")
    e2 = ndimage.minimum_filter(e1, 3, mode="nearest")
    comp, nc = ndimage.label(on, structure=np.ones((3, 3)))
    assert any((e1[comp == k] > 0).any() and not (e2[comp == k] > 0).any() for k in range(1, nc + 1))   # erode leaves it, erode^2 removes it
    touched = [sum(bool(x) for x in ((comp[0] == k).any(), (comp[-1] == k).any(), (comp[:, 0] == k).any(), (comp[:, -1] == k).any()))
               for k in range(1, nc + 1)]
    assert max(touched) >= 3
    assert (e2[:, 0] > 0).any() and (e2[0] > 0).any()                                         # replicate border: the erosion keeps the frame's edge


@pytest.mark.parametrize("ext", [1, 2, 5])
def test_6_label_mosaic(ext):
    (_, _, mask, p), cand, oid, _ = tc.analysed("6_mosaic_ext%d" % ext)
    assert oid >= 0 and p["extract_threshold"] == ext
    assert [c["normal"]["extract_threshold"] for c in cand] == [ext, {1: 0, 2: 1, 5: 2}[ext]]
    for c in cand:
        assert (c["normal"]["label_counts"] > 0).all()
    n0 = cand[0]["normal"]
    sizes = []
    for k in range(8):
        region = n0["labelled"] & (n0["label_img"] == k)
        comp, nc = ndimage.label(region)
        sizes += list(ndimage.sum(region, comp, range(1, nc + 1)))
    assert len(sizes) >= 24 and np.median(sizes) <= 14 * 14                                  # many small regions (cells of 14 pixels)
    if ext >= 2:       # the finger: labelled pixels, every distance below the threshold (2 * ceil(width / 2) < 2 * ext), so no candidate
        finger = n0["labelled"][76:88, 36:56]
        assert finger.any() and n0["dist"][76:88, 36:56][finger].max() < ext
    else:              # at 1 every labelled pixel is a candidate (its distance is at least 1), and level 1 runs with threshold 0
        assert n0["n"] == n0["labelled"].sum() and cand[1]["normal"]["n"] == cand[1]["normal"]["labelled"].sum()
    # the mask touches the left frame border; the labelled runs under it end at the margin the quantiser leaves, not at the border
    assert (mask[:, 0] > 0).any()
    assert n0["labelled"][:, 5].any() and not n0["labelled"][:, :5].any()


def test_7_thresholds():
    for strong, trains in ((20, True), (55, True), (90, False)):
        (_, _, _, p), cand, oid, _ = tc.analysed("7_strong_%d" % strong)
        assert p["strong_threshold"] == strong and (oid >= 0) == trains
        assert cand[0]["color"]["n"] >= cand[0]["color"]["nf"]
        assert (cand[1]["color"]["n"] < cand[1]["color"]["nf"]) == (strong == 90)
    n = [tc.analysed("7_strong_%d" % s)[1][0]["color"]["n"] for s in (20, 55, 90)]
    assert n[0] >= n[1] > n[2]


def test_8_odd_levels():
    (_, _, mask, p), cand, oid, _ = tc.analysed("8_odd_levels")
    assert oid >= 0 and p["T"] == [4, 4, 8] and mask.shape == (110, 150)
    assert [c["mask"].shape for c in cand] == [(110, 150), (55, 75), (27, 37)]
    for c in cand:
        assert (c["mask"][:, -1] > 0).any() and (c["mask"][-1] > 0).any()
    assert (mask[::4, 148] > 0).any()              # a level-2 sample position whose column (37) is outside level 2: the pyramid's guard


def test_9_cap_boundary():
    _, cand, oid, _ = tc.analysed("9a_at_cap")
    assert oid >= 0 and cand[0]["normal"]["n"] == tc.K_TRAIN_CAP
    assert (cand[0]["normal"]["label_counts"] > 0).sum() == 1
    _, cand, oid, _ = tc.analysed("9b_over_cap")
    assert oid >= 0 and cand[0]["normal"]["n"] > tc.K_TRAIN_CAP


def test_10_feature_ceiling():
    for nf in (1024, 1025):
        (_, _, _, p), cand, oid, _ = tc.analysed("10%s_%d_features" % ("a" if nf == 1024 else "b", nf))
        assert oid >= 0 and p["num_features"] == nf and cand[0]["color"]["nf"] == nf and cand[1]["color"]["nf"] == 512
        assert all(s["nf"] <= s["n"] <= tc.K_TRAIN_CAP for _, _, s in _lists(cand))


def test_host_selection_refuses_zero_features(tmp_path):
    """tests/cpp/host_templates_zero_features.cpp: host_templates.cpp alone, under ASan + UBSan, with num_features == 0 (what
    num_features >> level gives for too few features): no division by zero (LL.cpp:632), a refusal instead.  Host code, no GPU."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "zero_features")
    cmd = [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(root, "6dpose_amd", "csrc"), os.path.join(root, "tests", "cpp", "host_templates_zero_features.cpp"),
           os.path.join(root, "6dpose_amd", "csrc", "host_templates.cpp"), "-o", exe]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:   # gcc: the runtimes inside the program
        subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
