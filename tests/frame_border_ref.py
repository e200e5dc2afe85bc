"""What the border policies of Detector.setBorder do to a frame, in numpy: the host-side padding and cropping the tests hold the device
against (tests/test_frame_border_host.py checks these helpers themselves by hand-written arrays)."""
import numpy as np


def pad_colour(img, Wa, Ha):
    """Colour (HxWx3) or grey (HxW): extended at the right and bottom by edge replication (the corner repeats the last pixel)."""
    H, W = img.shape[:2]
    assert Wa >= W and Ha >= H
    return np.ascontiguousarray(np.pad(img, ((0, Ha - H), (0, Wa - W)) + ((0, 0),) * (img.ndim - 2), mode="edge"))


def pad_zero(img, Wa, Ha):
    """Depth and masks (HxW): extended at the right and bottom with 0."""
    H, W = img.shape
    assert Wa >= W and Ha >= H
    return np.ascontiguousarray(np.pad(img, ((0, Ha - H), (0, Wa - W)), mode="constant"))


def pad_frame(colour, depth, Wa, Ha, masks=()):
    """(colour, depth, [masks]) of the aligned size; None stays None (a detector of one modality, a missing mask)."""
    return (None if colour is None else pad_colour(colour, Wa, Ha), None if depth is None else pad_zero(depth, Wa, Ha),
            [None if m is None else pad_zero(m, Wa, Ha) for m in masks])


def crop_frame(colour, depth, Wa, Ha, masks=()):
    """frame[:Ha, :Wa] of everything."""
    cut = lambda a: None if a is None else np.ascontiguousarray(a[:Ha, :Wa])
    return cut(colour), cut(depth), [cut(m) for m in masks]


def aligned_table(T, N):
    """ok[h, w] for h, w in 0..N-1: does a w x h frame meet the four conditions of the rule at every level?  Each condition is written
    down as the rule states it, for all sizes at once."""
    L = len(T)
    h, w = np.mgrid[0:N, 0:N]
    ok = (w % (1 << (L - 1)) == 0) & (h % (1 << (L - 1)) == 0)
    for l in range(L):
        wl, hl = w >> l, h >> l
        ok &= (wl > 0) & (hl > 0) & (wl % T[l] == 0) & (hl % T[l] == 0) & ((wl * hl) % 16 == 0)
    return ok


def brute_aligned_size(ok, W, H, border, rows):
    """The aligned size by searching the table ok = aligned_table(T, N).  "pad": the smallest Ha >= H that has an aligned width >= W
    (rows = ok[:, W:].any(1), the same for every H), then the smallest such width; "crop": the largest Ha in 16..H that has an aligned
    width in 16..W (rows = ok[:, 16:W + 1].any(1)), then the largest; None where nothing fits."""
    if border == "pad":
        hit = np.flatnonzero(rows[H:])
        assert len(hit), "table too small"
        Ha = H + int(hit[0])
        return W + int(np.flatnonzero(ok[Ha, W:])[0]), Ha
    hit = np.flatnonzero(rows[16:H + 1])
    if not len(hit):
        return None
    Ha = 16 + int(hit[-1])
    return 16 + int(np.flatnonzero(ok[Ha, 16:W + 1])[-1]), Ha
