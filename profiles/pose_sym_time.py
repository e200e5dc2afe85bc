"""Times pose_errors(metrics=("mssd", "mspd")) as DESIGN.md 7b times the other pose errors: 640x480 camera, E = 16 estimates,
G = 1, synth.icosphere(5) (10242 vertices), S = 24 (the cube's rotations) and S = 314 (one continuous symmetry at the default
step); 3 warm-up calls, then the median of 20, device events around the whole call (which blocks until its results are on
the host) and the host clock beside them.  --adi adds the ADI of the same pairs, --numpy the numpy restatement.
Run: python profiles/pose_sym_time.py [--adi] [--numpy]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "6dpose_amd"), os.path.join(ROOT, "tests")]
import linemodLevelup_pybind as lm  # noqa: E402
import pose_sym_ref as psr  # noqa: E402
import synth  # noqa: E402

K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float64)


def timed(fn, warm=3, reps=20):
    import torch
    for _ in range(warm):
        fn()
    dev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return float(np.median(dev)), float(np.median(wall)), float(np.min(dev)), float(np.max(dev))


def main():
    V, F, _, _ = synth.icosphere(5, radius=80.0, seed=2)
    mesh = lm.Mesh(V, F)
    rng = np.random.default_rng(1)
    Rg, tg = psr.rodrigues([0.3, 1.0, 0.2], 0.6), np.array([20.0, -10.0, 800.0])
    eR = np.stack([psr.rodrigues(rng.normal(size=3), rng.uniform(0, 0.5)) @ Rg for _ in range(16)])
    et = tg + rng.uniform(-20, 20, (16, 3))
    sets = {24: lm.symmetry_transforms([psr.as4x4(R) for R in psr.cube_rotations()[1:]]),
            314: lm.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))])}
    for S, syms in sets.items():
        assert len(syms[0]) == S
        for metrics in (("mssd", "mspd"), ("mssd",), ("mspd",)):
            med, wall, lo, hi = timed(lambda: lm.pose_errors(mesh, eR, et, Rg, tg, K, metrics=metrics, symmetries=syms))
            print("S = %3d  %-12s  %.3f ms per call (events; min %.3f, max %.3f), wall %.3f ms" % (S, "+".join(metrics), med, lo, hi, wall))
    if "--adi" in sys.argv:
        med, wall, lo, hi = timed(lambda: lm.pose_errors(mesh, eR, et, Rg, tg, metrics=("adi",)))
        print("ADI of the same 16 pairs  %.3f ms per call (events; min %.3f, max %.3f), wall %.3f ms" % (med, lo, hi, wall))
    if "--numpy" in sys.argv:
        V64 = V.astype(np.float64)
        for S, syms in sets.items():
            t0 = time.perf_counter()
            want = psr.errors(eR, et, Rg[None], tg[None], K, V64, *syms)
            dt = time.perf_counter() - t0
            got = lm.pose_errors(mesh, eR, et, Rg, tg, K, metrics=("mssd", "mspd"), symmetries=syms)
            print("S = %3d  numpy restatement, both metrics, 16 pairs: %.1f ms; max |device - numpy| = %.2e mm, %.2e px"
                  % (S, dt * 1e3, np.abs(got["mssd"] - want["mssd"]).max(), np.abs(got["mspd"] - want["mspd"]).max()))
    mesh.close()


if __name__ == "__main__":
    main()
