"""Times the particle-swarm pose refiner: 16 hypotheses x 64 particles x 30 generations, a 128 x 128 window on a
640 x 480 scene, synth.icosphere(3) (1280 triangles).  3 warm-up calls, then nine regions of --calls calls each; a region's figure
is its mean device_ms (the HIP events lm_pso_run puts around its own enqueue), reported is the median of the nine.  Writes
profiles/pso_refine.txt.
  python profiles/pso_refine.py                      the timing
  python profiles/pso_refine.py --kernels DIR        reads the kernel-stats CSV a separate
      rocprofv3 --kernel-trace --stats -d DIR -o pso -- python profiles/pso_refine.py --once
  run left under DIR and appends the per-kernel split (the share of k_raster against k_pso_cost)."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "6dpose_amd"), os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "profiles", "pso_refine.txt")
H, P, G, WIN = 16, 64, 30, (128, 128)
ICP_MS = 0.69          # the 16-hypothesis ICP leg, for scale


def setup():
    import linemodLevelup_pybind as lm
    import synth
    V, F, _, _ = synth.icosphere(3, radius=60.0, seed=2)
    assert len(F) == 1280
    mesh = lm.Mesh(V, F)
    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float64)
    rng = np.random.default_rng(1)
    t_true = np.array([15.0, -10.0, 420.0])
    scene = mesh.render((640, 480), K, np.eye(3, dtype=np.float32)[None], t_true[None].astype(np.float32), mode="depth")[0]
    ts = t_true + rng.uniform(-12, 12, (H, 3))
    a = rng.uniform(-0.06, 0.06, (H, 3))
    Rs = np.stack([np.eye(3) + np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) for v in a])
    Rs = np.stack([np.linalg.svd(R)[0] @ np.linalg.svd(R)[2] for R in Rs])           # the nearest rotations
    xy, _ = lm.derive_windows(K, ts, 64.0, WIN)
    ctx = lm.PsoContext(0)
    ctx.set_scene(scene, K)
    return ctx, mesh, Rs, ts, xy, t_true


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one warm-up call and one call (the run profiled under rocprofv3)")
    ap.add_argument("--kernels", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.kernels:
        files = glob.glob(os.path.join(args.kernels, "**", "*kernel_stats.csv"), recursive=True)
        assert files, "no *kernel_stats.csv under %s" % args.kernels
        rows = list(csv.DictReader(open(files[0])))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        lines = ["", "per-kernel split of one profiled run (rocprofv3 --kernel-trace --stats; 2 calls, the first cold):"]
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            lines.append("  %-60s calls %6s  total %10.3f ms  mean %8.2f us  %5.1f %%" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6,
                                                                                          float(r["AverageNs"]) / 1e3, 100.0 * float(r["TotalDurationNs"]) / total))
        with open(OUT, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    ctx, mesh, Rs, ts, xy, t_true = setup()
    opts = dict(particles=P, generations=G, seed=1)
    if args.once:
        ctx.run(mesh, Rs, ts, xy, WIN, **opts)
        res, ms = ctx.run(mesh, Rs, ts, xy, WIN, **opts)
        print("one call: %.3f ms" % ms)
        return
    for _ in range(3):
        ctx.run(mesh, Rs, ts, xy, WIN, **opts)
    regions = []
    for _ in range(9):
        regions.append(float(np.mean([ctx.run(mesh, Rs, ts, xy, WIN, **opts)[1] for _ in range(args.calls)])))
    res, _ = ctx.run(mesh, Rs, ts, xy, WIN, **opts)
    e0 = np.linalg.norm(ts - t_true, axis=1); e1 = np.array([np.linalg.norm(r["t"] - t_true) for r in res])
    med = float(np.median(regions))
    lines = ["pso_refine: %d hypotheses x %d particles x %d generations, window %dx%d, 640x480 scene, 1280 triangles" % (H, P, G, WIN[0], WIN[1]),
             "regions (ms per call, mean of %d calls each): %s" % (args.calls, " ".join("%.3f" % r for r in regions)),
             "median %.3f ms per call (min %.3f, max %.3f) = %.4f ms per generation (%d evaluations per call)" % (med, min(regions), max(regions), med / (G + 1), G + 1),
             "for scale: the 16-hypothesis ICP leg is %.2f ms (DESIGN.md §7)" % ICP_MS,
             "translation error mm, median over the hypotheses: start %.2f, refined %.2f; cost start %.2f, refined %.2f"
             % (np.median(e0), np.median(e1), np.median([r["initial_cost"] for r in res]), np.median([r["cost"] for r in res]))]
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
