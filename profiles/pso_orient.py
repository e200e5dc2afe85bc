"""Times the particle-swarm refiner's directional edge cost beside its edge cost in the configuration of
profiles/pso_edges.py: 16 hypotheses x 64 particles x 30 generations, a 128 x 128 window on a 640 x 480 scene, synth.icosphere(3).  The
oriented scene is the silhouette of the depth scene with the bins of a Sobel of its mask.  Medians of nine regions, in one process:
  run:       cost="oriented" and cost="edges" alternate within a region, --calls calls each, a region's figure the mean device_ms;
  transform: set_scene_orientations and set_scene_edges alternate on the same 640 x 480 frame at max_dist 32, on the host clock;
  hand-over: set_scene_from_detector(directional=True) and the host path directional=False alternate on a colour-only detector after one
             match of a 640 x 480 synthetic frame, on the host clock.
Writes profiles/pso_orient.txt.
  python profiles/pso_orient.py                      the timing
  python profiles/pso_orient.py --kernels DIR        reads the kernel statistics a separate
      rocprofv3 --kernel-trace --stats -d DIR -o pso -- python profiles/pso_orient.py --once
  run left under DIR and appends the per-kernel figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "6dpose_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]
OUT = os.path.join(ROOT, "profiles", "pso_orient.txt")
TAU_PX, M, P_ORIENT = 16, 32, 16
KERNELS = ("k_pso_orient_cost", "k_pso_edge_cost", "k_edt_rows", "k_edt_cols", "k_edt_orient", "k_raster")


def orientations(edges, on):
    """Bins for the silhouette pixels from a Sobel of the object mask, quantised as the front end does."""
    m = on.astype(np.float64)
    p = np.pad(m, 1)
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    k = np.rint((np.degrees(np.arctan2(gy, gx)) % 360.0) * 16.0 / 360.0).astype(np.int64) & 7
    return np.where(edges, 1 << k, 0).astype(np.uint8)


def setup():
    import pso_edges as base
    ctx, mesh, Rs, ts, xy, t_true, edges, K = base.setup()
    scene = mesh.render((640, 480), K, np.eye(3, dtype=np.float32)[None], t_true[None].astype(np.float32), mode="depth")[0]
    q = orientations(edges, scene > 0)
    ctx.set_scene_orientations(q, K, M, P_ORIENT)
    return ctx, mesh, Rs, ts, xy, t_true, edges, q, K


def detector():
    import linemodLevelup_pybind as lm
    import synth
    rgb, _ = synth.make_frame(5, 640, 480, 40)
    det = lm.Detector(64, [4, 8], device=0, modalities=("ColorGradient",))
    det.addClassPacked("e", np.zeros((0, 3), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
    det.setFrame([rgb])
    det.matchResident(75.0, ["e"])
    return det


def alternate(a, b, n=9):
    """Host-clock milliseconds of a() and b(), alternating, n each after one warm-up each."""
    a(); b()
    ta, tb = [], []
    for _ in range(n):
        for f, t in ((a, ta), (b, tb)):
            s = time.perf_counter(); f(); t.append((time.perf_counter() - s) * 1e3)
    return ta, tb


def main():
    import pso_edges
    import pso_refine as base
    H, P, G, WIN = base.H, base.P, base.G, base.WIN
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="per cost one warm-up call and one call, each transform twice (the run profiled under rocprofv3)")
    ap.add_argument("--kernels", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.kernels:
        rows = [r for r in pso_edges.kernel_rows(args.kernels) if any(k in r["Name"] for k in KERNELS)]
        lines = ["", "per kernel, one profiled run (rocprofv3 --kernel-trace --stats; per cost 2 calls, the first cold; transforms at 640x480, M = 32):"]
        for r in sorted(rows, key=lambda r: r["Name"]):
            lines.append("  %-48s calls %5s  mean %8.2f us  min %8.2f us  max %8.2f us" % (r["Name"].split("(")[0][:48], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                         float(r.get("MinNs", "nan")) / 1e3, float(r.get("MaxNs", "nan")) / 1e3))
        with open(OUT, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    ctx, mesh, Rs, ts, xy, t_true, edges, q, K = setup()
    edge = dict(particles=P, generations=G, seed=1, tau=TAU_PX, cost="edges")
    orient = dict(edge, cost="oriented")
    if args.once:
        for o in (edge, edge, orient, orient):
            print("one call: %.3f ms" % ctx.run(mesh, Rs, ts, xy, WIN, **o)[1])
        for _ in range(2):
            ctx.set_scene_edges(edges, K, M)
            ctx.set_scene_orientations(q, K, M, P_ORIENT)
        return
    for o in (edge, orient) * 3:
        ctx.run(mesh, Rs, ts, xy, WIN, **o)
    regions = {"edges": [], "oriented": []}
    for _ in range(9):
        for name, o in (("edges", edge), ("oriented", orient)):
            regions[name].append(float(np.mean([ctx.run(mesh, Rs, ts, xy, WIN, **o)[1] for _ in range(args.calls)])))
    lines = ["pso oriented beside edges: %d hypotheses x %d particles x %d generations, window %dx%d, 640x480 scene, 1280 triangles; tau %d px, max_dist %d, "
             "orient_penalty %d, edge_step_mm 0" % (H, P, G, WIN[0], WIN[1], TAU_PX, M, P_ORIENT)]
    for name in ("edges", "oriented"):
        r = regions[name]
        lines.append("cost=%-8s regions (ms per call, mean of %d calls each): %s" % (name, args.calls, " ".join("%.3f" % v for v in r)))
        lines.append("cost=%-8s median %.3f ms per call (min %.3f, max %.3f)" % (name, float(np.median(r)), min(r), max(r)))
    to, te = alternate(lambda: ctx.set_scene_orientations(q, K, M, P_ORIENT), lambda: ctx.set_scene_edges(edges, K, M))
    for name, t in (("set_scene_orientations", to), ("set_scene_edges", te)):
        lines.append("%-24s 640x480, max_dist %d (host clock: upload of 300 KiB, the transforms, synchronise): median %.3f ms (min %.3f, max %.3f)"
                     % (name, M, float(np.median(t)), min(t), max(t)))
    det = detector()
    td, th = alternate(lambda: ctx.set_scene_from_detector(det, K, (640, 480), max_dist=M, directional=True, orient_penalty=P_ORIENT),
                       lambda: ctx.set_scene_from_detector(det, K, (640, 480), max_dist=M))
    for name, t in (("directional=True (device hand-over, nine planes)", td), ("directional=False (host round trip, one plane)", th)):
        lines.append("set_scene_from_detector %-50s 640x480, max_dist %d (host clock): median %.3f ms (min %.3f, max %.3f)"
                     % (name, M, float(np.median(t)), min(t), max(t)))
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
