"""Times the particle-swarm refiner's edge cost beside its depth cost in the configuration of profiles/pso_refine.py:
16 hypotheses x 64 particles x 30 generations, a 128 x 128 window on a 640 x 480 scene, synth.icosphere(3) (1280 triangles).  The edge
scene is the silhouette of the depth scene.  3 warm-up calls per cost, then nine regions; in a region the two costs alternate, --calls
calls each, and a region's figure is the mean device_ms (the HIP events of lm_pso_run / lm_pso_run_edges); reported are the medians of
the nine.  The distance transform (lm_pso_set_scene_edges: upload, k_edt_rows, k_edt_cols, synchronise) is timed on the host clock at
max_dist 32 and 255.  Writes profiles/pso_edges.txt.
  python profiles/pso_edges.py                       the timing
  python profiles/pso_edges.py --kernels DIR         reads the kernel-stats CSV a separate
      rocprofv3 --kernel-trace --stats -d DIR -o pso -- python profiles/pso_edges.py --once
  run left under DIR and appends the per-kernel figures (k_pso_edge_cost beside k_pso_cost, the two EDT kernels)."""
import argparse
import csv
import glob
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "6dpose_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]
OUT = os.path.join(ROOT, "profiles", "pso_edges.txt")
TAU_PX, M = 16, 32


def setup():
    import pso_refine as base
    ctx, mesh, Rs, ts, xy, t_true = base.setup()
    K = ctx.K
    scene = mesh.render((640, 480), K, np.eye(3, dtype=np.float32)[None], t_true[None].astype(np.float32), mode="depth")[0]
    on = scene > 0
    edges = on & ~(np.roll(on, 1, 0) & np.roll(on, -1, 0) & np.roll(on, 1, 1) & np.roll(on, -1, 1))        # the silhouette (the object is far from the border)
    ctx.set_scene_edges(edges, K, M)
    return ctx, mesh, Rs, ts, xy, t_true, edges, K


def kernel_rows(directory):
    """Name, Calls, AverageNs, MinNs, MaxNs per kernel from what rocprofv3 left: the kernel-stats CSV, or, where this rocprofv3 writes its
    database instead (its default output format since ROCm 7), the `kernels` view of *_results.db."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if files:
        return list(csv.DictReader(open(files[0])))
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    assert dbs, "no *kernel_stats.csv and no *_results.db under %s" % directory
    q = "select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name"
    return [dict(zip(("Name", "Calls", "AverageNs", "MinNs", "MaxNs"), r)) for r in sqlite3.connect(dbs[0]).execute(q)]


def main():
    import pso_refine as base
    H, P, G, WIN = base.H, base.P, base.G, base.WIN
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="per cost one warm-up call and one call, and the EDT at both caps (the run profiled under rocprofv3)")
    ap.add_argument("--kernels", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.kernels:
        rows = [r for r in kernel_rows(args.kernels) if any(k in r["Name"] for k in ("k_pso_edge_cost", "k_pso_cost", "k_edt_rows", "k_edt_cols", "k_raster"))]
        lines = ["", "per kernel, one profiled run (rocprofv3 --kernel-trace --stats; per cost 2 calls, the first cold; EDT: 640x480, once at M = 32 and "
                 "once at M = 255 besides setup's M = 32, so its mean mixes the caps and min / max bracket them):"]
        for r in sorted(rows, key=lambda r: r["Name"]):
            lines.append("  %-48s calls %5s  mean %8.2f us  min %8.2f us  max %8.2f us" % (r["Name"].split("(")[0][:48], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                         float(r.get("MinNs", "nan")) / 1e3, float(r.get("MaxNs", "nan")) / 1e3))
        with open(OUT, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    ctx, mesh, Rs, ts, xy, t_true, edges, K = setup()
    depth = dict(particles=P, generations=G, seed=1)
    edge = dict(particles=P, generations=G, seed=1, tau=TAU_PX, cost="edges")
    if args.once:
        for o in (depth, depth, edge, edge):
            print("one call: %.3f ms" % ctx.run(mesh, Rs, ts, xy, WIN, **o)[1])
        for m in (32, 255):
            ctx.set_scene_edges(edges, K, m)
        return
    for o in (depth, edge) * 3:
        ctx.run(mesh, Rs, ts, xy, WIN, **o)
    regions = {"depth": [], "edges": []}
    for _ in range(9):
        for name, o in (("depth", depth), ("edges", edge)):
            regions[name].append(float(np.mean([ctx.run(mesh, Rs, ts, xy, WIN, **o)[1] for _ in range(args.calls)])))
    res, _ = ctx.run(mesh, Rs, ts, xy, WIN, **edge)
    e0 = np.linalg.norm(ts - t_true, axis=1); e1 = np.array([np.linalg.norm(r["t"] - t_true) for r in res])
    px = lambda t: np.array([K[0, 0] * t[0] / t[2], K[1, 1] * t[1] / t[2]])
    p0 = [np.linalg.norm(px(t) - px(t_true)) for t in ts]; p1 = [np.linalg.norm(px(r["t"]) - px(t_true)) for r in res]
    lines = ["pso edges beside depth: %d hypotheses x %d particles x %d generations, window %dx%d, 640x480 scene, 1280 triangles; edges: tau %d px, max_dist %d, "
             "edge_step_mm 0" % (H, P, G, WIN[0], WIN[1], TAU_PX, M)]
    for name in ("depth", "edges"):
        r = regions[name]
        lines.append("cost=%-5s regions (ms per call, mean of %d calls each): %s" % (name, args.calls, " ".join("%.3f" % v for v in r)))
        lines.append("cost=%-5s median %.3f ms per call (min %.3f, max %.3f)" % (name, float(np.median(r)), min(r), max(r)))
    lines.append("edges: projected-centre error px, median over the hypotheses: start %.2f, refined %.2f; translation error mm: start %.2f, refined %.2f; "
                 "cost px^2 start %.2f, refined %.2f" % (np.median(p0), np.median(p1), np.median(e0), np.median(e1),
                                                       np.median([r["initial_cost"] for r in res]), np.median([r["cost"] for r in res])))
    for m in (32, 255):
        ctx.set_scene_edges(edges, K, m)
        t = []
        for _ in range(9):
            a = time.perf_counter(); ctx.set_scene_edges(edges, K, m); t.append((time.perf_counter() - a) * 1e3)
        lines.append("set_scene_edges 640x480, max_dist %3d (host clock: upload of 300 KiB, k_edt_rows, k_edt_cols, synchronise): median %.3f ms (min %.3f, max %.3f)"
                     % (m, float(np.median(t)), min(t), max(t)))
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
