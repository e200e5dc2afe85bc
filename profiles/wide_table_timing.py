"""Kernel time per frame under a response table and a pair of matching paths, by the method of DESIGN.md section 3.1.1 (GPU): the shape of
bench.py's configs[1] (2000 planted templates, 640x480, Detector(150, [4, 8])), eight distinct synthetic frames streamed as 8-frame batches
(submitFrame x 8, collect x 8, setBatchQueue(0)); per-frame kernel time = (front end + coarse + refinement of lastTimings()) / 8; a region =
the mean of 5 batches, nine regions after 3 warm-up batches.  Prints one JSON line: median, min and max of the regions in microseconds, the
stages split out, the candidate count and what getPaths() reports.

    python profiles/wide_table_timing.py --table linemod --threshold 86 --paths wide wide
    python profiles/wide_table_timing.py --table levelup --threshold 75            # the default table on the default paths

--package DIR imports the Python binding from DIR instead of 6dpose_amd/ (another build of the library — AMD_LINEMOD_LIB — with the binding
that declares its ABI), e.g. to time the parent commit in the same visit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--table", default="levelup")
ap.add_argument("--threshold", type=float, default=75.0)
ap.add_argument("--paths", nargs=2, default=None, metavar=("REFINE", "COARSE"))
ap.add_argument("--package", default=os.path.join(ROOT, "6dpose_amd"))
ap.add_argument("--label", default="")
ap.add_argument("--regions", type=int, default=9)
args = ap.parse_args()
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), args.package):
    sys.path.insert(0, p)
import linemodLevelup_pybind as lm          # (before bench, which puts 6dpose_amd/ in front of --package)
import bench, synth
import linemod_oracle as lo

frames = bench.noisy_frames(9)
od = lo.OracleDetector(bench.NFEAT[0], bench.T_LEVELS)
pyr0 = od.quantize_pyramid(*frames[0])
bank = synth.make_planted_bank(1234, bench.N_TEMPLATES, [(p[0], p[1]) for p in pyr0], bench.T_LEVELS, bench.NFEAT)
det = lm.Detector(bench.NFEAT[0], bench.T_LEVELS, device=0)
det.addClassPacked("obj", *bank)
if args.paths:
    det.setPaths(*args.paths)
if args.table != "levelup":
    det.setResponseTable(args.table)
det.setBatch(8); det.setBatchQueue(0)


def batch():
    for f in frames[1:9]:
        det.submitFrame(list(f), args.threshold, ["obj"])
    cands = 0
    for _ in range(8):
        det.collect()
        tm = det.lastTimings()
        cands += tm["coarse_candidates"]
    assert tm["batch_frames"] == 8, tm["batch_frames"]
    return [1e3 * tm[k] / 8 for k in ("frontend_ms", "coarse_ms", "local_ms")], cands // 8


for _ in range(3):
    batch()
regions, cands = [], None
for _ in range(args.regions):
    rows = [batch() for _ in range(5)]
    cands = rows[-1][1]
    regions.append([sum(r[0][k] for r in rows) / 5 for k in range(3)])
total = [sum(r) for r in regions]
med = lambda v: round(statistics.median(v), 2)
print(json.dumps({"label": args.label, "table": args.table, "threshold": args.threshold, "paths": list(det.getPaths()), "coarse_candidates_per_frame": cands,
                  "kernel_us": {"median": med(total), "min": round(min(total), 2), "max": round(max(total), 2)},
                  "frontend_coarse_refine_us": [med([r[k] for r in regions]) for k in range(3)]}))
