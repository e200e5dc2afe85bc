"""What part-based matching (Detector.setPartMatching) costs, streamed (GPU).
640x480, Detector(150, [4, 8]), --templates (2000) planted templates, eight frames per launch; in every frame the right half of --occluded (20)
planted templates' boxes is set to a constant colour and depth 0.  The legs:

  parts        setPartMatching(2), threshold 75                                      (this commit: k_coarse_parts, k_local_parts)
  holistic     the holistic kernels at the same threshold                           (either library: --package DIR runs the parent commit's)
  lowered      the holistic kernels at --lowered (45), the threshold a user needs today to keep half-occluded objects: the honest alternative

Per leg: ms per frame = --steps frames through matchStream between two fences, nine regions after one warm-up region, median / min / max;
coarse candidates and records per frame.  One JSON line per leg.

    python profiles/part_match.py --legs parts,holistic,lowered [--package DIR] [--steps 64]
    rocprofv3 --kernel-trace --stats -d OUT -o parts -- python profiles/part_match.py --legs parts --regions 1      # kernel microseconds"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="parts,holistic,lowered")
ap.add_argument("--package", default=os.path.join(ROOT, "6dpose_amd"))
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--regions", type=int, default=9)
ap.add_argument("--templates", type=int, default=2000)
ap.add_argument("--occluded", type=int, default=20)
ap.add_argument("--lowered", type=float, default=45.0)
args = ap.parse_args()
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), args.package):
    sys.path.insert(0, p)
import linemodLevelup_pybind as lm
import linemod_oracle as lo
import synth

T, NFEAT, THR, W, H = [4, 8], (150, 75), 75.0, 640, 480
rgb, dep = synth.make_frame(11, W, H)
pyr = lo.OracleDetector(NFEAT[0], T).quantize_pyramid(rgb, dep)
bank = synth.make_planted_bank(21, args.templates, [(p[0], p[1]) for p in pyr], T, NFEAT)
det = lm.Detector(NFEAT[0], T, device=0)
det.addClassPacked("obj", *bank)
clean = det.matchArray([rgb, dep], THR, ["obj"])
frames = []
for k in range(8):                                           # eight frames, each with its own occluded plants
    f_rgb, f_dep = rgb.copy(), dep.copy()
    for tid in range(k * args.occluded, (k + 1) * args.occluded):
        m = clean[clean["template_id"] == tid]
        if len(m) == 0:
            continue
        x0, y0, (w, h) = int(m[0]["x"]), int(m[0]["y"]), bank[2][4 * tid]
        f_rgb[y0:y0 + h + 1, x0 + (w + 1) // 2:x0 + w + 1] = (90, 90, 90)
        f_dep[y0:y0 + h + 1, x0 + (w + 1) // 2:x0 + w + 1] = 0
    frames.append([f_rgb, f_dep])
det.setBatch(8)


def leg(name):
    thr = args.lowered if name == "lowered" else THR
    if name == "parts":
        det.setPartMatching(2)
    elif hasattr(det, "setPartMatching"):
        det.setPartMatching(0)
    times, cands, recs = [], 0, 0
    for region in range(args.regions + 1):
        t0 = time.perf_counter()
        n = 0
        for out in det.matchStream((frames[i % 8] for i in range(args.steps)), thr, ["obj"]):
            n += len(out)
        dt = time.perf_counter() - t0
        if region:
            times.append(1e3 * dt / args.steps)
        cands, recs = det.lastTimings()["coarse_candidates"], n / args.steps
    print(json.dumps({"leg": name, "threshold": thr, "ms_per_frame_median": statistics.median(times), "min": min(times), "max": max(times),
                      "coarse_candidates_last_frame": cands, "records_per_frame": recs, "package": args.package}))


for name in args.legs.split(","):
    leg(name)
