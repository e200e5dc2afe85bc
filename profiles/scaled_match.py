"""What depth-scaled matching (Detector.matchScaledResident) costs on a resident frame (GPU).
640x480, Detector(150, [4, 8]), --templates (2000) planted templates trained at 1000 mm, a ladder of 9 (0.5 .. 2 in quarter octaves).  The legs:

  scaled   matchScaledResident(75, ["obj"])                                          (k_depth_probe, k_coarse_scaled, k_local_scaled)
  slabs    what the API offers without it: the bank scaled in numpy into 9 classes (lm.scaled_features per entry), each with the depth range
           its scale is the nearest for, matched by matchSlabsResident — nine times the bank.  NOT the same coverage: it matches only at the
           modes of the depth histogram, so it returns fewer records; its time is not like for like
  plain    matchResident(75, ["obj"])                                                (one scale: what the others are measured against)

Per leg: ms per call = --steps calls between two host clock reads, nine regions after one warm-up region, median / min / max; records per call.
One JSON line per leg; --out FILE also writes them there, replacing the file (profiles/scaled_match.txt holds one such run).

    python profiles/scaled_match.py [--legs scaled,slabs,plain] [--steps 10]
    rocprofv3 --kernel-trace --stats -d OUT -o scaled -- python profiles/scaled_match.py --legs scaled --regions 1      # kernel microseconds"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="scaled,slabs,plain")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--regions", type=int, default=9)
ap.add_argument("--templates", type=int, default=2000)
ap.add_argument("--out", default="")
args = ap.parse_args()
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "6dpose_amd")):
    sys.path.insert(0, p)
import numpy as np

import linemodLevelup_pybind as lm
import linemod_oracle as lo
import synth

T, NFEAT, THR, W, H, D_TRAIN = [4, 8], (150, 75), 75.0, 640, 480, 1000
SCALES = lm.DEFAULT_SCALES
Q = [lm.scale_q10(s) for s in SCALES]
rgb, dep = synth.make_frame(11, W, H)
pyr = lo.OracleDetector(NFEAT[0], T).quantize_pyramid(rgb, dep)
bank = synth.make_planted_bank(21, args.templates, [(p[0], p[1]) for p in pyr], T, NFEAT)


def scaled_bank(q):
    """every entry's features scaled about its box centre by q (the box stays: positions and clamps are the unscaled template's)"""
    feat, offs, wh = bank
    out = feat.copy()
    for e in range(len(offs) - 1):
        a, b = offs[e], offs[e + 1]
        out[a:b, 0], out[a:b, 1] = lm.scaled_features(int(wh[e][0]), int(wh[e][1]), feat[a:b, 0], feat[a:b, 1], q)
    return np.ascontiguousarray(out), offs, wh


def detector(leg):
    det = lm.Detector(NFEAT[0], T, device=0)
    if leg == "slabs":
        for k, q in enumerate(Q):                            # class k is valid where scale k is the nearest: d between the midpoints of 1024 d_train / q
            det.addClassPacked("obj%d" % k, *scaled_bank(q))
            hi = 65535 if k == 0 else int(2 * 1024 * D_TRAIN / (Q[k] + Q[k - 1]))
            lo_mm = 1 if k == len(Q) - 1 else int(2 * 1024 * D_TRAIN / (Q[k] + Q[k + 1])) + 1
            det.setClassDepthRange("obj%d" % k, lo_mm, hi)
    else:
        det.addClassPacked("obj", *bank)
        det.setClassTrainDepth("obj", D_TRAIN)
    det.setFrame([rgb, dep])
    return det


def leg(name):
    det = detector(name)
    call = {"scaled": lambda: det.matchScaledResident(THR, ["obj"], scales=SCALES),
            "slabs": lambda: det.matchSlabsResident(THR, ["obj%d" % k for k in range(len(Q))])[0],
            "plain": lambda: det.matchResident(THR, ["obj"])}[name]
    times, recs = [], 0
    for region in range(args.regions + 1):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            recs = len(call())
        if region:
            times.append(1e3 * (time.perf_counter() - t0) / args.steps)
    line = json.dumps({"leg": name, "threshold": THR, "templates": args.templates, "ms_per_call_median": statistics.median(times), "min": min(times),
                       "max": max(times), "records_per_call": recs})
    print(line, flush=True)
    return line


lines = [leg(name) for name in args.legs.split(",")]
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
