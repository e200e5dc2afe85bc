"""Depth slabs (Detector.matchSlabsResident) against what the parent commit offers for the same result, on a resident frame (GPU).
640x480, Detector(150, [4, 8]), --templates (2000) planted templates split over five scale classes with depth ranges (radii 700, 850, 1000,
1200 and 1450 mm, +-15 %), threshold 75, default mode options.  The legs:

  slabs        matchSlabsResident(thr, classes)                                                            (this commit)
  host_masks   the same records through the parent commit's public API: the modes and a mask per slab in numpy, match(..., masks=) per slab
               (an upload of frame and masks and a front end each), merge_matches over the lists             (what a user of the parent commit must do)
  plain        matchResident of all five classes, no slabs                                                  (what a user does today; another result)

Per leg: ms per call = --steps calls between two fences, nine regions after one warm-up region, reported as median / min / max.  host_masks
and plain use nothing this commit adds, so they run on either library (--package).  The slabs and host_masks records are compared once.

    python profiles/depth_slabs.py --legs slabs,host_masks,plain [--package DIR] [--steps 50]
    rocprofv3 --kernel-trace --stats -d OUT -o slabs -- python profiles/depth_slabs.py --legs slabs --regions 1 --steps 20    # kernel listing"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="slabs,host_masks,plain")
ap.add_argument("--package", default=os.path.join(ROOT, "6dpose_amd"))
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--regions", type=int, default=9)
ap.add_argument("--templates", type=int, default=2000)
args = ap.parse_args()
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), args.package):
    sys.path.insert(0, p)
import linemodLevelup_pybind as lm
import depth_slabs_ref as ds
import linemod_oracle as lo
import synth

T, NFEAT, THR, SLAB = [4, 8], (150, 75), 75.0, 150
W, H = 640, 480
RADII = (700, 850, 1000, 1200, 1450)
NAMES = ["scale%d" % r for r in RADII]
RANGES = {n: (int(0.85 * r), int(1.15 * r)) for n, r in zip(NAMES, RADII)}

rgb, dep = synth.make_frame(0, W, H)
pyr = lo.OracleDetector(NFEAT[0], T).quantize_pyramid(rgb, dep)
banks = {n: synth.make_planted_bank(1234 + i, args.templates // len(NAMES), [(p[0], p[1]) for p in pyr], T, NFEAT) for i, n in enumerate(NAMES)}


def med_min_max(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def host_masks(det):
    """the definition of matchSlabs through match(..., masks=): every class here has a range"""
    lists = []
    for m in ds.depth_modes(dep):
        p = int(m["depth_mm"])
        pos = [i for i, n in enumerate(NAMES) if RANGES[n][0] <= p <= RANGES[n][1]]
        if not pos:
            continue
        S = ds.slab_mask(dep, p, SLAB)
        recs = det.matchArray([rgb, dep], THR, [NAMES[i] for i in pos], masks=[S, S])
        recs["class_index"] = np.asarray(pos, np.int32)[recs["class_index"]]
        lists.append(recs)
    return lm.merge_matches(np.concatenate(lists)) if lists else np.zeros(0, lm.MATCH_DTYPE)


def leg(name):
    det = lm.Detector(NFEAT[0], T, device=0)
    for n in NAMES:
        det.addClassPacked(n, *banks[n])
    if name == "slabs":
        for n in NAMES:
            det.setClassDepthRange(n, *RANGES[n])
    det.setFrame([rgb, dep])
    call = {"slabs": lambda: det.matchSlabsResident(THR, NAMES, slab_mm=SLAB)[0], "host_masks": lambda: host_masks(det),
            "plain": lambda: det.matchResident(THR, NAMES)}[name]

    def region():
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = call()                                     # (every call ends in a collect: the records are on the host)
        return (time.perf_counter() - t0) / args.steps * 1e3, last

    region()
    runs = [region() for _ in range(args.regions)]
    out = {"leg": name, "ms_per_call": med_min_max([r[0] for r in runs]), "records": len(runs[-1][1])}
    if name == "slabs":
        _recs, slabs = det.matchSlabsResident(THR, NAMES, slab_mm=SLAB)
        out["slabs"] = [{k: s[k] for k in ("depth_mm", "pixels", "class_ids", "records")} for s in slabs]
        out["equals_host_masks"] = bool(runs[-1][1].tobytes() == host_masks(det).tobytes())
    return out


print(json.dumps({"size": [W, H], "templates": args.templates, "steps": args.steps, "regions": args.regions, "ranges": RANGES,
                  "library": "this commit" if os.path.samefile(args.package, os.path.join(ROOT, "6dpose_amd")) else "--package",
                  "legs": [leg(n) for n in args.legs.split(",")]}))
