"""Frames whose size is not aligned (Detector.setBorder("pad")) against host-side padding, streamed (GPU).  The shape of bench.py's
configs[1] — Detector(150, [4, 8]), 2000 templates planted in the padded frame, threshold 75 — at a camera's native size.  One process
runs the legs named on the command line on ONE library, so that the parent commit's library (which has no border policy) can run the
host-padding legs from its own checkout:

  feature      submitFrame of the native frame under setBorder("pad")               (this commit)
  host_pad     np.pad of every frame inside the timed loop, then submitFrame         (what a user of the parent commit must do)
  pre_padded   frames padded before the timed loop                                   (upload and device cost of the aligned frame alone)
  strict       aligned frames as they are (640x480: the default path)

Per leg: stream_ms_per_frame = 200 submitFrame / collect steps with 12 frames in flight between two fences, nine regions after one warm-up
region, reported as median / min / max; upload_bytes_per_frame = what one submitFrame copies to the device.

    python profiles/frame_border.py --size 720x540 --legs feature [--package DIR] [--steps 200]
    LM_BORDER_COPY2D=1 python profiles/frame_border.py --size 720x540 --legs feature      # the 2-D copy variant of the re-pitch

--package: the directory holding linemodLevelup_pybind.py and libamdlinemod.so to measure (default: this checkout's 6dpose_amd)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--size", default="720x540")
ap.add_argument("--legs", default="feature")
ap.add_argument("--package", default=os.path.join(ROOT, "6dpose_amd"))
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--regions", type=int, default=9)
ap.add_argument("--templates", type=int, default=2000)
args = ap.parse_args()
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), args.package):
    sys.path.insert(0, p)
import linemodLevelup_pybind as lm
import synth
import linemod_oracle as lo

T, NFEAT, THR, DEPTH = [4, 8], (150, 75), 75.0, 12
W, H = (int(v) for v in args.size.split("x"))


def aligned_pad(w, h):                                          # T = (4, 8): both sides to multiples of 16 (aligned_size([4, 8], w, h, "pad"))
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


Wa, Ha = aligned_pad(W, H)


def pad(rgb, dep):
    return (np.ascontiguousarray(np.pad(rgb, ((0, Ha - H), (0, Wa - W), (0, 0)), mode="edge")),
            np.ascontiguousarray(np.pad(dep, ((0, Ha - H), (0, Wa - W)))))


rgb0, dep0 = synth.make_frame(0, W, H)
frames = [(rgb0, dep0)]
for k in range(1, 9):                                           # one scene, fresh sensor noise per frame (bench.noisy_frames)
    rng = np.random.default_rng(1000 + k)
    rgb = np.clip(rgb0.astype(np.int16) + rng.integers(-2, 3, rgb0.shape), 0, 255).astype(np.uint8)
    dn = dep0.astype(np.int32) + rng.integers(-1, 2, dep0.shape)
    frames.append((np.ascontiguousarray(rgb), np.ascontiguousarray(np.where(dep0 > 0, np.clip(dn, 300, 65535), 0).astype(np.uint16))))
padded = [pad(*f) for f in frames]
pyr0 = lo.OracleDetector(NFEAT[0], T).quantize_pyramid(*padded[0])
bank = synth.make_planted_bank(1234, args.templates, [(p[0], p[1]) for p in pyr0], T, NFEAT)


def med_min_max(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def leg(name):
    det = lm.Detector(NFEAT[0], T, device=0)
    det.addClassPacked("obj", *bank)
    if name == "feature":
        det.setBorder("pad")
    src = frames if name in ("feature", "host_pad", "strict") else padded
    if name == "strict":
        assert (Wa, Ha) == (W, H), "the strict leg takes an aligned size"

    def region():
        t0 = time.perf_counter()
        inflight = 0
        for k in range(args.steps):
            f = src[1 + k % 8]
            if name == "host_pad":
                f = pad(*f)
            det.submitFrame(list(f), THR, ["obj"])
            inflight += 1
            if inflight == DEPTH:
                det.collect(); inflight -= 1
        for _ in range(inflight):
            last = det.collect()
        return (time.perf_counter() - t0) / args.steps * 1e3, len(last)

    region()
    runs = [region() for _ in range(args.regions)]
    n_up = W * H if name in ("feature", "strict") else Wa * Ha
    return {"leg": name, "stream_ms_per_frame": med_min_max([r[0] for r in runs]), "spread_ms": round(max(r[0] for r in runs) - min(r[0] for r in runs), 4),
            "upload_bytes_per_frame": ((n_up * 3 + 15) & ~15) + 2 * n_up, "matches_last_frame": runs[-1][1],
            "coarse_candidates_last_frame": det.lastTimings()["coarse_candidates"]}


print(json.dumps({"size": [W, H], "aligned": [Wa, Ha], "templates": args.templates, "library": "this commit" if os.path.samefile(args.package, os.path.join(ROOT, "6dpose_amd")) else "--package",
                  "copy2d": os.environ.get("LM_BORDER_COPY2D", "0"), "legs": [leg(n) for n in args.legs.split(",")]}))
