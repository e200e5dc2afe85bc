"""Grey (colour_channels=1) against RGB colour frames, in one process (GPU): the shape of bench.py's configs[1] (640x480, 2000 planted templates,
Detector(150, [4, 8]), threshold 75), the grey channel of eight synthetic frames and — for the RGB legs, which run the parent's kernels — the
same channel replicated to three.  Four legs: ("ColorGradient", "DepthNormal") and ("ColorGradient",), each RGB and grey.  Per leg

  front_end_us_per_batch   device events around the front end of an 8-frame batch (lastTimings()["frontend_ms"]: the stage launches and the
                           bit-plane launch, which both formats share): a region = the mean of 5 batches, nine regions after 3 warm-up
                           batches, reported as median / min / max;
  stream_ms_per_frame      200 submitFrame / collect steps with 12 frames in flight between two fences, nine regions after one warm-up region;
  upload_bytes_per_frame   what one submitFrame copies to the device.

    python profiles/grey_frontend.py            # one JSON line

The colour-only legs match the colour entries of the same planted bank (the normal entries dropped)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "6dpose_amd")):
    sys.path.insert(0, p)
import linemodLevelup_pybind as lm
import bench, synth
import linemod_oracle as lo

REGIONS, STEPS, DEPTH = 9, 200, 12
W, H = bench.W, bench.H
pool = bench.noisy_frames(9)
greys = [np.ascontiguousarray(rgb[..., 1]) for rgb, _ in pool]
deps = [dep for _, dep in pool]
reps = [np.repeat(g[..., None], 3, 2) for g in greys]
od = lo.OracleDetector(bench.NFEAT[0], bench.T_LEVELS)
pyr0 = od.quantize_pyramid(reps[0], deps[0])
feat, offs, wh = synth.make_planted_bank(1234, bench.N_TEMPLATES, [(p[0], p[1]) for p in pyr0], bench.T_LEVELS, bench.NFEAT)


def colour_entries(feat, offs, wh):
    """the bank's colour entries alone (entries alternate colour, normal)"""
    keep = range(0, len(offs) - 1, 2)
    parts = [feat[offs[e]:offs[e + 1]] for e in keep]
    new_offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    return np.concatenate(parts), new_offs, np.ascontiguousarray(wh[::2])


def med_min_max(v, digits):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def leg(mods, channels):
    det = lm.Detector(bench.NFEAT[0], bench.T_LEVELS, device=0, modalities=mods, colour_channels=channels)
    det.addClassPacked("obj", *((feat, offs, wh) if len(mods) == 2 else colour_entries(feat, offs, wh)))
    colour = greys if channels == 1 else reps
    frames = [[c, d][:len(mods)] for c, d in zip(colour, deps)]
    det.setBatch(8); det.setBatchQueue(0)

    def batch():
        for f in frames[1:9]:
            det.submitFrame(f, bench.THRESHOLD, ["obj"])
        for _ in range(8):
            det.collect()
        tm = det.lastTimings()
        assert tm["batch_frames"] == 8, tm["batch_frames"]
        return 1e3 * tm["frontend_ms"], tm["coarse_candidates"]

    for _ in range(3):
        batch()
    fe = [sum(batch()[0] for _ in range(5)) / 5 for _ in range(REGIONS)]
    cands = batch()[1]

    det.setBatchQueue(2)                                        # the stream as bench.py runs it

    def region():
        t0 = time.perf_counter()
        inflight = 0
        for k in range(STEPS):
            det.submitFrame(frames[1 + k % 8], bench.THRESHOLD, ["obj"])
            inflight += 1
            if inflight == DEPTH:
                det.collect(); inflight -= 1
        for _ in range(inflight):
            det.collect()
        return (time.perf_counter() - t0) / STEPS * 1e3

    region()
    stream = [region() for _ in range(REGIONS)]
    n = W * H
    upload = (((n * channels + 15) & ~15) if len(mods) == 2 else n * channels) + (2 * n if len(mods) == 2 else 0)
    return {"modalities": list(mods), "colour_channels": channels, "front_end_us_per_batch": med_min_max(fe, 1), "stream_ms_per_frame": med_min_max(stream, 4),
            "upload_bytes_per_frame": upload, "coarse_candidates_last_frame": cands, "paths": list(det.getPaths())}


out = [leg(mods, ch) for mods in (("ColorGradient", "DepthNormal"), ("ColorGradient",)) for ch in (3, 1)]
ratios = {"+".join(out[i]["modalities"]): {"front_end": round(out[i + 1]["front_end_us_per_batch"]["median"] / out[i]["front_end_us_per_batch"]["median"], 3),
                                            "stream": round(out[i + 1]["stream_ms_per_frame"]["median"] / out[i]["stream_ms_per_frame"]["median"], 3),
                                            "upload": round(out[i + 1]["upload_bytes_per_frame"] / out[i]["upload_bytes_per_frame"], 3)} for i in (0, 2)}
print(json.dumps({"legs": out, "grey_over_rgb": ratios}))
