"""Generates tests/golden/pose_matching_golden.json: the reference's own pysixd/pose_matching.py:4-36 (match_poses) on small
random error tables, E and G in 0..6.  Run: python tests/golden/make_pose_matching_golden.py [path of the reference]

Errors and scores are drawn from small sets of multiples of 1/4, so that tied scores, tied errors and errors equal to the
threshold are frequent; the first cases force each of them, a max_ests_count below E, GT masks as lists (one all-false, one
empty = all valid) and E = 0.  The test reads only the JSON."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_matches(pose_matching, errs, scores, thresh, max_ests, mask):
    table = [{"est_id": e, "score": scores[e], "errors": {g: errs[e][g] for g in range(len(errs[e]))}} for e in range(len(errs))]
    args = (table, thresh) if max_ests is None and mask is None else (table, thresh, -1 if max_ests is None else max_ests, mask)
    return pose_matching.match_poses(*args)


def main():
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    from pysixd import pose_matching

    q = lambda a: [[float(v) for v in row] for row in a]  # noqa: E731
    forced = [
        # tied scores: input order decides who takes GT 0
        dict(errs=[[1.0, 2.0], [0.5, 3.0], [0.25, 0.75]], scores=[0.5, 0.5, 0.5], thresh=2.5, max_ests=None, mask=None),
        # tied errors within a row: the first lowest GT wins
        dict(errs=[[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], scores=[0.25, 0.75], thresh=1.5, max_ests=None, mask=None),
        # an error equal to the threshold does not match
        dict(errs=[[2.0, 3.0], [2.5, 1.75]], scores=[1.0, 0.5], thresh=2.0, max_ests=None, mask=None),
        # max_ests_count below E
        dict(errs=[[0.5, 2.0], [0.25, 0.5], [1.0, 0.25], [0.75, 0.75]], scores=[0.25, 1.0, 0.5, 0.75], thresh=1.5, max_ests=2, mask=None),
        dict(errs=[[0.5, 2.0], [0.25, 0.5], [1.0, 0.25]], scores=[0.25, 1.0, 1.0], thresh=1.5, max_ests=1, mask=[1, 1]),
        # masks as lists: partly valid, all false, empty (= all valid)
        dict(errs=[[0.5, 2.0, 1.0], [0.25, 0.5, 0.75]], scores=[1.0, 0.5], thresh=1.5, max_ests=-1, mask=[0, 1, 1]),
        dict(errs=[[0.5, 2.0, 1.0], [0.25, 0.5, 0.75]], scores=[1.0, 0.5], thresh=1.5, max_ests=-1, mask=[False, False, False]),
        dict(errs=[[0.5, 2.0, 1.0], [0.25, 0.5, 0.75]], scores=[1.0, 0.5], thresh=1.5, max_ests=0, mask=[]),
        # E = 0, G = 0
        dict(errs=[], scores=[], thresh=1.0, max_ests=None, mask=None, G=3),
        dict(errs=[], scores=[], thresh=1.0, max_ests=3, mask=[1, 0, 1], G=3),
        dict(errs=[[], []], scores=[0.5, 0.25], thresh=1.0, max_ests=None, mask=None),
    ]
    rng = np.random.default_rng(19)
    cases = list(forced)
    while len(cases) < 32:
        E, G = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        errs = q(rng.integers(0, 12, (E, G)) * 0.25)
        scores = [float(v) for v in rng.integers(0, 4, E) * 0.25]
        thresh = float(rng.integers(1, 10) * 0.25)
        max_ests = [None, -1, 0, 1, 2, 3][int(rng.integers(0, 6))]
        kind = int(rng.integers(0, 4))
        mask = None if kind == 0 else [int(v) for v in rng.integers(0, 2, G)] if kind < 3 else [False] * G
        cases.append(dict(errs=errs, scores=scores, thresh=thresh, max_ests=max_ests, mask=mask, G=G))
    out = []
    for c in cases:
        c.setdefault("G", len(c["errs"][0]) if c["errs"] else 0)
        c["errs"], c["scores"] = q(c["errs"]), [float(v) for v in c["scores"]]
        c["matches"] = reference_matches(pose_matching, c["errs"], c["scores"], c["thresh"], c["max_ests"], c["mask"])
        out.append(c)
    path = os.path.join(HERE, "pose_matching_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes), %d cases, %d matches" % (path, os.path.getsize(path), len(out), sum(len(c["matches"]) for c in out)))


if __name__ == "__main__":
    main()
