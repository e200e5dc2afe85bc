"""CPU: the numpy restatement of pysixd's pose errors (tests/pose_error_ref.py) against pysixd's own numbers, recorded in
tests/golden/pose_error_golden.npz (make_pose_error_golden.py) and, where the reference tree is present, computed live."""
import os
import sys

import numpy as np
import pytest

import pose_error_ref as per

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "pose_error_golden.npz")))


def restated(gold, tag):
    """Every metric of the restatement for model `tag` on the recorded renders: {name: (E, G)}."""
    eR, et = (gold["est_R"], gold["est_t"]) if tag == "A" else (gold["cest_R"], gold["cest_t"])
    gR, gt = (gold["gt_R"], gold["gt_t"]) if tag == "A" else (gold["cgt_R"], gold["cgt_t"])
    pts, K, scene = gold[tag + "_pts"], gold["K"], gold["scene"]
    ed, gd = gold[tag + "_est_depth"], gold[tag + "_gt_depth"]
    out = {k: np.zeros((len(eR), len(gR))) for k in ("vsd_step", "vsd_tlinear", "cou", "add", "adi", "re", "te")}
    for e in range(len(eR)):
        for g in range(len(gR)):
            out["vsd_step"][e, g] = per.vsd(ed[e], gd[g], scene, K, 15, 20, "step")
            out["vsd_tlinear"][e, g] = per.vsd(ed[e], gd[g], scene, K, 15, 20, "tlinear")
            out["cou"][e, g] = per.cou(ed[e], gd[g])
            out["add"][e, g] = per.add(eR[e], et[e], gR[g], gt[g], pts)
            out["adi"][e, g] = per.adi(eR[e], et[e], gR[g], gt[g], pts)
            out["re"][e, g] = per.re(eR[e], gR[g])
            out["te"][e, g] = per.te(et[e], gt[g])
    return out


@pytest.mark.parametrize("tag", ["A", "B"])
def test_restatement_equals_recorded_pysixd(gold, tag):
    got = restated(gold, tag)
    for k in ("vsd_step", "cou"):
        assert np.array_equal(got[k], gold["%s_%s" % (tag, k)]), k
    for k in ("vsd_tlinear", "add", "adi", "re", "te"):
        want = gold["%s_%s" % (tag, k)]
        assert np.allclose(got[k], want, rtol=1e-12, atol=1e-12), (k, np.abs(got[k] - want).max())


def test_golden_covers_the_cases_it_claims(gold):
    """identical poses, an estimate outside the frame, a fully occluded GT, a partly hidden one, a symmetric pose."""
    assert gold["A_vsd_step"][0, 0] == 0.0 and gold["A_cou"][0, 0] == 0.0 and gold["A_add"][0, 0] == 0.0
    assert not gold["A_est_depth"][3].any() and gold["A_cou"][3, 0] == 1.0
    assert gold["gts_int"][2, 2] == 0 and gold["gts_int"][2, 0] > 0           # GT 2 fully occluded
    assert 0 < gold["gts_int"][0, 2] < gold["gts_int"][0, 0]                  # GT 0 partly occluded
    assert gold["gts_int"][1, 3] < 0                                          # GT 1 partly outside the frame (bbox_obj x < 0)
    assert gold["B_adi"][0, 0] < 1e-9 < gold["B_add"][0, 0]                   # cube under a symmetry: ADI 0, ADD not


def test_gt_stats_restatement_equals_recorded(gold):
    for g in range(len(gold["gt_R"])):
        s = per.gt_stats(gold["gts_depth"][g], gold["scene"], gold["K"], gold["gt_R"][g], gold["gt_t"][g], gold["A_pts"])
        row = [s["px_count_all"], s["px_count_valid"], s["px_count_visib"]] + s["bbox_obj"] + s["bbox_visib"]
        assert row == gold["gts_int"][g].tolist()
        assert s["visib_fract"] == gold["gts_visib_fract"][g]


def test_restatement_against_live_pysixd(gold):
    """Recompute the golden with the reference's pysixd (renderer stubbed as in make_pose_error_golden.py)."""
    if not os.path.isdir(os.path.join(REF, "pysixd")):
        pytest.skip("reference tree not present on this machine")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_pose_error_golden as mk
    finally:
        sys.path.remove(os.path.join(HERE, "golden"))
    import types
    if not hasattr(np, "int"):
        np.int = int
    saved = {k: sys.modules.get(k) for k in ("pysixd", "pysixd.renderer", "pysixd.pose_error", "pysixd.misc", "pysixd.visibility")}
    stub = types.ModuleType("pysixd.renderer")
    stub.render = mk.render
    sys.modules["pysixd.renderer"] = stub
    sys.path.insert(0, REF)
    try:
        from pysixd import pose_error
        A, B, scene, gt_R, gt_t, est_R, est_t, *_ = mk.build()
        assert np.array_equal(scene, gold["scene"])
        K = gold["K"]
        for e, g in ((0, 0), (1, 0), (2, 0), (4, 1), (5, 2)):
            t_e, t_g = est_t[e].reshape(3, 1), gt_t[g].reshape(3, 1)
            ed = mk.render(A, (mk.W, mk.H), K, est_R[e], t_e, 100, 10000)
            gd = mk.render(A, (mk.W, mk.H), K, gt_R[g], t_g, 100, 10000)
            assert pose_error.vsd(est_R[e], t_e, gt_R[g], t_g, A, scene, K, 15, 20, "step") == per.vsd(ed, gd, scene, K, 15, 20, "step")
            assert pose_error.cou(est_R[e], t_e, gt_R[g], t_g, A, (mk.W, mk.H), K) == per.cou(ed, gd)
            want = pose_error.vsd(est_R[e], t_e, gt_R[g], t_g, A, scene, K, 15, 20, "tlinear")
            assert abs(want - per.vsd(ed, gd, scene, K, 15, 20, "tlinear")) <= 1e-12 * max(1.0, abs(want))
            for name in ("add", "adi"):
                want = getattr(pose_error, name)(est_R[e], t_e, gt_R[g], t_g, A)
                assert abs(want - getattr(per, name)(est_R[e], t_e, gt_R[g], t_g, A["pts"])) <= 1e-12 * max(1.0, want)
            assert abs(pose_error.re(est_R[e], gt_R[g]) - per.re(est_R[e], gt_R[g])) <= 1e-12 * 180
            assert abs(pose_error.te(t_e, t_g) - per.te(t_e, t_g)) <= 1e-12 * 1e3
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
