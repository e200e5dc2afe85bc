"""Generates tests/golden/pose_error_golden.npz: pysixd's own pose errors (pose_error.vsd with both costs, cou, add, adi,
re, te) and the GT statistics of tools/calc_gt_stats.py:103-155, on a small deterministic scene.  The reference's
pysixd/renderer.py needs glumpy / OpenGL, absent here: sys.modules['pysixd.renderer'] is replaced by the rasteriser's numpy
restatement (oracle/render_oracle.rasterise; float32 eye depth, background 0), fed with R, t and K cast to float32 as
lm_mesh_pose_errors renders them.  Run: python tests/golden/make_pose_error_golden.py

Cases: the bumpy synth.icosphere (asymmetric) and an exactly symmetric cube; a 320x240 scene holding three GT instances of the
icosphere (one partly occluded, one partly outside the frame, one fully occluded), an occluder, a hole without depth, all
quantised to whole mm; estimates identical to, slightly and strongly perturbed from the GTs, and one fully outside the frame."""
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import render_oracle as ro  # noqa: E402
import synth  # noqa: E402

W, H = 320, 240
K = np.array([[286.0, 0.0, 160.3], [0.0, 286.5, 120.7], [0.0, 0.0, 1.0]])


def render(model, im_size, K, R, t, clip_near=100, clip_far=2000, mode="depth", **_):
    """pysixd.renderer.render (renderer.py:306, defaults 100 / 2000), depth mode, through render_oracle.rasterise."""
    assert mode == "depth"
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    z, tri = ro.rasterise(model["pts"], model["faces"], f32(K), f32(R), f32(t).ravel(), im_size[0], im_size[1], clip_near, clip_far)
    return np.where(tri >= 0, z, 0).astype(np.float32)


def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def cube(h=40.0):
    V = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int32)
    return V, F


def build():
    Va, Fa, _, _ = synth.icosphere(2, radius=50.0, seed=3)
    Vb, Fb = cube()
    A = {"pts": Va.astype(np.float64), "faces": Fa}
    B = {"pts": Vb.astype(np.float64), "faces": Fb}
    R0 = rot([0.3, 1.0, 0.2], 35.0)
    gt_R = np.stack([R0, rot([1.0, 0.2, 0.1], 120.0), rot([0.0, 0.4, 1.0], -70.0)]).astype(np.float32).astype(np.float64)
    gt_t = np.array([[10.0, 5.0, 800.0], [-505.0, 20.0, 900.0], [250.0, -120.0, 950.0]], np.float32).astype(np.float64)
    # scene: back plane, the three GT instances, an occluder over part of GT 0 and all of GT 2, a hole without depth
    u = np.arange(W)[None, :]; v = np.arange(H)[:, None]
    scene = (1300.0 + 0.8 * u + 0.3 * v).astype(np.float32)
    for R, t in zip(gt_R, gt_t):
        d = render(A, (W, H), K, R, t)
        scene = np.where((d > 0) & (d < scene), d, scene)
    occ = np.zeros((H, W), bool)
    occ[122:150, 165:200] = True                                      # in front of the lower right of GT 0
    occ[60:112, 210:265] = True                                       # all of GT 2
    scene = np.where(occ, np.float32(600.0) + 0.1 * u.astype(np.float32), scene)
    scene[125:150, 0:30] = 0.0                                         # no depth, over part of GT 1
    scene = np.round(scene).astype(np.float32)
    # estimates of the icosphere
    est_R = np.stack([gt_R[0], rot([0.1, 0.9, 0.3], 2.0) @ gt_R[0], rot([1.0, 0.0, 0.5], 30.0) @ gt_R[0], gt_R[0],
                      rot([0.5, 0.5, 0.0], 5.0) @ gt_R[1], rot([0.0, 0.0, 1.0], 15.0) @ gt_R[2]])
    est_t = np.stack([gt_t[0], gt_t[0] + [3.0, -2.0, 4.0], gt_t[0] + [40.0, -25.0, 30.0], [2500.0, 0.0, 800.0],
                      gt_t[1] + [-8.0, 6.0, 12.0], gt_t[2] + [5.0, 5.0, -20.0]])
    # the cube: GT, its image under a symmetry (90 deg about the cube's z axis), and a perturbed estimate
    cgt_R = rot([0.2, 0.7, 0.1], 25.0)[None]
    cgt_t = np.array([[-60.0, 40.0, 750.0]])
    cest_R = np.stack([cgt_R[0] @ rot([0, 0, 1], 90.0), rot([1.0, 0.3, 0.0], 8.0) @ cgt_R[0]])
    cest_t = np.stack([cgt_t[0], cgt_t[0] + [6.0, 0.0, -9.0]])
    return A, B, scene, gt_R, gt_t, est_R, est_t, cgt_R, cgt_t, cest_R, cest_t


def main():
    if not hasattr(np, "int"):
        np.int = int                                                  # misc.calc_pose_2d_bbox uses np.int (NumPy < 1.24)
    sys.path.insert(0, "/root/reference")
    stub = types.ModuleType("pysixd.renderer")
    stub.render = render
    sys.modules["pysixd.renderer"] = stub
    from pysixd import misc, pose_error, visibility

    A, B, scene, gt_R, gt_t, est_R, est_t, cgt_R, cgt_t, cest_R, cest_t = build()
    out = {"K": K, "scene": scene, "A_pts": A["pts"].astype(np.float32), "A_faces": A["faces"], "B_pts": B["pts"].astype(np.float32),
           "B_faces": B["faces"], "gt_R": gt_R, "gt_t": gt_t, "est_R": est_R, "est_t": est_t, "cgt_R": cgt_R, "cgt_t": cgt_t,
           "cest_R": cest_R, "cest_t": cest_t}
    for tag, model, eR, et, gR, gt in (("A", A, est_R, est_t, gt_R, gt_t), ("B", B, cest_R, cest_t, cgt_R, cgt_t)):
        res = {k: np.zeros((len(eR), len(gR))) for k in ("vsd_step", "vsd_tlinear", "cou", "add", "adi", "re", "te")}
        et, gt = et.reshape(-1, 3, 1), gt.reshape(-1, 3, 1)           # SIXD poses: cam_t_m2c is 3x1
        for e in range(len(eR)):
            for g in range(len(gR)):
                res["vsd_step"][e, g] = pose_error.vsd(eR[e], et[e], gR[g], gt[g], model, scene, K, 15, 20, "step")
                res["vsd_tlinear"][e, g] = pose_error.vsd(eR[e], et[e], gR[g], gt[g], model, scene, K, 15, 20, "tlinear")
                res["cou"][e, g] = pose_error.cou(eR[e], et[e], gR[g], gt[g], model, (W, H), K)
                res["add"][e, g] = pose_error.add(eR[e], et[e], gR[g], gt[g], model)
                res["adi"][e, g] = pose_error.adi(eR[e], et[e], gR[g], gt[g], model)
                res["re"][e, g] = pose_error.re(eR[e], gR[g])
                res["te"][e, g] = pose_error.te(et[e], gt[g])
        for k, a in res.items():
            out["%s_%s" % (tag, k)] = a
        # the renders the errors above were computed on (VSD / COU clip planes), for the restatement
        out["%s_est_depth" % tag] = np.stack([render(model, (W, H), K, R, t, 100, 10000) for R, t in zip(eR, et)])
        out["%s_gt_depth" % tag] = np.stack([render(model, (W, H), K, R, t, 100, 10000) for R, t in zip(gR, gt)])
    # calc_gt_stats.py:103-155 for the icosphere's GTs, with pysixd's own misc / visibility (renderer defaults 100 / 2000)
    stats = []
    gdep = []
    for R, t in zip(gt_R, gt_t):
        depth_gt = render(A, (W, H), K, R, t)
        gdep.append(depth_gt)
        dist_gt = misc.depth_im_to_dist_im(depth_gt, K)
        dist_im = misc.depth_im_to_dist_im(scene, K)
        visib_gt = visibility.estimate_visib_mask_gt(dist_im, dist_gt, 15)
        obj_mask_gt = dist_gt > 0
        px_valid = np.sum(dist_im[obj_mask_gt] > 0)
        px_visib = visib_gt.sum()
        px_all = obj_mask_gt.sum()
        bbox_obj = misc.calc_pose_2d_bbox(A, (W, H), K, R, t.reshape(3, 1))
        bbox_visib = [-1, -1, -1, -1]
        if px_visib > 0:
            ys, xs = visib_gt.nonzero()
            bbox_visib = misc.calc_2d_bbox(xs, ys, (W, H))
        stats.append([int(px_all), int(px_valid), int(px_visib)] + [int(e) for e in bbox_obj] + [int(e) for e in bbox_visib])
        out.setdefault("gts_visib_fract", []).append(px_visib / float(px_all) if px_all > 0 else 0.0)
    out["gts_int"] = np.array(stats, np.int64)        # px_count_all, px_count_valid, px_count_visib, bbox_obj[4], bbox_visib[4]
    out["gts_visib_fract"] = np.array(out["gts_visib_fract"])
    out["gts_depth"] = np.stack(gdep)
    path = os.path.join(HERE, "pose_error_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    print({k: np.round(v, 4).tolist() for k, v in out.items() if k.startswith("A_") and k[2:] in ("vsd_step", "cou", "adi", "add")})
    print(out["gts_int"].tolist(), out["gts_visib_fract"].tolist())


if __name__ == "__main__":
    main()
