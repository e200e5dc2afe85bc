"""Inputs that take the preparation of the ICP clouds (icp.hip: k_icp_voxel_wide / k_icp_voxel, k_icp_grid_wide / k_icp_grid,
k_icp_knn / k_icp_knn_far, k_icp_normals) off its usual route, each proving ON THE CPU, from the oracle's own voxel indices and
distances, that it sits on the edge it is named after (check_edges).

All cases but mid_cloud share ONE 640x480 frame (frame_cases): every case owns the pixels under its dilated mask, the model image and
the scene hold the case at the same pixels (detect = the mask's first column and row), the scene is the model 3 mm further back, and
model and scene camera are K512 (fx = fy = 512, cx = 320, cy = 240: lattice_ties needs it, the others do not care).  So one run
registers every case as a hypothesis of one batch.  Only lattice_ties covers the frame's centre pixel, so the init guess of every
other case is NaN in the oracle and on the device alike (LL.cpp:91-104 reads the model depth there).

The numpy restatements of the kernels' group rules (voxel_groups, grid_groups, far_ring) are the test's statement of what sends a
cloud down a path; the GPU test asserts through the debug read-back that the device took that path."""
import numpy as np

import linemod_oracle as lo

W, H = 640, 480
K512 = np.array([512, 0, 320, 0, 512, 240, 0, 0, 1], np.float32).reshape(3, 3)
SORT_GROUPS, GROUP_CAP, COLUMN_MAX, CHUNK = 8, 8192, 64, 1024      # kIcpSortGroups, kGroupCap, kColumnMax, kWG (icp.hip)
GRID, CELL_MIN, SLAB_PTS, FAR_MAX = 64, 0.005, 2048, 256          # kIcpGrid, kCellMin, kKnnSlabPts; far points a case must exceed (the issue's figure)
SCENE_BACK = 3                                                     # mm the scene lies behind the model
# Relative eigenvalue gap (l1 - l0) / l2 of a neighbourhood's covariance from which a normal is compared as a direction.  Measured
# (tests/test_icp_prepare_cases.py asserts it): the oracle's normals were computed a second time from centred neighbours in np.longdouble
# (exact_normals); over all 56k targets of the cases here the two agree to 1.2e-15 in 1 - |cos| at every gap above zero — the smallest
# such gap is 8.56e-7 (deep_range: the far blob with 21 neighbours 60 m away) — and disagree (up to 0.15) only where the gap is 0 to
# rounding (the 1-px line of wire, the three collinear points of tiny_3).  So the threshold is the smallest gap seen to agree to 1e-10.
NORMAL_GAP_MIN = 8.5e-7


def _blank():
    return np.zeros((H, W), np.uint16)


def _rect(md, x0, y0, w, h, depth):
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w]
    md[y0:y0 + h, x0:x0 + w] = np.asarray(depth(xx, yy) if callable(depth) else depth).astype(np.uint16)
    return md


# ---- the model images ---------------------------------------------------------------------------------
def near_many():
    """90x90 px sloping from 100 to 140 mm: a voxel is ~12 px wide, a (ix, iy) column holds a few hundred points."""
    return _rect(_blank(), 20, 160, 90, 90, lambda x, y: 100 + np.rint((x - 20) * 30 / 89.0 + (y - 160) * 10 / 89.0))


def near_few():
    """90x90 px, flat at 60 mm: ~10 mm across, fewer than 30 voxels (and so fewer than 30 targets: k = n_target)."""
    return _rect(_blank(), 20, 262, 90, 90, 60)


def cap(extra):
    """128x64 px at 2 m (every pixel its own voxel) far left, a 3x3 blob at 6 m far right: the patch is group 0 of 8 by the span rule
    (voxel_groups).  extra: one more pixel beside the patch."""
    y0 = 84 if extra else 8
    md = _rect(_blank(), 8, y0, 128, 64, 2000)
    if extra:
        md[y0, 136] = 2000
    return _rect(md, 620, 200 if extra else 170, 3, 3, 6000)


def deep_range():
    """Every fifth pixel of 250x250 px at 300 mm (2.9 mm apart: each its own voxel) and a 3x3 blob at 60 m in the far corner."""
    md = _blank()
    md[215:465:5, 370:620:5] = 300
    return _rect(md, 10, 458, 3, 3, 60000)


TINY = (1, 2, 3, 29, 30, 31)


def tiny(n):
    """n pixels at 2 m, rows of ten (1, 2, 3: one row, collinear)."""
    md = _blank()
    x0 = 160 + 40 * TINY.index(n)
    for i in range(n):
        md[14 + i // 10, x0 + i % 10] = 2000 + (i % 10) + 2 * (i // 10)
    if n <= 3:
        md[14, x0:x0 + n] = 2000
    return md


def lattice_ties():
    """A fronto-parallel plane at 2048 mm over the frame's centre: x = (u - 320) / 512 * 2.048 and y = (v - 240) / 512 * 2.048 take the
    same values, so on the diagonals the neighbours (a, b) and (b, a) are exactly equidistant."""
    return _rect(_blank(), 288, 208, 64, 64, 2048)


def wire():
    """A 1-px line and a 2-px ridge, 30 px from each other and from a patch, all at 2 m."""
    md = _rect(_blank(), 170, 392, 1, 70, 2000)
    _rect(md, 200, 392, 2, 70, 2000)
    return _rect(md, 232, 392, 40, 70, lambda x, y: 2000 + np.rint(6 * np.sin(x / 7.0) + 5 * np.cos(y / 9.0)))


def many_far():
    """A patch and 480 single pixels 6 px apart whose depths are scattered over 2.2-7 m: each is centimetres from every other point, and
    the 30 nearest of most lie beyond the widest ring k_icp_knn tries (the xy grid's cell grows with the cloud, the depth range is free)."""
    md = _rect(_blank(), 130, 160, 40, 40, lambda x, y: 2000 + np.rint(5 * np.sin(x / 6.0) + 4 * np.cos(y / 8.0)))
    for i in range(480):
        md[285 + 6 * (i // 30), 128 + 6 * (i % 30)] = 2200 + ((i * 37) % 480) * 10
    return md


def mid_cloud():
    """160x120 px at 2 m: 19200 points, more than the 16384 whose radix keys k_icp_voxel holds in LDS, fewer than 32768."""
    return _rect(_blank(), 240, 180, 160, 120, lambda x, y: 2000 + np.rint(8 * np.sin(x / 11.0) * np.cos(y / 13.0)))


FRAME = [("near_many", near_many), ("near_few", near_few), ("cap_8192", lambda: cap(False)), ("cap_8193", lambda: cap(True)),
         ("deep_range", deep_range)] + [("tiny_%d" % n, (lambda n=n: tiny(n))) for n in TINY] + [
         ("lattice_ties", lattice_ties), ("wire", wire), ("many_far", many_far)]


class PrepCase:
    def __init__(self, name, md, scene):
        self.name, self.md, self.scene = name, md, scene
        ys, xs = np.nonzero(md)
        self.xy = (int(xs.min()), int(ys.min()))
        self.K = K512
        self._o = {}

    def oracle(self, scene_mode):
        """The oracle's preparation and registration (poseRefine::process as lo.pose_refine runs it, the pieces kept)."""
        if scene_mode in self._o:
            return self._o[scene_mode]
        model_pts, scene_pts, tr = lo.backproject_clouds(self.scene, self.md, K512, K512, *self.xy)
        src = lo.voxel_down_sample(model_pts)
        raw_tgt = scene_pts if scene_mode else model_pts
        tgt = lo.voxel_down_sample(raw_tgt) if scene_mode else src
        nn = "kdtree" if len(tgt) > 600 else "brute"
        k = min(lo.KNN, len(tgt))
        lists = lo.knn_lists(tgt, lo.KNN + 1, nn)                   # one more than k: the tie at the k-th distance is visible
        d = (tgt[:, None, :] - tgt[lists]) ** 2
        d2 = d[..., 0] + d[..., 1] + d[..., 2]                      # (lo._sqdist's expression)
        nrm, cov = normals_from_lists(tgt, lists[:, :k])
        init = np.eye(4)
        init[:3, 3] = tr
        history = []
        T, fit, rmse, iters = lo.icp_point_to_plane(src, tgt, nrm, init, nn=nn, history=history)
        self._o[scene_mode] = dict(model_pts=model_pts, scene_pts=scene_pts, raw_tgt=raw_tgt, init=tr, src=src, tgt=tgt, k=k, lists=lists[:, :k],
                                   d2=d2, normals=nrm, cov=cov, T=T, fitness=float(np.float32(fit)), rmse=rmse, iterations=iters,
                                   history=history, nn=nn)
        return self._o[scene_mode]


def normals_from_lists(pts, lists):
    """lo.estimate_normals on given neighbour lists (its statements), and the covariances."""
    n, k = lists.shape
    out, covs = np.zeros((n, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        if k < 3:
            out[i] = (0, 0, 1)
            continue
        q = pts[lists[i]]
        mean = lo._seq_sum(q) / k
        cum = lo._seq_sum(q[:, :, None] * q[:, None, :]) / k
        covs[i] = cum - np.outer(mean, mean)
        w, v = np.linalg.eigh(covs[i])
        out[i] = v[:, 0] if np.linalg.norm(v[:, 0]) > 0 else (0, 0, 1)
    return out, covs


def exact_normals(pts, lists):
    """The same normals a second way: covariance of the CENTRED neighbours in np.longdouble (no cancellation of E[xx] - E[x]E[x]),
    eigenvectors by eigh of its float64 rounding.  Returns (normal, largest eigenvector, relative gap (l1 - l0) / l2) per point."""
    n, k = lists.shape
    nrm, big, gap = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    for i in range(n):
        if k < 3:
            nrm[i] = (0, 0, 1)
            gap[i] = np.inf
            continue
        q = pts[lists[i]].astype(np.longdouble)
        c = q - q.mean(0)
        w, v = np.linalg.eigh((c.T @ c / k).astype(np.float64))
        nrm[i], big[i] = v[:, 0], v[:, 2]
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
    return nrm, big, gap


_CACHE = {}


def frame_cases():
    """The shared frame: {name: PrepCase}; no case's dilated mask touches another's pixels."""
    if "frame" not in _CACHE:
        from scipy.ndimage import maximum_filter
        mds = [(name, f()) for name, f in FRAME]
        owner = np.zeros((H, W), np.int32)
        scene = _blank()
        for i, (name, md) in enumerate(mds):
            ys, xs = np.nonzero(md)
            assert xs.min() >= 4 and ys.min() >= 4 and xs.max() + 9 < W and ys.max() + 9 < H, name      # the window stays in the frame, no clamp
            mask = maximum_filter((md > 0).astype(np.uint8), size=9, mode="constant", cval=0) > 0
            assert not (owner[mask] > 0).any(), (name, FRAME[int(owner[mask].max()) - 1][0])
            owner[mask] = i + 1
            scene = np.where(md > 0, md + SCENE_BACK, scene).astype(np.uint16)
        for i, (name, md) in enumerate(mds):                         # (and no case's content under another's mask)
            assert (owner[md > 0] == i + 1).all(), name
        _CACHE["frame"] = {name: PrepCase(name, md, scene) for name, md in mds}
    return _CACHE["frame"]


def mid_case():
    if "mid" not in _CACHE:
        md = mid_cloud()
        _CACHE["mid"] = PrepCase("mid_cloud", md, np.where(md > 0, md + SCENE_BACK, 0).astype(np.uint16))
    return _CACHE["mid"]


# ---- the kernels' rules, restated -----------------------------------------------------------------------
def _bits(v):
    return 1 if v <= 0 else int(v).bit_length()


def voxel_index(pts):
    """lo.voxel_down_sample's voxel indices."""
    mn = pts.min(0) - lo.VOXEL_SIZE * 0.5
    return np.floor((pts - mn) / lo.VOXEL_SIZE).astype(np.int64)


def voxel_groups(pts):
    """k_icp_voxel_wide on a back-projected cloud.  The span rule: group g of SORT_GROUPS takes the points whose leading voxel index ix
    lies in [span * g // 8, span * (g + 1) // 8) with span = max ix + 1.  Returns dict(bits = index bits bx + by + bz, group = the
    group of every point, counts = points per group, wide = the eight groups do the cloud: bits <= 32 and no group over GROUP_CAP)."""
    idx = voxel_index(pts)
    bits = [_bits(int(idx[:, a].max())) for a in range(3)]
    span = int(idx[:, 0].max()) + 1
    edges = np.array([span * g // SORT_GROUPS for g in range(SORT_GROUPS + 1)])
    group = np.searchsorted(edges, idx[:, 0], side="right") - 1
    counts = np.bincount(group, minlength=SORT_GROUPS)
    return dict(idx=idx, bits=sum(bits), axis_bits=bits, group=group, counts=counts, wide=sum(bits) <= 32 and counts.max() <= GROUP_CAP)


def grid_of(raw, tgt, wide):
    """The search grid of the target cloud: k_icp_grid_wide spans the extent of the cloud the target was down-sampled from (raw),
    k_icp_grid the target's own.  Returns dict(cell, gx, gy, cx, cy: the column of every target)."""
    e = raw if wide else tgt
    mn, mx = e.min(0), e.max(0)
    cell = max(max(mx[0] - mn[0], mx[1] - mn[1]) / GRID, CELL_MIN)
    if not cell > CELL_MIN:
        cell = CELL_MIN
    inv = 1.0 / cell

    def coord(v, m, g):
        return np.clip(np.floor((v - m) * inv), 0, g - 1).astype(np.int64)
    gx = int(coord(mx[0], mn[0], GRID)) + 1
    gy = int(coord(mx[1], mn[1], GRID)) + 1
    return dict(cell=cell, gx=gx, gy=gy, cx=coord(tgt[:, 0], mn[0], gx), cy=coord(tgt[:, 1], mn[1], gy))


def grid_groups(raw, tgt):
    """k_icp_grid_wide: group g takes the x columns [gx * g // 8, gx * (g + 1) // 8).  counts per group, wide = none over GROUP_CAP."""
    g = grid_of(raw, tgt, True)
    edges = np.array([g["gx"] * q // SORT_GROUPS for q in range(SORT_GROUPS + 1)])
    group = np.searchsorted(edges, g["cx"], side="right") - 1
    counts = np.bincount(group, minlength=SORT_GROUPS)
    return dict(grid=g, group=group, counts=counts, wide=counts.max() <= GROUP_CAP)


def far_ring(cell):
    """The widest ring (in cells) a whole wave of k_icp_knn tries before it leaves a point to k_icp_knn_far: it starts at
    R0 + 1 + (R0 + 1) // 2, R0 = max(1, ceil(9 mm / cell)), and doubles while R < 8."""
    R0 = max(1, int(np.ceil(0.009 / cell)))
    R = R0 + 1 + ((R0 + 1) >> 1)
    while R < 8:
        R *= 2
    return R


def surely_far(o, wide_grid):
    """Targets whose k-th neighbour lies beyond the widest ring's guarantee radius on the grid the device builds: k_icp_knn cannot
    finish them, they go to k_icp_knn_far."""
    g = grid_of(o["raw_tgt"], o["tgt"], wide_grid)
    return int((o["d2"][:, o["k"] - 1] > (far_ring(g["cell"]) * g["cell"]) ** 2).sum())


# ---- every case on its edge -------------------------------------------------------------------------------
def _group_runs(vg):
    """Per group of voxel_groups: the (start, end) of every voxel's run in the group's sorted order, and the largest (ix, iy) column."""
    out = []
    for g in range(SORT_GROUPS):
        idx = vg["idx"][vg["group"] == g]
        if len(idx) == 0:
            out.append((np.zeros((0, 2), np.int64), 0))
            continue
        order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
        s = idx[order]
        new = np.ones(len(s), bool)
        new[1:] = np.any(s[1:] != s[:-1], axis=1)
        starts = np.nonzero(new)[0]
        ends = np.append(starts[1:], len(s))
        col = np.unique(s[:, :2], axis=0, return_counts=True)[1].max()
        out.append((np.stack([starts, ends], 1), int(col)))
    return out


def straddling_runs(vg):
    """Voxels whose run of points crosses a multiple of CHUNK in their group's sorted order (the HBM half of the voxel sums)."""
    n = 0
    for runs, _ in _group_runs(vg):
        for a, b in runs:
            n += int((a // CHUNK) != ((b - 1) // CHUNK))
    return n


def check_edges(name, c):
    """The assertions of the case `name` on the oracle's data; returns a dict of the figures (printed by the CPU test)."""
    v, s = c.oracle(False), c.oracle(True) if name != "mid_cloud" and name != "lattice_ties" else None
    vg = voxel_groups(v["model_pts"])
    fig = dict(n_model=len(v["model_pts"]), n_src=len(v["src"]), bits=vg["bits"], groups=vg["counts"].tolist())
    clouds = [v["model_pts"]] + ([s["scene_pts"]] if s else [])
    if name.startswith("near"):
        for pts in clouds:
            g = voxel_groups(pts)
            assert g["wide"], (name, g["counts"], g["bits"])
            fig["column"] = max(col for _, col in _group_runs(g))
            fig["straddle"] = straddling_runs(g)
            assert fig["column"] > COLUMN_MAX and fig["straddle"] >= 1, (name, fig)
        assert (len(v["src"]) > 30) if name == "near_many" else (len(v["src"]) < 30), (name, len(v["src"]))
        if name == "near_many":
            assert 100 <= c.md[c.md > 0].min() and c.md.max() <= 140
    elif name.startswith("cap"):
        want = 8192 if name == "cap_8192" else 8193
        for pts, o in zip(clouds, (v, s)):
            g = voxel_groups(pts)
            tgt = lo.voxel_down_sample(pts) if o is s else v["src"]
            assert len(pts) == want + 9 and len(tgt) == want + 9, (name, len(pts), len(tgt))          # every pixel its own voxel
            assert g["bits"] <= 32 and g["counts"][0] == want and g["counts"][1:7].sum() == 0 and g["counts"][7] == 9, (name, g["counts"], g["bits"])
            assert g["wide"] == (want == 8192)
            gg = grid_groups(pts, tgt)
            assert gg["counts"][0] == want and gg["counts"][7] == 9 and gg["wide"] == (want == 8192), (name, gg["counts"])
    elif name == "deep_range":
        for pts, o in zip(clouds, (v, s)):
            g = voxel_groups(pts)
            assert 32 < g["bits"] and g["bits"] + _bits(len(pts) - 1) <= 64 and not g["wide"], (name, g["axis_bits"])
            gg = grid_groups(pts, o["tgt"])
            cols = np.unique(gg["grid"]["cx"] * gg["grid"]["gy"] + gg["grid"]["cy"], return_counts=True)[1]
            fig["column_targets"] = int(cols.max())
            assert cols.max() > SLAB_PTS and len(o["tgt"]) > SLAB_PTS and gg["wide"], (name, cols.max())
    elif name == "mid_cloud":
        assert 17000 <= len(v["model_pts"]) <= 32000 and vg["bits"] <= 32 and len(v["src"]) > 16384, (name, fig)
    elif name.startswith("tiny"):
        n = int(name.split("_")[1])
        assert len(v["src"]) == n and len(s["tgt"]) == n, (name, len(v["src"]), len(s["tgt"]))
        if n == 3:
            d = v["src"] - v["src"][0]
            assert np.linalg.matrix_rank(d, tol=1e-12) == 1
    elif name == "lattice_ties":
        k = v["k"]
        ties = int((v["d2"][:, k - 1] == v["d2"][:, k]).sum())
        fig["tied_queries"] = ties
        assert k == lo.KNN and ties >= 36, (name, ties)
        assert len(v["src"]) == len(v["model_pts"]) == 64 * 64    # every pixel its own voxel: the lattice survives the down-sampling
    elif name == "wire":
        for o in (v, s):
            _, _, gap = exact_normals(o["tgt"], o["lists"])
            fig["gap_below_1e-6"] = int((gap < 1e-6).sum())
            assert fig["gap_below_1e-6"] >= 10, (name, fig)
    elif name == "many_far":
        for o in (v, s):
            fig["surely_far"] = surely_far(o, True)
            assert fig["surely_far"] > FAR_MAX and surely_far(o, False) > FAR_MAX, (name, fig)
            iso = o["d2"][:, 1] > 0.01 ** 2                         # (nearest other point centimetres away)
            assert iso.sum() >= 480, (name, int(iso.sum()))
    return fig


def all_cases():
    d = dict(frame_cases())
    d["mid_cloud"] = mid_case()
    return d
