"""numpy restatement (float64) of the symmetry sets and the symmetry-aware pose errors MSSD and MSPD, written straight from
the formulas of DESIGN.md, "Pose errors".  They follow the BOP toolkit (get_symmetry_transformations, pose_error.mssd /
mspd) from memory: the toolkit is not part of the reference, so this file is the definition the device code is held to."""
import math

import numpy as np


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def disc_count(max_sym_disc_step):
    """n = ceil(pi / max_sym_disc_step): a continuous symmetry is sampled at i * 2 pi / n, i = 1 .. n-1."""
    return int(math.ceil(math.pi / max_sym_disc_step))


def symmetry_transforms(discrete=(), continuous=(), max_sym_disc_step=0.01):
    D = [(np.eye(3), np.zeros(3))]
    for M in discrete:
        M = np.asarray(M, np.float64).reshape(4, 4)
        D.append((M[:3, :3], M[:3, 3]))
    n = disc_count(max_sym_disc_step)
    step = 2.0 * math.pi / n
    C = []
    for axis, offset in continuous:
        offset = np.asarray(offset, np.float64)
        for i in range(1, n):
            R = rodrigues(axis, i * step)
            C.append((R, offset - R @ offset))
    if not C:
        out = D
    else:
        out = []
        for Rd, td in D:
            for Rc, tc in C:
                out.append((Rc @ Rd, Rc @ td + tc))
    return np.stack([R for R, _ in out]), np.stack([t for _, t in out])


def transform(R, t, pts):
    return pts @ np.asarray(R, np.float64).T + np.asarray(t, np.float64).reshape(1, 3)


def project(K, pts):
    w = pts @ np.asarray(K, np.float64).reshape(3, 3).T
    return w[:, :2] / w[:, 2:3]


def mssd(R_e, t_e, R_g, t_g, pts, Rs, ts):
    """min_s max_v || (R_e v + t_e) - (R_g (R_s v + t_s) + t_g) ||, mm."""
    pts = np.asarray(pts, np.float64)
    pe = transform(R_e, t_e, pts)
    return min(np.linalg.norm(pe - transform(R_g, t_g, transform(R, t, pts)), axis=1).max() for R, t in zip(Rs, ts))


def mspd(R_e, t_e, R_g, t_g, K, pts, Rs, ts):
    """min_s max_v || proj(R_e v + t_e) - proj(R_g (R_s v + t_s) + t_g) ||, pixels."""
    pts = np.asarray(pts, np.float64)
    ue = project(K, transform(R_e, t_e, pts))
    return min(np.linalg.norm(ue - project(K, transform(R_g, t_g, transform(R, t, pts))), axis=1).max() for R, t in zip(Rs, ts))


def errors(eR, et, gR, gt, K, pts, Rs, ts):
    """{"mssd", "mspd"}: (E, G) tables."""
    out = {"mssd": np.zeros((len(eR), len(gR))), "mspd": np.zeros((len(eR), len(gR)))}
    for e in range(len(eR)):
        for g in range(len(gR)):
            out["mssd"][e, g] = mssd(eR[e], et[e], gR[g], gt[g], pts, Rs, ts)
            out["mspd"][e, g] = mspd(eR[e], et[e], gR[g], gt[g], K, pts, Rs, ts)
    return out


def errors_batched(eR, et, gR, gt, K, pts, Rs, ts):
    """errors() with the loop over the symmetries folded into array operations, for sets of thousands of transformations:
    the same formulas, the products summed in numpy's order instead (differences of a few ulp, far below the tests' 1e-9)."""
    pts = np.asarray(pts, np.float64)
    Rs, ts = np.asarray(Rs, np.float64), np.asarray(ts, np.float64)
    K = np.asarray(K, np.float64).reshape(3, 3)
    sym = np.einsum("sij,vj->svi", Rs, pts) + ts[:, None, :]                 # (S, V, 3): R_s v + t_s
    out = {"mssd": np.zeros((len(eR), len(gR))), "mspd": np.zeros((len(eR), len(gR)))}
    for g in range(len(gR)):
        pg = sym @ np.asarray(gR[g], np.float64).T + np.asarray(gt[g], np.float64).reshape(1, 1, 3)
        wg = pg @ K.T
        ug = wg[..., :2] / wg[..., 2:3]
        for e in range(len(eR)):
            pe = transform(eR[e], et[e], pts)
            out["mssd"][e, g] = np.linalg.norm(pe[None] - pg, axis=2).max(1).min()
            out["mspd"][e, g] = np.linalg.norm(project(K, pe)[None] - ug, axis=2).max(1).min()
    return out


def cube_rotations():
    """The 24 rotations of the cube: signed permutation matrices of determinant +1, the identity first."""
    out = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                for sz in (1.0, -1.0):
                    R = np.zeros((3, 3))
                    R[0, p[0]], R[1, p[1]], R[2, p[2]] = sx, sy, sz
                    if abs(np.linalg.det(R) - 1.0) < 1e-12:
                        out.append(R)
    assert len(out) == 24 and np.array_equal(out[0], np.eye(3))
    return out


def as4x4(R, t=(0.0, 0.0, 0.0)):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M
