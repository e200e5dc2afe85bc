"""Edge cases of the rasteriser (6dpose_amd/csrc/render.hip) and references that do NOT restate it.  TEST
INFRASTRUCTURE ONLY, numpy only.

oracle/render_oracle.py repeats the kernel rule for rule, so a rule that is wrong in both goes unseen.  The references
here share nothing with the kernel but the camera convention (OpenCV: p_cam = R v + t, u = fx x/z + cx, pixel (i, j)
sampled at (i, j)):

  * raycast_depth: float64 Moeller-Trumbore, one ray per pixel centre; no snapping, no edge functions, no 1/z
    interpolation;
  * lattice: sheets whose corners project exactly onto a grid of pixel fractions, so that every edge passes through
    pixel centres and the covered set is known in closed form (a half-open rectangle), whatever the diagonals, the
    windings and the face order are;
  * face_id_colours / decode_owner: the colour image names the face that owns a pixel;
  * owners_contain: exact integer test that a pixel centre lies in its owner's closed triangle;
  * ssaa_expected: the box average of a supersampled rectangle, counted in integers.

tests/test_render_edges_ref.py holds the oracle to these on the CPU, tests/test_gpu_render_edges.py the kernels (and the
kernels to the oracle, bit for bit)."""
import numpy as np

K_LATTICE = np.array([[256, 0, 16], [0, 256, 12], [0, 0, 1]], np.float32)
LATTICES = [(3, 2, 4, 256), (2.5, 1.5, 3, 256), (-6, -5, 5, 512), (3.25, 2.75, 2.5, 256)]     # (x0, y0, step, z)
LATTICE_NX, LATTICE_NY, LATTICE_W, LATTICE_H = 8, 7, 48, 40
LATTICE_SEEDS = (0, 1, 2)
EYE = np.eye(3, dtype=np.float32)
ZERO = np.zeros(3, np.float32)
# Largest |z_oracle - z_ray| on the first ray-caster view is 0.126 mm (99.9th percentile 0.037 mm): the 1/256-pixel
# snap moves a grazing surface by that much.  Used where a clip plane is compared with the ray caster.
RAY_BOUND_MM = 0.13


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float32)


def raycast_depth(V, F, K, R, t, W, H):
    """z of the nearest positive hit of the ray through every pixel centre, float64 (H, W), inf where nothing is hit."""
    V = np.asarray(V, np.float64); K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    P = V @ R.T + t
    ys, xs = np.mgrid[0:H, 0:W]
    D = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones((H, W))], -1).reshape(-1, 3)
    best = np.full(H * W, np.inf)
    for i0, i1, i2 in np.asarray(F, np.int64):
        p0 = P[i0]; e1 = P[i1] - p0; e2 = P[i2] - p0
        h = np.cross(D, e2)
        a = h @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / a
            s = -p0                                                    # ray origin (the camera centre) - p0
            u = f * (h @ s)
            q = np.cross(s, e1)
            v = f * (D @ q)
            tt = f * (e2 @ q)                                          # ray parameter = z, the direction's z being 1
            hit = (a != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 0) & (tt < best)
        best = np.where(hit, tt, best)
    return best.reshape(H, W)


def lattice(x0, y0, nx, ny, step, z, rng, K, unshared=False):
    """Fronto-parallel sheet of nx x ny quads at depth z whose corners project exactly to (x0 + i step, y0 + j step) under
    R = I, t = 0.  Diagonal per quad, winding per triangle and the order of the faces come from rng.  Returns (V float32,
    F int32, quad (nf,) = j nx + i of every face); unshared: three vertices of its own per face (V[3 f : 3 f + 3])."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    X = (x0 + step * np.arange(nx + 1) - K[0, 2]) * z / K[0, 0]
    Y = (y0 + step * np.arange(ny + 1) - K[1, 2]) * z / K[1, 1]
    Vg = np.array([[X[i], Y[j], z] for j in range(ny + 1) for i in range(nx + 1)], np.float64)
    assert np.array_equal(Vg.astype(np.float32), Vg)                                      # exact in float32 ...
    assert np.array_equal(K[0, 0] * Vg[:, 0] / z + K[0, 2], np.tile(x0 + step * np.arange(nx + 1), ny + 1))   # ... and projecting exactly
    assert np.array_equal(K[1, 1] * Vg[:, 1] / z + K[1, 2], np.repeat(y0 + step * np.arange(ny + 1), nx + 1))
    faces, quad = [], []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            for tri in ([(a, b, c), (a, c, d)] if rng.integers(2) else [(a, b, d), (b, c, d)]):
                faces.append(tri if rng.integers(2) else (tri[0], tri[2], tri[1]))
                quad.append(j * nx + i)
    perm = rng.permutation(len(faces))
    F, quad = np.array(faces, np.int64)[perm], np.array(quad, np.int64)[perm]
    V = Vg
    if unshared:
        V, F = Vg[F.ravel()], np.arange(3 * len(F)).reshape(-1, 3)
    return V.astype(np.float32), F.astype(np.int32), quad


def unshare(V, F):
    """The same faces with three vertices of their own each."""
    F = np.asarray(F, np.int64)
    return np.ascontiguousarray(np.asarray(V)[F.ravel()]), np.arange(3 * len(F), dtype=np.int32).reshape(-1, 3)


def face_id_colours(nf):
    """Vertex colours (3 nf, 3) uint8 of an unshared mesh: all three vertices of face f carry f + 1 in 24 bits."""
    f = np.repeat(np.arange(nf, dtype=np.int64) + 1, 3)
    return np.stack([f & 255, (f >> 8) & 255, f >> 16], 1).astype(np.uint8)


def decode_owner(rgb):
    """Face index per pixel of an image rendered with face_id_colours, ambient 1, ssaa 1; -1 = background."""
    c = np.asarray(rgb, np.int64)
    return (c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)) - 1


def rect_mask(x0, y0, nx, ny, step, W, H):
    """Pixels with x0 <= x < x0 + nx step and y0 <= y < y0 + ny step: what a lattice covers."""
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs >= x0) & (xs < x0 + nx * step) & (ys >= y0) & (ys < y0 + ny * step)


def grid256(V, K):
    """Vertices of a lattice in 1/256 pixel, int64 (n, 2): exact by construction, asserted."""
    V = np.asarray(V, np.float64); K = np.asarray(K, np.float64).reshape(3, 3)
    g = np.stack([(K[0, 0] * V[:, 0] / V[:, 2] + K[0, 2]) * 256.0, (K[1, 1] * V[:, 1] / V[:, 2] + K[1, 2]) * 256.0], 1)
    assert np.array_equal(g, np.rint(g))
    return g.astype(np.int64)


def _orient(a, b, p):
    return (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])


def in_triangle(g, F, f, px, py, strict=False):
    """Pixel centres (px, py) inside triangle f (arrays of equal shape) of the mesh (g = grid256, F): the three orientations
    agree in sign, zeros allowed unless strict.  Exact integers; knows neither winding nor fill rule."""
    F = np.asarray(F, np.int64)
    a, b, c = g[F[f, 0]], g[F[f, 1]], g[F[f, 2]]
    p = np.stack([np.asarray(px, np.int64) << 8, np.asarray(py, np.int64) << 8], -1)
    o = np.stack([_orient(a, b, p), _orient(b, c, p), _orient(c, a, p)], -1)
    if strict:
        return (o > 0).all(-1) | (o < 0).all(-1)
    return (o >= 0).all(-1) | (o <= 0).all(-1)


def owners_contain(owner, g, F):
    """Every covered pixel's centre lies in the closed triangle of its owner."""
    ys, xs = np.nonzero(owner >= 0)
    return bool(in_triangle(g, F, owner[ys, xs], xs, ys).all())


def faces_with_interior_pixel(g, F, W, H):
    """Faces that have a pixel centre of the frame strictly inside: such a pixel can belong to no other face of a sheet."""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.array([in_triangle(g, F, np.full(xs.shape, f), xs, ys, strict=True).any() for f in range(len(F))])


def lattice_case(k, seed, unshared=False):
    x0, y0, step, z = LATTICES[k]
    rng = np.random.default_rng(1000 * k + seed)
    V, F, quad = lattice(x0, y0, LATTICE_NX, LATTICE_NY, step, z, rng, K_LATTICE, unshared)
    return dict(V=V, F=F, quad=quad, z=z, K=K_LATTICE, R=EYE, t=ZERO, W=LATTICE_W, H=LATTICE_H,
                rect=rect_mask(x0, y0, LATTICE_NX, LATTICE_NY, step, LATTICE_W, LATTICE_H))


def check_lattice_coverage(depth, case):
    """Case 1: covered exactly the half-open rectangle, depth z inside.  Returns a message, None when met."""
    cov = np.asarray(depth) > 0
    if not np.array_equal(cov, case["rect"]):
        return "coverage differs from the half-open rectangle at %d pixels (%d holes, %d extra)" % (
            (cov != case["rect"]).sum(), (case["rect"] & ~cov).sum(), (cov & ~case["rect"]).sum())
    if not (np.asarray(depth)[cov] == case["z"]).all():
        return "depth differs from z inside"
    return None


def check_owners(owner, case):
    """Case 2: the owner map covers the rectangle, every owner contains its pixel, and every face that has a pixel centre
    strictly inside owns a pixel (both triangles of every quad inside the frame are such faces)."""
    g = grid256(case["V"], case["K"])
    assert np.array_equal(owner >= 0, case["rect"])
    assert owner.max() < len(case["F"])
    assert owners_contain(owner, g, case["F"])
    must = faces_with_interior_pixel(g, case["F"], case["W"], case["H"])
    owns = np.bincount(owner[owner >= 0], minlength=len(case["F"])) > 0
    assert owns[must].all()
    return must


# ---- case 3: depth ties ------------------------------------------------------------------------------
def _tilted(seed, sx, sy, x0=4, y0=3, nx=5, ny=4, step=6):
    rng = np.random.default_rng(seed)
    V, F, _ = lattice(x0, y0, nx, ny, step, 256, rng, K_LATTICE, unshared=True)
    V = V.copy()
    V[:, 2] += np.float32(sx) * V[:, 0] + np.float32(sy) * V[:, 1]
    return V, F, rng


def _shuffled(V, F, rng):
    perm = rng.permutation(len(F))
    Vn, Fn = unshare(V, np.asarray(F)[perm])
    return Vn, Fn, perm


def tie_case(seed=7):
    """A tilted sheet whose face list is there twice, the copy with vertices (so colours) of its own, all 2 nf faces in
    shuffled positions: every fragment has a twin at exactly its depth.  twin[f] = the face coincident with f."""
    V, F, rng = _tilted(seed, 0.35, -0.2)
    nf = len(F)
    V2, F2 = np.concatenate([V, V]), np.concatenate([F, F + len(V)])
    Vn, Fn, perm = _shuffled(V2, F2, rng)
    pos = np.argsort(perm)                                             # pos[old face] = its new index
    twin = np.empty(2 * nf, np.int64)
    twin[pos] = pos[(np.arange(2 * nf) + nf) % (2 * nf)]
    return dict(V=Vn, F=Fn, twin=twin, K=K_LATTICE, R=EYE, t=ZERO, W=LATTICE_W, H=LATTICE_H)


def crossing_case(seed=11):
    """Two sheets tilted against each other: they interpenetrate along the pixel column x = 16 (X = 0), where both are at z = 256."""
    Va, Fa, rng = _tilted(seed, 0.5, 0.1, x0=2, nx=7, step=4)
    Vb, Fb, _ = _tilted(seed + 1, -0.5, -0.05, x0=2, nx=7, step=4)
    Vn, Fn, _ = _shuffled(np.concatenate([Va, Vb]), np.concatenate([Fa, Fb + len(Va)]), rng)
    return dict(V=Vn, F=Fn, K=K_LATTICE, R=EYE, t=ZERO, W=LATTICE_W, H=LATTICE_H)


# ---- case 4: the ray caster ----------------------------------------------------------------------------
K_RAY = np.array([[572.4114, 0, 80], [0, 573.57043, 60], [0, 0, 1]], np.float32)
RAY_W, RAY_H = 160, 120


def ray_cases():
    from synth import icosphere
    V, F, _, _ = icosphere(2)
    s = 80.0
    Vc = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], np.float32)
    Fc = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    a, b = np.radians(33.0), np.radians(-21.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]); Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Kc = (np.array([572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1], np.float32).reshape(3, 3) * np.array([[.25], [.25], [1]], np.float32))
    common = dict(W=RAY_W, H=RAY_H)
    return [
        dict(name="sphere", V=V, F=F, K=K_RAY, R=rot("y", 0.7), t=np.array([5, -3, 600], np.float32), clip=(10.0, 10000.0), **common),
        dict(name="sphere cut by the right edge", V=V, F=F, K=K_RAY, R=(rot("x", -0.4) @ rot("y", 2.1)).astype(np.float32),
             t=np.array([78, 12, 560], np.float32), clip=(10.0, 10000.0), **common),
        dict(name="cube 0", V=Vc, F=Fc, K=Kc, R=(Rx @ Ry).astype(np.float32), t=np.array([150, -90, 420], np.float32), clip=(100.0, 2000.0), **common),
        dict(name="cube 1", V=Vc, F=Fc, K=Kc, R=(Ry @ Rx).astype(np.float32), t=np.array([-260, 140, 380], np.float32), clip=(100.0, 2000.0), **common),
    ]


def check_against_rays(depth, z_ray, where=None):
    """The two conditions of case 4 on a uint16 depth image: coverage equals the rays' hits, and |d - floor(z_ray)| <= 1 on
    every covered pixel.  where: restrict both to these pixels.  Returns the largest |d - floor(z_ray)|."""
    d = np.asarray(depth, np.int64)
    where = np.ones(d.shape, bool) if where is None else where
    hit = np.isfinite(z_ray)
    assert np.array_equal((d > 0) & where, hit & where), "coverage differs from the rays at %d pixels" % (((d > 0) != hit) & where).sum()
    m = (d > 0) & where
    assert m.any()
    err = np.abs(d[m] - np.floor(z_ray[m]).astype(np.int64)).max()
    assert err <= 1, err
    return int(err)


# ---- case 5: vertices at and behind the camera plane ----------------------------------------------------
def behind_case():
    """A floor (Y = 16 mm under the optical axis) that runs from in front of the camera to behind it, 64 x 48, f = 64.  Rows of
    vertices at p_z = -64, (-8, 0, -8), 64, 128, 256: with t_z = 32 every sum is exact.  All projections of the rows in front
    are multiples of 1/256 pixel, so the steep perspective carries no snapping error.  front[f]: all three p_z > 0."""
    K = np.array([[64, 0, 32], [0, 64, 24.5], [0, 0, 1]], np.float32)     # c_y = 24.5: no outline edge through a pixel centre, where
    t = np.array([0, 0, 32], np.float32)                                  # the fill rule and the (closed) ray caster would differ
    zrows = [[-96, -96, -96], [-40, -32, -40], [32, 32, 32], [96, 96, 96], [224, 224, 224]]
    Vg = np.array([[(j - 1) * 40.0, 16.0, zrows[i][j]] for i in range(5) for j in range(3)], np.float32)
    rng = np.random.default_rng(5)
    faces = []
    for i in range(4):
        for j in range(2):
            a, b, c, d = 3 * i + j, 3 * i + j + 1, 3 * (i + 1) + j + 1, 3 * (i + 1) + j
            for tri in ([(a, b, c), (a, c, d)] if (i + j) % 2 else [(a, b, d), (b, c, d)]):
                faces.append(tri if rng.integers(2) else (tri[0], tri[2], tri[1]))
    F = np.array(faces, np.int32)[rng.permutation(len(faces))]
    pz = Vg[:, 2].astype(np.float64) + 32.0                            # exact
    nbehind = (pz[F] <= 0).sum(1)
    assert set(nbehind.tolist()) == {0, 1, 2, 3} and (pz == 0).sum() == 1
    return dict(V=Vg, F=F, K=K, R=EYE, t=t, W=64, H=48, clip=(1.0, 10000.0), front=nbehind == 0)


# ---- case 6: the 1e9 guard ------------------------------------------------------------------------------
def guard_cases():
    """beyond: a vertex at p_z = 1e-7, x = 50 mm: 256 u = 256 (256 * 50 / 1e-7 + 32) = 3.3e13, past the guard -> the triangle is not
    drawn.  half: a vertex at p_z = 2^-7, x = 59.6 mm: 256 u = 5.0e8, inside the guard, two vertices on screen -> drawn."""
    K = np.array([[256, 0, 32], [0, 256, 24], [0, 0, 1]], np.float32)
    on_screen = [[-10.5, -14.25, 256.0], [13.0, 17.5, 300.0]]
    beyond = np.array(on_screen + [[50.0, 3.0, 1e-7]], np.float32)
    half = np.array(on_screen + [[59.6, 0.004, 2.0 ** -7]], np.float32)
    F = np.array([[0, 1, 2]], np.int32)
    u = 256.0 * (256.0 * half[2, 0].astype(np.float64) / half[2, 2] + 32.0)
    assert 4e8 < u < 6e8
    common = dict(F=F, K=K, R=EYE, t=ZERO, W=64, H=48, clip=(10.0, 10000.0))
    return dict(V=beyond, **common), dict(V=half, **common)


# ---- case 8: clip planes ---------------------------------------------------------------------------------
def clip_case():
    """One big quad, z from 150 mm (left) to 900 mm (right) across a 96 x 64 frame that it overfills; clip planes at 300 and 600."""
    K = np.array([[128, 0, 48], [0, 128, 32], [0, 0, 1]], np.float32)
    V = np.array([[-68.3, -310.7, 150.0], [409.1, -297.2, 900.0], [405.6, 305.9, 900.0], [-70.9, 301.3, 150.0]], np.float32)
    F = np.array([[0, 1, 2], [0, 3, 2]], np.int32)
    return dict(V=V, F=F, K=K, R=EYE, t=ZERO, W=96, H=64, clip=(300.0, 600.0))


def check_clip_against_rays(depth, z_ray, near, far):
    """Coverage equals near <= z_ray <= far outside a band of RAY_BOUND_MM around either plane.  Returns (excluded, covered)."""
    cov = np.asarray(depth) > 0
    band = (np.abs(z_ray - near) < RAY_BOUND_MM) | (np.abs(z_ray - far) < RAY_BOUND_MM)
    want = (z_ray >= near) & (z_ray <= far)
    assert np.array_equal(cov & ~band, want & ~band)
    excluded, covered = int(band.sum()), int(cov.sum())
    assert covered > 1000 and excluded < 0.02 * covered, (excluded, covered)
    return excluded, covered


# ---- case 9: uint16 ----------------------------------------------------------------------------------------
U16_Z = [(65534.9, 65534), (65535.0, 65535), (65535.5, 65535), (70000.0, 65535)]
U16_W, U16_H = 16, 12
K_U16 = np.array([[256, 0, 8], [0, 256, 6], [0, 0, 1]], np.float32)


def sheet(z, W=U16_W, H=U16_H, K=K_U16, margin=3.0):
    """A fronto-parallel quad at depth z that overfills the frame by margin pixels on every side."""
    K = np.asarray(K, np.float64)
    X = [(-margin - K[0, 2]) * z / K[0, 0], (W + margin - K[0, 2]) * z / K[0, 0]]
    Y = [(-margin - K[1, 2]) * z / K[1, 1], (H + margin - K[1, 2]) * z / K[1, 1]]
    V = np.array([[X[0], Y[0], z], [X[1], Y[0], z], [X[1], Y[1], z], [X[0], Y[1], z]], np.float32)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# ---- case 10: supersampling -------------------------------------------------------------------------------
SSAA_COLOUR = (200, 100, 50)
SSAA_FACTORS = (1, 2, 3, 8)


def ssaa_expected(x0, y0, nx, ny, step, W, H, ssaa, colour=SSAA_COLOUR):
    """Box average of the rectangle at ssaa x: sample (X, Y) of the ssaa grid is inside iff ssaa x0 <= X < ssaa (x0 + nx step)
    (in quarter pixels, all integers); pixel = floor((2 k c + n) / (2 n)), k samples inside of n = ssaa^2."""
    q = lambda v: int(round(4 * v * ssaa))
    assert all(abs(4 * v * ssaa - q(v)) == 0 for v in (x0, y0, x0 + nx * step, y0 + ny * step))
    X, Y = 4 * np.arange(W * ssaa, dtype=np.int64), 4 * np.arange(H * ssaa, dtype=np.int64)
    inx = ((X >= q(x0)) & (X < q(x0 + nx * step))).reshape(W, ssaa).sum(1)
    iny = ((Y >= q(y0)) & (Y < q(y0 + ny * step))).reshape(H, ssaa).sum(1)
    k = iny[:, None] * inx[None, :]
    n = ssaa * ssaa
    return np.stack([(2 * k * c + n) // (2 * n) for c in colour], -1).astype(np.uint8), k


# ---- case 7: a NaN or Inf pose inside a batch ---------------------------------------------------------------
def pose_batch():
    """Five views of a lattice; R of view 2 is all NaN, t of view 3 all +inf: those two render nothing."""
    c = lattice_case(0, 0)
    Rs = np.tile(EYE, (5, 1, 1))
    ts = np.array([[0, 0, 0], [3, -2, 0], [0, 0, 0], [0, 0, 0], [-5, 4, 64]], np.float32)
    Rs[2] = np.nan
    ts[3] = np.inf
    return c, Rs, ts, (2, 3)
