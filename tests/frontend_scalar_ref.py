"""A per-pixel restatement of the front end's quantisation in Python integers (they cannot overflow), written from the reference's lines and
sharing no code with the oracle's vector statement (oracle/linemod_oracle.py):

  * quantizedNormals before the median (LL.cpp:729-817): accumBilateral over the eight taps, the 2 x 2 solve, the float steps as single
    float32 operations in the reference's order, the flat read of NORMAL_LUT[v3][v2][v1] — and cv::medianBlur(5) as the 13th smallest of the
    25 replicate-border taps;
  * of quantizedOrientations / hysteresisGradient (LL.cpp:395-504): the channel pick, cv::phase, the 16-bin code & 7 inside the border and the
    3 x 3 vote.  Blur and Sobel are taken from the oracle (dx3, dy3).

The three strict comparisons can be exchanged for their non-strict mutants (`lt`, `dist_lt`, `gt`): the tests show that the frames built for
a comparison tell the two apart."""
import math
import operator

import numpy as np

f32 = np.float32
TAPS = ((-5, -5), (0, -5), (5, -5), (-5, 0), (5, 0), (-5, 5), (0, 5), (5, 5))          # l_offset0 .. l_offset7, LL.cpp:741-748


def normal_lut_entry(v3, v2, v1):
    """NORMAL_LUT[v3][v2][v1] read as the reference reads memory: a flat index into 20 x 20 x 20 bytes (an index of 20 runs into the next row /
    plane; past the last plane the table is taken to repeat — its planes are all equal).  The plane: the octant of atan2(v2 - 10, v1 - 10),
    half-octant borders rounded up."""
    flat = (v3 * 400 + v2 * 20 + v1) % 8000
    iy, ix = (flat % 400) // 20, flat % 20
    ang = math.degrees(math.atan2(iy - 10, ix - 10)) % 360.0
    return 1 << (int(math.floor(ang / 45.0 + 0.5)) % 8)


def raw_normals(depth, distance_threshold, difference_threshold, lt=operator.lt, dist_lt=operator.lt):
    H, W = depth.shape
    d = depth.astype(np.int64).tolist()
    out = np.zeros((H, W), np.uint8)
    r = 5
    for y in range(r, H - r - 1):                                                       # LL.cpp:753, 758
        for x in range(r, W - r - 1):
            l_d = d[y][x]
            if not dist_lt(l_d, distance_threshold):                                    # :762
                continue
            A0 = A1 = A3 = b0 = b1 = 0
            for i, j in TAPS:
                delta = d[y + j][x + i] - l_d
                f = 1 if lt(abs(delta), difference_threshold) else 0                    # :703
                fi, fj = f * i, f * j
                A0 += fi * i; A1 += fi * j; A3 += fj * j
                b0 += fi * delta; b1 += fj * delta
            det = A0 * A3 - A1 * A1                                                     # :777-779
            ddx = A3 * b0 - A1 * b1
            ddy = -A1 * b0 + A0 * b1
            nx, ny, nz = f32(1150 * ddx), f32(1150 * ddy), f32(-det * l_d)               # :783-785 (int -> float: round to nearest)
            sq = np.sqrt(f32(f32(f32(nx * nx) + f32(ny * ny)) + f32(nz * nz)))          # :787
            if sq > 0:
                inv = f32(f32(1.0) / sq)
                nx, ny, nz = f32(nx * inv), f32(ny * inv), f32(nz * inv)
                v1 = int(f32(f32(nx * f32(10)) + f32(10)))                              # :799-801 (truncation)
                v2 = int(f32(f32(ny * f32(10)) + f32(10)))
                v3 = int(f32(f32(nz * f32(20)) + f32(20)))
                out[y, x] = normal_lut_entry(v3, v2, v1)
    return out


def median5(img):
    """cv::medianBlur(5): the 13th smallest of the 5 x 5 window, BORDER_REPLICATE"""
    H, W = img.shape
    a = img.tolist()
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        rows = [a[min(max(y + j, 0), H - 1)] for j in range(-2, 3)]
        for x in range(W):
            cols = [min(max(x + i, 0), W - 1) for i in range(-2, 3)]
            out[y, x] = sorted(row[c] for row in rows for c in cols)[12]
    return out


def fast_atan2(y, x):
    """OpenCV's fastAtan2 (cv::phase in degrees), float32 step by step"""
    scale = f32(180.0 / math.pi)
    p1, p3 = f32(f32(0.9997878412794807) * scale), f32(f32(-0.3258083974640975) * scale)
    p5, p7 = f32(f32(0.1555786518463281) * scale), f32(f32(-0.04432655554792128) * scale)
    eps = f32(2.220446049250313e-16)
    x, y = f32(x), f32(y)
    ax, ay = abs(x), abs(y)
    if ax >= ay:
        c = f32(ay / f32(ax + eps))
        c2 = f32(c * c)
        a = f32(f32(f32(f32(f32(f32(f32(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
    else:
        c = f32(ax / f32(ay + eps))
        c2 = f32(c * c)
        a = f32(f32(90.0) - f32(f32(f32(f32(f32(f32(f32(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c))
    if x < 0:
        a = f32(f32(180.0) - a)
    if y < 0:
        a = f32(f32(360.0) - a)
    return a


def orientations(dx3, dy3, weak_threshold, gt=operator.gt):
    """(magnitude f32, quantised orientation u8) from the per-channel Sobel derivatives (H, W, 3)"""
    H, W = dx3.shape[:2]
    X, Y = dx3.astype(np.int64).tolist(), dy3.astype(np.int64).tolist()
    mag = np.zeros((H, W), np.float32)
    code = [[0] * W for _ in range(H)]
    with np.errstate(divide="ignore", invalid="ignore"):
        for y in range(H):
            for x in range(W):
                m = [X[y][x][c] * X[y][x][c] + Y[y][x][c] * Y[y][x][c] for c in range(3)]
                if m[0] >= m[1] and m[0] >= m[2]:                                       # LL.cpp:395
                    c = 0
                elif m[1] >= m[0] and m[1] >= m[2]:                                     # :401
                    c = 1
                else:
                    c = 2
                mag[y, x] = f32(m[c])
                if 0 < y < H - 1 and 0 < x < W - 1:                                     # :438-455: the border is zeroed, the rest masked to 0 .. 7
                    v = float(f32(fast_atan2(Y[y][x][c], X[y][x][c]) * f32(16.0 / 360.0)))
                    q = int(round(v))                                                   # cvRound: half to even (Python's round)
                    code[y][x] = min(max(q, 0), 255) & 7
    thr = f32(f32(weak_threshold) * f32(weak_threshold))                                # :424
    out = np.zeros((H, W), np.uint8)
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            if gt(mag[y, x], thr):                                                      # :466
                hist = [0] * 8
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        hist[code[y + j][x + i]] += 1
                votes, index = 0, -1
                for i in range(8):
                    if votes < hist[i]:                                                 # :491
                        index, votes = i, hist[i]
                if votes >= 5:                                                          # :500
                    out[y, x] = 1 << index
    return mag, out
