"""The bit planes of the "wide" matching paths (Detector.setPaths("wide", "wide"); match_wide.hip) stated in numpy:
the encoding of the response bytes into two sets of strip records / pair streams, and the lane-level sum of k_local_wide.

What the detector does under "wide" depends on the table.
  * A table of three or four distinct non-zero values: a response v = 0..4 is three binary digits; set 0 holds digit 0 (v & 1) where the
    two-plane layout holds "is a" and digit 2 (v == 4) where it holds "is 4", set 1 holds digit 1 ((v >> 1) & 1) where set 0 holds digit 0
    and nothing else.  The sum of a position is c0 + 2 c1 + 4 c2, c_i = the number of features whose digit i is set there.
  * A table of at most two distinct non-zero values {a, 4}: exactly what "bits" does — set 0 is the two-plane packing ("is a", "is 4"), set 1
    is empty (the detector does not even allocate it) and the sum is a c0 + 4 c2.
weights(r) = (the weight of c0, 2, 4) covers both: (1, 2, 4) for the first kind, (a, 2, 4) with c1 = 0 for the second."""
import numpy as np

import response_table_ref as rt


def low_value(r):
    """the second distinct non-zero value of a two-plane table (None when 4 is the only one)"""
    vals = sorted(set(v for v in r if v and v != 4))
    assert len(vals) <= 1
    return vals[0] if vals else None


def weights(r):
    if rt.distinct_nonzero(r) > 2:
        return (1, 2, 4)
    return (low_value(r) or 1, 2, 4)


def digits(v, r):
    """response bytes -> three boolean arrays: what set 0 holds at bit 2c, set 1 at bit 2c, set 0 at bit 2c + 1"""
    v = np.asarray(v, np.uint8)
    if rt.distinct_nonzero(r) > 2:
        return (v & 1).astype(bool), ((v >> 1) & 1).astype(bool), v == 4
    a = low_value(r)
    return (v == a) if a else np.zeros(v.shape, bool), np.zeros(v.shape, bool), v == 4


def from_digits(d0, d1, d2, r):
    w = weights(r)
    return (w[0] * d0.astype(np.uint8) + w[1] * d1.astype(np.uint8) + w[2] * d2.astype(np.uint8)).astype(np.uint8)


# ---- levels below the top: strip records [8 labels][T*T phases][NS strips][Hd rows] of 64 bits, cells [16 s, 16 s + 32) of the row, two bits per cell
def strip_records(lm_flat, T, Wd, Hd, r):
    NS = (Wd + 15) // 16
    planes = lm_flat[:8 * T * T * Wd * Hd].reshape(8, T * T, Hd, Wd)
    pad = np.zeros((8, T * T, Hd, NS * 16 + 32), np.uint8)
    pad[..., :Wd] = planes
    d0, d1, d2 = digits(pad, r)
    w = np.uint64(1) << (2 * np.arange(32, dtype=np.uint64))
    sets = [np.zeros((8, T * T, NS, Hd), np.uint64) for _ in range(2)]
    for s in range(NS):
        seg = slice(16 * s, 16 * s + 32)
        sets[0][:, :, s, :] = (d0[..., seg].astype(np.uint64) * w).sum(axis=-1) + (d2[..., seg].astype(np.uint64) * (w << np.uint64(1))).sum(axis=-1)
        sets[1][:, :, s, :] = (d1[..., seg].astype(np.uint64) * w).sum(axis=-1)
    return sets


def unpack_strip_records(set0, set1, Wd, r):
    """-> response bytes [8][T*T][Hd][Wd], from the first 16 cells of every record (the second 16 repeat the next strip's first)"""
    def cells(rec, odd):
        bits = (rec[..., None] >> (2 * np.arange(16, dtype=np.uint64) + np.uint64(odd))) & np.uint64(1)      # [8][TT][NS][Hd][16]
        return np.moveaxis(bits, 2, 3).reshape(bits.shape[0], bits.shape[1], bits.shape[3], -1)[..., :Wd].astype(bool)
    assert not cells(set1, 1).any()
    return from_digits(cells(set0, 0), cells(set1, 0), cells(set0, 1), r)


def strip_overlap_ok(rec, Wd):
    """cells 16..31 of strip s are cells 0..15 of strip s + 1 (zero beyond the last strip)"""
    hi = rec >> np.uint64(32)
    nxt = np.zeros_like(rec)
    nxt[:, :, :-1, :] = rec[:, :, 1:, :] & np.uint64(0xFFFFFFFF)
    return np.array_equal(hi, nxt)


# ---- the top level: per 32 bytes of the flat memories (colour block, normal block, zero tails included) a pair of dwords
def pair_streams(lm_colour, lm_normal, T, Wd, Hd, npairs, r):
    block = npairs * 16
    flat = np.zeros(2 * block, np.uint8)
    n = 8 * T * T * Wd * Hd
    flat[:n] = lm_colour[:n]; flat[block:block + n] = lm_normal[:n]
    d0, d1, d2 = (d.reshape(npairs, 32) for d in digits(flat, r))
    w = np.uint32(1) << np.arange(32, dtype=np.uint32)
    sets = [np.zeros((npairs, 2), np.uint32) for _ in range(2)]
    sets[0][:, 0] = (d0.astype(np.uint32) * w).sum(axis=1); sets[0][:, 1] = (d2.astype(np.uint32) * w).sum(axis=1)
    sets[1][:, 0] = (d1.astype(np.uint32) * w).sum(axis=1)
    return sets


def unpack_pair_streams(set0, set1, r):
    def bits(col):
        return ((col[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool).reshape(-1)
    assert not set1[:, 1].any()
    return from_digits(bits(set0[:, 0]), bits(set1[:, 0]), bits(set0[:, 1]), r)


# ---- the lane-level sum of k_local_wide: 8 lanes per candidate, lane j = window rows 2j, 2j + 1; per feature two records from either set, one
# funnel shift per row; three bit-sliced Harley-Seal counters (cA / cB: set 0 of the lane's two rows, cC: digit 1 of both rows side by side)
def _csa(a, b, c):
    return a ^ b ^ c, (a & b) | (a & c) | (b & c)


def _add8(x, c):
    c[0], ta = _csa(c[0], x[0], x[1]); c[0], tb = _csa(c[0], x[2], x[3]); c[1], fa = _csa(c[1], ta, tb)
    c[0], ta = _csa(c[0], x[4], x[5]); c[0], tb = _csa(c[0], x[6], x[7]); c[1], fb = _csa(c[1], ta, tb)
    c[2], e = _csa(c[2], fa, fb)
    return e


def _add_eights(c, e1, e2):
    c[3], k16 = _csa(c[3], e1, e2)
    for k in range(4, len(c)):
        t = c[k] & k16; c[k] = c[k] ^ k16; k16 = t
    assert not k16.any()                                       # the counter holds the entry's features


def lane_counts(rec0, rec1, F, T, Hd, gx, gy, kn=9):
    """rec0 / rec1: [modality][8][T*T][NS][Hd] u64; F: rows (x, y, label, modality); window origin (gx, gy) in cells, the windows inside their
    planes.  -> (n1, n2, n4): per digit a list of kn dwords per lane, bit 2c = row 2j, bit 2c + 1 = row 2j + 1 of window column c."""
    lanes = np.arange(8)
    zero = np.zeros(8, np.uint32)
    cA, cB, cC = ([zero.copy() for _ in range(kn)] for _ in range(3))

    def window(rec, x, y, lab, m):
        cx, cy = x // T, y // T
        ph = (y % T) * T + (x % T)
        s2 = ((cx & 15) + (gx & 15)) << 1                      # 2 x (column class + window column): bit 5 = strip carry
        s = (cx >> 4) + (gx >> 4) + (s2 >> 5)
        rows = cy + gy + 2 * lanes
        assert rows.max() + 1 < Hd and s < rec.shape[3]
        sh = np.uint64(s2 & 31)                                # v_alignbit(hi, lo, s2)
        return [((rec[m, lab, ph, s, rows + k] >> sh) & np.uint64(0xFFFFFFFF)).astype(np.uint32) for k in range(2)]

    nfp = (len(F) + 7) // 8 * 8
    for f0 in range(0, nfp, 16):
        es = []
        for half in range(2):
            if f0 + 8 * half >= nfp:
                break
            xa, xb, xc = [], [], []
            for f in range(f0 + 8 * half, f0 + 8 * half + 8):
                if f < len(F):
                    a, b = window(rec0, *F[f])
                    c, d = window(rec1, *F[f])
                else:
                    a = b = c = d = zero                       # padding features read the zero plane
                xa.append(a); xb.append(b); xc.append(c | (d << np.uint32(1)))
            es.append((_add8(xa, cA), _add8(xb, cB), _add8(xc, cC)))
        for c, i in ((cA, 0), (cB, 1), (cC, 2)):
            _add_eights(c, es[0][i], es[1][i] if len(es) == 2 else zero)
    M, M2 = np.uint32(0x55555555), np.uint32(0xAAAAAAAA)
    n1 = [(cA[k] & M) | ((cB[k] << np.uint32(1)) & M2) for k in range(kn)]
    n4 = [((cA[k] >> np.uint32(1)) & M) | (cB[k] & M2) for k in range(kn)]
    return n1, cC, n4


def weighted_sum_wide(n1, n2, n4):
    """S = n1 + 2 n2 + 4 n4 bit-sliced (match_wide.hip): kn + 3 dwords per lane"""
    kn = len(n1)
    zero = np.zeros_like(n1[0])
    t, carry = [n1[0]], zero
    for k in range(1, kn + 2):
        s, carry = _csa(n1[k] if k < kn else zero, n2[k - 1] if k - 1 < kn else zero, carry)
        t.append(s)
    S, carry = [t[0], t[1]], zero
    for k in range(2, kn + 3):
        s, carry = _csa(t[k] if k < kn + 2 else zero, n4[k - 2] if k - 2 < kn else zero, carry)
        S.append(s)
    assert not carry.any()
    return S


def positions(sliced):
    """bit-sliced dwords per lane -> integers [16 rows][16 columns] of the window"""
    val = np.zeros((8, 32), np.int64)
    for k, d in enumerate(sliced):
        val += (((d[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(np.int64)) << k
    out = np.zeros((16, 16), np.int64)
    out[0::2] = val[:, 0::2]                                   # bit 2c: row 2j
    out[1::2] = val[:, 1::2]                                   # bit 2c + 1: row 2j + 1
    return out


def byte_window_sums(planes, F, T, gx, gy):
    """planes[modality]: [8][T*T][Hd][Wd] response bytes -> the 16 x 16 sums of the window at (gx, gy)"""
    out = np.zeros((16, 16), np.int64)
    for x, y, lab, m in F:
        cx, cy, ph = x // T, y // T, (y % T) * T + (x % T)
        out += planes[m][lab, ph, gy + cy:gy + cy + 16, gx + cx:gx + cx + 16]
    return out
