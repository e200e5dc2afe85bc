"""The selectable response table (Detector.setResponseTable) stated in numpy, and the shared inputs of its tests.

A feature of label `ori` scores r[d] at a position, d = the cyclic distance (0..4, eight orientations) between ori and the nearest
orientation bit set in the spread byte there, and 0 where no bit is set.  r = (4, 1, 0, 0, 0) is the table the oracle (and the reference's
golden file behind it) has built in; the oracle's match half takes linear memories as input, so the memories of any other table are built
here and handed to it unchanged."""
import functools
import itertools

import numpy as np

import linemod_oracle as lo
import synth

NAMED = {"linemod": (4, 3, 2, 1, 0), "drop1": (4, 2, 1, 0, 0), "drop1_keep3": (4, 3, 1, 0, 0), "levelup": (4, 1, 0, 0, 0),
         "levelup2": (4, 2, 0, 0, 0)}
DEFAULT = NAMED["levelup"]


def legal_tables():
    """r[0] == 4, non-increasing, values 0..4: 70 tables."""
    return [(4,) + t for t in itertools.product(range(5), repeat=4) if all(a >= b for a, b in zip((4,) + t, t))]


def distinct_nonzero(r):
    return len(set(v for v in r if v))


def response_np(spread, r):
    """(8,) + spread.shape u8: max over the set bits b of r[min(|b - ori|, 8 - |b - ori|)], 0 when no bit is set."""
    spread = np.asarray(spread, np.uint8)
    out = np.zeros((8,) + spread.shape, np.uint8)
    for ori in range(8):
        for b in range(8):
            d = min(abs(b - ori), 8 - abs(b - ori))
            out[ori] = np.maximum(out[ori], np.where((spread >> b) & 1, np.uint8(r[d]), np.uint8(0)))
    return out


def linear_memory(quantised, T, r):
    """One modality of one level: flat u8 [8][T*T][(W/T)*(H/T)] + the oracle's zero tail (the layout of lo.build_linear_memories)."""
    H, W = quantised.shape
    resp = response_np(lo.spread_np(np.ascontiguousarray(quantised, np.uint8), T), r)
    out = np.zeros(8 * W * H + lo.lm_tail_pad(W // T, H // T), np.uint8)
    out[:8 * W * H] = np.concatenate([lo.linearize_np(resp[ori], T).reshape(-1) for ori in range(8)])
    return out


def linear_memories(pyr, T, r):
    """The whole pyramid, as lo.match_bank_c expects it: (lms[level][modality], sizes[level] = (W, H)).  pyr[l] = (colour, normals, ...)."""
    lms = [[linear_memory(p[0], T[l], r), linear_memory(p[1], T[l], r)] for l, p in enumerate(pyr)]
    return lms, [(p[0].shape[1], p[0].shape[0]) for p in pyr]


# ---- the inputs shared by test_response_table_ref.py (condition on the inputs) and test_gpu_response_table.py ------------------------------
# Geometries: the smallest that reach every writer and both passes.  G1: dword rows at both levels; G2: the reference's default T, 15 cells per
# row at level 1 (the byte-store body, rows that are no whole dwords); G3: three levels.
GEOMETRIES = {"G1": (192, 160, (4, 8)), "G2": (240, 160, (5, 8)), "G3": (256, 192, (4, 4, 8))}
FRAME_SEED = {"G1": 31, "G2": 32, "G3": 33}
# Thresholds per bank kind and table: scores of different tables are not comparable (the denominator stays 4 * features), so every table has
# its own; chosen on the CPU so that every bank yields matches under every table and the lists differ from the default table's.
THRESHOLDS = {
    "planted": {"levelup": 70.0, "levelup2": 72.0, "linemod": 84.0, "drop1": 74.0, "drop1_keep3": 78.0},
    "small": {"levelup": 70.0, "levelup2": 72.0, "linemod": 84.0, "drop1": 74.0, "drop1_keep3": 78.0},
    "random": {"levelup": 30.0, "levelup2": 38.0, "linemod": 60.0, "drop1": 42.0, "drop1_keep3": 50.0},
}
BANKS = ("planted", "small", "random")


def _nfeat(kind, levels):
    base = {"planted": 150, "small": 60, "random": 150}[kind]      # "small": fewer than 64 features per modality, the oracle's 8-bit path
    return tuple(max(8, base >> l) for l in range(levels))


@functools.lru_cache(maxsize=None)
def scene(geom):
    """frame, oracle detector, quantised pyramid and the three banks of a geometry (computed once per process)."""
    W, H, T = GEOMETRIES[geom]
    rgb, dep = synth.make_frame(FRAME_SEED[geom], W, H, 14)
    od = lo.OracleDetector(150, list(T))
    pyr = od.quantize_pyramid(rgb, dep)
    qp = [(p[0], p[1]) for p in pyr]
    rng = np.random.default_rng(1000 + FRAME_SEED[geom])
    border = 8 * T[0] + 2
    windows = []
    for _ in range(40):                                            # templates of 48..100 px: room inside the refinement border
        w, h = int(rng.integers(48, min(100, W - 2 * border - 2))), int(rng.integers(40, min(100, H - 2 * border - 2)))
        windows.append((int(rng.integers(border, W - w - border)), int(rng.integers(border, H - h - border)), w, h))
    banks = {
        "planted": synth.make_planted_bank(41, 40, qp, list(T), _nfeat("planted", len(T)), windows=windows),
        "small": synth.make_planted_bank(42, 24, qp, list(T), _nfeat("small", len(T)), windows=windows[:24]),
        "random": _shrunk_random_bank(43, 40, W, H, _nfeat("random", len(T))),
    }
    return {"W": W, "H": H, "T": list(T), "rgb": rgb, "dep": dep, "od": od, "pyr": pyr, "banks": banks}


def _shrunk_random_bank(seed, n, W, H, nfeat):
    """synth.make_random_bank scales its templates by W / 640; at these frame sizes that leaves boxes of a dozen pixels, so the bank is drawn
    for a frame of twice the width (templates of 24..98 px here)."""
    return synth.make_random_bank(seed, n, 2 * W, H, nfeat)


@functools.lru_cache(maxsize=None)
def memories(geom, r):
    sc = scene(geom)
    return linear_memories(sc["pyr"], sc["T"], tuple(r))


@functools.lru_cache(maxsize=None)
def oracle(geom, kind, r, thr):
    """match_oracle.c on the spec's memories: (raw records with cls = 0, statistics)."""
    sc = scene(geom)
    feat, offs, wh = sc["banks"][kind]
    lms, sizes = memories(geom, tuple(r))
    P = (len(offs) - 1) // (2 * len(sc["T"]))
    raw, st = lo.match_bank_c(lo.PackedBank(P, len(sc["T"]), feat, offs, wh), lms, sizes, sc["T"], thr)
    raw["cls"] = 0
    return raw, st


def multiset(raw):
    return sorted(zip(raw["x"].tolist(), raw["y"].tolist(), raw["sim"].tolist(), raw["tid"].tolist()))
