"""Named, seeded cases for the ranking merge of csrc/exchange.hip (k_exchange_merge / rank_in_runs): W sorted runs of 128-bit keys whose
relative position is CHOSEN, so that every path of the routine is reached on purpose — a whole tile of another run below the chunk (counted
without being loaded), a tile above it (the loop breaks), runs of several 2048-key tiles, more runs than one boundary group holds
(group = 256 / tiles) — and so is the predecessor across runs that decides what std::unique drops.  Shared by tests/test_exchange_ref.py
(CPU: the cases are what they claim to be) and tests/test_gpu_exchange_keys.py (the kernel).

Every case keeps the kernels' contract: each run sorted, all keys of the case distinct, count <= capacity unless the case is a failure case.

    capacity  tiles  boundary group  worlds
    256       1      256             1, 2, 3, 257, 300
    4096      2      128             2, 129
    65536     32     8               3, 9
"""
import functools
import zlib

import numpy as np

import exchange_ref as xr

TILE = 2048          # kTile
CHUNK = 256          # kWG
_U64 = np.uint64

# background similarities: few values, so that many keys tie on similarity (template id decides) and on `hi` altogether (`lo` decides)
SIMS = np.array([97.5, 93.25, 90.0, 88.875, 84.5, 80.0625, 77.75, 75.0], np.float32)


class Case:
    """runs: per rank (hi, lo), sorted.  count / flags / cap_word: rank -> header word that differs from the honest one.  min_drops: records the
    case was built to have dropped by std::unique.  expect: None = the merged list; "none" = no list, any failure code; an int = that code."""

    def __init__(self, name, cap, runs, min_drops=0, count=None, flags=None, cap_word=None, expect=None, info=None, disjoint=None):
        self.name, self.cap, self.runs, self.min_drops = name, cap, runs, min_drops
        self.count, self.flags, self.cap_word, self.expect = count or {}, flags or {}, cap_word or {}, expect
        self.info = info or {}
        self.disjoint = disjoint          # "up" / "down": every key of rank r below / above every key of rank r + 1
        self.world = len(runs)

    def words(self):
        """[world][4 + 4 * cap] uint32: the blocks as an all-gather lays them out."""
        return np.stack([xr.block(run, self.cap, self.count.get(r), self.flags.get(r, 0), self.cap_word.get(r)) for r, run in enumerate(self.runs)])

    def counts(self):
        return [len(r[0]) for r in self.runs]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def pool(rng, n):
    """n distinct keys in ascending order: even template ids below 128 (odd ones are free for planted duplicates), classes below 128."""
    m = n + n // 4 + 64
    hi, lo = xr.make_key(rng.integers(-200, 800, m), rng.integers(-100, 600, m), SIMS[rng.integers(0, len(SIMS), m)], rng.integers(0, 128, m),
                         2 * rng.integers(0, 64, m))
    hi, lo = xr.sort_keys(hi, lo)
    keep = np.ones(m, bool)
    keep[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    idx = np.flatnonzero(keep)
    assert len(idx) >= n
    idx = np.sort(rng.choice(idx, n, replace=False))
    return hi[idx], lo[idx]


def mixed_counts(cap, world, shift=0):
    mix = sorted({c for c in (0, 1, 255, 256, 257, 2047, 2048, 2049, cap - 1, cap) if c <= cap})
    return [mix[(r * 7 + shift) % len(mix)] for r in range(world)]       # 7 is coprime to every length of `mix`: all values occur


def interleaved(rng, counts):
    """Random keys dealt to the ranks."""
    hi, lo = pool(rng, sum(counts))
    deal = rng.permutation(len(hi))
    runs, o = [], 0
    for c in counts:
        i = np.sort(deal[o:o + c])
        runs.append((hi[i], lo[i]))
        o += c
    return runs


def staircase(rng, counts, down=False):
    """Every key of rank r below (down: above) every key of rank r + 1."""
    hi, lo = pool(rng, sum(counts))
    runs, o = [None] * len(counts), 0
    for r in (range(len(counts) - 1, -1, -1) if down else range(len(counts))):
        runs[r] = (hi[o:o + counts[r]], lo[o:o + counts[r]])
        o += counts[r]
    return runs


def segments(rng, world, segs):
    """segs: (rank, length) pieces of the sorted pool, in ascending key order."""
    hi, lo = pool(rng, sum(n for _, n in segs))
    parts, o = [[] for _ in range(world)], 0
    for r, n in segs:
        parts[r].append(np.arange(o, o + n))
        o += n
    out = []
    for p in parts:
        i = np.concatenate(p) if p else np.zeros(0, np.int64)
        out.append((hi[i], lo[i]))
    return out


def insert(run, hi, lo):
    h = np.concatenate([run[0], np.atleast_1d(np.asarray(hi, _U64))])
    l = np.concatenate([run[1], np.atleast_1d(np.asarray(lo, _U64))])
    return xr.sort_keys(h, l)


def plant_dup(runs, src, idx, dst):
    """A record on rank dst that equals key idx of rank src except for the template id (+ 1), and directly follows it in the merged order: every
    key of the case between the two is removed.  Returns the index of the new key in rank dst's run."""
    h, l = runs[src][0][idx], runs[src][1][idx]
    for r, (hi, lo) in enumerate(runs):
        between = ((hi == h) & (lo > l)) | ((hi == h + _U64(1)) & (lo <= l))
        runs[r] = (hi[~between], lo[~between])
    assert runs[src][0][idx] == h and runs[src][1][idx] == l          # what was removed lies above the source key
    runs[dst] = insert(runs[dst], h + _U64(1), l)
    at = np.flatnonzero((runs[dst][0] == h + _U64(1)) & (runs[dst][1] == l))
    assert len(at) == 1
    return int(at[0])


# ---- layouts --------------------------------------------------------------------------------------------------------------------------------
def _layout(name, cap, world, kind, shift=0):
    rng = _rng(name)
    counts = mixed_counts(cap, world, shift)
    if kind == "interleaved":
        return Case(name, cap, interleaved(rng, counts))
    return Case(name, cap, staircase(rng, counts, down=(kind == "down")), disjoint=kind)


def _explicit(name, cap, counts, kind="interleaved"):
    rng = _rng(name)
    if kind == "interleaved":
        return Case(name, cap, interleaved(rng, counts))
    return Case(name, cap, staircase(rng, counts, down=(kind == "down")), disjoint=kind)


def _tile_staircase(name, cap, world, segs):
    return Case(name, cap, segments(_rng(name), world, segs))


# ---- duplicates across runs -----------------------------------------------------------------------------------------------------------------
def _dup_chains(name):
    """Chains of 2 and of 3 = W records equal in (x, y, similarity, class) on different ranks, on similarities nothing else has (so each chain is
    contiguous in the merged order), and a near-duplicate — the similarity differs in the last bit — that must be kept."""
    rng = _rng(name)
    runs = interleaved(rng, [200, 129, 77])
    add = [(0, (5, 6, 91.125, 3, 11)), (2, (5, 6, 91.125, 3, 12)),                                       # chain of 2: drops 1
           (0, (-7, 300, 91.25, 0, 1)), (1, (-7, 300, 91.25, 0, 2)), (2, (-7, 300, 91.25, 0, 3)),        # chain of 3: drops 2
           (1, (40, 41, np.float32(91.375), 9, 5)), (2, (40, 41, np.nextafter(np.float32(91.375), np.float32(100)), 9, 6))]   # kept, both
    for r, (x, y, s, c, t) in add:
        runs[r] = insert(runs[r], *xr.make_key(x, y, s, c, t))
    return Case(name, 256, runs, min_drops=3)


def _dup_chain_world(name, world):
    """One chain through ALL ranks: rank r holds (x, y, s, class) under template id r."""
    rng = _rng(name)
    runs = interleaved(rng, [c and c - 1 for c in mixed_counts(256, world)])
    for r in range(world):
        runs[r] = insert(runs[r], *xr.make_key(17, -4, 91.5, 2, r))
    return Case(name, 256, runs, min_drops=world - 1)


def _dup_skipped_tile(name, cap, counts, down=False):
    """A staircase whose neighbouring ranks meet in a duplicate: the first key of the upper rank equals the last key of the lower one except for
    the template id.  Seen from the upper rank's first chunk, the lower rank's last tile lies wholly below: the kernel counts it without loading
    it, and the predecessor that marks the duplicate is that tile's last key."""
    rng = _rng(name)
    runs = staircase(rng, counts, down=down)
    order = list(range(len(counts) - 1, -1, -1)) if down else list(range(len(counts)))
    planted = []
    for lower, upper in zip(order[:-1], order[1:]):
        if len(runs[lower][0]) == 0:
            continue
        src_idx = len(runs[lower][0]) - 1
        at = plant_dup(runs, lower, src_idx, upper)
        planted.append((upper, at, lower, src_idx))
    return Case(name, cap, runs, min_drops=len(planted), info={"skipped": planted}, disjoint="down" if down else "up")


def _dup_same_run(name):
    """The predecessor that marks the duplicate is in the record's OWN run (run(self)[idx - 1]): inside a chunk, across the boundary of two
    256-key chunks, and across a tile boundary."""
    rng = _rng(name)
    runs = interleaved(rng, [3000, 2500])
    planted = []
    for src_idx in (100, 255, 2047):           # ascending: planting a key moves only what lies above it
        at = plant_dup(runs, 0, src_idx, 0)
        assert at == src_idx + 1
        planted.append(at)
    return Case(name, 4096, runs, min_drops=3, info={"same_run": planted})


# ---- field extremes -------------------------------------------------------------------------------------------------------------------------
def _extremes(name):
    """x, y at -32768 / 32767, similarity 0, 100, the smallest denormal and two values one ulp apart, template id 0 / 2^31 - 1, class 0 / 127, in
    every combination: keys that agree in `hi` and differ in `lo` and the other way round (both branches of key_less)."""
    rng = _rng(name)
    s = np.float32(61.03125)
    sims = np.array([0.0, 100.0, np.finfo(np.float32).smallest_subnormal, s, np.nextafter(s, np.float32(100))], np.float32)
    g = np.array(np.meshgrid([-32768, 32767], [-32768, 32767], np.arange(len(sims)), [0, 127], [0, 2 ** 31 - 1], indexing="ij")).reshape(5, -1)
    hi, lo = xr.sort_keys(*xr.make_key(g[0], g[1], sims[g[2]], g[3], g[4]))
    rank = rng.integers(0, 3, len(hi))
    return Case(name, 256, [(hi[rank == r], lo[rank == r]) for r in range(3)])


# ---- failure blocks -------------------------------------------------------------------------------------------------------------------------
def _failure(name, **kw):
    return Case(name, 256, interleaved(_rng(name), [100, 256, 31]), **kw)


def _run_overflow(name, at, world=300):
    """Every rank holds 7 records but one, which reports 5000 of them for blocks of 256 (as the pack kernels do: count, flag, no keys)."""
    counts = [7] * world
    counts[at] = 0
    return Case(name, 256, interleaved(_rng(name), counts), count={at: 5000}, flags={at: xr.RUN_OVERFLOW}, expect=5000, info={"others": 7})


BUILDERS = {
    # capacity 256: one tile per run, one boundary group of 256 runs
    "c256_w1_full": lambda n: _explicit(n, 256, [256]),
    "c256_w1_one": lambda n: _explicit(n, 256, [1]),
    "c256_w2_interleaved": lambda n: _explicit(n, 256, [256, 255]),
    "c256_w3_interleaved": lambda n: _explicit(n, 256, [255, 0, 256]),
    "c256_w3_up": lambda n: _explicit(n, 256, [256, 1, 255], "up"),
    "c256_w3_down": lambda n: _explicit(n, 256, [255, 256, 1], "down"),
    "c256_w257_interleaved": lambda n: _layout(n, 256, 257, "interleaved"),
    "c256_w257_up": lambda n: _layout(n, 256, 257, "up", 1),
    "c256_w300_interleaved": lambda n: _layout(n, 256, 300, "interleaved", 2),
    "c256_w300_down": lambda n: _layout(n, 256, 300, "down", 3),
    "c256_w300_all_empty": lambda n: _explicit(n, 256, [0] * 300),
    "c256_w300_only_last": lambda n: _explicit(n, 256, [0] * 299 + [255]),
    "c256_w300_only_one": lambda n: _explicit(n, 256, [0] * 5 + [256] + [0] * 294),
    # capacity 4096: two tiles per run, boundary groups of 128 runs
    "c4096_w2_interleaved": lambda n: _explicit(n, 4096, [4096, 4095]),
    "c4096_w2_up": lambda n: _explicit(n, 4096, [2049, 2047], "up"),
    "c4096_w2_down": lambda n: _explicit(n, 4096, [2048, 4096], "down"),
    "c4096_w2_tiles": lambda n: _tile_staircase(n, 4096, 2, [(0, 256), (1, 2048), (0, 256), (1, 2047), (0, 255)]),
    "c4096_w129_interleaved": lambda n: _layout(n, 4096, 129, "interleaved"),
    "c4096_w129_up": lambda n: _layout(n, 4096, 129, "up", 4),
    # capacity 65536: 32 tiles per run, boundary groups of 8 runs
    "c65536_w3_interleaved": lambda n: _explicit(n, 65536, [65536, 2049, 65535]),
    "c65536_w3_tiles": lambda n: _tile_staircase(n, 65536, 3, [s for i in range(10) for s in ((0, 256), (1 + i % 2, 2048))] + [(1, 1), (0, 1)]),
    "c65536_w9_interleaved": lambda n: _explicit(n, 65536, [65535, 0, 1, 257, 2047, 2048, 2049, 65536, 255]),
    "c65536_w9_up": lambda n: _explicit(n, 65536, [2049, 0, 4097, 2047, 256, 1, 2048, 257, 6000], "up"),
    "c65536_w9_down": lambda n: _explicit(n, 65536, [2047, 2048, 1, 0, 2049, 255, 4096, 300, 257], "down"),
    # duplicates across runs
    "dup_chains": _dup_chains,
    "dup_chain_w3": lambda n: _dup_chain_world(n, 3),
    "dup_chain_w257": lambda n: _dup_chain_world(n, 257),
    "dup_skipped_c256_w3": lambda n: _dup_skipped_tile(n, 256, [255, 200, 100]),
    "dup_skipped_c256_w3_down": lambda n: _dup_skipped_tile(n, 256, [100, 200, 255], down=True),
    "dup_skipped_c4096_w2": lambda n: _dup_skipped_tile(n, 4096, [4096, 2049]),
    "dup_skipped_c65536_w3": lambda n: _dup_skipped_tile(n, 65536, [2049, 4100, 300]),
    "dup_same_run": _dup_same_run,
    "extremes": _extremes,
    # failure blocks
    "fail_capacity_word": lambda n: _failure(n, cap_word={1: 512}, expect="none"),
    "fail_field_overflow": lambda n: _failure(n, flags={2: xr.FIELD_OVERFLOW}, expect=-xr.FIELD_OVERFLOW),
    "fail_cand_overflow": lambda n: _failure(n, flags={0: xr.CAND_OVERFLOW}, expect=-xr.CAND_OVERFLOW),
    "fail_run_overflow_r0": lambda n: _run_overflow(n, 0),
    "fail_run_overflow_r247": lambda n: _run_overflow(n, 247),
    "fail_run_overflow_r248": lambda n: _run_overflow(n, 248),
    "fail_run_overflow_r299": lambda n: _run_overflow(n, 299),
}
NAMES = list(BUILDERS)
MERGE_NAMES = [n for n in NAMES if not n.startswith("fail_")]
FAIL_NAMES = [n for n in NAMES if n.startswith("fail_")]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name](name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """merge_expected of the case: computed once, shared by the tests; treat as read-only."""
    return xr.merge_expected(case(name).runs)


# ---- key buffers for the pack kernels (k_exchange_sort256 / k_exchange_merge256: tests/cpp/exchange_pack_keys.cpp) ---------------------------
PACK_ARRANGEMENTS = ("random", "sorted", "reversed", "equal_hi", "chunks_up", "chunks_down")


def pack_sizes(cap):
    return sorted({n for n in (0, 1, 2, 255, 256, 257, 511, 512, 513, 2048, 2049, cap - 1, cap) if n <= cap})


def pack_keys(name, n, arrangement):
    """n distinct keys as the detector's key buffer could hold them, (hi, lo) in buffer order."""
    rng = _rng(name)
    if arrangement == "equal_hi":                     # one similarity, one template: the order is decided by `lo` alone
        v = rng.choice(1 << 22, n, replace=False)
        hi, lo = xr.make_key(v & 0x7FF, (v >> 11) & 0x7FF, 88.5, 3, 9)
        return hi, lo
    hi, lo = pool(rng, n)
    if arrangement == "random":
        p = rng.permutation(n)
    elif arrangement == "sorted":
        p = np.arange(n)
    elif arrangement == "reversed":
        p = np.arange(n)[::-1]
    else:                                             # 256-key chunks with disjoint ranges, ascending / descending, shuffled inside
        p = np.concatenate([rng.permutation(np.arange(s, min(n, s + CHUNK))) for s in range(0, n, CHUNK)]) if n else np.zeros(0, np.int64)
        if arrangement == "chunks_down":              # chunk b of the buffer holds the b-th range from the top
            p = n - 1 - p
    return hi[p], lo[p]
