"""The rule of the multi-GPU exchange (csrc/exchange.hip) in numpy, host only: the 128-bit key of a match record, the merge of sorted
runs of keys into the list Detector::match returns (canonical order, then what std::unique drops), and the block a rank contributes to
the all-gather.  Written from the comment and code of xchg_make_key (csrc/lm_kernels.h); nothing here calls the library."""
import numpy as np

MATCH_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("similarity", np.float32), ("class_index", np.int32), ("template_id", np.int32)])

RUN_OVERFLOW, CAND_OVERFLOW, FIELD_OVERFLOW = 1, 2, 4       # kXchgRunOverflow, kXchgCandOverflow, kXchgFieldOverflow
HEADER_WORDS = 256                                           # kXchgHeaderWords
POISON = np.uint32(0xA5C3F00D)                               # unused key slots: not ~0 (the pack kernels' padding, which sorts last)

_U64 = np.uint64


def _orderable(bits):
    """uint32 that orders like the float whose bits are `bits`."""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def make_key(x, y, sim, cls, tid):
    """(hi, lo) uint64: hi = ~orderable(sim) << 32 | tid, lo = cls << 32 | (y + 32768) << 16 | (x + 32768)."""
    x, y, cls, tid = (np.atleast_1d(np.asarray(a, np.int64)) for a in (x, y, cls, tid))        # scalars give arrays of one key
    sim = np.atleast_1d(np.asarray(sim, np.float32))
    x, y, sim, cls, tid = np.broadcast_arrays(x, y, sim, cls, tid)
    assert x.size == 0 or (x.min() >= -32768 and x.max() <= 32767 and y.min() >= -32768 and y.max() <= 32767 and cls.min() >= 0 and tid.min() >= 0
                           and cls.max() < 2 ** 31 and tid.max() < 2 ** 31), "xchg_key_fits"
    u = ~_orderable(np.ascontiguousarray(sim).view(np.uint32))
    hi = (u.astype(_U64) << _U64(32)) | tid.astype(_U64)
    lo = (cls.astype(_U64) << _U64(32)) | ((y + 32768).astype(_U64) << _U64(16)) | (x + 32768).astype(_U64)
    return hi, lo


def split_key(hi, lo):
    """Inverse of make_key: x, y, sim (float32), cls, tid."""
    hi, lo = np.asarray(hi, _U64), np.asarray(lo, _U64)
    u = ~(hi >> _U64(32)).astype(np.uint32)
    bits = u ^ np.where(u >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))
    sim = np.ascontiguousarray(bits).view(np.float32)
    x = (lo & _U64(0xFFFF)).astype(np.int64) - 32768
    y = ((lo >> _U64(16)) & _U64(0xFFFF)).astype(np.int64) - 32768
    return x.astype(np.int32), y.astype(np.int32), sim, (lo >> _U64(32)).astype(np.int32), (hi & _U64(0xFFFFFFFF)).astype(np.int32)


def decode(hi, lo):
    """MATCH_DTYPE records of the keys, in their order."""
    x, y, sim, cls, tid = split_key(hi, lo)
    rec = np.zeros(len(x), MATCH_DTYPE)
    rec["x"], rec["y"], rec["similarity"], rec["class_index"], rec["template_id"] = x, y, sim, cls, tid
    return rec


def sort_keys(hi, lo):
    """The keys in ascending (hi, lo) order."""
    order = np.lexsort((lo, hi))
    return hi[order], lo[order]


def merge_expected(runs):
    """runs: list of (hi, lo).  Returns (kept, merged, dropped): `merged` = all records in ascending key order, `dropped[i]` = record i agrees
    with record i - 1 on x, y, similarity (float bits) and class — Match::operator== as std::unique applies it to a sorted list (the relation is
    an equivalence, so comparing with the predecessor and with the last record kept is the same) —, `kept` = merged[~dropped]."""
    hi = np.concatenate([np.asarray(r[0], _U64) for r in runs]) if runs else np.zeros(0, _U64)
    lo = np.concatenate([np.asarray(r[1], _U64) for r in runs]) if runs else np.zeros(0, _U64)
    hi, lo = sort_keys(hi, lo)
    merged = decode(hi, lo)
    dropped = np.zeros(len(merged), bool)
    if len(merged) > 1:
        a, b = merged[1:], merged[:-1]
        dropped[1:] = ((a["x"] == b["x"]) & (a["y"] == b["y"]) & (a["class_index"] == b["class_index"])
                       & (a["similarity"].view(np.uint32) == b["similarity"].view(np.uint32)))
    return merged[~dropped], merged, dropped


def key_words(hi, lo):
    """The keys as the uint32 words of an array of ulonglong2 {x = hi, y = lo} (little endian)."""
    k = np.empty((len(hi), 2), "<u8")
    k[:, 0], k[:, 1] = hi, lo
    return k.reshape(-1).view("<u4")


def block(keys, cap, count=None, flags=0, cap_word=None):
    """The uint32 words of one rank's block: {count, flags, capacity, 0}, then `cap` 128-bit key slots: keys = (hi, lo), the rest poison."""
    hi, lo = keys
    assert len(hi) == len(lo) <= cap
    w = np.full(4 + 4 * cap, POISON, np.uint32)
    w[0] = len(hi) if count is None else count
    w[1], w[2], w[3] = flags, (cap if cap_word is None else cap_word), 0
    w[4:4 + 4 * len(hi)] = key_words(hi, lo)
    return w
