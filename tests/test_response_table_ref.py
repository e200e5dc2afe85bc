"""The numpy statement of the selectable response table (response_table_ref.py) pinned to the oracle for the default table, the set of legal
tables, and the condition on the shared inputs of the GPU tests: every non-default named table must change what the oracle finds."""
import ctypes

import numpy as np
import pytest

import linemod_oracle as lo
import response_table_ref as rt
import synth


def test_default_table_equals_the_oracle():
    rng = np.random.default_rng(0)
    spread = rng.integers(0, 256, (64, 96), dtype=np.uint8)
    assert np.array_equal(rt.response_np(spread, rt.DEFAULT), lo.response_np(spread))
    # all 8 x 256 entries of the oracle's look-up table (two 16-entry halves per orientation, combined with a maximum)
    lut = np.zeros(256, np.uint8)
    lo.clib().mo_similarity_lut(lut.ctypes.data_as(ctypes.c_void_p))
    v = np.arange(256, dtype=np.uint8)
    resp = rt.response_np(v, rt.DEFAULT)
    for ori in range(8):
        assert np.array_equal(np.maximum(lut[32 * ori:32 * ori + 16][v & 15], lut[32 * ori + 16:32 * ori + 32][v >> 4]), resp[ori]), ori


@pytest.mark.parametrize("T", [5, 8])
def test_default_linear_memories_equal_the_oracle_byte_for_byte(T):
    rgb, dep = synth.make_frame(9, 240, 160, 14)
    od = lo.OracleDetector(63, [T])
    qc, qn = od.quantize_pyramid(rgb, dep)[0][:2]
    assert qc.any() and qn.any()
    for q in (qc, qn):
        assert np.array_equal(rt.linear_memory(q, T, rt.DEFAULT), lo.build_linear_memories(q, T))


def test_closed_form_is_the_distance_to_the_nearest_bit():
    """every table, every spread byte: the response is r[distance to the nearest set bit]."""
    v = np.arange(256, dtype=np.uint8)
    dist = np.full((8, 256), 9)
    for ori in range(8):
        for b in range(8):
            d = min(abs(b - ori), 8 - abs(b - ori))
            dist[ori] = np.where((v >> b) & 1, np.minimum(dist[ori], d), dist[ori])
    for r in rt.legal_tables():
        want = np.where(dist < 9, np.asarray(r + (0,) * 5, np.uint8)[np.minimum(dist, 5)], 0)
        assert np.array_equal(rt.response_np(v, r), want), r


def test_legal_tables():
    tabs = rt.legal_tables()
    assert len(tabs) == 70 and len(set(tabs)) == 70
    assert all(t in tabs for t in rt.NAMED.values()) and (4, 1, 1, 0, 0) in tabs and (4, 4, 4, 4, 4) in tabs
    assert sorted(rt.distinct_nonzero(t) for t in rt.NAMED.values()) == [2, 2, 3, 3, 4]


@pytest.mark.parametrize("geom", sorted(rt.GEOMETRIES))
def test_named_tables_change_what_the_oracle_finds(geom):
    """A condition on the inputs of test_gpu_response_table.py: on its frames, banks and thresholds every table yields matches, and the
    pre-unique multiset of each non-default named table differs from the default table's (at the default's threshold for that bank too,
    so that the difference is the table's and not the threshold's)."""
    for kind in rt.BANKS:
        base_thr = rt.THRESHOLDS[kind]["levelup"]
        base, st = rt.oracle(geom, kind, rt.DEFAULT, base_thr)
        assert len(base) > 0 and st["coarse_candidates"] > len(base) // 2, (geom, kind)
        for name, r in rt.NAMED.items():
            if name == "levelup":
                continue
            raw, st = rt.oracle(geom, kind, r, rt.THRESHOLDS[kind][name])
            assert len(raw) > 0 and st["local_evals"] > 0, (geom, kind, name)
            assert rt.multiset(raw) != rt.multiset(base), (geom, kind, name)
            same_thr, _ = rt.oracle(geom, kind, r, base_thr)
            assert rt.multiset(same_thr) != rt.multiset(base), (geom, kind, name)
    sc = rt.scene(geom)
    assert all(n < 64 for n in np.diff(sc["banks"]["small"][1])), "the small bank takes the oracle's 8-bit path"
