"""CPU tests that pin tests/exchange_ref.py (the exchange's rule in numpy) and prove that the cases of tests/exchange_cases.py are what they
claim to be: sorted runs of distinct keys, staircases with disjoint ranges, duplicates that really are adjacent in the merged order, and a
"skipped tile" duplicate whose predecessor really is the last key of a tile the ranking kernel never loads.  The host merge of the library
(lm_merge_matches, an independent implementation: radix sort + std::unique's rule) must give the same lists."""
import numpy as np
import pytest

import exchange_cases as xc
import exchange_ref as xr


def _random_records(rng, n):
    rec = np.zeros(n, xr.MATCH_DTYPE)
    rec["x"] = rng.integers(-32768, 32768, n); rec["y"] = rng.integers(-32768, 32768, n)
    sims = np.concatenate([xc.SIMS, np.float32([0.0, 100.0, 1e-40, 61.03125]), np.nextafter(np.float32([61.03125]), np.float32(100))])
    rec["similarity"] = sims[rng.integers(0, len(sims), n)]
    rec["class_index"] = rng.integers(0, 128, n)
    rec["template_id"] = rng.choice(np.array([0, 1, 2, 3, 1000, 2 ** 31 - 1]), n)
    return rec


def _keys_of(rec):
    return xr.make_key(rec["x"], rec["y"], rec["similarity"], rec["class_index"], rec["template_id"])


def test_codec_round_trips():
    rng = np.random.default_rng(1)
    rec = _random_records(rng, 5000)
    assert xr.decode(*_keys_of(rec)).tobytes() == rec.tobytes()
    hi, lo = xr.make_key(-32768, 32767, np.float32(100.0), 127, 2 ** 31 - 1)          # one key by hand, from the comment of xchg_make_key
    bits = 0x42C80000                                                                  # 100.0f
    assert int(hi[0]) == ((~(bits ^ 0x80000000) & 0xFFFFFFFF) << 32 | (2 ** 31 - 1)) and int(lo[0]) == (127 << 32 | 65535 << 16 | 0)
    assert xr.key_words(np.uint64([0x1122334455667788]), np.uint64([0x99AABBCCDDEEFF00])).tolist() == [0x55667788, 0x11223344, 0xDDEEFF00, 0x99AABBCC]
    with pytest.raises(AssertionError):
        xr.make_key(32768, 0, 1.0, 0, 0)


def test_key_order_is_the_canonical_order():
    """similarity descending, then template id, class, y, x."""
    rng = np.random.default_rng(2)
    rec = _random_records(rng, 20000)
    hi, lo = _keys_of(rec)
    by_key = np.lexsort((lo, hi))
    by_fields = np.lexsort((rec["x"], rec["y"], rec["class_index"], rec["template_id"], -rec["similarity"].astype(np.float64)))
    assert rec[by_key].tobytes() == rec[by_fields].tobytes()


def _loop_merge(runs):
    keys = sorted((int(h), int(l)) for hi, lo in runs for h, l in zip(hi.tolist(), lo.tolist()))
    out, dropped = [], []
    for i, (h, l) in enumerate(keys):
        dup = i > 0 and (keys[i - 1][0] >> 32, keys[i - 1][1]) == (h >> 32, l)
        dropped.append(dup)
        if not dup:
            out.append((h, l))
    hi = np.array([k[0] for k in out], np.uint64); lo = np.array([k[1] for k in out], np.uint64)
    return xr.decode(hi, lo), np.array(dropped, bool)


@pytest.mark.parametrize("name", ["c256_w3_interleaved", "dup_chains", "dup_skipped_c256_w3", "extremes", "c256_w300_all_empty", "dup_chain_w257"])
def test_merge_expected_equals_a_plain_loop(name):
    kept, merged, dropped = xc.expected(name)
    want, want_dropped = _loop_merge(xc.case(name).runs)
    assert kept.tobytes() == want.tobytes() and np.array_equal(dropped, want_dropped) and len(merged) == sum(xc.case(name).counts())


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    import os
    if not os.path.exists(mod.library_path()):
        g.build()
    mod.load_library()
    return mod


@pytest.mark.parametrize("name", xc.MERGE_NAMES)
def test_merge_expected_equals_the_librarys_host_merge(lm, name):
    assert lm.MATCH_DTYPE == xr.MATCH_DTYPE
    kept, merged, _ = xc.expected(name)
    rng = np.random.default_rng(3)
    assert lm.merge_matches(merged[rng.permutation(len(merged))]).tobytes() == kept.tobytes()


@pytest.mark.parametrize("name", xc.NAMES)
def test_cases_keep_the_kernels_contract(name):
    c = xc.case(name)
    assert c.world == len(c.runs) and c.cap in (256, 4096, 65536)
    for r, (hi, lo) in enumerate(c.runs):
        assert hi.dtype == lo.dtype == np.uint64 and len(hi) == len(lo) <= c.cap, (name, r)
        if len(hi) > 1:
            assert np.all((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))), (name, r, "run not strictly ascending")
    hi = np.concatenate([r[0] for r in c.runs]); lo = np.concatenate([r[1] for r in c.runs])
    hi, lo = xr.sort_keys(hi, lo)
    assert not np.any((hi[1:] == hi[:-1]) & (lo[1:] == lo[:-1])), (name, "keys not distinct")
    w = c.words()
    assert w.shape == (c.world, 4 + 4 * c.cap) and w.dtype == np.uint32
    for r, (rh, rl) in enumerate(c.runs):
        n = len(rh)
        assert w[r, 0] == c.count.get(r, n) and w[r, 1] == c.flags.get(r, 0) and w[r, 2] == c.cap_word.get(r, c.cap) and w[r, 3] == 0
        assert np.array_equal(w[r, 4:4 + 4 * n].view(np.uint64).reshape(-1, 2), np.stack([rh, rl], 1))
        assert np.all(w[r, 4 + 4 * n:] == xr.POISON) and xr.POISON != 0xFFFFFFFF
    if c.expect is None:
        assert not c.count and not c.flags and not c.cap_word


def test_the_cases_cover_what_the_issue_lists():
    worlds = {}
    counts = {256: set(), 4096: set(), 65536: set()}
    for n in xc.MERGE_NAMES:
        c = xc.case(n)
        worlds.setdefault(c.cap, set()).add(c.world)
        counts[c.cap].update(c.counts())
    assert worlds[256] >= {1, 2, 3, 257, 300} and worlds[4096] >= {2, 129} and worlds[65536] >= {3, 9}
    for cap, seen in counts.items():
        assert seen >= {c for c in (0, 1, 255, 256, 257, 2047, 2048, 2049, cap - 1, cap) if c <= cap}, (cap, sorted(seen))
    assert sum(xc.case("c256_w300_all_empty").counts()) == 0
    assert xc.case("c256_w300_only_last").counts()[:-1] == [0] * 299 and xc.case("c256_w300_only_last").counts()[-1] > 0
    assert sorted(xc.case("c256_w300_only_one").counts())[-2:] == [0, 256]
    assert [xc.case(n).expect for n in xc.FAIL_NAMES] == ["none", -4, -2, 5000, 5000, 5000, 5000]
    for at in (0, 247, 248, 299):
        c = xc.case("fail_run_overflow_r%d" % at)
        assert c.world == 300 and c.words()[at, :3].tolist() == [5000, xr.RUN_OVERFLOW, 256] and max(c.counts()) == 7 < c.cap
    x, y, sim, cls, tid = xr.split_key(*[np.concatenate(k) for k in zip(*xc.case("extremes").runs)])
    assert {int(x.min()), int(x.max()), int(y.min()), int(y.max())} == {-32768, 32767} and {int(tid.min()), int(tid.max())} == {0, 2 ** 31 - 1}
    assert {int(cls.min()), int(cls.max())} == {0, 127}
    bits = np.unique(sim.view(np.uint32))
    assert bits[0] == 0 and bits[1] == 1 and 0x42C80000 in bits and np.any(np.diff(bits.astype(np.int64)) == 1)


@pytest.mark.parametrize("name", [n for n in xc.MERGE_NAMES if n.startswith("dup_")])
def test_duplicate_cases_drop_what_they_were_built_to_drop(name):
    c = xc.case(name)
    kept, merged, dropped = xc.expected(name)
    assert c.min_drops > 0 and dropped.sum() >= c.min_drops and len(kept) == len(merged) - dropped.sum()


def test_near_duplicate_is_kept():
    kept, _, _ = xc.expected("dup_chains")
    near = kept[(kept["x"] == 40) & (kept["y"] == 41) & (kept["class_index"] == 9)]
    assert len(near) == 2 and np.diff(np.sort(near["similarity"].view(np.uint32)).astype(np.int64)).tolist() == [1]
    assert len(kept[kept["similarity"] == np.float32(91.125)]) == 1 and len(kept[kept["similarity"] == np.float32(91.25)]) == 1


def _less(ah, al, bh, bl):
    return ah < bh or (ah == bh and al < bl)


@pytest.mark.parametrize("name", [n for n in xc.MERGE_NAMES if n.startswith("dup_skipped")])
def test_skipped_tile_duplicates_have_their_predecessor_in_a_tile_below_the_chunk(name):
    """The chunk and tile bounds of rank_in_runs, recomputed: for the planted record (rank d, index i) the chunk is the 256 keys of rank d around i;
    its predecessor in the merged order is the last key of rank s — the last key of rank s's last tile — and that tile's last key lies below the
    chunk's first key: the branch that counts the tile without loading it, and takes its last key as the predecessor."""
    c = xc.case(name)
    tile_len = min(c.cap, xc.TILE)
    all_hi = np.concatenate([r[0] for r in c.runs]); all_lo = np.concatenate([r[1] for r in c.runs])
    all_hi, all_lo = xr.sort_keys(all_hi, all_lo)
    assert len(c.info["skipped"]) == c.min_drops >= 1
    for d, i, s, si in c.info["skipped"]:
        dh, dl = c.runs[d]
        sh, sl = c.runs[s]
        assert d != s and si == len(sh) - 1
        c0 = i // xc.CHUNK * xc.CHUNK
        t0 = si // tile_len * tile_len
        assert min(len(sh), t0 + tile_len) - 1 == si                                          # last key of its tile
        assert _less(int(sh[si]), int(sl[si]), int(dh[c0]), int(dl[c0]))                       # the whole tile is below the chunk
        at = np.flatnonzero((all_hi == dh[i]) & (all_lo == dl[i]))[0]
        assert at > 0 and all_hi[at - 1] == sh[si] and all_lo[at - 1] == sl[si]                # predecessor in the merged order
        assert (dh[i] >> np.uint64(32)) == (sh[si] >> np.uint64(32)) and dl[i] == sl[si] and dh[i] != sh[si]   # equal but for the template id


def test_same_run_duplicates_follow_their_original():
    c = xc.case("dup_same_run")
    hi, lo = c.runs[0]
    assert c.info["same_run"] == [101, 256, 2048]              # inside a chunk, first key of a chunk, first key of a tile
    for i in c.info["same_run"]:
        assert (hi[i] >> np.uint64(32)) == (hi[i - 1] >> np.uint64(32)) and lo[i] == lo[i - 1]
    _, merged, dropped = xc.expected("dup_same_run")
    all_hi, all_lo = xr.sort_keys(np.concatenate([r[0] for r in c.runs]), np.concatenate([r[1] for r in c.runs]))   # the order of `merged`
    for i in c.info["same_run"]:
        at = np.flatnonzero((all_hi == hi[i]) & (all_lo == lo[i]))[0]
        assert dropped[at] and all_hi[at - 1] == hi[i - 1] and all_lo[at - 1] == lo[i - 1]      # the predecessor is the key before it in its own run


@pytest.mark.parametrize("name", [n for n in xc.NAMES if xc.case(n).disjoint])
def test_staircases_have_disjoint_ranges(name):
    c = xc.case(name)
    order = [r for r in (range(c.world) if c.disjoint == "up" else range(c.world - 1, -1, -1)) if len(c.runs[r][0])]
    assert len(order) >= 2
    for a, b in zip(order[:-1], order[1:]):
        assert _less(int(c.runs[a][0][-1]), int(c.runs[a][1][-1]), int(c.runs[b][0][0]), int(c.runs[b][1][0])), (name, a, b)


@pytest.mark.parametrize("name", ["c4096_w2_tiles", "c65536_w3_tiles"])
def test_tile_staircases_put_whole_tiles_between_chunks(name):
    """Between two consecutive 256-key chunks of rank 0 lies at least one whole tile of another rank (first and last key inside the gap)."""
    c = xc.case(name)
    tile_len = min(c.cap, xc.TILE)
    h0, l0 = c.runs[0]
    gaps = 0
    for b in range(xc.CHUNK, len(h0), xc.CHUNK):
        below, above = (int(h0[b - 1]), int(l0[b - 1])), (int(h0[b]), int(l0[b]))
        found = False
        for r in range(1, c.world):
            hi, lo = c.runs[r]
            for t0 in range(0, len(hi), tile_len):
                t1 = min(len(hi), t0 + tile_len) - 1
                found |= _less(*below, int(hi[t0]), int(lo[t0])) and _less(int(hi[t1]), int(lo[t1]), *above)
        assert found, (name, b)
        gaps += 1
    assert gaps >= 2


def test_pack_key_buffers_are_distinct_and_arranged_as_named():
    for cap in (256, 4096):
        for arr in xc.PACK_ARRANGEMENTS:
            for n in xc.pack_sizes(cap):
                hi, lo = xc.pack_keys("pack_%d_%s_%d" % (cap, arr, n), n, arr)
                assert len(hi) == len(lo) == n
                sh, sl = xr.sort_keys(hi, lo)
                assert not np.any((sh[1:] == sh[:-1]) & (sl[1:] == sl[:-1]))
                if arr == "sorted":
                    assert np.array_equal(hi, sh) and np.array_equal(lo, sl)
                if arr == "reversed":
                    assert np.array_equal(hi[::-1], sh) and np.array_equal(lo[::-1], sl)
                if arr == "equal_hi":
                    assert len(np.unique(hi)) <= 1
                if arr in ("chunks_up", "chunks_down") and n > xc.CHUNK:
                    rank = np.lexsort((lo, hi)).argsort()                   # position of every buffer entry in the sorted order
                    lo_b = [rank[s:s + xc.CHUNK].min() for s in range(0, n, xc.CHUNK)]
                    hi_b = [rank[s:s + xc.CHUNK].max() for s in range(0, n, xc.CHUNK)]
                    for b in range(len(lo_b) - 1):
                        assert (hi_b[b] < lo_b[b + 1]) if arr == "chunks_up" else (lo_b[b] > hi_b[b + 1])
