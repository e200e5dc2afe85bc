"""CPU tests of part_match_cases.py: every condition on the inputs that test_gpu_part_match_edges.py relies on, proven on the reference
(part_match_ref.py) alone — no case there may pass on an empty list, on a list that another rule would give as well, or on a map, a bank or a
threshold that does not reach the code it is meant for."""
import numpy as np
import pytest

import part_match_cases as pc
import part_match_ref as pm
import response_table_ref as rt
import test_part_match_ref as cpu


# ---- the reference's new arguments change nothing -----------------------------------------------------------------------------------------------
def test_trace_and_class_column_leave_the_records_alone():
    bank, lms, sizes, T = cpu.tiny_case(5)
    for mp, mpf in ((0, 8), (1, 1), (2, 8)):
        plain = pm.match_parts(bank, lms, sizes, T, 20.0, mp, mpf)
        tr = []
        traced = pm.match_parts(bank, lms, sizes, T, 20.0, mp, mpf, cls=3, trace=tr)
        assert (plain["cls"] == 0).all() and (traced["cls"] == 3).all() and pm.multiset(plain) == pm.multiset(traced) and len(plain) > 0
        assert sum(t["left"] for t in tr if t["level"] == 0) == len(plain)
        for t in tr:
            assert t["entered"] == len(t["raw"]) == len(t["hit"]) and t["left"] == int(t["hit"].sum())
        for a, b in zip(tr, tr[1:]):
            if a["tid"] == b["tid"]:
                assert a["level"] == b["level"] + 1 and a["left"] == b["entered"]


# ---- 1. every kernel build ----------------------------------------------------------------------------------------------------------------------
def test_the_tables_of_the_builds():
    """low weights 2, 3 and (one non-zero value) 1; all accepted by part matching: at most two distinct non-zero values"""
    assert [sorted(set(v for v in t if v)) for t in pc.TABLES.values()] == [[2, 4], [3, 4], [4], [4]]
    assert all(t in rt.legal_tables() and rt.distinct_nonzero(t) <= 2 and t != rt.DEFAULT for t in pc.TABLES.values())
    assert pc.max_entry(pc.build_bank("planted"), 2) <= 511 < pc.max_entry(pc.build_bank("edge"), 2)
    assert all(cpu.windows_stay_inside(pc.build_bank("edge"), 192, 160, [4, 8], p) for p in range(5))


@pytest.mark.parametrize("bank", pc.BUILD_BANKS)
@pytest.mark.parametrize("table", list(pc.TABLES))
def test_conditions_on_the_build_inputs(table, bank):
    hol = pm.multiset(pc.build_reference(table, bank, 0, 8))
    for mpf in (1, 8):
        lists = [pm.multiset(pc.build_reference(table, bank, mp, mpf)) for mp in (1, 2, 3, 4)]
        print(table, bank, mpf, [len(l) for l in lists], len(hol))
        assert sum(len(l) > 0 for l in lists) >= 3
        for mp, l in zip((1, 2, 3, 4), lists):
            if l:
                assert l != hol and l != pm.multiset(pc.build_reference(table, bank, mp, mpf, "levelup")), (mp, mpf)


# ---- 2. maps of more than 2048 positions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.BIG))
def test_conditions_on_the_big_maps(name):
    s = pc.big_scene(name)
    L = len(s["T"])
    assert s["npos"] == 2560 and pc.pyramids(s["bank"], L) == 10
    assert all(cpu.windows_stay_inside(s["bank"], s["W"], s["H"], s["T"], p) for p in range(10))
    rules = [(0,) + r for r in pc.BIG_RULES] + [(f,) + pc.BIG_STREAM_RULE for f in (1, 2)]
    for frame, mp, mpf, thr in rules:
        rec, tr = pc.big_reference(name, frame, mp, mpf, thr)
        top = [t for t in tr if t["level"] == L - 1]
        hits = [np.nonzero(t["hit"])[0] for t in top]
        beyond = [t["entered"] > 2048 and (h >= 2048).any() for t, h in zip(top, hits)]        # limit > 2048 and candidates in the second pass
        short = [t["entered"] < 2048 for t in top]                                                # limit ends inside the first pass
        straddle = [(h < 2048).any() and (h >= 2048).any() for h in hits]
        print(name, frame, mp, mpf, thr, "records", len(rec), "second-pass candidates", sum(int((h >= 2048).sum()) for h in hits), sum(beyond), sum(short), sum(straddle))
        assert any(beyond) and any(short) and any(straddle) and len(rec) > 0
        assert (rec["y"] >= (128 << (L - 1))).any()                                            # ... and records that come from there
    lists = [pm.multiset(pc.big_reference(name, f, *pc.BIG_STREAM_RULE)[0]) for f in (0, 1, 2)]
    assert lists[0] != lists[1] != lists[2] != lists[0]                                        # three different frames


# ---- 3. several classes -----------------------------------------------------------------------------------------------------------------------------
def test_conditions_on_the_class_requests():
    banks = pc.class_banks()
    assert [pc.pyramids(banks[n], 2) for n in pc.CLASS_ORDER] == [7, 10, 5] and sorted(pc.CLASS_ORDER) != list(pc.CLASS_ORDER)
    assert pc.max_entry(banks["m"], 2) > 511 >= max(pc.max_entry(banks["z"], 2), pc.max_entry(banks["b"], 2))
    for n in pc.CLASS_ORDER:
        assert all(cpu.windows_stay_inside(banks[n], 192, 160, [4, 8], p) for p in range(pc.pyramids(banks[n], 2)))
    for req in pc.CLASS_REQUESTS:
        want = pc.request_reference(req)
        per_class = np.bincount(want["cls"], minlength=len(req))
        known = [i for i, n in enumerate(req) if n in pc.CLASS_ORDER]
        assert all(per_class[i] > 0 for i in known) and len(known) >= 2 and per_class.sum() == len(want)
        four = {}
        for x, y, s, c, t in pc.multiset5(want):
            four.setdefault((x, y, s, t), set()).add(c)
        assert any(len(v) >= 2 for v in four.values())                                          # only the class tells them apart
    last = pc._class_reference("m")
    assert (last["tid"] == 4).any() and (pc._class_reference("b")["tid"] >= 2).any()           # the 600-feature entry and random templates have records


# ---- 4. ties, 100 and beyond, 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,min_parts", list(pc.TIES))
def test_the_tie_thresholds_have_witnesses_at_both_levels(table, min_parts):
    below, t, above = pc.around(pc.TIES[(table, min_parts)])
    assert below < t < above and np.float32(t) == t
    (r0, tr0), (r1, tr1), (r2, tr2) = (pc.tie_reference(table, min_parts, v) for v in (below, t, above))
    top0, top1, top2 = (pc.level_counts(tr, 1)[0] for tr in (tr0, tr1, tr2))
    drop1, drop2 = pc.level_counts(tr1, 1)[1], pc.level_counts(tr2, 1)[1]
    # attained exactly: positions whose critical score is t are candidates below t and not at t ...
    at_top = sum(int((pc.critical(x["raw"], x["n"], min_parts, 8) == np.float32(t)).sum()) for x in tr1 if x["level"] == 1)
    # ... and candidates whose critical score at the refined position is t stay at t and are dropped above it
    at_low = sum(int((pc.critical(x["raw"], x["n"], min_parts, 8) == np.float32(t)).sum()) for x in tr1 if x["level"] == 0)
    print(table, min_parts, t, "witnesses: top level", at_top, "below the top", at_low)
    assert at_top > 0 and top0 - top1 == at_top                 # `>` excludes equality at the top
    assert top1 == top2                                         # (the same candidates enter at t and above it)
    assert at_low > 0 and drop2 - drop1 == at_low               # `>=` includes equality below
    assert len(r1) > len(r2) > 0 and pm.multiset(r0) != pm.multiset(r1)


def test_a_perfect_part_and_the_thresholds_from_100():
    just_below, hundred, more, inf = pc.HUNDRED
    assert just_below < 100.0 and pc.pyramids(pc.perfect_bank(), 2) >= 3
    for mp in (1, 2):
        rec, tr = pc.perfect_reference(just_below, mp)
        perfect = [x for x in tr if ((x["raw"] == 4 * x["n"][None, :]) & (x["n"] >= 8)[None, :]).any()]
        assert {x["level"] for x in perfect} == {0, 1}           # parts that score exactly 100 at the top and at refined positions
        assert len(rec) > 0 and (rec["sim"] == 100.0).any()
        for thr in (hundred, more, inf):
            assert len(pc.perfect_reference(thr, mp)[0]) == 0    # nothing is > 100 at the top
    # what a perfect part needs below the top: >= 100 holds, > 100 does not (the raw bounds the kernels form: 4 n resp. 4 n + 1)
    assert pm.score_of(4 * 24, 24) >= np.float32(100.0) and not pm.score_of(4 * 24, 24) > np.float32(100.0) and not pm.score_of(4 * 24, 24) >= np.float32(100.5)


def test_parts_without_responses_pass_at_threshold_zero():
    mp, mpf, thr = pc.ZERO_RULE
    rec, tr = pc.zero_reference()
    saved = 0
    for x in tr:
        if x["level"] == 0:
            eligible = (x["n"] >= mpf)[None, :]
            responding = ((x["raw"] > 0) & eligible).sum(1)
            silent = ((x["raw"] == 0) & eligible).any(1)
            assert x["hit"].all()                                # every eligible part passes >= 0 (all four are eligible)
            assert (x["n"] >= mpf).all()
            saved += int((silent & (responding < mp)).sum())     # kept although fewer than min_parts parts respond at all
    print("candidates kept by parts with a sum of 0:", saved, "of", len(rec))
    assert saved > 0 and len(rec) > 0


# ---- 5. detectors of other kinds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.KINDS)
def test_conditions_on_the_kinds(kind):
    c = pc.kind_case(kind)
    W, H = c["sizes"][0]
    n = pc.pyramids(c["bank"], 2)
    assert n >= 5 and all(cpu.windows_stay_inside(c["bank"], W, H, c["T"], p) for p in range(n))
    if kind in ("colour", "depth"):
        assert all(len(pm.entry_of(c["bank"], p, l, 2)[0]) > 0 and (pm.entry_of(c["bank"], p, l, 2)[0][:, 3] == 0).all() for p in range(n) for l in range(2))
        assert not c["lms"][0][1].any() and c["lms"][0][0].any()
    hol = pm.multiset(pc.kind_reference(kind, 0, 8))
    for mp, mpf in pc.KIND_RULES:
        got = pm.multiset(pc.kind_reference(kind, mp, mpf))
        print(kind, mp, mpf, len(got), len(hol))
        assert len(got) > 0 and got != hol and len(hol) > 0
