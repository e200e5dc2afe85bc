"""CPU proofs of the conditions on the inputs of scaled_edge_cases.py, on the reference (scaled_match_ref.py) alone: what each case is meant to
reach, it reaches.  test_gpu_scaled_edges.py then holds the kernels to the reference on the same inputs, so a failure there can only mean the
kernels.  No GPU is needed here."""
import numpy as np
import pytest

import scaled_cases as sc
import scaled_edge_cases as ec
import scaled_match_ref as sm

F32 = np.float32


def records(case, **over):
    return sm.canonical(ec.reference(case, **over))


# ---- a. several classes ---------------------------------------------------------------------------------------------------------------------------
def test_the_classes_differ_in_size_depth_and_feature_counts():
    banks, d = ec.class_banks()
    assert list(banks) == ["c", "a", "b"] and sorted(banks) == ["a", "b", "c"]                 # added in another order than the names'
    assert [len(ec.top_nf(banks[n], 2)) for n in "abc"] == [1, 5, 3] and len(ec.top_nf(d, 2)) == 2
    assert [ec.TRAIN[n] for n in "abc"] == [700, 1000, 1400]
    tops = {n: set(ec.top_nf(banks[n], 2)) for n in "abc"}
    assert len(tops["b"]) == 2 and len(tops["a"] | tops["b"] | tops["c"]) == 4                   # counts differ between the classes and inside b


def test_every_class_needs_its_own_training_depth():
    """every class returns records under its own training depth that it returns under neither of the other two: a swapped depth cannot pass"""
    c = ec.class_case("all")
    for name in "abc":
        alone = dict(c, classes={name: c["classes"][name]}, selection=(name,))
        own = set(sm.rows(records(alone)))
        for other in "abc":
            if other != name:
                own -= set(sm.rows(records(alone, d_train={name: ec.TRAIN[other]})))
        assert own, name


@pytest.mark.parametrize("selection", sorted(ec.SELECTIONS))
def test_the_selections_return_records_of_every_listed_class(selection):
    c = ec.class_case(selection)
    rec = records(c)
    names = c["selection"] or ("a", "b", "c")
    known = [i for i, n in enumerate(names) if n in c["classes"]]
    assert sorted(set(rec["class_index"].tolist())) == known
    if selection == "c_nope_a":
        assert known == [0, 2]                                                                    # the unknown name keeps its position
    if selection == "a_a":
        part = [rec[rec["class_index"] == i][["x", "y", "similarity", "template_id", "scale_index", "depth_mm"]].tolist() for i in (0, 1)]
        assert part[0] == part[1] and len(part[0]) > 0                                            # the class is matched twice
    for i in known:                                                                               # ... and every template of every class
        n_tmpl = len(ec.top_nf(c["classes"][names[i]], 2))
        assert set(rec["template_id"][rec["class_index"] == i].tolist()) == set(range(n_tmpl)), (selection, i)


# ---- b. big tables --------------------------------------------------------------------------------------------------------------------------------
def test_the_big_tables_have_the_stated_sizes_and_return_records():
    K = len(sc.LADDERS[16])
    assert K == 16
    mixed, limit, over = ec.big_case("mixed"), ec.big_case("limit"), ec.big_case("over")
    assert ec.top_nf(mixed["classes"]["big"], 2) == [40, 600] and K * 600 * 8 == 76800 > 65536
    assert ec.top_nf(limit["classes"]["big"], 2) == [1280] and K * 1280 * 8 == 163840
    assert ec.top_nf(over["classes"]["big"], 2) == [1281] and over["expect"] == "refused"
    for c in (mixed, limit):
        rec = records(c)
        assert set(rec["template_id"].tolist()) == set(range(len(ec.top_nf(c["classes"]["big"], 2)))), c["threshold"]
        assert len(set(rec["scale_index"].tolist())) > 1                                          # more than one row of the table is read


# ---- c. entries without features ----------------------------------------------------------------------------------------------------------------------
def test_what_the_rule_yields_for_entries_without_features():
    """No features at the top level: the score is 0 / 0 = nan, which passes no comparison: never a candidate, at any threshold.  No features at
    level 0: every window sums to 0, so the record gets similarity 0 and position cell -1; it is dropped when 0 < threshold and kept otherwise.
    The ordinary pyramid between the two is not touched by either."""
    c, cm = ec.zero_case(), ec.zero_case(-1.0)
    assert ec.top_nf(c["classes"]["z"], 2)[0] == 0 and len(sm.pm.entry_of(c["classes"]["z"], 2, 0, 2)[0]) == 0
    rec, recm = records(c), records(cm)
    assert set(rec["template_id"].tolist()) == {1}
    assert set(recm["template_id"].tolist()) == {1, 2} and (recm["similarity"][recm["template_id"] == 2] == 0).all()
    for case, got in ((c, rec), (cm, recm)):
        alone = records(dict(case, classes={"z": ec.pyramids(case["classes"]["z"], 2, [1])}))
        alone["template_id"] = 1
        assert sm.rows(got[got["template_id"] == 1]) == sm.rows(alone) and len(alone) > 0


# ---- d. edges of the level ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ladder", sorted(ec.EDGE_LADDERS))
def test_flush_boxes_are_sampled_beyond_the_right_and_bottom_edges(ladder):
    c = ec.flush_case(ladder)
    rec = records(c)
    out = np.array([ec.outside(c, r) for r in rec])
    assert (out[:, 0] > 0).any() and (out[:, 1] > 0).any(), out.sum(0)                            # a cell column >= Wd, a cell row >= Hd
    assert (out[:, 2] > 0).any() and (out[:, 3] > 0).any()                                        # ... and the left and the top as well
    if ladder == "both":
        assert set(rec["scale_index"].tolist()) == {0, 1}


def test_the_wide_box_has_an_empty_clamp_range_and_the_huge_one_no_position():
    c = ec.wide_case()
    _, w, _ = sm.pm.entry_of(c["classes"]["wide"], 0, 0, 2)
    assert ec.W - w - 32 < 32 and len(records(c)) > 0
    h = ec.huge_case()
    _, w1, h1 = sm.pm.entry_of(h["classes"]["huge"], 0, 1, 2)
    assert w1 > ec.W // 2 and h1 > ec.H // 2
    assert all(len(t[0]) == 0 for t in ec.top_level(h, "huge")) and len(records(h)) == 0


# ---- e. thresholds at and below zero ----------------------------------------------------------------------------------------------------------------------
def test_thresholds_at_and_below_zero_reach_rawmax_zero():
    """At -1.0 top-level cells of raw sum 0 become candidates (0 > -1) and go through rawmax == 0 at level 0: similarity 0.0, position cell -1 of
    the window, kept (0 < -1 is false).  At 0.0 no cell of sum 0 passes the top level (0 > 0 is false)."""
    for thr, want in ((-1.0, True), (0.0, False)):
        c = ec.masked_case(thr)
        hits = sum(int(((sm.pm.score_of(raw, nf) > F32(thr)) & (raw == 0)).sum()) for _, _, _, raw, nf in ec.top_level(c, "m"))
        rec = records(c)
        assert (hits > 0) == want and len(rec) > 0
        zero = rec[rec["similarity"] == 0]
        assert (len(zero) > 0) == want
        # position cell -1: x = (gx - 1) T + offset with gx = clamped x // T - 8 >= 0, so such a record may lie at cell -1 of the level itself
        assert ((zero["x"] - 1) % 4 == 0).all() and ((zero["y"] - 1) % 4 == 0).all()
    assert c["frame"]["dep"][:, :ec.W // 2].any()                                                 # the masked half keeps its depth


def test_a_threshold_equal_to_a_score_is_strict_on_top_and_not_below():
    base, t_top, t_low = ec.exact_thresholds()
    tops = np.concatenate([sm.pm.score_of(raw, nf) for _, _, _, raw, nf in ec.top_level(base, "b")])
    assert (tops == F32(t_top)).any()
    st = {}
    ec.reference(base, threshold=t_top, stats=st)
    assert st["candidates"] == int((tops > F32(t_top)).sum()) < int((tops >= F32(t_top)).sum())
    rec = records(base, threshold=t_low)
    assert (rec["similarity"] == F32(t_low)).any()


# ---- f. geometry, and the inputs of the one-detector sequence -------------------------------------------------------------------------------------------
def test_the_geometry_has_partial_probe_tiles_in_both_axes():
    c = ec.geometry_case()
    w, h = c["frame"]["size"]
    assert (w, h) == (328, 200) and w % 64 and h % 16 and w % 8 == 0 and h % 8 == 0 and len(records(c)) > 0


def test_the_sequence_changes_its_records_at_every_step():
    c = ec.class_case("all")
    d = ec.class_banks()[1]
    first = records(c)
    moved = records(c, d_train=dict(ec.TRAIN, b=1400))
    assert sm.rows(first) != sm.rows(moved)
    four = dict(c, classes=dict(c["classes"], d=d), d_train=dict(ec.TRAIN, b=1400))
    assert 3 in records(four)["class_index"]
    small = records(dict(four, frame=ec.small_frame()))
    assert len(small) > 0 and sm.rows(small) != sm.rows(records(four))
    st = {}
    ec.reference(four, threshold=ec.GROW_THRESHOLD, stats=st)
    assert st["candidates"] > 2 * ec.GROW_CAPACITY
    st = {}
    ec.reference(c, threshold=ec.GROW_THRESHOLD, stats=st)                                        # ... and with the three classes alone: one doubling
    assert st["candidates"] > ec.GROW_CAPACITY
