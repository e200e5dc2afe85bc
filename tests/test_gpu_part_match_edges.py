"""GPU tests (`-m gpu`) of part-based matching at its edges (k_coarse_parts / k_local_parts, match_parts.hip) against part_match_ref.py, record
for record: every build of the two kernels (table low weight 1, 2, 3 x counters of 9 and 14 bits), the second pass of the coarse loop (maps
of more than 2048 positions), several classes in one request (the class is compared), thresholds that a part's score attains exactly, 100 and
beyond and 0, and the detectors part matching accepts besides the default one (one modality, grey frames, padded and cropped frames).

The inputs and the reference's answers are those of part_match_cases.py; test_part_match_cases.py proves on the CPU what each of them contains.
Everything is exact: the pre-unique records are the reference's multiset of (x, y, similarity, class_index, template_id), the canonical list
its sorted unique."""
import os

import pytest

import part_match_cases as pc
import response_table_ref as rt

pytestmark = pytest.mark.gpu
FIELDS = ["x", "y", "similarity", "class_index", "template_id"]


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def tuples(rec):
    return list(zip(*[rec[n].tolist() for n in FIELDS]))


def check(det, thr, classes, want, note):
    """the pre-unique records and the canonical list of the resident frame against reference records"""
    assert sorted(tuples(det.matchResident(thr, list(classes), sort_unique=False))) == pc.multiset5(want), note
    assert tuples(det.matchResident(thr, list(classes))) == pc.canonical(want), note


def g1_detector(lm, banks, table=None):
    sc = rt.scene("G1")
    det = lm.Detector(150, sc["T"], device=0)
    for name, bank in banks.items():
        det.addClassPacked(name, *bank)
    if table is not None:
        det.setResponseTable(table)
        assert det.getResponseTable() == tuple(table)
    det.setFrame([sc["rgb"], sc["dep"]])
    return det


# ---- 1. every kernel build ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank", pc.BUILD_BANKS)
@pytest.mark.parametrize("table", list(pc.TABLES))
def test_every_build_equals_the_reference(lm, table, bank):
    """low weight 2 (4 2 0 0 0), 3 (4 3 0 0 0) and 1 (the one-value tables) on counters of 9 bits (planted) and 14 bits (edge)"""
    det = g1_detector(lm, {"obj": pc.build_bank(bank)}, pc.TABLES[table])
    thr = pc.BUILD_THRESHOLDS[bank][table]
    for mp, mpf in pc.BUILD_RULES:
        det.setPartMatching(mp, mpf)
        check(det, thr, ["obj"], pc.build_reference(table, bank, mp, mpf), (mp, mpf))
    assert det.getResponseTable() == pc.TABLES[table] and det.getPaths() == ("bits", "bits")
    det.setPartMatching(0)
    check(det, thr, ["obj"], pc.build_reference(table, bank, 0, 8), "holistic")


# ---- 2. maps of more than 2048 top-level positions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.BIG))
def test_the_second_pass_of_the_coarse_loop(lm, name):
    s = pc.big_scene(name)
    det = lm.Detector(150, s["T"], device=0)
    det.addClassPacked("obj", *s["bank"])
    det.setFrame(list(s["frames"][0]))
    for mp, mpf, thr in pc.BIG_RULES:
        det.setPartMatching(mp, mpf)
        check(det, thr, ["obj"], pc.big_reference(name, 0, mp, mpf, thr)[0], (mp, mpf, thr))
    mp, mpf, thr = pc.BIG_STREAM_RULE                             # a batch of three different frames: each frame's second pass reads its own planes
    det.setPartMatching(mp, mpf)
    det.setBatch(3)
    streamed = list(det.matchStream([list(f) for f in s["frames"]], thr, ["obj"]))
    assert len(streamed) == 3
    for f, got in enumerate(streamed):
        assert tuples(got) == pc.canonical(pc.big_reference(name, f, mp, mpf, thr)[0]), f


# ---- 3. several classes in one request --------------------------------------------------------------------------------------------------------------
def test_several_classes_in_one_request(lm):
    banks = pc.class_banks()
    det = g1_detector(lm, {n: banks[n] for n in pc.CLASS_ORDER})
    mp, mpf, thr = pc.CLASS_RULE
    det.setPartMatching(mp, mpf)
    for req in pc.CLASS_REQUESTS:
        check(det, thr, req, pc.request_reference(req), req)
    check(det, thr, [], pc.request_reference(tuple(sorted(pc.CLASS_ORDER))), "all classes: the bank's order")


# ---- 4. ties, 100 and beyond, 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,min_parts", list(pc.TIES))
def test_thresholds_that_a_part_attains(lm, table, min_parts):
    """`>` at the top level, `>=` below: t, the float below it and the float above it"""
    det = g1_detector(lm, {"obj": pc.build_bank("planted")}, rt.NAMED[table])
    det.setPartMatching(min_parts, 8)
    for thr in pc.around(pc.TIES[(table, min_parts)]):
        check(det, thr, ["obj"], pc.tie_reference(table, min_parts, thr)[0], thr)


def test_thresholds_from_100_and_threshold_0(lm):
    det = g1_detector(lm, {"perfect": pc.perfect_bank(), "zero": pc.zero_bank()})
    for mp in (1, 2):
        det.setPartMatching(mp, 8)
        for thr in pc.HUNDRED:
            check(det, thr, ["perfect"], pc.perfect_reference(thr, mp)[0], (mp, thr))
    mp, mpf, thr = pc.ZERO_RULE
    det.setPartMatching(mp, mpf)
    check(det, thr, ["zero"], pc.zero_reference()[0], "threshold 0")


# ---- 5. detectors of other kinds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.KINDS)
def test_detectors_of_other_kinds(lm, kind):
    c = pc.kind_case(kind)
    det = lm.Detector(c["nf"], c["T"], device=0, **c["kwargs"])
    det.addClassPacked("obj", *c["packed"])
    if c["border"]:
        det.setBorder(c["border"])
    det.setFrame(c["sources"])
    thr = pc.KIND_THRESHOLD[kind]
    for mp, mpf in pc.KIND_RULES:
        det.setPartMatching(mp, mpf)
        check(det, thr, ["obj"], pc.kind_reference(kind, mp, mpf), (mp, mpf))
    det.setPartMatching(0)
    check(det, thr, ["obj"], pc.kind_reference(kind, 0, 8), "holistic")
