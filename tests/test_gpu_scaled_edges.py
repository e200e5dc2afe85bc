"""GPU tests (`-m gpu`) of depth-scaled matching (Detector.matchScaled; k_depth_probe / k_coarse_scaled / k_local_scaled, match_scaled.hip; the
host side in detector_scaled.cpp) on the edge cases of scaled_edge_cases.py, against scaled_match_ref.py record for record: all seven fields
exact, the similarity bit for bit.  test_scaled_edge_cases.py proves on the CPU that the cases reach what they are meant to reach: the training
depth per work item, K-row tables above 64 KB and at the limit, mixed and zero feature counts, cells beyond all four edges of a level, rawmax
== 0 and both comparisons with the threshold, partial probe tiles through the Detector, and the cached tables across every change of the
bank, the selection and the frame size."""
import os

import numpy as np
import pytest

import scaled_cases as sc
import scaled_edge_cases as ec
import scaled_match_ref as sm
from test_gpu_scaled_match import device_memories, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    assert mod.load_library().lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


def detector(lm, case):
    det = lm.Detector(150, list(case["frame"]["T"]), device=0)
    for name, bank in case["classes"].items():                                          # in the order of the dict, not of the names
        det.addClassPacked(name, *bank)
        det.setClassTrainDepth(name, case["d_train"][name])
    return det


def run(det, case, **over):
    c = dict(case, **over)
    fr = c["frame"]
    lo_, hi_ = c["lo_hi"]
    return det.matchScaled([fr["rgb"], fr["dep"]], c["threshold"], list(c["selection"]), masks=fr["masks"], scales=c["scales"], min_scale=lo_, max_scale=hi_,
                           probe=c["probe"])


# ---- 1. parity on every case -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.PARITY_NAMES)
def test_records_equal_the_reference(lm, name):
    """(big_limit: a launch with 163,840 bytes of dynamic LDS, all a CU has.)"""
    case = ec.case(name)
    det = detector(lm, case)
    if case["expect"] == "refused":
        with pytest.raises(RuntimeError, match=r"16 scales x 1281 features x 8 bytes = 163968 bytes do not fit the 163840 bytes of LDS"):
            run(det, case)
        return
    got = run(det, case)
    same(got, ec.reference(case))
    assert (len(got) == 0) == (case["expect"] == "empty")


def test_the_ordinary_pyramid_is_not_touched_by_its_empty_neighbours(lm):
    for thr in (ec.CLASS_THRESHOLD, -1.0):
        case = ec.zero_case(thr)
        got = run(detector(lm, case), case)
        alone = dict(case, classes={"z": ec.pyramids(case["classes"]["z"], 2, [1])})
        one = run(detector(lm, alone), alone)
        one["template_id"] = 1
        mine = got[got["template_id"] == 1]
        assert len(one) > 0 and mine.tobytes() == one.tobytes()


# ---- 2. thresholds at and below zero, and equal to a score ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.0, -1.0])
def test_thresholds_at_and_below_zero_on_a_half_masked_frame(lm, threshold):
    """The reference runs on the detector's own byte memories (readStage kinds 2 and 3, which other suites hold to the oracle): the oracle's
    quantiser takes no mask per modality.  At -1.0 records of similarity 0.0 (rawmax == 0, position cell -1) must be there, at 0.0 none whose
    top-level sum was 0."""
    case = ec.masked_case(threshold)
    det = detector(lm, case)
    got = run(det, case)
    lms = device_memories(det, case["frame"]["T"])
    want = ec.reference(case, lms=lms, sizes=case["frame"]["sizes"])
    same(got, want)
    assert len(got) > 0
    on_device = dict(case, frame=dict(case["frame"], lms=lms))
    hits = sum(int(((sm.pm.score_of(raw, nf) > np.float32(threshold)) & (raw == 0)).sum()) for _, _, _, raw, nf in ec.top_level(on_device, "m"))
    assert (hits > 0) == (threshold < 0) and ((got["similarity"] == 0).any()) == (threshold < 0)


@pytest.mark.parametrize("which", ["top", "level0"])
def test_a_threshold_equal_to_a_score(lm, which):
    """`score > threshold` at the top level, `sim < threshold` drops below it: a cell whose score equals the threshold is no candidate, a record
    whose similarity equals it at level 0 stays"""
    base, t_top, t_low = ec.exact_thresholds()
    t = t_top if which == "top" else t_low
    det = detector(lm, base)
    got = run(det, base, threshold=t)
    same(got, ec.reference(base, threshold=t))
    assert len(got) > 0
    if which == "level0":
        assert (got["similarity"] == np.float32(t)).any()


# ---- 3. one detector through every change that the cached tables must follow ------------------------------------------------------------------------------
def test_one_detector_follows_every_change(lm):
    """the K-row tables are kept between calls; they bake in the selection, the bank and the geometry, the training depths travel beside them"""
    case = ec.class_case("all")
    det = detector(lm, case)
    same(run(det, case), ec.reference(case))                                             # 1. selection ()
    det.setClassTrainDepth("b", 1400)                                                    # 2. another depth, the same tables
    case = dict(case, d_train=dict(ec.TRAIN, b=1400))
    got = run(det, case)
    same(got, ec.reference(case))
    assert len(got) > 0
    case = dict(case, classes=dict(case["classes"], d=ec.class_banks()[1]))              # 3. a fourth class
    det.addClassPacked("d", *case["classes"]["d"])
    det.setClassTrainDepth("d", ec.TRAIN["d"])
    step3 = run(det, case)
    same(step3, ec.reference(case))
    assert 3 in step3["class_index"]
    got = run(det, case, selection=("c", "a"))                                           # 4. another selection
    same(got, ec.reference(case, selection=("c", "a")))
    assert len(got) > 0
    small = dict(case, frame=ec.small_frame())                                           # 5. another frame size, and back
    got = run(det, small)
    same(got, ec.reference(small))
    assert len(got) > 0
    assert run(det, case).tobytes() == step3.tobytes()
    with pytest.raises(RuntimeError, match="at least 1024"):                             # 6. (256 is below what the library accepts)
        det.setCandidateCapacity(256)
    det.setCandidateCapacity(ec.GROW_CAPACITY)
    st = {}
    want = ec.reference(case, threshold=ec.GROW_THRESHOLD, stats=st)
    assert st["candidates"] > 2 * ec.GROW_CAPACITY
    same(run(det, case, threshold=ec.GROW_THRESHOLD), want)
    assert run(det, case).tobytes() == step3.tobytes()


def test_grow_and_rerun_with_several_classes(lm):
    """a capacity set before the first match is the one the scaled matcher starts from: more candidates than that, nothing dropped"""
    case = ec.class_case("all")
    det = detector(lm, case)
    det.setCandidateCapacity(ec.GROW_CAPACITY)
    same(run(det, case, threshold=ec.GROW_THRESHOLD), ec.reference(case, threshold=ec.GROW_THRESHOLD))
    same(run(det, case), ec.reference(case))
