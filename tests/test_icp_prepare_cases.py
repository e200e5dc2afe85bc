"""The inputs of tests/test_gpu_icp_prepare_edges.py prove on the CPU that they sit on the edges they are named after
(icp_prepare_cases.check_edges: the oracle's voxel indices, neighbour distances and covariances against the kernels' constants), and the
oracle's own modes agree on them."""
import numpy as np
import pytest

import linemod_oracle as lo
import icp_prepare_cases as pc

NAMES = [n for n, _ in pc.FRAME] + ["mid_cloud"]
SMALL = ["near_many", "near_few", "wire", "many_far"] + ["tiny_%d" % n for n in pc.TINY]


@pytest.mark.parametrize("name", NAMES)
def test_case_sits_on_its_edge(name):
    fig = pc.check_edges(name, pc.all_cases()[name])
    print("\n%s: %s" % (name, fig))


def test_frame_holds_every_case_apart():
    cases = pc.frame_cases()
    assert list(cases) == [n for n, _ in pc.FRAME]
    scene = next(iter(cases.values())).scene
    for c in cases.values():
        assert c.scene is scene and np.array_equal(scene[c.md > 0], c.md[c.md > 0] + pc.SCENE_BACK)
        # the scene cloud of a case is its own pixels alone: as many scene points as model points
        o = c.oracle(True)
        assert len(o["scene_pts"]) == len(o["model_pts"]) == int((c.md > 0).sum()), c.name


@pytest.mark.parametrize("name", SMALL)
def test_oracle_modes_agree(name):
    """lo.estimate_normals by brute force and through the KD tree, and the neighbour lists the case keeps, on the small cases: the
    same lists in the same order, so the same normals bit for bit."""
    c = pc.all_cases()[name]
    for mode in (False, True):
        o = c.oracle(mode)
        brute = lo.estimate_normals(o["tgt"], nn="brute")
        assert np.array_equal(brute, lo.estimate_normals(o["tgt"], nn="kdtree")), (name, mode)
        assert np.array_equal(brute, o["normals"]), (name, mode)
        assert np.array_equal(lo.knn_lists(o["tgt"], nn="brute"), o["lists"]), (name, mode)


def test_normal_gap_threshold_is_what_the_oracle_supports():
    """NORMAL_GAP_MIN of the GPU test, measured: the oracle's normals (covariance E[xx^T] - E[x]E[x]^T in double) and the same from
    centred neighbours in np.longdouble agree to 1e-10 wherever the relative gap (l1 - l0) / l2 is at least the threshold; what lies
    below it has no gap at all (the 1-px line, three collinear points)."""
    NORMAL_GAP_MIN = pc.NORMAL_GAP_MIN
    below, n = [], 0
    for name, c in pc.all_cases().items():
        for mode in ((False,) if name == "mid_cloud" else (False, True)):
            o = c.oracle(mode)
            if o["k"] < 3:
                continue
            nrm, _, gap = pc.exact_normals(o["tgt"], o["lists"])
            dis = 1 - np.abs((nrm * o["normals"]).sum(1))
            ok = gap >= NORMAL_GAP_MIN
            assert (dis[ok] < 1e-10).all(), (name, mode, float(dis[ok].max()))
            n += int(ok.sum())
            below += gap[~ok].tolist()
    assert n > 50000 and below and max(below) < 1e-12, (n, len(below), max(below))
