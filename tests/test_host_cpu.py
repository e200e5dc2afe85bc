"""CPU-only tests of the host side: the C-ABI library loads and exports every symbol the header
declares, the wrapper mirrors the pybind11 surface, merge/NMS host logic equals the oracle's, the
product refuses to run without a GPU, and the N>1 gather works over gloo (world_size 2)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import linemodLevelup_pybind as lm
    return lm.load_library()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "amd_linemod.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(lm_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "missing symbol " + n
    assert b"gfx950" in lib.lm_version()


def test_python_surface_mirrors_pybind11_module():
    import linemodLevelup_pybind as lm
    for cls, methods in {"Detector": ["addTemplate", "writeClasses", "readClasses", "match", "getTemplates"],
                         "poseRefine": ["process", "getResidual", "getR", "getT"]}.items():
        for m in methods:
            assert callable(getattr(getattr(lm, cls), m))
    m = lm.Match()
    for a in ("x", "y", "similarity", "class_id", "template_id"):
        assert hasattr(m, a)
        setattr(m, a, getattr(m, a))            # def_readwrite
    assert lm.poseRefine().getResidual() == -1  # poseRefine(): residual(-1), LL.h:10


def test_no_gpu_means_loud_failure(lib):
    import linemodLevelup_pybind as lm
    if lib.lm_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.Detector(63, [5, 8])
    pr = lm.poseRefine()
    z = np.zeros((32, 32), np.uint16)
    z[10:20, 10:20] = 900
    K = np.eye(3, dtype=np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pr.process(z, z, K, K, K, np.zeros(3, np.float32), 1, 1)


def test_wrapper_validates_dtypes():
    import linemodLevelup_pybind as lm
    with pytest.raises(RuntimeError):
        lm._as_depth(np.zeros((4, 4), np.float32))     # the reference would reinterpret the bytes
    with pytest.raises(RuntimeError):
        lm._as_rgb(np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError):
        lm._as_mask(np.zeros((3, 3), np.uint8), (4, 4))


def _rand_matches(rng, n, dtype):
    m = np.zeros(n, dtype)
    m["x"] = rng.integers(0, 6, n); m["y"] = rng.integers(0, 6, n)
    m[dtype.names[2]] = rng.choice(np.array([75.5, 80.25, 80.25, 91.0], np.float32), n)
    m[dtype.names[3]] = rng.integers(0, 2, n)
    m[dtype.names[4]] = rng.integers(0, 5, n)
    return m


def test_merge_matches_equals_oracle_canonical_order(lib):
    import linemodLevelup_pybind as lm
    import linemod_oracle as lo
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 300):
        a = _rand_matches(rng, n, lm.MATCH_DTYPE)
        got = lm.merge_matches(a)
        b = np.zeros(n, lo.MATCH_DTYPE)
        for f, g in zip(lo.MATCH_DTYPE.names, lm.MATCH_DTYPE.names):
            b[f] = a[g]
        want = lo.canonical_sort_unique(b)
        assert len(got) == len(want)
        for f, g in zip(lo.MATCH_DTYPE.names, lm.MATCH_DTYPE.names):
            assert np.array_equal(got[g], want[f])


def test_nms_equals_driver_numpy_nms(lib):
    import linemodLevelup_pybind as lm
    import linemod_oracle as lo
    rng = np.random.default_rng(1)
    for n in (1, 5, 200):
        x1 = rng.integers(0, 300, n).astype(np.float64); y1 = rng.integers(0, 300, n).astype(np.float64)
        dets = np.stack([x1, y1, x1 + rng.integers(20, 90, n), y1 + rng.integers(20, 90, n),
                         rng.permutation(n) + rng.uniform(0, 0.5, n)], 1)      # distinct scores
        assert lm.nms(dets, 0.5) == lo.nms_boxes(dets, 0.5)
    assert lm.nms(np.zeros((0, 5)), 0.5) == []


_GLOO_WORKER = r'''
import os, sys, numpy as np, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "6dpose_amd"))
import linemodLevelup_pybind as lm, sharded
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % sys.argv[2], rank=int(sys.argv[3]), world_size=2)
rank = dist.get_rank()
rng = np.random.default_rng(5)
allm = np.zeros(40, lm.MATCH_DTYPE)
allm["x"] = rng.integers(0, 4, 40); allm["y"] = rng.integers(0, 4, 40)
allm["similarity"] = rng.choice(np.array([76.0, 88.5], np.float32), 40)
allm["class_index"] = rng.integers(0, 2, 40)
allm["template_id"] = np.sort(rng.integers(0, 9, 40))
local = allm[:17] if rank == 0 else allm[17:]          # ragged shards (17 / 23)
got = lm.merge_matches(sharded.gather_records(local))
want = lm.merge_matches(allm)
assert got.tobytes() == want.tobytes(), (rank, len(got), len(want))
empty = sharded.gather_records(np.zeros(0, lm.MATCH_DTYPE))   # nobody has matches
assert len(empty) == 0
one = sharded.gather_records(allm[:3] if rank == 1 else np.zeros(0, lm.MATCH_DTYPE))   # one empty rank
assert one.tobytes() == allm[:3].tobytes()
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_gather_over_gloo_world_size_2(lib, tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_GLOO_WORKER)
    port = str(29500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, port, str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_view_sampler_reproduces_the_reference_golden():
    """6dpose_amd/views.py vs tests/golden/views_golden.npz (pysixd/view_sampler.py imported by make_views_golden.py)."""
    import math
    import views
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views_golden.npz"))
    vs, lv = views.sample_views(100, 1000, (0, 2 * math.pi), (0, 0.5 * math.pi), tilt_range=(0, 2 * math.pi), tilt_step=0.5 * math.pi)
    assert len(vs) == len(g["a_R"]) and lv == g["a_levels"].tolist()
    assert np.abs(np.stack([v["R"] for v in vs]) - g["a_R"]).max() < 1e-12 and np.abs(np.stack([v["t"] for v in vs]) - g["a_t"]).max() < 1e-9
    vs, _ = views.sample_views(100, 1000, (0, 2 * math.pi), (0, 0.5 * math.pi), tilt_range=(0, 2 * math.pi), tilt_step=0.1 * math.pi)   # the driver's call
    assert len(vs) == int(g["b_count"][0])
    assert abs(sum(v["R"].sum() for v in vs) - g["b_sum"][0]) < 1e-9 and abs(sum(v["t"].sum() for v in vs) - g["b_sum"][1]) < 1e-6
    for k, i in enumerate((0, 1, 777, len(vs) - 1)):
        assert np.abs(np.concatenate([vs[i]["R"].ravel(), vs[i]["t"].ravel()]) - g["b_first_last"][k]).max() < 1e-9
    # whole sphere, 642 points.  Inside a ring the reference orders by azimuth with a stable sort of a list built from a
    # Python set (view_sampler.py:141-150), so points of a ring with EQUAL azimuth (here the x == 0 ones of the last ring)
    # come out in CPython's set-iteration order — an interpreter detail, not an algorithm; views.py breaks such ties by
    # vertex number.  Everything else is position-for-position identical.
    pts, lv = views.hinter_sampling(300, radius=2.5)
    ref_pts, ref_lv = g["c_pts"], g["c_levels"]
    moved = np.abs(pts - ref_pts).max(1) > 1e-12
    az = lambda P: np.mod(np.arctan2(P[:, 1], P[:, 0]) + 2 * math.pi, 2 * math.pi)
    assert moved.sum() <= 4 and np.array_equal(az(pts[moved]), az(ref_pts[moved]))
    key = lambda P, L: sorted((round(float(x), 9), round(float(y), 9), round(float(z), 9), int(l)) for (x, y, z), l in zip(P, L))
    assert key(pts, lv) == key(ref_pts, ref_lv)
    assert np.array_equal(np.array(lv)[~moved], ref_lv[~moved])
    vs, _ = views.sample_views(42, 600.0, tilt_step=0.25 * math.pi)
    assert np.abs(np.stack([v["R"] for v in vs]) - g["d_R"]).max() < 1e-12 and np.abs(np.stack([v["t"] for v in vs]) - g["d_t"]).max() < 1e-9


def test_new_entry_points_fail_loudly_without_a_gpu():
    """lm_icp / lm_mesh / lm_pipeline: no CPU fallback — creation reports LM_ERR_NO_DEVICE (or rejects bad arguments first)."""
    import linemodLevelup_pybind as mod
    lib = mod.load_library()
    if lib.lm_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        mod.IcpContext(device=0)
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        mod.Mesh(V, np.array([[0, 1, 2]], np.int32))
    with pytest.raises(RuntimeError, match="out of range"):
        mod.Mesh(V, np.array([[0, 1, 3]], np.int32))            # face index checked before any device use
    with pytest.raises(RuntimeError):
        mod.Mesh("/nonexistent/model.ply")
    # host placement helper: without a device it reports nothing and leaves the caller's affinity alone
    before = os.sched_getaffinity(0)
    assert mod.bind_near_device(0) is None and os.sched_getaffinity(0) == before


def _bank_file_bytes(levels, classes):
    """The packed bank layout of csrc/bank_file.cpp written from numpy: classes = [(name, wh [P*E][2], counts [P*E], feats [n][3])]."""
    import struct
    body = bytearray(40)
    dirs = []
    for name, wh, counts, feats in classes:
        begins = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        recs = np.zeros(len(begins), dtype=[("w", "<i4"), ("h", "<i4"), ("b", "<u8")])
        recs["w"][:-1], recs["h"][:-1], recs["b"] = wh[:, 0], wh[:, 1], begins
        packed = ((feats[:, 0].astype(np.int64) & 0xFFFF) | ((feats[:, 1].astype(np.int64) & 0x1FFF) << 16) | (feats[:, 2].astype(np.int64) << 29)).astype("<u4")
        body += b"\0" * (-len(body) % 8); toff = len(body); body += recs.tobytes()
        body += b"\0" * (-len(body) % 8); foff = len(body); body += packed.tobytes()
        dirs.append((name.encode(), len(counts) // (2 * levels), toff, foff, len(feats)))
    body += b"\0" * (-len(body) % 8)
    dir_off = len(body)
    names_off = dir_off + 40 * len(dirs)
    for nm, P, toff, foff, nf in dirs:
        body += struct.pack("<QIIQQQ", names_off, len(nm), P, toff, foff, nf)
        names_off += len(nm)
    for nm, *_ in dirs:
        body += nm
    body[0:40] = b"LMBANK01" + struct.pack("<IIIIQQ", 1, levels, len(dirs), 0, dir_off, len(body))
    return bytes(body)


def test_packed_bank_file_header_and_rejections(lib, tmp_path):
    """lm_bank_file_info needs no GPU: a file laid out by hand is understood, damaged ones are refused."""
    import linemodLevelup_pybind as lm
    rng = np.random.default_rng(3)
    classes = []
    for name, P in (("obj_01", 3), ("a much longer class id / with spaces", 2)):
        counts = rng.integers(0, 40, P * 4)
        feats = np.stack([rng.integers(-5, 600, counts.sum()), rng.integers(-5, 400, counts.sum()), rng.integers(0, 8, counts.sum())], 1)
        classes.append((name, rng.integers(20, 200, (P * 4, 2)), counts, feats))
    blob = _bank_file_bytes(2, classes)
    good = tmp_path / "bank.lmb"
    good.write_bytes(blob)
    info = lm.bank_file_info(good)
    assert info == {"pyramid_levels": 2, "class_ids": [c[0] for c in classes], "num_pyramids": 5,
                    "num_features": int(sum(c[2].sum() for c in classes))}
    for bad in (blob[:-3], b"LMBANK02" + blob[8:], blob[:24] + (2 ** 40).to_bytes(8, "little") + blob[32:], b"short"):
        (tmp_path / "bad.lmb").write_bytes(bad)
        with pytest.raises(RuntimeError):
            lm.bank_file_info(tmp_path / "bad.lmb")
    with pytest.raises(RuntimeError, match="cannot open"):
        lm.bank_file_info(tmp_path / "missing.lmb")


def test_bench_gpus_flag_spawns_one_rank_per_gpu(monkeypatch):
    """`python bench.py --gpus N` started without a launcher re-executes itself under torch.distributed.run with N
    ranks on 127.0.0.1 (round-1 finding: the flag was parsed and never read).  CPU: only the command is checked; the
    GPU suite runs it for real (test_bench_launcher_runs_two_ranks)."""
    import argparse
    import importlib
    import subprocess
    import sys
    bench = importlib.import_module("bench")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2", "--scaling", "strong"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(bench.__file__ if bench.__file__ in cmd else os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "2", "--scaling", "strong"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_nms_norms_and_nmsboxes_equal_the_oracle(lib):
    """The other two NMS flavours of SURVEY A17: `nms_norms` (linemod_ros/detect.py:41-51, plain numpy = the reference itself)
    and cv::dnn::NMSBoxes as test.cpp:132-144 calls it (oracle = restatement of OpenCV 3.4's published algorithm)."""
    import linemodLevelup_pybind as mod
    import linemod_oracle as lo
    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 16, 200):
        ts = rng.uniform(-200, 200, (n, 3)).round(0)                 # rounded: exact ties of the distance occur
        sc = -rng.permutation(n).astype(np.float64) / 8.0            # distinct scores: the visiting order is defined
        tied = -rng.integers(0, 6, n).astype(np.float64) / 8.0       # equal scores: the order among them is numpy's unstable
        for thr in (0.0, 40.0, 150.0, 1e9):                          # argsort's business (SIMD sort on this host), see lm_nms_boxes
            assert mod.nms_norms(ts, sc, thr) == (lo.nms_norms(ts, sc, thr) if n else []), (n, thr)
            got, want = mod.nms_norms(ts, tied, thr), (lo.nms_norms(ts, tied, thr) if n else [])
            assert (thr not in (0.0, 1e9)) or sorted(tied[got].tolist()) == sorted(tied[want].tolist())
            assert len(set(got)) == len(got) and all(np.linalg.norm(ts[a] - ts[b]) > thr for a in got for b in got if a != b)
    for n in (0, 1, 9, 300):
        xy = rng.integers(0, 600, (n, 2))
        for wh in (np.full((n, 2), 40), rng.integers(0, 90, (n, 2))):
            rects = np.concatenate([xy, wh], 1).astype(np.int32)
            sc = (rng.integers(0, 40, n) / 40.0 * 100).astype(np.float32)
            for st, nt, eta, topk in ((0.0, 0.4, 1.0, 0), (50.0, 0.4, 1.0, 0), (0.0, 0.7, 0.9, 0), (0.0, 0.4, 1.0, 5)):
                assert mod.NMSBoxes(rects, sc, st, nt, eta, topk) == lo.nms_boxes_cv(rects, sc, st, nt, eta, topk), (n, st, nt, eta, topk)
    # test.cpp's use: 40x40 boxes at the match positions, threshold 0, overlap 0.4
    rects = np.array([[100, 100, 40, 40], [105, 100, 40, 40], [160, 100, 40, 40], [100, 130, 40, 40]], np.int32)
    assert mod.NMSBoxes(rects, np.array([90, 95, 80, 85], np.float32), 0.0, 0.4) == [1, 3, 2]   # by score: 95 kept, 90 overlaps it (IoU 0.78), 85 and 80 kept


def test_launch_model_decides_as_stated(tmp_path):
    """tests/cpp/launch_model_cases.cpp: the launch-timing model of the streamed path (csrc/launch_model.h) alone, under ASan + UBSan, with a
    table in place of the GPU: the estimate of a batch's time, the moving averages of the submit gap and the launch cost with their clamps,
    when a partial batch is due (never / sparse / tight, the one early batch per burst, and that the GPU is asked only where the answer is
    needed), the bookkeeping of a launch and of a collect's wait.  Host code, no GPU."""
    import shutil
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "launch_model_cases")
    cmd = [cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "6dpose_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "launch_model_cases.cpp"), "-o", exe]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:   # gcc: the runtimes inside the program
        subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_magic_division_with_one_correction_is_exact():
    """fe_device.h fast_div: q = umulhi(n, ceil(2^32 / d)) is floor(n / d) or one more for EVERY 32-bit n (the excess n e / (d 2^32) with
    e = m d - 2^32 < d stays below 1), so `q - (q d > n)` is exact — also where n d passes 2^32 (8000 x 6000 frames: ADVICE r03; the bare
    product was wrong there).  Checked here on the index ranges the front end divides (flat block index / blocks of a job, linear-memory
    index / row length) up to 16384 x 16384 frames and on random 31-bit values."""
    rng = np.random.default_rng(7)
    def check(n, d):
        n = np.asarray(n, np.uint64); d = np.uint64(d)
        m = (np.uint64(1) << np.uint64(32)) // d + (np.uint64(1) if (np.uint64(1) << np.uint64(32)) % d else np.uint64(0))
        q = (n * m) >> np.uint64(32)
        q = q - (q * d > n).astype(np.uint64)
        assert np.array_equal(q, n // d), (int(d),)
        bare = (n * m) >> np.uint64(32)
        return bool((bare != n // d).any())
    wrong_without_correction = False
    for W, H, T in ((640, 480, 4), (8000, 6000, 4), (12000, 9000, 4), (16384, 16384, 2), (16380, 16380, 4), (4096, 4096, 8)):
        Wd, Hd = W // T, H // T
        npos = Wd * Hd
        idx = np.concatenate([np.arange(0, min(npos, 70000)), np.arange(max(0, npos - 70000), npos + 256), rng.integers(0, npos + 256, 50000)])
        wrong_without_correction |= check(idx, Wd)
        gx, gy = (npos + 255) // 256, T * T
        blocks = gx * gy * 2
        b = np.concatenate([np.arange(max(0, blocks - 70000), blocks), rng.integers(0, blocks, 50000)])
        wrong_without_correction |= check(b, gx * gy)
        wrong_without_correction |= check(b % (gx * gy), gx)
    for d in (3, 5, 7, 160, 19200, 65535, 1 << 20):
        wrong_without_correction |= check(rng.integers(0, 1 << 31, 200000), d)
    assert wrong_without_correction, "the cases must include some the uncorrected product gets wrong"


def test_floor_of_a_quotient_without_the_division():
    """k_icp_voxel_wide (csrc/icp.hip, floor_quotient) takes floor(a / v) from a * (1 / v) wherever the fraction of that product is further than
    1e-6 from an integer and divides only otherwise: the two floors must agree on every value the shortcut accepts — voxel indices of points
    up to a few metres from the cloud's corner at the reference's 2.5 mm voxels and at sizes around it, including quotients that sit exactly
    on and next to integers."""
    rng = np.random.default_rng(11)
    for v in (0.0025, 0.002, 0.005, 0.0031, 1.0 / 3.0):
        inv = 1.0 / v
        a = np.concatenate([rng.uniform(0.0, 4.0, 400000), np.arange(0, 2000) * v, np.nextafter(np.arange(1, 2000) * v, 0.0), np.nextafter(np.arange(1, 2000) * v, 10.0),
                            rng.integers(0, 1600, 100000) * v + rng.uniform(-1e-12, 1e-12, 100000)])
        a = a[a >= 0]
        q = a * inv
        f = np.floor(q)
        d = q - f
        accepted = (d > 1e-6) & (d < 1.0 - 1e-6)
        assert accepted[:400000].mean() > 0.99                               # (the random points; the rest are the constructed boundary cases)
        assert np.array_equal(f[accepted], np.floor(a[accepted] / v))
