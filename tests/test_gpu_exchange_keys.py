"""The kernels of the multi-GPU exchange (csrc/exchange.hip) on CHOSEN keys (`-m gpu`).

The ranking merge k_exchange_merge — the shipped kernel, through the public calls — on the cases of tests/exchange_cases.py: blocks laid out the
way an all-gather leaves them, with the runs' relative position, the duplicates across runs and the failure headers chosen by the case, not by
the content of a frame.  A small detector only provides the frame in flight the calls want: exchangePack into a scratch block, then
exchangeMerge / exchangeMergeGroup / exchangeMergeFrame on the synthetic blocks, then exchangeCollect / exchangeCollectInto.  The result must
equal exchange_ref.merge_expected byte for byte, and lm.merge_matches of the decoded keys (a second, independent host implementation).
The device-side list with its `-1 - class` marks is not read back: the library has no call that exposes it; the marks are checked through what
the host drops while copying out.

The pack kernels k_exchange_sort256 / k_exchange_merge256 read the detector's own key buffer, so they are driven by tests/cpp/exchange_pack_keys.cpp:
that part tests the SOURCE csrc/exchange.hip compiled at the Makefile's device flags next to the driver, not the object inside the library.

All comparisons are exact."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import exchange_cases as xc
import exchange_ref as xr
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as g
    import linemodLevelup_pybind as mod
    if not os.path.exists(mod.library_path()):
        g.build()
    lib = mod.load_library()
    assert lib.lm_device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback)"
    return mod


class Rig:
    """One small detector with an empty class and a 64 x 64 frame: submit is cheap, and every frame in flight can be merged with any blocks."""

    def __init__(self, lm):
        import torch
        self.lm, self.torch = lm, torch
        self.lib = lm.load_library()
        self.det = lm.Detector(64, [4, 8], device=0)
        self.det.addClassPacked("e", np.zeros((0, 3), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
        rgb, dep = synth.make_frame(3, 64, 64, 4)
        self.det.setFrame([rgb, dep])
        self.scratch = {}
        self.calls = 0

    def scratch_block(self, cap, n=1):
        key = (cap, n)
        if key not in self.scratch:
            self.scratch[key] = self.torch.zeros(self.lib.lm_exchange_block_bytes(cap) * n, dtype=self.torch.uint8, device="cuda:0")
        return self.scratch[key]

    def device(self, words):
        t = self.torch.from_numpy(np.ascontiguousarray(words).view(np.uint8).reshape(-1)).to("cuda:0")
        self.torch.cuda.synchronize()                          # the exchange stream does not wait for torch's
        return t

    def collect(self, world, cap):
        self.calls += 1
        if self.calls % 2:
            return self.det.exchangeCollect()
        got, failed = self.det.exchangeCollectInto(np.empty(world * cap, self.lm.MATCH_DTYPE))
        return (None if got is None else got.copy()), failed

    def merge(self, c):
        """One frame: submit, pack, merge with the case's blocks, collect.  Returns (records or None, failed)."""
        self.det.submit(75.0, ["e"])
        self.det.exchangePack(self.scratch_block(c.cap).data_ptr(), c.cap)
        recv = self.device(c.words())
        self.det.exchangeMerge(recv.data_ptr(), c.world, c.cap)
        return self.collect(c.world, c.cap)


@pytest.fixture(scope="module")
def rig(lm):
    return Rig(lm)


def _explain(name, got):
    """Which rule broke: the order, a record that should have been dropped, or one that should not."""
    kept, merged, dropped = xc.expected(name)
    if len(got) == len(merged) and got.tobytes() == merged.tobytes():
        return "%s: nothing was dropped (%d duplicates expected)" % (name, dropped.sum())
    if len(got) != len(kept):
        return "%s: %d records, expected %d (%d of %d dropped)" % (name, len(got), len(kept), dropped.sum(), len(merged))
    bad = np.flatnonzero(got.view(np.int32).reshape(-1, 5) != kept.view(np.int32).reshape(-1, 5))
    i = int(bad[0]) // 5
    return "%s: first difference at record %d: got %s, expected %s" % (name, i, got[i], kept[i])


@pytest.mark.parametrize("name", xc.MERGE_NAMES)
def test_ranking_merge_on_chosen_keys(lm, rig, name):
    c = xc.case(name)
    kept, merged, _ = xc.expected(name)
    got, failed = rig.merge(c)
    assert failed == 0 and got is not None, (name, failed)
    assert got.tobytes() == kept.tobytes(), _explain(name, got)
    assert got.tobytes() == lm.merge_matches(merged[::-1]).tobytes(), name


def test_group_merge_gives_every_frame_its_own_case(lm, rig):
    """Three frames packed and merged by one launch each (exchangePackGroup / exchangeMergeGroup): the received blocks are rank-major, the three
    frames' blocks of a rank back to back; every frame must come out as ITS case."""
    names = ["c256_w3_interleaved", "dup_chains", "c256_w3_down"]
    cases = [xc.case(n) for n in names]
    assert all(c.cap == 256 and c.world == 3 for c in cases)
    det = rig.det
    first = det.framesSubmitted()
    for _ in names:
        det.submit(75.0, ["e"])
    det.flush()
    assert det.framesLaunched() == first + 3
    det.exchangePackGroup(first, 3, rig.scratch_block(256, 3).data_ptr(), 256)
    recv = rig.device(np.stack([c.words() for c in cases], 1))                 # [rank][frame][words]
    det.exchangeMergeGroup(first, 3, recv.data_ptr(), 3, 256)
    for n in names:
        got, failed = rig.collect(3, 256)
        assert failed == 0 and got.tobytes() == xc.expected(n)[0].tobytes(), _explain(n, got)


@pytest.mark.parametrize("name", ["dup_skipped_c256_w3", "c4096_w2_tiles"])
def test_merge_of_strided_blocks_ignores_the_padding(lm, rig, name):
    """exchangeMergeFrame with a rank stride larger than the block: what lies between two ranks' blocks is poison."""
    c = xc.case(name)
    det = rig.det
    det.submit(75.0, ["e"])
    frame = det.framesSubmitted() - 1
    det.flush()
    det.exchangePackFrame(frame, rig.scratch_block(c.cap).data_ptr(), c.cap)
    pad = 36                                                                     # words: the stride stays a multiple of 16 bytes
    w = np.full((c.world, c.words().shape[1] + pad), xr.POISON, np.uint32)
    w[:, :-pad] = c.words()
    recv = rig.device(w)
    det.exchangeMergeFrame(frame, recv.data_ptr(), c.world, c.cap, w.shape[1] * 4)
    got, failed = rig.collect(c.world, c.cap)
    assert failed == 0 and got.tobytes() == xc.expected(name)[0].tobytes(), _explain(name, got)


@pytest.mark.parametrize("name", xc.FAIL_NAMES)
def test_failure_blocks_are_reported_to_every_rank(lm, rig, name):
    """A block whose capacity word is wrong, the three flags, and a run overflow wherever its rank stands among 300: the size the blocks have to
    grow to is the overflowing rank's count (5000), also at ranks 248 and 299, whose counts the merged header does not list.  (Before the header
    carried the largest count of all ranks those two reported 7, the largest count among the first 248 ranks: no growth, ever.)"""
    c = xc.case(name)
    got, failed = rig.merge(c)
    print(name, "failed =", failed)
    assert got is None and failed != 0
    if c.expect != "none":
        assert failed == c.expect, (name, failed)
    if c.expect == 5000:
        assert failed > c.cap


@pytest.mark.parametrize("at", [0, 247, 248, 299])
def test_device_exchange_grows_after_an_overflow_on_any_rank(lm, at):
    """sharded.DeviceExchange.collect's own arithmetic on the value the library reports (no process group: one rank, the blocks of 300 handed to
    the merge directly): 256 -> 8192, the first power of two that holds 5000 records."""
    import sharded
    r = Rig(lm)
    ex = sharded.DeviceExchange(r.det, "cuda:0", capacity=256)
    assert ex.capacity == 256 and not ex.queue
    c = xc.case("fail_run_overflow_r%d" % at)
    r.det.submit(75.0, ["e"])
    r.det.exchangePack(r.scratch_block(c.cap).data_ptr(), c.cap)
    recv = r.device(c.words())
    r.det.exchangeMerge(recv.data_ptr(), c.world, c.cap)
    assert ex.collect() is None
    ex.grow_if_needed()
    assert ex.capacity == 8192, (at, ex.capacity)


# ---- the pack kernels ---------------------------------------------------------------------------------------------------------------------------
CAND_CAP = 1 << 20
FILL = 0x5EEDB10C


def _pack_launches():
    """[(cap, [(label, n, (hi, lo) buffer, counters, flagged)])]: one launch per entry, up to three frames each."""
    launches = []
    for cap in (256, 4096, 65536):
        frames = []
        for arr in xc.PACK_ARRANGEMENTS:
            for n in xc.pack_sizes(cap):
                label = "pack_%d_%s_%d" % (cap, arr, n)
                frames.append((label, n, xc.pack_keys(label, n, arr), [n + 5, n, 0, 0, 0, 0, 0, 0], 0))
        keys = xc.pack_keys("pack_flag_%d" % cap, 300 if cap > 256 else 200, "random")
        nk = len(keys[0])
        frames.append(("run_overflow_%d" % cap, cap + 1, keys, [cap + 9, cap + 1, 0, 0, 0, 0, 0, 0], xr.RUN_OVERFLOW))
        frames.append(("field_overflow_%d" % cap, nk, keys, [nk, nk, 0, 2, 0, 0, 0, 0], xr.FIELD_OVERFLOW))
        frames.append(("cand_overflow_%d" % cap, nk, keys, [CAND_CAP + 1, nk, 0, 0, 0, 0, 0, 0], xr.CAND_OVERFLOW))
        frames.append(("all_flags_%d" % cap, cap + 7, keys, [CAND_CAP + 1, cap + 7, 0, 1, 0, 0, 0, 0], xr.RUN_OVERFLOW | xr.CAND_OVERFLOW | xr.FIELD_OVERFLOW))
        # launches of 1, 2 and 3 frames; the frames of a launch differ in n (neighbours in the list do)
        i, size = 0, 1
        while i < len(frames):
            launches.append((cap, frames[i:i + size]))
            i += size
            size = size % 3 + 1
    return launches


@pytest.fixture(scope="module")
def packed_blocks(lm, tmp_path_factory):
    """Builds tests/cpp/exchange_pack_keys.cpp with csrc/exchange.hip once, runs it once on every case; returns [(cap, label, n, keys, flagged, block)]."""
    tmp = tmp_path_factory.mktemp("exchange_pack_keys")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, cases, blocks = str(tmp / "exchange_pack_keys"), str(tmp / "cases.bin"), str(tmp / "blocks.bin")
    csrc = os.path.join(ROOT, "6dpose_amd", "csrc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Werror", "-I", csrc, "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "exchange_pack_keys.cpp"), os.path.join(csrc, "exchange.hip"), "-o", exe], timeout=600)
    launches = _pack_launches()
    with open(cases, "wb") as f:
        f.write(struct.pack("<III", 0x314B5058, len(launches), FILL))
        for cap, frames in launches:
            f.write(struct.pack("<III", len(frames), cap, CAND_CAP))
            for _label, _n, (hi, lo), counters, _flag in frames:
                f.write(struct.pack("<I8Q", len(hi), *counters))
                f.write(xr.key_words(hi, lo).tobytes())
    r = subprocess.run([exe, cases, blocks], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"ok:" in r.stdout, r.stdout.decode()[-2000:]
    out, data, o = [], np.fromfile(blocks, np.uint32), 0
    for cap, frames in launches:
        for label, n, keys, _counters, flag in frames:
            out.append((cap, label, n, keys, flag, data[o:o + 4 + 4 * cap]))
            o += 4 + 4 * cap
    assert o == len(data)
    assert any(len(fr) == 3 and len({f[1] for f in fr}) == 3 for _c, fr in launches)      # a group launch of three frames of different n
    return out


def test_pack_kernels_sort_chosen_key_buffers(packed_blocks):
    """Header {n, 0, cap, 0} and keys[0:n] = the numpy sort of the buffer, for every n around the 256-key chunks and the 2048-key tiles, keys
    random, sorted, reversed, equal in `hi`, and in 256-key chunks of disjoint ranges; the words beyond n are not compared."""
    seen = 0
    for cap, label, n, (hi, lo), flag, blk in packed_blocks:
        if flag:
            continue
        assert blk[:4].tolist() == [n, 0, cap, 0], (label, blk[:4].tolist())
        sh, sl = xr.sort_keys(hi, lo)
        got = blk[4:4 + 4 * n]
        want = xr.key_words(sh, sl)
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0]) // 4
            raise AssertionError("%s: key %d of %d is %s, expected %s" % (label, bad, n, got[4 * bad:4 * bad + 4], want[4 * bad:4 * bad + 4]))
        seen += 1
    assert seen == sum(len(xc.pack_sizes(cap)) for cap in (256, 4096, 65536)) * len(xc.PACK_ARRANGEMENTS)


def test_pack_kernels_flag_what_they_cannot_send(packed_blocks):
    """More records than the block holds: the count and kXchgRunOverflow; a record that did not fit the key: kXchgFieldOverflow; a candidate
    buffer that overflowed: kXchgCandOverflow; and the key area stays as it was."""
    seen = 0
    for cap, label, n, _keys, flag, blk in packed_blocks:
        if not flag:
            continue
        assert blk[:4].tolist() == [n, flag, cap, 0], (label, blk[:4].tolist())
        assert np.all(blk[4:] == FILL), label
        seen += 1
    assert seen == 12
