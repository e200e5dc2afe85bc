"""The detector of the drop-in: Match, Template, Detector with its streaming and multi-GPU exchange calls, the RCCL communicator
Comm, the packed bank's file queries and the host NMS helpers (lm_detector_*, lm_comm_*, lm_bank_file_*, lm_nms_*)."""
from __future__ import annotations

import ctypes
import gzip
import os
import shutil
import tempfile
from typing import List, Optional, Sequence

import numpy as np

from lm_abi import (BORDER_POLICIES, DEPTH_MODE_DTYPE, MATCH_DTYPE, SCALED_MATCH_DTYPE, DepthModeOptions, ScaledOptions, Timings, _CMatch, _CScaledMatch, _CSlab, _as_depth, _as_grey, _as_mask,
                    _as_rgb, _border_code, _check, _ptr, _rgb_last_axis, aligned_size, load_library)

DEFAULT_SCALES = tuple(2.0 ** (i / 4.0 - 1.0) for i in range(9))     # 0.5 .. 2 in quarter octaves: the ladder of lm_scaled_options_init


class Match:
    """linemodLevelup::Match (LL.h:225-258, pybind11.cpp:16-22)."""
    __slots__ = ("x", "y", "similarity", "class_id", "template_id")

    def __init__(self, x: int = 0, y: int = 0, similarity: float = 0.0, class_id: str = "", template_id: int = 0):
        self.x, self.y, self.similarity, self.class_id, self.template_id = x, y, similarity, class_id, template_id

    def __repr__(self):
        return "Match(x=%d, y=%d, similarity=%r, class_id=%r, template_id=%d)" % (
            self.x, self.y, self.similarity, self.class_id, self.template_id)


class Template:
    """linemodLevelup::Template (LL.h:36-45); features is an (N,3) int32 array of x,y,label."""
    __slots__ = ("width", "height", "pyramid_level", "features")

    def __init__(self, width, height, pyramid_level, features):
        self.width, self.height, self.pyramid_level, self.features = width, height, pyramid_level, features


class Comm:
    """An RCCL communicator owned by the C library (lm_comm_*: librccl.so loaded with dlopen).  Rank 0 calls Comm.unique_id() and the
    caller carries the 128 bytes to every rank (sharded.DeviceExchange uses torch.distributed's broadcast; a C++ caller MPI or a file)."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int = 0):
        self._lib = load_library()
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        h = ctypes.c_void_p()
        _check(self._lib.lm_comm_create(ctypes.c_char_p(bytes(unique_id)), rank, world, device, ctypes.byref(h)))
        self._h = h
        self.rank, self.world = rank, world

    @staticmethod
    def available() -> bool:
        return bool(load_library().lm_comm_available())

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        _check(load_library().lm_comm_unique_id(buf))
        return bytes(buf.raw)

    def close(self):
        if self._h:
            self._lib.lm_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Detector:
    """linemodLevelup::Detector (LL.h:264-375) running on one MI355X."""

    def __init__(self, *args, device: Optional[int] = None, modalities: Optional[Sequence[str]] = None, colour_channels: int = 3):
        """Detector(), Detector(T), Detector(num_features, T) (pybind11.cpp:26-28).  modalities= selects the modality set, the
        counterpart of Detector(const std::vector<Ptr<Modality>>&, T) (LL.cpp:1694-1700): ("ColorGradient", "DepthNormal") — the
        default —, ("ColorGradient",) or ("DepthNormal",), with the parameters of the reference's constructors (LL.cpp:1684-1692).
        `sources` and `masks` then carry one array per modality of the set, in its order.  colour_channels=1 makes the colour source a grey
        image, uint8 HxW (a mono8 camera): the results are those of the same image replicated to three channels, at a third of the upload and
        of the colour chain's work (lm_detector_set_colour_channels)."""
        lib = load_library()
        num_features, T = 0, None
        if len(args) == 1:
            T = [int(t) for t in args[0]]                          # Detector(std::vector<int> T)
        elif len(args) == 2:
            num_features, T = int(args[0]), [int(t) for t in args[1]]   # Detector(int, std::vector<int>)
        elif len(args) != 0:
            raise TypeError("Detector(), Detector(T) or Detector(num_features, T)")
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) if lib.lm_device_count() > 1 else 0
        self._h = ctypes.c_void_p()
        Tarr = (ctypes.c_int * len(T))(*T) if T is not None else None
        if modalities is None:
            _check(lib.lm_detector_create(num_features, Tarr, len(T) if T is not None else 0, device, ctypes.byref(self._h)))
        else:
            if isinstance(modalities, (str, bytes)):
                raise RuntimeError("modalities must be a sequence of names, e.g. ('ColorGradient',)")
            names = [str(m).encode() for m in modalities]
            marr = (ctypes.c_char_p * max(1, len(names)))(*names)
            _check(lib.lm_detector_create_modalities(num_features, Tarr, len(T) if T is not None else 0, device, marr, len(names),
                                                     ctypes.byref(self._h)))
        out = (ctypes.c_char_p * 2)()
        self._mods = tuple(out[i].decode() for i in range(lib.lm_detector_get_modalities(self._h, out)))
        self._lib = lib
        self.device = device
        self._shard = (0, 1)
        self._cch = 3
        if colour_channels != 3:
            self.setColourChannels(colour_channels)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value and getattr(self, "_lib", None) is not None:
            self._lib.lm_detector_destroy(h)

    def getModalities(self) -> tuple:
        """The detector's modality set, names as in the class YAML (lm_detector_get_modalities)."""
        return self._mods

    def setColourChannels(self, channels: int) -> None:
        """lm_detector_set_colour_channels: 3 (uint8 HxWx3 colour sources) or 1 (uint8 HxW grey).  Refused with frames in flight and, for 1, on a
        detector without ColorGradient; drops the resident and the stored frames.  No file stores it."""
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)):
            raise RuntimeError("colour_channels must be 3 or 1, got %r" % (channels,))
        _check(self._lib.lm_detector_set_colour_channels(self._h, int(channels)))
        self._cch = int(channels)

    def getColourChannels(self) -> int:
        return int(self._lib.lm_detector_get_colour_channels(self._h))

    def setBorder(self, border: str) -> None:
        """lm_detector_set_border: what match, setFrame, storeFrame, submitFrame / matchStream and Pipeline do with a frame whose size is not
        aligned to the T grid (the reference's asserts at LL.cpp:1136 and 1217-1218).  "strict" (the default) refuses it; "pad" extends it at the
        right and bottom to alignedSize() — colour by edge replication, depth and masks with 0; "crop" cuts it there.  The results are bit for
        bit those of "strict" on the frame padded or cropped that way on the host; matches whose box reaches into the padded margin are kept.
        Sources, masks and ingestBuffers() keep the source size; readStage() returns arrays of the aligned size.  Refused with frames in flight."""
        _check(self._lib.lm_detector_set_border(self._h, _border_code(border)))

    def getBorder(self) -> str:
        code = _check(self._lib.lm_detector_get_border(self._h))
        return {v: k for k, v in BORDER_POLICIES.items()}[code]

    def alignedSize(self, width: int, height: int, border: Optional[str] = None):
        """lm_detector_aligned_size: (width, height) of the frame buffers a width x height source gets under `border` (None: the detector's
        own policy) — what the module's aligned_size(T, width, height, border) says in plain Python."""
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.lm_detector_aligned_size(self._h, -1 if border is None else _border_code(border), int(width), int(height),
                                                  ctypes.byref(w), ctypes.byref(h)))
        return int(w.value), int(h.value)

    def _colour(self, a):
        return _as_grey(a) if self._cch == 1 else _as_rgb(a)

    def _sources(self, sources, check_len: bool = False):
        """(rgb or None, depth or None, (H, W)): one array per modality of the set, in its order."""
        if check_len and len(sources) != len(self._mods):
            raise RuntimeError("sources.size() == modalities.size() [LL.cpp:1707]")
        if len(self._mods) == 2:
            rgb, depth = self._colour(sources[0]), _as_depth(sources[1])
            if rgb.shape[:2] != depth.shape:
                raise RuntimeError("rgb and depth sizes differ")
            return rgb, depth, depth.shape
        if len(sources) != 1:
            raise RuntimeError("sources.size() == modalities.size() [LL.cpp:1707]")
        if self._mods[0] == "ColorGradient":
            rgb = self._colour(sources[0])
            return rgb, None, rgb.shape[:2]
        depth = _as_depth(sources[0], "sources[0]")
        return None, depth, depth.shape

    # ---- training -------------------------------------------------------------------------------
    def addTemplate(self, sources: Sequence[np.ndarray], class_id: str, object_mask: np.ndarray) -> int:
        rgb, depth, shape = self._sources(sources, True)
        mask = _as_mask(object_mask, shape)
        rc = self._lib.lm_detector_add_template(self._h, _ptr(rgb), _ptr(depth), _ptr(mask), shape[1], shape[0],
                                                class_id.encode())
        if rc < -1:
            _check(rc)
        return rc

    def writeClasses(self, format: str) -> None:
        for cid in self.classIds():
            _check(self._lib.lm_detector_write_class(self._h, cid.encode(), (format % cid).encode()))

    def readClasses(self, class_ids: Sequence[str], format: str) -> None:
        for cid in class_ids:
            path = format % cid
            if path.endswith(".gz"):                        # FileStorage reads .gz transparently
                with tempfile.NamedTemporaryFile(suffix=".yaml", delete=False) as tmp, gzip.open(path, "rb") as src:
                    shutil.copyfileobj(src, tmp)
                try:
                    _check(self._lib.lm_detector_read_class(self._h, tmp.name.encode(), None))
                finally:
                    os.unlink(tmp.name)
            else:
                _check(self._lib.lm_detector_read_class(self._h, path.encode(), None))

    def addClassPacked(self, class_id: str, features: np.ndarray, tmpl_offsets: np.ndarray, tmpl_wh: np.ndarray) -> None:
        """Bulk import (lm_detector_add_class_packed): the binary bank path for >=16k templates."""
        features = np.ascontiguousarray(features, np.int32).reshape(-1, 3)
        tmpl_offsets = np.ascontiguousarray(tmpl_offsets, np.int32)
        tmpl_wh = np.ascontiguousarray(tmpl_wh, np.int32).reshape(-1, 2)
        E = len(self._mods) * self.pyramidLevels()
        if (len(tmpl_offsets) - 1) % E or len(tmpl_wh) != len(tmpl_offsets) - 1:
            raise RuntimeError("packed bank arrays have inconsistent sizes")
        _check(self._lib.lm_detector_add_class_packed(self._h, class_id.encode(), (len(tmpl_offsets) - 1) // E,
                                                      _ptr(features), _ptr(tmpl_offsets), _ptr(tmpl_wh)))

    # ---- queries --------------------------------------------------------------------------------
    def writeBank(self, path, class_ids: Sequence[str] = ()) -> None:
        """All classes (or the named ones) into ONE packed binary file (lm_detector_write_bank): 4 bytes per feature
        against ~45 text bytes in the YAML files of writeClasses (LL.cpp:2124-2146)."""
        arr, n, _ = self._class_args(class_ids)
        _check(self._lib.lm_detector_write_bank(self._h, os.fspath(path).encode(), arr, n))

    def readBank(self, path, class_ids: Sequence[str] = ()) -> None:
        """Adds the classes of a packed bank file (all, or the named ones), mmap'ed (lm_detector_read_bank)."""
        arr, n, _ = self._class_args(class_ids)
        _check(self._lib.lm_detector_read_bank(self._h, os.fspath(path).encode(), arr, n))

    def classIds(self) -> List[str]:
        return [self._lib.lm_detector_class_id(self._h, i).decode() for i in range(self._lib.lm_detector_num_classes(self._h))]

    def numClasses(self) -> int:
        return self._lib.lm_detector_num_classes(self._h)

    def numTemplates(self, class_id: Optional[str] = None) -> int:
        return self._lib.lm_detector_num_templates(self._h, None if class_id is None else class_id.encode())

    def pyramidLevels(self) -> int:
        return self._lib.lm_detector_pyramid_levels(self._h)

    def getT(self, level: int) -> int:
        return self._lib.lm_detector_get_T(self._h, level)

    def write(self, path: str) -> None:
        """Detector::write (LL.cpp:2029-2041, C++-only in the reference): pyramid levels, T and modality parameters as YAML."""
        _check(self._lib.lm_detector_write_params(self._h, os.fspath(path).encode()))

    def read(self, path: str) -> None:
        """Detector::read (LL.cpp:2013-2027): replaces the parameters and clears the classes."""
        _check(self._lib.lm_detector_read_params(self._h, os.fspath(path).encode()))

    def getTemplates(self, class_id: str, template_id: int) -> List[Template]:
        out = []
        for idx in range(len(self._mods) * self.pyramidLevels()):
            w, h, lvl, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
            _check(self._lib.lm_detector_get_template(self._h, class_id.encode(), template_id, idx, ctypes.byref(w), ctypes.byref(h),
                                                      ctypes.byref(lvl), ctypes.byref(n), None, 0))
            feats = np.zeros((n.value, 3), np.int32)
            _check(self._lib.lm_detector_get_template(self._h, class_id.encode(), template_id, idx, None, None, None, None,
                                                      _ptr(feats), n.value))
            out.append(Template(w.value, h.value, lvl.value, feats))
        return out

    # ---- matching -------------------------------------------------------------------------------
    def setReferenceOrder(self, on: bool = True) -> None:
        """match() / collect() return the list exactly as the reference's Detector::match does — the permutation libstdc++'s
        std::sort leaves and the duplicates std::unique then keeps (LL.cpp:1771-1776) — instead of the canonical order
        (lm_detector_set_reference_order).  Single GPU; costs a host-side sort of all pre-unique records."""
        _check(self._lib.lm_detector_set_reference_order(self._h, 1 if on else 0))

    def setShard(self, rank: int, world: int) -> None:
        """This process searches slice `rank` of `world` of the selected template pyramids."""
        _check(self._lib.lm_detector_set_shard(self._h, rank, world))
        self._shard = (rank, world)

    def _class_args(self, class_ids):
        ids = [c for c in (class_ids or [])]
        if not ids:
            return None, 0, self.classIds()
        key = tuple(ids)
        hit = self.__dict__.setdefault("_cls_cache", {}).get(key)      # a stream passes the same list every frame
        if hit is None:
            if len(self._cls_cache) > 64:
                self._cls_cache.clear()
            hit = self._cls_cache[key] = ((ctypes.c_char_p * len(ids))(*[c.encode() for c in ids]), len(ids), ids)
        return hit

    def _mask_args(self, masks, shape):
        if masks is None or len(masks) == 0:
            return None, []
        if len(masks) != len(self._mods):
            raise RuntimeError("masks.size() == modalities.size() [LL.cpp:1714]")
        keep = [_as_mask(m, shape) for m in masks]
        arr = (ctypes.c_void_p * 2)(*[None if m is None else m.ctypes.data for m in keep])       # (one entry used by a set of one)
        return arr, keep

    def setFrame(self, sources, masks=()) -> None:
        rgb, depth, shape = self._sources(sources)
        marr, keep = self._mask_args(masks, shape)
        _check(self._lib.lm_detector_set_frame(self._h, _ptr(rgb), _ptr(depth), shape[1], shape[0], marr))

    def storeFrame(self, slot: int, sources) -> None:
        """Parks a frame in HBM slot `slot` (lm_detector_store_frame)."""
        rgb, depth, shape = self._sources(sources)
        _check(self._lib.lm_detector_store_frame(self._h, slot, _ptr(rgb), _ptr(depth), shape[1], shape[0]))

    def selectFrame(self, slot: int) -> None:
        """Makes a parked frame current with a device-to-device copy (lm_detector_select_frame)."""
        _check(self._lib.lm_detector_select_frame(self._h, slot))

    def matchResident(self, threshold: float, class_ids: Sequence[str] = (), sort_unique: bool = True, distinct: bool = False) -> np.ndarray:
        """Front end + matching on the frame uploaded by setFrame(); returns MATCH_DTYPE records."""
        carr, n, _names = self._class_args(class_ids)
        out, cnt = ctypes.POINTER(_CMatch)(), ctypes.c_size_t()
        _check(self._lib.lm_detector_match_resident(self._h, float(threshold), carr, n, 1 if sort_unique else (2 if distinct else 0),
                                                    ctypes.byref(out), ctypes.byref(cnt)))
        return self._take(out, cnt.value)

    def submit(self, threshold: float, class_ids: Sequence[str] = ()) -> None:
        """Pipelined mode: enqueue front end + matching of the current frame and return (lm_detector_submit)."""
        carr, n, _names = self._class_args(class_ids)
        _check(self._lib.lm_detector_submit(self._h, float(threshold), carr, n))

    def submitFrame(self, sources, threshold: float, class_ids: Sequence[str] = ()) -> None:
        """Live-stream ingest (lm_detector_submit_frame): hands a NEW host frame to the detector and returns as soon as its
        upload (pinned ring, copy stream) is enqueued; front end and matching are launched for getBatch() consecutive frames at
        a time (or at flush() / the collect() that needs them); collect() returns the results in submission
        order.  Up to lm_detector_max_in_flight() frames in flight.  `sources` are borrowed only during the call; arrays
        obtained from ingestBuffers() skip the staging copy."""
        rgb, depth, shape = self._sources(sources)
        carr, n, _names = self._class_args(class_ids)
        _check(self._lib.lm_detector_submit_frame(self._h, _ptr(rgb), _ptr(depth), shape[1], shape[0], float(threshold), carr, n))

    def flush(self) -> None:
        """Launches the streamed frames that are still waiting for their batch to fill (lm_detector_flush); collect() does it by itself."""
        _check(self._lib.lm_detector_flush(self._h))

    def setBatch(self, frames: int) -> None:
        """Frames per kernel launch in stream mode, 1..8 (lm_detector_set_batch; default 8 or LM_FRAME_BATCH).  Results do not depend on it."""
        _check(self._lib.lm_detector_set_batch(self._h, int(frames)))

    def setBatchQueue(self, batches: int) -> None:
        """Streamed frames are launched at once while fewer than `batches` launched batches are unfinished on the GPU (default 2);
        0 = always wait for a full batch (deterministic batch sizes: tests, kernel measurements)."""
        _check(self._lib.lm_detector_set_batch_queue(self._h, int(batches)))

    def setAsyncCollect(self, on: bool) -> None:
        """Streamed frames: the result lists of a batch's later frames are prepared by the library's helper threads while the caller collects its first
        (lm_detector_set_async_collect; on by default, LM_ASYNC_COLLECT=0 turns it off; LM_HOST_THREADS=0: no helper threads at all)."""
        _check(self._lib.lm_detector_set_async_collect(self._h, 1 if on else 0))

    def hostProfile(self, reset: bool = True) -> dict:
        """Accumulated host wall time of the streamed path (lm_detector_host_profile), seconds."""
        out = (ctypes.c_double * 8)()
        _check(self._lib.lm_detector_host_profile(self._h, out, 1 if reset else 0))
        k = ("frames", "staging_copy", "h2d_enqueue", "slot_bookkeeping", "batch_launches", "collect_wait", "record_conversion", "sort_unique")
        return dict(zip(k, [float(x) for x in out]))

    def refinesOnBitPlanes(self) -> bool:
        """lm_detector_refines_on_bit_planes: which refinement kernel the current bank / geometry uses (valid after a match).  True on
        k_local_bits and, under "wide" with a table of three or four distinct non-zero values, on k_local_wide."""
        return bool(self._lib.lm_detector_refines_on_bit_planes(self._h))

    _REFINE = {"bits": 0, "tiles": 1, "single": 2, "wide": 3}
    _COARSE = {"bits": 0, "bytes": 1, "wide": 2}

    def setPaths(self, refine: str = "bits", coarse: str = "bits", direct: bool = True) -> None:
        """lm_detector_set_paths: which kernels serve the refinement ("bits" = k_local_bits, "tiles" / "single" = k_local with / without
        tiles) and the coarse pass ("bits" = k_coarse_bits, "bytes" = k_coarse); lm_detector_set_direct_bits: the front end writes the
        bit planes itself (direct) or byte linear memories that a second kernel packs.  "wide" (refine, and coarse together with it) is
        "bits" for a response table of at most two distinct non-zero values — the same kernels and memory, and getPaths() says "bits" —
        and two sets of bit planes (k_local_wide / k_coarse_wide, packed from the byte planes whatever `direct` says) for the other
        tables, which "bits" sends to the byte kernels.  Not on a sharded detector.  Results do not depend on any of it."""
        _check(self._lib.lm_detector_set_paths(self._h, self._REFINE[refine], self._COARSE[coarse]))
        _check(self._lib.lm_detector_set_direct_bits(self._h, int(direct)))          # True / False; tests: + 2 the top level's bit planes stay readable, + 4 / + 8 which writer of the top level (amd_linemod.h)

    CANDIDATE_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("score", np.float32), ("work", np.int32)])

    def setCoarseBatch(self, mode) -> None:
        """lm_detector_set_coarse_batch: the coarse pass on the pair stream by k_coarse_bits (False / 0: a wave serves one template on one
        frame), by k_coarse_bits_batch (True / 1: the frames of a batch launch share a template's waves) or by the launcher's rule (None / -1,
        the default unless LM_COARSE_BATCH says otherwise).  Results do not depend on it."""
        _check(self._lib.lm_detector_set_coarse_batch(self._h, -1 if mode is None else int(mode)))

    def coarseBatched(self) -> bool:
        """lm_detector_get_coarse_batch: whether the last coarse pass on the pair stream ran k_coarse_bits_batch."""
        return bool(self._lib.lm_detector_get_coarse_batch(self._h))

    def setCandidateCapacity(self, candidates: int) -> None:
        """lm_detector_set_candidate_capacity (tests of the overflow): coarse candidates per frame the buffers are first laid out for; before the first match."""
        _check(self._lib.lm_detector_set_candidate_capacity(self._h, int(candidates)))

    def readCandidates(self, frame_no: int):
        """lm_detector_read_candidates: (produced, records) of collected frame `frame_no` — the frame's candidate counter and the coarse
        candidates in slot order (CANDIDATE_DTYPE; `work` = index into the work list), min(produced, capacity) of them."""
        n = int(self._lib.lm_detector_read_candidates(self._h, int(frame_no), None, 0))
        if n < 0:
            raise RuntimeError(self._lib.lm_last_error().decode("utf-8", "replace"))
        out = np.zeros(n, self.CANDIDATE_DTYPE)
        out["work"] = -1                                      # (a frame that overflowed its buffers: only the first `capacity` records exist)
        got = int(self._lib.lm_detector_read_candidates(self._h, int(frame_no), out.ctypes.data_as(ctypes.c_void_p), n)) if n else 0
        if got < 0:
            raise RuntimeError(self._lib.lm_last_error().decode("utf-8", "replace"))
        return n, out[out["work"] >= 0]

    def getPaths(self):
        """lm_detector_get_paths: (refine, coarse) the current bank and frame geometry actually use, as the names of setPaths (valid after a match)."""
        r, c = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.lm_detector_get_paths(self._h, ctypes.byref(r), ctypes.byref(c)))
        return ({v: k for k, v in self._REFINE.items()}[r.value], {v: k for k, v in self._COARSE.items()}[c.value])

    # the reference's five SIMILARITY_LUTs (linemodLevelup.cpp:1112-1124) as r[d], d = cyclic distance 0..4 between a feature's label
    # and the nearest orientation of the spread image
    RESPONSE_TABLES = {
        "linemod": (4, 3, 2, 1, 0),        # :1112, the original LINE-MOD / cv::linemod table
        "drop1": (4, 2, 1, 0, 0),          # :1115
        "drop1_keep3": (4, 3, 1, 0, 0),    # :1118
        "levelup": (4, 1, 0, 0, 0),        # :1121, the reference's live one and the default here
        "levelup2": (4, 2, 0, 0, 0),       # :1124
    }

    def setResponseTable(self, table) -> None:
        """lm_detector_set_response_table: `table` is one of the names of RESPONSE_TABLES or five ints r[0..4] with r[0] == 4, non-increasing.
        State of this detector in this process only: no file format stores it and training does not read it; ranks of a sharded run must
        set the same table.  The next match (matchResident included) builds its response memories under it.  Refused with frames in
        flight.  A threshold has to be chosen again per table."""
        if isinstance(table, str):
            if table not in self.RESPONSE_TABLES:
                raise RuntimeError("unknown response table %r: one of %s or five ints" % (table, ", ".join(sorted(self.RESPONSE_TABLES))))
            table = self.RESPONSE_TABLES[table]
        r = list(table)
        if len(r) != 5 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > 4 for v in r):
            raise RuntimeError("a response table is five values r[0..4], integers in 0..4, got %r" % (tuple(r),))
        r = [int(v) for v in r]
        _check(self._lib.lm_detector_set_response_table(self._h, (ctypes.c_uint8 * 5)(*r)))

    def getResponseTable(self):
        """lm_detector_get_response_table: the table in use, a tuple r[0..4]."""
        out = (ctypes.c_uint8 * 5)()
        _check(self._lib.lm_detector_get_response_table(self._h, out))
        return tuple(int(v) for v in out)

    def setPartMatching(self, min_parts: int = 0, min_part_features: int = 8) -> None:
        """lm_detector_set_part_matching: accept a template when at least `min_parts` of its 4 quadrants (a feature at (x, y) belongs to part
        (2x >= width) + 2 (2y >= height)) pass the threshold on their own; quadrants of fewer than `min_part_features` features never pass.
        0 switches it off (the default), 2 tolerates half the object hidden, 4 is stricter than the holistic rule.  The similarity of a
        record stays the holistic score, so it may lie below the threshold.  Runs on the ("bits", "bits") paths with a response table of at
        most two distinct non-zero values and a threshold >= 0; anything else, a sharded detector, the exchange, matchSlabs and a Pipeline
        are refused, never matched holistically in silence.  Refused with frames in flight."""
        _check(self._lib.lm_detector_set_part_matching(self._h, int(min_parts), int(min_part_features)))

    def partMatching(self):
        """lm_detector_get_part_matching: (min_parts, min_part_features); min_parts 0 = off."""
        a, b = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.lm_detector_get_part_matching(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def trainStats(self):
        """lm_detector_train_stats: training views since creation or read() as (selected on the device, sent to the host selection,
        failed with -1, empty).  The two selections give the same templates; this is how a test sees which one ran."""
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.lm_detector_train_stats(self._h, out))
        return tuple(int(v) for v in out)

    def bitArenaBytes(self):
        """lm_detector_bit_arena_bytes: device bytes allocated for (strip records, pair stream), over all result slots (tests)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._lib.lm_detector_bit_arena_bytes(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def wideArenaBytes(self):
        """lm_detector_wide_arena_bytes: device bytes allocated for the second set of (strip records, pair stream) of the "wide" paths,
        over all result slots: (0, 0) until a table of three or four distinct non-zero values has run on them."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._lib.lm_detector_wide_arena_bytes(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def getBatch(self) -> int:
        return int(self._lib.lm_detector_get_batch(self._h))

    def ingestBuffers(self, width: int, height: int):
        """(rgb uint8 HxWx3 — HxW on a detector with colour_channels=1 —, depth uint16 HxW) views of the pinned staging memory the NEXT submitFrame() will upload from
        (lm_detector_ingest_buffer): fill them in place and pass them to submitFrame — no staging copy.  Valid until that
        frame has been collected.  A detector with one modality returns a 1-tuple: the buffer of that modality."""
        pr, pd = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self._lib.lm_detector_ingest_buffer(self._h, int(width), int(height), ctypes.byref(pr), ctypes.byref(pd)))
        n = int(width) * int(height)
        rgb = depth = None
        if pr.value:
            rgb = np.ctypeslib.as_array(ctypes.cast(pr, ctypes.POINTER(ctypes.c_uint8)), shape=(n * self._cch,))
            rgb = rgb.reshape(height, width) if self._cch == 1 else rgb.reshape(height, width, 3)
        if pd.value:
            depth = np.ctypeslib.as_array(ctypes.cast(pd, ctypes.POINTER(ctypes.c_uint16)), shape=(n,)).reshape(height, width)
        return tuple(b for b in (rgb, depth) if b is not None)

    def matchStream(self, frames, threshold: float, class_ids: Sequence[str] = (), depth: int = 3):
        """The dataset / camera loop of the reference (linemod_and_levelup_test.py:314-327: one Detector.match per frame) as a
        generator: yields Detector.match's result (MATCH_DTYPE records, canonical order) for every (rgb, depth) of `frames`,
        in order, keeping up to `depth` frames in flight so that upload, front end, matching and the host-side merge of
        neighbouring frames overlap.  A frame whose candidate buffer overflowed is redone synchronously."""
        depth = max(1, min(int(depth), self._lib.lm_detector_max_in_flight()))
        pending = []

        def collect_or_none():
            try:
                return self.collect()
            except RuntimeError as e:
                if "overflow" not in str(e):
                    raise
                return None                  # capacity has been raised by the library; the frame is redone below

        def drain():
            """Everything in flight, in order; overflowed frames are redone one at a time once nothing is in flight."""
            outs = [collect_or_none() for _ in pending]
            res = [o if o is not None else self.matchArray(list(src), threshold, class_ids) for src, o in zip(pending, outs)]
            del pending[:]
            return res

        for src in frames:
            self.submitFrame(src, threshold, class_ids)
            pending.append(src)
            if len(pending) == depth:
                out = collect_or_none()
                if out is not None:
                    pending.pop(0)
                    yield out
                else:
                    first = pending.pop(0)
                    rest = drain()
                    yield self.matchArray(list(first), threshold, class_ids)
                    for r in rest:
                        yield r
        for r in drain():
            yield r

    def collect(self, sort_unique: bool = True, distinct: bool = False) -> np.ndarray:
        """Pipelined mode: matches of the oldest submitted frame (lm_detector_collect)."""
        out, cnt = ctypes.POINTER(_CMatch)(), ctypes.c_size_t()
        _check(self._lib.lm_detector_collect(self._h, 1 if sort_unique else (2 if distinct else 0), ctypes.byref(out), ctypes.byref(cnt)))
        return self._take(out, cnt.value)

    # ---- multi-GPU exchange on the device (sharded.DeviceExchange drives these) ------------------
    def exchangeStream(self) -> int:
        """hipStream_t (as an integer) the exchange kernels run on; collectives go on the same stream."""
        h = self._lib.lm_detector_exchange_stream(self._h)
        if not h:
            raise RuntimeError(self._lib.lm_last_error().decode("utf-8", "replace"))
        return int(h)

    def framesSubmitted(self) -> int:
        """Frames submitted so far = the number the next submitted frame gets (lm_detector_frames_submitted)."""
        return int(self._lib.lm_detector_frames_submitted(self._h))

    def framesLaunched(self) -> int:
        """Frames whose kernels have been launched (streamed frames wait for their batch; lm_detector_frames_launched)."""
        return int(self._lib.lm_detector_frames_launched(self._h))

    def framesCollected(self) -> int:
        return int(self._lib.lm_detector_frames_collected(self._h))

    def exchangePackFrame(self, frame_no: int, send_ptr: int, capacity: int) -> None:
        _check(self._lib.lm_detector_exchange_pack_frame(self._h, frame_no, ctypes.c_void_p(send_ptr), capacity))

    def exchangeMergeFrame(self, frame_no: int, recv_ptr: int, world: int, capacity: int, rank_stride_bytes: int = 0) -> None:
        _check(self._lib.lm_detector_exchange_merge_frame_strided(self._h, frame_no, ctypes.c_void_p(recv_ptr), world, capacity, rank_stride_bytes))

    def exchangeGroup(self, comm: "Comm", first: int, n: int, send_ptr: int, recv_ptr: int, capacity: int) -> None:
        """pack + RCCL all-gather + merge of frames first .. first + n - 1, all issued by the library (lm_detector_exchange_group)."""
        _check(self._lib.lm_detector_exchange_group(self._h, comm._h, first, n, ctypes.c_void_p(send_ptr), ctypes.c_void_p(recv_ptr), capacity))

    def exchangePackGroup(self, first: int, n: int, send_ptr: int, capacity: int) -> None:
        _check(self._lib.lm_detector_exchange_pack_group(self._h, first, n, ctypes.c_void_p(send_ptr), capacity))

    def exchangeMergeGroup(self, first: int, n: int, recv_ptr: int, world: int, capacity: int) -> None:
        _check(self._lib.lm_detector_exchange_merge_group(self._h, first, n, ctypes.c_void_p(recv_ptr), world, capacity))

    def exchangePack(self, send_ptr: int, capacity: int) -> None:
        _check(self._lib.lm_detector_exchange_pack(self._h, ctypes.c_void_p(send_ptr), capacity))

    def exchangeMerge(self, recv_ptr: int, world: int, capacity: int) -> None:
        _check(self._lib.lm_detector_exchange_merge(self._h, ctypes.c_void_p(recv_ptr), world, capacity))

    def exchangeCollect(self):
        """(records, 0) — the frame's Detector.match result, identical on every rank — or (None, failed != 0)."""
        out = ctypes.POINTER(_CMatch)()
        n = ctypes.c_size_t(0)
        failed = ctypes.c_int(0)
        _check(self._lib.lm_detector_exchange_collect(self._h, ctypes.byref(out), ctypes.byref(n), ctypes.byref(failed)))
        if failed.value:
            return None, failed.value
        return self._take(out, n.value), 0

    def exchangeCollectInto(self, dst: np.ndarray):
        """Like exchangeCollect, written straight into `dst` (MATCH_DTYPE, >= world * capacity records): returns
        (dst[:n] — a view —, 0) or (None, failed)."""
        if dst.dtype != MATCH_DTYPE or not dst.flags.c_contiguous:
            raise TypeError("dst must be a C-contiguous MATCH_DTYPE array")
        n = ctypes.c_size_t(0)
        failed = ctypes.c_int(0)
        _check(self._lib.lm_detector_exchange_collect_into(self._h, dst.ctypes.data_as(ctypes.c_void_p), dst.size, ctypes.byref(n), ctypes.byref(failed)))
        if failed.value:
            return None, failed.value
        return dst[:n.value], 0

    def _take(self, out, n) -> np.ndarray:
        try:
            if n == 0:
                return np.zeros(0, MATCH_DTYPE)
            arr = np.empty(n, MATCH_DTYPE)
            ctypes.memmove(arr.ctypes.data, out, n * ctypes.sizeof(_CMatch))
            return arr
        finally:
            self._lib.lm_free(out)

    def matchArray(self, sources, threshold: float, class_ids: Sequence[str] = (), masks=()) -> np.ndarray:
        """match() returning a structured array (class_index refers to class_ids / sorted classIds())."""
        rgb, depth, shape = self._sources(sources, True)
        carr, n, _names = self._class_args(class_ids)
        marr, keep = self._mask_args(masks, shape)
        out, cnt = ctypes.POINTER(_CMatch)(), ctypes.c_size_t()
        _check(self._lib.lm_detector_match(self._h, _ptr(rgb), _ptr(depth), shape[1], shape[0], float(threshold),
                                           carr, n, marr, ctypes.byref(out), ctypes.byref(cnt)))
        return self._take(out, cnt.value)

    def match(self, sources, threshold: float, class_ids: Sequence[str] = (), masks=()) -> List[Match]:
        """Detector::match (LL.cpp:1702-1777).  With torch.distributed initialised and setShard()
        called by the caller, use `match_sharded` from `sharded.py` to gather all ranks."""
        recs = self.matchArray(sources, threshold, class_ids, masks)
        names = list(class_ids) if class_ids else self.classIds()
        # column lists first: indexing a structured array record by record costs ~5 us per match
        cols = [recs[f].tolist() for f in ("x", "y", "similarity", "class_index", "template_id")]
        return [Match(x, y, s, names[c], t) for x, y, s, c, t in zip(*cols)]

    # ---- depth slabs: template scales from the scene's depth histogram ----------------------------
    @staticmethod
    def _mode_options(bin_mm=25, near_mm=300, far_mm=4000, window=2, min_pixels=1000, max_modes=8) -> DepthModeOptions:
        vals = (bin_mm, near_mm, far_mm, window, min_pixels, max_modes)
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or abs(int(v)) > 2 ** 30 for v in vals):
            raise RuntimeError("depth modes: bin_mm, near_mm, far_mm, window, min_pixels and max_modes are integers, got %r" % (vals,))
        return DepthModeOptions(*[int(v) for v in vals])

    def depthModes(self, **mode_options) -> np.ndarray:
        """lm_detector_depth_modes: the primary depths of the resident frame (setFrame / selectFrame, in the aligned geometry of setBorder) as
        DEPTH_MODE_DTYPE records (bin, depth_mm, pixels), most pixels first.  Options: bin_mm=25, near_mm=300, far_mm=4000, window=2,
        min_pixels=1000, max_modes=8.  A pixel with near_mm <= d < far_mm counts in bin (d - near_mm) // bin_mm; bin b is a mode iff
        h[b] >= min_pixels, h[b] > h[j] for j in [b - window, b) and h[b] >= h[j] for j in (b, b + window]; depth_mm is the bin's centre
        near_mm + b * bin_mm + bin_mm // 2.  Exact: tests/depth_slabs_ref.py says the same in numpy."""
        opt = self._mode_options(**mode_options)
        out = np.zeros(16, DEPTH_MODE_DTYPE)
        n = ctypes.c_int()
        _check(self._lib.lm_detector_depth_modes(self._h, ctypes.byref(opt), _ptr(out), len(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def setClassDepthRange(self, class_id: str, lo_mm, hi_mm) -> None:
        """lm_detector_set_class_depth_range: the band of scene depths [lo_mm, hi_mm] at which this class's templates are valid — for a class
        rendered at radius r, say 0.85 r .. 1.15 r.  (None, None) clears it.  Host state of this detector: no file stores it, readClasses and
        readBank produce classes without a range."""
        if lo_mm is None and hi_mm is None:
            _check(self._lib.lm_detector_set_class_depth_range(self._h, class_id.encode(), 0, 0, 1))
            return
        if any(v is None or isinstance(v, bool) or not isinstance(v, (int, np.integer)) or abs(int(v)) > 2 ** 30 for v in (lo_mm, hi_mm)):
            raise RuntimeError("a depth range is two integers lo_mm <= hi_mm (mm), or None, None; got %r" % ((lo_mm, hi_mm),))
        _check(self._lib.lm_detector_set_class_depth_range(self._h, class_id.encode(), int(lo_mm), int(hi_mm), 0))

    def getClassDepthRange(self, class_id: str):
        """(lo_mm, hi_mm) of setClassDepthRange, or None for a class without a range."""
        lo, hi = ctypes.c_int(), ctypes.c_int()
        have = _check(self._lib.lm_detector_get_class_depth_range(self._h, class_id.encode(), ctypes.byref(lo), ctypes.byref(hi)))
        return (int(lo.value), int(hi.value)) if have else None

    def matchSlabsResident(self, threshold: float, class_ids: Sequence[str] = (), masks=(), slab_mm: int = 150, **mode_options):
        """lm_detector_match_slabs on the resident frame: every class with a depth range is matched once per primary depth p of the scene
        (depthModes(**mode_options)) inside its range, under the slab mask "d != 0 and p - slab_mm <= d <= p + slab_mm" ANDed with the frame's own
        masks; classes without a range are matched once, without a slab.  Returns (records, slabs): the canonical merge of all passes
        (MATCH_DTYPE, class_index as in matchArray) and one dict per mode, in mode order — depth_mm, pixels, lo_mm, hi_mm, class_ids, records
        (before the merge; 0 with class_ids == [] for a slab no class wanted) — plus a last one with depth_mm None for the pass of the classes
        without a range.  The masks of the resident frame are those given to setFrame: `masks` must be empty here (matchSlabs takes them)."""
        if masks is not None and len(masks):
            raise RuntimeError("matchSlabsResident matches the resident frame under the masks setFrame was given: pass masks to setFrame or matchSlabs")
        if isinstance(slab_mm, bool) or not isinstance(slab_mm, (int, np.integer)) or abs(int(slab_mm)) > 2 ** 30:
            raise RuntimeError("slab_mm must be an integer (mm), got %r" % (slab_mm,))
        opt = self._mode_options(**mode_options)
        carr, n, names = self._class_args(class_ids)
        out, cnt = ctypes.POINTER(_CMatch)(), ctypes.c_size_t()
        slabs = (_CSlab * 17)()
        ns, cls = ctypes.c_int(), ctypes.POINTER(ctypes.c_int32)()
        _check(self._lib.lm_detector_match_slabs(self._h, float(threshold), carr, n, int(slab_mm), ctypes.byref(opt), ctypes.byref(out),
                                                 ctypes.byref(cnt), slabs, len(slabs), ctypes.byref(ns), ctypes.byref(cls)))
        try:
            info = []
            for s in slabs[:ns.value]:
                ids = [names[cls[i]] for i in range(s.first_class, s.first_class + s.num_classes)]
                free = s.depth_mm < 0
                info.append({"depth_mm": None if free else int(s.depth_mm), "pixels": None if free else int(s.pixels),
                             "lo_mm": None if free else int(s.lo_mm), "hi_mm": None if free else int(s.hi_mm), "class_ids": ids,
                             "records": int(s.records)})
        finally:
            self._lib.lm_free(cls)
        return self._take(out, cnt.value), info

    def matchSlabs(self, sources, threshold: float, class_ids: Sequence[str] = (), masks=(), slab_mm: int = 150, **mode_options):
        """setFrame(sources, masks) followed by matchSlabsResident(threshold, class_ids, slab_mm=slab_mm, **mode_options)."""
        self._sources(sources, True)
        self._mode_options(**mode_options)                    # (refuse bad options before the upload)
        self.setFrame(sources, masks)
        return self.matchSlabsResident(threshold, class_ids, (), slab_mm, **mode_options)

    # ---- depth-scaled matching: every template scaled, per position, to the scene depth found there ----
    def setClassTrainDepth(self, class_id: str, depth_mm: int) -> None:
        """lm_detector_set_class_train_depth: the distance (mm, 1..65535) at which the templates of this class were made.  Host state of this
        detector: no file stores it, readClasses and readBank produce classes without one."""
        if isinstance(depth_mm, bool) or not isinstance(depth_mm, (int, np.integer)) or abs(int(depth_mm)) > 2 ** 30:
            raise RuntimeError("a training depth is an integer (mm), got %r" % (depth_mm,))
        _check(self._lib.lm_detector_set_class_train_depth(self._h, class_id.encode(), int(depth_mm)))

    def classTrainDepth(self, class_id: str):
        """The depth of setClassTrainDepth, or None for a class without one."""
        v = ctypes.c_int()
        have = _check(self._lib.lm_detector_get_class_train_depth(self._h, class_id.encode(), ctypes.byref(v)))
        return int(v.value) if have else None

    def matchScaledResident(self, threshold: float, class_ids: Sequence[str] = (), scales=DEFAULT_SCALES, min_scale=None, max_scale=None,
                            probe: int = 2) -> np.ndarray:
        """lm_detector_match_scaled on the resident frame: at every top-level position the template is scaled by the entry of `scales` nearest to
        d_train / d, d the smallest non-zero depth of the (2 probe + 1)^2 level-0 pixels under the template's centre and d_train the class's
        setClassTrainDepth; positions where d is 0 or d_train / d lies outside [min_scale, max_scale] (default: the first and last scale) are
        not matched.  `scales`, `min_scale` and `max_scale` are floats, converted to Q10 by scale_q10 (floor(1024 s + 0.5)); 1 to 16 strictly
        ascending scales in [0.5, 2].  Returns SCALED_MATCH_DTYPE records (x, y, similarity, class_index, template_id, scale_index, depth_mm): x,
        y, similarity as matchArray gives them (scaled_box turns a record into the object's box), ordered by similarity descending, then
        class_index, template_id, y, x, scale_index, depth_mm.  The rule is stated in numpy in tests/scaled_match_ref.py.  A cell outside the
        level reads 0 here (no wrap into the next row): the one departure from match().  Refused: a detector without DepthNormal, a sharded
        detector, part matching, a detector with a Pipeline, frames in flight, no resident frame, a bad ladder, a class without a training depth."""
        opt = scaled_options(scales, min_scale, max_scale, probe)
        carr, n, _names = self._class_args(class_ids)
        out, cnt = ctypes.POINTER(_CScaledMatch)(), ctypes.c_size_t()
        _check(self._lib.lm_detector_match_scaled(self._h, float(threshold), carr, n, ctypes.byref(opt), ctypes.byref(out), ctypes.byref(cnt)))
        try:
            arr = np.empty(cnt.value, SCALED_MATCH_DTYPE)
            if cnt.value:
                ctypes.memmove(arr.ctypes.data, out, cnt.value * ctypes.sizeof(_CScaledMatch))
            return arr
        finally:
            self._lib.lm_free(out)

    def matchScaled(self, sources, threshold: float, class_ids: Sequence[str] = (), masks=(), **scaled) -> np.ndarray:
        """setFrame(sources, masks) followed by matchScaledResident(threshold, class_ids, **scaled)."""
        self._sources(sources, True)
        scaled_options(scaled.get("scales", DEFAULT_SCALES), scaled.get("min_scale"), scaled.get("max_scale"), scaled.get("probe", 2))   # (refuse a bad ladder before the upload)
        self.setFrame(sources, masks)
        return self.matchScaledResident(threshold, class_ids, **scaled)

    def lastTimings(self) -> dict:
        t = Timings()
        _check(self._lib.lm_detector_last_timings(self._h, ctypes.byref(t)))
        return t.as_dict()

    def lastTimingsInto(self, t: "Timings") -> None:
        """lm_timings of the last collected frame into a caller-owned Timings struct (a per-frame loop that must stay cheap
        keeps an array of them and reads the fields afterwards)."""
        self._lib.lm_detector_last_timings(self._h, ctypes.byref(t))

    def readStage(self, level: int, kind: int) -> np.ndarray:  # (arrays of the aligned geometry: alignedSize() of the source under setBorder)
        """Device intermediates of the last front end run (tests): kind 0/1 quantised colour/normal,
        2/3 linear memories colour/normal, 4 strip records of a level below the top, 5 pair stream of the top level (bit planes),
        6 / 7 the second set of the "wide" paths in the layout of 4 / 5 (after a match that ran on it), 8 the quantised normals of level 0
        before the 5x5 median (level 0 only; of the last synchronous front end: addTemplate, a lone match, the first frame of a batch)."""
        n = _check(self._lib.lm_detector_read_stage(self._h, level, kind, None, 0))
        buf = np.zeros(n, np.uint8)
        _check(self._lib.lm_detector_read_stage(self._h, level, kind, _ptr(buf), n))
        return buf


def scale_q10(scale) -> int:
    """A scale as the Q10 integer the matcher uses: floor(1024 * scale + 0.5) (1024 is scale 1)."""
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale) or abs(scale) > 2 ** 20:
        raise RuntimeError("a scale is a finite number, got %r" % (scale,))
    return int(np.floor(1024.0 * float(scale) + 0.5))


def scaled_options(scales=DEFAULT_SCALES, min_scale=None, max_scale=None, probe: int = 2) -> ScaledOptions:
    """lm_scaled_options of a ladder of float scales (scale_q10 each), optional float bounds and the probe radius; the library checks the values."""
    q = [scale_q10(s) for s in scales]
    if not 1 <= len(q) <= 16:
        raise RuntimeError("scaled matching: the ladder has 1..16 scales, got %d" % len(q))
    if isinstance(probe, bool) or not isinstance(probe, (int, np.integer)) or abs(int(probe)) > 2 ** 30:
        raise RuntimeError("probe must be an integer, got %r" % (probe,))
    lo = 0 if min_scale is None else scale_q10(min_scale)
    hi = 0 if max_scale is None else scale_q10(max_scale)
    if (min_scale is not None and lo < 1) or (max_scale is not None and hi < 1):
        raise RuntimeError("scaled matching: bad scale bounds %r, %r" % (min_scale, max_scale))
    opt = ScaledOptions()
    opt.num_scales = len(q)
    for i, v in enumerate(q):
        opt.scales_q10[i] = v
    opt.min_scale_q10, opt.max_scale_q10, opt.probe = lo, hi, int(probe)
    return opt


def scaled_features(width: int, height: int, xs, ys, scale_q10_value: int):
    """lm_scaled_features (no detector, no GPU): the features (xs, ys) of an entry of box (width, height) scaled about its centre (width // 2,
    height // 2) by the Q10 scale: c + sign(v - c) * ((|v - c| * s + 512) >> 10).  Returns (xs, ys) as int32 arrays."""
    lib = load_library()
    xs = np.ascontiguousarray(xs, np.int32); ys = np.ascontiguousarray(ys, np.int32)
    if xs.shape != ys.shape or xs.ndim != 1:
        raise RuntimeError("xs and ys are 1-D arrays of one length")
    ox, oy = np.empty_like(xs), np.empty_like(ys)
    _check(lib.lm_scaled_features(int(width), int(height), _ptr(xs), _ptr(ys), len(xs), int(scale_q10_value), _ptr(ox), _ptr(oy)))
    return ox, oy


def scaled_box(record, template, scales=DEFAULT_SCALES):
    """The object's box (x0, y0, width, height), floats, of a SCALED_MATCH_DTYPE record: centre (x + w0 // 2, y + h0 // 2) of the level-0
    template (anything with .width and .height, or a (w0, h0) pair), size s_k * (w0, h0), s_k = scale_q10(scales[scale_index]) / 1024."""
    w0, h0 = (template.width, template.height) if hasattr(template, "width") else template
    s = scale_q10(scales[int(record["scale_index"])]) / 1024.0
    cx, cy = int(record["x"]) + int(w0) // 2, int(record["y"]) + int(h0) // 2
    return cx - s * w0 / 2.0, cy - s * h0 / 2.0, s * w0, s * h0


def bank_file_info(path) -> dict:
    """Header of a packed bank file (no detector, no GPU): pyramid levels, class ids, template pyramid and feature counts."""
    lib = load_library()
    lv, nc = ctypes.c_int32(), ctypes.c_int32()
    npyr, nf = ctypes.c_int64(), ctypes.c_int64()
    _check(lib.lm_bank_file_info(os.fspath(path).encode(), ctypes.byref(lv), ctypes.byref(nc), ctypes.byref(npyr), ctypes.byref(nf)))
    ids = []
    buf = ctypes.create_string_buffer(4096)
    for i in range(nc.value):
        _check(lib.lm_bank_file_class_id(os.fspath(path).encode(), i, buf, len(buf)))
        ids.append(buf.value.decode())
    return {"pyramid_levels": lv.value, "class_ids": ids, "num_pyramids": npyr.value, "num_features": nf.value}


def bank_file_modalities(path) -> tuple:
    """The modality set a packed bank file was written for (no detector, no GPU; lm_bank_file_modalities).  Files from before the set existed
    report ("ColorGradient", "DepthNormal")."""
    out = (ctypes.c_char_p * 2)()
    return tuple(out[i].decode() for i in range(_check(load_library().lm_bank_file_modalities(os.fspath(path).encode(), out))))


def rgb_to_grey(rgb, device: int = 0) -> np.ndarray:
    """The grey image a detector with colour_channels=1 trains on when add_templates_rendered feeds it a colour render, for any uint8 (..., 3)
    array in R, G, B order: (4899 R + 9617 G + 1868 B + 8192) >> 14, computed by the same kernel (lm_rgb_to_grey).  Train a mono camera's
    templates from colour photographs through it.  rgb_to_grey_ref is the formula in numpy."""
    a = np.ascontiguousarray(_rgb_last_axis(rgb))
    out = np.zeros(a.shape[:-1], np.uint8)
    _check(load_library().lm_rgb_to_grey(int(device), _ptr(a), out.size, _ptr(out)))
    return out


def merge_matches(records: np.ndarray) -> np.ndarray:
    """Canonical sort + unique of gathered MATCH_DTYPE records (lm_merge_matches; LL.cpp:1771-1776)."""
    recs = np.ascontiguousarray(records, MATCH_DTYPE).copy()
    n = load_library().lm_merge_matches(_ptr(recs), len(recs))
    return recs[:n]


def nms(dets: np.ndarray, thresh: float) -> List[int]:
    """The driver's box NMS (linemod_and_levelup_test.py:34-61): dets rows = x1,y1,x2,y2,score."""
    dets = np.ascontiguousarray(dets, np.float64)
    if len(dets) == 0:
        return []
    boxes = np.ascontiguousarray(dets[:, :4])
    scores = np.ascontiguousarray(dets[:, 4])
    keep = np.zeros(len(dets), np.int32)
    n = load_library().lm_nms_boxes(_ptr(boxes), _ptr(scores), len(dets), float(thresh), _ptr(keep))
    return keep[:n].tolist()


def nms_norms(ts: np.ndarray, scores: np.ndarray, thresh: float) -> List[int]:
    """Translation NMS over refined poses: linemod_ros/detect.py:41-51 (`nms_norms(ts, ts_scores, 40.0)`)."""
    ts = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(-1, 3))
    scores = np.ascontiguousarray(scores, np.float64)
    if len(ts) == 0:
        return []
    keep = np.zeros(len(ts), np.int32)
    n = load_library().lm_nms_norms(_ptr(ts), _ptr(scores), len(ts), float(thresh), _ptr(keep))
    return keep[:n].tolist()


def NMSBoxes(bboxes, scores, score_threshold: float, nms_threshold: float, eta: float = 1.0, top_k: int = 0) -> List[int]:
    """cv::dnn::NMSBoxes / cv2.dnn.NMSBoxes on integer rectangles (x, y, width, height), as linemodLevelup/test.cpp:132-144
    filters the matches (40x40 boxes, score_threshold 0, nms_threshold 0.4)."""
    rects = np.ascontiguousarray(np.asarray(bboxes, np.int32).reshape(-1, 4))
    sc = np.ascontiguousarray(scores, np.float32)
    if len(rects) == 0:
        return []
    keep = np.zeros(len(rects), np.int32)
    n = load_library().lm_nms_boxes_cv(_ptr(rects), _ptr(sc), len(rects), float(score_threshold), float(nms_threshold), float(eta), int(top_k), _ptr(keep))
    return keep[:n].tolist()
