"""The C ABI of libamdlinemod.so (include/amd_linemod.h) as ctypes sees it: where the library is found and loaded, the structures,
the argument checks every subsystem shares, and PROTOTYPES, the one place a function of the header is declared.  A new function gets
one line there; tests/test_abi_table.py holds the table to the header and to the library's exported symbols."""
from __future__ import annotations

import ctypes
import importlib.util
import os
import sys
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libamdlinemod.so"
_lib = None


class _CMatch(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("similarity", ctypes.c_float),
                ("class_index", ctypes.c_int32), ("template_id", ctypes.c_int32)]


class Timings(ctypes.Structure):
    """lm_timings (include/amd_linemod.h)."""
    _fields_ = [("h2d_ms", ctypes.c_float), ("frontend_ms", ctypes.c_float), ("coarse_ms", ctypes.c_float),
                ("local_ms", ctypes.c_float), ("d2h_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("coarse_candidates", ctypes.c_int64), ("local_evals", ctypes.c_int64),
                ("matches_pre_unique", ctypes.c_int64), ("templates", ctypes.c_int64),
                ("coarse_bytes", ctypes.c_int64), ("local_bytes", ctypes.c_int64),
                ("host_submit_ms", ctypes.c_float), ("host_wait_ms", ctypes.c_float),
                ("host_collect_ms", ctypes.c_float), ("host_merge_ms", ctypes.c_float), ("batch_frames", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _CPoseResult(ctypes.Structure):
    _fields_ = [("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("residual", ctypes.c_float),
                ("inlier_rmse", ctypes.c_float), ("iterations", ctypes.c_int32), ("n_source", ctypes.c_int32),
                ("n_target", ctypes.c_int32), ("stage", ctypes.c_int32)]


class _CDetection(ctypes.Structure):
    _fields_ = [("match", _CMatch), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("status", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("pose", _CPoseResult)]


class PipelineTimings(ctypes.Structure):
    """lm_pipeline_timings (include/amd_linemod.h)."""
    _fields_ = [("match_ms", ctypes.c_float), ("nms_ms", ctypes.c_float), ("icp_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("coarse_candidates", ctypes.c_int64), ("matches_pre_unique", ctypes.c_int64), ("icp_iterations", ctypes.c_int32),
                ("nms_records", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IcpOptions(ctypes.Structure):
    """lm_icp_options (include/amd_linemod.h): open3d ICPConvergenceCriteria."""
    _fields_ = [("max_iteration", ctypes.c_int32), ("reserved", ctypes.c_int32), ("relative_fitness", ctypes.c_double),
                ("relative_rmse", ctypes.c_double)]


class RenderOptions(ctypes.Structure):
    """lm_render_options (include/amd_linemod.h)."""
    _fields_ = [("size", ctypes.c_uint32), ("shading", ctypes.c_int32), ("use_texture", ctypes.c_int32), ("has_surf_color", ctypes.c_int32),
                ("surf_color", ctypes.c_float * 3), ("bg_color", ctypes.c_float * 4), ("ambient", ctypes.c_float), ("ssaa", ctypes.c_int32),
                ("clip_near", ctypes.c_float), ("clip_far", ctypes.c_float)]


class DepthModeOptions(ctypes.Structure):
    """lm_depth_mode_options (include/amd_linemod_depth.h)."""
    _fields_ = [("bin_mm", ctypes.c_int32), ("near_mm", ctypes.c_int32), ("far_mm", ctypes.c_int32), ("window", ctypes.c_int32),
                ("min_pixels", ctypes.c_int32), ("max_modes", ctypes.c_int32)]


class _CDepthMode(ctypes.Structure):
    _fields_ = [("bin", ctypes.c_int32), ("depth_mm", ctypes.c_int32), ("pixels", ctypes.c_uint32)]


class _CSlab(ctypes.Structure):
    _fields_ = [("depth_mm", ctypes.c_int32), ("pixels", ctypes.c_uint32), ("lo_mm", ctypes.c_int32), ("hi_mm", ctypes.c_int32),
                ("first_class", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("records", ctypes.c_int64)]


class ScaledOptions(ctypes.Structure):
    """lm_scaled_options (include/amd_linemod_scaled.h)."""
    _fields_ = [("num_scales", ctypes.c_int32), ("scales_q10", ctypes.c_int32 * 16), ("min_scale_q10", ctypes.c_int32),
                ("max_scale_q10", ctypes.c_int32), ("probe", ctypes.c_int32)]


class _CScaledMatch(ctypes.Structure):
    """lm_scaled_match (include/amd_linemod_scaled.h)."""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("similarity", ctypes.c_float), ("class_index", ctypes.c_int32),
                ("template_id", ctypes.c_int32), ("scale_index", ctypes.c_int32), ("depth_mm", ctypes.c_int32)]


class PsoOptions(ctypes.Structure):
    """lm_pso_options (include/amd_linemod_pso.h)."""
    _fields_ = [("size", ctypes.c_uint32), ("particles", ctypes.c_int32), ("generations", ctypes.c_int32), ("tau", ctypes.c_int32),
                ("cover_pixels", ctypes.c_int32), ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64), ("trans_range_mm", ctypes.c_double),
                ("rot_range", ctypes.c_double), ("inertia", ctypes.c_double), ("c1", ctypes.c_double), ("c2", ctypes.c_double),
                ("clip_near", ctypes.c_double), ("clip_far", ctypes.c_double)]


class _CPsoResult(ctypes.Structure):
    """lm_pso_result (include/amd_linemod_pso.h)."""
    _fields_ = [("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("cost", ctypes.c_double), ("initial_cost", ctypes.c_double),
                ("n_rendered", ctypes.c_int32), ("n_initial", ctypes.c_int32), ("best_particle", ctypes.c_int32), ("best_generation", ctypes.c_int32)]


DEPTH_MODE_DTYPE = np.dtype([("bin", np.int32), ("depth_mm", np.int32), ("pixels", np.uint32)])
MATCH_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("similarity", np.float32),
                        ("class_index", np.int32), ("template_id", np.int32)])
SCALED_MATCH_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("similarity", np.float32), ("class_index", np.int32),
                               ("template_id", np.int32), ("scale_index", np.int32), ("depth_mm", np.int32)])
LM_ICP_SCENE_FROM_SCENE = 1
LM_ICP_POINT_TO_POINT = 2

# ---- the prototype table: name -> (restype, [argtypes]), every function of include/amd_linemod.h exactly once, in its order ----------
# Pointers to plain buffers are c_void_p, so a numpy .ctypes.data_as(c_void_p), None and an integer address all pass; typed pointers
# stand where the callers hand over a ctypes object or array (byref of a handle, a c_char_p array, a structure).
P, I, F, D, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_char_p
Z, U64, I64 = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int64
PP, PI, PS, PZ = ctypes.POINTER(P), ctypes.POINTER(I), ctypes.POINTER(S), ctypes.POINTER(Z)
PM, PPM, PU8 = ctypes.POINTER(_CMatch), ctypes.POINTER(ctypes.POINTER(_CMatch)), ctypes.POINTER(ctypes.c_uint8)
PDMO = ctypes.POINTER(DepthModeOptions)
PPOSE, PICPO, PRO = ctypes.POINTER(_CPoseResult), ctypes.POINTER(IcpOptions), ctypes.POINTER(RenderOptions)
PPSOO = ctypes.POINTER(PsoOptions)
PROTOTYPES = {
    "lm_last_error": (S, []),
    "lm_version": (S, []),
    "lm_device_count": (I, []),
    "lm_bind_thread_near_device": (I, [I, S, Z]),
    # detector: creation, training, files, queries
    "lm_detector_create": (I, [I, PI, I, I, PP]),
    "lm_detector_create_modalities": (I, [I, PI, I, I, PS, I, PP]),
    "lm_detector_get_modalities": (I, [P, PS]),
    "lm_detector_set_colour_channels": (I, [P, I]),
    "lm_detector_get_colour_channels": (I, [P]),
    "lm_detector_set_border": (I, [P, I]),
    "lm_detector_get_border": (I, [P]),
    "lm_detector_aligned_size": (I, [P, I, I, I, PI, PI]),
    "lm_rgb_to_grey": (I, [I, P, I64, P]),
    "lm_detector_destroy": (None, [P]),
    "lm_detector_add_template": (I, [P, P, P, P, I, I, S]),
    "lm_detector_read_class": (I, [P, S, S]),
    "lm_detector_write_class": (I, [P, S, S]),
    "lm_detector_write_params": (I, [P, S]),
    "lm_detector_read_params": (I, [P, S]),
    "lm_detector_add_class_packed": (I, [P, S, I, P, P, P]),
    "lm_detector_write_bank": (I, [P, S, PS, I]),
    "lm_detector_read_bank": (I, [P, S, PS, I]),
    "lm_bank_file_info": (I, [S, P, P, P, P]),
    "lm_bank_file_class_id": (I, [S, I, P, I]),
    "lm_bank_file_modalities": (I, [S, PS]),
    "lm_detector_num_classes": (I, [P]),
    "lm_detector_class_id": (S, [P, I]),
    "lm_detector_num_templates": (I, [P, S]),
    "lm_detector_pyramid_levels": (I, [P]),
    "lm_detector_get_T": (I, [P, I]),
    "lm_detector_get_template": (I, [P, S, I, I, P, P, P, P, P, I]),
    "lm_detector_set_shard": (I, [P, I, I]),
    # multi-GPU exchange and the RCCL communicator
    "lm_exchange_max_capacity": (I, []),
    "lm_detector_max_in_flight": (I, []),
    "lm_detector_exchange_stream": (P, [P]),
    "lm_exchange_block_bytes": (Z, [I]),
    "lm_detector_exchange_pack": (I, [P, P, I]),
    "lm_detector_exchange_merge": (I, [P, P, I, I]),
    "lm_detector_frames_submitted": (U64, [P]),
    "lm_detector_frames_launched": (U64, [P]),
    "lm_detector_frames_collected": (U64, [P]),
    "lm_detector_exchange_pack_frame": (I, [P, U64, P, I]),
    "lm_detector_exchange_merge_frame": (I, [P, U64, P, I, I]),
    "lm_detector_exchange_merge_frame_strided": (I, [P, U64, P, I, I, Z]),
    "lm_detector_exchange_pack_group": (I, [P, U64, I, P, I]),
    "lm_detector_exchange_merge_group": (I, [P, U64, I, P, I, I]),
    "lm_detector_exchange_collect": (I, [P, PPM, PZ, PI]),
    "lm_detector_exchange_collect_into": (I, [P, P, Z, PZ, PI]),
    "lm_comm_available": (I, []),
    "lm_comm_unique_id": (I, [P]),
    "lm_comm_create": (I, [P, I, I, I, PP]),
    "lm_comm_destroy": (None, [P]),
    "lm_comm_rank": (I, [P]),
    "lm_comm_world": (I, [P]),
    "lm_exchange_allgather": (I, [P, P, P, P, Z]),
    "lm_detector_exchange_group": (I, [P, P, U64, I, P, P, I]),
    # matching: one call, resident frame, pipelined and streamed
    "lm_detector_match": (I, [P, P, P, I, I, F, PS, I, PP, PPM, PZ]),
    "lm_detector_set_frame": (I, [P, P, P, I, I, PP]),
    "lm_detector_store_frame": (I, [P, I, P, P, I, I]),
    "lm_detector_select_frame": (I, [P, I]),
    "lm_detector_match_resident": (I, [P, F, PS, I, I, PPM, PZ]),
    "lm_detector_submit": (I, [P, F, PS, I]),
    "lm_detector_collect": (I, [P, I, PPM, PZ]),
    "lm_detector_set_reference_order": (I, [P, I]),
    "lm_detector_submit_frame": (I, [P, P, P, I, I, F, PS, I]),
    "lm_detector_ingest_buffer": (I, [P, I, I, PP, PP]),
    "lm_detector_flush": (I, [P]),
    "lm_detector_set_batch": (I, [P, I]),
    "lm_detector_get_batch": (I, [P]),
    "lm_detector_set_batch_queue": (I, [P, I]),
    "lm_detector_set_async_collect": (I, [P, I]),
    "lm_detector_host_profile": (I, [P, ctypes.POINTER(D), I]),
    "lm_detector_refines_on_bit_planes": (I, [P]),
    "lm_detector_set_paths": (I, [P, I, I]),
    "lm_detector_get_paths": (I, [P, PI, PI]),
    "lm_detector_set_response_table": (I, [P, PU8]),
    "lm_detector_get_response_table": (I, [P, PU8]),
    "lm_detector_set_part_matching": (I, [P, I, I]),
    "lm_detector_get_part_matching": (I, [P, PI, PI]),
    "lm_part_table": (I, [I, I, P, P, I, I, P, P]),
    "lm_depth_mode_options_init": (None, [PDMO]),
    "lm_detector_depth_modes": (I, [P, PDMO, P, I, PI]),
    "lm_detector_set_class_depth_range": (I, [P, S, I, I, I]),
    "lm_detector_get_class_depth_range": (I, [P, S, PI, PI]),
    "lm_detector_match_slabs": (I, [P, F, PS, I, I, PDMO, PPM, PZ, ctypes.POINTER(_CSlab), I, PI, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32))]),
    "lm_scaled_options_init": (None, [ctypes.POINTER(ScaledOptions)]),
    "lm_detector_set_class_train_depth": (I, [P, S, I]),
    "lm_detector_get_class_train_depth": (I, [P, S, PI]),
    "lm_detector_match_scaled": (I, [P, F, PS, I, ctypes.POINTER(ScaledOptions), ctypes.POINTER(ctypes.POINTER(_CScaledMatch)), PZ]),
    "lm_scaled_features": (I, [I, I, P, P, I, I, P, P]),
    "lm_detector_bit_arena_bytes": (I, [P, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
    "lm_detector_wide_arena_bytes": (I, [P, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
    "lm_detector_train_stats": (I, [P, ctypes.POINTER(I64)]),
    "lm_detector_set_direct_bits": (I, [P, I]),
    "lm_detector_set_coarse_batch": (I, [P, I]),
    "lm_detector_get_coarse_batch": (I, [P]),
    "lm_detector_set_candidate_capacity": (I, [P, I]),
    "lm_detector_read_candidates": (I64, [P, U64, P, I64]),
    "lm_detector_last_timings": (I, [P, ctypes.POINTER(Timings)]),
    "lm_detector_read_stage": (I64, [P, I, I, P, I64]),
    # host helpers
    "lm_merge_matches": (Z, [P, Z]),
    "lm_nms_boxes": (I, [P, P, I, D, P]),
    "lm_nms_norms": (I, [P, P, I, D, P]),
    "lm_nms_boxes_cv": (I, [P, P, I, F, F, F, I, P]),
    "lm_free": (None, [P]),
    # poseRefine, the resident ICP context, the per-frame pipeline
    "lm_pose_refine": (I, [I, P, P, I, I, P, P, P, P, I, I, I, PPOSE]),
    "lm_pose_refine_batch": (I, [I, P, I, I, P, I, PP, P, P, P, P, I, PPOSE, ctypes.POINTER(F)]),
    "lm_icp_create": (I, [I, PP]),
    "lm_icp_destroy": (None, [P]),
    "lm_icp_options_init": (None, [PICPO]),
    "lm_icp_set_options": (I, [P, PICPO]),
    "lm_icp_set_scene": (I, [P, P, I, I, P]),
    "lm_icp_set_models": (I, [P, I, I, PP]),
    "lm_icp_run": (I, [P, I, P, P, P, P, P, I, PPOSE, ctypes.POINTER(F)]),
    "lm_icp_read_debug": (I64, [P, I, I, P, I64]),
    "lm_pipeline_create": (I, [P, I, I, PP]),
    "lm_pipeline_destroy": (None, [P]),
    "lm_pipeline_set_icp_options": (I, [P, PICPO]),
    "lm_pipeline_set_views": (I, [P, S, I, I, PP, P, P, P, P]),
    "lm_pipeline_read_icp_debug": (I64, [P, I, I, P, I64]),
    "lm_pipeline_run": (I, [P, F, PS, I, P, I, D, I, ctypes.POINTER(_CDetection), PI, ctypes.POINTER(PipelineTimings)]),
    # meshes and rendering
    "lm_mesh_create": (I, [I, P, P, P, I, P, I, PP]),
    "lm_mesh_load_ply": (I, [I, S, PP]),
    "lm_mesh_destroy": (None, [P]),
    "lm_mesh_counts": (I, [P, PI, PI]),
    "lm_mesh_render": (I, [P, I, I, I, P, P, P, F, F, F, I, P, P]),
    "lm_detector_add_templates_rendered": (I, [P, P, S, I, I, I, P, P, P, F, F, F, I, P, P]),
    "lm_render_options_init": (None, [PRO]),
    "lm_mesh_set_texcoords": (I, [P, P, I]),
    "lm_mesh_set_texture": (I, [P, P, I, I]),
    "lm_mesh_texture_info": (I, [P, PI, PI, PI]),
    "lm_mesh_render_ex": (I, [P, I, I, I, P, P, P, PRO, P, P]),
    "lm_detector_add_templates_rendered_ex": (I, [P, P, S, I, I, I, P, P, P, PRO, P, P]),
    "lm_mesh_overlay": (I, [P, I, I, I, P, P, P, P, P, PRO, P, I, P, P]),
    "lm_pipeline_set_views_rendered": (I, [P, P, S, I, I, P, P, P, F, F, P]),
    # pose errors
    "lm_mesh_pose_errors": (I, [P, I, P, P, I, P, P, P, I, I, P, I, D, D, I, D, D, P]),
    "lm_mesh_pose_errors_sym": (I, [P, I, P, P, I, P, P, I, P, P, P, I, P]),
    "lm_pose_sym_tile": (I, []),
    "lm_mesh_gt_stats": (I, [P, I, P, P, P, I, I, P, D, D, D, P, P, P, P]),
    "lm_mesh_diameter": (I, [P, ctypes.POINTER(D)]),
    # the particle-swarm refiner
    "lm_pso_options_init": (None, [PPSOO]),
    "lm_pso_create": (I, [I, PP]),
    "lm_pso_destroy": (None, [P]),
    "lm_pso_set_scene": (I, [P, P, I, I, P]),
    "lm_pso_run": (I, [P, P, I, P, P, P, I, I, PPSOO, ctypes.POINTER(_CPsoResult), ctypes.POINTER(F)]),
    "lm_pso_read_debug": (I64, [P, I, I, P, I64]),
    "lm_pso_set_scene_edges": (I, [P, P, I, I, P, I]),
    "lm_pso_read_edge_distance": (I64, [P, P, I64]),
    "lm_pso_run_edges": (I, [P, P, I, P, P, P, I, I, PPSOO, I, ctypes.POINTER(_CPsoResult), ctypes.POINTER(F)]),
    "lm_pso_set_scene_orientations": (I, [P, P, I, I, P, I, I]),
    "lm_pso_set_scene_from_detector": (I, [P, P, I, P, I, I]),
    "lm_pso_read_orient_distance": (I64, [P, I, P, I64]),
    "lm_pso_run_oriented": (I, [P, P, I, P, P, P, I, I, PPSOO, I, ctypes.POINTER(_CPsoResult), ctypes.POINTER(F)]),
}


def library_path() -> str:
    return os.environ.get("AMD_LINEMOD_LIB", os.path.join(_HERE, _LIB_NAME))


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so; if this library were bound to /opt/rocm's
    copy first, a later `import torch` would bring up a second runtime that finds no GPU ("No HIP GPUs are available"),
    and stream handles could not be shared (sharded.DeviceExchange hands the exchange stream to torch.distributed).
    So when torch is installed, its runtime is loaded first (without importing torch) and libamdlinemod.so binds to it."""
    if "torch" in sys.modules:
        return                                   # already loaded: the dynamic linker reuses it
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:                            # torch absent or not a ROCm build: /opt/rocm's runtime is used
        pass


def load_library():
    """Loads libamdlinemod.so and declares the C ABI (PROTOTYPES).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(lib, name)
        f.restype = restype
        f.argtypes = argtypes
    _lib = lib
    return lib


def bind_near_device(device: int = 0):
    """lm_bind_thread_near_device: the calling thread onto the CPUs next to the GPU; returns the CPU list, or None where sysfs does not tell."""
    lib = load_library()
    buf = ctypes.create_string_buffer(4096)
    if lib.lm_bind_thread_near_device(int(device), buf, 4096) != 0:
        return None
    return buf.value.decode()


def _check(rc: int) -> int:
    if rc < 0:
        raise RuntimeError(load_library().lm_last_error().decode("utf-8", "replace"))
    return rc


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _as_rgb(a, what="sources[0]") -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        hint = " — a grey image needs a detector made with colour_channels=1" if a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1)) else ""
        raise RuntimeError("%s must be a uint8 HxWx3 image (got %s %s)%s" % (what, a.dtype, a.shape, hint))
    return np.ascontiguousarray(a)


def _as_grey(a, what="sources[0]") -> np.ndarray:
    """The colour source of a detector with colour_channels=1: uint8 HxW (HxWx1 is taken as that)."""
    a = np.asarray(a)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.dtype != np.uint8 or a.ndim != 2:
        hint = " — this detector was made with colour_channels=1" if a.ndim == 3 else ""
        raise RuntimeError("%s must be a uint8 HxW grey image (got %s %s)%s" % (what, a.dtype, a.shape, hint))
    return np.ascontiguousarray(a)


def _rgb_last_axis(rgb) -> np.ndarray:
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != 3:
        raise RuntimeError("rgb must be a uint8 array whose last axis holds R, G, B (got %s %s)" % (a.dtype, a.shape))
    return a


def rgb_to_grey_ref(rgb) -> np.ndarray:
    """What rgb_to_grey computes, in numpy (no device): (4899 R + 9617 G + 1868 B + 8192) >> 14 per pixel of a uint8 (..., 3) array in
    R, G, B order — the 8-bit fixed point of OpenCV's RGB2GRAY (unpinned: stated from its documentation, not checked against a build)."""
    v = _rgb_last_axis(rgb).astype(np.int64)
    return ((4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14).astype(np.uint8)


BORDER_POLICIES = {"strict": 0, "pad": 1, "crop": 2}          # lm_detector_set_border


def _border_code(border) -> int:
    if not isinstance(border, str) or border not in BORDER_POLICIES:
        raise RuntimeError("unknown border policy %r: one of 'strict', 'pad', 'crop'" % (border,))
    return BORDER_POLICIES[border]


def aligned_size(T, width: int, height: int, border: str = "pad"):
    """(aligned width, aligned height) of a width x height source for a detector with T = T (one entry per pyramid level), in plain Python
    — the rule of lm_detector_aligned_size, which answers the same.  A size is aligned when at every level l of the L levels
    (W >> l) % T[l] == 0, (H >> l) % T[l] == 0, W and H are multiples of 2 ** (L - 1) and ((W >> l) * (H >> l)) % 16 == 0.  "pad": the
    smallest aligned height >= height, then the smallest width >= width; "crop": the largest height <= height, then the largest width <=
    width, both at least 16; "strict": the size itself.  RuntimeError where there is none ("crop": nothing of at least 16 fits; "strict":
    the size is not aligned)."""
    code = _border_code(border)
    T = [int(t) for t in T]
    L, W, H = len(T), int(width), int(height)
    if L < 1 or any(t < 1 for t in T) or W < 16 or H < 16 or W > 16384 or H > 16384:
        raise RuntimeError("unsupported frame size %dx%d" % (W, H))

    def side_ok(v):
        return v >= 1 and v % (1 << (L - 1)) == 0 and all((v >> l) >= 1 and (v >> l) % T[l] == 0 for l in range(L))

    def area_ok(w, h):
        return all(((w >> l) * (h >> l)) % 16 == 0 for l in range(L))

    if code == 0:
        if not (side_ok(W) and side_ok(H) and area_ok(W, H)):
            raise RuntimeError("%dx%d is not aligned to T = %s [LL.cpp:1136, 1217-1218]" % (W, H, T))
        return W, H
    if code == 1:
        h = next(v for v in range(H, 1 << 20) if side_ok(v))
        w = next(v for v in range(W, 1 << 20) if side_ok(v) and area_ok(v, h))
        if w > 16384 or h > 16384:
            raise RuntimeError("unsupported frame size %dx%d" % (W, H))
        return w, h
    for h in range(H, 15, -1):
        if side_ok(h):
            for w in range(W, 15, -1):
                if side_ok(w) and area_ok(w, h):
                    return w, h
    raise RuntimeError("unsupported frame size %dx%d" % (W, H))


def _as_depth(a, what="sources[1]") -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise RuntimeError("%s must be a uint16 HxW depth image in mm (got %s %s); the reference would "
                           "silently reinterpret the bytes" % (what, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def _as_mask(a, shape) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.asarray(a)
    if a.size == 0:
        return None
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype != np.uint8 or a.shape != tuple(shape):
        raise RuntimeError("mask.empty() || mask.size() == source.size() [LL.cpp:1717] (got %s %s)" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)
