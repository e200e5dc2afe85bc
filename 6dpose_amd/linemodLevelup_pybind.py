"""Drop-in replacement for the reference's pybind11 module `linemodLevelup_pybind`
(/root/reference/linemodLevelup/pybind11.cpp:7-35) on AMD Instinct MI355X.

Same classes, method names, positional order and keywords as the reference binding:

    Detector(), Detector(T), Detector(num_features, T)            pybind11.cpp:26-28
      .addTemplate(sources, class_id, object_mask) -> int          :29   (LL.cpp:1943)
      .writeClasses(format) / .readClasses(class_ids, format)      :30-31 (LL.cpp:2124-2146)
      .match(sources, threshold, class_ids, masks=[]) -> [Match]   :32-33 (LL.cpp:1702)
      .getTemplates(class_id, template_id)                         :34   (LL.cpp:1976)
    Match(): x, y, similarity, class_id, template_id               :16-22 (LL.h:225-258)
    poseRefine(): process(...), getResidual(), getR(), getT()      :9-14  (LL.cpp:27-170)

Everything numeric happens in libamdlinemod.so (hand-written HIP kernels for gfx950 behind the C ABI
of include/amd_linemod.h), reached through ctypes.  There is no CPU fallback: importing works
anywhere (so that host-side code can be unit-tested), but constructing a Detector or calling
poseRefine.process without the library or without a GPU raises RuntimeError.

Errors: the reference turns CV_Assert failures into Python RuntimeError (cv::Exception through
pybind11's default translator); this module raises RuntimeError with the message of
lm_last_error() for the same preconditions.  addTemplate keeps the -1 convention, poseRefine the
residual == -1 convention.

Array conventions (np2mat/ndarray_converter.cpp:159-336 is zero-copy and never checks dtypes, so a
float depth image is silently reinterpreted — driver comment linemod_and_levelup_test.py:117):
this wrapper validates instead: sources = [rgb uint8 HxWx3, depth uint16 HxW]; other dtypes raise.
Detector(..., colour_channels=1) takes a grey image, uint8 HxW, in the colour slot.

This file is the import name only.  The code lives in the flat modules beside it, one per subsystem: lm_abi (library loading, the
structures, the prototype table of the C ABI), lm_detector, lm_icp, lm_pso, lm_render and lm_pose_error.  The loaded library is
lm_abi._lib, set by load_library(); a global assigned after import does not travel through a re-export, so it has no alias here.
"""
from lm_abi import (DEPTH_MODE_DTYPE, LM_ICP_POINT_TO_POINT, LM_ICP_SCENE_FROM_SCENE, MATCH_DTYPE, SCALED_MATCH_DTYPE, DepthModeOptions, ScaledOptions, IcpOptions, PipelineTimings, RenderOptions, Timings,
                    _CDetection, _CMatch, _CPoseResult, _as_depth, _as_grey, _as_mask, _as_rgb, _check, _ptr, _share_hip_runtime_with_torch,
                    aligned_size, bind_near_device, library_path, load_library, rgb_to_grey_ref)
from lm_detector import (DEFAULT_SCALES, Comm, Detector, Match, NMSBoxes, Template, bank_file_info, bank_file_modalities, merge_matches, nms,
                         nms_norms, rgb_to_grey, scale_q10, scaled_box, scaled_features, scaled_options)
from lm_icp import (ICP_ESTIMATIONS, IcpContext, Pipeline, _icp_flags, _icp_options, _pose_dict, evaluate_registration, poseRefine,
                    pose_refine_batch)
from lm_pso import PSO_DEBUG_KINDS, PsoContext, derive_windows, pso_options, pso_refine, pso_refine_edges, pso_refine_oriented
from lm_render import OVERLAY_MODES, SHADINGS, Mesh, _colour, add_templates_rendered, render_options
from lm_pose_error import (POSE_METRICS, POSE_METRICS_SYM, _pose_batch, _scene_mm, bop19_thresholds, gt_stats, match_poses, pose_errors,
                           recall, symmetry_transforms)

__all__ = ["Detector", "Match", "poseRefine", "IcpContext", "Pipeline", "Mesh", "Template", "library_path", "load_library", "nms",
           "pose_errors", "gt_stats", "symmetry_transforms", "match_poses", "recall", "bop19_thresholds", "PsoContext", "pso_refine", "pso_refine_edges", "pso_refine_oriented"]
