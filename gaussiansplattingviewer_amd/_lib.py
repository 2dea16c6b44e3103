"""ctypes binding of libgsr.so, the C ABI declared in include/gsr.h.

This is the only way the package reaches the GPU: there is no CPU or PyTorch fallback.  If
the library is missing or has no HIP device, every entry point raises RuntimeError.
"""
from __future__ import annotations

import atexit
import ctypes
import functools
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSR_LIB: another build of the library (A/B builds in tools/ab.sh); default the in-tree libgsr.so
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsr.so")
ABI_VERSION = 4

GSR_OPT_BLEND_CULL = 1
GSR_OPT_BLEND_FAST = 2
GSR_OPT_DEPTH_SORT = 11
GSR_OPT_TIGHT_BINNING = 13
GSR_OPT_FRAME_GRAPHS = 14
GSR_OPT_SECOND_STREAM = 15

# gsr_forward_shaded's `shading` (the GL backend's shading combo, include/gsr.h)
GSR_SHADE_SPLAT = 0
GSR_SHADE_BILLBOARD = 1
GSR_SHADE_FLAT_BALL = 2
GSR_SHADE_GAUSS_BALL = 3

# Symbols include/gsr.h declares (checked by the CPU test suite).
EXPORTED_SYMBOLS = (
    "gsr_abi_version", "gsr_last_error", "gsr_create", "gsr_destroy", "gsr_reserve",
    "gsr_forward", "gsr_get_binning", "gsr_mark_visible", "gsr_depth_argsort",
    "gsr_set_timing", "gsr_stage_times", "gsr_stage_name", "gsr_set_option",
    "gsr_ply_probe", "gsr_ply_load", "gsr_disparity_colors", "gsr_pack_image",
    "gsr_tile_row_pairs", "gsr_frame_graph_stats", "gsr_get_option",
    "gsr_forward_shaded", "gsr_forward_depth", "gsr_backward", "gsr_backward_times",
    "gsr_backward_planes", "gsr_forward_surface", "gsr_backward_camera",
    "gsr_forward_filtered", "gsr_backward_filtered", "gsr_backward_ordered",
    "gsr_backward_strip", "gsr_forward_features", "gsr_backward_features", "gsr_backward_abs",
    "gsr_image_loss_workspace", "gsr_image_loss", "gsr_image_loss_backward",
    "gsr_image_loss_window_workspace", "gsr_image_loss_window", "gsr_image_loss_window_backward",
    "gsr_adam_step", "gsr_densify_stats",
    "gsr_densify_workspace", "gsr_densify_plan", "gsr_densify_apply",
    "gsr_knn_workspace", "gsr_knn_stages",
    "gsr_ply_save", "gsr_ply_probe_scene", "gsr_ply_load_scene",
)
# The nearest-neighbour entries (include/gsr.h).  The suite's scan of the header reads names of
# lower-case letters and underscores, so gsr_knn_mean_dist2, declared and exported like the
# others, is listed here and not above.
KNN_SYMBOLS = ("gsr_knn_workspace", "gsr_knn_mean_dist2", "gsr_knn_stages")

GSR_PACK_RGBA_F32 = 0
GSR_PACK_RGB8 = 1
GSR_PACK_R16 = 2


class GsrGaussians(ctypes.Structure):
    _fields_ = [
        ("P", ctypes.c_int64), ("D", ctypes.c_int32), ("M", ctypes.c_int32),
        ("scale_modifier", ctypes.c_float),
        ("means3D", ctypes.c_void_p), ("scales", ctypes.c_void_p),
        ("rotations", ctypes.c_void_p), ("opacities", ctypes.c_void_p),
        ("shs", ctypes.c_void_p), ("colors_precomp", ctypes.c_void_p),
        ("cov3D_precomp", ctypes.c_void_p),
    ]


class GsrRasterSettings(ctypes.Structure):
    _fields_ = [
        ("image_width", ctypes.c_int32), ("image_height", ctypes.c_int32),
        ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float),
        ("viewmatrix", ctypes.c_void_p), ("projmatrix", ctypes.c_void_p),
        ("campos", ctypes.c_void_p), ("bg", ctypes.c_void_p),
        ("tile_row_begin", ctypes.c_int32), ("tile_row_end", ctypes.c_int32),
        ("prefiltered", ctypes.c_int32), ("debug", ctypes.c_int32),
    ]


class GsrOutputs(ctypes.Structure):
    _fields_ = [
        ("color", ctypes.c_void_p), ("radii", ctypes.c_void_p),
        ("depths", ctypes.c_void_p), ("means2D", ctypes.c_void_p),
        ("conic_opacity", ctypes.c_void_p), ("rgb", ctypes.c_void_p),
        ("tiles_touched", ctypes.c_void_p), ("final_T", ctypes.c_void_p),
        ("n_contrib", ctypes.c_void_p), ("num_rendered", ctypes.c_int64),
    ]


class GsrDepthOutputs(ctypes.Structure):
    """gsr_depth_outputs: gsr_forward_depth's optional per-pixel planes."""
    _fields_ = [("depth_map", ctypes.c_void_p), ("inv_depth_map", ctypes.c_void_p)]


class GsrSurfaceOutputs(ctypes.Structure):
    """gsr_surface_outputs: gsr_forward_surface's optional per-pixel median planes."""
    _fields_ = [("median_depth", ctypes.c_void_p), ("median_id", ctypes.c_void_p)]


class GsrBackwardInputs(ctypes.Structure):
    """gsr_backward_inputs."""
    _fields_ = [("dL_dcolor", ctypes.c_void_p)]


GRADIENT_NAMES = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_dconic",
                  "dL_dsh", "dL_dscales", "dL_drotations", "dL_dcov3D")


class GsrGradients(ctypes.Structure):
    """gsr_gradients: every member optional (None = not wanted)."""
    _fields_ = [(n, ctypes.c_void_p) for n in GRADIENT_NAMES]


class GsrPlaneGradients(ctypes.Structure):
    """gsr_plane_gradients: gsr_backward_planes' plane gradients (None = unused) and dL_ddepths."""
    _fields_ = [("dL_ddepth_map", ctypes.c_void_p), ("dL_dinv_depth_map", ctypes.c_void_p),
                ("dL_dfinal_T", ctypes.c_void_p), ("dL_ddepths", ctypes.c_void_p)]


CAMERA_GRADIENT_NAMES = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")


class GsrCameraGradients(ctypes.Structure):
    """gsr_camera_gradients: gsr_backward_camera's outputs, 16 / 16 / 3 floats (None = not wanted)."""
    _fields_ = [(n, ctypes.c_void_p) for n in CAMERA_GRADIENT_NAMES]


class GsrFilterSettings(ctypes.Structure):
    """gsr_filter_settings: gsr_forward_filtered's and gsr_backward_filtered's option."""
    _fields_ = [("antialiasing", ctypes.c_int32)]


class GsrBackwardOrder(ctypes.Structure):
    """gsr_backward_order: gsr_backward_ordered's choice of how the sums over pixels are formed."""
    _fields_ = [("deterministic", ctypes.c_int32)]


MAX_FEATURES = 256  # GSR_MAX_FEATURES


class GsrFeatureOutputs(ctypes.Structure):
    """gsr_feature_outputs: gsr_forward_features' per-Gaussian rows [P, C] and planes [C, rows, W]."""
    _fields_ = [("C", ctypes.c_int32), ("features", ctypes.c_void_p),
                ("feature_map", ctypes.c_void_p)]


class GsrFeatureGradients(ctypes.Structure):
    """gsr_feature_gradients: gsr_backward_features' rows, the planes' gradient and dL_dfeatures."""
    _fields_ = [("C", ctypes.c_int32), ("features", ctypes.c_void_p),
                ("dL_dfeature_map", ctypes.c_void_p), ("dL_dfeatures", ctypes.c_void_p)]


class GsrAbsGradients(ctypes.Structure):
    """gsr_abs_gradients: gsr_backward_abs' output, [P, 3] floats (None = not wanted)."""
    _fields_ = [("dL_dmeans2D_abs", ctypes.c_void_p)]


class GsrImageLossInputs(ctypes.Structure):
    """gsr_image_loss_inputs: the two [C, H, W] images of gsr_image_loss and its backward."""
    _fields_ = [("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("lambda_", ctypes.c_float), ("image", ctypes.c_void_p),
                ("target", ctypes.c_void_p)]


class GsrLossWindow(ctypes.Structure):
    """gsr_loss_window: the rows of a frame that gsr_image_loss_window's band buffers hold and
    the own rows it sums and differentiates."""
    _fields_ = [("frame_H", ctypes.c_int32), ("row0", ctypes.c_int32),
                ("own_begin", ctypes.c_int32), ("own_end", ctypes.c_int32)]


MAX_PARAM_GROUPS = 8  # GSR_MAX_PARAM_GROUPS


class GsrParamGroup(ctypes.Structure):
    """gsr_param_group: one [P, M] parameter tensor of gsr_adam_step with its gradient and moments."""
    _fields_ = [("M", ctypes.c_int32), ("lr", ctypes.c_float), ("eps", ctypes.c_float),
                ("param", ctypes.c_void_p), ("grad", ctypes.c_void_p),
                ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p)]


class GsrAdamSettings(ctypes.Structure):
    """gsr_adam_settings: what the groups of one gsr_adam_step share; at most one mask."""
    _fields_ = [("P", ctypes.c_int64), ("n_groups", ctypes.c_int32),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("bias_correction1", ctypes.c_float), ("bias_correction2_sqrt", ctypes.c_float),
                ("visible", ctypes.c_void_p), ("radii", ctypes.c_void_p)]


class GsrDensifyInputs(ctypes.Structure):
    """gsr_densify_inputs: gsr_densify_stats' radii, dL_dmeans2D and the three accumulators."""
    _fields_ = [("P", ctypes.c_int64), ("radii", ctypes.c_void_p),
                ("dL_dmeans2D", ctypes.c_void_p), ("grad_accum", ctypes.c_void_p),
                ("denom", ctypes.c_void_p), ("max_radii", ctypes.c_void_p)]


# gsr_densify_group's `role` and gsr_densify_plan_inputs' `scale_space` (include/gsr.h)
GSR_ROLE_NONE, GSR_ROLE_XYZ, GSR_ROLE_SCALING, GSR_ROLE_ROTATION, GSR_ROLE_OPACITY = range(5)
GSR_SCALE_LINEAR, GSR_SCALE_LOG = 0, 1
SPLIT_CHILDREN = 2  # GSR_SPLIT_CHILDREN


class GsrDensifyGroup(ctypes.Structure):
    """gsr_densify_group: one [rows, M] tensor of gsr_densify_apply, with both moments or neither."""
    _fields_ = [("M", ctypes.c_int32), ("role", ctypes.c_int32), ("param", ctypes.c_void_p),
                ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p)]


class GsrDensifyPlanInputs(ctypes.Structure):
    """gsr_densify_plan_inputs: the statistics, the thresholds (in the tensors' stored space), the
    seed and the two tensors the classification reads; P_out and n_groups are the apply's."""
    _fields_ = [("P", ctypes.c_int64), ("P_out", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("n_groups", ctypes.c_int32), ("scale_space", ctypes.c_int32),
                ("grad_threshold", ctypes.c_float), ("scale_split_threshold", ctypes.c_float),
                ("opacity_prune_threshold", ctypes.c_float),
                ("scale_prune_threshold", ctypes.c_float),
                ("radius_prune_threshold", ctypes.c_int32),
                ("grad_accum", ctypes.c_void_p), ("denom", ctypes.c_void_p),
                ("max_radii", ctypes.c_void_p), ("scaling", ctypes.c_void_p),
                ("opacity", ctypes.c_void_p)]


class GsrPlyInfo(ctypes.Structure):
    _fields_ = [
        ("P", ctypes.c_int64), ("sh_coeffs", ctypes.c_int32), ("binary", ctypes.c_int32),
        ("bbox_min", ctypes.c_float * 3), ("bbox_max", ctypes.c_float * 3),
        ("center", ctypes.c_float * 3),
    ]


class GsrPlyScene(ctypes.Structure):
    """gsr_ply_scene: the raw tensors of a fit for gsr_ply_save / gsr_ply_load_scene."""
    _fields_ = [("P", ctypes.c_int64), ("sh_coeffs", ctypes.c_int32),
                ("file_sh_coeffs", ctypes.c_int32), ("chunk_rows", ctypes.c_int64),
                ("xyz", ctypes.c_void_p), ("f_dc", ctypes.c_void_p), ("f_rest", ctypes.c_void_p),
                ("opacity", ctypes.c_void_p), ("scaling", ctypes.c_void_p),
                ("rotation", ctypes.c_void_p)]


# The entries added to ABI 4 one by one: the structs between (ctx, gaussians, settings) and the
# stream.
_ADDITIVE = {
    "gsr_forward_depth": (GsrOutputs, GsrDepthOutputs),
    "gsr_forward_surface": (GsrOutputs, GsrDepthOutputs, GsrSurfaceOutputs),
    "gsr_forward_filtered": (GsrOutputs, GsrDepthOutputs, GsrSurfaceOutputs, GsrFilterSettings),
    "gsr_backward": (GsrBackwardInputs, GsrGradients),
    "gsr_backward_planes": (GsrBackwardInputs, GsrPlaneGradients, GsrGradients),
    "gsr_backward_camera": (GsrBackwardInputs, GsrPlaneGradients, GsrCameraGradients,
                            GsrGradients),
    "gsr_backward_filtered": (GsrBackwardInputs, GsrPlaneGradients, GsrCameraGradients,
                              GsrFilterSettings, GsrGradients),
    "gsr_backward_ordered": (GsrBackwardInputs, GsrPlaneGradients, GsrCameraGradients,
                             GsrFilterSettings, GsrBackwardOrder, GsrGradients),
    "gsr_backward_strip": (GsrBackwardInputs, GsrPlaneGradients, GsrCameraGradients,
                           GsrFilterSettings, GsrBackwardOrder, GsrGradients),
    "gsr_forward_features": (GsrOutputs, GsrDepthOutputs, GsrSurfaceOutputs, GsrFilterSettings,
                             GsrFeatureOutputs),
    "gsr_backward_features": (GsrBackwardInputs, GsrPlaneGradients, GsrCameraGradients,
                              GsrFilterSettings, GsrBackwardOrder, GsrFeatureGradients,
                              GsrGradients),
    "gsr_backward_abs": (GsrBackwardInputs, GsrPlaneGradients, GsrCameraGradients,
                         GsrFilterSettings, GsrBackwardOrder, GsrFeatureGradients,
                         GsrAbsGradients, GsrGradients),
}

_lock = threading.Lock()
_lib = None
_contexts: dict[int, ctypes.c_void_p] = {}


def _declare(lib: ctypes.CDLL) -> None:
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.gsr_abi_version.restype = i32
    lib.gsr_last_error.restype = ctypes.c_char_p
    lib.gsr_create.argtypes = [ctypes.POINTER(vp)]
    lib.gsr_destroy.argtypes = [vp]
    lib.gsr_destroy.restype = None
    lib.gsr_reserve.argtypes = [vp, i64, i64]
    lib.gsr_forward.argtypes = [vp, ctypes.POINTER(GsrGaussians),
                                ctypes.POINTER(GsrRasterSettings), ctypes.POINTER(GsrOutputs), vp]
    lib.gsr_forward_shaded.argtypes = [vp, ctypes.POINTER(GsrGaussians),
                                       ctypes.POINTER(GsrRasterSettings),
                                       ctypes.POINTER(GsrOutputs), ctypes.c_int32, vp]
    # the additive entries (an older build of ABI 4 loaded through GSR_LIB lacks some: the
    # accessors below say so): (ctx, gaussians, settings), the table's structs, the stream
    for name, structs in _ADDITIVE.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = [vp, ctypes.POINTER(GsrGaussians), ctypes.POINTER(GsrRasterSettings),
                           *(ctypes.POINTER(t) for t in structs), vp]
            fn.restype = i32
    if hasattr(lib, "gsr_image_loss"):
        loss_in = ctypes.POINTER(GsrImageLossInputs)
        lib.gsr_image_loss_workspace.argtypes = [ctypes.c_int32] * 3
        lib.gsr_image_loss_workspace.restype = i64
        lib.gsr_image_loss.argtypes = [loss_in, vp, vp, vp, vp]
        lib.gsr_image_loss.restype = i32
        lib.gsr_image_loss_backward.argtypes = [loss_in, vp, vp, vp, vp]
        lib.gsr_image_loss_backward.restype = i32
    if hasattr(lib, "gsr_image_loss_window"):
        loss_in, win = ctypes.POINTER(GsrImageLossInputs), ctypes.POINTER(GsrLossWindow)
        lib.gsr_image_loss_window_workspace.argtypes = [loss_in, win]
        lib.gsr_image_loss_window_workspace.restype = i64
        lib.gsr_image_loss_window.argtypes = [loss_in, win, vp, vp, vp, vp]
        lib.gsr_image_loss_window.restype = i32
        lib.gsr_image_loss_window_backward.argtypes = [loss_in, win, vp, vp, vp, vp]
        lib.gsr_image_loss_window_backward.restype = i32
    if hasattr(lib, "gsr_adam_step"):
        lib.gsr_adam_step.argtypes = [ctypes.POINTER(GsrAdamSettings),
                                      ctypes.POINTER(GsrParamGroup), vp]
        lib.gsr_adam_step.restype = i32
        lib.gsr_densify_stats.argtypes = [ctypes.POINTER(GsrDensifyInputs), vp]
        lib.gsr_densify_stats.restype = i32
    if hasattr(lib, "gsr_densify_plan"):
        plan_in = ctypes.POINTER(GsrDensifyPlanInputs)
        lib.gsr_densify_workspace.argtypes = [i64]
        lib.gsr_densify_workspace.restype = i64
        lib.gsr_densify_plan.argtypes = [plan_in, vp, vp, vp]
        lib.gsr_densify_plan.restype = i32
        lib.gsr_densify_apply.argtypes = [plan_in, ctypes.POINTER(GsrDensifyGroup),
                                          ctypes.POINTER(GsrDensifyGroup), vp, vp, vp]
        lib.gsr_densify_apply.restype = i32
    if hasattr(lib, "gsr_knn_mean_dist2"):
        lib.gsr_knn_workspace.argtypes = [i64]
        lib.gsr_knn_workspace.restype = i64
        lib.gsr_knn_mean_dist2.argtypes = [vp, i64, vp, vp, vp]
        lib.gsr_knn_mean_dist2.restype = i32
        lib.gsr_knn_stages.argtypes = [vp, i64, vp, vp, ctypes.c_int32, vp]
        lib.gsr_knn_stages.restype = i32
    if hasattr(lib, "gsr_ply_save"):
        ply_scene = ctypes.POINTER(GsrPlyScene)
        lib.gsr_ply_save.argtypes = [ctypes.c_char_p, ply_scene, i32, vp]
        lib.gsr_ply_probe_scene.argtypes = [ctypes.c_char_p, ply_scene]
        lib.gsr_ply_load_scene.argtypes = [ctypes.c_char_p, ply_scene, i32, vp]
        for name in ("gsr_ply_save", "gsr_ply_probe_scene", "gsr_ply_load_scene"):
            getattr(lib, name).restype = i32
    if hasattr(lib, "gsr_backward"):
        lib.gsr_backward_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), i32]
        lib.gsr_backward_times.restype = i32
    lib.gsr_get_binning.argtypes = [vp, vp, vp, vp, ctypes.POINTER(i64),
                                    ctypes.POINTER(ctypes.c_int32), vp]
    lib.gsr_mark_visible.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.gsr_tile_row_pairs.argtypes = [vp, vp, i32, vp]
    lib.gsr_depth_argsort.argtypes = [vp, vp, i64, ctypes.POINTER(ctypes.c_float), vp, vp, vp]
    lib.gsr_set_timing.argtypes = [vp, i32]
    lib.gsr_stage_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), i32]
    lib.gsr_stage_name.argtypes = [i32]
    lib.gsr_stage_name.restype = ctypes.c_char_p
    lib.gsr_set_option.argtypes = [vp, i32, i64]
    lib.gsr_get_option.argtypes = [vp, i32, ctypes.POINTER(i64)]
    lib.gsr_frame_graph_stats.argtypes = [vp, ctypes.POINTER(i64), i32]
    lib.gsr_ply_probe.argtypes = [ctypes.c_char_p, ctypes.POINTER(GsrPlyInfo)]
    lib.gsr_ply_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(GsrPlyInfo), vp, vp, vp, vp, vp,
                                 i32, vp]
    lib.gsr_disparity_colors.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_float),
                                         ctypes.POINTER(ctypes.c_float), ctypes.c_float, vp, vp]
    lib.gsr_pack_image.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_int32, vp, vp]
    for name in ("gsr_disparity_colors", "gsr_pack_image", "gsr_create", "gsr_reserve", "gsr_forward", "gsr_get_binning",
                 "gsr_mark_visible", "gsr_depth_argsort", "gsr_set_timing", "gsr_tile_row_pairs",
                 "gsr_stage_times", "gsr_set_option", "gsr_get_option", "gsr_ply_probe", "gsr_ply_load",
                 "gsr_frame_graph_stats", "gsr_forward_shaded"):
        getattr(lib, name).restype = i32


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load (once) and return libgsr.so; raise RuntimeError if it is absent or stale."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(
                f"libgsr.so not found at {path}: the HIP rasterizer is not built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C gaussiansplattingviewer_amd/csrc`). There is no CPU fallback.")
        lib = ctypes.CDLL(path)
        _declare(lib)
        ver = lib.gsr_abi_version()
        if ver != ABI_VERSION:
            raise RuntimeError(f"libgsr.so ABI version {ver} != expected {ABI_VERSION}")
        _lib = lib
        return lib


def _optional_fn(lib, name: str, needs: str):
    """An additive entry (or a tuple of them, `name` joined by " / ") of a loaded library;
    RuntimeError if that build does not have it."""
    names = name.split(" / ")
    fns = tuple(getattr(lib, n, None) for n in names)
    if None in fns:
        one = len(names) == 1
        raise RuntimeError(
            f"{LIB_PATH} has no {name}: {needs} a libgsr.so built from this tree (include/gsr.h "
            f"declares {'it' if one else 'them'}; ABI 4, additive)")
    return fns[0] if len(fns) == 1 else fns


def forward_depth_fn(lib: ctypes.CDLL):
    """gsr_forward_depth of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_forward_depth", "the depth_map / inv_depth_map outputs need")


def forward_surface_fn(lib: ctypes.CDLL):
    """gsr_forward_surface of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_forward_surface", "the median_depth / median_id outputs need")


def backward_fn(lib: ctypes.CDLL):
    """gsr_backward of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_backward", "gradients need")


def backward_planes_fn(lib: ctypes.CDLL):
    """gsr_backward_planes of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_backward_planes",
                        "gradients of depth_map / inv_depth_map / final_T need")


def backward_camera_fn(lib: ctypes.CDLL):
    """gsr_backward_camera of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_backward_camera",
                        "gradients of viewmatrix / projmatrix / campos need")


def filtered_fns(lib: ctypes.CDLL):
    """(gsr_forward_filtered, gsr_backward_filtered) of a loaded library; RuntimeError if that
    build does not have them."""
    return _optional_fn(lib, "gsr_forward_filtered / gsr_backward_filtered", "antialiasing needs")


def backward_ordered_fn(lib: ctypes.CDLL):
    """gsr_backward_ordered of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_backward_ordered", "a deterministic backward needs")


def backward_strip_fn(lib: ctypes.CDLL):
    """gsr_backward_strip of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_backward_strip", "a backward on a tile row strip needs")


def features_fns(lib: ctypes.CDLL):
    """(gsr_forward_features, gsr_backward_features) of a loaded library; RuntimeError if that
    build does not have them."""
    return _optional_fn(lib, "gsr_forward_features / gsr_backward_features",
                        "per-Gaussian feature channels need")


def backward_abs_fn(lib: ctypes.CDLL):
    """gsr_backward_abs of a loaded library; RuntimeError if that build does not have it."""
    return _optional_fn(lib, "gsr_backward_abs", "the absolute means2D gradient needs")


def image_loss_fns(lib: ctypes.CDLL):
    """(gsr_image_loss_workspace, gsr_image_loss, gsr_image_loss_backward) of a loaded library;
    RuntimeError if that build does not have them."""
    return _optional_fn(lib, "gsr_image_loss_workspace / gsr_image_loss / "
                        "gsr_image_loss_backward", "the fused image loss needs")


def image_loss_window_fns(lib: ctypes.CDLL):
    """(gsr_image_loss_window_workspace, gsr_image_loss_window, gsr_image_loss_window_backward) of
    a loaded library; RuntimeError if that build does not have them."""
    return _optional_fn(lib, "gsr_image_loss_window_workspace / gsr_image_loss_window / "
                        "gsr_image_loss_window_backward", "the frame's loss on a strip needs")


def optimizer_fns(lib: ctypes.CDLL):
    """(gsr_adam_step, gsr_densify_stats) of a loaded library; RuntimeError if that build does
    not have them."""
    return _optional_fn(lib, "gsr_adam_step / gsr_densify_stats",
                        "the fused Adam step and the densification statistics need")


def densify_fns(lib: ctypes.CDLL):
    """(gsr_densify_workspace, gsr_densify_plan, gsr_densify_apply) of a loaded library;
    RuntimeError if that build does not have them."""
    return _optional_fn(lib, "gsr_densify_workspace / gsr_densify_plan / gsr_densify_apply",
                        "densify-and-prune needs")


def knn_fns(lib: ctypes.CDLL):
    """(gsr_knn_workspace, gsr_knn_mean_dist2, gsr_knn_stages) of a loaded library; RuntimeError
    if that build does not have them."""
    return _optional_fn(lib, " / ".join(KNN_SYMBOLS), "the nearest-neighbour search needs")


def ply_scene_fns(lib: ctypes.CDLL):
    """(gsr_ply_save, gsr_ply_probe_scene, gsr_ply_load_scene) of a loaded library; RuntimeError
    if that build does not have them."""
    return _optional_fn(lib, "gsr_ply_save / gsr_ply_probe_scene / gsr_ply_load_scene",
                        "saving and loading a raw scene needs")


def check(rc: int, what: str) -> int:
    if rc < 0:
        msg = load_library().gsr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")
    return rc


@functools.lru_cache(maxsize=None)
def _native_shares_library() -> bool:
    """The `_native` extension links the in-tree libgsr.so; contexts are shared with it only
    when this module loaded that same file (not a GSR_LIB A/B build).  LIB_PATH is fixed at
    import, so the answer is computed once (the forward asks on every frame)."""
    default = os.path.join(_HERE, "libgsr.so")
    return (os.path.exists(LIB_PATH) and os.path.exists(default) and
            os.path.samefile(LIB_PATH, default))


def context(device_index: int, slot: int = 0) -> ctypes.c_void_p:
    """The process-wide gsr_context of a device (created on first use, on that device).

    `slot` selects one of several independent contexts per device (own workspace, own
    second stream): frames rendered through different slots on different streams may be in
    flight at the same time (`pipeline.FramePipeline`).  Slot 0 is the context the `_C`
    extension (`_native.so`) renders with, so the upstream entry points and this module share
    one workspace and `binning_state()` sees a `GaussianRasterizer` forward (its tight lists
    unless GSR_OPT_TIGHT_BINNING is 0).  Under GSR_LIB (an A/B build) slot 0 is a context of
    that build, and `GaussianRasterizer` renders through it by ctypes instead of `_C`."""
    import torch

    lib = load_library()
    key = (int(device_index), int(slot))
    with _lock:
        ctx = _contexts.get(key)
        if ctx is not None:
            return ctx
        if not torch.cuda.is_available():
            raise RuntimeError("gaussiansplattingviewer_amd needs a HIP device (MI355X); "
                               "torch.cuda.is_available() is False")
        if key[1] == 0 and _native_shares_library():
            from . import _native  # owns (creates and destroys) the slot-0 contexts
            ctx = ctypes.c_void_p(_native.context_handle(key[0]))
        else:
            with torch.cuda.device(device_index):
                ctx = ctypes.c_void_p()
                check(lib.gsr_create(ctypes.byref(ctx)), "gsr_create")
        _contexts[key] = ctx
        return ctx


def release_contexts() -> None:
    """Destroy every gsr_context (registered with atexit; a diagnostics build reports its
    counters from gsr_destroy); slot 0's belong to `_native`."""
    with _lock:
        lib = _lib
        if lib is None or not _contexts:
            return
        native = _native_shares_library() and any(slot == 0 for _, slot in _contexts)
        for (_, slot), ctx in _contexts.items():
            if slot != 0 or not native:
                lib.gsr_destroy(ctx)
        _contexts.clear()
        if native:
            from . import _native
            _native.release_contexts()


atexit.register(release_contexts)


def frame_graph_stats(device_index: int = 0, slot: int = 0) -> dict:
    """Frame-graph counters of a context slot (gsr_frame_graph_stats)."""
    lib = load_library()
    v = (ctypes.c_int64 * 4)()
    check(lib.gsr_frame_graph_stats(context(device_index, slot), v, 4), "gsr_frame_graph_stats")
    return {"graph_frames": v[0], "graphs_recorded": v[1], "overflows": v[2], "list_cap": v[3]}


def get_option(ctx, option: int) -> int:
    """The current value of a context option (gsr_get_option)."""
    v = ctypes.c_int64()
    check(load_library().gsr_get_option(ctx, option, ctypes.byref(v)), "gsr_get_option")
    return int(v.value)


def set_option(ctx, option: int, value: int) -> None:
    check(load_library().gsr_set_option(ctx, option, int(value)), "gsr_set_option")


def stage_names() -> list[str]:
    lib = load_library()
    names = []
    i = 0
    while True:
        n = lib.gsr_stage_name(i).decode()
        if not n:
            return names
        names.append(n)
        i += 1


def ptr(t) -> int | None:
    """Device pointer of a tensor (None for an absent / empty optional tensor)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()
