"""ctypes binding of ``libcanny_hip.so`` (C ABI in ``include/canny_hip.h``).

Two layers:

* :class:`Context` -- one GPU + one stream; methods take numpy arrays (host API) or raw device
  pointers as ints (``dev_*`` API, asynchronous on the context's stream).
* module-level functions named exactly like the reference's stage functions
  (``src/utils.h:8-22``: ``gaussian``, ``createGaussianKernel``, ``calculateXYGradient``,
  ``sobelOperator``, ``nonmaximalSuppression``, ``hysteresis``, ``findEdgePixels``, ``canny``) so that
  parity tests read like the reference's own tests.  They return new arrays instead of writing through
  reference-to-pointer out-parameters.

There is no CPU fallback anywhere in this module: if the shared library is missing, or no HIP device
is present, the call raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import threading
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CANNY_HIP_LIB: another build of the same library (A/B measurements of kernel variants, tools/ab_stage_times.py)
LIB_PATH = os.environ.get("CANNY_HIP_LIB") or os.path.join(_HERE, "libcanny_hip.so")

OK = 0
STAGE_GAUSSIAN, STAGE_SOBEL_NMS, STAGE_HYST_CLASSIFY, STAGE_HYST_PROPAGATE, STAGE_HYST_FINALIZE, \
    STAGE_SOBEL, STAGE_NMS, STAGE_XY_GRADIENT, STAGE_TO_GRAY = range(9)
STAGE_NAMES = ("gaussian", "sobel_nms", "hyst_classify", "hyst_propagate", "hyst_finalize", "sobel", "nms",
               "xy_gradient", "to_gray")
# stage of what is derived from a finished map (CANNY_HIP_STAGE_COMPACT; not one of the CANNY_HIP_STAGE_COUNT stages above)
STAGE_COMPACT = 9

# colour frame layouts (enum canny_hip_layout): interleaved, 1 byte per channel, no row padding
LAYOUT_GRAY8, LAYOUT_BGR8, LAYOUT_RGB8, LAYOUT_BGRA8, LAYOUT_RGBA8 = range(5)
LAYOUT_CHANNELS = {LAYOUT_GRAY8: 1, LAYOUT_BGR8: 3, LAYOUT_RGB8: 3, LAYOUT_BGRA8: 4, LAYOUT_RGBA8: 4}


def layout_of(shape, order: str = "bgr", batch: bool = False) -> int:
    """Layout of a frame of this shape: (H, W) -> GRAY8, (H, W, 3) -> BGR8 / RGB8, (H, W, 4) -> BGRA8 / RGBA8 by
    ``order`` ("bgr": cv::Mat / VideoCapture, "rgb": PIL / PPM / numpy).  batch=True: the same with a leading frame
    axis, (N, H, W[, CH]).  Pure host logic."""
    shape = tuple(int(d) for d in shape)
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order must be 'bgr' or 'rgb', not {order!r}")
    nd = len(shape) - (1 if batch else 0)
    if nd == 2:
        return LAYOUT_GRAY8
    if nd == 3 and shape[-1] in (3, 4):
        if shape[-1] == 3:
            return LAYOUT_BGR8 if order == "bgr" else LAYOUT_RGB8
        return LAYOUT_BGRA8 if order == "bgr" else LAYOUT_RGBA8
    raise ValueError(f"expected {'(N, ' if batch else '('}H, W) or {'(N, ' if batch else '('}H, W, 3|4) frames, "
                     f"got shape {shape}")

# automatic per-frame threshold rules (enum canny_hip_auto_rule)
AUTO_MEDIAN, AUTO_QUANTILE = 1, 2
# Context.selftest_sobel_pixel forms (enum canny_hip_pixel_form)
PIXEL_LDS_TILE, PIXEL_PACKED_I16, PIXEL_F32, PIXEL_F32_FLOOR = 0, 1, 2, 3
# Context.selftest_workspaces kinds (enum canny_hip_workspace_kind)
WS_DATA, WS_INDEX, WS_CACHE = 0, 1, 2
# launch_plan kinds (enum canny_hip_launch_plan_kind)
PLAN_KINDS = ("points_rows", "scan_frames", "cc_tiles", "cc_rows", "cc_fixup", "ct_rows", "edt_rows", "edt_columns",
              "pg_records", "pg_scan_sums", "hough_vote_strong", "hough_vote_bits", "hough_vote_points", "hough_cells",
              "circles_vote_strong", "circles_vote_bits", "circles_steps", "to_gray")
_AUTO_RULES = {"median": AUTO_MEDIAN, "quantile": AUTO_QUANTILE, AUTO_MEDIAN: AUTO_MEDIAN, AUTO_QUANTILE: AUTO_QUANTILE}


def _rule(rule) -> int:
    if rule not in _AUTO_RULES:
        raise ValueError(f"rule must be 'median', 'quantile', AUTO_MEDIAN or AUTO_QUANTILE, not {rule!r}")
    return _AUTO_RULES[rule]


# every symbol include/canny_hip.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "canny_hip_version", "canny_hip_status_string", "canny_hip_device_count", "canny_hip_ctx_create",
    "canny_hip_ctx_destroy", "canny_hip_ctx_set_stream", "canny_hip_ctx_device", "canny_hip_ctx_set_option", "canny_hip_synchronize",
    "canny_hip_last_error", "canny_hip_last_hysteresis_iterations", "canny_hip_malloc", "canny_hip_free",
    "canny_hip_host_alloc", "canny_hip_host_free", "canny_hip_memcpy_h2d", "canny_hip_memcpy_d2h",
    "canny_hip_gaussian_kernel", "canny_hip_gaussian", "canny_hip_xy_gradient", "canny_hip_sobel", "canny_hip_nms",
    "canny_hip_hysteresis", "canny_hip_find_edge_pixels", "canny_hip_canny", "canny_hip_canny_batch",
    "canny_hip_canny_batch_u8", "canny_hip_dev_canny_u8", "canny_hip_canny_multi_gpu", "canny_hip_shard_range", "canny_hip_dev_gaussian", "canny_hip_dev_xy_gradient",
    "canny_hip_dev_sobel", "canny_hip_dev_nms", "canny_hip_dev_sobel_nms", "canny_hip_dev_hysteresis",
    "canny_hip_dev_canny", "canny_hip_dev_canny_stream", "canny_hip_dev_canny_stream_flush", "canny_hip_profile_enable", "canny_hip_profile_reset", "canny_hip_profile_get",
    "canny_hip_selftest_mag_angle", "canny_hip_selftest_sobel_pixel", "canny_hip_selftest_div", "canny_hip_selftest_div_fma",
    "canny_hip_selftest_div_fma_table", "canny_hip_canny_multi_gpu_u8", "canny_hip_multi_gpu_set_option",
    "canny_hip_multi_gpu_release", "canny_hip_device_local_cpus", "canny_hip_selftest_cpulist_count",
    "canny_hip_dev_gaussian_u8", "canny_hip_dev_sobel_nms_u8in", "canny_hip_host_register", "canny_hip_host_unregister",
    "canny_hip_canny_batch_bits", "canny_hip_canny_multi_gpu_bits", "canny_hip_dev_canny_bits",
    "canny_hip_probe_copy", "canny_hip_ctx_get_option", "canny_hip_selftest_expand_bits",
    "canny_hip_selftest_march_order", "canny_hip_to_gray", "canny_hip_dev_to_gray", "canny_hip_dev_gaussian_u8_color",
    "canny_hip_dev_canny_color", "canny_hip_canny_color", "canny_hip_canny_batch_color", "canny_hip_canny_batch_color_u8",
    "canny_hip_canny_batch_color_bits", "canny_hip_auto_thresholds_from_histogram", "canny_hip_dev_canny_thresholds",
    "canny_hip_dev_canny_auto", "canny_hip_canny_batch_thresholds", "canny_hip_canny_batch_auto",
    "canny_hip_dev_canny_points", "canny_hip_dev_points_from_bits", "canny_hip_canny_points",
    "canny_hip_points_from_bits",
    "canny_hip_hough_geometry", "canny_hip_hough_tables", "canny_hip_hough_line_of", "canny_hip_dev_hough_points",
    "canny_hip_dev_hough_bits", "canny_hip_dev_canny_hough", "canny_hip_canny_hough", "canny_hip_hough_profile_get",
    "canny_hip_dev_canny_components", "canny_hip_dev_components_bits", "canny_hip_canny_components",
    "canny_hip_components_from_bits", "canny_hip_components_profile_get",
    "canny_hip_dev_canny_contours", "canny_hip_dev_contours_bits", "canny_hip_canny_contours",
    "canny_hip_contours_from_bits", "canny_hip_contours_profile_get",
    "canny_hip_dev_canny_edt", "canny_hip_dev_edt_bits", "canny_hip_canny_edt", "canny_hip_edt_from_bits",
    "canny_hip_edt_profile_get",
    "canny_hip_hough_segments_from_bits", "canny_hip_dev_hough_segments_bits", "canny_hip_dev_canny_hough_segments",
    "canny_hip_canny_hough_segments", "canny_hip_hough_segments_profile_get",
    "canny_hip_selftest_histogram", "canny_hip_selftest_select", "canny_hip_selftest_workspace",
    "canny_hip_selftest_launch_plan",
    "canny_hip_hough_circles_step_of", "canny_hip_hough_circles_from_bits", "canny_hip_dev_hough_circles_bits",
    "canny_hip_dev_canny_hough_circles", "canny_hip_canny_hough_circles", "canny_hip_dev_hough_circles_steps",
    "canny_hip_hough_circles_profile_get",
    "canny_hip_dev_polygons_chains", "canny_hip_dev_canny_polygons", "canny_hip_dev_polygons_bits",
    "canny_hip_canny_polygons", "canny_hip_polygons_from_chains", "canny_hip_polygons_profile_get",
    "canny_hip_dev_canny_edgels", "canny_hip_dev_edgels_at", "canny_hip_canny_edgels", "canny_hip_edgels_from_plane",
    "canny_hip_dev_edgels_arith", "canny_hip_edgels_profile_get", "canny_hip_selftest_edgels_plan",
    "canny_hip_line_fits_from_plane", "canny_hip_dev_line_fits_bits", "canny_hip_dev_canny_hough_line_fits",
    "canny_hip_canny_hough_line_fits", "canny_hip_dev_line_fits_arith", "canny_hip_line_fits_profile_get",
    "canny_hip_line_fits_finish",
    "canny_hip_circle_fits_from_plane", "canny_hip_dev_circle_fits_bits", "canny_hip_dev_canny_hough_circle_fits",
    "canny_hip_canny_hough_circle_fits", "canny_hip_dev_circle_fits_arith", "canny_hip_circle_fits_finish",
    "canny_hip_circle_fits_profile_get", "canny_hip_circle_fits_queue_capacity",
    "canny_hip_chamfer_set_create", "canny_hip_chamfer_set_destroy", "canny_hip_dev_chamfer_dist2",
    "canny_hip_dev_chamfer_bits", "canny_hip_dev_canny_chamfer", "canny_hip_canny_chamfer", "canny_hip_chamfer_from_dist2",
    "canny_hip_chamfer_cost_of", "canny_hip_dev_chamfer_costs", "canny_hip_chamfer_profile_get",
    "canny_hip_selftest_chamfer_plan", "canny_hip_selftest_chamfer_bands",
    "canny_hip_dev_shapes_chains", "canny_hip_dev_canny_shapes", "canny_hip_dev_shapes_bits", "canny_hip_canny_shapes",
    "canny_hip_shapes_from_chains", "canny_hip_shapes_profile_get", "canny_hip_selftest_shapes_plan",
    "canny_hip_dev_canny_curves", "canny_hip_dev_curves_bits", "canny_hip_canny_curves", "canny_hip_curves_from_bits",
    "canny_hip_curves_profile_get", "canny_hip_selftest_curves_plan",
    "canny_hip_dev_canny_corners", "canny_hip_dev_corners_plane", "canny_hip_canny_corners",
    "canny_hip_corners_from_plane", "canny_hip_corner_response_of", "canny_hip_dev_corners_arith",
    "canny_hip_corners_profile_get", "canny_hip_selftest_corners_plan",
    "canny_hip_dev_canny_corner_descriptors", "canny_hip_dev_corner_descriptors", "canny_hip_canny_corner_descriptors",
    "canny_hip_corner_descriptors_from_plane", "canny_hip_descriptor_pattern", "canny_hip_dev_match_descriptors",
    "canny_hip_match_descriptors", "canny_hip_descriptors_profile_get", "canny_hip_selftest_descriptors_plan",
    "canny_hip_dev_estimate_motion", "canny_hip_estimate_motion", "canny_hip_canny_motion", "canny_hip_motion_profile_get",
    "canny_hip_selftest_motion_plan",
    "canny_hip_dev_compose_motion", "canny_hip_compose_motion", "canny_hip_dev_warp_frames", "canny_hip_warp_frames",
    "canny_hip_canny_align", "canny_hip_warp_profile_get", "canny_hip_selftest_warp_plan",
    "canny_hip_dev_fuse_frames", "canny_hip_fuse_frames", "canny_hip_dev_change_mask", "canny_hip_change_mask",
    "canny_hip_canny_background", "canny_hip_fuse_profile_get", "canny_hip_selftest_fuse_plan",
    "canny_hip_selftest_fuse_mean",
    "canny_hip_dev_morph_bits", "canny_hip_dev_canny_morph", "canny_hip_canny_morph", "canny_hip_morph_bits",
    "canny_hip_morph_element", "canny_hip_selftest_morph_plan", "canny_hip_morph_profile_get",
    "canny_hip_dev_binarize", "canny_hip_binarize_batch", "canny_hip_binarize", "canny_hip_otsu_from_histogram",
    "canny_hip_selftest_binarize_plan", "canny_hip_profile_part_get",
    "canny_hip_dev_thin_bits", "canny_hip_dev_canny_thin", "canny_hip_thin_batch", "canny_hip_thin_bits",
    "canny_hip_selftest_thin_plan",
    "canny_hip_dev_reconstruct_bits", "canny_hip_dev_canny_reconstruct", "canny_hip_reconstruct_batch",
    "canny_hip_reconstruct_bits", "canny_hip_selftest_reconstruct_plan",
    "canny_hip_dev_gray_morph", "canny_hip_gray_morph_batch", "canny_hip_gray_morph", "canny_hip_selftest_gray_morph_plan",
    "canny_hip_pyramid_layout", "canny_hip_dev_pyr_down", "canny_hip_dev_pyramid", "canny_hip_dev_pyr_up",
    "canny_hip_pyramid_batch", "canny_hip_pyr_up_batch", "canny_hip_pyramid", "canny_hip_pyr_up", "canny_hip_selftest_pyramid_plan",
)

_lib: Optional[C.CDLL] = None


class CannyHipError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        self.status = status
        msg = f"{what}: {status_string(status)}"
        if detail:
            msg += f" ({detail})"
        super().__init__(msg)


def _ok(st: int, what: str):
    """Raise for a non-zero status of a call that has no context to ask for details."""
    if st:
        raise CannyHipError(st, what)


def _plan(name: str, *args, n: int = 5, tail=()):
    """canny_hip_selftest_<name>(*args, out, *tail) on a zeroed uint64 [n]: the LaunchPlan of its first five words and, with
    n > 5, the words behind them."""
    out = np.zeros(n, np.uint64)
    _ok(getattr(load(), "canny_hip_selftest_" + name)(*args, _hp(out), *tail), "selftest_" + name)
    plan = LaunchPlan(*(int(v) for v in out[:5]))
    return plan if n == 5 else (plan, *(int(v) for v in out[5:]))


def load() -> C.CDLL:
    """Load the HIP library; fail loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C canny_edge_amd/csrc`); there is no CPU fallback")
    # The batch pipeline's upload / compute / download streams want hardware queues of their own; HIP reads the variable
    # when its runtime initialises.  This module is host-application code (the library never touches the environment).
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    L = C.CDLL(LIB_PATH)
    i, f, p, sz = C.c_int, C.c_float, C.c_void_p, C.c_size_t
    pp, ip = C.POINTER(C.c_void_p), C.POINTER(C.c_int)
    ull = C.c_ulonglong
    sig = {
        "canny_hip_version": ([], i),
        "canny_hip_status_string": ([i], C.c_char_p),
        "canny_hip_device_count": ([ip], i),
        "canny_hip_ctx_create": ([pp, i], i),
        "canny_hip_ctx_destroy": ([p], None),
        "canny_hip_ctx_set_stream": ([p, p], i),
        "canny_hip_ctx_device": ([p], i),
        "canny_hip_ctx_set_option": ([p, C.c_char_p, i], i),
        "canny_hip_synchronize": ([p], i),
        "canny_hip_last_error": ([p], C.c_char_p),
        "canny_hip_last_hysteresis_iterations": ([p], i),
        "canny_hip_malloc": ([p, pp, sz], i),
        "canny_hip_free": ([p, p], i),
        "canny_hip_host_alloc": ([p, pp, sz], i),
        "canny_hip_host_free": ([p, p], i),
        "canny_hip_host_register": ([p, p, sz], i),
        "canny_hip_host_unregister": ([p, p], i),
        "canny_hip_memcpy_h2d": ([p, p, p, sz], i),
        "canny_hip_memcpy_d2h": ([p, p, p, sz], i),
        "canny_hip_gaussian_kernel": ([f, p, i, ip], i),
        "canny_hip_gaussian": ([p, p, f, i, i, p], i),
        "canny_hip_xy_gradient": ([p, p, i, i, p, p], i),
        "canny_hip_sobel": ([p, p, i, i, p, p], i),
        "canny_hip_nms": ([p, p, p, i, i, p], i),
        "canny_hip_hysteresis": ([p, p, i, i, i, i], i),
        "canny_hip_find_edge_pixels": ([p, p, p, i, i, i, i, i], i),
        "canny_hip_canny": ([p, p, f, i, i, i, i, p], i),
        "canny_hip_canny_batch": ([p, p, i, f, i, i, i, i, p], i),
        "canny_hip_canny_batch_u8": ([p, p, i, f, i, i, i, i, p], i),
        "canny_hip_dev_canny_u8": ([p, p, f, i, i, i, i, i, p], i),
        "canny_hip_dev_canny_bits": ([p, p, f, i, i, i, i, i, p], i),
        "canny_hip_canny_batch_bits": ([p, p, i, f, i, i, i, i, p], i),
        "canny_hip_canny_multi_gpu_bits": ([p, i, f, i, i, i, i, p, i], i),
        "canny_hip_canny_multi_gpu": ([p, i, f, i, i, i, i, p, i], i),
        "canny_hip_canny_multi_gpu_u8": ([p, i, f, i, i, i, i, p, i], i),
        "canny_hip_multi_gpu_set_option": ([C.c_char_p, i], i),
        "canny_hip_multi_gpu_release": ([], i),
        "canny_hip_device_local_cpus": ([i, C.c_char_p, i], i),
        "canny_hip_selftest_cpulist_count": ([C.c_char_p], i),
        "canny_hip_shard_range": ([i, i, i, ip, ip], i),
        "canny_hip_dev_gaussian": ([p, p, f, i, i, i, p], i),
        "canny_hip_dev_xy_gradient": ([p, p, i, i, i, p, p], i),
        "canny_hip_dev_sobel": ([p, p, i, i, i, p, p], i),
        "canny_hip_dev_nms": ([p, p, p, i, i, i, p], i),
        "canny_hip_dev_sobel_nms": ([p, p, i, i, i, p], i),
        "canny_hip_dev_hysteresis": ([p, p, i, i, i, i, i], i),
        "canny_hip_dev_gaussian_u8": ([p, p, f, i, i, i, p], i),
        "canny_hip_dev_sobel_nms_u8in": ([p, p, i, i, i, p], i),
        "canny_hip_dev_canny": ([p, p, f, i, i, i, i, i, p], i),
        "canny_hip_dev_canny_stream": ([p, p, f, i, i, i, i, i, p], i),
        "canny_hip_dev_canny_stream_flush": ([p], i),
        "canny_hip_profile_enable": ([p, i], i),
        "canny_hip_profile_reset": ([p], i),
        "canny_hip_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_probe_copy": ([p, p, p, C.c_size_t, i, C.POINTER(C.c_double)], i),
        "canny_hip_ctx_get_option": ([p, C.c_char_p, ip], i),
        "canny_hip_selftest_expand_bits": ([p, i, i, i, p, i], i),
        "canny_hip_selftest_march_order": ([i, i, p], i),
        "canny_hip_selftest_mag_angle": ([p, i, p, p], i),
        "canny_hip_selftest_sobel_pixel": ([p, i, i, p, p], i),
        "canny_hip_selftest_div": ([p, f, C.POINTER(C.c_ulonglong), C.POINTER(C.c_float)], i),
        "canny_hip_selftest_div_fma": ([p, f, f, C.POINTER(C.c_ulonglong), C.POINTER(C.c_float)], i),
        "canny_hip_selftest_div_fma_table": ([i, C.POINTER(C.c_float), C.POINTER(C.c_float)], i),
        "canny_hip_to_gray": ([p, p, i, i, i, p], i),
        "canny_hip_dev_to_gray": ([p, p, i, i, i, i, p], i),
        "canny_hip_dev_gaussian_u8_color": ([p, p, i, f, i, i, i, p], i),
        "canny_hip_dev_canny_color": ([p, p, i, f, i, i, i, i, i, p], i),
        "canny_hip_canny_color": ([p, p, i, f, i, i, i, i, p], i),
        "canny_hip_canny_batch_color": ([p, p, i, i, f, i, i, i, i, p], i),
        "canny_hip_canny_batch_color_u8": ([p, p, i, i, f, i, i, i, i, p], i),
        "canny_hip_canny_batch_color_bits": ([p, p, i, i, f, i, i, i, i, p], i),
        "canny_hip_auto_thresholds_from_histogram": ([p, i, f, f, ip, ip], i),
        "canny_hip_dev_canny_thresholds": ([p, p, f, p, i, i, i, p], i),
        "canny_hip_dev_canny_auto": ([p, p, f, i, f, f, i, i, i, p, p], i),
        "canny_hip_canny_batch_thresholds": ([p, p, i, f, p, i, i, p], i),
        "canny_hip_canny_batch_auto": ([p, p, i, f, i, f, f, i, i, p, p], i),
        "canny_hip_dev_canny_points": ([p, p, f, i, i, i, i, i, p, p, C.c_ulonglong, p], i),
        "canny_hip_dev_points_from_bits": ([p, p, i, i, i, p, C.c_ulonglong, p], i),
        "canny_hip_canny_points": ([p, p, i, f, i, i, i, i, p, C.c_ulonglong, p], i),
        "canny_hip_points_from_bits": ([p, i, i, p, C.c_ulonglong, C.POINTER(C.c_ulonglong)], i),
        "canny_hip_hough_geometry": ([i, i, f, f, f, f, ip, ip], i),
        "canny_hip_hough_tables": ([f, f, f, i, p, p], i),
        "canny_hip_hough_line_of": ([C.c_uint, i, f, f, f, C.POINTER(f), C.POINTER(f)], i),
        "canny_hip_dev_hough_points": ([p, p, p, i, i, i, f, f, i, i, f, f, p, p, p, p, p], i),
        "canny_hip_dev_hough_bits": ([p, p, i, i, i, f, f, i, i, f, f, p, p, p, p, p], i),
        "canny_hip_dev_canny_hough": ([p, p, f, i, i, i, i, i, p, f, f, i, i, f, f, p, p, p, p, p], i),
        "canny_hip_canny_hough": ([p, p, i, f, i, i, i, i, f, f, i, i, f, f, p, p, p, p], i),
        "canny_hip_hough_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_canny_components": ([p, p, f, i, i, i, i, i, p, i, p, p, p, C.c_ulonglong, p], i),
        "canny_hip_dev_components_bits": ([p, p, i, i, i, i, p, p, p, C.c_ulonglong, p], i),
        "canny_hip_canny_components": ([p, p, i, f, i, i, i, i, i, p, p, p, C.c_ulonglong, p], i),
        "canny_hip_components_from_bits": ([p, i, i, i, p, p, C.c_ulonglong, C.POINTER(C.c_ulonglong)], i),
        "canny_hip_components_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_canny_contours": ([p, p, f, i, i, i, i, i, p, i, p, C.c_ulonglong, p, p, p, C.c_ulonglong, p], i),
        "canny_hip_dev_contours_bits": ([p, p, i, i, i, i, p, C.c_ulonglong, p, p, p, C.c_ulonglong, p], i),
        "canny_hip_canny_contours": ([p, p, i, f, i, i, i, i, i, p, C.c_ulonglong, p, p, p, C.c_ulonglong, p], i),
        "canny_hip_contours_from_bits": ([p, i, i, i, p, C.c_ulonglong, C.POINTER(C.c_ulonglong), p, p, C.c_ulonglong,
                                          C.POINTER(C.c_ulonglong)], i),
        "canny_hip_contours_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_canny_edt": ([p, p, f, i, i, i, i, i, p, p, p, p], i),
        "canny_hip_dev_edt_bits": ([p, p, i, i, i, p, p, p], i),
        "canny_hip_canny_edt": ([p, p, i, f, i, i, i, i, p, p, p], i),
        "canny_hip_edt_from_bits": ([p, i, i, p, p, p], i),
        "canny_hip_edt_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_hough_segments_from_bits": ([p, i, i, f, f, f, f, p, i, i, i, i, p, i, ip], i),
        "canny_hip_dev_hough_segments_bits": ([p, p, i, i, i, f, f, f, f, p, p, i, i, i, i, p, i, p], i),
        "canny_hip_dev_canny_hough_segments": ([p, p, f, i, i, i, i, i, p, f, f, i, i, f, f, p, p, p, p, p, i, i, i, p, i,
                                                p], i),
        "canny_hip_canny_hough_segments": ([p, p, i, f, i, i, i, i, f, f, i, i, f, f, i, i, i, p, p, p, p, p, i, p], i),
        "canny_hip_hough_segments_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_histogram": ([p, p, i, i, i, i, i, p], i),
        "canny_hip_selftest_select": ([p, p, i, i, f, f, p], i),
        "canny_hip_selftest_workspace": ([p, i, C.POINTER(C.c_char_p), pp, C.POINTER(sz), ip], i),
        "canny_hip_selftest_launch_plan": ([i, i, i, i, C.c_longlong, p], i),
        "canny_hip_hough_circles_step_of": ([i, i, ip, ip], i),
        "canny_hip_hough_circles_from_bits": ([p, p, p, i, i, i, i, i, i, i, i, i, p, ip, ip, p], i),
        "canny_hip_dev_hough_circles_bits": ([p, p, p, p, i, i, i, i, i, i, i, i, i, i, p, p, p, p], i),
        "canny_hip_dev_canny_hough_circles": ([p, p, f, i, i, i, i, i, p, i, i, i, i, i, i, i, p, p, p, p], i),
        "canny_hip_canny_hough_circles": ([p, p, i, f, i, i, i, i, i, i, i, i, i, i, i, p, p, p], i),
        "canny_hip_dev_hough_circles_steps": ([p, p, p, C.c_size_t, p, p], i),
        "canny_hip_hough_circles_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_polygons_chains": ([p, p, i, ull, p, p, ull, i, i, C.c_uint, C.c_uint, p, p, ull, p], i),
        "canny_hip_dev_canny_polygons": ([p, p, f, i, i, i, i, i, p, i, p, ull, p, p, p, ull, p, C.c_uint, C.c_uint, p, p,
                                          ull, p], i),
        "canny_hip_dev_polygons_bits": ([p, p, i, i, i, i, p, ull, p, p, p, ull, p, C.c_uint, C.c_uint, p, p, ull, p], i),
        "canny_hip_canny_polygons": ([p, p, i, f, i, i, i, i, i, p, ull, p, p, p, ull, p, C.c_uint, C.c_uint, p, p, ull,
                                      p], i),
        "canny_hip_polygons_from_chains": ([p, p, ull, ull, i, i, C.c_uint, C.c_uint, p, p, ull, p], i),
        "canny_hip_polygons_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_canny_edgels": ([p, p, f, i, i, i, i, i, p, p, ull, p, p], i),
        "canny_hip_dev_edgels_at": ([p, p, i, i, i, i, p, p, p, ull], i),
        "canny_hip_canny_edgels": ([p, p, i, f, i, i, i, i, p, ull, p, p], i),
        "canny_hip_edgels_from_plane": ([p, i, i, i, p, ull, p], i),
        "canny_hip_dev_edgels_arith": ([p, p, p, sz, p, p, p, sz, p, p], i),
        "canny_hip_edgels_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_edgels_plan": ([i, i, i, ull, p], i),
        "canny_hip_line_fits_from_plane": ([p, p, i, i, i, f, i, i, p, p, p, i, p, i, i, p], i),
        "canny_hip_dev_line_fits_bits": ([p, p, p, i, i, i, i, f, f, f, f, p, p, i, p, p, i, i, p], i),
        "canny_hip_dev_canny_hough_line_fits": ([p, p, f, i, i, i, i, i, p, f, f, i, i, f, f, p, p, p, p, p, i, i, i, p, i,
                                                 p, i, p], i),
        "canny_hip_canny_hough_line_fits": ([p, p, i, f, i, i, i, i, f, f, i, i, f, f, i, i, i, i, p, p, p, p, p, i, p, p],
                                            i),
        "canny_hip_dev_line_fits_arith": ([p, p, sz, p], i),
        "canny_hip_line_fits_finish": ([p, sz, p], i),
        "canny_hip_line_fits_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_circle_fits_from_plane": ([p, p, i, i, i, p, i, i, i, i, p], i),
        "canny_hip_dev_circle_fits_bits": ([p, p, p, i, i, i, i, p, p, i, i, i, i, p], i),
        "canny_hip_dev_canny_hough_circle_fits": ([p, p, f, i, i, i, i, i, p, i, i, i, i, i, i, i, p, p, p, p, i, i, i, p],
                                                   i),
        "canny_hip_canny_hough_circle_fits": ([p, p, i, f, i, i, i, i, i, i, i, i, i, i, i, i, i, i, p, p, p, p], i),
        "canny_hip_dev_circle_fits_arith": ([p, p, sz, p], i),
        "canny_hip_circle_fits_finish": ([p, sz, p], i),
        "canny_hip_circle_fits_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_circle_fits_queue_capacity": ([], i),
        "canny_hip_chamfer_set_create": ([p, p, p, i, p], i),
        "canny_hip_chamfer_set_destroy": ([p, p], i),
        "canny_hip_dev_chamfer_dist2": ([p, p, i, i, i, p, i, i, i, i, p, p, p, p], i),
        "canny_hip_dev_chamfer_bits": ([p, p, i, i, i, p, p, i, i, i, i, p, p, p, p], i),
        "canny_hip_dev_canny_chamfer": ([p, p, f, i, i, i, i, i, p, p, p, i, i, i, i, p, p, p, p], i),
        "canny_hip_canny_chamfer": ([p, p, i, f, i, i, i, i, p, i, i, i, i, p, p, p], i),
        "canny_hip_chamfer_from_dist2": ([p, i, i, p, p, i, i, i, i, i, p, ip, ip, p], i),
        "canny_hip_chamfer_cost_of": ([i, i], i),
        "canny_hip_dev_chamfer_costs": ([p, p, sz, i, p], i),
        "canny_hip_chamfer_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_chamfer_plan": ([i, i, i, i, i, i, p], i),
        "canny_hip_selftest_chamfer_bands": ([p, p, i, i, p], i),
        "canny_hip_dev_shapes_chains": ([p, p, i, ull, p, p, ull, i, i, p, p, ull, p], i),
        "canny_hip_dev_canny_shapes": ([p, p, f, i, i, i, i, i, p, i, p, ull, p, p, p, ull, p, p, p, ull, p], i),
        "canny_hip_dev_shapes_bits": ([p, p, i, i, i, i, p, ull, p, p, p, ull, p, p, p, ull, p], i),
        "canny_hip_canny_shapes": ([p, p, i, f, i, i, i, i, i, p, ull, p, p, p, ull, p, p, p, ull, p], i),
        "canny_hip_shapes_from_chains": ([p, p, ull, ull, i, i, p, p, ull, p], i),
        "canny_hip_shapes_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_shapes_plan": ([i, ull, p], i),
        "canny_hip_dev_canny_curves": ([p, p, f, i, i, i, i, i, p, i, p, ull, p, p, p, ull, p], i),
        "canny_hip_dev_curves_bits": ([p, p, i, i, i, i, p, ull, p, p, p, ull, p], i),
        "canny_hip_canny_curves": ([p, p, i, f, i, i, i, i, i, p, ull, p, p, p, ull, p], i),
        "canny_hip_curves_from_bits": ([p, i, i, i, p, ull, C.POINTER(ull), p, p, ull, C.POINTER(ull)], i),
        "canny_hip_curves_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_curves_plan": ([i, i, i, p], i),
        "canny_hip_dev_canny_corners": ([p, p, f, i, i, i, i, i, p, i, i, i, i, C.c_longlong, i, i, p, p, p, p, p], i),
        "canny_hip_dev_corners_plane": ([p, p, i, i, i, i, i, i, i, C.c_longlong, i, i, p, p, p, p, p], i),
        "canny_hip_canny_corners": ([p, p, i, f, i, i, i, i, i, i, i, i, C.c_longlong, i, i, p, p, p, p], i),
        "canny_hip_corners_from_plane": ([p, i, i, i, i, i, i, C.c_longlong, i, i, p, ip, ip,
                                          C.POINTER(C.c_longlong), p], i),
        "canny_hip_corner_response_of": ([i, i, i, i, i, C.POINTER(C.c_longlong)], i),
        "canny_hip_dev_corners_arith": ([p, p, sz, i, i, p], i),
        "canny_hip_corners_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_corners_plan": ([i, i, i, i, ull, p], i),
        "canny_hip_dev_canny_corner_descriptors": ([p, p, f, i, i, i, i, i, p, i, i, i, i, C.c_longlong, i, i, p, p, p, p,
                                                    p, i, p, p], i),
        "canny_hip_dev_corner_descriptors": ([p, p, i, i, i, p, p, i, i, p, p], i),
        "canny_hip_canny_corner_descriptors": ([p, p, i, f, i, i, i, i, i, i, i, i, C.c_longlong, i, i, i, p, p, p, p], i),
        "canny_hip_corner_descriptors_from_plane": ([p, i, i, p, i, i, p, p], i),
        "canny_hip_descriptor_pattern": ([i, p], i),
        "canny_hip_dev_match_descriptors": ([p, p, p, i, i, p, p, i, i, p, i, i, i, i, p, p], i),
        "canny_hip_match_descriptors": ([p, i, p, i, i, i, i, p, ip], i),
        "canny_hip_descriptors_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_descriptors_plan": ([i, ull, i, p], i),
        "canny_hip_dev_estimate_motion": ([p, p, p, i, i, p, p, i, i, p, i, p, i, i, i, C.c_uint, p, p], i),
        "canny_hip_estimate_motion": ([p, i, p, i, p, i, i, i, C.c_uint, p, p], i),
        "canny_hip_canny_motion": ([p, p, i, f, i, i, i, i, i, i, i, i, C.c_longlong, i, i, i, p, i, i, i, i, i, i, i,
                                    C.c_uint, p, p, p, p, p], i),
        "canny_hip_motion_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_motion_plan": ([i, ull, i, p], i),
        "canny_hip_dev_compose_motion": ([p, p, i, i, p], i),
        "canny_hip_compose_motion": ([p, i, i, p], i),
        "canny_hip_dev_warp_frames": ([p, p, i, i, i, p, i, i, i, i, i, p, p], i),
        "canny_hip_warp_frames": ([p, i, i, i, p, i, i, i, i, i, p, p], i),
        "canny_hip_canny_align": ([p, p, i, f, i, i, i, i, i, i, i, i, C.c_longlong, i, i, i, i, i, i, i, i, i, C.c_uint, i, i,
                                   p, p, p, p], i),
        "canny_hip_warp_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_warp_plan": ([i, i, i, p, p, i, i, i, i, i, p], i),
        "canny_hip_dev_fuse_frames": ([p, p, p, i, i, i, i, i, i, i, i, p, p], i),
        "canny_hip_fuse_frames": ([p, p, i, i, i, i, i, i, i, i, p, p], i),
        "canny_hip_dev_change_mask": ([p, p, p, i, i, i, p, p, i, i, i, p, p], i),
        "canny_hip_change_mask": ([p, p, i, i, i, p, p, i, i, i, p, p], i),
        "canny_hip_canny_background": ([p, p, i, f, i, i, i, i, i, i, i, i, C.c_longlong, i, i, i, i, i, i, i, i, i, C.c_uint,
                                        i, i, i, i, i, i, p, p, p, p, p], i),
        "canny_hip_fuse_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_selftest_fuse_plan": ([i, i, i, i, i, i, p], i),
        "canny_hip_selftest_fuse_mean": ([p, p], i),
        "canny_hip_dev_morph_bits": ([p, p, i, i, i, i, p, i, i, i, i, p, p], i),
        "canny_hip_dev_canny_morph": ([p, i, i, i, i, p, i, i, i, i, p, p], i),
        "canny_hip_canny_morph": ([p, p, i, f, i, i, i, i, i, p, i, i, i, i, p, p], i),
        "canny_hip_morph_bits": ([p, i, i, i, i, p, i, i, i, i, p, p], i),
        "canny_hip_morph_element": ([i, i, i, p], i),
        "canny_hip_selftest_morph_plan": ([i, i, i, i, i, p], i),
        "canny_hip_morph_profile_get": ([p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_binarize": ([p, p, i, i, i, i, i, i, i, i, p, p, p], i),
        "canny_hip_binarize_batch": ([p, p, i, i, i, i, i, i, i, i, p, p, p], i),
        "canny_hip_binarize": ([p, i, i, i, i, i, i, i, i, p, p, p], i),
        "canny_hip_otsu_from_histogram": ([p, C.POINTER(C.c_int)], i),
        "canny_hip_selftest_binarize_plan": ([i, i, i, i, i, i, p], i),
        "canny_hip_profile_part_get": ([p, C.c_char_p, i, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "canny_hip_dev_thin_bits": ([p, p, i, i, i, i, i, p, p], i),
        "canny_hip_dev_canny_thin": ([p, i, i, i, i, i, p, p], i),
        "canny_hip_thin_batch": ([p, p, i, i, i, i, i, p, p], i),
        "canny_hip_thin_bits": ([p, i, i, i, i, i, p, p], i),
        "canny_hip_selftest_thin_plan": ([i, i, i, i, p], i),
        "canny_hip_dev_reconstruct_bits": ([p, p, p, i, i, i, i, i, p, p], i),
        "canny_hip_dev_canny_reconstruct": ([p, p, i, i, i, i, i, p, p], i),
        "canny_hip_reconstruct_batch": ([p, p, p, i, i, i, i, i, p, p], i),
        "canny_hip_reconstruct_bits": ([p, p, i, i, i, i, i, p, p], i),
        "canny_hip_selftest_reconstruct_plan": ([i, i, i, i, p], i),
        "canny_hip_dev_gray_morph": ([p, p, i, i, i, i, p, i, i, i, i, i, p], i),
        "canny_hip_gray_morph_batch": ([p, p, i, i, i, i, p, i, i, i, i, i, p], i),
        "canny_hip_gray_morph": ([p, i, i, i, i, p, i, i, i, i, i, p], i),
        "canny_hip_selftest_gray_morph_plan": ([i, i, i, i, i, i, p], i),
        "canny_hip_pyramid_layout": ([i, i, i, i, p, p], i),
        "canny_hip_dev_pyr_down": ([p, p, i, i, i, p], i),
        "canny_hip_dev_pyramid": ([p, p, i, i, i, i, p], i),
        "canny_hip_dev_pyr_up": ([p, p, i, i, i, i, i, p], i),
        "canny_hip_pyramid_batch": ([p, p, i, i, i, i, p], i),
        "canny_hip_pyr_up_batch": ([p, p, i, i, i, i, i, p], i),
        "canny_hip_pyramid": ([p, i, i, i, i, p], i),
        "canny_hip_pyr_up": ([p, i, i, i, i, i, p], i),
        "canny_hip_selftest_pyramid_plan": ([i, i, i, p], i),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def status_string(status: int) -> str:
    return load().canny_hip_status_string(status).decode()


def device_count() -> int:
    n = C.c_int(0)
    load().canny_hip_device_count(C.byref(n))
    return n.value


def expand_bits(bits: np.ndarray, height: int, width: int, u8: bool = False, threads: int = 4, out=None) -> np.ndarray:
    """Host-only: a packed bit map (rows MSB-first, padded to bytes) -> the short (or byte) edge plane, through the same
    thread pool the batch pipelines use for their compact transfer."""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    assert bits.size == height * ((width + 7) // 8)
    if out is None:
        out = np.empty((height, width), np.uint8 if u8 else np.int16)
    _ok(load().canny_hip_selftest_expand_bits(bits.ctypes.data_as(C.c_void_p), height, width, int(u8),
                                              out.ctypes.data_as(C.c_void_p), threads), "selftest_expand_bits")
    return out


def points_from_bits(bits, height: int, width: int, capacity: Optional[int] = None) -> np.ndarray:
    """Host-only: one packed bit map (rows MSB-first, padded to bytes: numpy.packbits(mask, axis=-1)) -> the ascending
    indices r * width + c of its set pixels, uint32 -- np.flatnonzero(mask).  Padding bits are ignored.  With a capacity
    the result is the prefix that fits, and the true count is returned too: (points, count)."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    n = C.c_ulonglong(0)
    L = load()
    if capacity is None:
        _ok(L.canny_hip_points_from_bits(_hp(b), height, width, None, 0, C.byref(n)), "points_from_bits")
    cap = n.value if capacity is None else int(capacity)
    pts = np.empty(cap, np.uint32)
    _ok(L.canny_hip_points_from_bits(_hp(b), height, width, _hp(pts) if cap else None, cap, C.byref(n)), "points_from_bits")
    return pts if capacity is None else (pts[:min(cap, n.value)], n.value)


CC_STATS = 6                                                    # ints per record: CANNY_HIP_CC_STAT_*
CC_LEFT, CC_TOP, CC_WIDTH, CC_HEIGHT, CC_AREA, CC_FIRST = range(6)
CC_PARTS = ("link", "resolve", "number", "write")


def components_from_bits(bits, height: int, width: int, min_area: int = 1, want_labels: bool = True,
                         capacity: Optional[int] = None):
    """Host-only: the 8-connected components of one packed bit map (numpy.packbits(mask, axis=-1); padding bits ignored)
    with at least min_area pixels, numbered 1..K by ascending first pixel -- scipy.ndimage.label(mask, np.ones((3, 3)))
    for min_area <= 1.  Returns (labels int32 [height, width] or None, stats int32 [K, 6], K); with a capacity, stats
    holds the first min(K, capacity) records and K is still the true count."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    L = load()
    n = C.c_ulonglong(0)
    if capacity is None:
        _ok(L.canny_hip_components_from_bits(_hp(b), height, width, min_area, None, None, 0, C.byref(n)), "components_from_bits")
    cap = n.value if capacity is None else int(capacity)
    labels = np.empty((height, width), np.int32) if want_labels else None
    stats = np.empty((cap, CC_STATS), np.int32)
    _ok(L.canny_hip_components_from_bits(_hp(b), height, width, min_area, _hp(labels) if want_labels else None,
                                         _hp(stats) if cap else None, cap, C.byref(n)), "components_from_bits")
    return labels, stats[:min(cap, n.value)], n.value


CONTOUR_PARTS = ("label", "count", "write", "stats")


def contours_from_bits(bits, height: int, width: int, min_area: int = 1, want_stats: bool = True,
                       capacity: Optional[int] = None, point_capacity: Optional[int] = None):
    """Host-only: the outer contour chain of every 8-connected component of one packed bit map (numpy.packbits(mask,
    axis=-1); padding bits ignored) with at least min_area pixels, in the components' order.  Returns (stats int32 [k, 6]
    or None, chain_offsets uint64 [k + 1], points int32, K, P): record j's chain is points[chain_offsets[j] :
    chain_offsets[j + 1]], pixel indices r * width + c.  With capacity / point_capacity None everything is returned
    (k = K, len(points) = P); otherwise k = min(K, capacity), points holds the positions below point_capacity that belong
    to those records, and K, P are still the true counts."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    L = load()
    k, n = C.c_ulonglong(0), C.c_ulonglong(0)
    if capacity is None or point_capacity is None:
        _ok(L.canny_hip_contours_from_bits(_hp(b), height, width, min_area, None, 0, C.byref(k), None, None, 0,
                                           C.byref(n)), "contours_from_bits")
    cap = k.value if capacity is None else int(capacity)
    pcap = n.value if point_capacity is None else int(point_capacity)
    stats = np.empty((cap, CC_STATS), np.int32) if want_stats else None
    chain = np.zeros(cap + 1, np.uint64)
    points = np.empty(pcap, np.int32)
    _ok(L.canny_hip_contours_from_bits(_hp(b), height, width, min_area, _hp(stats) if want_stats and cap else None, cap,
                                       C.byref(k), _hp(chain), _hp(points) if pcap else None, pcap, C.byref(n)),
        "contours_from_bits")
    fit = min(cap, k.value)
    return (stats[:fit] if want_stats else None, chain[:fit + 1], points[:min(pcap, int(chain[fit]))], k.value, n.value)


POLYGON_PARTS = ("simplify", "scan", "emit")
POLYGON_MEASURES = ("vertices", "length_q8", "area2", "convex")


def polygon_tolerance(epsilon: float = 0.0, ratio: float = 0.0) -> Tuple[int, int]:
    """(epsilon_q8, ratio_q16) of a tolerance in pixels and one relative to the chain's length, by rounding."""
    eq, rq = int(round(float(epsilon) * 256.0)), int(round(float(ratio) * 65536.0))
    if not (0 <= eq < 2 ** 32 and 0 <= rq < 65536):
        raise ValueError("epsilon must lie in [0, 2^24) pixels and ratio in [0, 1)")
    return eq, rq


def polygons_from_chains(chain_offsets, points, width: int, height: int, epsilon_q8: int = 0, ratio_q16: int = 0,
                         point_capacity: Optional[int] = None, vertex_capacity: Optional[int] = None,
                         want_measures: bool = True):
    """Host-only: the polygon of every chain.  chain_offsets uint64 [k + 1] and points int32 are
    what contours_from_bits / Context.canny_contours return.  Returns (vertex_offsets uint64 [k + 1], vertices int32,
    measures int64 [k, 4] or None): record j's polygon is vertices[vertex_offsets[j] : vertex_offsets[j + 1]], pixel
    indices r * width + c in chain order.  point_capacity (default: len(points)) says which chains are complete: one that
    ends beyond it has no vertices and the measures (-1, 0, 0, 0).  With vertex_capacity given, vertices holds the
    positions below it and vertex_offsets are still the true counts."""
    co = np.ascontiguousarray(chain_offsets, dtype=np.uint64)
    pts = np.ascontiguousarray(points, dtype=np.int32)
    k = co.size - 1
    if k < 0:
        raise ValueError("chain_offsets needs at least one entry")
    pcap = pts.size if point_capacity is None else int(point_capacity)
    if pcap > pts.size:
        raise ValueError("point_capacity exceeds the points given")
    L = load()
    voff = np.zeros(k + 1, np.uint64)
    measures = np.zeros((k, 4), np.int64) if want_measures else None

    def call(verts, vcap):
        _ok(L.canny_hip_polygons_from_chains(_hp(co), _hp(pts) if pts.size else None, k, pcap, width, height, epsilon_q8,
                                             ratio_q16, _hp(voff), _hp(verts) if vcap else None, vcap,
                                             _hp(measures) if want_measures and k else None), "polygons_from_chains")

    if vertex_capacity is None:
        call(None, 0)
    vcap = int(voff[-1]) if vertex_capacity is None else int(vertex_capacity)
    verts = np.empty(vcap, np.int32)
    call(verts, vcap)
    return voff, verts[:min(vcap, int(voff[-1]))], measures


SHAPE_PARTS = ("measure", "scan", "emit")
SHAPE_WORDS = 20
SHAPE_MEASURES = ("hull_vertices", "points", "anchor", "area2", "m10_6", "m01_6", "m20_12", "m11_24", "m02_12", "s10", "s01",
                  "s20", "s11", "s02", "hull_area2", "rect_edge", "rect_along_min", "rect_along_max", "rect_across",
                  "rect_len2")
SHAPES_PLANS = {"records": 0, "scan_sums": 1}


def shapes_from_chains(chain_offsets, points, width: int, height: int, point_capacity: Optional[int] = None,
                       hull_capacity: Optional[int] = None, want_measures: bool = True):
    """Host-only: the shape measures of every chain.  chain_offsets uint64 [k + 1] and points int32
    are what contours_from_bits / Context.canny_contours return.  Returns (hull_offsets uint64 [k + 1], hull int32,
    measures int64 [k, 20] or None): record j's convex hull is hull[hull_offsets[j] : hull_offsets[j + 1]], pixel indices
    r * width + c from the leftmost vertex on, and measures[j] holds the words named in SHAPE_MEASURES.  point_capacity
    (default: len(points)) says which chains are complete: one that ends beyond it has no hull and the measures
    (-1, 0, ...).  With hull_capacity given, hull holds the positions below it and hull_offsets are still the true counts."""
    co = np.ascontiguousarray(chain_offsets, dtype=np.uint64)
    pts = np.ascontiguousarray(points, dtype=np.int32)
    k = co.size - 1
    if k < 0:
        raise ValueError("chain_offsets needs at least one entry")
    pcap = pts.size if point_capacity is None else int(point_capacity)
    if pcap > pts.size:
        raise ValueError("point_capacity exceeds the points given")
    L = load()
    hoff = np.zeros(k + 1, np.uint64)
    measures = np.zeros((k, SHAPE_WORDS), np.int64) if want_measures else None

    def call(hull, hcap):
        _ok(L.canny_hip_shapes_from_chains(_hp(co), _hp(pts) if pts.size else None, k, pcap, width, height, _hp(hoff),
                                           _hp(hull) if hcap else None, hcap,
                                           _hp(measures) if want_measures and k else None), "shapes_from_chains")

    if hull_capacity is None:
        call(None, 0)
    hcap = int(hoff[-1]) if hull_capacity is None else int(hull_capacity)
    hull = np.empty(hcap, np.int32)
    call(hull, hcap)
    return hoff, hull[:min(hcap, int(hoff[-1]))], measures


def shape_rectangle(measures_row, hull, width: int):
    """The minimum-area rectangle of one record as floats: (corners [4, 2] as (x, y), (length, breadth), angle in radians of
    the side on the hull edge), from the exact words of measures_row and the record's hull (pixel indices).  A hull of one
    vertex gives that point four times."""
    m = [int(v) for v in measures_row]
    hx, hy = [int(q) % width for q in hull], [int(q) // width for q in hull]
    v = len(hx)
    if v == 0:
        raise ValueError("the record has no hull")
    k, lo, hi, across, len2 = m[15:20]
    if v == 1 or len2 == 0:
        return np.array([[hx[0], hy[0]]] * 4, float), (0.0, 0.0), 0.0
    ax, ay = hx[k], hy[k]
    dx, dy = hx[(k + 1) % v] - ax, hy[(k + 1) % v] - ay
    nx, ny = -dy, dx                     # cross(d, n) = len2 > 0: the side the hull lies on
    c = [(ax + (a * dx + b * nx) / len2, ay + (a * dy + b * ny) / len2) for a, b in ((lo, 0), (hi, 0), (hi, across), (lo, across))]
    return np.array(c, float), ((hi - lo) / len2 ** 0.5, across / len2 ** 0.5), float(np.arctan2(dy, dx))


def shapes_plan(which, capacity: int) -> "LaunchPlan":
    """Host-only: the launch plan of a capped launch of the shape stage ("records": the measure and the emit kernel,
    "scan_sums": the scan's pass over its chunks) at a record capacity; fields as launch_plan."""
    return _plan("shapes_plan", SHAPES_PLANS.get(which, which), int(capacity))


CURVE_PARTS = ("count", "write")
CURVE_RECORD = 4                                                # CANNY_HIP_CURVE_RECORD: start, end, points, flags
CURVE_CLOSED, CURVE_START_JUNCTION, CURVE_END_JUNCTION, CURVE_ISOLATED = 1, 2, 4, 8   # canny_hip_curve_flag
CURVE_FIRST_DIR_SHIFT, CURVE_LAST_DIR_SHIFT = 4, 8


def curves_from_bits(bits, height: int, width: int, min_length: int = 1, want_records: bool = True,
                     capacity: Optional[int] = None, point_capacity: Optional[int] = None):
    """Host-only: the edge curves of one packed bit map (numpy.packbits(mask, axis=-1); padding bits ignored) with at least
    min_length points, in key order: every set pixel once, in order along its curve, curves split at junctions.  Returns
    (records int32 [k, 4] or None, chain_offsets uint64 [k + 1], points int32, K, P): record j (start, end, points, flags)
    has the points points[chain_offsets[j] : chain_offsets[j + 1]], pixel indices r * width + c.  With capacity /
    point_capacity None everything is returned (k = K, len(points) = P); otherwise k = min(K, capacity), points holds the
    positions below point_capacity that belong to those records, and K, P are still the true counts."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    L = load()
    k, n = C.c_ulonglong(0), C.c_ulonglong(0)
    if capacity is None or point_capacity is None:
        _ok(L.canny_hip_curves_from_bits(_hp(b), height, width, min_length, None, 0, C.byref(k), None, None, 0, C.byref(n)),
            "curves_from_bits")
    cap = k.value if capacity is None else int(capacity)
    pcap = n.value if point_capacity is None else int(point_capacity)
    records = np.empty((cap, CURVE_RECORD), np.int32) if want_records else None
    chain = np.zeros(cap + 1, np.uint64)
    points = np.empty(pcap, np.int32)
    _ok(L.canny_hip_curves_from_bits(_hp(b), height, width, min_length, _hp(records) if want_records and cap else None, cap,
                                     C.byref(k), _hp(chain), _hp(points) if pcap else None, pcap, C.byref(n)), "curves_from_bits")
    fit = min(cap, k.value)
    return (records[:fit] if want_records else None, chain[:fit + 1], points[:min(pcap, int(chain[fit]))], k.value, n.value)


def curves_plan(n_frames: int, height: int, width: int) -> "LaunchPlan":
    """Host-only: the launch plan of the edge curves' row kernels (count and write: one wave per image row of the batch and
    trip) for a batch of these sizes; fields as launch_plan."""
    return _plan("curves_plan", int(n_frames), int(height), int(width))


EDT_NONE = 0x7FFFFFFF                                           # CANNY_HIP_EDT_NONE: dist2 of a frame without edge pixels
EDT_PARTS = ("rows", "columns")


def edt_from_bits(bits, height: int, width: int, want_dist2: bool = True, want_dist: bool = True,
                  want_nearest: bool = True):
    """Host-only: the exact Euclidean distance transform of one packed bit map (numpy.packbits(mask, axis=-1); padding
    bits ignored).  Returns (dist2 int32, dist float32, nearest int32), each [height, width] or None when not asked for:
    the squared distance to the nearest set pixel, its correctly rounded root -- scipy.ndimage.distance_transform_edt(
    ~mask).astype(float32) -- and that pixel's index r * width + c (the smallest among equally near ones).  A map
    without set pixels gives EDT_NONE, +inf and -1."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if height >= 1 and width >= 1 and b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    ok = height >= 1 and width >= 1 and height * width < 2 ** 31
    shape = (height, width) if ok else (1, 1)           # sizes the library rejects: it must not be handed real planes
    d2 = np.empty(shape, np.int32) if want_dist2 else None
    d = np.empty(shape, np.float32) if want_dist else None
    nn = np.empty(shape, np.int32) if want_nearest else None
    _ok(load().canny_hip_edt_from_bits(_hp(b), height, width, _hp(d2) if want_dist2 else None,
                                       _hp(d) if want_dist else None, _hp(nn) if want_nearest else None), "edt_from_bits")
    return d2, d, nn


HOUGH_MAX_LINES = 4096
HOUGH_PARTS = ("vote", "peaks", "select")


def hough_geometry(height: int, width: int, rho: float = 1.0, theta: float = np.pi / 180, min_theta: float = 0.0,
                   max_theta: float = np.pi) -> Tuple[int, int]:
    """(numangle, numrho) of the Hough accumulator for a frame size and resolution (host-only; the rule of
    include/canny_hip.h).  The accumulator of a frame is (numangle + 2) x (numrho + 2) int32."""
    na, nr = C.c_int(0), C.c_int(0)
    st = load().canny_hip_hough_geometry(height, width, rho, theta, min_theta, max_theta, C.byref(na), C.byref(nr))
    if st != OK:
        raise CannyHipError(st, "hough_geometry")
    return na.value, nr.value


def hough_tables(rho: float, theta: float, min_theta: float, numangle: int) -> Tuple[np.ndarray, np.ndarray]:
    """The vote tables (cos / rho, sin / rho per angle, float32) exactly as the device uses them (host-only)."""
    tc, ts = np.empty(max(numangle, 0), np.float32), np.empty(max(numangle, 0), np.float32)
    st = load().canny_hip_hough_tables(rho, theta, min_theta, numangle, _hp(tc) if numangle > 0 else None,
                                       _hp(ts) if numangle > 0 else None)
    if st != OK:
        raise CannyHipError(st, "hough_tables")
    return tc, ts


def hough_line_of(base: int, numrho: int, rho: float, theta: float, min_theta: float = 0.0) -> Tuple[np.float32, np.float32]:
    """(rho, theta) of accumulator cell `base`, as float32, exactly as the device writes them (host-only)."""
    lr, lt = C.c_float(0), C.c_float(0)
    st = load().canny_hip_hough_line_of(base, numrho, rho, theta, min_theta, C.byref(lr), C.byref(lt))
    if st != OK:
        raise CannyHipError(st, "hough_line_of")
    return np.float32(lr.value), np.float32(lt.value)


SEGMENT_INTS = 6                                                # ints per record: x0, y0, x1, y1, line, support
SEGMENT_PARTS = ("count", "emit", "exclusive")


def hough_segments_from_bits(bits, height: int, width: int, bases, rho: float = 1.0, theta: float = np.pi / 180,
                             min_theta: float = 0.0, max_theta: float = np.pi, min_length: int = 0, max_gap: int = 0,
                             exclusive: int = 0, segments_max: Optional[int] = None, out=None):
    """Host-only: the segment rule of include/canny_hip.h on one packed bit map (numpy.packbits(mask, axis=-1); padding
    bits ignored) along the lines `bases` (accumulator cells, in order).  Returns (segments int32 [k, 6], count): the rows
    x0, y0, x1, y1, line, support of the first k = min(segments_max, count) segments and the true count.  Without a
    segments_max everything is returned.  `out` (int32, at least segments_max * 6) receives the records in place."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if height >= 1 and width >= 1 and b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    ba = np.ascontiguousarray(bases, dtype=np.uint32).ravel()
    L = load()
    n = C.c_int(0)

    def run(buf, cap):
        _ok(L.canny_hip_hough_segments_from_bits(_hp(b), height, width, rho, theta, min_theta, max_theta,
                                                 _hp(ba) if ba.size else None, int(ba.size), min_length, max_gap,
                                                 exclusive, _hp(buf), cap, C.byref(n)), "hough_segments_from_bits")

    if segments_max is None:
        run(np.empty(SEGMENT_INTS, np.int32), 1)
        segments_max = max(n.value, 1)
    buf = out if out is not None else np.empty(max(int(segments_max), 1) * SEGMENT_INTS, np.int32)
    run(buf, int(segments_max))
    k = min(n.value, max(int(segments_max), 0))
    return buf[:k * SEGMENT_INTS].reshape(k, SEGMENT_INTS), n.value


CIRCLES_MAX_RADIUS = 1024                                       # CANNY_HIP_CIRCLES_MAX_RADIUS
CIRCLE_INTS = 6                                                 # ints per record: x2, y2, radius, votes, support, base
CIRCLE_PARTS = ("vote", "centres", "radius", "accept")
CIRCLE_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("x2", np.int32), ("y2", np.int32), ("radius", np.int32),
                         ("votes", np.int32), ("support", np.int32), ("base", np.int32)])


def hough_circles_step_of(gx: int, gy: int) -> Tuple[int, int]:
    """Host-only: the step (sx, sy) of one gradient as the rule of include/canny_hip.h defines it."""
    sx, sy = C.c_int(0), C.c_int(0)
    _ok(load().canny_hip_hough_circles_step_of(int(gx), int(gy), C.byref(sx), C.byref(sy)), "hough_circles_step_of")
    return sx.value, sy.value


def hough_circles_from_bits(bits, gx, gy, height: int, width: int, min_radius: int, max_radius: int, cell_shift: int = 0,
                            threshold: int = 20, support_threshold: int = 10, min_dist: int = 0, centres_max: int = 256,
                            want_accum: bool = False, out=None):
    """Host-only: the circle rule of include/canny_hip.h on one packed bit map (numpy.packbits(mask, axis=-1); padding bits
    ignored) and its int16 gradient planes.  Returns (circles int32 [k, 6], n_peaks[, accum]): the accepted records x2, y2,
    radius, votes, support, base and the true number of peaks.  `out` (int32, at least centres_max * 6) receives the
    records in place."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if height >= 1 and width >= 1 and b.size != height * ((width + 7) // 8):
        raise ValueError(f"expected {height} rows of {(width + 7) // 8} bytes, got {b.size} bytes")
    px, py = np.ascontiguousarray(gx, dtype=np.int16), np.ascontiguousarray(gy, dtype=np.int16)
    if px.size != height * width or py.size != height * width:
        raise ValueError("gx and gy must hold height * width shorts each")
    c = 1 << max(0, min(int(cell_shift), 3))
    acc = np.zeros(((height + c - 1) // c + 2, (width + c - 1) // c + 2), np.int32) if want_accum else None
    buf = out if out is not None else np.empty(max(int(centres_max), 1) * CIRCLE_INTS, np.int32)
    n, peaks = C.c_int(0), C.c_int(0)
    _ok(load().canny_hip_hough_circles_from_bits(_hp(b), _hp(px), _hp(py), height, width, min_radius, max_radius,
                                                 cell_shift, threshold, support_threshold, min_dist, centres_max,
                                                 _hp(buf), C.byref(n), C.byref(peaks), _hp(acc) if want_accum else None),
        "hough_circles_from_bits")
    rec = buf[:n.value * CIRCLE_INTS].reshape(n.value, CIRCLE_INTS)
    return (rec, peaks.value, acc) if want_accum else (rec, peaks.value)


# sub-pixel edgel records (include/canny_hip.h): (n, EDGEL_INTS) int32
EDGEL_INTS = 4
EDGEL_MAG_MASK, EDGEL_DIR_SHIFT, EDGEL_REFINED, EDGEL_INVALID = 0x00FFFFFF, 24, 0x10000000, 0x80000000
EDGEL_PART_LAYOUT, EDGEL_PART_REFINE = 0, 1


def edgels_from_plane(plane, points) -> np.ndarray:
    """Host-only: the edgel rule on one host plane (uint8 or int16, [H, W], H and W >= 2) at the pixel indices r * W + c of
    `points` (any unsigned 32-bit values; those >= H * W give invalid records) -> (n, 4) int32 records."""
    a = np.ascontiguousarray(plane)
    if a.ndim != 2 or a.dtype not in (np.uint8, np.int16):
        raise ValueError("expected a 2-D uint8 or int16 plane")
    pts = np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
    rec = np.empty((pts.size, EDGEL_INTS), np.int32)
    _ok(load().canny_hip_edgels_from_plane(_hp(a), int(a.dtype == np.uint8), a.shape[0], a.shape[1],
                                           _hp(pts) if pts.size else None, pts.size, _hp(rec) if pts.size else None),
        "edgels_from_plane")
    return rec


def edgels_xy(rec) -> Tuple[np.ndarray, np.ndarray]:
    """Sub-pixel (x, y) of edgel records, float64 pixels (x = column, y = row)."""
    r = np.asarray(rec, np.int32).reshape(-1, EDGEL_INTS)
    return r[:, 0] / 256.0, r[:, 1] / 256.0


def edgels_gradient(rec) -> Tuple[np.ndarray, np.ndarray]:
    """(gx, gy) of edgel records, int16."""
    w = np.ascontiguousarray(np.asarray(rec, np.int32).reshape(-1, EDGEL_INTS)[:, 2]).view(np.uint32)
    return (w & 0xFFFF).astype(np.uint16).view(np.int16), (w >> 16).astype(np.uint16).view(np.int16)


def edgels_magnitude(rec) -> np.ndarray:
    """Gradient magnitude of edgel records in grey levels, float64 (the record holds 1/16 levels)."""
    w = np.ascontiguousarray(np.asarray(rec, np.int32).reshape(-1, EDGEL_INTS)[:, 3]).view(np.uint32)
    return (w & EDGEL_MAG_MASK) / 16.0


def edgels_flags(rec) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(dir 0..3 -- step (1,0), (1,1), (0,1), (1,-1) --, refined, invalid) of edgel records."""
    w = np.ascontiguousarray(np.asarray(rec, np.int32).reshape(-1, EDGEL_INTS)[:, 3]).view(np.uint32)
    return ((w >> EDGEL_DIR_SHIFT) & 3).astype(np.int32), (w & EDGEL_REFINED) != 0, (w & EDGEL_INVALID) != 0


def edgels_plan(n_frames: int, height: int, width: int, n_points: int) -> "LaunchPlan":
    """Host-only: the launch plan of the index-driven edgel kernel (Context.dev_edgels_at) for a frame's list of n_points
    entries; fields as launch_plan."""
    return _plan("edgels_plan", int(n_frames), int(height), int(width), int(n_points))


LINE_FIT_INTS = 12
LINE_FIT_GATE, LINE_FIT_REFINED_ONLY = 1, 2
LINE_FIT_MAXD_MASK, LINE_FIT_DEGENERATE, LINE_FIT_INVALID = 0x00FFFFFF, 0x10000000, 0x80000000
LINE_FIT_PART_FIT = 0


def line_fits_from_plane(bits, plane, bases, segments, rho: float = 1.0, theta: float = np.pi / 180,
                         min_theta: float = 0.0, max_theta: float = np.pi, options: int = 0) -> np.ndarray:
    """Host-only: the line-fit rule of include/canny_hip.h on one host frame: a packed bit map (numpy.packbits(mask,
    axis=-1)), its plane (uint8 or int16 [H, W]), the line list `bases` and segment records (k, 6) as
    hough_segments_from_bits returns them -> (k, 12) int32 fit records; unpack them with line_fits_unpack."""
    a = np.ascontiguousarray(plane)
    if a.ndim != 2 or a.dtype not in (np.uint8, np.int16):
        raise ValueError("expected a 2-D uint8 or int16 plane")
    h, w = a.shape
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if b.size != h * ((w + 7) // 8):
        raise ValueError("bits must hold height * ceil(width / 8) bytes")
    numangle, numrho = hough_geometry(h, w, rho, theta, min_theta, max_theta)
    tc, ts = hough_tables(rho, theta, min_theta, numangle)
    bs = np.ascontiguousarray(bases, dtype=np.uint32).reshape(-1)
    seg = np.ascontiguousarray(segments, dtype=np.int32).reshape(-1, SEGMENT_INTS)
    fits = np.empty((seg.shape[0], LINE_FIT_INTS), np.int32)
    _ok(load().canny_hip_line_fits_from_plane(_hp(b), _hp(a), int(a.dtype == np.uint8), h, w, rho, numangle, numrho,
                                              _hp(tc), _hp(ts), _hp(bs) if bs.size else None, bs.size,
                                              _hp(seg) if seg.size else None, seg.shape[0], int(options),
                                              _hp(fits) if seg.size else None), "line_fits_from_plane")
    return fits


def line_fits_finish(moments) -> np.ndarray:
    """Host-only test hook: the finishing arithmetic of the rule in plain C++ on (k, 8) int64 moment sets (n, Su, Sv, Suu,
    Suv, Svv, ddx, ddy) -> (k, 6) int32 (mu, mv, dx_q30, dy_q30, n, DEGENERATE or 0)."""
    m = np.ascontiguousarray(moments, dtype=np.int64).reshape(-1, 8)
    out = np.empty((m.shape[0], 6), np.int32)
    _ok(load().canny_hip_line_fits_finish(_hp(m), m.shape[0], _hp(out)), "line_fits_finish")
    return out


def line_fits_unpack(fits) -> dict:
    """Floats from (k, 12) int32 fit records: p0, p1, centre ([k, 2] pixels, x then y), direction ([k, 2], unit), n,
    rms and maxd (pixels), degenerate, invalid."""
    r = np.ascontiguousarray(np.asarray(fits, np.int32).reshape(-1, LINE_FIT_INTS))
    w9 = np.ascontiguousarray(r[:, 9]).view(np.uint32)
    n = r[:, 8].astype(np.int64)
    sdd = (np.ascontiguousarray(r[:, 10]).view(np.uint32).astype(np.float64) +
           np.ascontiguousarray(r[:, 11]).view(np.uint32).astype(np.float64) * 4294967296.0)
    return {"p0": r[:, 0:2] / 65536.0, "p1": r[:, 2:4] / 65536.0, "centre": r[:, 4:6] / 65536.0,
            "direction": r[:, 6:8] / float(1 << 30), "n": n, "rms": np.sqrt(sdd / np.maximum(n, 1)) / 256.0,
            "maxd": (w9 & LINE_FIT_MAXD_MASK) / 256.0, "degenerate": (w9 & LINE_FIT_DEGENERATE) != 0,
            "invalid": (w9 & LINE_FIT_INVALID) != 0}


CIRCLE_FIT_INTS = 8
CIRCLE_FIT_GATE, CIRCLE_FIT_REFINED_ONLY = 1, 2
CIRCLE_FIT_MAXD_MASK, CIRCLE_FIT_TRIM_FAILED = 0x00FFFFFF, 0x08000000
CIRCLE_FIT_DEGENERATE, CIRCLE_FIT_INVALID = 0x10000000, 0x80000000
CIRCLE_FIT_MAX_BAND, CIRCLE_FIT_MOMENT_WORDS = 4, 12
CIRCLE_FIT_PART_FIT = 0


def circle_fits_from_plane(bits, plane, circles, band: int = 1, trim_q8: int = 0, options: int = 0) -> np.ndarray:
    """Host-only: the circle-fit rule of include/canny_hip.h on one host frame: a packed bit map (numpy.packbits(mask,
    axis=-1)), its plane (uint8 or int16 [H, W]) and circle records (k, 6) as hough_circles_from_bits returns them ->
    (k, 8) int32 fit records; unpack them with circle_fits_unpack."""
    a = np.ascontiguousarray(plane)
    if a.ndim != 2 or a.dtype not in (np.uint8, np.int16):
        raise ValueError("expected a 2-D uint8 or int16 plane")
    h, w = a.shape
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    if b.size != h * ((w + 7) // 8):
        raise ValueError("bits must hold height * ceil(width / 8) bytes")
    rec = np.ascontiguousarray(circles, dtype=np.int32).reshape(-1, CIRCLE_INTS)
    fits = np.empty((rec.shape[0], CIRCLE_FIT_INTS), np.int32)
    _ok(load().canny_hip_circle_fits_from_plane(_hp(b), _hp(a), int(a.dtype == np.uint8), h, w,
                                                _hp(rec) if rec.size else None, rec.shape[0], int(band), int(trim_q8),
                                                int(options), _hp(fits) if rec.size else None), "circle_fits_from_plane")
    return fits


def circle_fits_finish(moments) -> np.ndarray:
    """Host-only test hook: the finishing arithmetic of the rule in plain C++ on (k, 12) int64 moment sets (n, Su, Sv, Sz,
    Suu, Suv, Svv, Suz low, Suz high, Svz low, Svz high, band) -> (k, 4) int32 (move_x, move_y, n, DEGENERATE or 0)."""
    m = np.ascontiguousarray(moments, dtype=np.int64).reshape(-1, CIRCLE_FIT_MOMENT_WORDS)
    out = np.empty((m.shape[0], 4), np.int32)
    _ok(load().canny_hip_circle_fits_finish(_hp(m), m.shape[0], _hp(out)), "circle_fits_finish")
    return out


def circle_fits_queue_capacity() -> int:
    """Host-only: the band pixels of one record that the fit kernel keeps in LDS (more are recomputed, same bytes)."""
    return int(load().canny_hip_circle_fits_queue_capacity())


def circle_fits_unpack(fits) -> dict:
    """Floats from (k, 8) int32 fit records: centre ([k, 2] pixels, x then y), radius (pixels), n, rms and maxd (pixels),
    sectors (the 16-bit mask), sector_count, trim_failed, degenerate, invalid."""
    r = np.ascontiguousarray(np.asarray(fits, np.int32).reshape(-1, CIRCLE_FIT_INTS))
    w4 = np.ascontiguousarray(r[:, 4]).view(np.uint32)
    sec = np.ascontiguousarray(r[:, 5]).view(np.uint32) & 0xFFFF
    n = r[:, 3].astype(np.int64)
    sdd = (np.ascontiguousarray(r[:, 6]).view(np.uint32).astype(np.float64) +
           np.ascontiguousarray(r[:, 7]).view(np.uint32).astype(np.float64) * 4294967296.0)
    count = np.zeros(len(sec), np.int64)
    for k in range(16):
        count += (sec >> k) & 1
    return {"centre": r[:, 0:2] / 65536.0, "radius": r[:, 2] / 65536.0, "n": n,
            "rms": np.sqrt(sdd / np.maximum(n, 1)) / 256.0, "maxd": (w4 & CIRCLE_FIT_MAXD_MASK) / 256.0,
            "sectors": sec, "sector_count": count, "trim_failed": (w4 & CIRCLE_FIT_TRIM_FAILED) != 0,
            "degenerate": (w4 & CIRCLE_FIT_DEGENERATE) != 0, "invalid": (w4 & CIRCLE_FIT_INVALID) != 0}


# ---- corners, Harris / Shi-Tomasi -----------------------------------------------------------------
CORNER_WORDS = 4
CORNERS_MIN_EIGEN, CORNERS_HARRIS = 0, 1
CORNERS_MAX_SUM, CORNERS_MAX_K_Q8 = 50979600, 64
CORNER_PARTS = ("max", "candidates", "collect", "accept")
CORNERS_PLANS = ("tiles", "arith")
CORNER_DTYPE = np.dtype([("x", np.int64), ("y", np.int64), ("response", np.int64), ("rank", np.int64)])


def corner_response_of(sxx: int, syy: int, sxy: int, mode: int = CORNERS_MIN_EIGEN, k_q8: int = 0) -> int:
    """Host-only: the response R of the rule for one tensor (Sxx, Syy, Sxy)."""
    r = C.c_longlong(0)
    _ok(load().canny_hip_corner_response_of(int(sxx), int(syy), int(sxy), int(mode), int(k_q8), C.byref(r)), "corner_response_of")
    return r.value


def corners_from_plane(plane, mode: int = CORNERS_MIN_EIGEN, block: int = 3, k_q8: int = 0, quality_q16: int = 655,
                       min_response: int = 0, min_dist: int = 0, corners_max: int = 256, want_response: bool = False):
    """Host-only, needs no GPU: the corner rule on ONE uint8 plane [H, W] -> (corners int64 [k, 4]: x, y, response,
    rank; cand_count; max_response; response int64 [H, W] or None)."""
    a = np.ascontiguousarray(plane, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("expected a 2-D uint8 plane")
    h, w = a.shape
    rec = np.zeros((max(int(corners_max), 1), CORNER_WORDS), np.int64)
    resp = np.zeros((h, w), np.int64) if want_response else None
    n, nc, rmax = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _ok(load().canny_hip_corners_from_plane(_hp(a), h, w, int(mode), int(block), int(k_q8), int(quality_q16),
                                            int(min_response), int(min_dist), int(corners_max), _hp(rec), C.byref(n),
                                            C.byref(nc), C.byref(rmax), _hp(resp) if want_response else None),
        "corners_from_plane")
    return rec[:n.value].copy(), nc.value, rmax.value, resp


def corners_plan(which, n_frames: int = 1, height: int = 2, width: int = 2, n: int = 0):
    """Host-only: (LaunchPlan, frames per chunk) of a capped corners launch: "tiles" (the passes over the plane, sized by
    one frame) or "arith" (dev_corners_arith on n triples)."""
    k = CORNERS_PLANS.index(which) if isinstance(which, str) else int(which)
    return _plan("corners_plan", k, int(n_frames), int(height), int(width), int(n), n=6)


# ---- corner descriptors and Hamming matching -------------------------------------------------------
DESC_BITS, DESC_WORDS, DESC_RADIUS, DESC_ROTATIONS, MATCH_WORDS = 256, 4, 15, 32, 4
DESC_STEERED, MATCH_CROSS_CHECK = 1, 1
MATCH_MAX_PAIRS = 1 << 20
DESC_PARTS = ("describe", "match", "reverse", "finalize")
DESCRIPTORS_PLANS = ("describe", "match")
DESC_MATCH_DTYPE = np.dtype([("j", np.int32), ("d1", np.int32), ("d2", np.int32), ("flags", np.int32)])


def descriptor_pattern(k: int):
    """Host-only: int8 [256, 4], (ax, ay, bx, by) of every test in rotation k."""
    out = np.zeros((DESC_BITS, 4), np.int8)
    _ok(load().canny_hip_descriptor_pattern(int(k), _hp(out)), "descriptor_pattern")
    return out


def corner_descriptors_from_plane(plane, corners, steered: bool = False):
    """Host-only, needs no GPU: the descriptor rule on ONE uint8 plane [H, W] for records int64 [k, 4] (x, y, response,
    rank; or [k, 2]: x, y) -> (uint64 [k, 4], int32 [k]: k + 256 * border, -1 outside the frame)."""
    a = np.ascontiguousarray(plane, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("expected a 2-D uint8 plane")
    c = np.asarray(corners, np.int64).reshape(len(corners), -1)
    rec = np.zeros((len(c), CORNER_WORDS), np.int64)
    rec[:, :min(c.shape[1], CORNER_WORDS)] = c[:, :CORNER_WORDS]
    desc, meta = np.zeros((len(c), DESC_WORDS), np.uint64), np.zeros(len(c), np.int32)
    _ok(load().canny_hip_corner_descriptors_from_plane(_hp(a), a.shape[0], a.shape[1], _hp(rec), len(c),
                                                       DESC_STEERED if steered else 0, _hp(desc), _hp(meta)),
        "corner_descriptors_from_plane")
    return desc, meta


def match_descriptors(q, t, max_distance: int = 64, ratio_q8: int = 205, options: int = MATCH_CROSS_CHECK):
    """Host-only, needs no GPU: the matching rule on ONE pair of sets uint64 [nq, 4], [nt, 4] -> (int32 [nq, 4]: j, d1,
    d2, flags; the number accepted)."""
    q = np.ascontiguousarray(q, np.uint64).reshape(-1, DESC_WORDS)
    t = np.ascontiguousarray(t, np.uint64).reshape(-1, DESC_WORDS)
    out, acc = np.zeros((len(q), MATCH_WORDS), np.int32), C.c_int(0)
    _ok(load().canny_hip_match_descriptors(_hp(q) if len(q) else None, len(q), _hp(t) if len(t) else None, len(t),
                                           int(max_distance), int(ratio_q8), int(options),
                                           _hp(out) if len(q) else None, C.byref(acc)), "match_descriptors")
    return out, acc.value


def consecutive_pairs(n_frames: int):
    """int32 [n_frames - 1, 2]: the pairs (f, f + 1) of a batch of consecutive video frames, as the matcher takes them."""
    f = np.arange(max(int(n_frames) - 1, 0), dtype=np.int32)
    return np.ascontiguousarray(np.stack([f, f + 1], axis=1))


def descriptors_plan(which, n: int, stride: int):
    """Host-only: the LaunchPlan of a capped descriptor launch: "describe" (n frames, stride = corners_max) or "match" (n
    pairs, stride of the side held in registers)."""
    k = DESCRIPTORS_PLANS.index(which) if isinstance(which, str) else int(which)
    return _plan("descriptors_plan", k, int(n), int(stride))


# ---- frame-to-frame motion from the corner matches -------------------------------------------------
MOTION_TRANSLATION, MOTION_SIMILARITY, MOTION_AFFINE = 0, 1, 2
MOTION_WORDS, MOTION_MAX_HYPOTHESES = 16, 4096
MOTION_HAS_MODEL, MOTION_HAS_REFIT = 1, 2
MOTION_PARTS = ("gather", "score", "refit")
MOTION_PLANS = ("gather", "score", "refit")
MOTION_DTYPE = np.dtype([("flags", np.int64), ("m", np.int64), ("inliers", np.int64), ("h", np.int64), ("a11", np.int64),
                         ("a12", np.int64), ("tx", np.int64), ("a21", np.int64), ("a22", np.int64), ("ty", np.int64),
                         ("residual_sum", np.int64), ("residual_max", np.int64), ("i1", np.int64), ("i2", np.int64),
                         ("i3", np.int64), ("d", np.int64)])


def estimate_motion(q_corners, t_corners, matches, model: int = MOTION_SIMILARITY, thr_q4: int = 48, hypotheses: int = 256,
                    seed: int = 0):
    """Host-only, needs no GPU: the motion rule on ONE pair: records int64 [n_q, 4] and [n_t, 4] (x, y, response, rank; or
    [k, 2]: x, y), the matcher's row int32 [n_q, 4] -> (int64 [16] record, int32 [n_q] inlier flags: 1, 0, -1)."""
    def records(c):
        rec = np.zeros((len(c), CORNER_WORDS), np.int64)
        if len(c):
            c = np.asarray(c, np.int64).reshape(len(c), -1)
            rec[:, :min(c.shape[1], CORNER_WORDS)] = c[:, :CORNER_WORDS]
        return rec
    q, t = records(q_corners), records(t_corners)
    mt = np.ascontiguousarray(matches, np.int32).reshape(-1, MATCH_WORDS)
    if len(mt) != len(q):
        raise ValueError("one match row per query record")
    out, flags = np.zeros(MOTION_WORDS, np.int64), np.zeros(len(q), np.int32)
    _ok(load().canny_hip_estimate_motion(_hp(q) if len(q) else None, len(q), _hp(t) if len(t) else None, len(t),
                                         _hp(mt) if len(q) else None, int(model), int(thr_q4), int(hypotheses),
                                         int(seed) & 0xFFFFFFFF, _hp(out), _hp(flags) if len(q) else None), "estimate_motion")
    return out, flags


def motion_plan(which, n_pairs: int, hypotheses: int = 1):
    """Host-only: the LaunchPlan of a capped launch of the motion estimate: "gather", "score" or "refit"."""
    k = MOTION_PLANS.index(which) if isinstance(which, str) else int(which)
    return _plan("motion_plan", k, int(n_pairs), int(hypotheses))


# ---- frame alignment: the motions chained, frames warped ---------------------------------------------
XFORM_WORDS = 8
WARP_NEAREST, WARP_BILINEAR = 0, 1
WARP_LDS_BYTES = 16384
WARP_PARTS = ("compose", "warp")
WARP_ROUTE_AUTO, WARP_ROUTE_DIRECT, WARP_ROUTE_TILED = 0, 1, 2
XFORM_DTYPE = np.dtype([("flags", np.int64), ("src", np.int64), ("a11", np.int64), ("a12", np.int64), ("tx", np.int64),
                        ("a21", np.int64), ("a22", np.int64), ("ty", np.int64)])


def _words(records, words: int):
    a = np.asarray(records)
    if a.dtype.names:
        a = np.ascontiguousarray(a).view(np.int64)
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1, words)


def compose_motion(motion, first_frame: int = 0):
    """Host-only, needs no GPU: the motion records of the consecutive pairs (MOTION_DTYPE or int64 [n_pairs, 16]) chained
    into n_pairs + 1 transform records (XFORM_DTYPE); record k maps frame first_frame's pixels into frame first_frame + k."""
    m = _words(motion, MOTION_WORDS)
    out = np.zeros((len(m) + 1, XFORM_WORDS), np.int64)
    _ok(load().canny_hip_compose_motion(_hp(m) if len(m) else None, len(m), int(first_frame), _hp(out)), "compose_motion")
    return out.view(XFORM_DTYPE).reshape(-1)


def warp_frames(src, xforms, out_h: int, out_w: int, interp: int = WARP_BILINEAR, border: int = 0):
    """Host-only, needs no GPU: src uint8 [n_src, H, W] warped by the transform records (XFORM_DTYPE or int64 [n_out, 8]) ->
    (uint8 [n_out, out_h, out_w], valid bit maps uint8 [n_out, out_h, ceil(out_w / 8)], rows MSB-first)."""
    a = np.ascontiguousarray(src, dtype=np.uint8)
    if a.ndim != 3:
        raise ValueError("expected uint8 [n_src, H, W]")
    x = _words(xforms, XFORM_WORDS)
    out = np.zeros((len(x), max(int(out_h), 0), max(int(out_w), 0)), np.uint8)
    valid = np.zeros((len(x), max(int(out_h), 0), (max(int(out_w), 0) + 7) // 8), np.uint8)
    _ok(load().canny_hip_warp_frames(_hp(a), a.shape[0], a.shape[1], a.shape[2], _hp(x) if len(x) else None, len(x),
                                     int(out_h), int(out_w), int(interp), int(border), _hp(out), _hp(valid)), "warp_frames")
    return out, valid


WarpTile = collections.namedtuple("WarpTile", "staged x0 y0 x1 y1")


def warp_plan(n_out: int, out_h: int, out_w: int):
    """Host-only: the LaunchPlan of the warp's capped launch (one 64 x 16 output tile per workgroup and trip)."""
    return _plan("warp_plan", int(n_out), int(out_h), int(out_w), tail=(None, 1, 1, 0, 0, 0, None))


def warp_tile(xform, src_h: int, src_w: int, out_h: int, out_w: int, interp: int, tile_x: int, tile_y: int):
    """Host-only: what the tiled route does with one 64 x 16 output tile under one transform record: WarpTile(staged, x0, y0,
    x1, y1) -- staged in LDS or gathered directly, and the clipped source footprint (inclusive; x1 < x0: empty)."""
    x = _words(xform, XFORM_WORDS)[:1]
    out, box = np.zeros(5, np.uint64), np.zeros(5, np.int32)
    _ok(load().canny_hip_selftest_warp_plan(1, int(out_h), int(out_w), _hp(out), _hp(x), int(src_h), int(src_w), int(interp),
                                            int(tile_x), int(tile_y), _hp(box)), "selftest_warp_plan")
    return WarpTile(bool(box[0]), *(int(v) for v in box[1:]))


# ---- temporal fusion of aligned frames and change masks ---------------------------------------------
FUSE_MEAN, FUSE_MEDIAN, FUSE_MIN, FUSE_MAX = 0, 1, 2, 3
FUSE_ROUTE_AUTO, FUSE_ROUTE_REGISTERS, FUSE_ROUTE_PASSES = 0, 1, 2
FUSE_MAX_GROUP = 255
FUSE_MEAN_ROW = 65026
FUSE_PARTS = ("fuse", "mask")


def fuse_groups(n_frames: int, group_len: int, group_step: int) -> int:
    """The number of windows of group_len frames, group_step apart, in a stack of n_frames."""
    return (int(n_frames) - int(group_len)) // int(group_step) + 1


def _stack(frames, valid_bits):
    a = np.ascontiguousarray(frames, dtype=np.uint8)
    if a.ndim != 3:
        raise ValueError("expected uint8 [n_frames, H, W]")
    v = None
    if valid_bits is not None:
        v = np.ascontiguousarray(valid_bits, dtype=np.uint8)
        if v.shape != (a.shape[0], a.shape[1], (a.shape[2] + 7) // 8):
            raise ValueError("expected valid bit maps uint8 [n_frames, H, ceil(W / 8)]")
    return a, v


def fuse_frames(frames, valid_bits=None, group_len: Optional[int] = None, group_step: Optional[int] = None,
                op: int = FUSE_MEDIAN, fill: int = 0, min_count: int = 1):
    """Host-only, needs no GPU: frames uint8 [n_frames, H, W] reduced over windows of group_len frames (default: all of them),
    group_step apart (default: group_len), under the valid bit maps uint8 [n_frames, H, ceil(W / 8)] (rows MSB-first; None: all
    valid) -> (fused uint8 [n_groups, H, W], count uint8 [n_groups, H, W])."""
    a, v = _stack(frames, valid_bits)
    n, h, w = a.shape
    group_len = n if group_len is None else int(group_len)
    group_step = group_len if group_step is None else int(group_step)
    ok = 1 <= group_len <= n and group_step >= 1
    n_groups = fuse_groups(n, group_len, group_step) if ok else 1
    fused, count = np.zeros((n_groups, h, w), np.uint8), np.zeros((n_groups, h, w), np.uint8)
    _ok(load().canny_hip_fuse_frames(_hp(a), _hp(v) if v is not None else None, n, h, w, group_len, group_step, int(op),
                                     int(fill), int(min_count), _hp(fused), _hp(count)), "fuse_frames")
    return fused, count


def change_mask(frames, background, valid_bits=None, bg_count=None, frames_per_background: Optional[int] = None, thr: int = 0,
                min_count: int = 1):
    """Host-only, needs no GPU: the change masks of frames uint8 [n_frames, H, W] against background uint8 [n_background, H, W]
    (frame f against plane f // frames_per_background; default: one plane for all) -> (mask bit maps uint8 [n_frames, H,
    ceil(W / 8)], rows MSB-first with pad bits 0; changed int64 [n_frames], the set bits of each frame)."""
    a, v = _stack(frames, valid_bits)
    n, h, w = a.shape
    per = max(n, 1) if frames_per_background is None else int(frames_per_background)
    bg = np.ascontiguousarray(background, dtype=np.uint8)
    bg = bg[None] if bg.ndim == 2 else bg
    bc = None
    if bg_count is not None:
        bc = np.ascontiguousarray(bg_count, dtype=np.uint8)
        bc = bc[None] if bc.ndim == 2 else bc
    n_bg = -(-n // per) if per >= 1 else 1
    if bg.shape != (n_bg, h, w) or (bc is not None and bc.shape != bg.shape):
        raise ValueError("expected background (and bg_count) uint8 [ceil(n_frames / frames_per_background), H, W]")
    mask, changed = np.zeros((n, h, (w + 7) // 8), np.uint8), np.zeros(n, np.int64)
    _ok(load().canny_hip_change_mask(_hp(a), _hp(v) if v is not None else None, n, h, w, _hp(bg),
                                     _hp(bc) if bc is not None else None, per, int(thr), int(min_count), _hp(mask),
                                     _hp(changed)), "change_mask")
    return mask, changed


def fuse_plan(which, n_frames: int, h: int, w: int, group_len: int = 1, group_step: int = 1):
    """Host-only: the LaunchPlan of a capped launch of the temporal fusion (one 64 x 16 output tile per workgroup and trip):
    which is a name of FUSE_PARTS or its number.  "fuse": the tiles of the n_groups fused planes, aux = the route automatic
    takes for a MEDIAN of group_len frames; "mask": the tiles of the n_frames masks."""
    k = FUSE_PARTS.index(which) if isinstance(which, str) else int(which)
    return _plan("fuse_plan", k, int(n_frames), int(h), int(w), int(group_len), int(group_step))


# ---- binary morphology on packed bit maps ------------------------------------------------------------
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_GRADIENT, MORPH_TOPHAT, MORPH_BLACKHAT = range(7)
MORPH_OPS = ("erode", "dilate", "open", "close", "gradient", "tophat", "blackhat")
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2
MORPH_SHAPES = ("rect", "cross", "ellipse")
MORPH_BORDER_ZERO, MORPH_BORDER_ONE, MORPH_BORDER_NEUTRAL = 0, 1, 2
MORPH_ROUTE_AUTO, MORPH_ROUTE_GENERAL, MORPH_ROUTE_SEPARABLE = 0, 1, 2
MORPH_MAX_EXTENT, MORPH_MAX_ITERATIONS = 31, 16


def morph_element(shape: int, kw: int, kh: Optional[int] = None):
    """Host-only: the rows of a RECT, CROSS or ELLIPSE element of kw x kh (kh defaults to kw) as uint32 [kh]; bit i of row j
    is the offset (i - kw // 2, j - kh // 2)."""
    kh = kw if kh is None else kh
    rows = np.zeros(max(int(kh), 1), np.uint32)
    _ok(load().canny_hip_morph_element(int(shape), int(kw), int(kh), _hp(rows)), "morph_element")
    return rows


def _morph_rows(rows, kh: int):
    r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    if r.size != kh:
        raise ValueError("expected kh element rows")
    return r


def morph_bits(bits, w: int, op: int, rows, kw: int, kh: int, border: int = MORPH_BORDER_NEUTRAL, iterations: int = 1):
    """Host-only, needs no GPU: the operator on bit maps uint8 [n_frames, H, ceil(w / 8)] (rows MSB-first; pad bits ignored)
    -> (bit maps of the same shape with pad bits 0, counts int64 [n_frames])."""
    a = np.ascontiguousarray(bits, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != (int(w) + 7) // 8:
        raise ValueError("expected bit maps uint8 [n_frames, H, ceil(w / 8)]")
    n, h, _ = a.shape
    r = _morph_rows(rows, kh)
    out, counts = np.zeros_like(a), np.zeros(n, np.int64)
    _ok(load().canny_hip_morph_bits(_hp(a), n, h, int(w), int(op), _hp(r), int(kw), int(kh), int(border), int(iterations),
                                    _hp(out), _hp(counts)), "morph_bits")
    return out, counts


def morph_plan(n_frames: int, h: int, w: int, kw: int = 3, kh: int = 3):
    """Host-only: the LaunchPlan of one primitive step of the morphology (one tile of 8 words x 64 rows per workgroup and
    trip); aux = the route automatic takes for a full rectangle of kw x kh (1 general, 2 separable)."""
    return _plan("morph_plan", int(n_frames), int(h), int(w), int(kw), int(kh))


# ---- binarization: gray planes to packed bit maps --------------------------------------------------
BIN_FIXED, BIN_OTSU, BIN_ADAPTIVE_MEAN = range(3)
BIN_METHODS = ("fixed", "otsu", "mean")
BIN_PARTS = ("histogram", "select", "map")
BIN_ROUTE_AUTO, BIN_ROUTE_DIRECT, BIN_ROUTE_MARCH = 0, 1, 2
BIN_MAX_EXTENT, BIN_OTSU_MAX_PIXELS = 255, 1 << 26
BinarizeTiling = collections.namedtuple("BinarizeTiling", "strip_cols segment_rows direct_trips march_trips staged_cols")


def binarize(imgs, method: int, thr_or_c: int = 0, kw: int = 3, kh: Optional[int] = None, invert: int = 0):
    """Host-only, needs no GPU: the rule on frames uint8 [n_frames, H, W] -> (bit maps uint8 [n_frames, H, ceil(W / 8)] with
    rows MSB-first and pad bits 0, counts int64 [n_frames], thresholds int32 [n_frames]: OTSU t[f], FIXED thr, MEAN c)."""
    a = np.ascontiguousarray(imgs, dtype=np.uint8)
    if a.ndim != 3:
        raise ValueError("expected uint8 [n_frames, H, W]")
    n, h, w = a.shape
    out, counts, thr = np.zeros((n, h, (w + 7) // 8), np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int32)
    _ok(load().canny_hip_binarize(_hp(a), n, h, w, int(method), int(thr_or_c), int(kw), int(kw if kh is None else kh),
                                  int(invert), _hp(out), _hp(counts), _hp(thr)), "binarize")
    return out, counts, thr


def otsu_from_histogram(hist) -> int:
    """Host-only: Otsu's threshold of the rule for a histogram of 256 bins and at most 2^26 samples."""
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    if h.size != 256:
        raise ValueError("expected 256 bins")
    t = C.c_int(-1)
    _ok(load().canny_hip_otsu_from_histogram(_hp(h), C.byref(t)), "otsu_from_histogram")
    return t.value


def binarize_plan(n_frames: int, h: int, w: int, method: int = BIN_ADAPTIVE_MEAN, kw: int = 3, kh: int = 3):
    """Host-only: (LaunchPlan of the launch that writes the bits under the route automatic takes, aux = that route for
    ADAPTIVE_MEAN (1 straightforward, 2 marching; 0 otherwise), BinarizeTiling: the useful columns of a marching strip, the
    rows of a segment for kh, the trips of the straightforward (and FIXED / OTSU) launch, the trips of the marching launch,
    the staged columns of a strip for kw)."""
    plan, *tail = _plan("binarize_plan", int(n_frames), int(h), int(w), int(method), int(kw), int(kh), n=10)
    return plan, BinarizeTiling(*tail)


# ---- thinning of packed bit maps to one-pixel skeletons --------------------------------------------
THIN_ZHANGSUEN, THIN_GUOHALL = 0, 1
THIN_METHODS = ("zhangsuen", "guohall")
THIN_ROUTE_AUTO, THIN_ROUTE_STEPWISE, THIN_ROUTE_FUSED = 0, 1, 2
THIN_MAX_ITERATIONS, THIN_MAX_FUSE, THIN_INFO = 16384, 8, 4
THIN_PARTS = ("passes", "info")


def _thin_maps(bits, w: int):
    a = np.ascontiguousarray(bits, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != (int(w) + 7) // 8:
        raise ValueError("expected bit maps uint8 [n_frames, H, ceil(w / 8)]")
    return a


def thin_bits(bits, w: int, method: int = THIN_GUOHALL, max_iterations: int = 0):
    """Host-only, needs no GPU: the thinning rule on bit maps uint8 [n_frames, H, ceil(w / 8)] (rows MSB-first; pad bits
    ignored) -> (bit maps of the same shape with pad bits 0, info int64 [n_frames, 4]: set bits, iterations, pixels deleted,
    converged)."""
    a = _thin_maps(bits, w)
    n, h, _ = a.shape
    out, info = np.zeros_like(a), np.zeros((n, THIN_INFO), np.int64)
    _ok(load().canny_hip_thin_bits(_hp(a), n, h, int(w), int(method), int(max_iterations), _hp(out), _hp(info)), "thin_bits")
    return out, info


def thin_plan(n_frames: int, h: int, w: int, fuse: int = 0):
    """Host-only: the LaunchPlan of every launch of a thinning call (one tile of 8 words x 64 rows per workgroup and trip);
    aux = the full iterations a launch runs: fuse, or for 0 what automatic takes (0: automatic is the stepwise route)."""
    return _plan("thin_plan", int(n_frames), int(h), int(w), int(fuse))


# ---- morphological reconstruction of packed bit maps ----------------------------------------------
RECON_SEEDED, RECON_FILL_HOLES, RECON_CLEAR_BORDER = 0, 1, 2
RECON_OPS = ("seeded", "fill", "clear")
RECON_ROUTE_AUTO, RECON_ROUTE_STEPWISE, RECON_ROUTE_TILES = 0, 1, 2
RECON_INFO = 3
RECON_PARTS = ("sweeps", "info")


def _recon_maps(marker, mask, w: int, op: int):
    m = _thin_maps(mask, w)
    if (marker is None) != (int(op) != RECON_SEEDED):
        raise ValueError("a marker goes with RECON_SEEDED and with no other op")
    k = None if marker is None else _thin_maps(marker, w)
    if k is not None and k.shape != m.shape:
        raise ValueError("marker and mask differ in shape")
    return k, m


def reconstruct_bits(marker, mask, w: int, op: int = RECON_SEEDED, connectivity: int = 8):
    """Host-only, needs no GPU: the reconstruction rule on bit maps uint8 [n_frames, H, ceil(w / 8)] (rows MSB-first; pad bits
    ignored; marker None unless op is RECON_SEEDED) -> (bit maps of the same shape with pad bits 0, info int64 [n_frames, 3]:
    set bits of the output, of the mask, of the start set)."""
    k, m = _recon_maps(marker, mask, w, op)
    n, h, _ = m.shape
    out, info = np.zeros_like(m), np.zeros((n, RECON_INFO), np.int64)
    _ok(load().canny_hip_reconstruct_bits(None if k is None else _hp(k), _hp(m), n, h, int(w), int(op), int(connectivity),
                                          _hp(out), _hp(info)), "reconstruct_bits")
    return out, info


def reconstruct_plan(n_frames: int, h: int, w: int, route: int = 0):
    """Host-only: the LaunchPlan of the sweep launches of a reconstruction call (route 2: one tile of 8 words x 64 rows per
    workgroup and trip; route 1: 256 words); aux = the route automatic takes."""
    return _plan("reconstruct_plan", int(n_frames), int(h), int(w), int(route))


# ---- grey-level morphology and median filtering of u8 planes ----------------------------------------
(GRAY_ERODE, GRAY_DILATE, GRAY_OPEN, GRAY_CLOSE, GRAY_GRADIENT, GRAY_TOPHAT, GRAY_BLACKHAT, GRAY_MEDIAN) = range(8)
GRAY_OPS = MORPH_OPS + ("median",)
GRAY_BORDER_NEUTRAL, GRAY_BORDER_REPLICATE, GRAY_BORDER_CONSTANT = 0, 1, 2
GRAY_BORDERS = ("neutral", "replicate", "constant")
GRAY_ROUTE_AUTO, GRAY_ROUTE_GENERAL, GRAY_ROUTE_FAST = 0, 1, 2
GRAY_PARTS = ("steps",)


def _gray_planes(imgs):
    a = np.ascontiguousarray(imgs, dtype=np.uint8)
    if a.ndim != 3:
        raise ValueError("expected uint8 [n_frames, H, W]")
    return a


def gray_morph(imgs, op: int, rows, kw: int, kh: int, border_mode: int = GRAY_BORDER_NEUTRAL, border_value: int = 0,
               iterations: int = 1):
    """Host-only, needs no GPU: the grey-level operator on planes uint8 [n_frames, H, W] -> planes of the same shape.  The
    element is the binary morphology's (morph_element); GRAY_MEDIAN takes the full 3 x 3 or 5 x 5 rectangle."""
    a = _gray_planes(imgs)
    n, h, w = a.shape
    r = _morph_rows(rows, kh)
    out = np.zeros_like(a)
    _ok(load().canny_hip_gray_morph(_hp(a), n, h, w, int(op), _hp(r), int(kw), int(kh), int(border_mode), int(border_value),
                                    int(iterations), _hp(out)), "gray_morph")
    return out


def gray_morph_plan(n_frames: int, h: int, w: int, op: int = GRAY_ERODE, kw: int = 3, kh: int = 3):
    """Host-only: the LaunchPlan of one primitive step of the grey-level morphology (one tile of 128 columns x 32 rows per
    workgroup and trip); aux = the route automatic takes for op with a full rectangle of kw x kh (1 general, 2 fast)."""
    return _plan("gray_morph_plan", int(n_frames), int(h), int(w), int(op), int(kw), int(kh))


# ---- image pyramids of u8 planes: pyrDown, pyrUp, whole pyramids ------------------------------------
PYR_MAX_LEVELS = 15
PYR_ROUTE_AUTO, PYR_ROUTE_DIRECT, PYR_ROUTE_TILED = 0, 1, 2
PYR_PART_DOWN, PYR_PART_UP = 0, 1
PYR_PARTS = ("down", "up")


def pyramid_layout(n_frames: int, h: int, w: int, levels: int):
    """Host-only: (info, total_bytes) of the pyramid's one buffer; info int64 [levels, 4]: (h, w, offset, bytes) of level
    l + 1 in row l, every offset a multiple of 256; total_bytes: the end of the last level."""
    info = np.zeros((min(max(int(levels), 1), PYR_MAX_LEVELS), 4), np.int64)   # a refused call writes nothing
    total = np.zeros(1, np.int64)
    _ok(load().canny_hip_pyramid_layout(int(n_frames), int(h), int(w), int(levels), _hp(info), _hp(total)), "pyramid_layout")
    return info, int(total[0])


def _pyramid_levels(buf: np.ndarray, n: int, info: np.ndarray):
    """The levels of a pyramid buffer as views [n, h_l, w_l]."""
    return [buf[off:off + nbytes].reshape(n, hl, wl) for hl, wl, off, nbytes in info.tolist()]


def pyramid(imgs, levels: int):
    """Host-only, needs no GPU: the levels 1..levels of planes uint8 [n_frames, H, W], a list of arrays [n_frames, h_l, w_l]
    (views of one buffer in the layout of pyramid_layout)."""
    a = _gray_planes(imgs)
    n, h, w = a.shape
    info, total = pyramid_layout(n, h, w, levels)
    out = np.zeros(total, np.uint8)
    _ok(load().canny_hip_pyramid(_hp(a), n, h, w, int(levels), _hp(out)), "pyramid")
    return _pyramid_levels(out, n, info)


def pyr_up(imgs, oh: int, ow: int):
    """Host-only, needs no GPU: pyrUp of planes uint8 [n_frames, H, W] to [n_frames, oh, ow], oh in (2 H - 1, 2 H), ow in
    (2 W - 1, 2 W)."""
    a = _gray_planes(imgs)
    n, h, w = a.shape
    out = np.zeros((n, max(int(oh), 0), max(int(ow), 0)), np.uint8)
    _ok(load().canny_hip_pyr_up(_hp(a), n, h, w, int(oh), int(ow), _hp(out)), "pyr_up")
    return out


def pyramid_batch(ctx, imgs, levels: int):
    """ctx.pyramid_batch(imgs, levels)."""
    return ctx.pyramid_batch(imgs, levels)


def pyr_up_batch(ctx, imgs, oh: int, ow: int):
    """ctx.pyr_up_batch(imgs, oh, ow)."""
    return ctx.pyr_up_batch(imgs, oh, ow)


def pyramid_plan(n_frames: int, h: int, w: int):
    """Host-only: the LaunchPlan of one pyrDown of planes [n_frames, h, w] (one tile of 128 columns x 32 rows of the output
    per workgroup and trip; a pyrUp into planes of that output size has the same plan); aux = the route automatic takes."""
    return _plan("pyramid_plan", int(n_frames), int(h), int(w))


# ---- chamfer template matching --------------------------------------------------------------------
MATCH_INTS = 6
CHAMFER_MAX_EXTENT, CHAMFER_MAX_TEMPLATES, CHAMFER_MAX_POINTS, CHAMFER_MAX_TRUNC = 255, 1024, 65536, 4095
CHAMFER_PARTS = ("cost", "score", "candidates", "accept")
CHAMFER_PLANS = ("cost", "cells")
MATCH_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("template", np.int32), ("score", np.int32),
                        ("mean_q12", np.int32), ("base", np.int32)])


def chamfer_csr(templates) -> Tuple[np.ndarray, np.ndarray]:
    """A list of (K_t, 2) integer arrays of (dx, dy) -> (offsets int32 [T + 1], points int16 [sum K_t, 2]), the CSR shape
    the C entry points take.  Values outside int16 raise; the limits of the rule are the library's to check."""
    tpl = [np.asarray(t).reshape(-1, 2) for t in templates]
    off = np.zeros(len(tpl) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in tpl])
    cat = np.concatenate(tpl, axis=0) if tpl else np.zeros((0, 2), np.int64)
    if len(cat) and (cat.min() < -32768 or cat.max() > 32767):
        raise ValueError("template offsets must fit int16")
    return off, np.ascontiguousarray(cat, dtype=np.int16)


def chamfer_template_from_mask(mask, anchor=None) -> np.ndarray:
    """The non-zero pixels of a 2-D mask as template points (dx, dy) int16 [K, 2], in raster order, relative to anchor =
    (x, y); the default anchor is the centre (width // 2, height // 2)."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("expected a 2-D mask")
    ax, ay = (m.shape[1] // 2, m.shape[0] // 2) if anchor is None else (int(anchor[0]), int(anchor[1]))
    ys, xs = np.nonzero(m)
    return np.stack([xs - ax, ys - ay], axis=1).astype(np.int16)


def chamfer_rotations(points, angles_deg) -> list:
    """Host-side input preparation (not part of the rule): the template rotated about its anchor by each angle (degrees,
    counter-clockwise in image coordinates with y down: x' = x cos a + y sin a, y' = -x sin a + y cos a), rounded half
    away from zero to whole pixels and de-duplicated (np.unique order).  -> a list of int16 [K_a, 2] arrays."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    out = []
    for a in angles_deg:
        c, s_ = np.cos(np.deg2rad(float(a))), np.sin(np.deg2rad(float(a)))
        x = pts[:, 0] * c + pts[:, 1] * s_
        y = -pts[:, 0] * s_ + pts[:, 1] * c
        r = np.stack([np.sign(x) * np.floor(np.abs(x) + 0.5), np.sign(y) * np.floor(np.abs(y) + 0.5)], axis=1)
        out.append(np.unique(r.astype(np.int16), axis=0))
    return out


def chamfer_cost_of(d2: int, trunc_q4: int) -> int:
    """Host-only: cost(d2) of the rule = min(isqrt(d2 * 256), trunc_q4)."""
    v = load().canny_hip_chamfer_cost_of(int(d2), int(trunc_q4))
    if v < 0:
        raise CannyHipError(1, "chamfer_cost_of")
    return v


def chamfer_from_dist2(dist2, templates, trunc_q4: int, max_mean_q4: int, min_dist: int = 0, matches_max: int = 256,
                       want_scores: bool = False, csr=None):
    """Host-only, needs no GPU: the chamfer-matching rule on ONE int32 dist2 plane [H, W] with a list of templates (or
    csr = (offsets, points) as they are) -> (matches int32 [k, 6]: x, y, template, score, mean_q12, base; the true
    candidate count; scores uint32 [T, H, W] or None)."""
    d = np.ascontiguousarray(dist2, dtype=np.int32)
    if d.ndim != 2:
        raise ValueError("expected a 2-D dist2 plane")
    off, pts = csr if csr is not None else chamfer_csr(templates)
    off, pts = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.int16)
    h, w = d.shape
    T = len(off) - 1
    rec = np.zeros((max(int(matches_max), 1), MATCH_INTS), np.int32)
    scores = np.zeros((max(T, 1), h, w), np.uint32) if want_scores else None
    n, nc = C.c_int(0), C.c_int(0)
    _ok(load().canny_hip_chamfer_from_dist2(_hp(d), h, w, _hp(off), _hp(pts), T, trunc_q4, max_mean_q4, min_dist,
                                            matches_max, _hp(rec), C.byref(n), C.byref(nc),
                                            _hp(scores) if want_scores else None), "chamfer_from_dist2")
    return rec[:n.value].copy(), nc.value, scores


def chamfer_plan(which, n_frames: int, height: int, width: int, n_templates: int, with_scores: bool = False):
    """Host-only: (LaunchPlan, frames per chunk) of a capped chamfer launch ("cost" or "cells") for a full chunk."""
    k = CHAMFER_PLANS.index(which) if isinstance(which, str) else int(which)
    return _plan("chamfer_plan", k, int(n_frames), int(height), int(width), int(n_templates), int(bool(with_scores)), n=6)


def chamfer_bands(templates, t: int = 0, csr=None) -> Tuple[int, int, int, int]:
    """Host-only: (bands of dy, largest LDS tile of template t in u16, largest of the set, automatic route) of the tiled
    score kernel for a template list."""
    off, pts = csr if csr is not None else chamfer_csr(templates)
    out = np.zeros(4, np.int32)
    _ok(load().canny_hip_selftest_chamfer_bands(_hp(off), _hp(pts), len(off) - 1, int(t), _hp(out)), "selftest_chamfer_bands")
    return tuple(int(v) for v in out)


def points_to_rc(points, width: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pixel indices r * width + c -> (rows, cols), int64 (what np.nonzero(mask) returns for the same map)."""
    p = np.asarray(points).astype(np.int64)
    return p // int(width), p % int(width)


def auto_thresholds_from_histogram(hist, rule="median", low: float = 0.67, high: float = 1.33) -> Tuple[int, int]:
    """Host-only: the automatic rule (AUTO_MEDIAN / AUTO_QUANTILE, or "median" / "quantile") on one 257-bin histogram
    -> (min_val, max_val), exactly as the GPU selects it per frame."""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.shape != (257,):
        raise ValueError(f"expected 257 bins, got shape {h.shape}")
    lo, hi = C.c_int(0), C.c_int(0)
    _ok(load().canny_hip_auto_thresholds_from_histogram(_hp(h), int(rule) if isinstance(rule, (int, np.integer))
                                                        else _rule(rule), low, high, C.byref(lo), C.byref(hi)),
        "auto_thresholds_from_histogram")
    return lo.value, hi.value


def march_order(n_segs: int, n_strips: int) -> np.ndarray:
    """Host-only: the (segment, strip) cell each wave index of a marching launch takes within a frame (border first)."""
    out = np.empty((n_segs * n_strips, 2), np.int32)
    _ok(load().canny_hip_selftest_march_order(n_segs, n_strips, out.ctypes.data_as(C.c_void_p)), "selftest_march_order")
    return out


LaunchPlan = collections.namedtuple("LaunchPlan", "units per_group grid trips aux")


def launch_plan(kind, n_frames: int = 1, height: int = 1, width: int = 1, extra: int = 0) -> "LaunchPlan":
    """Host-only: how the capped grid of a launch divides its work.  kind is a name of PLAN_KINDS
    or its number; extra: the capacity, cell, pair or pixel count of the kinds sized by it, and the points of the frame
    for "hough_vote_points".  units: work items of the launch (of one frame for the Hough and circle votes and the cell passes),
    per_group: items a workgroup takes per trip of its grid-stride loop, grid: workgroups, trips: ceil(units / (grid *
    per_group)) -- 2 or more means some workgroup takes a second item --, aux: rows per wave for "edt_rows", else 0.
    The launchers take their grids from the helpers this reports, so it cannot drift from what runs."""
    k = PLAN_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    return _plan("launch_plan", k, int(n_frames), int(height), int(width), int(extra))


def fma_div_table():
    """The (divisor, c) pairs for which the Gaussian kernels replace a/divisor by fma(a, c, a)."""
    out, k = [], 0
    while True:
        s, c = C.c_float(0), C.c_float(0)
        if load().canny_hip_selftest_div_fma_table(k, C.byref(s), C.byref(c)):
            return out
        out.append((s.value, c.value))
        k += 1


def shard_range(n_frames: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous frame range of shard ``rank`` of ``world`` (pure host logic, no GPU needed)."""
    b, e = C.c_int(0), C.c_int(0)
    _ok(load().canny_hip_shard_range(n_frames, rank, world, C.byref(b), C.byref(e)), "canny_hip_shard_range")
    return b.value, e.value


def _hp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _u8(img) -> np.ndarray:
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("expected a 2-D uint8 image")
    return a


def _frame(img, order: str, batch: bool = False) -> Tuple[np.ndarray, int]:
    a = np.ascontiguousarray(img, dtype=np.uint8)
    return a, layout_of(a.shape, order, batch)


def _s16(img) -> np.ndarray:
    a = np.ascontiguousarray(img, dtype=np.int16)
    if a.ndim != 2:
        raise ValueError("expected a 2-D int16 plane")
    return a


class Context:
    """One GPU, one stream, reusable device workspaces (``canny_hip_ctx``)."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        _ok(self._L.canny_hip_ctx_create(C.byref(h), device), "canny_hip_ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):
                self._L.canny_hip_host_free(self._h, C.c_void_p(p))
            self._pinned = []
            self._L.canny_hip_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int, what: str):
        if st:
            raise CannyHipError(st, what, self._L.canny_hip_last_error(self._h).decode())

    # ---- plumbing ---------------------------------------------------------------------------
    @property
    def device(self) -> int:
        return self._L.canny_hip_ctx_device(self._h)

    def set_stream(self, hip_stream: int):
        """Launch on a caller-owned hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        self._check(self._L.canny_hip_ctx_set_stream(self._h, C.c_void_p(hip_stream)), "set_stream")

    def set_option(self, name: str, value: int):
        """Kernel-path selection ("gaussian_path" / "sobel_nms_path": 0 auto, 1 baseline, 2 wave-marching)."""
        self._check(self._L.canny_hip_ctx_set_option(self._h, name.encode(), value), f"set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        self._check(self._L.canny_hip_ctx_get_option(self._h, name.encode(), C.byref(v)), f"get_option({name})")
        return v.value

    def synchronize(self):
        self._check(self._L.canny_hip_synchronize(self._h), "synchronize")

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._L.canny_hip_malloc(self._h, C.byref(p), nbytes), "malloc")
        return p.value

    def free(self, dptr: int):
        self._check(self._L.canny_hip_free(self._h, C.c_void_p(dptr)), "free")

    def h2d(self, dptr: int, host: np.ndarray):
        host = np.ascontiguousarray(host)
        self._check(self._L.canny_hip_memcpy_h2d(self._h, C.c_void_p(dptr), _hp(host), host.nbytes), "h2d")

    def d2h(self, host: np.ndarray, dptr: int):
        assert host.flags["C_CONTIGUOUS"]
        self._check(self._L.canny_hip_memcpy_d2h(self._h, _hp(host), C.c_void_p(dptr), host.nbytes), "d2h")

    @property
    def last_hysteresis_iterations(self) -> int:
        return self._L.canny_hip_last_hysteresis_iterations(self._h)

    def profile_enable(self, on: bool = True):
        self._check(self._L.canny_hip_profile_enable(self._h, int(on)), "profile_enable")

    def profile_reset(self):
        self._check(self._L.canny_hip_profile_reset(self._h), "profile_reset")

    def _profile_part(self, fn_name: str, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of one slot through canny_hip_<fn_name>: what every *_profile_get method returns."""
        ms, n = C.c_double(0), C.c_long(0)
        self._check(getattr(self._L, "canny_hip_" + fn_name)(self._h, part, C.byref(ms), C.byref(n)), fn_name)
        return ms.value, n.value

    def profile_get(self, stage: int) -> Tuple[float, int]:
        return self._profile_part("profile_get", stage)

    # ---- host-array stage API -----------------------------------------------------------------
    def gaussian(self, img, sigma: float) -> np.ndarray:
        a = _u8(img)
        out = np.empty(a.shape, np.int16)
        self._check(self._L.canny_hip_gaussian(self._h, _hp(a), sigma, a.shape[0], a.shape[1], _hp(out)), "gaussian")
        return out

    def xy_gradient(self, img) -> Tuple[np.ndarray, np.ndarray]:
        a = _s16(img)
        gx, gy = np.empty(a.shape, np.int16), np.empty(a.shape, np.int16)
        self._check(self._L.canny_hip_xy_gradient(self._h, _hp(a), a.shape[0], a.shape[1], _hp(gx), _hp(gy)),
                    "xy_gradient")
        return gx, gy

    def sobel(self, img) -> Tuple[np.ndarray, np.ndarray]:
        a = _s16(img)
        mag, ang = np.empty(a.shape, np.int16), np.empty(a.shape, np.int16)
        self._check(self._L.canny_hip_sobel(self._h, _hp(a), a.shape[0], a.shape[1], _hp(mag), _hp(ang)), "sobel")
        return mag, ang

    def nms(self, mag, ang) -> np.ndarray:
        m, a = _s16(mag), _s16(ang)
        if m.shape != a.shape:
            raise ValueError("magnitude/angle shape mismatch")
        out = np.empty(m.shape, np.int16)
        self._check(self._L.canny_hip_nms(self._h, _hp(m), _hp(a), m.shape[0], m.shape[1], _hp(out)), "nms")
        return out

    def hysteresis(self, cand, min_val: int, max_val: int) -> np.ndarray:
        c = _s16(cand).copy()
        self._check(self._L.canny_hip_hysteresis(self._h, _hp(c), c.shape[0], c.shape[1], min_val, max_val),
                    "hysteresis")
        return c

    def find_edge_pixels(self, cand, visited, start: int, min_val: int, max_val: int):
        c = _s16(cand).copy()
        v = np.ascontiguousarray(visited, dtype=np.uint8).copy()
        self._check(self._L.canny_hip_find_edge_pixels(self._h, _hp(c), _hp(v), start, min_val, max_val, c.shape[0],
                                                       c.shape[1]), "find_edge_pixels")
        return c, v

    def canny(self, img, sigma: float, min_val: int, max_val: int) -> np.ndarray:
        a = _u8(img)
        out = np.empty(a.shape, np.int16)
        self._check(self._L.canny_hip_canny(self._h, _hp(a), sigma, min_val, max_val, a.shape[0], a.shape[1],
                                            _hp(out)), "canny")
        return out

    def pinned_array(self, shape, dtype) -> np.ndarray:
        """numpy array over page-locked host memory (canny_hip_host_alloc); freed when the context closes.
        canny_batch DMA's pinned inputs/outputs in place instead of staging them."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._check(self._L.canny_hip_host_alloc(self._h, C.byref(p), nbytes), "host_alloc")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def host_register(self, a: np.ndarray):
        """Page-lock an ordinary (C-contiguous) numpy array in place: canny_batch then DMA's it like pinned memory."""
        assert a.flags["C_CONTIGUOUS"]
        self._check(self._L.canny_hip_host_register(self._h, _hp(a), a.nbytes), "host_register")

    def host_unregister(self, a: np.ndarray):
        self._check(self._L.canny_hip_host_unregister(self._h, _hp(a)), "host_unregister")

    def canny_batch(self, imgs, sigma: float, min_val: int, max_val: int, out: Optional[np.ndarray] = None,
                    u8: bool = False, bits: bool = False) -> np.ndarray:
        """Host frames in, host edge maps out, transfers overlapped with the kernels.  u8=True returns the maps as
        uint8 (0 / 255) instead of the reference's int16: a third less PCIe traffic.  bits=True returns bit maps,
        uint8 [n_frames, H, (W + 7) // 8], rows packed MSB-first like numpy.packbits (see unpack_bits())."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError("expected uint8 [n_frames, H, W]")
        dtype = np.uint8 if (u8 or bits) else np.int16
        shape = bits_shape(a.shape) if bits else a.shape
        if out is None:
            out = np.empty(shape, dtype)
        elif out.shape != shape or out.dtype != dtype or not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"out must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        fn = self._L.canny_hip_canny_batch_bits if bits else \
            (self._L.canny_hip_canny_batch_u8 if u8 else self._L.canny_hip_canny_batch)
        self._check(fn(self._h, _hp(a), a.shape[0], sigma, min_val, max_val, a.shape[1], a.shape[2], _hp(out)),
                    "canny_batch")
        return out

    # ---- per-frame thresholds (explicit, or chosen on the GPU: DESIGN.md section 11) ------------------------------
    def canny_thresholds(self, imgs, sigma: float, thresholds, out: Optional[np.ndarray] = None) -> np.ndarray:
        """canny() with a pair per frame: imgs (H, W) or (N, H, W) uint8, thresholds (N, 2) -- or (2,) for one frame --
        with 1 <= min_val <= max_val <= 255 (else CANNY_HIP_ERR_INVALID and nothing is written).  Returns int16 maps
        shaped like imgs."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        single = a.ndim == 2
        if single:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        t = np.ascontiguousarray(thresholds, dtype=np.int32).reshape(-1)
        if t.size != 2 * a.shape[0]:
            raise ValueError(f"expected {a.shape[0]} (min_val, max_val) pairs, got {t.size} values")
        if out is None:
            out = np.empty(a.shape, np.int16)
        self._check(self._L.canny_hip_canny_batch_thresholds(self._h, _hp(a), a.shape[0], sigma, _hp(t), a.shape[1],
                                                             a.shape[2], _hp(out)), "canny_thresholds")
        return out[0] if single else out

    def canny_auto(self, imgs, sigma: float, rule="median", low: float = 0.67, high: float = 1.33):
        """canny() with thresholds chosen per frame on the GPU: rule "median" (auto_canny: low / high times the median
        of the smoothed frame) or "quantile" (low / high quantiles of the gradient magnitude).  imgs (H, W) or
        (N, H, W) uint8.  Returns (edges int16 shaped like imgs, thresholds int32 [N, 2] -- [2] for one frame)."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        single = a.ndim == 2
        if single:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        out = np.empty(a.shape, np.int16)
        thr = np.empty((a.shape[0], 2), np.int32)
        self._check(self._L.canny_hip_canny_batch_auto(self._h, _hp(a), a.shape[0], sigma, _rule(rule), low, high,
                                                       a.shape[1], a.shape[2], _hp(out), _hp(thr)), "canny_auto")
        return (out[0], thr[0]) if single else (out, thr)

    def dev_canny_thresholds(self, d_img: int, sigma: float, d_thresholds: int, h: int, w: int, n: int, d_edges: int):
        """dev_canny with per-frame pairs from a device array of 2 * n int32 (clamped into the domain)."""
        self._check(self._L.canny_hip_dev_canny_thresholds(self._h, C.c_void_p(d_img), sigma, C.c_void_p(d_thresholds),
                                                           h, w, n, C.c_void_p(d_edges)), "dev_canny_thresholds")

    def dev_canny_auto(self, d_img: int, sigma: float, rule, low: float, high: float, h: int, w: int, n: int,
                       d_edges: int, d_thresholds: int = 0):
        """dev_canny with pairs chosen per frame on the GPU; d_thresholds (2 * n int32, device) receives them if set."""
        self._check(self._L.canny_hip_dev_canny_auto(self._h, C.c_void_p(d_img), sigma, _rule(rule), low, high, h, w,
                                                     n, C.c_void_p(d_edges), C.c_void_p(d_thresholds or None)),
                    "dev_canny_auto")

    # ---- edge point lists (CSR of pixel indices r * width + c) ----------------------------
    def canny_points(self, imgs, sigma: float, min_val: int, max_val: int, capacity: Optional[int] = None):
        """canny() returning the edge pixels as index lists: imgs (H, W) or (N, H, W) uint8 ->
        (points uint32 [total], offsets uint64 [N + 1]); frame f's pixels are points[offsets[f]:offsets[f + 1]], ascending
        -- np.flatnonzero(canny(frame f)).  capacity=None sizes the buffer itself and never returns a truncated list (a
        batch denser than one pixel in eight runs twice); with a capacity, points holds the first
        min(offsets[-1], capacity) entries and offsets still holds the true counts."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets = np.zeros(n + 1, np.uint64)
        cap = max(1024, a.size // 8) if capacity is None else int(capacity)
        while True:
            pts = np.empty(cap, np.uint32)
            self._check(self._L.canny_hip_canny_points(self._h, _hp(a), n, sigma, min_val, max_val, h, w,
                                                       _hp(pts) if cap else None, cap, _hp(offsets)), "canny_points")
            total = int(offsets[-1])
            if capacity is not None or total <= cap:
                return pts[:min(total, cap)], offsets
            cap = total

    def dev_canny_points(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                         d_points: int, capacity: int, d_offsets: int, d_edges: int = 0):
        """dev_canny, then its map compacted to index lists on the same stream: d_points (capacity uint32, device; 0 with
        capacity 0 = counts only), d_offsets (n + 1 uint64, device), d_edges (the s16 map, device) or 0."""
        self._check(self._L.canny_hip_dev_canny_points(self._h, C.c_void_p(d_img), sigma, min_val, max_val, h, w, n,
                                                       C.c_void_p(d_edges or None), C.c_void_p(d_points or None),
                                                       capacity, C.c_void_p(d_offsets)), "dev_canny_points")

    def dev_points_from_bits(self, d_bits: int, h: int, w: int, n: int, d_points: int, capacity: int, d_offsets: int):
        """The compaction alone on device bit maps (layout of dev_canny_bits, any byte alignment)."""
        self._check(self._L.canny_hip_dev_points_from_bits(self._h, C.c_void_p(d_bits), h, w, n,
                                                           C.c_void_p(d_points or None), capacity,
                                                           C.c_void_p(d_offsets)), "dev_points_from_bits")

    # ---- sub-pixel edgels (one 16-byte record per edge pixel) -----------------------------
    def canny_edgels(self, imgs, sigma: float, min_val: int, max_val: int, capacity: Optional[int] = None,
                     want_points: bool = False):
        """canny() returning one edgel record per edge pixel: imgs (H, W) or (N, H, W) uint8 -> (edgels int32 [total, 4],
        offsets uint64 [N + 1]) and, with want_points, the pixel indices as canny_points returns them.  Records are in
        canny_points' order; unpack them with edgels_xy / edgels_gradient / edgels_magnitude / edgels_flags.  capacity as
        in canny_points."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets = np.zeros(n + 1, np.uint64)
        cap = max(1024, a.size // 8) if capacity is None else int(capacity)
        while True:
            rec = np.empty((cap, EDGEL_INTS), np.int32)
            pts = np.empty(cap, np.uint32) if want_points else None
            self._check(self._L.canny_hip_canny_edgels(self._h, _hp(a), n, sigma, min_val, max_val, h, w,
                                                       _hp(rec) if cap else None, cap, _hp(offsets),
                                                       _hp(pts) if want_points and cap else None), "canny_edgels")
            total = int(offsets[-1])
            if capacity is not None or total <= cap:
                fit = min(total, cap)
                return (rec[:fit], offsets, pts[:fit]) if want_points else (rec[:fit], offsets)
            cap = total

    def dev_canny_edgels(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                         d_edgels: int, capacity: int, d_offsets: int, d_edges: int = 0, d_points: int = 0):
        """dev_canny, then one record per edge pixel on the same stream: d_edgels (capacity records of 4 int32, device,
        16-byte aligned; 0 with capacity 0 for counts only), d_offsets (N + 1 uint64, device), d_edges (the s16 map) or 0,
        d_points (capacity uint32: the indices dev_canny_points would write) or 0."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_edgels(self._h, v(d_img), sigma, min_val, max_val, h, w, n,
                                                       v(d_edges or None), v(d_edgels or None), capacity, v(d_offsets),
                                                       v(d_points or None)), "dev_canny_edgels")

    def dev_edgels_at(self, d_plane: int, plane_is_u8: bool, h: int, w: int, n: int, d_points: int, d_point_offsets: int,
                      d_edgels: int, capacity: int):
        """The edgel rule at listed pixels: record q describes index d_points[q] (uint32 / int32, device) of the frame whose
        range in d_point_offsets (N + 1 uint64, device) holds q.  d_plane: N planes of h x w bytes (plane_is_u8) or shorts,
        or 0 for the smoothed plane the last dev_canny-family call on this context left (same n, h, w only)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_edgels_at(self._h, v(d_plane or None), int(plane_is_u8), h, w, n,
                                                    v(d_points or None), v(d_point_offsets or None), v(d_edgels or None),
                                                    capacity), "dev_edgels_at")

    def dev_edgels_arith(self, d_gx: int, d_gy: int, n_pairs: int, d_mag: int, d_dir: int, d_abc: int = 0,
                         n_triples: int = 0, d_t: int = 0, d_refined: int = 0):
        """Test hook: the kernels' device arithmetic on arrays (pairs -> mag_q4, dir; (a, b, c) triples -> t_q8, refined)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_edgels_arith(self._h, v(d_gx or None), v(d_gy or None), n_pairs,
                                                       v(d_mag or None), v(d_dir or None), v(d_abc or None), n_triples,
                                                       v(d_t or None), v(d_refined or None)), "dev_edgels_arith")

    def edgels_profile_get(self, part: int) -> Tuple[float, int]:
        return self._profile_part("edgels_profile_get", part)

    # ---- connected components of the finished map ----------------------------------------
    def canny_components(self, imgs, sigma: float, min_val: int, max_val: int, min_area: int = 1,
                         want_labels: bool = True, want_kept: bool = False, capacity: Optional[int] = None):
        """canny(), then the 8-connected components of each map with at least min_area pixels, numbered 1..K_f by
        ascending first pixel: imgs (H, W) or (N, H, W) uint8 -> (labels int32 [N, H, W] or None, kept uint8 [N, H, W] or
        None, stats int32 [total, 6], offsets uint64 [N + 1]); the record of label k of frame f is stats[offsets[f] + k - 1]
        = (left, top, width, height, area, first).  capacity=None never returns a truncated table (a batch with more
        components than one per 64 pixels runs twice); with a capacity, stats holds the first min(offsets[-1], capacity)
        records and offsets still holds the true counts."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets = np.zeros(n + 1, np.uint64)
        labels = np.empty((n, h, w), np.int32) if want_labels else None
        kept = np.empty((n, h, w), np.uint8) if want_kept else None
        cap = max(1024, a.size // 64) if capacity is None else int(capacity)
        while True:
            stats = np.empty((cap, CC_STATS), np.int32)
            self._check(self._L.canny_hip_canny_components(
                self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_area, _hp(labels) if want_labels else None,
                _hp(kept) if want_kept else None, _hp(stats) if cap else None, cap, _hp(offsets)), "canny_components")
            total = int(offsets[-1])
            if capacity is not None or total <= cap:
                return labels, kept, stats[:min(total, cap)], offsets
            cap = total

    def dev_canny_components(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                             min_area: int, d_labels: int, d_kept_u8: int, d_stats: int, capacity: int, d_offsets: int,
                             d_edges: int = 0):
        """dev_canny, then its map labelled on the same stream: d_labels (n*h*w int32), d_kept_u8 (n*h*w uint8), d_stats
        (capacity records of 6 int32) -- each a device pointer or 0 --, d_offsets (n + 1 uint64, device), d_edges (the
        s16 map, device) or 0."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_components(self._h, v(d_img), sigma, min_val, max_val, h, w, n,
                                                           v(d_edges or None), min_area, v(d_labels or None),
                                                           v(d_kept_u8 or None), v(d_stats or None), capacity,
                                                           v(d_offsets or None)), "dev_canny_components")

    def dev_components_bits(self, d_bits: int, h: int, w: int, n: int, min_area: int, d_labels: int, d_kept_u8: int,
                            d_stats: int, capacity: int, d_offsets: int):
        """The labelling alone on device bit maps (layout of dev_canny_bits, any byte alignment, padding ignored)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_components_bits(self._h, v(d_bits or None), h, w, n, min_area,
                                                          v(d_labels or None), v(d_kept_u8 or None), v(d_stats or None),
                                                          capacity, v(d_offsets or None)), "dev_components_bits")

    def components_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 link, 1 resolve, 2 number, 3 write (CC_PARTS)."""
        return self._profile_part("components_profile_get", part)

    # ---- outer contour chains of the finished map ----------------------------------------
    def canny_contours(self, imgs, sigma: float, min_val: int, max_val: int, min_area: int = 1, want_stats: bool = True,
                       capacity: Optional[int] = None, point_capacity: Optional[int] = None):
        """canny(), then the outer contour chain of every component of each map with at least min_area pixels: imgs
        (H, W) or (N, H, W) uint8 -> (stats int32 [k, 6] or None, offsets uint64 [N + 1], chain_offsets uint64 [k + 1],
        points int32, point_offsets uint64 [N + 1]).  Record j (offsets[f] <= j < offsets[f + 1] for frame f) has the chain
        points[chain_offsets[j] : chain_offsets[j + 1]], pixel indices r * W + c in the order of the walk.  With both
        capacities None a counts-only call sizes the buffers and everything is returned; otherwise k = min(offsets[-1],
        capacity), points holds the positions below point_capacity of those records, and offsets / point_offsets still hold
        the true counts."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets, point_offsets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)

        def call(stats, cap, chain, points, pcap):
            self._check(self._L.canny_hip_canny_contours(
                self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_area, _hp(stats) if stats is not None and cap else None,
                cap, _hp(offsets), _hp(chain) if chain is not None else None, _hp(points) if pcap else None, pcap,
                _hp(point_offsets)), "canny_contours")

        if capacity is None or point_capacity is None:
            call(None, 0, None, None, 0)
        cap = int(offsets[-1]) if capacity is None else int(capacity)
        pcap = int(point_offsets[-1]) if point_capacity is None else int(point_capacity)
        stats = np.empty((cap, CC_STATS), np.int32) if want_stats else None
        chain = np.zeros(cap + 1, np.uint64)
        points = np.empty(pcap, np.int32)
        call(stats, cap, chain, points, pcap)
        fit = min(cap, int(offsets[-1]))
        return (stats[:fit] if want_stats else None, offsets, chain[:fit + 1], points[:min(pcap, int(chain[fit]))],
                point_offsets)

    def dev_canny_contours(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                           min_area: int, d_stats: int, capacity: int, d_offsets: int, d_chain_offsets: int, d_points: int,
                           point_capacity: int, d_point_offsets: int, d_edges: int = 0):
        """dev_canny, then the chains of its map on the same stream: d_stats (capacity records of 6 int32) or 0,
        d_offsets and d_point_offsets (n + 1 uint64 each), d_chain_offsets (capacity + 1 uint64) or 0 with capacity 0,
        d_points (point_capacity int32) or 0 with point_capacity 0, d_edges (the s16 map) or 0 -- device pointers."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_contours(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                         v(d_edges or None), min_area, v(d_stats or None), capacity,
                                                         v(d_offsets or None), v(d_chain_offsets or None),
                                                         v(d_points or None), point_capacity, v(d_point_offsets or None)),
                    "dev_canny_contours")

    def dev_contours_bits(self, d_bits: int, h: int, w: int, n: int, min_area: int, d_stats: int, capacity: int,
                          d_offsets: int, d_chain_offsets: int, d_points: int, point_capacity: int, d_point_offsets: int):
        """The chains alone on device bit maps (layout of dev_canny_bits, any byte alignment, padding ignored)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_contours_bits(self._h, v(d_bits or None), h, w, n, min_area, v(d_stats or None),
                                                        capacity, v(d_offsets or None), v(d_chain_offsets or None),
                                                        v(d_points or None), point_capacity, v(d_point_offsets or None)),
                    "dev_contours_bits")

    def contours_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 label, 1 count, 2 write, 3 stats (CONTOUR_PARTS)."""
        return self._profile_part("contours_profile_get", part)

    # ---- edge curves: the map linked into ordered chains ------------------------------------
    def canny_curves(self, imgs, sigma: float, min_val: int, max_val: int, min_length: int = 1, want_records: bool = True,
                     capacity: Optional[int] = None, point_capacity: Optional[int] = None):
        """canny(), then the edge curves of each map with at least min_length points: imgs (H, W) or (N, H, W) uint8 ->
        (records int32 [k, 4] or None, offsets uint64 [N + 1], chain_offsets uint64 [k + 1], points int32, point_offsets
        uint64 [N + 1]).  Record j (offsets[f] <= j < offsets[f + 1] for frame f) is (start, end, points, flags) and has the
        points points[chain_offsets[j] : chain_offsets[j + 1]], pixel indices r * W + c along the curve.  With both
        capacities None a counts-only call sizes the buffers and everything is returned; otherwise k = min(offsets[-1],
        capacity), points holds the positions below point_capacity of those records, and offsets / point_offsets still hold
        the true counts."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets, point_offsets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)

        def call(records, cap, chain, points, pcap):
            self._check(self._L.canny_hip_canny_curves(
                self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_length,
                _hp(records) if records is not None and cap else None, cap, _hp(offsets),
                _hp(chain) if chain is not None else None, _hp(points) if pcap else None, pcap, _hp(point_offsets)),
                "canny_curves")

        if capacity is None or point_capacity is None:
            call(None, 0, None, None, 0)
        cap = int(offsets[-1]) if capacity is None else int(capacity)
        pcap = int(point_offsets[-1]) if point_capacity is None else int(point_capacity)
        records = np.empty((cap, CURVE_RECORD), np.int32) if want_records else None
        chain = np.zeros(cap + 1, np.uint64)
        points = np.empty(pcap, np.int32)
        call(records, cap, chain, points, pcap)
        fit = min(cap, int(offsets[-1]))
        return (records[:fit] if want_records else None, offsets, chain[:fit + 1], points[:min(pcap, int(chain[fit]))],
                point_offsets)

    def dev_canny_curves(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                         min_length: int, d_records: int, capacity: int, d_offsets: int, d_chain_offsets: int,
                         d_points: int, point_capacity: int, d_point_offsets: int, d_edges: int = 0):
        """dev_canny, then the curves of its map on the same stream: d_records (capacity records of 4 int32) or 0,
        d_offsets and d_point_offsets (n + 1 uint64 each), d_chain_offsets (capacity + 1 uint64) or 0 with capacity 0,
        d_points (point_capacity int32) or 0 with point_capacity 0, d_edges (the s16 map) or 0 -- device pointers."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_curves(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                       v(d_edges or None), min_length, v(d_records or None), capacity,
                                                       v(d_offsets or None), v(d_chain_offsets or None),
                                                       v(d_points or None), point_capacity, v(d_point_offsets or None)),
                    "dev_canny_curves")

    def dev_curves_bits(self, d_bits: int, h: int, w: int, n: int, min_length: int, d_records: int, capacity: int,
                        d_offsets: int, d_chain_offsets: int, d_points: int, point_capacity: int, d_point_offsets: int):
        """The curves alone on device bit maps (layout of dev_canny_bits, any byte alignment, padding ignored)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_curves_bits(self._h, v(d_bits or None), h, w, n, min_length,
                                                      v(d_records or None), capacity, v(d_offsets or None),
                                                      v(d_chain_offsets or None), v(d_points or None), point_capacity,
                                                      v(d_point_offsets or None)), "dev_curves_bits")

    def curves_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 count, 1 write (CURVE_PARTS)."""
        return self._profile_part("curves_profile_get", part)

    # ---- polygon approximation of the contour chains ---------------------------------------
    def canny_polygons(self, imgs, sigma: float, min_val: int, max_val: int, min_area: int = 1, epsilon: float = 0.0,
                       ratio: float = 0.0, want_stats: bool = False, want_points: bool = False):
        """canny(), the outer contour chains, then the polygon of every chain: imgs (H, W) or (N, H, W) uint8 ->
        (polygons, measures int64 [K, 4], offsets uint64 [N + 1], extra).  polygons is a list of K int32 arrays, views into
        one vertex array through the CSR, record j (offsets[f] <= j < offsets[f + 1] for frame f) holding its vertices as
        pixel indices r * W + c in chain order; measures[j] = (vertices, length_q8, area2, convex).  epsilon (pixels) and
        ratio (of the chain's length; 0.02 is the usual choice) are rounded to 1/256 and 1/65536 and add.  extra is a dict
        with vertex_offsets, vertices, point_offsets, and stats / chain_offsets, points when asked for.  Unless
        want_points, the chains never leave the device."""
        eq, rq = polygon_tolerance(epsilon, ratio)
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets, point_offsets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        sized = self.canny_contours(a, sigma, min_val, max_val, min_area, want_stats=False, capacity=0, point_capacity=0)
        cap, pcap = int(sized[1][-1]), int(sized[4][-1])
        stats = np.empty((cap, CC_STATS), np.int32) if want_stats else None
        chain = np.zeros(cap + 1, np.uint64)
        points = np.empty(pcap, np.int32) if want_points else None
        voff = np.zeros(cap + 1, np.uint64)
        verts = np.empty(pcap, np.int32)   # a polygon has no more vertices than its chain has points
        measures = np.zeros((cap, 4), np.int64)
        self._check(self._L.canny_hip_canny_polygons(
            self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_area, _hp(stats) if want_stats and cap else None, cap,
            _hp(offsets), _hp(chain), _hp(points) if want_points and pcap else None, pcap, _hp(point_offsets), eq, rq,
            _hp(voff), _hp(verts) if pcap else None, pcap, _hp(measures) if cap else None), "canny_polygons")
        verts = verts[:int(voff[-1])]
        polygons = [verts[int(voff[j]):int(voff[j + 1])] for j in range(cap)]
        extra = dict(vertex_offsets=voff, vertices=verts, point_offsets=point_offsets, chain_offsets=chain)
        if want_stats:
            extra["stats"] = stats
        if want_points:
            extra["points"] = points
        return polygons, measures, offsets, extra

    def dev_polygons_chains(self, d_offsets: int, n: int, capacity: int, d_chain_offsets: int, d_points: int,
                            point_capacity: int, w: int, h: int, epsilon_q8: int, ratio_q16: int, d_vertex_offsets: int,
                            d_vertices: int, vertex_capacity: int, d_measures: int = 0):
        """The polygon stage alone on chains a contours call left on the device: d_vertex_offsets (capacity + 1 uint64),
        d_vertices (vertex_capacity int32) or 0 with vertex_capacity 0, d_measures (capacity x 4 int64) or 0."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_polygons_chains(self._h, v(d_offsets or None), n, capacity,
                                                          v(d_chain_offsets or None), v(d_points or None), point_capacity,
                                                          w, h, epsilon_q8, ratio_q16, v(d_vertex_offsets or None),
                                                          v(d_vertices or None), vertex_capacity, v(d_measures or None)),
                    "dev_polygons_chains")

    def dev_canny_polygons(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                           min_area: int, d_stats: int, capacity: int, d_offsets: int, d_chain_offsets: int, d_points: int,
                           point_capacity: int, d_point_offsets: int, epsilon_q8: int, ratio_q16: int,
                           d_vertex_offsets: int, d_vertices: int, vertex_capacity: int, d_measures: int = 0,
                           d_edges: int = 0):
        """dev_canny_contours (same arguments), then the polygon stage on what it stored, on the same stream."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_polygons(
            self._h, v(d_img or None), sigma, min_val, max_val, h, w, n, v(d_edges or None), min_area, v(d_stats or None),
            capacity, v(d_offsets or None), v(d_chain_offsets or None), v(d_points or None), point_capacity,
            v(d_point_offsets or None), epsilon_q8, ratio_q16, v(d_vertex_offsets or None), v(d_vertices or None),
            vertex_capacity, v(d_measures or None)), "dev_canny_polygons")

    def dev_polygons_bits(self, d_bits: int, h: int, w: int, n: int, min_area: int, d_stats: int, capacity: int,
                          d_offsets: int, d_chain_offsets: int, d_points: int, point_capacity: int, d_point_offsets: int,
                          epsilon_q8: int, ratio_q16: int, d_vertex_offsets: int, d_vertices: int, vertex_capacity: int,
                          d_measures: int = 0):
        """dev_contours_bits (same arguments), then the polygon stage on what it stored."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_polygons_bits(
            self._h, v(d_bits or None), h, w, n, min_area, v(d_stats or None), capacity, v(d_offsets or None),
            v(d_chain_offsets or None), v(d_points or None), point_capacity, v(d_point_offsets or None), epsilon_q8,
            ratio_q16, v(d_vertex_offsets or None), v(d_vertices or None), vertex_capacity, v(d_measures or None)),
            "dev_polygons_bits")

    def polygons_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 simplify, 1 scan, 2 emit (POLYGON_PARTS)."""
        return self._profile_part("polygons_profile_get", part)

    # ---- contour shape measures ------------------------------------------------------------
    def canny_shapes(self, imgs, sigma: float, min_val: int, max_val: int, min_area: int = 1, want_stats: bool = False,
                     want_points: bool = False):
        """canny(), the outer contour chains, then the shape measures of every chain: imgs (H, W) or (N, H, W) uint8 ->
        (hulls, measures int64 [K, 20], offsets uint64 [N + 1], extra).  hulls is a list of K int32 arrays, views into one
        array through the CSR, record j (offsets[f] <= j < offsets[f + 1] for frame f) holding its convex hull as pixel
        indices r * W + c; measures[j] holds the words named in SHAPE_MEASURES.  extra is a dict with hull_offsets, hull,
        point_offsets, chain_offsets, and stats / points when asked for.  Unless want_points, the chains never leave the
        device."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        offsets, point_offsets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        sized = self.canny_contours(a, sigma, min_val, max_val, min_area, want_stats=False, capacity=0, point_capacity=0)
        cap, pcap = int(sized[1][-1]), int(sized[4][-1])
        stats = np.empty((cap, CC_STATS), np.int32) if want_stats else None
        chain = np.zeros(cap + 1, np.uint64)
        points = np.empty(pcap, np.int32) if want_points else None
        hoff = np.zeros(cap + 1, np.uint64)
        hull = np.empty(pcap, np.int32)   # a hull has no more vertices than its chain has points
        measures = np.zeros((cap, SHAPE_WORDS), np.int64)
        self._check(self._L.canny_hip_canny_shapes(
            self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_area, _hp(stats) if want_stats and cap else None, cap,
            _hp(offsets), _hp(chain), _hp(points) if want_points and pcap else None, pcap, _hp(point_offsets),
            _hp(hoff), _hp(hull) if pcap else None, pcap, _hp(measures) if cap else None), "canny_shapes")
        hull = hull[:int(hoff[-1])]
        hulls = [hull[int(hoff[j]):int(hoff[j + 1])] for j in range(cap)]
        extra = dict(hull_offsets=hoff, hull=hull, point_offsets=point_offsets, chain_offsets=chain)
        if want_stats:
            extra["stats"] = stats
        if want_points:
            extra["points"] = points
        return hulls, measures, offsets, extra

    def dev_shapes_chains(self, d_offsets: int, n: int, capacity: int, d_chain_offsets: int, d_points: int,
                          point_capacity: int, w: int, h: int, d_hull_offsets: int, d_hull: int, hull_capacity: int,
                          d_measures: int = 0):
        """The shape stage alone on chains a contours call left on the device: d_hull_offsets (capacity + 1 uint64), d_hull
        (hull_capacity int32) or 0 with hull_capacity 0, d_measures (capacity x 20 int64) or 0."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_shapes_chains(self._h, v(d_offsets or None), n, capacity,
                                                        v(d_chain_offsets or None), v(d_points or None), point_capacity,
                                                        w, h, v(d_hull_offsets or None), v(d_hull or None), hull_capacity,
                                                        v(d_measures or None)), "dev_shapes_chains")

    def dev_canny_shapes(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                         min_area: int, d_stats: int, capacity: int, d_offsets: int, d_chain_offsets: int, d_points: int,
                         point_capacity: int, d_point_offsets: int, d_hull_offsets: int, d_hull: int, hull_capacity: int,
                         d_measures: int = 0, d_edges: int = 0):
        """dev_canny_contours (same arguments), then the shape stage on what it stored, on the same stream."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_shapes(
            self._h, v(d_img or None), sigma, min_val, max_val, h, w, n, v(d_edges or None), min_area, v(d_stats or None),
            capacity, v(d_offsets or None), v(d_chain_offsets or None), v(d_points or None), point_capacity,
            v(d_point_offsets or None), v(d_hull_offsets or None), v(d_hull or None), hull_capacity,
            v(d_measures or None)), "dev_canny_shapes")

    def dev_shapes_bits(self, d_bits: int, h: int, w: int, n: int, min_area: int, d_stats: int, capacity: int,
                        d_offsets: int, d_chain_offsets: int, d_points: int, point_capacity: int, d_point_offsets: int,
                        d_hull_offsets: int, d_hull: int, hull_capacity: int, d_measures: int = 0):
        """dev_contours_bits (same arguments), then the shape stage on what it stored."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_shapes_bits(
            self._h, v(d_bits or None), h, w, n, min_area, v(d_stats or None), capacity, v(d_offsets or None),
            v(d_chain_offsets or None), v(d_points or None), point_capacity, v(d_point_offsets or None),
            v(d_hull_offsets or None), v(d_hull or None), hull_capacity, v(d_measures or None)), "dev_shapes_bits")

    def shapes_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 measure, 1 scan, 2 emit (SHAPE_PARTS)."""
        return self._profile_part("shapes_profile_get", part)

    # ---- Euclidean distance transform of the finished map ---------------------------------
    def canny_edt(self, imgs, sigma: float, min_val: int, max_val: int, want_dist2: bool = True, want_dist: bool = True,
                  want_nearest: bool = True):
        """canny(), then the exact Euclidean distance transform of each map: imgs (H, W) or (N, H, W) uint8 -> (dist2
        int32, dist float32, nearest int32), each [N, H, W] or None when not asked for (it is then neither computed for
        its own sake nor downloaded): the squared distance to the nearest edge pixel, its correctly rounded root, that
        pixel's index r * W + c.  A frame without edge pixels gives EDT_NONE, +inf and -1."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        d2 = np.empty((n, h, w), np.int32) if want_dist2 else None
        d = np.empty((n, h, w), np.float32) if want_dist else None
        nn = np.empty((n, h, w), np.int32) if want_nearest else None
        self._check(self._L.canny_hip_canny_edt(self._h, _hp(a), n, sigma, min_val, max_val, h, w,
                                                _hp(d2) if want_dist2 else None, _hp(d) if want_dist else None,
                                                _hp(nn) if want_nearest else None), "canny_edt")
        return d2, d, nn

    def dev_canny_edt(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, d_dist2: int,
                      d_dist: int, d_nearest: int, d_edges: int = 0):
        """dev_canny, then its map's distance transform on the same stream: d_dist2 (n*h*w int32), d_dist (n*h*w float32),
        d_nearest (n*h*w int32) -- each a device pointer or 0, not all 0 --, d_edges (the s16 map, device) or 0."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_edt(self._h, v(d_img), sigma, min_val, max_val, h, w, n,
                                                    v(d_edges or None), v(d_dist2 or None), v(d_dist or None),
                                                    v(d_nearest or None)), "dev_canny_edt")

    def dev_edt_bits(self, d_bits: int, h: int, w: int, n: int, d_dist2: int, d_dist: int, d_nearest: int):
        """The transform alone on device bit maps (layout of dev_canny_bits, any byte alignment, padding ignored)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_edt_bits(self._h, v(d_bits or None), h, w, n, v(d_dist2 or None),
                                                   v(d_dist or None), v(d_nearest or None)), "dev_edt_bits")

    def edt_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 rows, 1 columns (EDT_PARTS)."""
        return self._profile_part("edt_profile_get", part)

    # ---- Hough lines of the finished map (cv::HoughLines semantics) -----------------------
    def canny_hough(self, imgs, sigma: float, min_val: int, max_val: int, rho: float = 1.0, theta: float = np.pi / 180,
                    threshold: int = 100, lines_max: int = 256, min_theta: float = 0.0, max_theta: float = np.pi):
        """canny(), then the standard Hough line transform of each map on the GPU: imgs (H, W) or (N, H, W) uint8 ->
        (results, counts): results[f] = (lines float32 [k, 2] as (rho, theta), votes int32 [k], bases uint32 [k]) with
        k = min(lines_max, counts[f]), strongest first; counts int32 [N] holds the true number of peaks per frame."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        slots = n * max(int(lines_max), 1)
        lines, votes = np.zeros((slots, 2), np.float32), np.zeros(slots, np.int32)
        bases, counts = np.zeros(slots, np.uint32), np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_hough(self._h, _hp(a), n, sigma, min_val, max_val, h, w, rho, theta,
                                                  threshold, lines_max, min_theta, max_theta, _hp(lines), _hp(votes),
                                                  _hp(bases), _hp(counts)), "canny_hough")
        out = []
        for f in range(n):
            k, at = min(int(counts[f]), lines_max), f * lines_max
            out.append((lines[at:at + k].copy(), votes[at:at + k].copy(), bases[at:at + k].copy()))
        return out, counts

    def dev_hough_points(self, d_points: int, d_offsets: int, n: int, h: int, w: int, rho: float, theta: float,
                         threshold: int, lines_max: int, min_theta: float, max_theta: float, d_lines: int, d_votes: int,
                         d_bases: int, d_counts: int, d_accum: int = 0):
        """The transform of CSR point lists (as dev_canny_points writes them) on device pointers; d_lines (2 float32 per
        slot), d_votes, d_bases, d_accum may be 0; slot f * lines_max + k; d_counts: n int32."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_hough_points(self._h, v(d_points or None), v(d_offsets or None), n, h, w, rho,
                                                       theta, threshold, lines_max, min_theta, max_theta,
                                                       v(d_lines or None), v(d_votes or None), v(d_bases or None),
                                                       v(d_counts or None), v(d_accum or None)), "dev_hough_points")

    def dev_hough_bits(self, d_bits: int, n: int, h: int, w: int, rho: float, theta: float, threshold: int,
                       lines_max: int, min_theta: float, max_theta: float, d_lines: int, d_votes: int, d_bases: int,
                       d_counts: int, d_accum: int = 0):
        """The same from device bit maps (layout of dev_canny_bits, padding bits ignored)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_hough_bits(self._h, v(d_bits or None), n, h, w, rho, theta, threshold,
                                                     lines_max, min_theta, max_theta, v(d_lines or None),
                                                     v(d_votes or None), v(d_bases or None), v(d_counts or None),
                                                     v(d_accum or None)), "dev_hough_bits")

    def dev_canny_hough(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, rho: float,
                        theta: float, threshold: int, lines_max: int, min_theta: float, max_theta: float, d_lines: int,
                        d_votes: int, d_bases: int, d_counts: int, d_accum: int = 0, d_edges: int = 0):
        """dev_canny, then the transform of its map queued behind it on the same stream (no point list in between)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_hough(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                      v(d_edges or None), rho, theta, threshold, lines_max, min_theta,
                                                      max_theta, v(d_lines or None), v(d_votes or None),
                                                      v(d_bases or None), v(d_counts or None), v(d_accum or None)),
                    "dev_canny_hough")

    def hough_profile_get(self, part: int) -> Tuple[float, int]:
        """Accumulated device milliseconds and launch groups of a Hough part (0 vote, 1 peaks, 2 select + sort)."""
        return self._profile_part("hough_profile_get", part)

    # ---- Hough line segments --------------------------------------------------------------
    def canny_hough_segments(self, imgs, sigma: float, min_val: int, max_val: int, rho: float = 1.0,
                             theta: float = np.pi / 180, threshold: int = 100, lines_max: int = 256, min_length: int = 0,
                             max_gap: int = 0, exclusive: int = 0, segments_max: int = 4096, min_theta: float = 0.0,
                             max_theta: float = np.pi):
        """canny(), the Hough lines of each map and the segments along them, all on the GPU: imgs (H, W) or (N, H, W)
        uint8 -> (lines, line_counts, segments, seg_counts).  lines[f] as canny_hough returns it; segments[f] int32
        [k, 6] rows x0, y0, x1, y1, line, support with k = min(segments_max, seg_counts[f]), ordered by (line, start);
        both count arrays hold the true counts."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        slots = n * max(int(lines_max), 1)
        lines, votes = np.zeros((slots, 2), np.float32), np.zeros(slots, np.int32)
        bases, counts = np.zeros(slots, np.uint32), np.zeros(n, np.int32)
        segs = np.zeros((n, max(int(segments_max), 1), SEGMENT_INTS), np.int32)
        seg_counts = np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_hough_segments(self._h, _hp(a), n, sigma, min_val, max_val, h, w, rho, theta,
                                                           threshold, lines_max, min_theta, max_theta, min_length,
                                                           max_gap, exclusive, _hp(lines), _hp(votes), _hp(bases),
                                                           _hp(counts), _hp(segs), segments_max, _hp(seg_counts)),
                    "canny_hough_segments")
        out_l, out_s = [], []
        for f in range(n):
            k, at = min(int(counts[f]), lines_max), f * lines_max
            out_l.append((lines[at:at + k].copy(), votes[at:at + k].copy(), bases[at:at + k].copy()))
            out_s.append(segs[f, :min(int(seg_counts[f]), segments_max)].copy())
        return out_l, counts, out_s, seg_counts

    def dev_hough_segments_bits(self, d_bits: int, n: int, h: int, w: int, rho: float, theta: float, min_theta: float,
                                max_theta: float, d_bases: int, d_line_counts: int, lines_max: int, min_length: int,
                                max_gap: int, exclusive: int, d_segments: int, segments_max: int, d_seg_counts: int):
        """The segments of device bit maps (layout of dev_canny_bits) along the lines a Hough call left on the device
        (d_bases, d_line_counts, slot f * lines_max + k); d_segments: n * segments_max * 6 int32, d_seg_counts: n int32."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_hough_segments_bits(self._h, v(d_bits or None), n, h, w, rho, theta, min_theta,
                                                              max_theta, v(d_bases or None), v(d_line_counts or None),
                                                              lines_max, min_length, max_gap, exclusive,
                                                              v(d_segments or None), segments_max,
                                                              v(d_seg_counts or None)), "dev_hough_segments_bits")

    def dev_canny_hough_segments(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                                 rho: float, theta: float, threshold: int, lines_max: int, min_theta: float,
                                 max_theta: float, min_length: int, max_gap: int, exclusive: int, d_segments: int,
                                 segments_max: int, d_seg_counts: int, d_lines: int = 0, d_votes: int = 0, d_bases: int = 0,
                                 d_line_counts: int = 0, d_accum: int = 0, d_edges: int = 0):
        """dev_canny_hough, then the segments along its lines queued behind it on the same stream; the line outputs and
        d_edges are optional (0)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_hough_segments(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                               v(d_edges or None), rho, theta, threshold, lines_max,
                                                               min_theta, max_theta, v(d_lines or None),
                                                               v(d_votes or None), v(d_bases or None),
                                                               v(d_line_counts or None), v(d_accum or None), min_length,
                                                               max_gap, exclusive, v(d_segments or None), segments_max,
                                                               v(d_seg_counts or None)), "dev_canny_hough_segments")

    def hough_segments_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 count, 1 emit, 2 exclusive (SEGMENT_PARTS)."""
        return self._profile_part("hough_segments_profile_get", part)

    # ---- sub-pixel line fits (least-squares refit of the Hough segments from edgels) -------
    def canny_hough_line_fits(self, imgs, sigma: float, min_val: int, max_val: int, rho: float = 1.0,
                              theta: float = np.pi / 180, threshold: int = 100, lines_max: int = 256, min_length: int = 0,
                              max_gap: int = 0, exclusive: int = 0, segments_max: int = 4096, options: int = 0,
                              min_theta: float = 0.0, max_theta: float = np.pi):
        """canny_hough_segments plus one line-fit record per segment, all on the GPU: imgs (H, W) or (N, H, W) uint8 ->
        (lines, line_counts, segments, seg_counts, fits); fits[f] int32 [k, 12], slot for slot with segments[f]; unpack
        them with line_fits_unpack."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        slots = n * max(int(lines_max), 1)
        lines, votes = np.zeros((slots, 2), np.float32), np.zeros(slots, np.int32)
        bases, counts = np.zeros(slots, np.uint32), np.zeros(n, np.int32)
        segs = np.zeros((n, max(int(segments_max), 1), SEGMENT_INTS), np.int32)
        fits = np.zeros((n, max(int(segments_max), 1), LINE_FIT_INTS), np.int32)
        seg_counts = np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_hough_line_fits(self._h, _hp(a), n, sigma, min_val, max_val, h, w, rho, theta,
                                                            threshold, lines_max, min_theta, max_theta, min_length,
                                                            max_gap, exclusive, options, _hp(lines), _hp(votes),
                                                            _hp(bases), _hp(counts), _hp(segs), segments_max,
                                                            _hp(seg_counts), _hp(fits)), "canny_hough_line_fits")
        out_l, out_s, out_f = [], [], []
        for f in range(n):
            k, at = min(int(counts[f]), lines_max), f * lines_max
            out_l.append((lines[at:at + k].copy(), votes[at:at + k].copy(), bases[at:at + k].copy()))
            j = min(int(seg_counts[f]), segments_max)
            out_s.append(segs[f, :j].copy())
            out_f.append(fits[f, :j].copy())
        return out_l, counts, out_s, seg_counts, out_f

    def dev_line_fits_bits(self, d_bits: int, d_plane: int, plane_is_u8: bool, n: int, h: int, w: int, rho: float,
                           theta: float, min_theta: float, max_theta: float, d_bases: int, d_line_counts: int,
                           lines_max: int, d_segments: int, d_seg_counts: int, segments_max: int, options: int,
                           d_fits: int):
        """The fits of the segment records an earlier call left on the device (d_segments, d_seg_counts; lines in d_bases,
        d_line_counts) on device bit maps (layout of dev_canny_bits) and a device plane (u8 or s16; 0 = the smoothed plane
        the last canny call of the same shape left).  d_fits: n * segments_max * 12 int32, 16-byte aligned."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_line_fits_bits(self._h, v(d_bits or None), v(d_plane or None), int(plane_is_u8),
                                                         n, h, w, rho, theta, min_theta, max_theta, v(d_bases or None),
                                                         v(d_line_counts or None), lines_max, v(d_segments or None),
                                                         v(d_seg_counts or None), segments_max, options,
                                                         v(d_fits or None)), "dev_line_fits_bits")

    def dev_canny_hough_line_fits(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                                  rho: float, theta: float, threshold: int, lines_max: int, min_theta: float,
                                  max_theta: float, min_length: int, max_gap: int, exclusive: int, d_segments: int,
                                  segments_max: int, d_seg_counts: int, options: int, d_fits: int, d_lines: int = 0,
                                  d_votes: int = 0, d_bases: int = 0, d_line_counts: int = 0, d_accum: int = 0,
                                  d_edges: int = 0):
        """dev_canny_hough_segments, then the fits of its segments queued behind it on the same stream."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_hough_line_fits(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                                v(d_edges or None), rho, theta, threshold, lines_max,
                                                                min_theta, max_theta, v(d_lines or None),
                                                                v(d_votes or None), v(d_bases or None),
                                                                v(d_line_counts or None), v(d_accum or None), min_length,
                                                                max_gap, exclusive, v(d_segments or None), segments_max,
                                                                v(d_seg_counts or None), options, v(d_fits or None)),
                    "dev_canny_hough_line_fits")

    def dev_line_fits_arith(self, d_moments: int, n_sets: int, d_out: int):
        """Test hook: the device finishing arithmetic on n_sets x 8 int64 (n, Su, Sv, Suu, Suv, Svv, ddx, ddy) -> n_sets
        x 6 int32 (mu, mv, dx_q30, dy_q30, n, DEGENERATE or 0)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_line_fits_arith(self._h, v(d_moments or None), n_sets, v(d_out or None)),
                    "dev_line_fits_arith")

    def line_fits_profile_get(self, part: int = 0) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0, the fit kernel (LINE_FIT_PART_FIT)."""
        return self._profile_part("line_fits_profile_get", part)

    # ---- Hough circles (cv::HoughCircles(HOUGH_GRADIENT) semantics) ------------------------
    def canny_hough_circles(self, imgs, sigma: float, min_val: int, max_val: int, min_radius: int, max_radius: int,
                            cell_shift: int = 0, threshold: int = 20, support_threshold: int = 10, min_dist: int = 0,
                            centres_max: int = 256):
        """canny(), then the circle transform of each map on the GPU: imgs (H, W) or (N, H, W) uint8 -> (circles,
        centre_counts): circles[f] is a structured array (CIRCLE_DTYPE) of the accepted circles in candidate order, with
        float x = x2 / 2, y = y2 / 2 (pixel coordinates of the centre) beside the record's six ints; centre_counts int32
        [N] holds the true number of accumulator peaks per frame."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        rec = np.zeros((n, max(int(centres_max), 1), CIRCLE_INTS), np.int32)
        counts, peaks = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_hough_circles(self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_radius,
                                                          max_radius, cell_shift, threshold, support_threshold, min_dist,
                                                          centres_max, _hp(rec), _hp(counts), _hp(peaks)),
                    "canny_hough_circles")
        out = []
        for f in range(n):
            r = rec[f, :int(counts[f])]
            c = np.zeros(len(r), CIRCLE_DTYPE)
            c["x"], c["y"] = r[:, 0] / np.float32(2), r[:, 1] / np.float32(2)
            for j, name in enumerate(("x2", "y2", "radius", "votes", "support", "base")):
                c[name] = r[:, j]
            out.append(c)
        return out, peaks

    def dev_hough_circles_bits(self, d_bits: int, d_gx: int, d_gy: int, n: int, h: int, w: int, min_radius: int,
                               max_radius: int, cell_shift: int, threshold: int, support_threshold: int, min_dist: int,
                               centres_max: int, d_circles: int, d_counts: int, d_centre_counts: int = 0, d_accum: int = 0):
        """The transform of device bit maps (layout of dev_canny_bits, padding bits ignored) with full int16 gradient
        planes; d_circles (6 int32 per slot, slot f * centres_max + j), d_centre_counts, d_accum may be 0; d_counts: n
        int32."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_hough_circles_bits(self._h, v(d_bits or None), v(d_gx or None), v(d_gy or None), n,
                                                             h, w, min_radius, max_radius, cell_shift, threshold,
                                                             support_threshold, min_dist, centres_max,
                                                             v(d_circles or None), v(d_counts or None),
                                                             v(d_centre_counts or None), v(d_accum or None)),
                    "dev_hough_circles_bits")

    def dev_canny_hough_circles(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                                min_radius: int, max_radius: int, cell_shift: int, threshold: int, support_threshold: int,
                                min_dist: int, centres_max: int, d_circles: int, d_counts: int, d_centre_counts: int = 0,
                                d_accum: int = 0, d_edges: int = 0):
        """dev_canny, then the circle transform queued behind it on the same stream: the map from the hysteresis bit-plane,
        the gradient recomputed at the edge pixels from that call's smoothed plane."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_hough_circles(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                              v(d_edges or None), min_radius, max_radius, cell_shift,
                                                              threshold, support_threshold, min_dist, centres_max,
                                                              v(d_circles or None), v(d_counts or None),
                                                              v(d_centre_counts or None), v(d_accum or None)),
                    "dev_canny_hough_circles")

    def dev_hough_circles_steps(self, d_gx: int, d_gy: int, n: int, d_sx: int, d_sy: int):
        """The device's step arithmetic on n int16 gradient pairs -> n int32 each in d_sx, d_sy."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_hough_circles_steps(self._h, v(d_gx or None), v(d_gy or None), n,
                                                              v(d_sx or None), v(d_sy or None)), "dev_hough_circles_steps")

    def hough_circles_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 vote, 1 centres, 2 radius, 3 accept (CIRCLE_PARTS)."""
        return self._profile_part("hough_circles_profile_get", part)

    # ---- chamfer template matching on the distance transform -----------------------------
    def chamfer_set_create(self, templates=None, csr=None) -> int:
        """A template set on this context from a list of (K_t, 2) arrays of (dx, dy), or csr = (offsets, points) as they
        are -> an opaque handle for the chamfer calls; chamfer_set_destroy releases it (the context does at the latest)."""
        off, pts = csr if csr is not None else chamfer_csr(templates)
        off, pts = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.int16)
        h = C.c_void_p()
        self._check(self._L.canny_hip_chamfer_set_create(self._h, _hp(off), _hp(pts), len(off) - 1, C.byref(h)),
                    "chamfer_set_create")
        return h.value

    def chamfer_set_destroy(self, cset: int):
        self._check(self._L.canny_hip_chamfer_set_destroy(self._h, C.c_void_p(cset or None)), "chamfer_set_destroy")

    def dev_chamfer_dist2(self, d_dist2: int, n: int, h: int, w: int, cset: int, trunc_q4: int, max_mean_q4: int,
                          min_dist: int, matches_max: int, d_matches: int, d_counts: int, d_cand_counts: int = 0,
                          d_scores: int = 0):
        """Matching alone on a device dist2 plane; d_matches (6 int32 per slot, slot f * matches_max + j), d_cand_counts,
        d_scores ([n][T][h][w] uint32) may be 0; d_counts: n int32.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_chamfer_dist2(self._h, v(d_dist2 or None), n, h, w, v(cset or None), trunc_q4,
                                                        max_mean_q4, min_dist, matches_max, v(d_matches or None),
                                                        v(d_counts or None), v(d_cand_counts or None), v(d_scores or None)),
                    "dev_chamfer_dist2")

    def dev_chamfer_bits(self, d_bits: int, n: int, h: int, w: int, cset: int, trunc_q4: int, max_mean_q4: int,
                         min_dist: int, matches_max: int, d_matches: int, d_counts: int, d_cand_counts: int = 0,
                         d_scores: int = 0, d_dist2: int = 0):
        """dev_edt_bits on device bit maps, then the matching; d_dist2 0: a workspace holds the plane."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_chamfer_bits(self._h, v(d_bits or None), n, h, w, v(d_dist2 or None),
                                                       v(cset or None), trunc_q4, max_mean_q4, min_dist, matches_max,
                                                       v(d_matches or None), v(d_counts or None), v(d_cand_counts or None),
                                                       v(d_scores or None)), "dev_chamfer_bits")

    def dev_canny_chamfer(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, cset: int,
                          trunc_q4: int, max_mean_q4: int, min_dist: int, matches_max: int, d_matches: int, d_counts: int,
                          d_cand_counts: int = 0, d_scores: int = 0, d_edges: int = 0, d_dist2: int = 0):
        """dev_canny_edt, then the matching queued behind it on the same stream."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_chamfer(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                        v(d_edges or None), v(d_dist2 or None), v(cset or None), trunc_q4,
                                                        max_mean_q4, min_dist, matches_max, v(d_matches or None),
                                                        v(d_counts or None), v(d_cand_counts or None), v(d_scores or None)),
                    "dev_canny_chamfer")

    def canny_chamfer(self, imgs, sigma: float, min_val: int, max_val: int, cset: int, trunc_q4: int, max_mean_q4: int,
                      min_dist: int = 0, matches_max: int = 256):
        """canny(), the distance transform and the matching of each map on the GPU: imgs (H, W) or (N, H, W) uint8 ->
        (matches, cand_counts): matches[f] is a structured array (MATCH_DTYPE) of the accepted matches in order,
        cand_counts int32 [N] the true number of candidates per frame."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        rec = np.zeros((n, max(int(matches_max), 1), MATCH_INTS), np.int32)
        counts, cands = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_chamfer(self._h, _hp(a), n, sigma, min_val, max_val, h, w,
                                                    C.c_void_p(cset or None), trunc_q4, max_mean_q4, min_dist, matches_max,
                                                    _hp(rec), _hp(counts), _hp(cands)), "canny_chamfer")
        return [np.ascontiguousarray(rec[f, :int(counts[f])]).view(MATCH_DTYPE).reshape(-1) for f in range(n)], cands

    def dev_chamfer_costs(self, d_dist2: int, n: int, trunc_q4: int, d_costs: int):
        """The device's cost arithmetic on n int32 dist2 values -> n uint32 (trunc_q4 = 0: the untruncated root)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_chamfer_costs(self._h, v(d_dist2 or None), n, trunc_q4, v(d_costs or None)),
                    "dev_chamfer_costs")

    def chamfer_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 cost, 1 score, 2 candidates, 3 accept (CHAMFER_PARTS)."""
        return self._profile_part("chamfer_profile_get", part)

    # ---- corners, Harris / Shi-Tomasi on the smoothed plane ---------------------------------
    def dev_canny_corners(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, mode: int,
                          block: int, k_q8: int, quality_q16: int, min_response: int, min_dist: int, corners_max: int,
                          d_corners: int, d_counts: int, d_cand_counts: int = 0, d_max_response: int = 0,
                          d_response: int = 0, d_edges: int = 0):
        """dev_canny, then the corners of the smoothed plane it left, on the same stream; d_corners (4 int64 per slot,
        slot f * corners_max + j) and d_counts (n int32) are mandatory; d_cand_counts (n int32), d_max_response (n
        int64), d_response ([n][h][w] int64), d_edges may be 0.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_corners(self._h, v(d_img or None), sigma, min_val, max_val, h, w, n,
                                                        v(d_edges or None), mode, block, k_q8, quality_q16, min_response,
                                                        min_dist, corners_max, v(d_corners or None), v(d_counts or None),
                                                        v(d_cand_counts or None), v(d_max_response or None),
                                                        v(d_response or None)), "dev_canny_corners")

    def dev_corners_plane(self, d_plane: int, n: int, h: int, w: int, mode: int, block: int, k_q8: int, quality_q16: int,
                          min_response: int, min_dist: int, corners_max: int, d_corners: int, d_counts: int,
                          d_cand_counts: int = 0, d_max_response: int = 0, d_response: int = 0):
        """The corners of a device u8 plane [n][h][w]; d_plane 0: of the plane the context's last canny call left."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_corners_plane(self._h, v(d_plane or None), n, h, w, mode, block, k_q8,
                                                        quality_q16, min_response, min_dist, corners_max,
                                                        v(d_corners or None), v(d_counts or None), v(d_cand_counts or None),
                                                        v(d_max_response or None), v(d_response or None)),
                    "dev_corners_plane")

    def canny_corners(self, imgs, sigma: float, min_val: int, max_val: int, mode: int = CORNERS_MIN_EIGEN, block: int = 3,
                      k_q8: int = 0, quality_q16: int = 655, min_response: int = 0, min_dist: int = 0,
                      corners_max: int = 256):
        """canny() and the corners of each smoothed plane on the GPU: imgs (H, W) or (N, H, W) uint8 -> (corners,
        cand_counts, max_response): corners[f] is a structured array (CORNER_DTYPE) of the accepted corners in order,
        cand_counts int32 [N] the true number of candidates, max_response int64 [N] the largest response per frame."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        rec = np.zeros((n, max(int(corners_max), 1), CORNER_WORDS), np.int64)
        counts, cands, rmax = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        self._check(self._L.canny_hip_canny_corners(self._h, _hp(a), n, sigma, min_val, max_val, h, w, mode, block, k_q8,
                                                    quality_q16, min_response, min_dist, corners_max, _hp(rec),
                                                    _hp(counts), _hp(cands), _hp(rmax)), "canny_corners")
        return ([np.ascontiguousarray(rec[f, :int(counts[f])]).view(CORNER_DTYPE).reshape(-1) for f in range(n)], cands,
                rmax)

    def dev_corners_arith(self, d_sums: int, n: int, mode: int, k_q8: int, d_r: int):
        """The device's response function on n int32 triples (sxx, syy, sxy) -> n int64."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_corners_arith(self._h, v(d_sums or None), n, mode, k_q8, v(d_r or None)),
                    "dev_corners_arith")

    def corners_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 max, 1 candidates, 2 collect, 3 accept (CORNER_PARTS)."""
        return self._profile_part("corners_profile_get", part)

    # ---- corner descriptors and Hamming matching ---------------------------------------------
    def dev_canny_corner_descriptors(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                                     mode: int, block: int, k_q8: int, quality_q16: int, min_response: int, min_dist: int,
                                     corners_max: int, d_corners: int, d_counts: int, d_desc: int, d_meta: int,
                                     desc_options: int = 0, d_cand_counts: int = 0, d_max_response: int = 0,
                                     d_response: int = 0, d_edges: int = 0):
        """dev_canny_corners, then the descriptors of the corners on the smoothed plane, on the same stream; d_desc (4
        uint64 per slot) and d_meta (int32 per slot) are mandatory.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_corner_descriptors(
            self._h, v(d_img or None), sigma, min_val, max_val, h, w, n, v(d_edges or None), mode, block, k_q8, quality_q16,
            min_response, min_dist, corners_max, v(d_corners or None), v(d_counts or None), v(d_cand_counts or None),
            v(d_max_response or None), v(d_response or None), desc_options, v(d_desc or None), v(d_meta or None)),
            "dev_canny_corner_descriptors")

    def dev_corner_descriptors(self, d_plane: int, n: int, h: int, w: int, d_corners: int, d_counts: int, corners_max: int,
                               d_desc: int, d_meta: int, desc_options: int = 0):
        """The descriptors of device records on a device u8 plane [n][h][w]; d_plane 0: on the plane the context's last
        canny call left."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_corner_descriptors(self._h, v(d_plane or None), n, h, w, v(d_corners or None),
                                                             v(d_counts or None), corners_max, desc_options,
                                                             v(d_desc or None), v(d_meta or None)),
                    "dev_corner_descriptors")

    def canny_corner_descriptors(self, imgs, sigma: float, min_val: int, max_val: int, mode: int = CORNERS_MIN_EIGEN,
                                 block: int = 3, k_q8: int = 0, quality_q16: int = 655, min_response: int = 0,
                                 min_dist: int = 0, corners_max: int = 256, steered: bool = False):
        """canny(), the corners and their descriptors on the GPU: imgs (H, W) or (N, H, W) uint8 -> per frame a tuple
        (corners as CORNER_DTYPE, descriptors uint64 [k, 4], meta int32 [k])."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        cm = max(int(corners_max), 1)
        rec = np.zeros((n, cm, CORNER_WORDS), np.int64)
        desc, meta = np.zeros((n, cm, DESC_WORDS), np.uint64), np.zeros((n, cm), np.int32)
        counts = np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_corner_descriptors(self._h, _hp(a), n, sigma, min_val, max_val, h, w, mode,
                                                               block, k_q8, quality_q16, min_response, min_dist,
                                                               corners_max, DESC_STEERED if steered else 0, _hp(rec),
                                                               _hp(counts), _hp(desc), _hp(meta)),
                    "canny_corner_descriptors")
        return [(np.ascontiguousarray(rec[f, :int(counts[f])]).view(CORNER_DTYPE).reshape(-1),
                 desc[f, :int(counts[f])].copy(), meta[f, :int(counts[f])].copy()) for f in range(n)]

    def dev_match_descriptors(self, d_q_desc: int, d_q_counts: int, n_q_frames: int, stride_q: int, d_t_desc: int,
                              d_t_counts: int, n_t_frames: int, stride_t: int, pairs, d_matches: int, d_pair_counts: int,
                              max_distance: int = 64, ratio_q8: int = 205, options: int = MATCH_CROSS_CHECK):
        """Brute-force Hamming matching of the pairs (host int array [n_pairs, 2]: q frame, t frame; see
        consecutive_pairs) between two descriptor sets on the device (they may be the same buffers); d_matches receives
        [n_pairs][stride_q][4] int32 (j, d1, d2, flags), d_pair_counts [n_pairs] int32.  Asynchronous."""
        v = C.c_void_p
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        self._check(self._L.canny_hip_dev_match_descriptors(self._h, v(d_q_desc or None), v(d_q_counts or None), n_q_frames,
                                                            stride_q, v(d_t_desc or None), v(d_t_counts or None),
                                                            n_t_frames, stride_t, _hp(pr) if len(pr) else None, len(pr),
                                                            max_distance, ratio_q8, options, v(d_matches or None),
                                                            v(d_pair_counts or None)), "dev_match_descriptors")

    def descriptors_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 describe, 1 match, 2 reverse, 3 finalize (DESC_PARTS)."""
        return self._profile_part("descriptors_profile_get", part)

    # ---- frame-to-frame motion from the corner matches ---------------------------------------
    def dev_estimate_motion(self, d_q_corners: int, d_q_counts: int, n_q_frames: int, stride_q: int, d_t_corners: int,
                            d_t_counts: int, n_t_frames: int, stride_t: int, pairs, d_matches: int, d_motion: int,
                            d_inlier: int = 0, model: int = MOTION_SIMILARITY, thr_q4: int = 48, hypotheses: int = 256,
                            seed: int = 0):
        """Consensus over the accepted matches of the pairs (host int array [n_pairs, 2]: q frame, t frame) and one motion
        model per pair: d_matches is the matcher's [n_pairs][stride_q][4] int32, d_motion receives [n_pairs][16] int64
        (MOTION_DTYPE), d_inlier (optional) [n_pairs][stride_q] int32.  Asynchronous."""
        v = C.c_void_p
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        self._check(self._L.canny_hip_dev_estimate_motion(self._h, v(d_q_corners or None), v(d_q_counts or None), n_q_frames,
                                                          stride_q, v(d_t_corners or None), v(d_t_counts or None),
                                                          n_t_frames, stride_t, _hp(pr) if len(pr) else None, len(pr),
                                                          v(d_matches or None), model, thr_q4, hypotheses,
                                                          int(seed) & 0xFFFFFFFF, v(d_motion or None), v(d_inlier or None)),
                    "dev_estimate_motion")

    def canny_motion(self, imgs, sigma: float, min_val: int, max_val: int, pairs=None, mode: int = CORNERS_MIN_EIGEN,
                     block: int = 3, k_q8: int = 0, quality_q16: int = 655, min_response: int = 0, min_dist: int = 0,
                     corners_max: int = 256, steered: bool = False, max_distance: int = 64, ratio_q8: int = 205,
                     match_options: int = MATCH_CROSS_CHECK, model: int = MOTION_SIMILARITY, thr_q4: int = 48,
                     hypotheses: int = 256, seed: int = 0, details: bool = False):
        """canny(), corners, descriptors, matching over `pairs` (default: consecutive frames) and the motion of every pair,
        all on the GPU: imgs (N, H, W) uint8 -> the records as MOTION_DTYPE [n_pairs]; with details also (corners per frame
        as CORNER_DTYPE, matches per pair int32 [k, 4], inlier flags per pair int32 [k])."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError("expected uint8 [n_frames, H, W]")
        n, h, w = a.shape
        pr = np.ascontiguousarray(consecutive_pairs(n) if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        cm = max(int(corners_max), 1)
        motion = np.zeros((len(pr), MOTION_WORDS), np.int64)
        rec, counts = np.zeros((n, cm, CORNER_WORDS), np.int64), np.zeros(n, np.int32)
        mt, flags = np.zeros((len(pr), cm, MATCH_WORDS), np.int32), np.zeros((len(pr), cm), np.int32)
        self._check(self._L.canny_hip_canny_motion(self._h, _hp(a), n, sigma, min_val, max_val, h, w, mode, block, k_q8,
                                                   quality_q16, min_response, min_dist, corners_max,
                                                   DESC_STEERED if steered else 0, _hp(pr) if len(pr) else None, len(pr),
                                                   max_distance, ratio_q8, match_options, model, thr_q4, hypotheses,
                                                   int(seed) & 0xFFFFFFFF, _hp(motion) if len(pr) else None,
                                                   _hp(rec) if details else None, _hp(counts) if details else None,
                                                   _hp(mt) if details else None, _hp(flags) if details else None),
                    "canny_motion")
        records = motion.view(MOTION_DTYPE).reshape(-1)
        if not details:
            return records
        k = [int(counts[q]) for q, _ in pr.tolist()]
        return (records, [np.ascontiguousarray(rec[f, :int(counts[f])]).view(CORNER_DTYPE).reshape(-1) for f in range(n)],
                [mt[p, :k[p]].copy() for p in range(len(pr))], [flags[p, :k[p]].copy() for p in range(len(pr))])

    # ---- frame alignment: the motions chained, frames warped ---------------------------------
    def dev_compose_motion(self, d_motion: int, n_pairs: int, first_frame: int, d_xforms: int):
        """The device motion records of the consecutive pairs (f, f + 1), f = first_frame .., chained into n_pairs + 1
        transform records at d_xforms ([n_pairs + 1][8] int64, XFORM_DTYPE).  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_compose_motion(self._h, v(d_motion or None), n_pairs, first_frame,
                                                         v(d_xforms or None)), "dev_compose_motion")

    def dev_warp_frames(self, d_src: int, n_src: int, src_h: int, src_w: int, d_xforms: int, n_out: int, out_h: int,
                        out_w: int, d_out: int, d_valid_bits: int = 0, interp: int = WARP_BILINEAR, border: int = 0):
        """u8 planes [n_src][src_h][src_w] warped by the n_out device transform records into d_out [n_out][out_h][out_w]
        and, if given, the valid bit maps [n_out][out_h][ceil(out_w / 8)].  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_warp_frames(self._h, v(d_src or None), n_src, src_h, src_w, v(d_xforms or None),
                                                      n_out, out_h, out_w, interp, border, v(d_out or None),
                                                      v(d_valid_bits or None)), "dev_warp_frames")

    def canny_align(self, imgs, sigma: float, min_val: int, max_val: int, mode: int = CORNERS_MIN_EIGEN, block: int = 3,
                    k_q8: int = 0, quality_q16: int = 655, min_response: int = 0, min_dist: int = 0, corners_max: int = 256,
                    steered: bool = False, max_distance: int = 64, ratio_q8: int = 205,
                    match_options: int = MATCH_CROSS_CHECK, model: int = MOTION_SIMILARITY, thr_q4: int = 48,
                    hypotheses: int = 256, seed: int = 0, interp: int = WARP_BILINEAR, border: int = 0,
                    details: bool = False):
        """canny(), corners, descriptors, matching and motion over the consecutive pairs, the chain from frame 0 and the warp
        of the input frames onto frame 0, all on the GPU: imgs (N, H, W) uint8 -> (aligned uint8 [N, H, W], transform
        records XFORM_DTYPE [N]); with details also (motion records MOTION_DTYPE [N - 1], valid bit maps uint8
        [N, H, ceil(W / 8)])."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError("expected uint8 [n_frames, H, W]")
        n, h, w = a.shape
        aligned, xf = np.zeros((n, h, w), np.uint8), np.zeros((n, XFORM_WORDS), np.int64)
        motion, valid = np.zeros((max(n - 1, 0), MOTION_WORDS), np.int64), np.zeros((n, h, (w + 7) // 8), np.uint8)
        self._check(self._L.canny_hip_canny_align(self._h, _hp(a), n, sigma, min_val, max_val, h, w, mode, block, k_q8,
                                                  quality_q16, min_response, min_dist, corners_max,
                                                  DESC_STEERED if steered else 0, max_distance, ratio_q8, match_options,
                                                  model, thr_q4, hypotheses, int(seed) & 0xFFFFFFFF, interp, border,
                                                  _hp(aligned), _hp(xf), _hp(motion) if details and n > 1 else None,
                                                  _hp(valid) if details else None), "canny_align")
        records = xf.view(XFORM_DTYPE).reshape(-1)
        if not details:
            return aligned, records
        return aligned, records, motion.view(MOTION_DTYPE).reshape(-1), valid

    def warp_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 compose, 1 warp (WARP_PARTS)."""
        return self._profile_part("warp_profile_get", part)

    # ---- temporal fusion of aligned frames and change masks ------------------------------------
    def dev_fuse_frames(self, d_frames: int, d_valid_bits: int, n_frames: int, h: int, w: int, group_len: int,
                        group_step: int, d_fused: int, d_count: int = 0, op: int = FUSE_MEDIAN, fill: int = 0,
                        min_count: int = 1):
        """u8 planes [n_frames][h][w] reduced over windows of group_len frames, group_step apart, under the valid bit maps
        (0: every pixel valid) into d_fused [n_groups][h][w] and, if given, the counts d_count.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_fuse_frames(self._h, v(d_frames or None), v(d_valid_bits or None), n_frames, h, w,
                                                      group_len, group_step, op, fill, min_count, v(d_fused or None),
                                                      v(d_count or None)), "dev_fuse_frames")

    def dev_change_mask(self, d_frames: int, d_valid_bits: int, n_frames: int, h: int, w: int, d_background: int,
                        d_bg_count: int, frames_per_background: int, d_mask_bits: int, d_changed: int = 0, thr: int = 0,
                        min_count: int = 1):
        """The change masks of the frames against background plane f // frames_per_background into d_mask_bits
        [n_frames][h][ceil(w / 8)] (the layout dev_components_bits takes) and, if given, the set bits of each frame as
        int64 at d_changed.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_change_mask(self._h, v(d_frames or None), v(d_valid_bits or None), n_frames, h, w,
                                                      v(d_background or None), v(d_bg_count or None), frames_per_background,
                                                      thr, min_count, v(d_mask_bits or None), v(d_changed or None)),
                    "dev_change_mask")

    def canny_background(self, imgs, sigma: float, min_val: int, max_val: int, mode: int = CORNERS_MIN_EIGEN, block: int = 3,
                         k_q8: int = 0, quality_q16: int = 655, min_response: int = 0, min_dist: int = 0,
                         corners_max: int = 256, steered: bool = False, max_distance: int = 64, ratio_q8: int = 205,
                         match_options: int = MATCH_CROSS_CHECK, model: int = MOTION_SIMILARITY, thr_q4: int = 48,
                         hypotheses: int = 256, seed: int = 0, interp: int = WARP_BILINEAR, border: int = 0,
                         op: int = FUSE_MEDIAN, fill: int = 0, min_count: int = 1, thr: int = 0, details: bool = False):
        """canny_align's chain, the fusion of all aligned frames into one background and the change masks of the aligned
        frames against it, all on the GPU: imgs (N, H, W) uint8, N <= 255 -> (background uint8 [H, W], mask bit maps uint8
        [N, H, ceil(W / 8)], changed int64 [N]); with details also (count uint8 [H, W], transform records XFORM_DTYPE
        [N])."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError("expected uint8 [n_frames, H, W]")
        n, h, w = a.shape
        bg, count = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        mask, changed, xf = np.zeros((n, h, (w + 7) // 8), np.uint8), np.zeros(n, np.int64), np.zeros((n, XFORM_WORDS), np.int64)
        self._check(self._L.canny_hip_canny_background(self._h, _hp(a), n, sigma, min_val, max_val, h, w, mode, block, k_q8,
                                                       quality_q16, min_response, min_dist, corners_max,
                                                       DESC_STEERED if steered else 0, max_distance, ratio_q8,
                                                       match_options, model, thr_q4, hypotheses, int(seed) & 0xFFFFFFFF,
                                                       interp, border, op, fill, min_count, thr, _hp(bg),
                                                       _hp(count) if details else None, _hp(mask), _hp(changed), _hp(xf)),
                    "canny_background")
        if not details:
            return bg, mask, changed
        return bg, mask, changed, count, xf.view(XFORM_DTYPE).reshape(-1)

    def fuse_profile(self, part) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 fuse, 1 mask (FUSE_PARTS; a name or its number)."""
        k = FUSE_PARTS.index(part) if isinstance(part, str) else int(part)
        return self._profile_part("fuse_profile_get", k)

    def selftest_fuse_mean(self):
        """The fuse kernels' rounded mean over every c = 1..255, s = 0..255 c, from the device: uint8 [255, FUSE_MEAN_ROW],
        row c - 1, unused cells 0."""
        out = np.zeros((255, FUSE_MEAN_ROW), np.uint8)
        self._check(self._L.canny_hip_selftest_fuse_mean(self._h, _hp(out)), "selftest_fuse_mean")
        return out

    # ---- binary morphology on packed bit maps --------------------------------------------------
    def dev_morph_bits(self, d_bits: int, n_frames: int, h: int, w: int, op: int, rows, kw: int, kh: int, d_out_bits: int,
                       d_counts: int = 0, border: int = MORPH_BORDER_NEUTRAL, iterations: int = 1):
        """The operator on device bit maps [n_frames][h][ceil(w / 8)] into d_out_bits and, if given, the set bits of each
        output frame as int64 at d_counts.  rows: the element's kh words (host).  Asynchronous."""
        v = C.c_void_p
        r = _morph_rows(rows, kh)
        self._check(self._L.canny_hip_dev_morph_bits(self._h, v(d_bits or None), n_frames, h, w, op, _hp(r), kw, kh, border,
                                                     iterations, v(d_out_bits or None), v(d_counts or None)), "dev_morph_bits")

    def dev_canny_morph(self, n_frames: int, h: int, w: int, op: int, rows, kw: int, kh: int, d_out_bits: int,
                        d_counts: int = 0, border: int = MORPH_BORDER_NEUTRAL, iterations: int = 1):
        """The operator on the strong bit-plane the preceding dev_canny of the same geometry left in the context.
        Asynchronous."""
        v = C.c_void_p
        r = _morph_rows(rows, kh)
        self._check(self._L.canny_hip_dev_canny_morph(self._h, n_frames, h, w, op, _hp(r), kw, kh, border, iterations,
                                                      v(d_out_bits or None), v(d_counts or None)), "dev_canny_morph")

    def canny_morph(self, imgs, sigma: float, min_val: int, max_val: int, op: int, rows, kw: int, kh: int,
                    border: int = MORPH_BORDER_NEUTRAL, iterations: int = 1):
        """Upload, canny and the operator on the finished map, all on the GPU: imgs (N, H, W) uint8 -> (bit maps uint8 [N, H,
        ceil(W / 8)], counts int64 [N])."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError("expected uint8 [n_frames, H, W]")
        n, h, w = a.shape
        r = _morph_rows(rows, kh)
        out, counts = np.zeros((n, h, (w + 7) // 8), np.uint8), np.zeros(n, np.int64)
        self._check(self._L.canny_hip_canny_morph(self._h, _hp(a), n, sigma, min_val, max_val, h, w, op, _hp(r), kw, kh,
                                                  border, iterations, _hp(out), _hp(counts)), "canny_morph")
        return out, counts

    def morph_profile(self, part: int = 0) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0, all primitive steps of the morphology calls."""
        return self._profile_part("morph_profile_get", int(part))

    # ---- binarization: gray planes to packed bit maps -----------------------------------------
    def dev_binarize(self, d_plane: int, n_frames: int, h: int, w: int, method: int, thr_or_c: int, d_out_bits: int,
                     d_counts: int = 0, d_thresholds: int = 0, kw: int = 3, kh: int = 3, invert: int = 0):
        """The operator on device planes uint8 [n_frames][h][w] (d_plane 0: the smoothed plane the preceding dev_canny of
        the same geometry left in the context) into d_out_bits [n_frames][h][ceil(w / 8)] and, if given, the set bits of
        each output frame as int64 at d_counts and the thresholds as int32 at d_thresholds.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_binarize(self._h, v(d_plane or None), n_frames, h, w, method, thr_or_c, kw, kh,
                                                   invert, v(d_out_bits or None), v(d_counts or None),
                                                   v(d_thresholds or None)), "dev_binarize")

    def binarize_batch(self, imgs, method: int, thr_or_c: int = 0, kw: int = 3, kh: Optional[int] = None, invert: int = 0):
        """Upload and the operator on the GPU: imgs (N, H, W) uint8 -> (bit maps uint8 [N, H, ceil(W / 8)], counts int64 [N],
        thresholds int32 [N])."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError("expected uint8 [n_frames, H, W]")
        n, h, w = a.shape
        out, counts, thr = np.zeros((n, h, (w + 7) // 8), np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int32)
        self._check(self._L.canny_hip_binarize_batch(self._h, _hp(a), n, h, w, int(method), int(thr_or_c), int(kw),
                                                     int(kw if kh is None else kh), int(invert), _hp(out), _hp(counts),
                                                     _hp(thr)), "binarize_batch")
        return out, counts, thr

    # ---- thinning of packed bit maps -------------------------------------------------------------
    def dev_thin_bits(self, d_bits: int, n_frames: int, h: int, w: int, method: int, d_out_bits: int, d_info: int = 0,
                      max_iterations: int = 0):
        """Thins device bit maps [n_frames][h][ceil(w / 8)] into d_out_bits and, if given, 4 int64 a frame at d_info (set bits,
        iterations, pixels deleted, converged).  max_iterations >= 1: asynchronous; 0 (to the fixed point): the stream is
        synchronised before the call returns."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_thin_bits(self._h, v(d_bits or None), n_frames, h, w, int(method), int(max_iterations),
                                                    v(d_out_bits or None), v(d_info or None)), "dev_thin_bits")

    def dev_canny_thin(self, n_frames: int, h: int, w: int, method: int, d_out_bits: int, d_info: int = 0,
                       max_iterations: int = 0):
        """The same on the strong bit-plane the preceding dev_canny of the same geometry left in the context."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_thin(self._h, n_frames, h, w, int(method), int(max_iterations),
                                                     v(d_out_bits or None), v(d_info or None)), "dev_canny_thin")

    def thin_batch(self, bits, w: int, method: int = THIN_GUOHALL, max_iterations: int = 0):
        """Upload and the operator on the GPU: bit maps uint8 [N, H, ceil(w / 8)] -> (bit maps, info int64 [N, 4])."""
        a = _thin_maps(bits, w)
        n, h, _ = a.shape
        out, info = np.zeros_like(a), np.zeros((n, THIN_INFO), np.int64)
        self._check(self._L.canny_hip_thin_batch(self._h, _hp(a), n, h, int(w), int(method), int(max_iterations), _hp(out),
                                                 _hp(info)), "thin_batch")
        return out, info

    # ---- morphological reconstruction of packed bit maps ------------------------------------------
    def dev_reconstruct_bits(self, d_marker: int, d_mask: int, n_frames: int, h: int, w: int, op: int, connectivity: int,
                             d_out_bits: int, d_info: int = 0):
        """Floods the start set of `op` (d_marker for RECON_SEEDED, else 0: the border ring) inside device bit maps
        [n_frames][h][ceil(w / 8)] to the fixed point, into d_out_bits and, if given, 3 int64 a frame at d_info (set bits of the
        output, of the mask, of the start set).  The stream is synchronised before the call returns."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_reconstruct_bits(self._h, v(d_marker or None), v(d_mask or None), n_frames, h, w, int(op),
                                                           int(connectivity), v(d_out_bits or None), v(d_info or None)),
                    "dev_reconstruct_bits")

    def dev_canny_reconstruct(self, d_marker: int, n_frames: int, h: int, w: int, op: int, connectivity: int, d_out_bits: int,
                              d_info: int = 0):
        """The same with the strong bit-plane the preceding dev_canny of the same geometry left in the context as the mask."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_reconstruct(self._h, v(d_marker or None), n_frames, h, w, int(op), int(connectivity),
                                                            v(d_out_bits or None), v(d_info or None)), "dev_canny_reconstruct")

    def reconstruct_batch(self, marker, mask, w: int, op: int = RECON_SEEDED, connectivity: int = 8):
        """Upload and the operator on the GPU: bit maps uint8 [N, H, ceil(w / 8)] -> (bit maps, info int64 [N, 3])."""
        k, m = _recon_maps(marker, mask, w, op)
        n, h, _ = m.shape
        out, info = np.zeros_like(m), np.zeros((n, RECON_INFO), np.int64)
        self._check(self._L.canny_hip_reconstruct_batch(self._h, None if k is None else _hp(k), _hp(m), n, h, int(w), int(op),
                                                        int(connectivity), _hp(out), _hp(info)), "reconstruct_batch")
        return out, info

    # ---- grey-level morphology and median filtering of u8 planes -----------------------------------
    def dev_gray_morph(self, d_plane: int, n_frames: int, h: int, w: int, op: int, rows, kw: int, kh: int, d_out: int,
                       border_mode: int = GRAY_BORDER_NEUTRAL, border_value: int = 0, iterations: int = 1):
        """The grey-level operator on device planes uint8 [n_frames][h][w] (d_plane 0: the smoothed plane the preceding
        dev_canny of the same geometry left in the context) into d_out of the same size.  Asynchronous."""
        v = C.c_void_p
        r = _morph_rows(rows, kh)
        self._check(self._L.canny_hip_dev_gray_morph(self._h, v(d_plane or None), n_frames, h, w, int(op), _hp(r), kw, kh,
                                                     int(border_mode), int(border_value), int(iterations), v(d_out or None)),
                    "dev_gray_morph")

    def gray_morph_batch(self, imgs, op: int, rows, kw: int, kh: int, border_mode: int = GRAY_BORDER_NEUTRAL,
                         border_value: int = 0, iterations: int = 1):
        """Upload, the grey-level operator on the GPU and download: imgs (N, H, W) uint8 -> planes of the same shape."""
        a = _gray_planes(imgs)
        n, h, w = a.shape
        r = _morph_rows(rows, kh)
        out = np.zeros_like(a)
        self._check(self._L.canny_hip_gray_morph_batch(self._h, _hp(a), n, h, w, int(op), _hp(r), int(kw), int(kh),
                                                       int(border_mode), int(border_value), int(iterations), _hp(out)),
                    "gray_morph_batch")
        return out

    # ---- image pyramids of u8 planes --------------------------------------------------------------
    def dev_pyr_down(self, d_plane: int, n_frames: int, h: int, w: int, d_out: int):
        """pyrDown of device planes uint8 [n_frames][h][w] (d_plane 0: the smoothed plane the preceding dev_canny of the same
        geometry left in the context) into d_out [n_frames][(h + 1) // 2][(w + 1) // 2].  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_pyr_down(self._h, v(d_plane or None), n_frames, h, w, v(d_out or None)), "dev_pyr_down")

    def dev_pyramid(self, d_plane: int, n_frames: int, h: int, w: int, levels: int, d_out: int):
        """The levels 1..levels into d_out in the layout of pyramid_layout, one launch per level.  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_pyramid(self._h, v(d_plane or None), n_frames, h, w, int(levels), v(d_out or None)),
                    "dev_pyramid")

    def dev_pyr_up(self, d_plane: int, n_frames: int, h: int, w: int, oh: int, ow: int, d_out: int):
        """pyrUp of device planes uint8 [n_frames][h][w] into d_out [n_frames][oh][ow].  Asynchronous."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_pyr_up(self._h, v(d_plane or None), n_frames, h, w, int(oh), int(ow), v(d_out or None)),
                    "dev_pyr_up")

    def pyramid_batch(self, imgs, levels: int):
        """Upload, the levels on the GPU and download: imgs (N, H, W) uint8 -> a list of arrays [N, h_l, w_l]."""
        a = _gray_planes(imgs)
        n, h, w = a.shape
        info, total = pyramid_layout(n, h, w, levels)
        out = np.zeros(total, np.uint8)
        self._check(self._L.canny_hip_pyramid_batch(self._h, _hp(a), n, h, w, int(levels), _hp(out)), "pyramid_batch")
        return _pyramid_levels(out, n, info)

    def pyr_up_batch(self, imgs, oh: int, ow: int):
        """Upload, pyrUp on the GPU and download: imgs (N, H, W) uint8 -> (N, oh, ow)."""
        a = _gray_planes(imgs)
        n, h, w = a.shape
        out = np.zeros((n, max(int(oh), 0), max(int(ow), 0)), np.uint8)
        self._check(self._L.canny_hip_pyr_up_batch(self._h, _hp(a), n, h, w, int(oh), int(ow), _hp(out)), "pyr_up_batch")
        return out

    def profile_part(self, feature: str, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part `part` of the named group of the profile table ("stages", "hough", ..., "morph",
        "binarize": BIN_PARTS, "thin": THIN_PARTS, "reconstruct": RECON_PARTS, "pyramid": PYR_PARTS): what the group's own getter answers."""
        ms, n = C.c_double(0), C.c_long(0)
        self._check(self._L.canny_hip_profile_part_get(self._h, str(feature).encode(), int(part), C.byref(ms), C.byref(n)),
                    "profile_part_get")
        return ms.value, n.value

    def motion_profile_get(self, part: int) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0 gather, 1 score, 2 refit (MOTION_PARTS)."""
        return self._profile_part("motion_profile_get", part)

    # ---- sub-pixel circle fits (least-squares refit of the Hough circles from edgels) ------
    def canny_hough_circle_fits(self, imgs, sigma: float, min_val: int, max_val: int, min_radius: int, max_radius: int,
                                cell_shift: int = 0, threshold: int = 20, support_threshold: int = 10, min_dist: int = 0,
                                centres_max: int = 256, band: int = 1, trim_q8: int = 0,
                                options: int = CIRCLE_FIT_REFINED_ONLY):
        """canny_hough_circles plus one circle-fit record per circle, all on the GPU: imgs (H, W) or (N, H, W) uint8 ->
        (records, counts, centre_counts, fits); records[f] int32 [k, 6] and fits[f] int32 [k, 8], slot for slot; unpack
        the fits with circle_fits_unpack."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected uint8 [H, W] or [n_frames, H, W]")
        n, h, w = a.shape
        rec = np.zeros((n, max(int(centres_max), 1), CIRCLE_INTS), np.int32)
        fits = np.zeros((n, max(int(centres_max), 1), CIRCLE_FIT_INTS), np.int32)
        counts, peaks = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self._L.canny_hip_canny_hough_circle_fits(self._h, _hp(a), n, sigma, min_val, max_val, h, w, min_radius,
                                                              max_radius, cell_shift, threshold, support_threshold,
                                                              min_dist, centres_max, band, trim_q8, options, _hp(rec),
                                                              _hp(counts), _hp(peaks), _hp(fits)),
                    "canny_hough_circle_fits")
        return ([rec[f, :int(counts[f])].copy() for f in range(n)], counts, peaks,
                [fits[f, :int(counts[f])].copy() for f in range(n)])

    def dev_circle_fits_bits(self, d_bits: int, d_plane: int, plane_is_u8: bool, n: int, h: int, w: int, d_circles: int,
                             d_counts: int, centres_max: int, band: int, trim_q8: int, options: int, d_fits: int):
        """The fits of circle records on the device (d_circles, d_counts; an earlier call's or the caller's) on device bit
        maps (layout of dev_canny_bits) and a device plane (u8 or s16; 0 = the smoothed plane the last canny call of the
        same shape left).  d_fits: n * centres_max * 8 int32, 16-byte aligned."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_circle_fits_bits(self._h, v(d_bits or None), v(d_plane or None), int(plane_is_u8),
                                                           n, h, w, v(d_circles or None), v(d_counts or None), centres_max,
                                                           band, trim_q8, options, v(d_fits or None)),
                    "dev_circle_fits_bits")

    def dev_canny_hough_circle_fits(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                                    min_radius: int, max_radius: int, cell_shift: int, threshold: int,
                                    support_threshold: int, min_dist: int, centres_max: int, band: int, trim_q8: int,
                                    options: int, d_fits: int, d_circles: int = 0, d_counts: int = 0,
                                    d_centre_counts: int = 0, d_accum: int = 0, d_edges: int = 0):
        """dev_canny_hough_circles, then the fits of its circles queued behind it on the same stream; d_circles and
        d_counts are optional (0: a context workspace holds them)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_canny_hough_circle_fits(self._h, v(d_img or None), sigma, min_val, max_val, h, w,
                                                                  n, v(d_edges or None), min_radius, max_radius,
                                                                  cell_shift, threshold, support_threshold, min_dist,
                                                                  centres_max, v(d_circles or None), v(d_counts or None),
                                                                  v(d_centre_counts or None), v(d_accum or None), band,
                                                                  trim_q8, options, v(d_fits or None)),
                    "dev_canny_hough_circle_fits")

    def dev_circle_fits_arith(self, d_moments: int, n_sets: int, d_out: int):
        """Test hook: the device finishing arithmetic on n_sets x 12 int64 moment sets -> n_sets x 4 int32 (move_x, move_y,
        n, DEGENERATE or 0)."""
        v = C.c_void_p
        self._check(self._L.canny_hip_dev_circle_fits_arith(self._h, v(d_moments or None), n_sets, v(d_out or None)),
                    "dev_circle_fits_arith")

    def circle_fits_profile_get(self, part: int = 0) -> Tuple[float, int]:
        """(total ms, launch groups) of part 0, the fit kernel (CIRCLE_FIT_PART_FIT)."""
        return self._profile_part("circle_fits_profile_get", part)

    # ---- colour frames (interleaved BGR / RGB / BGRA / RGBA; the rule is the "gray_rule" option) --------------
    def to_gray(self, frame, order: str = "bgr") -> np.ndarray:
        """(H, W, 3|4) uint8 frame -> its (H, W) gray plane, converted on the GPU."""
        a, lay = _frame(frame, order)
        out = np.empty(a.shape[:2], np.uint8)
        self._check(self._L.canny_hip_to_gray(self._h, _hp(a), lay, a.shape[0], a.shape[1], _hp(out)), "to_gray")
        return out

    def canny_color(self, frame, sigma: float, min_val: int, max_val: int, order: str = "bgr") -> np.ndarray:
        """canny() of a colour frame: the same map as canny(to_gray(frame))."""
        a, lay = _frame(frame, order)
        out = np.empty(a.shape[:2], np.int16)
        self._check(self._L.canny_hip_canny_color(self._h, _hp(a), lay, sigma, min_val, max_val, a.shape[0],
                                                  a.shape[1], _hp(out)), "canny_color")
        return out

    def canny_batch_color(self, imgs, sigma: float, min_val: int, max_val: int, order: str = "bgr",
                          out: Optional[np.ndarray] = None, fmt: str = "s16") -> np.ndarray:
        """canny_batch() of (N, H, W, 3|4) colour frames; fmt "s16" (int16 maps), "u8" or "bits" (see canny_batch)."""
        a, lay = _frame(imgs, order, batch=True)
        if fmt not in ("s16", "u8", "bits"):
            raise ValueError(f"fmt must be 's16', 'u8' or 'bits', not {fmt!r}")
        n, h, w = a.shape[:3]
        dtype = np.int16 if fmt == "s16" else np.uint8
        shape = bits_shape((n, h, w)) if fmt == "bits" else (n, h, w)
        if out is None:
            out = np.empty(shape, dtype)
        elif out.shape != shape or out.dtype != dtype or not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"out must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        fn = {"s16": self._L.canny_hip_canny_batch_color, "u8": self._L.canny_hip_canny_batch_color_u8,
              "bits": self._L.canny_hip_canny_batch_color_bits}[fmt]
        self._check(fn(self._h, _hp(a), lay, n, sigma, min_val, max_val, h, w, _hp(out)), "canny_batch_color")
        return out

    def selftest_mag_angle(self, lim: int = 1020):
        side = 2 * lim + 1
        mags = np.empty((side, side), np.int16)
        bins = np.empty((side, side), np.uint8)
        self._check(self._L.canny_hip_selftest_mag_angle(self._h, lim, _hp(mags), _hp(bins)), "selftest")
        return mags, bins

    def selftest_sobel_pixel(self, form: int, lim: int = 1020):
        """Magnitude and bin tables of one Sobel+NMS kernel form's per-pixel helpers (PIXEL_* constants), indexed
        [gy + lim, gx + lim] like selftest_mag_angle."""
        side = 2 * lim + 1
        mags = np.empty((side, side), np.int16)
        bins = np.empty((side, side), np.uint8)
        self._check(self._L.canny_hip_selftest_sobel_pixel(self._h, form, lim, _hp(mags), _hp(bins)),
                    "selftest_sobel_pixel")
        return mags, bins

    def selftest_div(self, divisor: float) -> Tuple[int, float]:
        """(mismatches, largest mismatching dividend) of the Gaussian's reciprocal division against IEEE
        a/divisor over all floats a in [0,256]."""
        bad, worst = C.c_ulonglong(0), C.c_float(0.0)
        self._check(self._L.canny_hip_selftest_div(self._h, divisor, C.byref(bad), C.byref(worst)), "selftest_div")
        return bad.value, worst.value

    def selftest_div_fma(self, divisor: float, c: float) -> Tuple[int, float]:
        """Same for the one-instruction form fma(a, c, a)."""
        bad, worst = C.c_ulonglong(0), C.c_float(0.0)
        self._check(self._L.canny_hip_selftest_div_fma(self._h, divisor, c, C.byref(bad), C.byref(worst)),
                    "selftest_div_fma")
        return bad.value, worst.value

    def selftest_histogram(self, d_plane: int, plane_is_u8: bool, kind, h: int, w: int, n: int, d_hist: int):
        """The automatic rules' histogram pass alone on a device plane (bytes or shorts in [0,255], n frames of h x w):
        kind "median" counts the values, "quantile" min(Sobel magnitude, 256), into d_hist (n x 257 uint32, device; zeroed
        first).  Asynchronous."""
        self._check(self._L.canny_hip_selftest_histogram(self._h, C.c_void_p(d_plane), int(plane_is_u8), _rule(kind), h,
                                                         w, n, C.c_void_p(d_hist)), "selftest_histogram")

    def selftest_select(self, d_hist: int, n: int, rule, low: float, high: float, d_pairs: int):
        """The select pass alone: the rule on n device histograms (n x 257 uint32) -> d_pairs (2 * n int32, device)."""
        self._check(self._L.canny_hip_selftest_select(self._h, C.c_void_p(d_hist), n, _rule(rule), low, high,
                                                      C.c_void_p(d_pairs)), "selftest_select")

    # ---- device-pointer stage API (ints are device addresses; n_frames contiguous planes) -------
    def selftest_workspaces(self):
        """Every device workspace of the context as (name, device pointer, allocated bytes, kind) -- kind is WS_DATA,
        WS_INDEX or WS_CACHE (canny_hip_selftest_workspace).  Synchronises the stream; launches and changes nothing."""
        out, index = [], 0
        while True:
            name, ptr, size, kind = C.c_char_p(), C.c_void_p(), C.c_size_t(), C.c_int()
            st = self._L.canny_hip_selftest_workspace(self._h, index, C.byref(name), C.byref(ptr), C.byref(size),
                                                      C.byref(kind))
            if st == 1 and index > 0:  # CANNY_HIP_ERR_INVALID: past the end
                return out
            self._check(st, "selftest_workspace")
            out.append((name.value.decode(), ptr.value or 0, size.value, kind.value))
            index += 1

    def dev_gaussian(self, d_img: int, sigma: float, h: int, w: int, n: int, d_out: int):
        self._check(self._L.canny_hip_dev_gaussian(self._h, C.c_void_p(d_img), sigma, h, w, n, C.c_void_p(d_out)),
                    "dev_gaussian")

    def dev_xy_gradient(self, d_img: int, h: int, w: int, n: int, d_gx: int, d_gy: int):
        self._check(self._L.canny_hip_dev_xy_gradient(self._h, C.c_void_p(d_img), h, w, n, C.c_void_p(d_gx),
                                                      C.c_void_p(d_gy)), "dev_xy_gradient")

    def dev_sobel(self, d_img: int, h: int, w: int, n: int, d_mag: int, d_ang: int):
        self._check(self._L.canny_hip_dev_sobel(self._h, C.c_void_p(d_img), h, w, n, C.c_void_p(d_mag),
                                                C.c_void_p(d_ang)), "dev_sobel")

    def dev_nms(self, d_mag: int, d_ang: int, h: int, w: int, n: int, d_out: int):
        self._check(self._L.canny_hip_dev_nms(self._h, C.c_void_p(d_mag), C.c_void_p(d_ang), h, w, n,
                                              C.c_void_p(d_out)), "dev_nms")

    def dev_sobel_nms(self, d_smoothed: int, h: int, w: int, n: int, d_out: int):
        self._check(self._L.canny_hip_dev_sobel_nms(self._h, C.c_void_p(d_smoothed), h, w, n, C.c_void_p(d_out)),
                    "dev_sobel_nms")

    def probe_copy(self, d_src: int, d_dst: int, nbytes: int, launches: int = 10) -> float:
        """Average device milliseconds of a plain copy of nbytes (measurement aid, see canny_hip_probe_copy)."""
        ms = C.c_double(0)
        self._check(self._L.canny_hip_probe_copy(self._h, C.c_void_p(d_src), C.c_void_p(d_dst), nbytes, launches,
                                                 C.byref(ms)), "probe_copy")
        return ms.value

    def dev_gaussian_u8(self, d_img: int, sigma: float, h: int, w: int, n: int, d_out: int):
        """Gaussian storing the smoothed plane as bytes (the "smoothed_u8" path of canny())."""
        self._check(self._L.canny_hip_dev_gaussian_u8(self._h, C.c_void_p(d_img), sigma, h, w, n, C.c_void_p(d_out)),
                    "dev_gaussian_u8")

    def dev_sobel_nms_u8in(self, d_smoothed: int, h: int, w: int, n: int, d_out: int):
        self._check(self._L.canny_hip_dev_sobel_nms_u8in(self._h, C.c_void_p(d_smoothed), h, w, n, C.c_void_p(d_out)),
                    "dev_sobel_nms_u8in")

    def dev_hysteresis(self, d_cand: int, h: int, w: int, n: int, min_val: int, max_val: int):
        self._check(self._L.canny_hip_dev_hysteresis(self._h, C.c_void_p(d_cand), h, w, n, min_val, max_val),
                    "dev_hysteresis")

    def dev_canny(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, d_edges: int):
        self._check(self._L.canny_hip_dev_canny(self._h, C.c_void_p(d_img), sigma, min_val, max_val, h, w, n,
                                                C.c_void_p(d_edges)), "dev_canny")

    def dev_canny_stream(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int,
                         d_edges: int):
        """canny() for a stream of batches: returns with this batch's hysteresis sweeps in flight; d_edges is
        complete once the next dev_canny_stream call or dev_canny_stream_flush() has returned."""
        self._check(self._L.canny_hip_dev_canny_stream(self._h, C.c_void_p(d_img), sigma, min_val, max_val, h, w, n,
                                                       C.c_void_p(d_edges)), "dev_canny_stream")

    def dev_canny_stream_flush(self):
        self._check(self._L.canny_hip_dev_canny_stream_flush(self._h), "dev_canny_stream_flush")

    def dev_canny_bits(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, d_bits: int):
        self._check(self._L.canny_hip_dev_canny_bits(self._h, C.c_void_p(d_img), sigma, min_val, max_val, h, w, n,
                                                     C.c_void_p(d_bits)), "dev_canny_bits")

    def dev_canny_u8(self, d_img: int, sigma: float, min_val: int, max_val: int, h: int, w: int, n: int, d_edges: int):
        self._check(self._L.canny_hip_dev_canny_u8(self._h, C.c_void_p(d_img), sigma, min_val, max_val, h, w, n,
                                                   C.c_void_p(d_edges)), "dev_canny_u8")

    def dev_to_gray(self, d_src: int, layout: int, h: int, w: int, n: int, d_gray: int):
        self._check(self._L.canny_hip_dev_to_gray(self._h, C.c_void_p(d_src), layout, h, w, n, C.c_void_p(d_gray)),
                    "dev_to_gray")

    def dev_gaussian_u8_color(self, d_src: int, layout: int, sigma: float, h: int, w: int, n: int, d_out: int):
        """The fused Gaussian alone (colour in, u8 smoothed plane out); raises UNSUPPORTED where it does not apply."""
        self._check(self._L.canny_hip_dev_gaussian_u8_color(self._h, C.c_void_p(d_src), layout, sigma, h, w, n,
                                                            C.c_void_p(d_out)), "dev_gaussian_u8_color")

    def dev_canny_color(self, d_src: int, layout: int, sigma: float, min_val: int, max_val: int, h: int, w: int,
                        n: int, d_edges: int):
        self._check(self._L.canny_hip_dev_canny_color(self._h, C.c_void_p(d_src), layout, sigma, min_val, max_val, h,
                                                      w, n, C.c_void_p(d_edges)), "dev_canny_color")


def bits_shape(frames_shape) -> Tuple[int, int, int]:
    """Shape of the bit maps of [n_frames, H, W] frames: every row padded to whole bytes."""
    n, h, w = frames_shape
    return (n, h, (w + 7) // 8)


def unpack_bits(bits: np.ndarray, width: int) -> np.ndarray:
    """Bit maps [n_frames, H, (W + 7) // 8] -> the reference's int16 edge maps (0 / 255)."""
    return np.unpackbits(bits, axis=-1)[..., :width].astype(np.int16) * 255


def canny_multi_gpu(imgs, sigma: float, min_val: int, max_val: int, n_devices: int = 0, u8: bool = False,
                    out: Optional[np.ndarray] = None, bits: bool = False) -> np.ndarray:
    """Shard [n_frames, H, W] by contiguous ranges over the node's GPUs (one host thread per GPU, each running
    the batch pipeline; per-device contexts are cached until multi_gpu_release())."""
    a = np.ascontiguousarray(imgs, dtype=np.uint8)
    if a.ndim != 3:
        raise ValueError("expected uint8 [n_frames, H, W]")
    dtype = np.uint8 if (u8 or bits) else np.int16
    shape = bits_shape(a.shape) if bits else a.shape
    if out is None:
        out = np.empty(shape, dtype)
    elif out.shape != shape or out.dtype != dtype or not out.flags["C_CONTIGUOUS"]:
        raise ValueError(f"out must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
    fn = load().canny_hip_canny_multi_gpu_bits if bits else \
        (load().canny_hip_canny_multi_gpu_u8 if u8 else load().canny_hip_canny_multi_gpu)
    _ok(fn(_hp(a), a.shape[0], sigma, min_val, max_val, a.shape[1], a.shape[2], _hp(out), n_devices), "canny_multi_gpu")
    return out


def multi_gpu_set_option(name: str, value: int):
    _ok(load().canny_hip_multi_gpu_set_option(name.encode(), value), f"multi_gpu_set_option({name})")


def multi_gpu_release():
    load().canny_hip_multi_gpu_release()


def device_local_cpus(device: int) -> Optional[str]:
    """sysfs CPU list local to a GPU ("0-31,128-159"), None if the platform does not say."""
    buf = C.create_string_buffer(4096)
    st = load().canny_hip_device_local_cpus(device, buf, len(buf))
    return buf.value.decode() if st == 0 else None


def cpulist_count(text: str) -> int:
    return load().canny_hip_selftest_cpulist_count(text.encode())


# ---- the reference's stage names (src/utils.h:8-22) on a default context per calling thread --------
# (the reference's functions are re-entrant; a context serves one thread at a time, so -- like the C++ shim's
# thread_local context, csrc/utils_shim.cpp -- every thread that uses these names gets a context of its own)
_default = threading.local()


def default_context() -> Context:
    ctx = getattr(_default, "ctx", None)
    if ctx is None:
        ctx = _default.ctx = Context(int(os.environ.get("CANNY_HIP_DEVICE", "0")))
    return ctx


def createGaussianKernel(sigma: float) -> np.ndarray:
    """src/utils.cpp:77-95 (host-side): returns the normalised float taps; len() is the window."""
    taps = np.zeros(129, np.float32)
    w = C.c_int(0)
    _ok(load().canny_hip_gaussian_kernel(sigma, _hp(taps), taps.size, C.byref(w)), "createGaussianKernel")
    return taps[:w.value].copy()


def gaussian(img, sigma: float) -> np.ndarray:
    return default_context().gaussian(img, sigma)


def calculateXYGradient(img):
    return default_context().xy_gradient(img)


def sobelOperator(img):
    return default_context().sobel(img)


def nonmaximalSuppression(grad, angle) -> np.ndarray:
    return default_context().nms(grad, angle)


def hysteresis(edgeCandidates, minVal: int, maxVal: int) -> np.ndarray:
    return default_context().hysteresis(edgeCandidates, minVal, maxVal)


def findEdgePixels(edgeCandidates, visited, start: int, minVal: int, maxVal: int):
    return default_context().find_edge_pixels(edgeCandidates, visited, start, minVal, maxVal)


def canny(img, sigma: float, minVal: int, maxVal: int) -> np.ndarray:
    return default_context().canny(img, sigma, minVal, maxVal)


def canny_color(frame, sigma: float, minVal: int, maxVal: int, order: str = "bgr") -> np.ndarray:
    """canny() of an (H, W, 3|4) colour frame -- the reference's cvtColor + canny() (src/main.cpp:114-136)."""
    return default_context().canny_color(frame, sigma, minVal, maxVal, order)


def canny_auto(img, sigma: float, rule="median", low: float = 0.67, high: float = 1.33):
    """canny() with per-frame thresholds chosen on the GPU (see Context.canny_auto): returns (edges, thresholds)."""
    return default_context().canny_auto(img, sigma, rule, low, high)
