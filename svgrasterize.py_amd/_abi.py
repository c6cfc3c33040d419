"""ctypes binding of libsvgr_hip.so (include/svgr.h).

There is deliberately no fallback: if the HIP library is missing or no gfx950 device is
visible, every entry point raises.  The only thing that works without a GPU is loading the
library and inspecting its symbols (used by the CPU-side ABI test).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libsvgr_hip.so")

OUT_CANVAS_F32, OUT_CANVAS_F64, OUT_MASK_F64, OUT_FILL_F64, OUT_MASKS_F64, OUT_FILLS_F64 = 0, 1, 2, 3, 4, 5
RENDER_CLIP01, RENDER_TIMED, RENDER_DETERMINISTIC, RENDER_SAME_GEOMETRY = 1, 2, 4, 8
SEG_LINE, SEG_CUBIC = 0, 1

CONVERT_PRE_TO_STRAIGHT, CONVERT_SRGB_TO_LINEAR, CONVERT_LINEAR_TO_SRGB, CONVERT_STRAIGHT_TO_PRE = 1, 2, 4, 8


class SvgrError(RuntimeError):
    """Raised for every non-zero status of the C ABI except SVGR_E_INVALID (-> ValueError)."""


class BatchDesc(C.Structure):
    _fields_ = [
        ("segs", C.c_void_p), ("seg_kind", C.c_void_p), ("n_segs", C.c_int64),
        ("path_seg_off", C.c_void_p), ("n_paths", C.c_int64),
        ("path_m6", C.c_void_p), ("path_rule", C.c_void_p), ("path_paint", C.c_void_p),
        ("viewport", C.c_int64 * 4), ("flatness", C.c_double),
    ]


class BatchStats(C.Structure):
    _fields_ = [
        ("n_edges", C.c_int64), ("path_pixels", C.c_int64), ("n_band_segs", C.c_int64),
        ("n_path_bands", C.c_int64), ("n_nonempty", C.c_int64), ("bbox_union", C.c_int64 * 4),
        ("tile_rows", C.c_int64), ("tile_cols", C.c_int64),
    ]


class Gradient(C.Structure):
    _fields_ = [
        ("kind", C.c_int), ("spread", C.c_int), ("has_gt", C.c_int), ("n_stops", C.c_int), ("excl_enabled", C.c_int),
        ("user_m6", C.c_double * 6), ("gt_m6", C.c_double * 6),
        ("p0", C.c_double * 2), ("vec", C.c_double * 2), ("vv", C.c_double),
        ("center", C.c_double * 2), ("radius", C.c_double),
        ("fcenter", C.c_double * 2), ("fradius", C.c_double), ("cd", C.c_double * 2), ("rd", C.c_double), ("a", C.c_double),
        ("frad_rd", C.c_double), ("frad2", C.c_double), ("excl_thresh", C.c_double),
        ("stop_off", C.c_void_p), ("stop_rgba", C.c_void_p),
    ]


class PatternArgs(C.Structure):  # svgr_pattern
    _fields_ = [
        ("inv_m6", C.c_double * 6), ("fwd_m6", C.c_double * 6), ("cell", C.c_double * 4),
        ("min_xy", C.c_int64 * 2), ("pat_shape", C.c_int64 * 2), ("tile_bbox", C.c_int64 * 4),
    ]


class ImageArgs(C.Structure):  # svgr_image
    _fields_ = [
        ("inv_m6", C.c_double * 6), ("height", C.c_int64), ("width", C.c_int64), ("lod", C.c_double), ("smooth", C.c_int),
    ]


class JpegFrame(C.Structure):  # svgr_jpeg_frame
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("n_comp", C.c_int32), ("h", C.c_int32 * 3), ("v", C.c_int32 * 3),
        ("colour", C.c_int32),
    ]


class JpegScan(C.Structure):  # svgr_jpeg_scan
    _fields_ = [
        ("frame", JpegFrame), ("progressive", C.c_int32), ("restart_interval", C.c_int32), ("n_scan", C.c_int32),
        ("scan_comp", C.c_int32 * 3), ("dc_table", C.c_int32 * 3), ("ac_table", C.c_int32 * 3),
        ("ss", C.c_int32), ("se", C.c_int32), ("ah", C.c_int32), ("al", C.c_int32),
    ]


class TensorDesc(C.Structure):  # svgr_tensor_desc
    _fields_ = [
        ("source", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32), ("has_bg", C.c_int32), ("bg", C.c_double * 3),
        ("scale", C.c_double * 4), ("bias", C.c_double * 4), ("rows", C.c_int64), ("cols", C.c_int64),
        ("stride_c", C.c_int64), ("stride_h", C.c_int64), ("stride_w", C.c_int64), ("offset", C.c_int64),
    ]


class CoverDesc(C.Structure):  # svgr_cover_desc
    _fields_ = [
        ("n_segs", C.c_int64), ("n_paths", C.c_int64), ("viewport", C.c_int64 * 4), ("flatness", C.c_double), ("plane", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ComposeDesc(C.Structure):  # svgr_compose_desc
    _fields_ = [
        ("n_paths", C.c_int64), ("rows", C.c_int64), ("cols", C.c_int64), ("bg", C.c_double * 4), ("plane", C.c_int32), ("has_bg", C.c_int32),
    ]


class PaintedDesc(C.Structure):  # svgr_painted_desc
    _fields_ = [
        ("n_paths", C.c_int64), ("rows", C.c_int64), ("cols", C.c_int64), ("bg", C.c_double * 4), ("plane", C.c_int32), ("has_bg", C.c_int32),
        ("row0", C.c_int64), ("col0", C.c_int64), ("n_stops", C.c_int64), ("kind", C.POINTER(C.c_int32)), ("spread", C.POINTER(C.c_int32)),
        ("path_stop_off", C.POINTER(C.c_int32)),
    ]


class GroupedDesc(C.Structure):  # svgr_grouped_desc
    _fields_ = PaintedDesc._fields_ + [
        ("n_items", C.c_int64), ("n_groups", C.c_int64), ("n_clip_planes", C.c_int64), ("n_opacities", C.c_int64),
        ("items", C.POINTER(C.c_int32)), ("clip_off", C.POINTER(C.c_int32)), ("clip_planes", C.POINTER(C.c_int32)),
    ]


TENSOR_SRC_RGBA_F64, TENSOR_SRC_RGBA_F32, TENSOR_SRC_MASK_F64 = 0, 1, 2
COVER_F64, COVER_F32 = 0, 1
COVER_STATUS_DEPTH, COVER_STATUS_RANGE = 1, 2
TENSOR_F32, TENSOR_F16, TENSOR_BF16, TENSOR_U8 = 0, 1, 2, 3
TENSOR_RGBA, TENSOR_RGB, TENSOR_ALPHA, TENSOR_LUMA = 0, 1, 2, 3
JPEG_GREY, JPEG_YCBCR, JPEG_RGB = 0, 1, 2
_JPEG_STATUS = {1: "the entropy-coded data ends before the scan does", 2: "a bad Huffman table or code",
                3: "a restart marker is missing or out of sequence", 4: "a run of zeros leads past the end of the block"}
JPEG_NO_ROOM = 5

_P = C.c_void_p
_PROTOS = {
    "svgr_abi_version": (C.c_int, []),
    "svgr_hash_buffers": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_uint64)]),
    "svgr_tile_rows": (C.c_int, []),
    "svgr_tile_cols": (C.c_int, []),
    "svgr_last_error": (C.c_char_p, []),
    "svgr_device_count": (C.c_int, []),
    "svgr_init": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "svgr_shutdown": (C.c_int, [_P]),
    "svgr_set_stream": (C.c_int, [_P, _P]),
    "svgr_sync": (C.c_int, [_P]),
    "svgr_device_name": (C.c_int, [_P, C.c_char_p, C.c_size_t]),
    "svgr_measure_begin": (C.c_int, [_P, C.c_double]),
    "svgr_measure_end": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "svgr_measure_launches": (C.c_int, [C.POINTER(C.c_uint64)]),
    "svgr_buf_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "svgr_buf_wrap": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(_P)]),
    "svgr_buf_free": (C.c_int, [_P, _P]),
    "svgr_buf_ptr": (_P, [_P]),
    "svgr_buf_bytes": (C.c_size_t, [_P]),
    "svgr_buf_zero": (C.c_int, [_P, _P]),
    "svgr_buf_copy": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "svgr_upload": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "svgr_download": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "svgr_batch_create": (C.c_int, [_P, C.POINTER(BatchDesc), C.POINTER(_P)]),
    "svgr_batch_destroy": (C.c_int, [_P]),
    "svgr_batch_set_paints": (C.c_int, [_P, _P]),
    "svgr_batch_set_transforms": (C.c_int, [_P, _P]),
    "svgr_batch_set_bands": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "svgr_batch_set_groups": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "svgr_batch_set_gradients": (C.c_int, [_P, _P, C.c_int64, _P]),
    "svgr_batch_plan": (C.c_int, [_P]),
    "svgr_batch_get_stats": (C.c_int, [_P, C.POINTER(BatchStats)]),
    "svgr_batch_get_bboxes": (C.c_int, [_P, _P]),
    "svgr_batch_get_edges": (C.c_int, [_P, _P, _P, C.c_int64]),
    "svgr_batch_get_extents": (C.c_int, [_P, _P]),
    "svgr_batch_all_edges": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "svgr_batch_render": (C.c_int, [_P, _P, C.c_int, C.c_uint]),
    "svgr_batch_draw": (C.c_int, [_P, _P, C.c_int, C.c_uint]),
    "svgr_batch_render_window": (C.c_int, [_P, _P, C.c_int, C.c_uint, _P]),
    "svgr_batch_render_windows": (C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_uint, _P]),
    "svgr_batch_plan_many": (C.c_int, [_P, C.c_int64]),
    "svgr_batch_owned_rows": (C.c_int64, [_P]),
    "svgr_batch_timings": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgr_layer_over": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int]),
    "svgr_layer_crop4": (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    "svgr_layer_in": (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    "svgr_layer_scale": (C.c_int, [_P, _P, C.c_int64, C.c_double]),
    "svgr_layer_scale_to": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double]),
    "svgr_layer_background": (C.c_int, [_P, _P, C.c_int64, _P]),
    "svgr_layer_clip01": (C.c_int, [_P, _P, C.c_int64]),
    "svgr_layer_convert": (C.c_int, [_P, _P, C.c_int64, C.c_uint]),
    "svgr_layer_convert_to": (C.c_int, [_P, _P, _P, C.c_int64, C.c_uint]),
    "svgr_layer_convert_scale_to": (C.c_int, [_P, _P, _P, C.c_int64, C.c_uint, C.c_double]),
    "svgr_layer_compose_over": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "svgr_layer_compose_in": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "svgr_layer_to_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int]),
    "svgr_layer_to_rgba8": (C.c_int, [_P, _P, _P, C.c_int64]),
    "svgr_layer_blend": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "svgr_layer_color_matrix": (C.c_int, [_P, _P, C.c_int64, _P]),
    "svgr_layer_morphology": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int]),
    "svgr_layer_luminance": (C.c_int, [_P, _P, _P, C.c_int64]),
    "svgr_layer_turbulence": (C.c_int, [_P, _P, _P, _P, C.c_double, C.c_double, _P, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "svgr_layer_component_transfer": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P]),
    "svgr_layer_convolve_matrix": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_double, C.c_double, C.c_int, C.c_int]),
    "svgr_layer_displacement_map": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_double, C.c_int, C.c_int]),
    "svgr_layer_lighting": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P, C.c_double, C.c_double, C.c_double, C.c_int]),
    "svgr_layer_mix_blend": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int]),
    "svgr_layer_tile": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "svgr_gradient_fill": (C.c_int, [_P, C.POINTER(Gradient), _P, _P, _P]),
    "svgr_gradient_eval": (C.c_int, [_P, C.POINTER(Gradient), _P, C.c_int64, _P]),
    "svgr_pattern_fill": (C.c_int, [_P, C.POINTER(PatternArgs), _P, _P, _P, _P]),
    "svgr_image_upload": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, _P]),
    "svgr_image_fill": (C.c_int, [_P, C.POINTER(ImageArgs), _P, _P, _P, _P]),
    "svgr_layer_convolve": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64]),
    "svgr_layer_convolve_ops": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64, C.c_uint]),
    "svgr_path_stroke": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_int, C.c_int, C.POINTER(_P)]),
    "svgr_path_dash": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, C.c_int64, C.c_double, C.c_double, C.POINTER(_P)]),
    "svgr_dash_scan_segments": (C.c_int, []),
    "svgr_path_markers": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(_P)]),
    "svgr_marker_out_counts": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "svgr_marker_out_copy": (C.c_int, [_P, _P, _P]),
    "svgr_marker_out_free": (None, [_P]),
    "svgr_marker_block_segments": (C.c_int, []),
    "svgr_path_sample": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, C.c_int64, _P, _P, C.POINTER(C.c_double)]),
    "svgr_path_place_glyphs": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64, _P, _P,
                                        C.POINTER(C.c_double)]),
    "svgr_textpath_block": (C.c_int, []),
    "svgr_glyf_outline": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(_P)]),
    "svgr_glyf_block": (C.c_int, []),
    "svgr_gvar_deltas": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    "svgr_glyf_outline_var": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64,
                                        _P, _P, C.c_int64, _P, _P, _P, C.c_int64, C.POINTER(_P)]),
    "svgr_gvar_block": (C.c_int, []),
    "svgr_cff_outline": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(_P)]),
    "svgr_cff_block": (C.c_int, []),
    "svgr_stroke_out_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "svgr_stroke_out_copy": (C.c_int, [_P, _P, _P, _P]),
    "svgr_stroke_out_free": (None, [_P]),
    "svgr_png_unfilter": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P]),
    "svgr_jpeg_entropy": (C.c_int, [C.POINTER(JpegScan), _P, _P, _P, C.c_int64, _P, C.c_int64]),
    "svgr_jpeg_decode": (C.c_int, [_P, C.POINTER(JpegFrame), _P, C.c_int64, _P, _P]),
    "svgr_jpeg_encode": (C.c_int, [_P, C.POINTER(JpegFrame), _P, _P, _P, C.c_int64]),
    "svgr_jpeg_entropy_encode": (C.c_int, [C.POINTER(JpegScan), _P, _P, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "svgr_jpeg_symbol_counts": (C.c_int, [C.POINTER(JpegScan), _P, C.c_int64, _P]),
    "svgr_png_filter": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, _P]),
    "svgr_deflate": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "svgr_deflate_chunk": (C.c_int, []),
    "svgr_layer_to_tensor": (C.c_int, [_P, C.POINTER(TensorDesc), _P, _P, _P]),
    "svgr_tensor_to_layer": (C.c_int, [_P, C.POINTER(TensorDesc), _P, _P]),
    "svgr_tensor_block": (C.c_int, []),
    "svgr_tensor_run": (C.c_int, []),
    "svgr_stream_wait_for": (C.c_int, [_P, _P]),
    "svgr_stream_signal_to": (C.c_int, [_P, _P]),
    "svgr_batch_winding": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "svgr_batch_pick": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, C.c_size_t, _P, _P]),
    "svgr_hit_block": (C.c_int, []),
    "svgr_hit_chunk": (C.c_int, []),
    "svgr_batch_distance": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_int, C.c_size_t, _P]),
    "svgr_batch_msdf": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_int, _P, _P, _P, C.c_int64, C.c_size_t, _P]),
    "svgr_quant_distinct": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "svgr_quant_bins": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "svgr_quant_index": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int, _P, _P]),
    "svgr_quant_block": (C.c_int, []),
    "svgr_quant_groups": (C.c_int, []),
    "svgr_quant_dither": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "svgr_dither_tile_rows": (C.c_int, []),
    "svgr_dither_tile_cols": (C.c_int, []),
    "svgr_png_samples": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, _P]),
    "svgr_png_filter_bytes": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, C.c_int, _P]),
    "svgr_png_filter_span": (C.c_int, []),
    "svgr_cover_forward": (C.c_int, [_P, C.POINTER(CoverDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "svgr_cover_backward": (C.c_int, [_P, C.POINTER(CoverDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "svgr_cover_block": (C.c_int, []),
    "svgr_cover_scan": (C.c_int, []),
    "svgr_compose_forward": (C.c_int, [_P, C.POINTER(ComposeDesc), _P, _P, _P]),
    "svgr_compose_backward": (C.c_int, [_P, C.POINTER(ComposeDesc), _P, _P, _P, _P, _P]),
    "svgr_compose_block": (C.c_int, []),
    "svgr_compose_groups": (C.c_int, []),
    "svgr_compose_painted_forward": (C.c_int, [_P, C.POINTER(PaintedDesc)] + [_P] * 7),
    "svgr_compose_painted_backward": (C.c_int, [_P, C.POINTER(PaintedDesc)] + [_P] * 13),
    "svgr_compose_grouped_forward": (C.c_int, [_P, C.POINTER(GroupedDesc)] + [_P] * 8),
    "svgr_compose_grouped_backward": (C.c_int, [_P, C.POINTER(GroupedDesc)] + [_P] * 15),
    "svgr_group_depth": (C.c_int, []),
    "svgr_compose_masked_forward": (C.c_int, [_P, C.POINTER(GroupedDesc)] + [_P] * 8),
    "svgr_compose_masked_backward": (C.c_int, [_P, C.POINTER(GroupedDesc)] + [_P] * 15),
}
EXPORTS = tuple(_PROTOS)

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen libsvgr_hip.so and declare prototypes; raises if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise SvgrError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)"
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def tile_rows() -> int:
    """Band height of the built library (row granularity of Batch.set_bands)."""
    return int(load_library().svgr_tile_rows())


def tile_cols() -> int:
    """Tile width of the built library."""
    return int(load_library().svgr_tile_cols())


def _check(rc: int):
    if rc == 0:
        return
    msg = load_library().svgr_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    raise SvgrError(f"svgr status {rc}: {msg}")


class Context:
    """One per device (svgr_ctx)."""

    _by_device: dict[int, "Context"] = {}

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = _P()
        _check(self.lib.svgr_init(device, C.byref(h)))
        self.handle = h
        self.device = device
        self._fin = weakref.finalize(self, self.lib.svgr_shutdown, h)

    _default: "Context | None" = None   # the context of $SVGR_DEVICE / $LOCAL_RANK, resolved once (a document render asks 200 times)

    @classmethod
    def get(cls, device: int | None = None) -> "Context":
        if device is None:
            ctx = cls._default
            if ctx is not None:
                return ctx
            device = int(os.environ.get("SVGR_DEVICE") or os.environ.get("LOCAL_RANK") or "0")
            ctx = cls._default = cls.get(device)
            return ctx
        ctx = cls._by_device.get(device)
        if ctx is None:
            ctx = cls._by_device[device] = Context(device)
        return ctx

    def name(self) -> str:
        buf = C.create_string_buffer(160)
        _check(self.lib.svgr_device_name(self.handle, buf, 160))
        return buf.value.decode()

    def sync(self):
        _check(self.lib.svgr_sync(self.handle))

    # -- measurement helpers (bench.py) -------------------------------------------------------
    def measure_begin(self, hold_ms: float = 0.0):
        _check(self.lib.svgr_measure_begin(self.handle, float(hold_ms)))

    def measure_end(self) -> float:
        ms = C.c_double()
        _check(self.lib.svgr_measure_end(self.handle, C.byref(ms)))
        return ms.value

    def launches(self) -> int:
        n = C.c_uint64()
        _check(self.lib.svgr_measure_launches(C.byref(n)))
        return int(n.value)

    def set_stream(self, hip_stream: int):
        _check(self.lib.svgr_set_stream(self.handle, _P(hip_stream)))

    # -- buffers -------------------------------------------------------------------------
    def alloc(self, nbytes: int) -> "DeviceBuffer":
        h = _P()
        _check(self.lib.svgr_buf_alloc(self.handle, nbytes, C.byref(h)))
        return DeviceBuffer(self, h, nbytes)

    def wrap(self, device_ptr: int, nbytes: int) -> "DeviceBuffer":
        h = _P()
        _check(self.lib.svgr_buf_wrap(self.handle, _P(device_ptr), nbytes, C.byref(h)))
        return DeviceBuffer(self, h, nbytes)

    def from_host(self, arr: np.ndarray) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        buf = self.alloc(arr.nbytes)
        buf.upload(arr)
        return buf


class DeviceBuffer:
    # (freed by `__del__`, not by a weakref.finalize: a document's render makes and drops 150 of these, and a finalizer object
    #  apiece was 0.3 ms of it.  svgr_buf_free does not touch the context -- the block goes back to the library's pool, which
    #  outlives every context --, so the order of the interpreter's teardown does not matter)
    __slots__ = ("ctx", "handle", "nbytes", "_free", "_parent", "__weakref__")   # (`_parent`: the buffer a view made by `wrap` lives in)

    def __init__(self, ctx: Context, handle, nbytes: int):
        self.ctx, self.handle, self.nbytes = ctx, handle, nbytes
        self._free = ctx.lib.svgr_buf_free

    @property
    def ptr(self) -> int:
        return int(self.ctx.lib.svgr_buf_ptr(self.handle) or 0)

    def zero(self):
        _check(self.ctx.lib.svgr_buf_zero(self.ctx.handle, self.handle))

    def upload(self, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        _check(self.ctx.lib.svgr_upload(self.ctx.handle, self.handle, offset, arr.ctypes.data_as(_P), arr.nbytes))

    def download(self, shape, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        _check(self.ctx.lib.svgr_download(self.ctx.handle, self.handle, offset, out.ctypes.data_as(_P), out.nbytes))
        return out

    def free(self):
        h = self.handle
        if h is not None:
            self.handle = None
            try:
                self._free(None, h)
            except Exception:  # noqa: BLE001  (interpreter teardown)
                pass

    __del__ = free


def _i64x4(v):
    return (C.c_int64 * 4)(*[int(x) for x in v])


def ptr(arr) -> int:
    """Address of a numpy array's data (``arr.ctypes`` builds a helper object on every access: 4 us that add up over a
    scene's hundreds of small arrays)."""
    return arr.__array_interface__["data"][0]


class Batch:
    """svgr_batch: a paint-ordered list of paths resident in HBM."""

    def __init__(self, ctx: Context, segs, seg_kind, path_seg_off, path_m6, path_rule, path_paint,
                 viewport=None, flatness: float = 0.1):
        self.ctx = ctx
        lib = ctx.lib
        segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 8)
        seg_kind = np.ascontiguousarray(seg_kind, dtype=np.uint8).reshape(-1)
        path_seg_off = np.ascontiguousarray(path_seg_off, dtype=np.int64).reshape(-1)
        n_paths = len(path_seg_off) - 1
        path_m6 = np.ascontiguousarray(path_m6, dtype=np.float64).reshape(-1, 6)
        path_rule = np.ascontiguousarray(path_rule, dtype=np.uint8).reshape(-1)
        path_paint = np.ascontiguousarray(path_paint, dtype=np.float64).reshape(-1, 4)
        if len(seg_kind) != len(segs) or len(path_m6) != n_paths or len(path_rule) != n_paths or len(path_paint) != n_paths:
            raise ValueError("inconsistent batch arrays")
        d = BatchDesc()
        d.segs = ptr(segs)
        d.seg_kind = ptr(seg_kind)
        d.n_segs = len(segs)
        d.path_seg_off = ptr(path_seg_off)
        d.n_paths = n_paths
        d.path_m6 = ptr(path_m6)
        d.path_rule = ptr(path_rule)
        d.path_paint = ptr(path_paint)
        d.viewport = _i64x4(viewport if viewport is not None else (0, 0, 0, 0))
        d.flatness = flatness
        h = _P()
        _check(lib.svgr_batch_create(ctx.handle, C.byref(d), C.byref(h)))
        self.handle = h
        self.n_paths = n_paths
        self.n_segs = len(segs)
        self._fin = weakref.finalize(self, lib.svgr_batch_destroy, h)
        self._stats = None

    def destroy(self):
        """Free the batch now.  (Dropping the last reference does the same: callers that hand out lazy views of a batch -- the
        hulls of Path.mask / Scene.render -- simply let go of it.)  A destroyed batch refuses every later call."""
        self._fin()
        self.handle = None

    def plan(self) -> "BatchStats":
        _check(self.ctx.lib.svgr_batch_plan(self.handle))
        st = BatchStats()
        _check(self.ctx.lib.svgr_batch_get_stats(self.handle, C.byref(st)))
        self._stats = st
        return st

    @staticmethod
    def plan_many(batches) -> None:
        """svgr_batch_plan for all of `batches` behind one wait (svgr_batch_plan_many); their `stats` are set."""
        batches = list(batches)
        if not batches:
            return
        arr = (_P * len(batches))(*[b.handle for b in batches])
        _check(batches[0].ctx.lib.svgr_batch_plan_many(arr, len(batches)))
        for b in batches:
            st = BatchStats()
            _check(b.ctx.lib.svgr_batch_get_stats(b.handle, C.byref(st)))
            b._stats = st

    @property
    def stats(self) -> BatchStats:
        if self._stats is None:
            st = BatchStats()
            if self.ctx.lib.svgr_batch_get_stats(self.handle, C.byref(st)) == 0:   # (planned already, e.g. by draw())
                self._stats = st
            else:
                self.plan()
        return self._stats

    def bboxes(self) -> np.ndarray:
        out = np.empty((self.n_paths, 4), dtype=np.int32)
        _check(self.ctx.lib.svgr_batch_get_bboxes(self.handle, out.ctypes.data_as(_P)))
        return out

    def edges(self):
        n = int(self.stats.n_edges)
        edges = np.empty((n, 2, 2), dtype=np.float64)
        edge_path = np.empty(n, dtype=np.int32)
        _check(self.ctx.lib.svgr_batch_get_edges(self.handle, edges.ctypes.data_as(_P), edge_path.ctypes.data_as(_P), n))
        return edges, edge_path

    def all_edges(self):
        """Every flattened edge, also those off the viewport (what the reference builds Path.mask's hull from)."""
        n = C.c_int64()
        _check(self.ctx.lib.svgr_batch_all_edges(self.handle, None, None, 0, C.byref(n)))
        edges = np.empty((n.value, 2, 2), dtype=np.float64)
        edge_path = np.empty(n.value, dtype=np.int32)
        if n.value:
            _check(self.ctx.lib.svgr_batch_all_edges(self.handle, edges.ctypes.data_as(_P), edge_path.ctypes.data_as(_P), n.value, C.byref(n)))
        return edges, edge_path

    def _hit_points(self, points, grid):
        """(points pointer, grid pointer, n, keep-alive) of a hit query: `points` (n, 2) doubles, or grid = (row0, col0, rows, cols)."""
        if (points is None) == (grid is None):
            raise ValueError("give the points or the grid, one of them")
        if grid is not None:
            g = _i64x4(grid)
            if g[2] < 0 or g[3] < 0:
                raise ValueError("a grid has rows >= 0 and cols >= 0")
            return None, g, int(g[2]) * int(g[3]), g
        pts = hit_points(points)
        return ptr(pts), None, len(pts), pts

    def winding(self, points=None, grid=None) -> np.ndarray:
        """svgr_batch_winding: the (n, n_paths) int32 winding numbers of every path at the points (`points`: (n, 2) in the
        edges' coordinate order, or the pixel centres of grid = (row0, col0, rows, cols), row-major)."""
        p, g, n, _keep = self._hit_points(points, grid)
        out = np.zeros((n, self.n_paths), dtype=np.int32)
        _check(self.ctx.lib.svgr_batch_winding(self.handle, p, g, n, ptr(out) if out.size else None))
        return out

    def pick(self, points=None, grid=None, pickable=None, clips=None, scratch_bytes: int = 0, want_bits: bool = False):
        """svgr_batch_pick: (top (n,) int32, pass bits (n, ceil(n_paths / 32)) uint32 or None).  `clips`: per path a sequence of
        clip groups, each a sequence of earlier path indices (None: no clips)."""
        p, g, n, _keep = self._hit_points(points, grid)
        npaths = self.n_paths
        pk = np.ones(npaths, dtype=np.uint8) if pickable is None else np.ascontiguousarray(pickable, dtype=np.uint8).reshape(-1)
        if len(pk) != npaths:
            raise ValueError("one pickable flag per path")
        clip_off, clip_group, group_off, group_src = clip_tables(clips, npaths)
        top = np.full(n, -1, dtype=np.int32)
        bits = np.zeros((n, (npaths + 31) // 32), dtype=np.uint32) if want_bits else None
        _check(self.ctx.lib.svgr_batch_pick(self.handle, p, g, n, ptr(pk) if npaths else None, ptr(clip_off), ptr(clip_group) if len(clip_group) else None,
                                            ptr(group_off), ptr(group_src) if len(group_src) else None, len(group_off) - 1, int(scratch_bytes),
                                            ptr(top) if n else None, ptr(bits) if want_bits and bits.size else None))
        return top, bits

    def distance(self, points=None, grid=None, spread: float = math.inf, out: str = "f64", union: bool = False, signed: bool = True,
                 scratch_bytes: int = 0) -> np.ndarray:
        """svgr_batch_distance: the distance of every point to every path's outline, negative inside (`signed`), clamped to
        +-`spread`: (n, n_paths), or (n,) with `union` (the minimum over the paths).  `out`: "f64" the clamped distance, "f32" /
        "u8" the value 0.5 - d / (2 * spread) as float32 / rounded to uint8 (a finite spread).  Points as for `winding`."""
        if out not in SDF_OUT:
            raise ValueError(f"out is one of {sorted(SDF_OUT)}, not {out!r}")
        enc, dtype = SDF_OUT[out]
        spread = sdf_spread(spread, finite=enc != SDF_F64)
        p, g, n, _keep = self._hit_points(points, grid)
        res = np.zeros(n if union else (n, self.n_paths), dtype=dtype)
        flags = enc | (SDF_UNION if union else 0) | (0 if signed else SDF_UNSIGNED)
        _check(self.ctx.lib.svgr_batch_distance(self.handle, p, g, n, spread, flags, int(scratch_bytes), ptr(res) if res.size else None))
        return res

    def msdf(self, colour, group_off, orient, points=None, grid=None, spread: float = math.inf, out: str = "f64", scratch_bytes: int = 0) -> np.ndarray:
        """svgr_batch_msdf: (n, 4) R, G, B, A at every point -- A the signed distance of `distance`, R / G / B the pseudo-distance to
        the nearest edge of that colour -- over groups of paths: `colour` (n_paths,) masks 1 .. 7, group g the paths
        group_off[g] .. group_off[g + 1], `orient` (n_groups,) +1 / -1; every channel the minimum over the groups.  `out` and the
        points as for `distance`."""
        if out not in SDF_OUT:
            raise ValueError(f"out is one of {sorted(SDF_OUT)}, not {out!r}")
        enc, dtype = SDF_OUT[out]
        spread = sdf_spread(spread, finite=enc != SDF_F64)
        colour = np.ascontiguousarray(colour, dtype=np.uint8).reshape(-1)
        group_off = np.ascontiguousarray(group_off, dtype=np.int32).reshape(-1)
        orient = np.ascontiguousarray(orient, dtype=np.int8).reshape(-1)
        if len(colour) != self.n_paths or len(group_off) != len(orient) + 1:
            raise ValueError("one colour per path, one orient per group and one more group_off than groups")
        p, g, n, _keep = self._hit_points(points, grid)
        res = np.zeros((n, 4), dtype=dtype)
        _check(self.ctx.lib.svgr_batch_msdf(self.handle, p, g, n, spread, enc, ptr(colour), ptr(group_off), ptr(orient) if len(orient) else None,
                                            len(orient), int(scratch_bytes), ptr(res) if res.size else None))
        return res

    def set_bands(self, rank: int, world: int, strip_bands: int = 1):
        """Shard by interleaved strips of `strip_bands` bands; call plan() again afterwards."""
        _check(self.ctx.lib.svgr_batch_set_bands(self.handle, rank, world, strip_bands))
        self._stats = None

    def set_groups(self, path_group, group_clip_src, group_opacity):
        """Isolated groups (CLIP / OPACITY over a GROUP of solid fills): see svgr_batch_set_groups; call before plan()."""
        pg = np.ascontiguousarray(path_group, dtype=np.int32).reshape(self.n_paths)
        cs = np.ascontiguousarray(group_clip_src, dtype=np.int32).reshape(-1)
        op = np.ascontiguousarray(group_opacity, dtype=np.float64).reshape(-1)
        if len(cs) != len(op):
            raise ValueError("one clip source and one opacity per group")
        _check(self.ctx.lib.svgr_batch_set_groups(self.handle, C.c_void_p(ptr(pg)), len(cs), C.c_void_p(ptr(cs)), C.c_void_p(ptr(op))))
        self._stats = None

    def extents(self) -> np.ndarray:
        """(n_paths, 4) doubles {min row, min col, max row, max col} of every path's flattened points, unclipped
        (svgr_batch_get_extents: between plan() and the first render)."""
        out = np.empty((self.n_paths, 4), dtype=np.float64)
        _check(self.ctx.lib.svgr_batch_get_extents(self.handle, C.c_void_p(ptr(out))))
        return out

    def set_gradients(self, path_grad, grads):
        """Gradient paints inside the batch: path_grad[p] = index into `grads` (a list of `Gradient` structs, one per
        gradient-filled path) or -1; see svgr_batch_set_gradients.  Call before plan()."""
        pg = np.ascontiguousarray(path_grad, dtype=np.int32).reshape(self.n_paths)
        arr = (Gradient * max(len(grads), 1))(*grads)
        _check(self.ctx.lib.svgr_batch_set_gradients(self.handle, C.c_void_p(ptr(pg)), len(grads), C.cast(arr, _P)))
        self._stats = None

    def set_paints(self, paints):
        paints = np.ascontiguousarray(paints, dtype=np.float64).reshape(self.n_paths, 4)
        _check(self.ctx.lib.svgr_batch_set_paints(self.handle, paints.ctypes.data_as(_P)))

    def set_transforms(self, path_m6):
        """New transforms for the same geometry (svgr_batch_set_transforms): the plan is void until plan() runs again."""
        m6 = np.ascontiguousarray(path_m6, dtype=np.float64).reshape(self.n_paths, 6)
        _check(self.ctx.lib.svgr_batch_set_transforms(self.handle, m6.ctypes.data_as(_P)))
        self._stats = None

    def owned_rows(self) -> int:
        return int(self.ctx.lib.svgr_batch_owned_rows(self.handle))

    def render(self, out: DeviceBuffer, kind: int, flags: int = 0, window=None):
        """`window` (row0, col0, rows, cols): only that part of the canvas, into a buffer of its size (svgr_batch_render_window)."""
        if window is None:
            _check(self.ctx.lib.svgr_batch_render(self.handle, out.handle, kind, flags))
        else:
            w = (C.c_int32 * 4)(*[int(v) for v in window])
            _check(self.ctx.lib.svgr_batch_render_window(self.handle, out.handle, kind, flags, w))

    def draw(self, out: DeviceBuffer, kind: int, flags: int = 0):
        """svgr_batch_draw: plan (if the batch has no valid plan) and render behind ONE wait -- a frame with new geometry, the
        reference's only mode (S:948-957).  The picture is in `out` and the stream has drained when the call returns."""
        _check(self.ctx.lib.svgr_batch_draw(self.handle, out.handle, kind, flags))
        self._stats = None   # (whatever plan() returned before describes other geometry: `stats` asks again)

    def render_windows(self, outs, kind: int, windows, flags: int = 0):
        """svgr_batch_render_windows: `windows[i]` (row0, col0, rows, cols) into `outs[i]`, all from one geometry pass, side by side."""
        n = len(outs)
        if n == 0:
            return
        arr = (_P * n)(*[o.handle for o in outs])
        w = (C.c_int32 * (4 * n))(*[int(v) for win in windows for v in win])
        _check(self.ctx.lib.svgr_batch_render_windows(self.handle, n, arr, kind, flags, w))

    def render_masks(self):
        """SVGR_OUT_MASKS_F64: Path.mask of every path of the batch in one launch.  Returns (buffer, offsets, bboxes):
        path p's (rows_p, cols_p) doubles start `offsets[p]` doubles into `buffer`."""
        bb = self.bboxes()
        area = np.where((bb[:, 2] > 0) & (bb[:, 3] > 0), bb[:, 2].astype(np.int64) * bb[:, 3], 0)
        offs = np.concatenate([[0], np.cumsum(area)]).astype(np.int64)
        buf = self.ctx.alloc(max(int(offs[-1]) * 8, 8))
        self.render(buf, OUT_MASKS_F64)
        return buf, offs, bb

    def render_fills(self):
        """SVGR_OUT_FILLS_F64: Path.fill of every path of the batch (its own solid paint) in one launch.  Returns (buffer,
        offsets, bboxes): path p's (rows_p, cols_p, 4) doubles start `4 * offsets[p]` doubles into `buffer`."""
        bb = self.bboxes()
        area = np.where((bb[:, 2] > 0) & (bb[:, 3] > 0), bb[:, 2].astype(np.int64) * bb[:, 3], 0)
        offs = np.concatenate([[0], np.cumsum(area)]).astype(np.int64)
        buf = self.ctx.alloc(max(int(offs[-1]) * 32, 32))
        self.render(buf, OUT_FILLS_F64)
        return buf, offs, bb

    def timings(self):
        n = C.c_int()
        tot, geo, tile = C.c_double(), C.c_double(), C.c_double()
        _check(self.ctx.lib.svgr_batch_timings(self.handle, C.byref(n), C.byref(tot), C.byref(geo), C.byref(tile)))
        return dict(n=n.value, ms_total=tot.value, ms_geometry=geo.value, ms_tile=tile.value)


def hash_buffers(ptrs: np.ndarray, sizes: np.ndarray) -> int:
    """svgr_hash_buffers (host only): 64-bit hash over the bytes of the buffers (ptrs uint64, sizes int64)."""
    lib = load_library()
    out = C.c_uint64()
    n = len(ptrs)
    _check(lib.svgr_hash_buffers(ptrs.ctypes.data_as(_P), sizes.ctypes.data_as(_P), n, C.byref(out)))
    return int(out.value)


def path_stroke(seg_types, seg_params, subpath_sizes, width: float, linecap: int, linejoin: int):
    """svgr_path_stroke (host C++, no GPU involved): (types, params (n, 8), sizes) of the stroke outline."""
    lib = load_library()
    seg_types = np.ascontiguousarray(seg_types, dtype=np.int32)
    seg_params = np.ascontiguousarray(seg_params, dtype=np.float64).reshape(-1, 8)
    subpath_sizes = np.ascontiguousarray(subpath_sizes, dtype=np.int32)
    if int(subpath_sizes.sum()) != len(seg_types) or len(seg_params) != len(seg_types):
        raise ValueError("segment arrays do not match the subpath sizes")
    out = _P()
    rc = lib.svgr_path_stroke(seg_types.ctypes.data_as(_P), seg_params.ctypes.data_as(_P), subpath_sizes.ctypes.data_as(_P),
                              len(subpath_sizes), float(width), int(linecap), int(linejoin), C.byref(out))
    if rc != 0:
        why = {-1: "unsupported segment type or bad cap / join", -3: "out of memory"}.get(
            rc, "the offset of a cubic does not converge (degenerate control points)")
        raise ValueError(f"svgr_path_stroke failed ({rc}): {why}")
    return _stroke_out(lib, out)


def _stroke_out(lib, out):
    """The arrays of a svgr_stroke_out, which is freed."""
    try:
        n, ns = C.c_int64(), C.c_int64()
        lib.svgr_stroke_out_counts(out, C.byref(n), C.byref(ns))
        types = np.empty(n.value, dtype=np.int32)
        params = np.empty((n.value, 8), dtype=np.float64)
        sizes = np.empty(ns.value, dtype=np.int32)
        lib.svgr_stroke_out_copy(out, types.ctypes.data_as(_P), params.ctypes.data_as(_P), sizes.ctypes.data_as(_P))
    finally:
        lib.svgr_stroke_out_free(out)
    return types, params, sizes


def dash_is_solid(dashes) -> bool:
    """Whether a dash list asks for a solid stroke (svgr_path_dash hands the path back unchanged, without touching a device):
    empty, a negative or non-finite entry, a zero sum, or no gap of non-zero length."""
    d = [float(v) for v in dashes] if dashes is not None else []
    if not d or any(not np.isfinite(v) or v < 0 for v in d) or not sum(d) > 0 or not np.isfinite(sum(d)):
        return True
    return not any(v > 0 for v in (d * 2 if len(d) & 1 else d)[1::2])


def path_dash(seg_types, seg_params, subpath_sizes, dashes, offset: float = 0.0, path_length: float = 0.0, ctx: "Context | None" = None):
    """svgr_path_dash: (types, params (n, 8), sizes) of the path cut into its dashes, on the device of `ctx` (default: the
    process's context; none is made for a dash list that asks for a solid stroke)."""
    lib = load_library()
    seg_types = np.ascontiguousarray(seg_types, dtype=np.int32)
    seg_params = np.ascontiguousarray(seg_params, dtype=np.float64).reshape(-1, 8)
    subpath_sizes = np.ascontiguousarray(subpath_sizes, dtype=np.int32)
    dashes = np.ascontiguousarray(dashes if dashes is not None else [], dtype=np.float64).reshape(-1)
    if int(subpath_sizes.sum()) != len(seg_types) or len(seg_params) != len(seg_types):
        raise ValueError("segment arrays do not match the subpath sizes")
    handle = None
    if not dash_is_solid(dashes) and len(seg_types):
        handle = (ctx if ctx is not None else Context.get()).handle
    out = _P()
    _check(lib.svgr_path_dash(handle, seg_types.ctypes.data_as(_P), seg_params.ctypes.data_as(_P), subpath_sizes.ctypes.data_as(_P),
                              len(subpath_sizes), dashes.ctypes.data_as(_P), len(dashes), float(offset),
                              float(path_length or 0.0), C.byref(out)))
    return _stroke_out(lib, out)


def dash_scan_segments() -> int:
    """Segments per workgroup of the dasher's scans (svgr_dash_scan_segments)."""
    return int(load_library().svgr_dash_scan_segments())


def path_markers(seg_types, seg_params, subpath_sizes, seg_vertex=None, ctx: "Context | None" = None):
    """svgr_path_markers: (xy (n, 2), direction (n, 2), kind (n,) int32) of the path's vertices, on the device of `ctx` (default:
    the process's context; none is made for a path without segments).  `seg_vertex`: non-zero where a segment ends at a vertex
    of the author's path (None: every segment does)."""
    lib = load_library()
    seg_types = np.ascontiguousarray(seg_types, dtype=np.int32)
    seg_params = np.ascontiguousarray(seg_params, dtype=np.float64).reshape(-1, 8)
    subpath_sizes = np.ascontiguousarray(subpath_sizes, dtype=np.int32)
    if int(subpath_sizes.sum()) != len(seg_types) or len(seg_params) != len(seg_types):
        raise ValueError("segment arrays do not match the subpath sizes")
    vertex = None
    if seg_vertex is not None:
        vertex = np.ascontiguousarray(seg_vertex, dtype=np.int32).reshape(-1)
        if len(vertex) != len(seg_types):
            raise ValueError("the vertex flags do not match the segments")
    handle = (ctx if ctx is not None else Context.get()).handle if len(seg_types) else None
    out = _P()
    _check(lib.svgr_path_markers(handle, seg_types.ctypes.data_as(_P), seg_params.ctypes.data_as(_P),
                                 None if vertex is None else vertex.ctypes.data_as(_P), subpath_sizes.ctypes.data_as(_P),
                                 len(subpath_sizes), C.byref(out)))
    try:
        n = C.c_int64()
        lib.svgr_marker_out_counts(out, C.byref(n))
        xyuv = np.zeros((n.value, 4), dtype=np.float64)
        kind = np.zeros(n.value, dtype=np.int32)
        lib.svgr_marker_out_copy(out, xyuv.ctypes.data_as(_P), kind.ctypes.data_as(_P))
    finally:
        lib.svgr_marker_out_free(out)
    return np.ascontiguousarray(xyuv[:, :2]), np.ascontiguousarray(xyuv[:, 2:]), kind


def marker_block_segments() -> int:
    """Segments per workgroup of the marker pass's own kernels (svgr_marker_block_segments)."""
    return int(load_library().svgr_marker_block_segments())


def _path_arrays(seg_types, seg_params, subpath_sizes):
    seg_types = np.ascontiguousarray(seg_types, dtype=np.int32)
    seg_params = np.ascontiguousarray(seg_params, dtype=np.float64).reshape(-1, 8)
    subpath_sizes = np.ascontiguousarray(subpath_sizes, dtype=np.int32)
    if int(subpath_sizes.sum()) != len(seg_types) or len(seg_params) != len(seg_types):
        raise ValueError("segment arrays do not match the subpath sizes")
    return seg_types, seg_params, subpath_sizes


def hit_points(points) -> np.ndarray:
    """The points of a hit query as a contiguous (n, 2) float64 array: (n, 2), or a single pair.  Anything else is a ValueError
    (before any device work)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1 and pts.shape == (2,):
        pts = pts.reshape(1, 2)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"points are (n, 2) or a single pair, not {pts.shape}")
    return np.ascontiguousarray(pts)


# svgr_batch_distance's flags (include/svgr.h)
SDF_F64, SDF_F32, SDF_U8, SDF_UNION, SDF_UNSIGNED = 0, 1, 2, 4, 8
SDF_OUT = {"f64": (SDF_F64, np.float64), "f32": (SDF_F32, np.float32), "u8": (SDF_U8, np.uint8)}


def sdf_spread(spread, finite: bool = False) -> float:
    """A spread as a float: +inf or finite and > 0, `finite` asking for the latter.  Anything else is a ValueError (before any
    device work)."""
    try:
        s = float(spread)
    except (TypeError, ValueError):
        raise ValueError(f"a spread is a number, not {spread!r}") from None
    if not s > 0.0:
        raise ValueError(f"a spread is +inf or a finite value > 0, not {spread!r}")
    if finite and math.isinf(s):
        raise ValueError("the float32 and uint8 encodings need a finite spread")
    return s


def sdf_encode(d, spread: float, out: str) -> np.ndarray:
    """Clamped distances in svgr_batch_distance's encoding `out` (csrc/svgr_sdf.h), on the host: for the constant fields of
    queries that never reach a device (an empty path, an empty atlas)."""
    d = np.asarray(d, dtype=np.float64)
    if out == "f64":
        return d
    v = 0.5 - d / (2.0 * spread)
    if out == "f32":
        return v.astype(np.float32)
    return np.clip(np.rint(v * 255.0), 0.0, 255.0).astype(np.uint8)


def clip_tables(clips, n_paths):
    """The four int32 tables of svgr_batch_pick from `clips`: per path a sequence of clip groups, each a sequence of path indices
    (None: no path is clipped).  Equal groups are stored once.  Returns (clip_off, clip_group, group_off, group_src)."""
    clip_off, clip_group, group_off, group_src, seen = [0], [], [0], [], {}
    for p in range(n_paths):
        for grp in (clips[p] if clips is not None else ()):
            key = tuple(int(s) for s in grp)
            g = seen.get(key)
            if g is None:
                g = seen[key] = len(group_off) - 1
                group_src.extend(key)
                group_off.append(len(group_src))
            clip_group.append(g)
        clip_off.append(len(clip_group))
    return tuple(np.asarray(a, dtype=np.int32) for a in (clip_off, clip_group, group_off, group_src))


def path_sample(seg_types, seg_params, subpath_sizes, s=(), ctx: "Context | None" = None):
    """svgr_path_sample: (xy (n, 2), direction (n, 2), inside (n,) bool, total length) of the path at the arc lengths `s`, on the
    device of `ctx` (default: the process's context; none is made for a path without segments)."""
    lib = load_library()
    seg_types, seg_params, subpath_sizes = _path_arrays(seg_types, seg_params, subpath_sizes)
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    handle = (ctx if ctx is not None else Context.get()).handle if len(seg_types) else None
    xyuv = np.zeros((len(s), 4), dtype=np.float64)
    inside = np.zeros(len(s), dtype=np.int32)
    total = C.c_double()
    _check(lib.svgr_path_sample(handle, seg_types.ctypes.data_as(_P), seg_params.ctypes.data_as(_P), subpath_sizes.ctypes.data_as(_P),
                                len(subpath_sizes), s.ctypes.data_as(_P), len(s), xyuv.ctypes.data_as(_P), inside.ctypes.data_as(_P),
                                C.byref(total)))
    return np.ascontiguousarray(xyuv[:, :2]), np.ascontiguousarray(xyuv[:, 2:]), inside != 0, total.value


def path_place_glyphs(seg_types, seg_params, subpath_sizes, atlas_types, atlas_params, glyph_seg_off, inst_glyph, inst_s_mid, inst_half,
                      inst_dy, ctx: "Context | None" = None):
    """svgr_path_place_glyphs: (params (n_out, 8), visible (n_inst,) bool, total length): the atlas segments of every instance's
    glyph, in instance order, placed on the path; the rows of a hidden instance are 0.  Instance k owns the rows
    [off[k], off[k + 1]), off = the prefix sums of ``diff(glyph_seg_off)[inst_glyph]``."""
    lib = load_library()
    seg_types, seg_params, subpath_sizes = _path_arrays(seg_types, seg_params, subpath_sizes)
    atlas_types = np.ascontiguousarray(atlas_types, dtype=np.int32)
    atlas_params = np.ascontiguousarray(atlas_params, dtype=np.float64).reshape(-1, 8)
    glyph_seg_off = np.ascontiguousarray(glyph_seg_off, dtype=np.int32)
    inst_glyph = np.ascontiguousarray(inst_glyph, dtype=np.int32).reshape(-1)
    inst = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (inst_s_mid, inst_half, inst_dy)]
    n_inst = len(inst_glyph)
    if len(glyph_seg_off) < 1 or len(atlas_types) != len(atlas_params) or any(len(a) != n_inst for a in inst):
        raise ValueError("the glyph arrays do not match")
    if len(atlas_types) != int(glyph_seg_off[-1]):
        raise ValueError("the atlas does not match the glyph offsets")
    n_glyphs = len(glyph_seg_off) - 1
    counts = np.diff(glyph_seg_off.astype(np.int64))
    ok = (inst_glyph >= 0) & (inst_glyph < n_glyphs)
    n_out = int(counts[inst_glyph[ok]].clip(min=0).sum()) if n_glyphs else 0   # (the library refuses what is not `ok`)
    handle = (ctx if ctx is not None else Context.get()).handle if len(seg_types) else None
    params = np.zeros((n_out, 8), dtype=np.float64)
    visible = np.zeros(n_inst, dtype=np.int32)
    total = C.c_double()
    _check(lib.svgr_path_place_glyphs(handle, seg_types.ctypes.data_as(_P), seg_params.ctypes.data_as(_P), subpath_sizes.ctypes.data_as(_P),
                                      len(subpath_sizes), atlas_types.ctypes.data_as(_P), atlas_params.ctypes.data_as(_P),
                                      glyph_seg_off.ctypes.data_as(_P), n_glyphs, inst_glyph.ctypes.data_as(_P), inst[0].ctypes.data_as(_P),
                                      inst[1].ctypes.data_as(_P), inst[2].ctypes.data_as(_P), n_inst, params.ctypes.data_as(_P),
                                      visible.ctypes.data_as(_P), C.byref(total)))
    return params, visible != 0, total.value


def textpath_block() -> int:
    """Queries / output segments per workgroup of the text-on-a-path kernels (svgr_textpath_block)."""
    return int(load_library().svgr_textpath_block())


def glyf_outline(pt_xy, pt_on, contour_off, glyph_contour_off, part_glyph, part_m, part_pen, part_sx, part_sy,
                 ctx: "Context | None" = None):
    """svgr_glyf_outline: (types, params (n, 8), sizes) of the TrueType outlines of the parts.  The atlas holds every distinct
    simple glyph once: `pt_xy` (n_points, 2) int16, `pt_on` uint8, `contour_off` (n_contours + 1, in points), `glyph_contour_off`
    (n_glyphs + 1, in contours); part k shows glyph ``part_glyph[k]`` under ``part_m[k]`` = (m00, m01, m10, m11, dx, dy), then
    ``X = (x' + pen) * sx``, ``Y = y' * sy``.  On the device of `ctx` (default: the process's context; none is made when no part
    has a point)."""
    lib = load_library()
    args, _n_glyphs, lanes = _glyf_args(pt_xy, pt_on, contour_off, glyph_contour_off, part_glyph, part_m, part_pen, part_sx, part_sy)
    handle = (ctx if ctx is not None else Context.get()).handle if lanes else None
    out = _P()
    _check(lib.svgr_glyf_outline(handle, *args, C.byref(out)))
    return _stroke_out(lib, out)


def _glyf_args(pt_xy, pt_on, contour_off, glyph_contour_off, part_glyph, part_m, part_pen, part_sx, part_sy):
    """(the atlas and part arguments of svgr_glyf_outline behind its context, the glyph count, the lanes the call has)."""
    pt_xy = np.ascontiguousarray(pt_xy, dtype=np.int16).reshape(-1, 2)
    pt_on = np.ascontiguousarray(pt_on, dtype=np.uint8).reshape(-1)
    contour_off = np.ascontiguousarray(contour_off, dtype=np.int32).reshape(-1)
    glyph_contour_off = np.ascontiguousarray(glyph_contour_off, dtype=np.int32).reshape(-1)
    part_glyph = np.ascontiguousarray(part_glyph, dtype=np.int32).reshape(-1)
    part_m = np.ascontiguousarray(part_m, dtype=np.float64).reshape(-1, 6)
    part = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (part_pen, part_sx, part_sy)]
    n_parts = len(part_glyph)
    if len(contour_off) < 1 or len(glyph_contour_off) < 1 or len(pt_on) != len(pt_xy):
        raise ValueError("the atlas arrays do not match")
    if len(part_m) != n_parts or any(len(a) != n_parts for a in part):
        raise ValueError("the part arrays do not match")
    # (what the library cannot see: that the tables are as long as the counts say; what they hold it checks itself)
    n_glyphs, n_contours = len(glyph_contour_off) - 1, len(contour_off) - 1
    lanes = 0   # (tables the library is going to refuse count as none: it refuses them before it asks for a context)
    if (n_parts and n_glyphs and int(part_glyph.min()) >= 0 and int(part_glyph.max()) < n_glyphs
            and int(glyph_contour_off.min()) >= 0 and int(glyph_contour_off.max()) <= n_contours):
        first = contour_off.astype(np.int64)[glyph_contour_off]
        lanes = int((first[part_glyph + 1] - first[part_glyph]).clip(min=0).sum())
    args = (pt_xy.ctypes.data_as(_P), pt_on.ctypes.data_as(_P), len(pt_xy), contour_off.ctypes.data_as(_P), n_contours,
            glyph_contour_off.ctypes.data_as(_P), n_glyphs, part_glyph.ctypes.data_as(_P), part_m.ctypes.data_as(_P),
            part[0].ctypes.data_as(_P), part[1].ctypes.data_as(_P), part[2].ctypes.data_as(_P), n_parts)   # (a pointer keeps its array alive)
    return args, n_glyphs, lanes


def glyf_block() -> int:
    """(part, point) pairs per workgroup of the TrueType outline kernel (svgr_glyf_block)."""
    return int(load_library().svgr_glyf_block())


def _tuple_arrays(n_glyphs, glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy):
    """The tuple arrays of the two variable-font entries in the library's types; what the library cannot see -- that the tables
    are as long as the counts say -- is checked here, what they hold it checks itself."""
    glyph_tuple_off = np.ascontiguousarray(glyph_tuple_off, dtype=np.int32).reshape(-1)
    tuple_scalar = np.ascontiguousarray(tuple_scalar, dtype=np.float64).reshape(-1)
    tuple_pt_off = np.ascontiguousarray(tuple_pt_off, dtype=np.int32).reshape(-1)
    tp_index = np.ascontiguousarray(tp_index, dtype=np.int32).reshape(-1)
    tp_dxy = np.ascontiguousarray(tp_dxy, dtype=np.int16).reshape(-1, 2)
    if len(glyph_tuple_off) != n_glyphs + 1 or len(tuple_pt_off) != len(tuple_scalar) + 1 or len(tp_dxy) != len(tp_index):
        raise ValueError("the tuple arrays do not match")
    return glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy


def gvar_deltas(pt_xy, contour_off, glyph_contour_off, glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy,
                ctx: "Context | None" = None):
    """svgr_gvar_deltas: (n_points, 2) float64, the delta of every atlas point at one instance of a variable font.  The atlas is
    `glyf_outline`'s; glyph g owns the tuples ``[glyph_tuple_off[g], glyph_tuple_off[g + 1])``, tuple t the scalar
    ``tuple_scalar[t]`` and the entries ``[tuple_pt_off[t], tuple_pt_off[t + 1])`` of `tp_index` (glyph-local, strictly increasing)
    and `tp_dxy` (n, 2) int16.  On the device of `ctx` (default: the process's context; none is made without points or tuples)."""
    lib = load_library()
    pt_xy = np.ascontiguousarray(pt_xy, dtype=np.int16).reshape(-1, 2)
    contour_off = np.ascontiguousarray(contour_off, dtype=np.int32).reshape(-1)
    glyph_contour_off = np.ascontiguousarray(glyph_contour_off, dtype=np.int32).reshape(-1)
    if len(contour_off) < 1 or len(glyph_contour_off) < 1:
        raise ValueError("the atlas arrays do not match")
    n_glyphs, n_contours = len(glyph_contour_off) - 1, len(contour_off) - 1
    tuples = _tuple_arrays(n_glyphs, glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy)
    handle = (ctx if ctx is not None else Context.get()).handle if len(pt_xy) and len(tuples[1]) else None
    out = np.zeros((len(pt_xy), 2), dtype=np.float64)
    _check(lib.svgr_gvar_deltas(handle, pt_xy.ctypes.data_as(_P), len(pt_xy), contour_off.ctypes.data_as(_P), n_contours,
                                glyph_contour_off.ctypes.data_as(_P), n_glyphs, tuples[0].ctypes.data_as(_P), tuples[1].ctypes.data_as(_P),
                                len(tuples[1]), tuples[2].ctypes.data_as(_P), tuples[3].ctypes.data_as(_P), tuples[4].ctypes.data_as(_P),
                                len(tuples[3]), out.ctypes.data_as(_P)))
    return out


def glyf_outline_var(pt_xy, pt_on, contour_off, glyph_contour_off, part_glyph, part_m, part_pen, part_sx, part_sy,
                     glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy, ctx: "Context | None" = None):
    """svgr_glyf_outline_var: `glyf_outline` of the points varied by `gvar_deltas`' tuples -- the delta pass and the outline pass
    in one call; the deltas stay on the device."""
    lib = load_library()
    args, n_glyphs, lanes = _glyf_args(pt_xy, pt_on, contour_off, glyph_contour_off, part_glyph, part_m, part_pen, part_sx, part_sy)
    tuples = _tuple_arrays(n_glyphs, glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy)
    handle = (ctx if ctx is not None else Context.get()).handle if lanes else None
    out = _P()
    _check(lib.svgr_glyf_outline_var(handle, *args, tuples[0].ctypes.data_as(_P), tuples[1].ctypes.data_as(_P), len(tuples[1]),
                                     tuples[2].ctypes.data_as(_P), tuples[3].ctypes.data_as(_P), tuples[4].ctypes.data_as(_P),
                                     len(tuples[3]), C.byref(out)))
    return _stroke_out(lib, out)


def gvar_block() -> int:
    """Atlas points per workgroup of the variable-font delta kernel (svgr_gvar_block)."""
    return int(load_library().svgr_gvar_block())


def cff_outline(pt_xy, pt_kind, contour_off, glyph_contour_off, part_glyph, part_m, part_pen, part_sx, part_sy,
                ctx: "Context | None" = None):
    """svgr_cff_outline: (types, params (n, 8), sizes) of the CFF outlines of the parts.  The atlas holds every distinct glyph
    once: `pt_xy` (n_points, 2) float64 in font units, `pt_kind` uint8 (0 MOVE, 1 LINE, 2 C1, 3 C2, 4 CURVE), `contour_off`
    (n_contours + 1, in points), `glyph_contour_off` (n_glyphs + 1, in contours); the parts are `glyf_outline`'s.  On the device of
    `ctx` (default: the process's context; none is made when nothing can be drawn)."""
    lib = load_library()
    pt_xy = np.ascontiguousarray(pt_xy, dtype=np.float64).reshape(-1, 2)
    pt_kind = np.ascontiguousarray(pt_kind, dtype=np.uint8).reshape(-1)
    contour_off = np.ascontiguousarray(contour_off, dtype=np.int32).reshape(-1)
    glyph_contour_off = np.ascontiguousarray(glyph_contour_off, dtype=np.int32).reshape(-1)
    part_glyph = np.ascontiguousarray(part_glyph, dtype=np.int32).reshape(-1)
    part_m = np.ascontiguousarray(part_m, dtype=np.float64).reshape(-1, 6)
    part = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (part_pen, part_sx, part_sy)]
    n_parts = len(part_glyph)
    if len(contour_off) < 1 or len(glyph_contour_off) < 1 or len(pt_kind) != len(pt_xy):
        raise ValueError("the atlas arrays do not match")
    if len(part_m) != n_parts or any(len(a) != n_parts for a in part):
        raise ValueError("the part arrays do not match")
    # (what the library cannot see: that the tables are as long as the counts say; what they hold it checks itself)
    n_glyphs, n_contours = len(glyph_contour_off) - 1, len(contour_off) - 1
    points = 0   # (tables the library is going to refuse count as none: it refuses them before it asks for a context)
    if (n_parts and n_glyphs and int(part_glyph.min()) >= 0 and int(part_glyph.max()) < n_glyphs
            and int(glyph_contour_off.min()) >= 0 and int(glyph_contour_off.max()) <= n_contours):
        first = contour_off.astype(np.int64)[glyph_contour_off]
        points = int((first[part_glyph + 1] - first[part_glyph]).clip(min=0).sum())
    draws = points and bool(((pt_kind == 1) | (pt_kind == 4)).any())   # (lone MOVEs draw nothing: no launch, no context)
    handle = (ctx if ctx is not None else Context.get()).handle if draws else None
    out = _P()
    _check(lib.svgr_cff_outline(handle, pt_xy.ctypes.data_as(_P), pt_kind.ctypes.data_as(_P), len(pt_xy), contour_off.ctypes.data_as(_P),
                                n_contours, glyph_contour_off.ctypes.data_as(_P), n_glyphs, part_glyph.ctypes.data_as(_P),
                                part_m.ctypes.data_as(_P), part[0].ctypes.data_as(_P), part[1].ctypes.data_as(_P),
                                part[2].ctypes.data_as(_P), n_parts, C.byref(out)))
    return _stroke_out(lib, out)


def cff_block() -> int:
    """Output segments per workgroup of the CFF outline kernel (svgr_cff_block)."""
    return int(load_library().svgr_cff_block())


def image_levels(h: int, w: int):
    """[(offset, rows, cols)] in texels of every mip level of an (h, w) image, level 0 first, down to 1 x 1 (the layout
    svgr_image_upload writes): a function of the size alone."""
    out, off = [], 0
    while True:
        out.append((off, h, w))
        off += h * w
        if h == 1 and w == 1:
            return out
        h, w = (h + 1) // 2, (w + 1) // 2


def image_upload(ctx: Context, pixels: np.ndarray, linear_rgb: bool) -> DeviceBuffer:
    """svgr_image_upload: an (h, w, 4) uint8 straight-alpha sRGB image -> a device buffer holding its premultiplied float32x4
    mip chain (levels as `image_levels` lays them out)."""
    px = np.ascontiguousarray(pixels, dtype=np.uint8)
    if px.ndim != 3 or px.shape[2] != 4:
        raise ValueError("an image is an (h, w, 4) uint8 array")
    h, w = px.shape[:2]
    off, lh, lw = image_levels(h, w)[-1]
    buf = ctx.alloc((off + lh * lw) * 16)
    _check(ctx.lib.svgr_image_upload(ctx.handle, ptr(px), h, w, int(bool(linear_rgb)), buf.handle))
    return buf


def png_unfilter(data, rows: int, row_bytes: int, bytes_per_pixel: int) -> np.ndarray:
    """svgr_png_unfilter (host only): `rows` filtered PNG scanlines of 1 + row_bytes bytes -> (rows, row_bytes) uint8.
    ValueError on a filter type above 4 or a short input."""
    src = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    dst = np.empty((rows, row_bytes), dtype=np.uint8)
    rc = load_library().svgr_png_unfilter(src.ctypes.data_as(_P), src.size, rows, row_bytes, bytes_per_pixel, dst.ctypes.data_as(_P))
    if rc != 0:
        raise ValueError("PNG scanlines: unknown filter type or truncated data")
    return dst


def jpeg_entropy(scan: JpegScan, huff_counts: np.ndarray, huff_symbols: np.ndarray, data, coef: np.ndarray) -> None:
    """svgr_jpeg_entropy (host only): one scan's entropy-coded segment decoded into `coef`, the frame's int16 coefficients
    (include/svgr.h has the layout), in place.  ValueError with the reason when the data does not decode."""
    src = np.frombuffer(data, dtype=np.uint8)
    assert huff_counts.dtype == np.uint8 and huff_counts.shape == (8, 16) and huff_counts.flags.c_contiguous
    assert huff_symbols.dtype == np.uint8 and huff_symbols.shape == (8, 256) and huff_symbols.flags.c_contiguous
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and coef.flags.writeable
    rc = load_library().svgr_jpeg_entropy(C.byref(scan), ptr(huff_counts), ptr(huff_symbols), src.ctypes.data_as(_P), src.size,
                                          ptr(coef), coef.size)
    if rc:
        raise ValueError(_JPEG_STATUS.get(rc, "a scan header that does not fit the frame"))


def jpeg_decode(ctx: Context, frame: JpegFrame, coef: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """svgr_jpeg_decode: the (height, width, 4) uint8 pixels of a frame from its coefficients and its components'
    quantisation tables (n_comp, 64) uint16, made on the device and downloaded."""
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    quant = np.ascontiguousarray(quant, dtype=np.uint16)
    if quant.shape != (frame.n_comp, 64):
        raise ValueError("jpeg_decode: one quantisation table of 64 entries per component")
    out = ctx.alloc(frame.width * frame.height * 4)
    _check(ctx.lib.svgr_jpeg_decode(ctx.handle, C.byref(frame), ptr(coef), coef.size, ptr(quant), out.handle))
    return out.download((frame.height, frame.width, 4), np.uint8)


def jpeg_n_coef(frame: JpegFrame) -> int:
    """The number of int16 coefficients of a frame (the layout of include/svgr.h)."""
    hmax, vmax = max(frame.h[:frame.n_comp]), max(frame.v[:frame.n_comp])
    mcus = -(-frame.width // (8 * hmax)) * -(-frame.height // (8 * vmax))
    return 64 * mcus * sum(frame.h[i] * frame.v[i] for i in range(frame.n_comp))


def jpeg_encode(ctx: Context, frame: JpegFrame, rgba8, quant: np.ndarray) -> np.ndarray:
    """svgr_jpeg_encode: the frame's quantised int16 coefficients from its (height, width, 4) uint8 pixels -- a DeviceBuffer
    that holds them, or a host array, which is uploaded first -- and its components' quantisation tables (n_comp, 64)."""
    quant = np.ascontiguousarray(quant, dtype=np.uint16)
    if quant.shape != (frame.n_comp, 64):
        raise ValueError("jpeg_encode: one quantisation table of 64 entries per component")
    if not isinstance(rgba8, DeviceBuffer):
        px = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if px.shape != (frame.height, frame.width, 4):
            raise ValueError("jpeg_encode: the pixels are a (height, width, 4) uint8 array of the frame's size")
        rgba8 = ctx.from_host(px)
    coef = np.empty(jpeg_n_coef(frame), dtype=np.int16)
    _check(ctx.lib.svgr_jpeg_encode(ctx.handle, C.byref(frame), rgba8.handle, ptr(quant), ptr(coef), coef.size))
    return coef


def _huff_tables(huff_counts, huff_symbols):
    assert huff_counts.dtype == np.uint8 and huff_counts.shape == (8, 16) and huff_counts.flags.c_contiguous
    assert huff_symbols.dtype == np.uint8 and huff_symbols.shape == (8, 256) and huff_symbols.flags.c_contiguous


def jpeg_entropy_encode(scan: JpegScan, huff_counts: np.ndarray, huff_symbols: np.ndarray, coef: np.ndarray) -> bytes:
    """svgr_jpeg_entropy_encode (host only): the entropy-coded segment of one baseline scan of `coef`.  ValueError when the
    tables cannot code the data."""
    _huff_tables(huff_counts, huff_symbols)
    assert coef.dtype == np.int16 and coef.flags.c_contiguous
    lib, n = load_library(), C.c_int64()
    out = np.empty(coef.size // 4 + 4096, dtype=np.uint8)   # (a first guess; the call reports what it needs)
    for _ in range(2):
        rc = lib.svgr_jpeg_entropy_encode(C.byref(scan), ptr(huff_counts), ptr(huff_symbols), ptr(coef), coef.size, ptr(out), out.size,
                                          C.byref(n))
        if rc != JPEG_NO_ROOM:
            break
        out = np.empty(n.value, dtype=np.uint8)
    if rc:
        raise ValueError("the Huffman tables have no code for a value of the scan" if rc == 2 else
                         "a scan description that does not fit the frame")
    return out[:n.value].tobytes()


def jpeg_symbol_counts(scan: JpegScan, coef: np.ndarray) -> np.ndarray:
    """svgr_jpeg_symbol_counts (host only): (8, 256) int64, how often the scan uses each symbol of DC tables 0-3 and AC
    tables 0-3."""
    assert coef.dtype == np.int16 and coef.flags.c_contiguous
    counts = np.zeros((8, 256), dtype=np.int64)
    if load_library().svgr_jpeg_symbol_counts(C.byref(scan), ptr(coef), coef.size, ptr(counts)):
        raise ValueError("a scan description that does not fit the frame, or a value no baseline table can code")
    return counts


DEFLATE_NO_ROOM = 5   # SVGR_DEFLATE_NO_ROOM


def deflate_chunk() -> int:
    """Bytes per chunk (= per workgroup and per block of the stream) of the deflate kernels (svgr_deflate_chunk)."""
    return int(load_library().svgr_deflate_chunk())


def png_filter(ctx: Context, rgba8: DeviceBuffer, rows: int, cols: int, filter: int) -> DeviceBuffer:
    """svgr_png_filter: the filtered scanlines (rows * (1 + 4 * cols) bytes, on the device) of the RGBA8 bytes in `rgba8`;
    `filter` is a type 0-4 or 5 for the adaptive choice."""
    out = ctx.alloc(max(rows, 1) * (1 + 4 * max(cols, 1)))
    _check(ctx.lib.svgr_png_filter(ctx.handle, rgba8.handle, rows, cols, filter, out.handle))
    return out


PNG_SRC_RGBA_F64, PNG_SRC_MASK_F64, PNG_SRC_RGBA_U8 = 0, 1, 2   # SVGR_PNG_SRC_*
PNG_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}                         # SVGR_PNG_COLOR_* -> samples per pixel


def png_filter_span() -> int:
    """Bytes of a row per pass of a workgroup of the general filter kernel (svgr_png_filter_span)."""
    return int(load_library().svgr_png_filter_span())


def png_samples(ctx: Context, src: DeviceBuffer, kind: int, rows: int, cols: int, color: int, depth: int) -> DeviceBuffer:
    """svgr_png_samples: the packed samples (rows * cols * bpp bytes, on the device) of the pixels in `src`; `kind` is one of
    PNG_SRC_*, `color` a PNG colour type (0, 2, 4, 6), `depth` 8 or 16."""
    out = ctx.alloc(max(rows * cols, 1) * PNG_CHANNELS.get(color, 4) * 2)
    _check(ctx.lib.svgr_png_samples(ctx.handle, src.handle, kind, rows, cols, color, depth, out.handle))
    return out


def png_filter_bytes(ctx: Context, src: DeviceBuffer, rows: int, row_bytes: int, bpp: int, filter: int) -> DeviceBuffer:
    """svgr_png_filter_bytes: the filtered scanlines (rows * (1 + row_bytes) bytes, on the device) of `rows` rows of `row_bytes`
    bytes at `bpp` bytes a pixel; `filter` is a type 0-4 or 5 for the adaptive choice."""
    out = ctx.alloc(max(rows, 1) * (1 + max(row_bytes, 1)))
    _check(ctx.lib.svgr_png_filter_bytes(ctx.handle, src.handle, rows, row_bytes, bpp, filter, out.handle))
    return out


def deflate_once(ctx: Context, src: DeviceBuffer, n_bytes: int, huffman: int, out_cap: int):
    """One svgr_deflate call with room for `out_cap` bytes: ``(status, length needed, bytes written)``; the status is 0 or
    DEFLATE_NO_ROOM (nothing is written then)."""
    n = C.c_int64()
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    rc = ctx.lib.svgr_deflate(ctx.handle, src.handle, n_bytes, huffman, ptr(out), out_cap, C.byref(n))
    if rc not in (0, DEFLATE_NO_ROOM):
        _check(rc)
    return rc, int(n.value), out[:n.value if rc == 0 else 0].tobytes()


def deflate(ctx: Context, src: DeviceBuffer, n_bytes: int, huffman: int) -> bytes:
    """svgr_deflate: the zlib stream of the first `n_bytes` of `src`."""
    n = C.c_int64()
    # (9 bits per byte at the worst plus a header per chunk: untouched pages of the array cost nothing, a second call would
    #  compress everything again; the call reports what it needs all the same)
    out = np.empty(n_bytes + n_bytes // 4 + 4096, dtype=np.uint8)
    for _ in range(2):
        rc = ctx.lib.svgr_deflate(ctx.handle, src.handle, n_bytes, huffman, ptr(out), out.size, C.byref(n))
        if rc != DEFLATE_NO_ROOM:
            break
        out = np.empty(n.value, dtype=np.uint8)
    _check(rc)
    return out[:n.value].tobytes()


def quant_block() -> int:
    """Pixels per workgroup of the quantiser's kernels (svgr_quant_block)."""
    return int(load_library().svgr_quant_block())


def quant_groups() -> int:
    """The most workgroups of svgr_quant_bins' histogram kernel (svgr_quant_groups): beyond that many blocks a workgroup takes several."""
    return int(load_library().svgr_quant_groups())


def quant_distinct(ctx: Context, rgba8: DeviceBuffer, rows: int, cols: int, max_colors: int):
    """svgr_quant_distinct: the distinct canonical pixels of the image as ascending uint32, or None when there are more than
    `max_colors`."""
    colors = np.zeros(max(max_colors, 1), dtype=np.uint32)
    n, overflow = C.c_int64(), C.c_int()
    _check(ctx.lib.svgr_quant_distinct(ctx.handle, rgba8.handle, rows, cols, max_colors, ptr(colors), C.byref(n), C.byref(overflow)))
    return None if overflow.value else colors[:n.value].copy()


def quant_bins(ctx: Context, rgba8: DeviceBuffer, rows: int, cols: int):
    """svgr_quant_bins: ``(keys (n,) uint32 ascending, bins (n, 5) uint64)``: per non-empty bin its pixels and the sums of X."""
    cap = max(min(rows * cols, 1 << 20), 1)
    keys, bins = np.empty(cap, dtype=np.uint32), np.empty((cap, 5), dtype=np.uint64)   # (untouched pages cost nothing)
    n = C.c_int64()
    _check(ctx.lib.svgr_quant_bins(ctx.handle, rgba8.handle, rows, cols, ptr(keys), ptr(bins), cap, C.byref(n)))
    return keys[:n.value].copy(), bins[:n.value].copy()


def _quant_index_buffers(ctx: Context, rows: int, cols: int, palette: np.ndarray, stream: bool, indices: bool):
    """(entries, palette on the device, stream buffer or None, index buffer or None) of svgr_quant_index and svgr_quant_dither."""
    pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 4)
    n = len(pal)
    depth = 1 if n <= 2 else 2 if n <= 4 else 4 if n <= 16 else 8
    d_pal = ctx.from_host(pal) if n else ctx.alloc(4)
    out_s = ctx.alloc(max(rows, 1) * (1 + (max(cols, 1) * depth + 7) // 8)) if stream else None
    out_i = ctx.alloc(max(rows * cols, 1)) if indices else None
    return n, d_pal, out_s, out_i


def quant_index(ctx: Context, rgba8: DeviceBuffer, rows: int, cols: int, palette: np.ndarray, stream: bool = True, indices: bool = False):
    """svgr_quant_index: ``(stream, indices)``, each a DeviceBuffer or None: the packed scanlines (filter bytes included) and
    the plain byte indices of the image under `palette`, an (n, 4) uint8 array of RGBA entries."""
    n, d_pal, out_s, out_i = _quant_index_buffers(ctx, rows, cols, palette, stream, indices)
    _check(ctx.lib.svgr_quant_index(ctx.handle, rgba8.handle, rows, cols, d_pal.handle, n, out_s.handle if stream else None,
                                    out_i.handle if indices else None))
    ctx.sync()   # (the palette's block is released when this returns)
    return out_s, out_i


DITHER_MODES = {"ordered": 1, "diffusion": 2}


def dither_tile() -> tuple:
    """(rows, columns) of a tile of the diffusion kernel (svgr_dither_tile_rows, svgr_dither_tile_cols): its launch seams."""
    lib = load_library()
    return int(lib.svgr_dither_tile_rows()), int(lib.svgr_dither_tile_cols())


def quant_dither(ctx: Context, rgba8: DeviceBuffer, rows: int, cols: int, palette: np.ndarray, mode, amp: int = 0, stream: bool = True,
                 indices: bool = False):
    """svgr_quant_dither: ``quant_index`` with dithering: ``mode`` is "ordered" (with ``amp``, the palette's amplitude:
    ``quant.ordered_amplitude``), "diffusion", or the entry's own number."""
    n, d_pal, out_s, out_i = _quant_index_buffers(ctx, rows, cols, palette, stream, indices)
    _check(ctx.lib.svgr_quant_dither(ctx.handle, rgba8.handle, rows, cols, d_pal.handle, n, DITHER_MODES.get(mode, mode), int(amp),
                                     out_s.handle if stream else None, out_i.handle if indices else None))
    ctx.sync()   # (the palette's block is released when this returns)
    return out_s, out_i
