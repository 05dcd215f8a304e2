"""ctypes binding of libwvn_hip.so (include/wvn_hip.h).

PyTorch supplies device memory and streams; every compute call on the hot path goes through this
module into hand-written HIP kernels.  There is NO fallback: if the shared library is missing or a
call returns non-zero the caller gets an exception.
"""
import ctypes as C
import os
import threading

import torch  # noqa: F401  (must be imported first: its bundled libamdhip64.so.7 is the one HIP runtime of the process)

_HERE = os.path.dirname(os.path.abspath(__file__))
# WVN_LIB_PATH: load another build of the same library (same-box A/B runs of compiler flags, scripts/ab_lib.sh); never a fallback
LIB_PATH = os.environ.get("WVN_LIB_PATH") or os.path.join(_HERE, "lib", "libwvn_hip.so")
if os.environ.get("WVN_LIB_PATH"):
    import sys as _sys

    print(f"[wild_visual_navigation_amd] WVN_LIB_PATH is set: loading {LIB_PATH} instead of the in-tree build", file=_sys.stderr)

WVN_MAX_DEPTH = 32
PREC_F32, PREC_BF16, PREC_X3, PREC_FP8, PREC_F16, PREC_MIX = 0, 1, 2, 3, 4, 5
VIT_MLP_FUSED = 1
VIT_QKV_FUSED = 2
VIT_FUSE_ANY_SIZE = 4
VIT_NO_PROJ_IN_MLP = 8
VIT_NO_LN_HANDOVER = 16
VIT_NO_A384_X3 = 32
VIT_NO_MX = 1024


def vit_qsplit_blocks(n: int) -> int:
    """WVN_VIT_QSPLIT_BLOCKS(n) of include/wvn_hip.h: the flag bits that make the first n blocks of WVN_PREC_MIX take q as two planes."""
    return ((int(n) + 1) & 63) << 16

PROF_CATS = ("patchify", "patch_gemm", "layernorm", "qkv_gemm", "attention", "proj_gemm", "fc1_gemm", "fc2_gemm")

# epilogue codes (wvn_internal.h)
EPI_BF16, EPI_GELU_BF16, EPI_RELU_BF16, EPI_F32, EPI_RESID_F32, EPI_ACCUM_F32 = range(6)
EPI_QKV = 7   # (q | k | v^T in the attention kernels' layouts: wvn_gemm_a768_fp8)
EPI_GELU_MX8 = 9   # (gelu -> e4m3 with MX block scales: wvn_gemm_a768_fp8 -> wvn_gemm_fp8_mx)
F32_NONE, F32_RELU, F32_GELU, F32_RESID, F32_SIGMOID0, F32_RELUMASK = range(6)


class WvnError(RuntimeError):
    pass


ERR_ARG = 1001   # WVN_ERR_ARG: bad argument, or "this route is not eligible" -- returned before anything is launched


# ConfidenceGenerator methods of the training step (include/wvn_hip.h: WVN_CONF_*, wvn_conf_desc)
CONF_METHODS = {"latest_measurement": 0, "running_mean": 1, "kalman_filter": 2, "moving_average": 3}
CONF_WINDOW = 5
CONF_STATE_DOUBLES = 32
CONF_S_MEAN, CONF_S_VAR, CONF_S_STD, CONF_S_RUN_N, CONF_S_RUN_SUM, CONF_S_RUN_SUMSQ, CONF_S_HEAD, CONF_S_FILL, CONF_S_RING = range(9)


class ConfDesc(C.Structure):
    _fields_ = [("method", C.c_int), ("balanced", C.c_int), ("state", C.c_void_p), ("minmax", C.c_void_p)]


class VitLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "qkv_w", "proj_w", "fc1_w", "fc2_w", "qkv_b", "proj_b", "fc1_b", "fc2_b", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "ls1", "ls2", "qkv_s", "proj_s", "fc1_s", "fc2_s", "fc2_w_fused", "fc1_w_fused", "qkv_w_fused", "proj_w_frag",
        "qkv_w_mx", "proj_w_mx", "fc1_w_mx", "fc2_w_mx")]


class VitModel(C.Structure):
    _fields_ = [
        ("img_size", C.c_int), ("patch", C.c_int), ("dim", C.c_int), ("depth", C.c_int), ("heads", C.c_int),
        ("mlp_dim", C.c_int), ("precision", C.c_int), ("flags", C.c_int),
        ("patch_w", C.c_void_p), ("patch_b", C.c_void_p), ("cls_pos", C.c_void_p), ("pos", C.c_void_p),
        ("norm_g", C.c_void_p), ("norm_b", C.c_void_p),
        ("layers", VitLayer * WVN_MAX_DEPTH),
    ]


class StegoHead(C.Structure):
    """include/wvn_hip.h: wvn_stego_head (the head of wvn_vit_forward_frames_head)."""
    _fields_ = [("w_cat", C.c_void_p), ("b_cat", C.c_void_p), ("w_nl", C.c_void_p), ("b_nl", C.c_void_p), ("code", C.c_void_p),
                ("code_dim", C.c_int), ("ld_code", C.c_int)]


class MlpDesc(C.Structure):
    _fields_ = [("D", C.c_int), ("H1", C.c_int), ("H2", C.c_int), ("reserved", C.c_int)]


class RnvpDesc(C.Structure):
    _fields_ = [("D", C.c_int), ("h", C.c_int), ("flows", C.c_int)]


class OverlayDesc(C.Structure):
    """include/wvn_hip.h: wvn_overlay_desc."""
    _fields_ = [("img", C.c_void_p), ("frame_max", C.c_void_p), ("maps", C.c_void_p * 4), ("seg", C.c_void_p), ("lut", C.c_void_p),
                ("mask", C.c_void_p), ("boundary_seg", C.c_void_p), ("out", C.c_void_p),
                ("out_row_bytes", C.c_longlong), ("out_frame_bytes", C.c_longlong)] + \
               [(n, C.c_int) for n in ("img_u8", "unit_range", "B", "H", "W", "kind", "nmaps", "plain", "id_bytes", "seg_bytes",
                                       "boundary_bytes", "S", "lut_u8", "N", "alpha", "boundary_alpha")]


class DrawDesc(C.Structure):
    """include/wvn_hip.h: wvn_draw_desc."""
    _fields_ = [(n, C.c_void_p) for n in ("canvas", "kinds", "points", "colours", "frame", "panel", "skipped")] + \
               [("row_bytes", C.c_longlong), ("frame_bytes", C.c_longlong)] + [(n, C.c_int) for n in ("B", "H", "P", "Wp", "N")]


class MetricDesc(C.Structure):
    """include/wvn_hip.h: wvn_metric_desc."""
    _fields_ = [("score", C.c_void_p * 2), ("target", C.c_void_p * 2), ("seg", C.c_void_p), ("seg_off", C.c_void_p),
                ("thresholds", C.c_void_p), ("state", C.c_void_p), ("seg_counts", C.c_void_p),
                ("score_stride", C.c_longlong * 2), ("target_stride", C.c_longlong * 2), ("state_stride", C.c_longlong),
                ("tau", C.c_float), ("score_kind", C.c_int * 2), ("target_kind", C.c_int * 2), ("target_dtype", C.c_int * 2)] + \
               [(n, C.c_int) for n in ("n_scores", "n_targets", "B", "H", "W", "S", "T", "has_ignore", "ignore_index", "seg_bytes")]


class JpegGeometry(C.Structure):
    """include/wvn_hip.h: wvn_jpeg_geometry."""
    _fields_ = [(n, C.c_int) for n in ("width", "height", "components", "sampling", "restart_interval")]


# include/wvn_hip.h: WVN_JPEG_* statuses and samplings
JPEG_STATUS = ("OK", "TRUNCATED", "BAD_MARKER", "BAD_TABLE", "BAD_HUFFMAN", "BAD_COEFFICIENT", "UNSUPPORTED", "GEOMETRY_MISMATCH",
               "BAD_GEOMETRY", "OUT_OF_RANGE")
(JPEG_OK, JPEG_TRUNCATED, JPEG_BAD_MARKER, JPEG_BAD_TABLE, JPEG_BAD_HUFFMAN, JPEG_BAD_COEFFICIENT, JPEG_UNSUPPORTED,
 JPEG_GEOMETRY_MISMATCH, JPEG_BAD_GEOMETRY, JPEG_OUT_OF_RANGE) = range(10)
JPEG_SAMPLING = ("gray", "4:4:4", "4:2:2", "4:2:0")
JPEG_MAX_THREADS = 16
JPEG_MAX_BATCH = 4096
# include/wvn_hip.h: WVN_SRC_* source kinds and WVN_ORDER_* output orders of the raw camera ingest (the names are ROS's encodings)
SRC_KINDS = {"mono8": 0, "rgb8": 1, "bgr8": 2, "planar": 3, "bayer_rggb8": 4, "bayer_bggr8": 5, "bayer_gbrg8": 6, "bayer_grbg8": 7}
ORDER_RGB, ORDER_BGR, ORDER_GRAY = 0, 1, 2
FRAME_MAX_DIM = 65535
METRIC_MAX_T, METRIC_STATE_TAIL = 8192, 8
METRIC_DENSE, METRIC_PER_SEGMENT = 0, 1
METRIC_U8, METRIC_I32, METRIC_F32 = 0, 1, 2
OVERLAY_MAX_COLOURS, OVERLAY_MAX_MAPS = 1024, 4
OVERLAY_VALUES, OVERLAY_LABELS, OVERLAY_SEGMENTS = 0, 1, 2
DRAW_MAX_PRIMITIVES = 65536
DRAW_LINE, DRAW_LINE2, DRAW_DISC = 0, 1, 2
# include/wvn_hip.h: WVN_GRID_* limits and the `unknown` modes of wvn_grid_sdf
GRID_MAX_N, GRID_MAX_CHANNELS, GRID_MAX_CAMERAS, GRID_MAX_DISCS = 4096, 4, 64, 8
GRID_UNKNOWN = {"obstacle": 0, "free": 1, "neither": 2}
# include/wvn_hip.h: WVN_GRID_ELEVATION_* / WVN_GRID_DEPTH_*
GRID_ELEVATION_MAX_POINTS = 1 << 22
GRID_ELEVATION_STATS = ("invalid", "near", "high", "ramp", "outside", "gated", "unrepresentable", "inliers")
GRID_DEPTH_F32, GRID_DEPTH_U16 = 0, 1
GRID_ELEVATION_CLEAR_RAYS = 1


class GridElevationParams(C.Structure):
    """include/wvn_hip.h: wvn_grid_elevation_params."""
    _fields_ = [(n, C.c_float) for n in ("sensor_noise_factor", "mahalanobis_thresh", "outlier_variance", "min_valid_distance",
                                         "max_height_range", "ramp_a", "ramp_b", "ramp_c", "initial_variance", "max_variance",
                                         "max_ray_length", "clear_margin")] + [("clear_min_rays", C.c_int)]


MLP_KIND_DOUBLE = 1   # include/wvn_hip.h: WVN_MLP_KIND_DOUBLE (MlpDesc.reserved)


_lib = None
_lock = threading.Lock()

_i, _f, _p, _ll, _sz = C.c_int, C.c_float, C.c_void_p, C.c_longlong, C.c_size_t
_SIGNATURES = {
    "wvn_version": ([], _i),
    "wvn_vit_workspace_bytes": ([_p, _i], _sz),
    "wvn_vit_forward": ([_p, _p, _i, _p, _p, _i, _p, _sz, _p], _i),
    "wvn_vit_forward_u8": ([_p, _p, _i, _p, _p, _i, _p, _sz, _p], _i),
    "wvn_vit_forward_frames": ([_p, _p, _i, _i, _i, _p, _p, _i, _p, _p, _i, _p, _sz, _p], _i),
    "wvn_vit_forward_frames_pair": ([_p, _p, _i, _i, _i, _p, _p, _p, _i, _p, _p, _i, _p, _sz, _p], _i),
    "wvn_vit_forward_frames_head": ([_p, _p, _i, _i, _i, _p, _p, _p, _i, _p, _p, _sz, _p], _i),
    "wvn_debug_stego_head_fused": ([_p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_resize_nearest_crop": ([_p, _p, _ll, _i, _i, _p, _p, _i, _i, _i, _p], _i),
    "wvn_prof_enable": ([_i], _i),
    "wvn_prof_collect": ([_p, _p], _i),
    "wvn_gemm_bf16": ([_p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_debug_attention_variant": ([_i], _i),
    "wvn_debug_attention_planes": ([_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_debug_kmeans_assign_form": ([_i], _i),
    "wvn_debug_kmeans_screen_stats": ([_p, _i], _i),
    "wvn_debug_mlp_x3_frag": ([_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p], _i),
    "wvn_debug_gemm_n384_x3": ([_p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p], _i),
    "wvn_debug_gemm_n384_mx": ([_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p], _i),
    "wvn_debug_mlp_mx": ([_p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p], _i),
    "wvn_debug_qkv_mx": ([_p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p, _p], _i),
    "wvn_debug_gemm_a384_x3": ([_p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p], _i),
    "wvn_stream_create_cu_mask": ([_p, _p, _i], _i),
    "wvn_stream_destroy": ([_p], _i),
    "wvn_debug_qkv_fused_timing": ([_p], _i),
    "wvn_debug_mlp_fused_timing": ([_p], _i),
    "wvn_qkv_fused": ([_p, _i, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p], _i),
    "wvn_proj_mlp_fused": ([_p, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p], _i),
    "wvn_mlp_fused": ([_p, _i, _p, _p, _f, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p], _i),
    "wvn_gemm_f16": ([_p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_qkv_fused_f16": ([_p, _i, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p], _i),
    "wvn_proj_mlp_resident": ([_p, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _f, _p, _p], _i),
    "wvn_proj_mlp_resident_f16": ([_p, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _f, _p, _p], _i),
    "wvn_qkv_prenorm": ([_p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p], _i),
    "wvn_qkv_prenorm_f16": ([_p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p], _i),
    "wvn_proj_mlp_fused_f16": ([_p, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p], _i),
    "wvn_mlp_fused_f16": ([_p, _i, _p, _p, _f, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p], _i),
    "wvn_attention_f16": ([_p, _p, _p, _p, _i, _i, _i, _i, _f, _p], _i),
    "wvn_gemm_x3": ([_p, _p, _i, _p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_quantize_rows_fp8": ([_p, _i, _i, _p, _i, _p, _i, _i, _p], _i),
    "wvn_layernorm_fp8": ([_p, _p, _p, _p, _i, _p, _i, _i, _f, _p], _i),
    "wvn_gemm_fp8": ([_p, _i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_gemm_a768_fp8": ([_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _i, _i, _i, _f, _p], _i),
    "wvn_gemm_fp8_mx": ([_p, _i, _p, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_split_planes": ([_p, _i, _p, _p, _i, _i, _i, _p], _i),
    "wvn_attention_x3": ([_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p], _i),
    "wvn_gemm_f32": ([_p, _i, _i, _p, _i, _i, _p, _p, _i, _i, _i, _i, _i, _p, _i, _p], _i),
    "wvn_layernorm": ([_p, _p, _p, _p, _i, _i, _i, _f, _p], _i),
    "wvn_attention_bf16": ([_p, _p, _p, _p, _i, _i, _i, _i, _f, _p], _i),
    "wvn_attention_f32": ([_p, _p, _p, _p, _i, _i, _i, _i, _f, _p], _i),
    "wvn_patchify": ([_p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_patchify_u8": ([_p, _p, _i, _i, _i, _p], _i),
    "wvn_cast_f32_to_bf16": ([_p, _p, _ll, _p], _i),
    "wvn_upsample_bilinear": ([_p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_upsample_nearest_i32": ([_p, _p, _i, _i, _i, _p], _i),
    "wvn_segpool_bilinear_mean": ([_p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_segpool_patch_labels": ([_p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_segmean_scratch_bytes": ([_i, _i, _i, _i], _sz),
    "wvn_segmean_tokens": ([_p, _p, _p, _p, _p, _sz, _i, _i, _i, _i, _p], _i),
    "wvn_label_pool": ([_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p], _i),
    "wvn_label_pool_batched": ([_p, _i, _i, _i, _i, _i, _p, _p, _p], _i),
    "wvn_random_pixels": ([C.c_uint, C.c_uint, _i, _i, _i, _i, _p, _p, _p], _i),
    "wvn_gather_bilinear": ([_p, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_dense_sift": ([_p, _i, _p, _i, _i, _i, _i, _p], _i),
    "wvn_dense_sift_segpool": ([_p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_project_render_fmin": ([_p, _i, _p, _i, _i, _i, _i, _i, _p, _f, _p], _i),
    "wvn_wire_bytes": ([_i, _i, _i, _i], _sz),
    "wvn_wire_pack": ([_p, _i, _p, _i, _p, _i, _i, _i, _i, _p], _i),
    "wvn_wire_unpack": ([_p, _p, _p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_slic_num_clusters": ([_i, _i, _i], _i),
    "wvn_slic_scratch_bytes": ([_i, _i, _i], _sz),
    "wvn_slic": ([_p, _i, _i, _i, _i, _f, _i, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_slic_connectivity_scratch_bytes": ([_i, _i, _i, _i], _sz),
    "wvn_slic_connectivity": ([_p, _p, _i, _i, _i, _i, _i, _p, _sz, _p], _i),
    "wvn_seg_centers": ([_p, _p, _p, _i, _i, _i, _p], _i),
    "wvn_seg_adjacency": ([_p, _p, _p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_normalize_rows": ([_p, _i, _p, _i, _i, _p], _i),
    "wvn_argmax_rows": ([_p, _i, _i, _i, _p, _p], _i),
    "wvn_kmeans_scratch_bytes": ([_i, _i, _i, _i], _sz),
    "wvn_kmeans_pixels_scratch_bytes": ([_i, _i, _i, _i, _i], _sz),
    "wvn_kmeans_cosine_pixels": ([_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_flip_average": ([_p, _p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_kmeans_pixels_linear_supported_shape": ([_i, _i, _i, _i], _i),
    "wvn_kmeans_pixels_linear_scratch_bytes": ([_i, _i, _i, _i, _i], _sz),
    "wvn_kmeans_cosine_pixels_linear": ([_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_debug_kmeans_linear_rows": ([_i], _i),
    "wvn_debug_n384_pair": ([_i], _i),
    "wvn_table_argmax_slots": ([_i], _i),
    "wvn_table_bilerp_argmax": ([_p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_table_bilerp_argmax_ac": ([_p, _p, _i, _i, _i, _i, _i, _p], _i),
    "wvn_kmeans_cosine_pixels_linear_ac": ([_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_cast_rows": ([_p, _i, _p, _i, _i, _i, _i, _p], _i),
    "wvn_kmeans_cosine": ([_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_mlp_param_count": ([_p], _sz),
    "wvn_mlp_workspace_bytes": ([_p, _i], _sz),
    "wvn_double_mlp_row_tile": ([], _i),
    "wvn_double_mlp_fused_ok": ([_p, _i], _i),
    "wvn_mlp_forward": ([_p, _p, _p, _i, _i, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_mlp_train_phase_a": ([_p, _p, _p, _i, _p, _i, _p, _p, _sz, _p], _i),
    "wvn_mlp_train_phase_b": ([_p, _p, _p, _i, _p, _p, _i, _p, _f, _f, _f, _p, _p, _p, _sz, _p], _i),
    "wvn_compact_segment_rows": ([_p, _i, _p, _i, _p, _i, _i, _p, _p, _p, _p], _i),
    "wvn_mlp_train_phase_a_rows": ([_p, _p, _p, _i, _p, _i, _p, _p, _p, _sz, _p, _p], _i),
    "wvn_mlp_train_phase_b_rows": ([_p, _p, _p, _i, _p, _p, _i, _p, _p, _f, _f, _f, _p, _p, _p, _sz, _i, _p], _i),
    "wvn_mlp_train_phase_c": ([_p, _p, _p, _p, _p, _i, _f, _p, _f, _f, _p, _p], _i),
    "wvn_mlp_train_phase_a_conf": ([_p, _p, _p, _i, _p, _i, _p, _p, _p, _sz, _p, _p, _p], _i),
    "wvn_mlp_train_phase_b_conf": ([_p, _p, _p, _i, _p, _p, _i, _p, _p, _f, _f, _f, _p, _p, _p, _sz, _i, _p, _p], _i),
    "wvn_mlp_train_phase_c_conf": ([_p, _p, _p, _p, _p, _i, _f, _p, _f, _f, _p, _p, _p], _i),
    "wvn_mlp_confidence": ([_p, _i, _p, _i, _f, _f, _f, _p, _p, _i, _i, _p], _i),
    "wvn_pixel_mlp_pack_bytes": ([_p], _sz),
    "wvn_pixel_mlp_zx_cols": ([_p], _i),
    "wvn_pixel_mlp_pack": ([_p, _p, _p, _p], _i),
    "wvn_pixel_mlp_exact_pack_bytes": ([_p], _sz),
    "wvn_pixel_mlp_exact_workspace_bytes": ([_p, _i, _i], _sz),
    "wvn_pixel_mlp_exact_pack": ([_p, _p, _p, _p], _i),
    "wvn_pixel_mlp_infer_exact": ([_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_pixel_mlp_infer": ([_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _p], _i),
    "wvn_rnvp_pack_bytes": ([_p], _sz),
    "wvn_rnvp_row_tile": ([], _i),
    "wvn_rnvp_pack": ([_p, _p, _p, _p, _p, _p], _i),
    "wvn_rnvp_forward_rows": ([_p, _p, _p, _i, _ll, _f, _f, _f, _p, _p, _p, _p, _p, _i, _p], _i),
    "wvn_rnvp_forward_pixels": ([_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _p, _i, _p], _i),
    "wvn_rnvp_train_param_count": ([_p], _sz),
    "wvn_rnvp_train_workspace_bytes": ([_p, _ll], _sz),
    "wvn_rnvp_train_pack_bytes": ([_p], _sz),
    "wvn_rnvp_train_pack": ([_p, _p, _p, _p, _p], _i),
    "wvn_rnvp_train_phase_a": ([_p, _p, _p, _i, _ll, _p, _p, _p, _sz, _p], _i),
    "wvn_rnvp_train_phase_b": ([_p, _p, _p, _ll, _p, _p, _p, _sz, _p], _i),
    "wvn_rnvp_train_phase_c": ([_p, _p, _p, _p, _p, _i, _f, _p, _i, _p, _p, _p, _p, _p, _p, _p], _i),
    "wvn_segment_predict_workspace_bytes": ([_p, _i, _i], _sz),
    "wvn_segment_predict": ([_p, _p, _p, _i, _ll, _i, _i, _p, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_gcn_workspace_bytes": ([_p, _i, _ll], _sz),
    "wvn_gcn_graph_from_edges": ([_p, _ll, _ll, _i, _i, _ll, _p, _p, _sz, _p], _i),
    "wvn_gcn_graph_from_bitmaps": ([_p, _ll, _ll, _ll, _i, _i, _ll, _p, _p, _sz, _p], _i),
    "wvn_gcn_forward": ([_p, _p, _p, _i, _i, _ll, _p, _p, _sz, _p], _i),
    "wvn_gcn_segment_predict": ([_p, _p, _p, _i, _i, _i, _ll, _p, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_gcn_train_workspace_bytes": ([_p, _i, _ll], _sz),
    "wvn_gcn_train_saved": ([_p, _i, _ll, _p], _i),
    "wvn_gcn_train_phase_a": ([_p, _p, _p, _i, _p, _ll, _ll, _i, _p, _i, _ll, _p, _p, _p, _sz, _p, _p, _p], _i),
    "wvn_gcn_train_phase_b": ([_p, _p, _p, _i, _p, _p, _i, _ll, _p, _f, _f, _f, _p, _p, _p, _sz, _p, _p], _i),
    "wvn_seg_adjacency_batched": ([_p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_debug_gemm_bf16_timed": ([_p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p, _p], _i),
    "wvn_debug_f16_saturate": ([_p, _p, _i, _p], _i),
    "wvn_debug_slic_lab": ([_p, _i, _i, _p, _p, _p, _p], _i),
    "wvn_debug_attention_timing": ([_p], _i),
    "wvn_debug_gemm_n384": ([_p, _i, _p, _i, _p, _p, _i, _i, _i, _p], _i),
    "wvn_dense_crf_workspace_bytes": ([_i, _i, _i, _i], _sz),
    "wvn_dense_crf": ([_p, _i, _ll, _ll, _ll, _p, _i, _ll, _ll, _ll, _p, _i, _i, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_crf_image": ([_p, _i, _i, _i, _i, _p, _p, _i, _i, _p, _p], _i),
    "wvn_dense_crf_permutohedral_workspace_bytes": ([_i, _i, _i, _i], _sz),
    "wvn_dense_crf_permutohedral": ([_p, _i, _ll, _ll, _ll, _p, _i, _ll, _ll, _ll, _p, _i, _i, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_debug_permutohedral_lattice": ([_p, _i, _i, _i, _i, _f, _f, _p, _p, _p, _p, _p, _p, _sz, _p], _i),
    "wvn_frame_max": ([_p, _i, _i, _ll, _p, _p], _i),
    "wvn_overlay": ([_p, _p], _i),
    "wvn_overlay_panels": ([_p, _p], _i),
    "wvn_draw": ([_p, _p], _i),
    "wvn_metric_accumulate": ([_p, _p], _i),
    "wvn_metric_curve": ([_p, _p, _i, _p, _p, _p, _p, _p, _p], _i),
    "wvn_metric_auroc_weighted": ([_p, _p, _p, _ll, _p, _p, _p], _i),
    "wvn_conv2d_pack_floats": ([_i, _i, _i], _sz),
    "wvn_conv2d_pack": ([_p, _p, _i, _i, _i, _p], _i),
    "wvn_conv2d_bn_act": ([_p, _i, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p], _i),
    "wvn_maxpool3x3s2": ([_p, _p, _i, _i, _i, _i, _p], _i),
    "wvn_resnet18_pack_bytes": ([], _sz),
    "wvn_resnet18_pack": ([_p, _p, _p, _p, _sz, _p], _i),
    "wvn_resnet18_workspace_bytes": ([_i, _i, _i], _sz),
    "wvn_resnet18_level_offset": ([_i, _i, _i, _i], _sz),
    "wvn_resnet18_forward": ([_p, _p, _i, _i, _i, _i, _p, _sz, _p], _i),
    "wvn_segpool_pyramid_scratch_bytes": ([_i, _i], _sz),
    "wvn_segpool_pyramid": ([_p, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _i, _p], _i),
    "wvn_jpeg_info": ([_p, _sz, _p], _i),
    "wvn_jpeg_probe_batch": ([_p, _p, _i, _p, _p], _i),
    "wvn_jpeg_coef_bytes": ([_p], _sz),
    "wvn_jpeg_plane_bytes": ([_p], _sz),
    "wvn_jpeg_workspace_bytes": ([_p, _i], _sz),
    "wvn_jpeg_coefficients": ([_p, _sz, _p, _p, _sz, _p], _i),
    "wvn_jpeg_coefficients_batch": ([_p, _p, _i, _p, _p, _sz, _p, _i, _p], _i),
    "wvn_jpeg_device_stage": ([_p, _i, _p, _p, _i, _p], _i),
    "wvn_jpeg_decode_batch": ([_p, _p, _i, _p, _p, _i, _p, _i, _p, _p], _i),
    "wvn_unpack_frames": ([_p, _i, _i, _i, _i, _ll, _ll, _p, _i, _p], _i),
    "wvn_rectify_frames": ([_p, _i, _i, _i, _i, _ll, _ll, _p, _p, _i, _i, _p, _i, _p], _i),
    "wvn_grid_fuse_images": ([_p, _i, _i, _i, _i, _p, _p, _p, _i, _f, _f, _f, _p, _p, _f, _f, _f, _f, _p], _i),
    "wvn_grid_sdf": ([_p, _i, _f, _i, _f, _p, _p, _p], _i),
    "wvn_grid_carrot": ([_p, _p, _i, C.c_double, C.c_double, _f, _f, _p, _i, _f, _f, _f, _p, _p, _p, _p], _i),
    "wvn_grid_elevation_workspace_bytes": ([_i], _sz),
    "wvn_grid_elevation_accumulate_points": ([_p, _p, _i, _i, _p, _p, _p, _i, _f, _f, _f, _p, _p, _i, _p, _p], _i),
    "wvn_grid_elevation_accumulate_depth": ([_p, _i, _i, _i, _i, _p, _p, _p, _p, _i, _f, _f, _f, _p, _p, _i, _p, _p], _i),
    "wvn_grid_elevation_finalise": ([_p, _p, _p, _i, _p, _i, _p, _p, _i, _p, _p, _p], _i),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib() -> C.CDLL:
    """Load (once) and return the shared library.  Raises WvnError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise WvnError(
                        f"{LIB_PATH} not found: build it with `python -m wild_visual_navigation_amd.csrc.build` "
                        "(there is no CPU / eager fallback for the HIP path)"
                    )
                h = C.CDLL(LIB_PATH)
                for name, (args, res) in _SIGNATURES.items():
                    fn = getattr(h, name)  # AttributeError if the header and the library disagree
                    fn.argtypes = args
                    fn.restype = res
                _lib = h
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        kind = {1001: "bad argument", 1002: "workspace too small"}.get(rc, f"hipError_t {rc}")
        raise WvnError(f"libwvn_hip: {what} failed: {kind}")


def ptr(t) -> int:
    """Device pointer of a tensor (None -> NULL).  Tensors must be contiguous where a dense layout is assumed."""
    return 0 if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def require_cuda(t: "torch.Tensor", name: str = "tensor") -> None:
    if not t.is_cuda:
        raise WvnError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
