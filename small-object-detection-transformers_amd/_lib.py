"""ctypes binding of libsodt_hip.so (declarations mirror include/sodt_hip.h).

The product path has NO fallback: if the library is missing or cannot be loaded the
import raises, and every op raises on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(HERE, "libsodt_hip.so")
# SODT_LIB_PATH swaps in an experimental build (tools/exp/ab_build.sh) for A/B timing on one box.  It is a tools-only switch:
# overrides() reports it, ops.version() carries it, and bench.py refuses to run with it set.
LIB_PATH = os.environ.get("SODT_LIB_PATH") or DEFAULT_LIB_PATH
# environment switches that change WHICH native code runs or what it skips; the library itself reads none of them any more
# (round 4), the names stay listed so that bench.py also refuses the retired ones instead of silently ignoring a typo'd intent
DIAGNOSTIC_ENV = ("SODT_LIB_PATH", "SODT_HG_DBG", "SODT_WMSA_ONE_WAVE")


def overrides():
    """Diagnostic environment switches that are set in this process (empty for a product run)."""
    return {k: os.environ[k] for k in DIAGNOSTIC_ENV if os.environ.get(k)}

MAX_SEG = 9
EINVAL, ELAUNCH = 1, 2                                # SODT_EINVAL: refused, nothing launched; SODT_ELAUNCH: the runtime failed
F32, BF16 = 0, 1
U8 = 2                                                # SODT_U8: target dtype of sodt_sr_l1_fwd / _bwd
SR_MODES = {"IR": 0, "RGB": 1, "RGB+IR": 2}           # SODT_SR_IR / SODT_SR_RGB / SODT_SR_RGB_IR
EPI_BIAS, EPI_RESID, EPI_GELU_DUAL, EPI_DGELU = 1, 2, 4, 8
EPI_STATS, EPI_AFFINE_SILU, EPI_DETECT, EPI_OUT_F32 = 16, 32, 64, 128
EPI_GELU, EPI_DGELU_RC, EPI_RELU, EPI_DRELU = 256, 512, 2048, 4096      # (1024: retired, see include/sodt_hip.h)
DETECT_NO_WGRAD, DETECT_NO_DX = 1, 2                  # SODT_DETECT_NO_WGRAD / SODT_DETECT_NO_DX
CHOICES_BLOCK = 1024                                  # SODT_CHOICES_BLOCK: weights per block of sodt_weighted_choices' scan
SAMPLING_BAD_CLASS, SAMPLING_BAD_IMAGE, SAMPLING_ZERO_TOTAL, SAMPLING_NONFINITE_TOTAL = 1, 2, 4, 8     # SODT_SAMPLING_*
STATS_REPL = 16      # SODT_STATS_REPL: replicas of the [2][N] f64 BatchNorm statistics buffer


class Seg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("ld", C.c_int), ("klen", C.c_int), ("dy", C.c_int), ("dx", C.c_int),
                ("mul", C.c_int), ("shr", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int)]


class ASpec(C.Structure):
    _fields_ = [("s", Seg * MAX_SEG), ("nseg", C.c_int), ("spatial", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int)]


class GemmArgs(C.Structure):
    _fields_ = [("a", ASpec),
                ("W", C.c_void_p), ("ldw", C.c_int),
                ("C", C.c_void_p), ("ldc", C.c_int),
                ("C2", C.c_void_p), ("ldc2", C.c_int),
                ("bias", C.c_void_p),
                ("R", C.c_void_p), ("ldr", C.c_int), ("rmod", C.c_int),
                ("aux", C.c_void_p), ("ldaux", C.c_int),
                ("stats", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("flags", C.c_int),
                ("oscatter", C.c_int), ("omul", C.c_int), ("ody", C.c_int), ("odx", C.c_int),
                ("OH", C.c_int), ("OW", C.c_int),
                ("det_na", C.c_int), ("det_no", C.c_int), ("det_hw", C.c_int)]


class GemmTnArgs(C.Structure):
    _fields_ = [("dY", C.c_void_p), ("ldy", C.c_int),
                ("x", ASpec),
                ("dW", C.c_void_p), ("lddw", C.c_int),
                ("dbias", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("kperm_c", C.c_int), ("kperm_t", C.c_int), ("splits", C.c_int),
                ("partial", C.c_void_p), ("partial_floats", C.c_long)]


class LinBwdArgs(C.Structure):
    """sodt_linbwd_args (include/sodt_hip.h): the square 192 -> 192 linear backward, dX and dW from one read of dY."""
    _fields_ = [("dY", C.c_void_p), ("ldy", C.c_int),
                ("X", C.c_void_p), ("ldx", C.c_int),
                ("wT", C.c_void_p), ("ldw", C.c_int),
                ("aux", C.c_void_p), ("ldaux", C.c_int),
                ("dX", C.c_void_p), ("lddx", C.c_int),
                ("dW", C.c_void_p), ("lddw", C.c_int),
                ("dbias", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("flags", C.c_int),
                ("splits", C.c_int),
                ("partial", C.c_void_p), ("partial_floats", C.c_long)]


class DetectArgs(C.Structure):
    """sodt_detect_args (include/sodt_hip.h): the Detect level, forward or backward, in one pass."""
    _fields_ = [("X", C.c_void_p), ("ldx", C.c_int),
                ("W", C.c_void_p), ("ldw", C.c_int),
                ("bias", C.c_void_p),
                ("pred", C.c_void_p),
                ("dX", C.c_void_p), ("lddx", C.c_int),
                ("dW", C.c_void_p), ("lddw", C.c_int),
                ("dbias", C.c_void_p),
                ("B", C.c_int), ("HW", C.c_int), ("na", C.c_int), ("no", C.c_int), ("K", C.c_int), ("flags", C.c_int),
                ("splits", C.c_int),
                ("partial", C.c_void_p), ("partial_floats", C.c_long)]


class StepCtl(C.Structure):
    """sodt_step_ctl (include/sodt_hip.h): the 64-byte device record sodt_grad_stats fills and the _ctl steps read."""
    _fields_ = [("acc_sumsq", C.c_double), ("acc_found", C.c_uint), ("ticket", C.c_uint),
                ("sumsq", C.c_double), ("grad_norm", C.c_double), ("step", C.c_longlong),
                ("found_inf", C.c_float), ("inv_scale_eff", C.c_float), ("clip_coef", C.c_float), ("skip", C.c_int),
                ("reserved", C.c_int * 2)]


# the 64-byte record of sodt_sam_norm / _perturb (include/sodt_hip.h documents it; the header declares no C type for it):
# field -> (byte offset, ctypes type)
SAM_REC_BYTES = 64
SAM_REC = {"acc_sumsq": (0, C.c_double), "acc_found": (8, C.c_uint), "ticket": (12, C.c_uint), "sumsq": (16, C.c_double),
           "norm": (24, C.c_double), "inv": (32, C.c_double), "found": (40, C.c_float), "inv_scale": (44, C.c_float)}


TTA_MAX_PASSES = 4                                    # SODT_TTA_MAX_PASSES


class TtaPass(C.Structure):
    """sodt_tta_pass (include/sodt_hip.h): one augmented input pair of sodt_tta_scale."""
    _fields_ = [("out_rgb", C.c_void_p), ("out_ir", C.c_void_p), ("h", C.c_int), ("w", C.c_int),
                ("Hp", C.c_int), ("Wp", C.c_int), ("flip", C.c_int)]


class PrepDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p),
                ("d0", C.c_int), ("d1", C.c_int), ("d2", C.c_int),
                ("p0", C.c_int), ("p1", C.c_int), ("p2", C.c_int),
                ("dst_ld", C.c_int), ("inner_ld", C.c_int)]


class Conv3Geo(C.Structure):
    """sodt_conv3_geo (include/sodt_hip.h): weight-row / input-pixel / output-pixel maps of the direct 3x3 kernels."""
    _fields_ = [("w_row_stride", C.c_int), ("w_row_off", C.c_int), ("in_mul", C.c_int), ("in_i", C.c_int), ("in_j", C.c_int),
                ("out_mul", C.c_int), ("out_i", C.c_int), ("out_j", C.c_int)]


# name -> argtypes of EVERY exported symbol, type for type what include/sodt_hip.h declares (tests/test_abi_and_host.py parses the
# header and compares); they return int except the ones in RESTYPES
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
SIGNATURES = {
    "sodt_nms_candidates": [_P, _I, _I, C.c_float, _I, _P, _P, _I, _P, _P],
    "sodt_nms_workspace_bytes": [_L, C.POINTER(C.c_size_t)],
    "sodt_nms_select": [_P, _I, _P, _L, C.c_float, _I, _P, C.c_size_t, _P, _P, _P, _P],
    # general.py:425-512 for a whole batch (csrc/nms_batch.hip)
    "sodt_nms_batch_workspace_bytes": [_I, _L, _I, _I, C.POINTER(C.c_size_t)],
    "sodt_nms_batch": [_P, _I, _I, _I, _P, _P, _I, _F, _F, _I, _P, _I, _P, C.c_size_t, _P, _P, _P, _P],
    "sodt_wbf_candidates": [_P, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P],
    "sodt_wbf_fuse_workspace_bytes": [_I, _L, C.POINTER(C.c_size_t)],
    "sodt_wbf_fuse": [_P, _P, _P, _P, _P, _P, _I, _L, C.POINTER(C.c_double), _I, C.c_double, _F, _I, _I, _I, _P, C.c_size_t,
                      _P, _P, _P, _P, _P, _P],
    "sodt_eval_match_workspace_bytes": [_I, _L, _L, C.POINTER(C.c_size_t)],
    "sodt_eval_match": [_P, _P, _I, _L, _P, _L, _P, C.POINTER(C.c_float), _P, C.c_size_t, _P, _P, _P],
    "sodt_ap_per_class_workspace_bytes": [_L, _L, _I, C.POINTER(C.c_size_t)],
    "sodt_ap_per_class": [_P, _P, _P, _L, _P, _L, _I, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P],
    "sodt_confusion_update_workspace_bytes": [_I, _L, _L, C.POINTER(C.c_size_t)],
    "sodt_confusion_update": [_P, _P, _I, _L, _P, _L, _P, _I, _F, _F, _P, C.c_size_t, _P, _P, _P],
    "sodt_gemm_nt": [C.POINTER(GemmArgs), _I, _P],
    "sodt_gemm_tn": [C.POINTER(GemmTnArgs), _I, _P],
    "sodt_linear_bwd_sq": [C.POINTER(LinBwdArgs), _I, _P],
    "sodt_linear_bwd_wide": [C.POINTER(LinBwdArgs), _I, _P],
    "sodt_mlp_bwd": [_P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _L, _I, _I, _P, _L, _I, _P],
    "sodt_layernorm_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "sodt_layernorm_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "sodt_window_attn_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_window_attn_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_wmsa_pack_bytes": [_I, _I, _I, _I],
    "sodt_wmsa_pack": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "sodt_wmsa_block_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_window_attn_sp_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_window_attn_sp_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_window_attn_bwd_wm": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_wmsa_block_bwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_frontend_fwd": [_P, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_frontend_bwd_workspace_bytes": [_I, _I, _I],
    "sodt_frontend_bwd": [_P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _L, _I, _P],
    "sodt_patch_embed4_fwd": [_P, _P, _L, _P, _P, _P, _I, _I, _I, _P],
    "sodt_patch_embed4_bwd": [_P, _P, _L, _P, _P, _P, _I, _I, _I, _P],
    "sodt_cross_attn_ln_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "sodt_cross_attn_ln_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "sodt_bn_finalize": [_P, _P, _P, _P, _L, _I, _F, _F, _P],
    "sodt_bn_affine": [_P, _P, _P, _P, _P, _I, _P],
    "sodt_bn_silu_fwd": [_P, _P, _P, _P, _P, _I, _L, _I, _I, _P],
    "sodt_bn_silu_bwd_reduce": [_P, _I, _P, _P, _P, _P, _P, _L, _I, _I, _P],
    "sodt_bn_silu_bwd_apply": [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P],
    "sodt_bn_silu_bwd_apply_sync": [_P, _I, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L, _I, _I, _I, _P],
    "sodt_copy_rows": [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_gather_sum_rows": [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_detect_unpermute": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "sodt_detect_decode": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    # basics/models/model.py:155-184 (csrc/tta.hip)
    "sodt_tta_scale": [_P, _P, _I, _I, _I, _I, _I, C.POINTER(TtaPass), _I, _P],
    "sodt_detect_decode_tta": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _L, _L, _F, _I, _I, _I, _P],
    "sodt_detect_fwd": [C.POINTER(DetectArgs), _I, _P],
    "sodt_detect_bwd": [C.POINTER(DetectArgs), _I, _P],
    "sodt_prep_weights": [_P, _I, _I, _I, _P],
    "sodt_transpose_f32": [_P, _P, _I, _I, _I, _P],
    "sodt_cast": [_P, _P, _L, _I, _I, _P],
    "sodt_batch_sum": [_P, _P, _I, _L, _I, _P],
    "sodt_memset_zero": [_P, _L, _P],
    "sodt_gemm_set_variant": [_I],
    "sodt_maxpool5_fwd": [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P],
    "sodt_maxpool5_bwd": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_yolo_loss_workspace_bytes": [_L, _I, _I, C.POINTER(C.c_size_t)],
    "sodt_yolo_loss": [_P, _P, _I, _P, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _F, _P, C.c_size_t, _P, _P, _P],
    "sodt_yolo_loss_fl": [_P, _P, _I, _P, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _F, _F, _P, C.c_size_t, _P, _P, _P],
    "sodt_adam_ema_step": [_P, _P, _P, _P, _P, _P, _I, _P, _L, _I, C.POINTER(C.c_double), C.POINTER(C.c_double),
                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _I, _L, _F, _F, _P],
    "sodt_sgd_ema_step": [_P, _P, _P, _P, _P, _I, _P, _L, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                          _I, _F, _F, _P],
    "sodt_grad_stats": [_P, _P, _L, _P, _P, _F, _F, _I, _P, _P],
    "sodt_sgd_ema_step_ctl": [_P, _P, _P, _P, _P, _I, _P, _L, _I, C.POINTER(C.c_float), C.POINTER(C.c_float),
                              C.POINTER(C.c_float), _I, _P, _F, _P],
    "sodt_adam_ema_step_ctl": [_P, _P, _P, _P, _P, _P, _I, _P, _L, _I, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _I, _P, _F, _P],
    # basics/utils/sam.py (csrc/sam.hip); the 64-byte record goes down as a plain pointer (SAM_REC names its words)
    "sodt_sam_norm": [_P, _P, _P, _L, _I, _P, _P, _F, _P, _P],
    "sodt_sam_perturb": [_P, _P, _P, _P, _I, _P, _L, _I, C.POINTER(C.c_float), _P, _P, _P],
    "sodt_sam_restore": [_P, _P, _P, _L, _P],
    "sodt_preprocess_u8": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_preprocess_u8_ms": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "sodt_quad_u8": [_P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_ulonglong, _P],
    "sodt_preprocess_u8_quad": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.c_ulonglong, _P],
    "sodt_sr_l1_workspace_bytes": [_I, _I, _I, _I, C.POINTER(C.c_size_t)],
    "sodt_sr_l1_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P],
    "sodt_sr_l1_bwd": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "sodt_anchor_stats_workspace_bytes": [_L, _I, C.POINTER(C.c_size_t)],
    "sodt_anchor_stats": [_P, _L, _P, _I, _I, _F, _P, C.c_size_t, _P, _P],
    "sodt_anchor_evolve_workspace_bytes": [_L, C.POINTER(C.c_size_t)],
    "sodt_anchor_evolve": [_P, _L, _F, _P, _I, _P, _P, _I, _P, _P, C.c_size_t, _P],
    "sodt_kmeans_lloyd_workspace_bytes": [_L, _I, _I, C.POINTER(C.c_size_t)],
    "sodt_kmeans_lloyd": [_P, _L, _P, _P, _P, _P, _I, _I, C.c_double, _I, _P, C.c_size_t, _P],
    # Train.py:335-341 / general.py:220-244 (csrc/sampling.hip)
    "sodt_class_counts": [_P, _P, _L, _I, _I, _P, _P, _P, _P],
    "sodt_image_weights": [_P, _P, _I, _I, _P, _P],
    "sodt_weighted_choices_workspace_bytes": [_I, _I, C.POINTER(C.c_size_t)],
    "sodt_weighted_choices": [_P, _I, _P, _I, _P, _P, _P, _P, C.c_size_t, _P],
    "sodt_bilinear_up2_fwd": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "sodt_bilinear_up2_bwd": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_pixel_shuffle2": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "sodt_add_rows": [_P, _I, _I, _P, _I, _I, _L, _I, _I, _P],
    "sodt_nchw_f32_from_rows": [_P, _I, _P, _I, _I, _I, _I, _I, _P],
    "sodt_rows_from_nchw_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "sodt_convmlp_compose": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "sodt_convmlp_border_fix": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_convmlp_border_sums": [_P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_convmlp_decompose": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "sodt_mlp_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P],
    "sodt_col_stats": [_P, _I, _P, _L, _I, _I, _P],
    "sodt_conv3x3_c64n8_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_conv3x3_c64n8_dgrad": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_conv3x3_c64n8_wgrad": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "sodt_conv3x3_c64n8_wgrad_scratch_bytes": [],
    "sodt_conv3x3_c64_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P],
    "sodt_conv3x3_c64_wgrad": [_P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P],
    "sodt_conv3x3_c64_wgrad_scratch_bytes": [],
    "sodt_debug_wmsa_stamps": [_P, _I],
    "sodt_debug_wmsa_hg_stamps": [_P, _I],
    "sodt_version": [],
}
RESTYPES = {
    "sodt_version": C.c_char_p,
    "sodt_wmsa_pack_bytes": _L,
    "sodt_frontend_bwd_workspace_bytes": _L,
    "sodt_conv3x3_c64n8_wgrad_scratch_bytes": _L,
    "sodt_conv3x3_c64_wgrad_scratch_bytes": _L,
}

_lib = None


def load():
    """Load the library (once).  Raises if it is absent: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python small-object-detection-transformers_amd/build.py` "
            "(hipcc --offload-arch=gfx950). The MI355X path has no fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = RESTYPES.get(name, C.c_int)
    _lib = lib
    return lib


def exported_symbols():
    return list(SIGNATURES)
