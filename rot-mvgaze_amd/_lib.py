"""ctypes binding of librotmvgaze_hip.so (the C ABI declared in include/rotmvgaze.h).

There is no fallback: if the library is missing or fails to load, ``lib()`` raises.  Build it with
``python rot-mvgaze_amd/csrc/build.py`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librotmvgaze_hip.so")

K_FAMILIES = 18
ABI_VERSION = 13
SESSION_FP32, SESSION_BF16 = 0, 1         # MVG_SESSION_FP32 / MVG_SESSION_BF16 (mvg_session_create_ex)
ADAM_MAX_SEGMENTS = 16                    # MVG_ADAM_MAX_SEGMENTS: segments per launch of mvg_adam_step_segments
# MVG_GAZE_ERR_*: the fields of one cell of mvg_gaze_error_update's record (doubles)
GAZE_ERR_COUNT, GAZE_ERR_SUM, GAZE_ERR_SUMSQ, GAZE_ERR_MAX, GAZE_ERR_NONFINITE, GAZE_ERR_FIELDS = range(6)


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("groups", "n", "h", "w", "cin", "cout", "r", "s", "stride", "pad", "ho", "wo")]

    @classmethod
    def make(cls, groups, n, h, w, cin, cout, k, stride, pad):
        ho = (h + 2 * pad - k) // stride + 1
        wo = (w + 2 * pad - k) // stride + 1
        return cls(groups, n, h, w, cin, cout, k, k, stride, pad, ho, wo)

    @classmethod
    def linear(cls, rows, fin, fout):
        return cls(1, rows, 1, 1, fin, fout, 1, 1, 1, 0, 1, 1)


PLAN_FPROP, PLAN_FPROP_STATS, PLAN_DGRAD, PLAN_FUSER_FPROP = 0, 1, 2, 3       # MVG_PLAN_* (mvg_conv_plan_query)
PLAN_BF16_FPROP, PLAN_BF16_DGRAD, PLAN_BF16_DGRAD_BNREDUCE, PLAN_BF16_AFFINE, PLAN_BF16_LINEAR_FPROP_MIXED, \
    PLAN_BF16_LINEAR_DGRAD_MIXED = range(6)                                   # MVG_PLAN_BF16_* (mvg_conv_plan_query_bf16)


class ConvPlan(C.Structure):
    """mvg_conv_plan (include/rotmvgaze.h)."""
    _fields_ = [("bm", C.c_int32), ("bn", C.c_int32), ("bk", C.c_int32), ("fasta", C.c_int32), ("ncls", C.c_int32),
                ("cls_tiles", C.c_int32 * 4), ("cls_kt", C.c_int32 * 4), ("streamk_grid", C.c_int32), ("splitk", C.c_int32),
                ("scratch_floats", C.c_int64)]


BN_PASS_APPLY, BN_PASS_BWD_APPLY, BN_PASS_BWD_REDUCE, BN_PASS_EVAL_BWD, BN_PASS_POOL_BWD_REDUCE, BN_PASS_POOL_EVAL_BWD, \
    BN_PASS_FINALIZE = range(7)                                             # MVG_BN_PASS_* (mvg_bn_plan_query)
BN_ELEM_FP32, BN_ELEM_BF16, BN_ELEM_SP = 0, 1, 2                            # MVG_BN_ELEM_*
BN_MERGE_WALK_GROUPS, BN_MERGE_ALL_GROUPS, BN_MERGE_PER_GROUP = 0, 1, 2     # MVG_BN_MERGE_*


class BnPlan(C.Structure):
    """mvg_bn_plan (include/rotmvgaze.h)."""
    _fields_ = [("accesses_per_group", C.c_int64), ("grid_x", C.c_int32), ("trips", C.c_int32), ("step", C.c_int32),
                ("cwn", C.c_int32), ("cw", C.c_int32), ("column_blocks", C.c_int32), ("row_lanes", C.c_int32), ("chunks", C.c_int32),
                ("empty_chunks", C.c_int32), ("rows_per_chunk", C.c_int64), ("workspace_floats", C.c_int64), ("form", C.c_int32),
                ("lanes_per_group", C.c_int32), ("slices", C.c_int32), ("partials_per_slice", C.c_int32), ("scratch_floats", C.c_int64)]


class ProfEntry(C.Structure):
    _fields_ = [("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class SessionCfg(C.Structure):
    """mvg_session_cfg (include/rotmvgaze.h)."""
    _fields_ = [(n, C.c_int32) for n in
                ("depth", "num_iter", "views", "batch", "height", "width", "share_weights", "ignore_rotmat", "split", "raw_u8",
                 "in_h", "in_w", "input_bgr")]


_P = C.c_void_p
_I = C.c_int
_I64 = C.c_int64
_F = C.c_float
_D = C.POINTER(ConvDesc)

# name -> (restype, argtypes); must list every function include/rotmvgaze.h declares
SIGNATURES = {
    "mvg_abi_version": (_I, []),
    "mvg_last_error": (C.c_char_p, []),
    "mvg_device_cus": (_I, []),
    "mvg_set_scratch": (_I, [_P, C.c_size_t, _P]),
    "mvg_scratch_bytes": (C.c_size_t, []),
    "mvg_set_reserved_cus": (_I, [_I]),
    "mvg_stream_create_low_priority": (_P, []),
    "mvg_prof_enable": (_I, [_I]),
    "mvg_prof_reset": (_I, []),
    "mvg_prof_collect": (_I, [C.POINTER(ProfEntry)]),
    "mvg_prof_family_name": (C.c_char_p, [_I]),
    "mvg_conv_fprop": (_I, [_D, _P, _P, _P, _P, _I, _P, _P]),
    "mvg_conv_fprop_affine": (_I, [_D, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mvg_conv_stats_partials": (_I, [_D, C.POINTER(C.c_int32)]),
    "mvg_conv_dgrad": (_I, [_D, _P, _P, _P, _P, _P, _P]),
    "mvg_conv_wgrad": (_I, [_D, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_conv_wgrad_splits": (_I, [_D]),
    "mvg_conv_plan_query": (_I, [_D, _I, C.c_size_t, C.POINTER(ConvPlan)]),
    "mvg_bn_plan_query": (_I, [_I, _I, _I, _I64, _I, _I, _I, _I, _I, C.c_size_t, C.POINTER(BnPlan)]),
    "mvg_conv_wgrad_tile": (_I, [_D, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mvg_linear_wgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P]),
    "mvg_fuser_fprop": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P]),
    "mvg_fuser_wgrad": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "mvg_linear_workspace_floats": (C.c_size_t, [_I, _I, _I]),
    "mvg_linear_fprop": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _P, C.c_size_t, _P]),
    "mvg_linear_dgrad": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, C.c_size_t, _P]),
    "mvg_bn_finalize": (_I, [_P, _I, _I, _I, _I64, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P]),
    "mvg_bn_eval_affine": (_I, [_I, _I, _P, _P, _P, _P, _F, _P, _P, _P]),
    "mvg_bn_eval_affine_batch": (_I, [_P, _I, _I, _F, _P]),
    "mvg_bn_apply": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _I, _I64, _I, _P]),
    "mvg_bn_bwd_reduce": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "mvg_split_f32": (_I, [_P, _P, _I64, _F, _P]),
    "mvg_merge_sp": (_I, [_P, _P, _I64, _F, _P]),
    "mvg_split_weights": (_I, [_D, _P, _P, _P, _P, _P, _P]),
    "mvg_weights_prep_batch": (_I, [_P, _I, _I, _I, _P]),
    "mvg_conv_stats_partials_split": (_I, [_D, C.POINTER(C.c_int32)]),
    "mvg_conv_fprop_split": (_I, [_D, _P, _P, _P, _P, _P, _P, _P]),
    "mvg_conv_fprop_split_affine": (_I, [_D, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P]),
    "mvg_conv_dgrad_split": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mvg_bn_apply_split": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _I, _I64, _I, _P]),
    "mvg_bn_bwd_apply_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P, _I, _P]),
    "mvg_bn_bwd_reduce_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "mvg_bn_relu_maxpool_fwd_split": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mvg_avgpool_fwd_split": (_I, [_P, _P, _I, _I, _I, _P]),
    # per-tensor scales of the backbone's sp activations (training steps)
    "mvg_act_scales": (_I, [_P, _I, _P, _I, _P]),
    "mvg_bn_apply_split_scaled": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _I64, _I, _P]),
    "mvg_bn_relu_maxpool_fwd_split_scaled": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mvg_avgpool_fwd_split_scaled": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    # frozen-BatchNorm training steps on the split kernels (Backbone.split_frozen)
    "mvg_bn_frozen_finalize": (_I, [_P, _I, _I, _I, _I64, _I, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mvg_bn_frozen_bwd_apply_split": (_I, [_P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P]),
    "mvg_conv_wgrad_split_xs":(_I, [_D, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_conv_wgrad_split_slabs_xs": (_I, [_D, _P, _P, _P, _P, _P, _I, _P]),
    "mvg_stem_rowwindow_split": (_I, [_P, _P, _I64, _I, _I, _P]),
    "mvg_stem_rowwindow_split_nchw": (_I, [_P, _P, _I64, _I, _I, _P]),
    "mvg_stem_fprop_split": (_I, [_D, _P, _P, _P, _P, _P, _P]),
    "mvg_stem_wgrad_splits_split": (_I, [_D]),
    "mvg_stem_wgrad_split": (_I, [_D, _P, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_stem_plan_query_split": (_I, [_D] + [C.POINTER(C.c_int32)] * 6),
    "mvg_bn_relu_maxpool_bwd_reduce_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "mvg_bn_relu_maxpool_bwd_apply_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "mvg_conv_dgrad_bn_partials_split": (_I, [_D]),
    "mvg_conv_dgrad_split_bnreduce": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mvg_conv_dgrad_split_bnapply_bnreduce": (_I, [_D] + [_P] * 9 + [_I64] + [_P] * 15 + [_I, _P, _P, _P, _P]),
    "mvg_conv_fprop_split_stages": (_I, [_D]),
    "mvg_conv_dgrad_split_stages": (_I, [_D, _I]),
    "mvg_conv_fprop_split_bnapply": (_I, [_D] + [_P] * 6 + [_I] + [_P] * 9),
    "mvg_conv_wgrad_splits_split": (_I, [_D]),
    "mvg_conv_wgrad_split_tile": (_I, [_D, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mvg_conv_wgrad_split": (_I, [_D, _P, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_conv_wgrad_split_slabs": (_I, [_D, _P, _P, _P, _P, _I, _P]),
    "mvg_wgrad_reduce_batch": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), _I, _P]),
    "mvg_bn_apply_bits": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P]),
    "mvg_bn_bwd_reduce_bits": (_I, [_P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "mvg_bn_apply_bits_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P]),
    "mvg_bn_bwd_reduce_bits_bf16": (_I, [_P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "mvg_bn_bwd_workspace_floats": (C.c_size_t, [_I, _I64, _I]),
    "mvg_bn_bwd_apply": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P]),
    "mvg_maxpool3x3s2_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mvg_maxpool3x3s2_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mvg_bn_relu_maxpool_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mvg_bn_relu_maxpool_bwd_reduce": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P,
                                            _P]),
    "mvg_bn_relu_maxpool_bwd_apply": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    # eval mode (running statistics): one-pass BatchNorm backward, and its stem-tail form
    "mvg_bn_eval_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P]),
    "mvg_bn_eval_bwd_workspace_floats": (C.c_size_t, [_I, _I64, _I]),
    "mvg_bn_relu_maxpool_eval_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P,
                                          _P]),
    "mvg_avgpool_fwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "mvg_avgpool_bwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "mvg_nchw_to_nhwc4": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "mvg_nhwc4_to_nchw": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "mvg_preprocess_u8hwc": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mvg_gaze_lp_loss": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "mvg_preprocess_u8hwc_resize": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mvg_multi_erase_nchw": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "mvg_augment_u8hwc": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mvg_augment_u8hwc_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    # the device draws of TrainAugment(draws="device"): cfg is a host mvg_augment_draw_cfg (augment.DRAW_CFG_DTYPE)
    "mvg_augment_draw": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, C.c_uint64, _P, _P]),
    "mvg_rotation_matrix_2d": (_I, [_P, _P, _I, _I, _P]),
    "mvg_relative_rotation": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "mvg_rotcat_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mvg_rotcat_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mvg_rotcat_ext_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "mvg_rotcat_ext_bwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mvg_ibn_scales": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _P, _I, _I, _I, _P]),
    "mvg_paircat_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "mvg_paircat_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "mvg_segment_sum": (_I, [_P, _I64, _I, _P, _P, _I, _I, _I, _I, _P]),
    "mvg_axpby": (_I, [_P, _P, _F, _F, _I64, _P]),
    "mvg_scale_by": (_I, [_P, _P, _P, _I64, _P]),
    "mvg_linear_skinny_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "mvg_linear_skinny_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "mvg_adam_step": (_I, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I, _P]),
    "mvg_gaze_angular_loss": (_I, [_P, _P, _I, _F, _P, _I, _P, _P, _P]),
    "mvg_gaze_angular_loss_multi": (_I, [_P, _P, _I, _I, _I, C.POINTER(C.c_float), _P, _P, _P]),
    "mvg_adam_step_dev": (_I, [_P, _P, _P, _P, _I64, _P, _P, _F, _F, _F, _F, _P]),
    "mvg_adam_step_segments": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32), _I, _P]),
    "mvg_adam_step_segments_dev": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32), _I, _P, _I, _P,
                                        _P]),
    "mvg_grad_norm_workspace_bytes": (_I64, [_I]),
    "mvg_grad_norm_segments": (_I, [_P, _I64, C.POINTER(C.c_int64), _I, _F, _I, _P, _I64, _P, _P]),
    "mvg_adam_step_segments_clip": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32), _I, _P,
                                         _P]),
    "mvg_adam_step_segments_dev_clip": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32), _I, _P,
                                             _I, _P, _P, _P]),
    # decoupled weight decay (AdamW): the two plain forms, and the segmented forms with a mode per segment
    "mvg_adamw_step": (_I, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I, _P]),
    "mvg_adamw_step_dev": (_I, [_P, _P, _P, _P, _I64, _P, _P, _F, _F, _F, _F, _P]),
    "mvg_adam_step_segments_ex": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), _I, _P, _P]),
    "mvg_adam_step_segments_dev_ex": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), _I, _P, _I, _P, _P, _P]),
    # the fusion block on the split kernels
    "mvg_absmax_multi": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), _I, _P]),
    "mvg_fuse_build_split": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "mvg_fuse_unbuild": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "mvg_linear_fprop_split": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "mvg_linear_dgrad_split": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mvg_linear_wgrad_split": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_split_colsum": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "mvg_linear_plan_query_split": (_I, [_I, _I, _I, _I] + [C.POINTER(C.c_int32)] * 3),
    # bf16 storage path (same argument lists as the fp32 entry points)
    "mvg_cast_weights_bf16": (_I, [_D, _P, _I, _P, _P, _P]),
    "mvg_conv_fprop_bf16": (_I, [_D, _P, _P, _P, _P, _I, _P, _P]),
    "mvg_conv_stats_partials_bf16": (_I, [_D, C.POINTER(C.c_int32)]),
    "mvg_conv_fprop_bf16_affine": (_I, [_D, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mvg_conv_dgrad_bf16": (_I, [_D, _P, _P, _P, _P, _P, _P]),
    "mvg_conv_dgrad_bn_partials_bf16": (_I, [_D]),
    "mvg_conv_dgrad_bf16_bnreduce": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mvg_conv_wgrad_bf16": (_I, [_D, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_stem_rowwindow_bf16": (_I, [_P, _P, _I64, _I, _I, _P]),
    "mvg_stem_fprop_bf16": (_I, [_D, _P, _P, _P, _P, _P]),
    "mvg_stem_wgrad_splits_bf16": (_I, [_D]),
    "mvg_stem_wgrad_bf16": (_I, [_D, _P, _P, _P, _P, _I, _I, _P]),
    "mvg_conv_wgrad_splits_bf16": (_I, [_D]),
    "mvg_conv_wgrad_bf16_slabs": (_I, [_D, _P, _P, _P, _I, _P]),
    "mvg_conv_plan_query_bf16": (_I, [_D, _I, C.POINTER(ConvPlan)]),
    "mvg_conv_wgrad_tile_bf16": (_I, [_D, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mvg_stem_plan_query_bf16": (_I, [_D, C.POINTER(ConvPlan), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mvg_linear_fprop_mixed": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "mvg_linear_dgrad_mixed": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "mvg_linear_wgrad_mixed": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P]),
    "mvg_bn_apply_bf16": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _I, _I64, _I, _P]),
    "mvg_bn_bwd_reduce_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "mvg_bn_bwd_apply_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _P]),
    "mvg_bn_relu_maxpool_fwd_bf16": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mvg_bn_relu_maxpool_bwd_reduce_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I,
                                                 _P, _P]),
    "mvg_bn_relu_maxpool_bwd_apply_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    # frozen BatchNorm on the bf16 path: the one-pass backward on the running statistics in bf16 storage
    "mvg_bn_eval_bwd_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _I64, _I, _P, _P, _P, _P, _I, _P, _P]),
    "mvg_bn_relu_maxpool_eval_bwd_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I,
                                               _P, _P]),
    "mvg_avgpool_fwd_bf16": (_I, [_P, _P, _I, _I, _I, _P]),
    "mvg_avgpool_bwd_bf16": (_I, [_P, _P, _I, _I, _I, _P]),
    "mvg_nchw_to_nhwc8_bf16": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "mvg_preprocess_u8hwc_resize_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mvg_mt19937_seed": (_I, [_P, C.c_uint64]),
    "mvg_pair_index_build": (_I64, [_P, _P, _I, _I, _P, _I64]),
    # inference session: one call queues the whole eval-mode forward (session.py)
    "mvg_session_create": (_I, [C.POINTER(SessionCfg), C.POINTER(_P)]),
    "mvg_session_destroy": (None, [_P]),
    "mvg_session_num_tensors": (_I, [_P]),
    "mvg_session_tensor_name": (C.c_char_p, [_P, _I]),
    "mvg_session_tensor_numel": (_I64, [_P, _I]),
    "mvg_session_workspace_bytes": (C.c_size_t, [_P]),
    "mvg_session_launches": (_I, [_P]),
    "mvg_session_bind": (_I, [_P, C.POINTER(_P), _P, C.c_size_t, _P]),
    "mvg_session_forward": (_I, [_P, C.POINTER(_P), _P, _P, _P, _P, _P, _P]),
    # activation range record of the guarded inference forward (Backbone.split_eval_guard, InferenceSession(range_record=True))
    "mvg_conv_fprop_split_affine_ranged": (_I, [_D, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P]),
    "mvg_split_f32_ranged": (_I, [_P, _P, _I64, _F, _P, _P]),
    "mvg_session_num_range_units": (_I, [_P]),
    "mvg_session_range_unit_name": (C.c_char_p, [_P, _I]),
    "mvg_session_set_range_record": (_I, [_P, _P]),
    # the session's compute forms (fp32 | bf16) and its step list
    "mvg_session_create_ex": (_I, [C.POINTER(SessionCfg), C.c_int32, C.POINTER(_P)]),
    "mvg_session_compute": (_I, [_P]),
    "mvg_session_num_steps": (_I, [_P]),
    "mvg_session_step_name": (C.c_char_p, [_P, _I]),
    # gaze error meter (metrics.AngularErrorMeter): float64 angular error accumulated on the device, and its session hook
    "mvg_gaze_error_update": (_I, [_P, _P, _I, _I, _I, _P, _P, _I64, _P]),
    "mvg_session_set_error_record": (_I, [_P, _P, _P, _P, _I64]),
    # multi-view consensus gaze (consensus.gaze_consensus): one estimate per sample from all directed pairs, and its session hook
    "mvg_gaze_consensus_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "mvg_gaze_consensus_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "mvg_session_set_consensus": (_I, [_P, _P, _P, _P, _P]),
}

_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the library; raise if it is not there - no CPU fallback exists."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is required (python rot-mvgaze_amd/csrc/build.py); "
            "this package has no CPU fallback")
    try:
        l = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"failed to load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)           # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if l.mvg_abi_version() != ABI_VERSION:
        raise RuntimeError(f"librotmvgaze_hip.so ABI {l.mvg_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = l
    return l


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mvg_last_error()
        raise RuntimeError(f"librotmvgaze_hip {what} failed (rc={rc}): {msg.decode() if msg else '?'}")
