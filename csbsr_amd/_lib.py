"""ctypes binding of libcsbsr_hip.so (the C ABI declared in include/csbsr_hip.h).

The product path has NO fallback: if the shared library is missing or a kernel reports an error this
module raises.  PyTorch-ROCm is used only for device memory (tensors) and streams; every pointer that
crosses this boundary is a raw ``data_ptr()``.
"""
import ctypes as C
import os
from collections import namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSBSR_LIB") or os.path.join(_HERE, "libcsbsr_hip.so")       # CSBSR_LIB: a variant build (kernel A/B experiments)

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_PRELU, ACT_SIGMOID = 0, 1, 2, 3, 4
RES_NONE, RES_ADD, RES_SUB, RES_MUL, RES_FMA = 0, 1, 2, 3, 4
STAT_NONE, STAT_BN, STAT_SAMPLE_SUM = 0, 1, 2

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class Seg(C.Structure):
    _fields_ = [("ptr", vp), ("sn", i64), ("sy", i64), ("sx", i64), ("c", i32), ("creal", i32)]


class ConvDesc(C.Structure):
    _fields_ = [("inp", Seg * 2), ("N", i32), ("H", i32), ("W", i32), ("OH", i32), ("OW", i32),
                ("transposed", i32), ("KH", i32), ("KW", i32), ("stride", i32), ("pad", i32), ("dil", i32),
                ("wt", vp), ("cout", i32), ("coutp", i32),
                ("out16", vp), ("o_sn", i64), ("o_sy", i64), ("o_sx", i64),
                ("out32", vp), ("o32_sn", i64), ("o32_sy", i64), ("o32_sx", i64), ("o32_sc", i64),
                ("bias", vp), ("cbias", vp), ("act", i32), ("act_slope", f32), ("prelu", vp),
                ("res_mode", i32), ("res", vp), ("r_sn", i64), ("r_sy", i64), ("r_sx", i64),
                ("res2", vp), ("r2_sn", i64), ("r2_sy", i64), ("r2_sx", i64),
                ("accumulate", i32), ("stat_mode", i32), ("stat", vp), ("out_scale", f32),
                ("o_lo", i64), ("r_lo", i64), ("r2_lo", i64),
                ("mask", vp), ("m_sn", i64), ("m_sy", i64), ("m_sx", i64), ("mask_slope", f32), ("cbias_mode", i32),
                ("mask_prelu", vp), ("dact_bias", vp), ("dact_prelu", vp),
                ("dres", vp), ("dr_sn", i64), ("dr_sy", i64), ("dr_sx", i64),
                ("split_fused", i32), ("_pad_sf", i32), ("bias_sn", i64)]


class WgradDesc(C.Structure):
    _fields_ = [("a", vp), ("a_sn", i64), ("a_sy", i64), ("a_sx", i64), ("ca", i32), ("ca_real", i32),
                ("b", Seg * 2), ("N", i32), ("AH", i32), ("AW", i32), ("BH", i32), ("BW", i32),
                ("KH", i32), ("KW", i32), ("stride", i32), ("pad", i32), ("dil", i32),
                ("g", vp), ("splits", i32), ("_pad1", i32)]


class EpiBwdDesc(C.Structure):
    _fields_ = [("npix", i64), ("c", i32), ("creal", i32),
                ("dout", vp), ("dout_ld", i64), ("out", vp), ("out_ld", i64),
                ("res", vp), ("res_ld", i64), ("res2", vp), ("res2_ld", i64),
                ("act", i32), ("act_slope", f32), ("prelu", vp), ("res_mode", i32), ("_pad", i32),
                ("dpre", vp), ("dpre_ld", i64),
                ("dres", vp), ("dres_ld", i64), ("dres_accumulate", i32), ("_pad1", i32),
                ("dres2", vp), ("dres2_ld", i64), ("dres2_accumulate", i32), ("_pad2", i32),
                ("dbias", vp), ("dprelu", vp)]


class BnDesc(C.Structure):
    _fields_ = [("npix", i64), ("hw", i64), ("c", i32), ("creal", i32),
                ("x", vp), ("x_ld", i64), ("mean", vp), ("invstd", vp), ("gamma", vp), ("beta", vp),
                ("res", vp), ("res_ld", i64), ("act", i32), ("_pad", i32), ("prelu", vp), ("drop", vp),
                ("y", vp), ("y_ld", i64), ("dy", vp), ("dy_ld", i64), ("red", vp), ("dprelu", vp),
                ("dx", vp), ("dx_ld", i64), ("dres", vp), ("dres_ld", i64), ("dres_accumulate", i32), ("_pad1", i32),
                ("dgamma", vp), ("dbeta", vp), ("x_lo", i64), ("res_lo", i64), ("y_lo", i64)]


# name -> (restype, argtypes): every symbol include/csbsr_hip.h declares
SIGNATURES = {
    "csbsr_version": (i32, []),
    "csbsr_last_error": (C.c_char_p, []),
    "csbsr_conv_forward": (i32, [C.POINTER(ConvDesc), vp]),
    "csbsr_conv_wgrad": (i32, [C.POINTER(WgradDesc), vp]),
    "csbsr_conv_hr_eligible": (i32, [C.POINTER(ConvDesc)]),
    "csbsr_conv_hr_forward": (i32, [C.POINTER(ConvDesc), vp]),
    "csbsr_conv_x3_eligible": (i32, [C.POINTER(ConvDesc)]),
    "csbsr_conv_x3_forward": (i32, [C.POINTER(ConvDesc), vp]),
    "csbsr_packed_weight_elems_x3": (i64, [i32, i32]),
    "csbsr_pack_weights_x3": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_conv_x3n_eligible": (i32, [C.POINTER(ConvDesc)]),
    "csbsr_conv_x3n_forward": (i32, [C.POINTER(ConvDesc), vp]),
    "csbsr_packed_weight_elems_x3n": (i64, [i32, i32]),
    "csbsr_pack_weights_x3n": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.c_float, vp]),
    "csbsr_conv_x3w_eligible": (i32, [C.POINTER(ConvDesc)]),
    "csbsr_conv_x3w_forward": (i32, [C.POINTER(ConvDesc), vp]),
    "csbsr_packed_weight_elems_x3w": (i64, [i32, i32]),
    "csbsr_pack_weights_x3w": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_packed_weight_elems_x3_strided": (i64, [i32, i32, i32]),
    "csbsr_pack_weights_x3_strided": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_conv_tp_eligible": (i32, [C.POINTER(ConvDesc)]),
    "csbsr_conv_tp_forward": (i32, [C.POINTER(ConvDesc), vp]),
    "csbsr_packed_weight_elems_tp": (i64, [i32, i32]),
    "csbsr_pack_weights_tp": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_packed_weight_elems_hr": (i64, [i32, i32, i32]),
    "csbsr_pack_weights_hr": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_packed_weight_elems": (i64, [i32] * 9),
    "csbsr_pack_weights": (i32, [vp, vp] + [i32] * 12 + [vp]),
    "csbsr_packed_weight_elems_split": (i64, [i32] * 9),
    "csbsr_pack_weights_split": (i32, [vp, vp] + [i32] * 11 + [f32, i32, vp]),
    "csbsr_axpby_split": (i32, [i64, i32, vp, i64, i64, f32, vp, i64, i64, f32, vp, i64, i64, vp]),
    "csbsr_nchw32_to_nhwc16_split": (i32, [vp, vp, i32, i32, i32, i32, i32, i64, i64, vp, vp, vp]),
    "csbsr_maxpool3x3s2_fwd_split": (i32, [vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, vp]),
    "csbsr_maxpool3x3s2_bwd_split": (i32, [vp, i64, i64, vp, i64, i64, vp, vp, i32, i32, i32, i32, vp]),
    "csbsr_adaptive_avgpool_fwd_split": (i32, [vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_sum_act_split": (i32, [i64, i32, i32, vp, vp, vp, vp, i64, i64, i32, vp]),
    "csbsr_weighted_pool_fwd_split": (i32, [vp, i64, i64, vp, vp, i32, i64, i32, vp]),
    "csbsr_bilinear_fwd_split": (i32, [vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "csbsr_unpack_wgrad": (i32, [vp, vp] + [i32] * 9 + [f32, i32, i32, vp]),
    "csbsr_wgrad_splits": (i32, [i32, i32, i64]),
    "csbsr_wgrad_splits_desc": (i32, [vp]),
    "csbsr_epilogue_backward": (i32, [C.POINTER(EpiBwdDesc), vp]),
    "csbsr_set_reduction_scratch": (i32, [vp, i64]),
    "csbsr_axpby": (i32, [i64, i32, vp, i64, f32, vp, i64, f32, vp, i64, vp]),
    "csbsr_fill_f16": (i32, [vp, i64, i32, i64, f32, vp]),
    "csbsr_sum_act": (i32, [i64, i32, i32, vp, vp, vp, i64, i32, vp]),
    "csbsr_weighted_pool_fwd": (i32, [vp, i64, vp, vp, i32, i64, i32, vp]),
    "csbsr_weighted_pool_bwd": (i32, [vp, i64, vp, vp, vp, i64, vp, i32, i64, i32, vp]),
    "csbsr_nchw32_to_nhwc16": (i32, [vp, vp, i32, i32, i32, i32, i32, i64, vp, vp, vp]),
    "csbsr_nhwc16_to_nchw32": (i32, [vp, i64, vp, i32, i32, i32, i32, f32, f32, vp]),
    "csbsr_plane_reduce": (i32, [vp, vp, i32, i64, vp, vp]),
    "csbsr_channel_mean_sub": (i32, [vp, i64, i64, i64, i32, i32, i32, i32, i32, vp, vp]),
    "csbsr_thin_tp_backward_slabs": (i32, [i32, i32]),
    "csbsr_conv_thin_dact_eligible": (i32, [vp]),
    "csbsr_conv_split_fused_eligible": (i32, [C.POINTER(ConvDesc)]),
    "csbsr_thin_tp_backward": (i32, [vp, i64, i64, i64, vp, i64, i64, i64, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, i64, i64, i64, vp, vp, vp]),
    "csbsr_conv_pair1x1_slabs": (i32, [i32, i32, i32, vp]),
    "csbsr_conv_pair1x1_backward": (i32, [vp, i64, i64, i64, vp, i64, i64, i64, vp, f32, i32, i32, i32, vp, i64, i64, i64, vp, vp]),
    "csbsr_round_weights": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "csbsr_dc_bias": (i32, [vp, i32, i32, vp, i64, i32, vp, i64, i32, vp, i32, vp, vp]),
    "csbsr_instnorm_bwd": (i32, [vp, i64, vp, vp, vp, vp, i32, i32, i32, i64, vp, vp]),
    "csbsr_border_class_fill": (i32, [vp, vp, i64, i32, i32, i32, i32, vp]),
    "csbsr_border_class_fill_masked": (i32, [vp, vp, i64, vp, i64, C.c_float, i32, i32, i32, i32, vp]),
    "csbsr_border_class_sums": (i32, [vp, i64, vp, i32, i32, i32, i32, vp]),
    "csbsr_border_class_fill_masked_sums": (i32, [vp, vp, i64, vp, i64, C.c_float, vp, i32, i32, i32, i32, vp]),
    "csbsr_border_class_sums_prelu": (i32, [vp, i64, vp, i64, vp, vp, i32, i32, i32, i32, vp]),
    "csbsr_ring_class_sums": (i32, [vp, i64, vp, i32, i32, i32, i32, vp]),
    "csbsr_bn_finalize": (i32, [vp, i64, i32, i32, f32, f32, vp, vp, vp, vp, vp]),
    "csbsr_bn_apply": (i32, [C.POINTER(BnDesc), vp]),
    "csbsr_bn_backward": (i32, [C.POINTER(BnDesc), vp]),
    "csbsr_maxpool3x3s2_fwd": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "csbsr_maxpool3x3s2_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "csbsr_adaptive_avgpool_fwd": (i32, [vp, i64, vp, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_adaptive_avgpool_bwd": (i32, [vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_bilinear_fwd": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "csbsr_bilinear_bwd": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "csbsr_bilinear32_fwd": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_bilinear32_bwd": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_bicubic_up_add": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "csbsr_aa_bicubic_up": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_aa_bicubic_down_fwd": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "csbsr_aa_bicubic_down_bwd": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_area_down_fwd": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "csbsr_area_down_bwd": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "csbsr_blur_fwd": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]),
    "csbsr_blur_bwd_input": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_blur_bwd_kernel": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "csbsr_sdf": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "csbsr_crack_weight": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp]),
    "csbsr_segloss_reduce": (i32, [vp, vp, vp, i32, i64, vp, f32, f32, vp]),
    "csbsr_segloss_finish": (i32, [vp, vp, vp, i32, i64, vp, f32, f32, f32, f32, f32, f32, vp, vp, vp, i32, vp]),
    "csbsr_l1_fwd_bwd": (i32, [vp, vp, vp, i32, i32, i64, vp, f32, vp, vp, i32, vp]),
    "csbsr_sigmoid_bwd_to_nhwc8": (i32, [vp, vp, vp, i64, f32, vp]),
    "csbsr_gaussian_kernels": (i32, [vp, vp, i32, i32, vp]),
    "csbsr_gather_crop_u8": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, vp, vp]),
    "csbsr_gather_resize_u8": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp]),
    "csbsr_stitch_clip_u8": (i32,[vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "csbsr_stitch_tiles_u8": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp]),
    "csbsr_threshold_planes_u8": (i32, [vp, vp, i32, i64, i32, vp, vp]),
    "csbsr_iou_sweep": (i32, [vp, vp, vp, i32, i64, i32, f32, vp, vp, vp, vp, vp]),
    "csbsr_psnr_ssim": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "csbsr_surface_prepare": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "csbsr_surface_gather": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp]),
    "csbsr_pr_sweep": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "csbsr_skeleton_max_passes": (i32, []),
    "csbsr_skeleton_init": (i32, [vp, f32, i32, i32, i32, vp, vp]),
    "csbsr_skeleton_passes": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "csbsr_skeleton_finish": (i32, [vp, i32, i32, i32, vp, vp]),
    "csbsr_centerline_counts": (i32, [vp, vp, f32, vp, vp, i32, i32, i32, vp, vp]),
    "csbsr_ccl_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "csbsr_ccl_label": (i32, [vp, f32, i32, i32, i32, i32, vp, vp, vp]),
    "csbsr_component_sums": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "csbsr_component_keep": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "csbsr_width_max_radius": (i32, []),
    "csbsr_width_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "csbsr_skeleton_width": (i32, [vp, f32, vp, i32, i32, i32, i32, vp, vp, vp]),
    "csbsr_component_width": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "csbsr_skeleton_topology": (i32, [vp, i32, i32, i32, vp, vp, vp]),
    "csbsr_component_topology": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "csbsr_branch_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "csbsr_branch_label": (i32, [vp, i32, i32, i32, vp, vp, vp]),
    "csbsr_branch_sums": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "csbsr_branch_count": (i32, [vp, i32, i32, i32, vp, vp]),
    "csbsr_branch_order_work_bytes": (i64, [i32]),
    "csbsr_branch_order_rounds": (i32, [i32]),
    "csbsr_branch_order": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "csbsr_branch_scatter": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "csbsr_simplify_max_tol_q": (i32, []),
    "csbsr_simplify_route_limits": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "csbsr_polyline_simplify_work_bytes": (i64, [i32, i32]),
    "csbsr_polyline_simplify": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "csbsr_gap_max_radius": (i32, []),
    "csbsr_endpoint_gaps": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "csbsr_gap_groups": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "csbsr_gap_draw": (i32, [vp, i32, i32, i32, vp, vp]),
    "csbsr_prune_max_spur": (i32, []),
    "csbsr_prune_steps": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "csbsr_prune_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "csbsr_prune_work_bytes": (i64, [i32, i32, i32]),
    "csbsr_skeleton_prune": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "csbsr_head1_fwd":(i32, [vp, i64, i64, i32, vp, vp, i32, vp, i64, vp]),
    "csbsr_head1_bwd_input": (i32, [vp, i64, vp, i32, vp, i64, i64, vp]),
    "csbsr_adam_step": (i32, [vp, vp, vp, i32, C.c_double, C.c_double, C.c_float, vp]),
    "csbsr_sgd_step": (i32, [vp, vp, vp, i32, C.c_double, C.c_double, C.c_double, vp]),
    "csbsr_fingerprint": (i32, [vp, vp, vp, i32, vp, vp]),
}

# private hooks (csbsr_amd/csrc/csbsr_debug.h): kernel selection for A/B timing and kernel attribution for bench.py
DEBUG_SIGNATURES = {
    "csbsr_debug_set_wgrad_tr": (None, [i32]),
    "csbsr_debug_set_conv_glds": (None, [i32]),
    "csbsr_debug_set_conv_tp": (None, [i32]),
    "csbsr_debug_set_conv_x3": (None, [i32]),
    "csbsr_debug_set_conv_x3w": (None, [i32]),
    "csbsr_debug_set_conv_x3n": (None, [i32]),
    "csbsr_debug_set_wgrad_hr": (None, [i32]),
    "csbsr_debug_last_conv_kernel": (i32, []),
    "csbsr_debug_last_wgrad_kernel": (i32, []),
    "csbsr_debug_cu_trace": (i32, [vp, i32, i32, vp]),
    "csbsr_debug_stream_create_cu_mask": (i32, [C.POINTER(vp), C.POINTER(C.c_uint32), i32]),
    "csbsr_debug_stream_destroy": (i32, [vp]),
    "csbsr_debug_stream_set_cu_budget": (i32, [vp, i32]),
    "csbsr_debug_stream_cu_budget": (i32, [vp]),
}

# The CSBSR_* environment hooks (A/B switches), declared once: variable, default, Engine attribute + how its value is parsed, library
# setter (csbsr_debug.h) + how its argument is parsed.  load() calls the setter of every variable that is set; Engine.__init__ sets every
# attribute, from the default where the variable is unset.  (CSBSR_LIB, the path of a variant build, is read above.)
Hook = namedtuple("Hook", "var default attr parse setter setter_parse", defaults=(None, None, None, None, int))
_not0, _is1 = "0".__ne__, "1".__eq__           # the usual parse rules: on unless "0", on only for "1"
ENV_HOOKS = (
    Hook("CSBSR_WGRAD_DBG", setter="csbsr_debug_set_wgrad_tr"),      # bit0 transpose reads, 2 no thin, 4 no tap order, 8 no flat grid, 16 flat everywhere
    # the library modes: 0 off, 1 default, 2 every eligible launch; the Engine flag: 0 routes the family's layers through the implicit-GEMM kernels
    Hook("CSBSR_CONV_X3", "1", "use_x3", _not0, "csbsr_debug_set_conv_x3"),          # the wide 3x3 layers
    # Winograd F(2,3)-along-x kernel for the wide 3x3 layers (csrc/conv_x3w.hip): built, parity-tested, 3-9 % faster per launch than the
    # direct kernels (-9 ms per config-2 step on the SFT convs) for a composed map 13 % further from the reference --
    # opt-in: CSBSR_CONV_X3W=1.  TWO parse rules, kept as they are: the Engine reads 0 off, "all" = 2 every eligible 3x3 layer, anything
    # else 1 = the SFT convs (Conv.winograd); the library reads "all" as mode 1 and a number as the mode (+ 8 x min input channels / 32)
    Hook("CSBSR_CONV_X3W", "0", "use_x3w", lambda v: {"0": 0, "all": 2}.get(v, 1), "csbsr_debug_set_conv_x3w", lambda v: 1 if v == "all" else int(v)),
    Hook("CSBSR_CONV_X3N", "1", "use_x3n", _not0, "csbsr_debug_set_conv_x3n"),       # 0 keeps the many-channels -> <= 64-cout 3x3 layers on the LDS-DMA tiles (csrc/conv_x3n.hip)
    Hook("CSBSR_WGRAD_HR", setter="csbsr_debug_set_wgrad_hr"),
    Hook("CSBSR_CONV_TP", "1", "use_tp", _not0, "csbsr_debug_set_conv_tp"),          # the 2x2-tap transposed layers
    Hook("CSBSR_CONV_GLDS", setter="csbsr_debug_set_conv_glds"),     # kernel selection experiments
    Hook("CSBSR_CONV_HR", "1", "use_hr", _not0),                 # 0 routes the HR small-channel layers through the implicit-GEMM kernels
    Hook("CSBSR_HEAD1", "1", "use_head1", _not0),                # 0 runs the 1-channel heads on the general conv kernels
    Hook("CSBSR_SPLIT_FUSED", "1", "split_fused", _not0),        # 0 = the three-block split forward (x_hi staged twice)
    Hook("CSBSR_DC_COMP", "1", "dc_comp", _not0),                # 0 = no compensation of the forward weights' fp16 rounding (Conv._dc_bias)
    Hook("CSBSR_TAPSUM", "1", "tapsum", _not0),                  # 0 = KBPN weights rounded to nearest instead of tap-sum-preserving (Conv._wq)
    Hook("CSBSR_WGRAD_MIRROR", "1", "wgrad_mirror", _is1),       # see Conv._bwd_weights_impl
    Hook("CSBSR_KBUP_FUSED", "1", "thin_tp_fused", _is1),        # see Conv.bwd_thin_tp_fused (A/B timing: 0)
    # up_conv3's epilogue-backward pass on kb.sr_reconst's dgrad (csrc/conv_thin.hip, DACT): 26 GB per step less fabric traffic, but the
    # fused launch is no faster than the two it replaces (1065 vs 1067 ms per step, same run) -- opt-in
    Hook("CSBSR_THIN_DACT", "0", "thin_dact", _is1),
    Hook("CSBSR_FOLD_PRELU", "1", "fold_prelu", _is1),           # blocks.py sft_bwd, BlurSkip's learned slopes (A/B timing: 0)
    # Weight gradients on a second HIP stream (opt-in, CSBSR_WGRAD_STREAM=1).  In the backward a layer's wgrad is a side branch (it
    # only feeds the parameter's gradient accumulator) while the dgrad chain is the critical path; the wgrads are MFMA-bound on
    # L2-resident tiles, much of what the chain runs between two of its convolutions is HBM-bound, so two streams could let the
    # dispatcher fill CUs an HBM-bound kernel leaves idle.  Same kernels, same per-parameter accumulation order (all wgrads stay
    # in program order on the side stream): bit-identical results (the GPU suite passes with it on).  Measured, round 4, same-run A/B: config 4
    # (HRNet-OCR, hundreds of small launches) 5.57 vs 5.57 img/s; config 2 at B = 4 6.92 -> 6.88 (the big kernels each fill the
    # chip: nothing to overlap); config 2 at B = 8 collapses to 2.4 img/s -- at 239 of 288 GB the operands the lagging side
    # stream still holds (record_stream) leave the caching allocator without free blocks and it falls back to synchronising
    # hipFree / hipMalloc cycles.  Hence off by default.
    Hook("CSBSR_WGRAD_STREAM", "0", "_wg_on", _is1),
)

_lib = None


class CsbsrHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once).  Raises if it is not built -- there is no CPU / torch fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CsbsrHipError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"(or `make -C csbsr_amd/csrc`).  csbsr_amd has no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for table in (SIGNATURES, DEBUG_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
    _lib = lib
    for h in ENV_HOOKS:
        if h.setter and os.environ.get(h.var):
            getattr(lib, h.setter)(h.setter_parse(os.environ[h.var]))
    return lib


def stream(device):
    """The current HIP stream of ``device`` as the ``csbsr_stream_t`` argument of an entry point."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, *args):
    """Invoke an int-returning entry point and raise on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise CsbsrHipError(f"{name} failed ({rc}): {lib.csbsr_last_error().decode()}")
