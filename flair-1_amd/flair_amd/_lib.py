"""ctypes binding of libflair_hip.so (C ABI declared in include/flair_hip.h).

There is NO CPU fallback: if the shared library is missing or a tensor is not on a HIP device the
product path raises.  (Build: ``python flair-1_amd/build.py`` or ``__graft_entry__.build()``.)
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLAIR_HIP_LIB") or os.path.join(_HERE, "libflair_hip.so")   # override: A/B of two builds on one box

_lib = None

vp, i32, i64, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes); must list every symbol of include/flair_hip.h
PROTOTYPES = {
    "flair_strerror": (C.c_char_p, [i32]),
    "flair_version": (i32, []),
    "flair_unet_create": (i32, [C.POINTER(vp), i32, i32, i32]),
    "flair_unet_destroy": (None, [vp]),
    "flair_unet_param_count": (i64, [vp]),
    "flair_unet_buffer_count": (i64, [vp]),
    "flair_unet_num_tensors": (i32, [vp]),
    "flair_unet_tensor_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64),
                                     C.POINTER(i32), C.POINTER(i32)]),
    "flair_unet_stage_range": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i64)]),
    "flair_unet_workspace_bytes": (i64, [vp, i32, i32, i32, i32]),
    "flair_unet_forward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp]),
    "flair_unet_backward": (i32, [vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(vp)]),
    "flair_unet_head_ld": (i32, [vp]),
    "flair_unet_encoder_forward": (i32, [vp, vp, vp, vp, C.POINTER(vp), i32, i32, i32, i32, vp, sz, vp]),
    "flair_unet_decoder_forward": (i32, [vp, vp, vp, C.POINTER(vp), vp, i32, i32, i32, i32, vp, sz, vp]),
    "flair_unet_head_forward": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
    "flair_unet_head_backward": (i32, [vp, vp, vp, vp, vp, vp, sz, vp]),
    "flair_unet_decoder_backward": (i32, [vp, vp, vp, C.POINTER(vp), vp, vp, sz, vp]),
    "flair_unet_encoder_backward": (i32, [vp, vp, C.POINTER(vp), vp, vp, sz, vp]),
    "flair_ce_workspace_bytes": (sz, [i32, i32, i32]),
    "flair_ce_head": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "flair_unet_logits_nhwc": (vp, [vp]),
    "flair_ce_head_nhwc": (i32, [vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "flair_seg_loss_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "flair_seg_loss": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "flair_seg_loss_nhwc": (i32, [vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "flair_softmax_argmax_nhwc": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "flair_softmax_argmax": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "flair_confmat_update": (i32, [vp, i32, vp, i32, i64, i32, vp, vp]),
    "flair_jaccard": (i32, [vp, i32, vp, vp, vp, vp]),
    "flair_confmat_masks": (i32, [vp, vp, i64, i32, i32, vp, vp]),
    "flair_feed_tiles": (i32, [vp, vp, vp, i32, i32, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(C.c_double),
                               C.POINTER(C.c_double), i32, vp, vp, vp]),
    "flair_feed_tiles_ptrs": (i32, [vp, vp, vp, i32, i32, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), i32, vp, vp, vp]),
    "flair_detect_convert": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
    "flair_gather_tiles": (i32, [vp, i32, i32, i32, vp, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), vp, vp]),
    "flair_detect_stitch": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp]),
    "flair_sgd_step": (i32, [vp, vp, i64, f32, vp]),
    "flair_optim_sgd": (i32, [vp, vp, vp, i64, f32, f32, f32, f32, i32, i32, f32, vp, vp]),
    "flair_optim_adamw": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, f32, i32, f32, vp, vp]),
    "flair_grad_sqnorm_partials": (i32, []),
    "flair_grad_sqnorm": (i32, [vp, i64, vp, vp, i32, vp]),
    "flair_clip_coef": (i32, [vp, f32, f32, vp, vp, vp]),
    "flair_add_rowvec_nchw": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "flair_add_rowvec_nhwc": (i32, [i32, vp, vp, i32, i32, i32, i32, vp]),
    "flair_add_rowvec_nhwc_to": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "flair_rowvec_grad_nhwc": (i32, [i32, vp, vp, i32, i32, i32, i32, vp]),
    "flair_conv2d_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32]),
    "flair_conv2d_forward": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp,
                                   vp, sz, vp]),
    "flair_conv2d_backward": (i32, [i32, vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "flair_conv2d_ex_workspace_bytes": (sz, [vp]),
    "flair_conv2d_ex": (i32, [vp, vp, sz, vp]),
    "flair_conv2d_ex_grid_rows": (i32, [vp]),
    "flair_conv2d_wgrad_ex_workspace_bytes": (sz, [vp]),
    "flair_conv2d_wgrad_ex": (i32, [vp, vp, sz, vp]),
    "flair_bn_workspace_bytes": (sz, [i64, i32]),
    "flair_bn_relu_forward": (i32, [i32, vp, i64, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, sz, vp]),
    "flair_bn_relu_backward": (i32, [i32, vp, vp, vp, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    "flair_bn_backward_ex": (i32, [vp, vp, sz, vp]),
    "flair_bwd16_ex_workspace_bytes": (sz, [vp]),
    "flair_bwd16_ex_grid_rows": (i32, [vp]),
    "flair_bwd16_ex": (i32, [vp, vp, sz, vp]),
    "flair_maxpool_backward_ex": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "flair_bn_act": (i32, [i32, vp, vp, vp, vp, i64, i32, i32, vp]),
    "flair_bn_act_maxpool": (i32, [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "flair_upcat_bwd": (i32, [i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]),
    "flair_ew_add": (i32, [i32, vp, vp, i64, vp]),
    "flair_colsum": (i32, [i32, vp, i64, i32, i32, vp, vp, sz, vp]),
    "flair_pack_weights": (i32, [i32, vp, vp, i32, vp, vp]),
    "flair_pack_weight": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "flair_maxpool_forward": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "flair_maxpool_backward": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "flair_nchw_to_nhwc": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, vp]),
    "flair_nhwc_to_nchw": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, vp]),
    "flair_sf_layernorm": (i32, [i32, vp, vp, vp, vp, i64, i32, f32, vp]),
    "flair_sf_dwconv3x3_gelu": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "flair_sf_bilinear_nhwc": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "flair_sf_bilinear_nchw_f32": (i32, [vp, vp, i64, i32, i32, i32, i32, vp]),
    "flair_sf_slice_cols": (i32, [i32, vp, i32, i32, i32, i64, vp, vp]),
    "flair_sf_fuse_bias": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "flair_sf_upsample_sum_bn_relu": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "flair_sf_ffn_fused_ok": (i32, [i32, i32, i32, i32]),
    "flair_sf_ffn_dw_pack": (i32, [vp, vp, vp, i32, vp]),
    "flair_sf_ffn_fused": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp]),
    "flair_sf_head_fused_ok": (i32, [i32, i32, i32, i32, i32, i32]),
    "flair_sf_head_wint": (i32, [vp, vp]),
    "flair_sf_head_fused": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "flair_sf_attention": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "flair_swin_window_attention": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "flair_swin_layernorm": (i32, [i32, vp, vp, vp, vp, i64, i32, i32, f32, vp]),
    "flair_swin_patch_merge_ln": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp]),
    "flair_swin_adaptive_avgpool": (i32, [i32, vp, i32, vp, i32, i32, i32, i32, i32, vp]),
    "flair_swin_bilinear_add": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "flair_profile_start": (i32, [i32]),
    "flair_profile_stop": (i32, []),
    "flair_profile_kernel": (i32, [i32, C.c_char_p, i32, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    "flair_metadata_mlp_forward": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    "flair_metadata_mlp_backward": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "flair_detect_stitch_preds": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, vp]),
    "flair_detect_blend_accum": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp]),
    "flair_detect_blend_flush": (i32, [vp, i32, i32, i32, i32, vp, i32, i32, vp]),
    "flair_detect_stitch_max": (i32, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, i32, i32, vp]),
    "flair_detect_stitch_max_preds": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, vp, i32, i32, vp]),
    "flair_zone_window_confmat_preds": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "flair_zone_window_confmat_logits": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "flair_detect_convert_q4": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
    "flair_detect_stitch_q4": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp]),
    "flair_detect_blend_accum_q4": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp]),
    "flair_detect_stitch_max_q4": (i32, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, i32, i32, vp]),
    "flair_zone_window_confmat_logits_q4": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "flair_d4_nchw_f32": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "flair_tta_accum": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp]),
    "flair_tta_accum_q4": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp]),
    "flair_zone_window_confmat_raster": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "flair_zone_raster_confmat": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "flair_zone_error_map": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, i32, C.c_double, i32, vp, vp, vp, vp, vp, vp]),
    "flair_tiff_lzw_slot_bytes": (C.c_long, [i32, i32]),
    "flair_tiff_lzw_encode": (i32, [vp, i32, i32, i32, i32, vp, C.c_long, vp, vp]),
    "flair_tiff_lzw_tile_slot_bytes": (C.c_long, [i32, i32]),
    "flair_tiff_lzw_encode_tiles": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, C.c_long, C.c_long, vp, C.c_long, vp, vp]),
    "flair_tiff_pack_streams": (i32, [vp, C.c_long, vp, vp, C.c_long, vp, C.c_long, vp]),
    "flair_tiff_lzw_decode_max_strip": (i32, []),
    "flair_tiff_lzw_decode": (i32, [vp, C.c_long, vp, vp, vp, vp, vp, C.c_long, vp, C.c_long, vp, vp]),
    "flair_tiff_lzw_decode_chunks_cap": (i32, []),
    "flair_tiff_lzw_decode_chunks_window": (i32, []),
    "flair_tiff_lzw_decode_chunks": (i32, [vp, C.c_long, vp, vp, vp, vp, C.c_long, vp, C.c_long, vp, vp]),
    "flair_tiff_chunks_to_planes": (i32, [vp, C.c_long, vp, vp, C.c_long, i32, i32, i32, vp, i32, i32, i32, vp]),
    "flair_tiff_chunks_to_batch": (i32, [vp, C.c_long, vp, vp, C.c_long, i32, vp, i32, i32, i32, vp]),
    "flair_segformer_create": (i32, [C.POINTER(vp), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, i32]),
    "flair_segformer_destroy": (None, [vp]),
    "flair_segformer_param_count": (i64, [vp]),
    "flair_segformer_num_tensors": (i32, [vp]),
    "flair_segformer_tensor_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32)]),
    "flair_segformer_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "flair_segformer_weights_changed": (None, [vp]),
    "flair_segformer_forward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "flair_upernet_create": (i32, [C.POINTER(vp), i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, C.POINTER(i32), i32, i32, i32]),
    "flair_upernet_destroy": (None, [vp]),
    "flair_upernet_param_count": (i64, [vp]),
    "flair_upernet_num_tensors": (i32, [vp]),
    "flair_upernet_tensor_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32)]),
    "flair_upernet_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "flair_upernet_weights_changed": (None, [vp]),
    "flair_upernet_forward": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "flair_upernet_forward_quarter": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "flair_tune_set": (i32, [C.c_char_p, i32]),
    "flair_debug_buffer": (i32, [vp]),
}


class UnetFwdOpts(C.Structure):
    """flair_unet_fwd_opts_t: the last argument of flair_unet_forward (by reference; None = a plain forward)"""
    _fields_ = [("reuse_constants", i32), ("preds_u8", vp), ("maxprob_f32", vp),
                ("ce_labels", vp), ("ce_label_kind", i32), ("ce_class_weight", vp), ("ce_loss", vp),
                ("ce_preds_u8", vp), ("ce_confmat", vp), ("ce_workspace", vp),
                ("rows_f32", vp), ("drows_f32", vp)]


class SegLossSpec(C.Structure):
    """flair_seg_loss_t (flair_amd.losses.SegLoss.astuple() in its order)"""
    _fields_ = [("ce", f32), ("label_smoothing", f32), ("focal_gamma", f32), ("dice", f32), ("dice_smooth", f32), ("dice_eps", f32)]


class ConvEx(C.Structure):
    """flair_conv_ex_t"""
    _fields_ = [("dtype", i32), ("mode", i32), ("x0", vp), ("x1", vp),
                ("N", i32), ("H", i32), ("W", i32), ("C0", i32), ("C1", i32), ("up0", i32),
                ("w_oihw", vp), ("bias", vp), ("Cout", i32), ("R", i32), ("stride", i32), ("pad", i32),
                ("y_nhwc", vp), ("out_ld", i32), ("y_nchw", vp), ("stats", vp),
                ("in_scale", vp), ("in_shift", vp), ("oscale", vp), ("oshift", vp), ("ores", vp), ("orelu", i32),
                ("accumulate", i32), ("acc_src", vp),
                ("pool_c0", i32), ("out_skip", vp), ("out_skip_ld", i32), ("skip_accumulate", i32),
                ("preds_u8", vp), ("maxprob_f32", vp), ("ogelu", i32),
                ("bnr_y", vp), ("bnr_out", vp), ("bnr_scale", vp), ("bnr_shift", vp),
                ("bnr_partial", vp), ("bnr_rows", i32), ("bnr_mask", i32)]


class WgradEx(C.Structure):
    """flair_wgrad_ex_t"""
    _fields_ = [("dtype", i32), ("x0", vp), ("x1", vp),
                ("N", i32), ("H", i32), ("W", i32), ("C0", i32), ("C1", i32), ("up0", i32),
                ("dy", vp), ("dy_ld", i32), ("Cout", i32), ("R", i32), ("stride", i32), ("pad", i32),
                ("dw", vp), ("Cin_real", i32), ("accumulate", i32), ("in_scale", vp), ("in_shift", vp),
                ("dbias", vp), ("cus", i32),
                ("fuse_y", vp), ("fuse_coef", vp), ("fuse_msc", vp), ("fuse_msh", vp)]


class BnBwdEx(C.Structure):
    """flair_bn_bwd_ex_t"""
    _fields_ = [("dtype", i32), ("dout", vp), ("out", vp), ("y", vp), ("mean", vp), ("invstd", vp), ("gamma", vp),
                ("rows", i64), ("C", i32), ("partial", vp), ("pre_nblk", i32), ("premasked", i32),
                ("mscale", vp), ("mshift", vp), ("dgamma", vp), ("dbeta", vp), ("accumulate_param", i32),
                ("dy", vp), ("dres", vp), ("dres_accumulate", i32), ("coef", vp)]


class Bwd16Ex(C.Structure):
    """flair_bwd16_ex_t"""
    _fields_ = [("g", vp), ("gy", vp), ("gcoef", vp), ("gmsc", vp), ("gmsh", vp), ("x", vp), ("in_scale", vp), ("in_shift", vp),
                ("w_oihw", vp), ("Cout", i32), ("N", i32), ("H", i32), ("W", i32), ("dx", vp),
                ("bnr_scale", vp), ("bnr_shift", vp), ("bnr_partial", vp), ("bnr_rows", i32), ("dw", vp), ("dbias", vp)]


class PackDesc(C.Structure):
    """flair_pack_desc_t"""
    _fields_ = [("w_off", i64), ("dst_off", C.c_uint64),
                ("Cout", i32), ("Cin", i32), ("R", i32), ("S", i32), ("Cin_p", i32), ("rows_pad", i32), ("Kpad", i32), ("tf", i32),
                ("r0", i32), ("rstep", i32), ("Rc", i32), ("s0", i32), ("sstep", i32), ("Sc", i32)]


class FlairHipError(RuntimeError):
    pass


def lib():
    """Load the HIP library once; fail loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FlairHipError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
                "Build it with `python flair-1_amd/build.py`.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().flair_strerror(rc).decode()
        raise FlairHipError(f"{what}: {msg} (code {rc})" if what else f"{msg} (code {rc})")


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors: the product path is HIP-only."""
    if t is None:
        return None
    if not t.is_cuda:
        raise FlairHipError("flair_amd kernels need tensors on a HIP device (no CPU fallback)")
    if not t.is_contiguous():
        raise FlairHipError("flair_amd kernels need contiguous tensors")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


DT_F32, DT_BF16 = 0, 1


def torch_dtype(dt: int):
    return torch.float32 if dt == DT_F32 else torch.bfloat16


def dtype_code(name) -> int:
    if name in (0, "f32", "fp32", "float32", torch.float32):
        return DT_F32
    if name in (1, "bf16", "bfloat16", torch.bfloat16):
        return DT_BF16
    raise ValueError(f"unsupported compute dtype {name!r} (use 'f32' or 'bf16')")
