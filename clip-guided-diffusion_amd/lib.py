"""ctypes binding of libcgd_mi355x.so (the C ABI declared in include/cgd_mi355x.h).

The product path has NO fallback: if the HIP library is missing or fails to load this module raises, and
every wrapper raises RuntimeError(cgd_last_error()) on a non-zero status.
"""
import ctypes as C
import os
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))
# CGD_LIB_PATH: tuning knob for same-box A/B runs of two builds (benchmarks/ab.sh); the product loads the in-tree library
LIB_PATH = os.environ.get("CGD_LIB_PATH") or os.path.join(_HERE, "libcgd_mi355x.so")

F32P = C.POINTER(C.c_float)
vp = C.c_void_p
i32 = C.c_int
i64 = C.c_int64
f32 = C.c_float


class UNetConfig(C.Structure):
    _fields_ = [
        ("image_size", i32), ("model_channels", i32), ("num_res_blocks", i32), ("n_mult", i32),
        ("channel_mult", f32 * 8), ("n_att", i32), ("attention_ds", i32 * 8), ("num_classes", i32),
        ("num_heads", i32), ("num_head_channels", i32), ("use_new_attention_order", i32),
        ("in_channels", i32), ("out_channels", i32),
        # the classic architecture (0 / 0: the published guided-diffusion checkpoints, and what UNetConfig() gets)
        ("classic_resample", i32), ("additive_emb", i32),
    ]


class ClassifierConfig(C.Structure):
    """cgd_classifier_config"""
    _fields_ = [
        ("image_size", i32), ("model_channels", i32), ("num_res_blocks", i32), ("n_mult", i32),
        ("channel_mult", f32 * 8), ("n_att", i32), ("attention_ds", i32 * 8), ("num_head_channels", i32), ("out_channels", i32),
    ]


class ViTConfig(C.Structure):
    _fields_ = [("resolution", i32), ("patch", i32), ("width", i32), ("layers", i32), ("heads", i32), ("out_dim", i32)]


class DepthConfig(C.Structure):
    """cgd_depth_config"""
    _fields_ = [("patch", i32), ("width", i32), ("layers", i32), ("heads", i32), ("hooks", i32 * 4), ("native_grid", i32), ("features", i32),
                ("reassemble_channels", i32 * 4)]


class TextConfig(C.Structure):
    _fields_ = [("context_length", i32), ("vocab_size", i32), ("width", i32), ("layers", i32), ("heads", i32), ("out_dim", i32)]


class RNConfig(C.Structure):
    _fields_ = [("resolution", i32), ("width", i32), ("layers", i32 * 4), ("out_dim", i32), ("heads", i32)]


class StepCoef(C.Structure):
    _fields_ = [
        ("sqrt_recip", f32), ("sqrt_recipm1", f32), ("coef1", f32), ("coef2", f32), ("min_log", f32), ("max_log", f32),
        ("fac", f32), ("sqrt_one_minus_ab", f32), ("sqrt_ab_prev", f32), ("sqrt_one_minus_ab_prev", f32), ("nonzero", i32),
    ]


class Multistep(C.Structure):
    """cgd_multistep: phase 0 Adams-Bashforth, 1 start predictor, 2 start corrector, 3 DDIM with eta"""
    _fields_ = [("phase", i32), ("order", i32), ("sigma", f32), ("dir", f32)]


class MaskCoef(C.Structure):
    """cgd_mask_coef: coefficients of cgd_masked_merge at one step index; flags = the optional buffers passed (MASK_*)"""
    _fields_ = [("sqrt_ab_prev", f32), ("sqrt_one_minus_ab_prev", f32), ("renoise_x", f32), ("renoise_n", f32), ("flags", i32)]


MASK_PRED_XSTART, MASK_N_KNOWN, MASK_RENOISE = 1, 2, 4


class ReverseCoef(C.Structure):
    """cgd_reverse_coef: coefficients of cgd_ddim_reverse_update, the DDIM inversion step from level i up to level i + 1"""
    _fields_ = [("sqrt_recip", f32), ("sqrt_recipm1", f32), ("sqrt_ab_next", f32), ("sqrt_one_minus_ab_next", f32),
                ("inv_sqrt_one_minus_ab_next", f32)]


class Dpmpp(C.Structure):
    """cgd_dpmpp: coefficients of cgd_dpmpp_update, the DPM-Solver++ step from level i to level i - 1 (diffusion.dpmpp_coef)"""
    _fields_ = [("c_x", f32), ("c_d", f32), ("c_r", f32), ("c_n", f32)]


class Warp(C.Structure):
    """cgd_warp: the inverse affine map of cgd_frame_warp (source position of destination pixel (x, y): m0 x + m1 y + m2, m3 x + m4 y + m5),
    interp 0 bilinear / 1 bicubic, border 0 wrap / 1 reflect / 2 replicate, clamp 1 = clamp the result to [-1, 1]"""
    _fields_ = [("m", C.c_double * 6), ("interp", i32), ("border", i32), ("clamp", i32)]


class Camera(C.Structure):
    """cgd_camera: the pinhole camera of cgd_frame_warp3d.  X' = R X + T between two frames (R row-major), focal length f in pixels, principal
    point (cx, cy), flat depth z0, near plane, `iters` fixed-point steps of the depth lookup; interp / border / clamp as in cgd_warp"""
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z0", C.c_double),
                ("near", C.c_double), ("iters", i32), ("interp", i32), ("border", i32), ("clamp", i32)]


class FlowParams(C.Structure):
    """cgd_flow_params: pyramid levels, iterations per level, window radius, the regulariser lambda and the longest step of one iteration
    (pixels) of the Lucas-Kanade flow (cgd_flow_estimate)"""
    _fields_ = [("levels", i32), ("iters", i32), ("radius", i32), ("lam", f32), ("max_step", f32)]


class WarpFlow(C.Structure):
    """cgd_warp_flow: the settings of cgd_frame_warp_flow: blend, the forward-backward check's alpha and beta, interp / border / clamp as in
    cgd_warp"""
    _fields_ = [("blend", f32), ("alpha", f32), ("beta", f32), ("interp", i32), ("border", i32), ("clamp", i32)]


WARP_INTERP = {"bilinear": 0, "bicubic": 1}
WARP_BORDER = {"wrap": 0, "reflect": 1, "replicate": 2}

MANIFEST_CB = C.CFUNCTYPE(None, C.c_char_p, i64, vp)

# name -> (restype, argtypes).  Pointers to device memory are passed as integers (tensor.data_ptr()).
_SIGS = {
    "cgd_unet_manifest": (i32, [C.POINTER(UNetConfig), MANIFEST_CB, vp]),
    "cgd_vit_manifest": (i32, [C.POINTER(ViTConfig), MANIFEST_CB, vp]),
    "cgd_rn_manifest": (i32, [C.POINTER(RNConfig), MANIFEST_CB, vp]),
    "cgd_text_manifest": (i32, [C.POINTER(TextConfig), MANIFEST_CB, vp]),
    "cgd_lpips_manifest": (i32, [MANIFEST_CB, vp]),
    "cgd_version": (C.c_char_p, []),
    "cgd_ctx_create": (i32, [C.POINTER(vp), i32]),
    "cgd_ctx_destroy": (None, [vp]),
    "cgd_last_error": (C.c_char_p, [vp]),
    "cgd_set_precision": (i32, [vp, i32]),
    "cgd_get_precision": (i32, [vp]),
    "cgd_ctx_device_allocs": (i64, [vp]),
    "cgd_set_tiles": (i32, [vp, i32, i32]),
    "cgd_set_hgemm": (i32, [vp, i32, i32, i32]),
    "cgd_profile": (i32, [vp, i32]),
    "cgd_profile_read": (i32, [vp, C.POINTER(C.c_double)]),
    "cgd_profile_kinds": (i32, []),
    "cgd_launch_counts": (i32, [C.POINTER(C.c_uint64)]),
    "cgd_unet_create": (i32, [vp, C.POINTER(UNetConfig), C.POINTER(vp)]),
    "cgd_unet_destroy": (None, [vp]),
    "cgd_unet_num_params": (i32, [vp]),
    "cgd_unet_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_unet_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_unet_finalize": (i32, [vp]),
    "cgd_unet_forward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_unet_embed": (i32, [vp, vp, vp, i32, i32, vp]),
    "cgd_unet_forward_slot": (i32, [vp, vp, i32, vp, i32, i32, i32, vp]),
    "cgd_unet_dgrad": (i32, [vp, vp, vp, vp]),
    "cgd_unet_set_low_res": (i32, [vp, vp, i32, i32, i32, vp]),
    "cgd_vit_create": (i32, [vp, C.POINTER(ViTConfig), C.POINTER(vp)]),
    "cgd_vit_destroy": (None, [vp]),
    "cgd_vit_num_params": (i32, [vp]),
    "cgd_vit_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_vit_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_vit_finalize": (i32, [vp]),
    "cgd_vit_set_activation": (i32, [vp, i32]),
    "cgd_vit_forward": (i32, [vp, vp, i32, i32, vp, vp]),
    "cgd_vit_dgrad": (i32, [vp, vp, vp, vp]),
    "cgd_text_create": (i32, [vp, C.POINTER(TextConfig), C.POINTER(vp)]),
    "cgd_text_destroy": (None, [vp]),
    "cgd_text_num_params": (i32, [vp]),
    "cgd_text_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_text_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_text_finalize": (i32, [vp]),
    "cgd_text_set_activation": (i32, [vp, i32]),
    "cgd_text_forward": (i32, [vp, vp, i32, vp, vp]),
    "cgd_rn_create": (i32, [vp, C.POINTER(RNConfig), C.POINTER(vp)]),
    "cgd_rn_destroy": (None, [vp]),
    "cgd_rn_num_params": (i32, [vp]),
    "cgd_rn_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_rn_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_rn_finalize": (i32, [vp]),
    "cgd_rn_forward": (i32, [vp, vp, i32, vp, vp]),
    "cgd_rn_dgrad": (i32, [vp, vp, vp, vp]),
    "cgd_rn_debug_relu_count": (i32, [vp]),
    "cgd_rn_debug_relu_info": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i32)]),
    "cgd_rn_debug_relu_set": (i32, [vp, i32, vp, vp]),
    "cgd_lpips_create": (i32, [vp, C.POINTER(vp)]),
    "cgd_lpips_destroy": (None, [vp]),
    "cgd_lpips_num_params": (i32, [vp]),
    "cgd_lpips_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_lpips_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_lpips_finalize": (i32, [vp]),
    "cgd_lpips_set_reference": (i32, [vp, vp, i32, i32, i32, vp]),
    "cgd_lpips_loss_grad": (i32, [vp, vp, f32, vp, vp, i32, vp]),
    "cgd_lpips_debug_replay": (i32, [vp, C.POINTER(vp)]),
    "cgd_lpips_set_style": (i32, [vp, vp, i32, i32, C.POINTER(f32), vp]),
    "cgd_lpips_style_loss_grad": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, i32, vp]),
    "cgd_op_gram": (i32, [vp, vp, i32, i32, i32, i32, f32, vp, vp]),
    "cgd_secondary_manifest": (i32, [MANIFEST_CB, vp]),
    "cgd_secondary_create": (i32, [vp, C.POINTER(vp)]),
    "cgd_secondary_destroy": (None, [vp]),
    "cgd_secondary_num_params": (i32, [vp]),
    "cgd_secondary_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_secondary_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_secondary_finalize": (i32, [vp]),
    "cgd_secondary_forward": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "cgd_secondary_forward_blend": (i32, [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp]),
    "cgd_secondary_dgrad": (i32, [vp, vp, vp, vp]),
    "cgd_secondary_debug_replay": (i32, [vp, C.POINTER(vp)]),
    "cgd_secondary_head": (i32, [vp, vp, vp, vp, f32, vp, vp, i32, i32, i32, vp]),
    "cgd_secondary_combine": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, f32, f32, vp]),
    "cgd_op_secondary_pack": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_op_bilinear_up2x": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_depth_manifest": (i32, [C.POINTER(DepthConfig), MANIFEST_CB, vp]),
    "cgd_depth_create": (i32, [vp, C.POINTER(DepthConfig), C.POINTER(vp)]),
    "cgd_depth_destroy": (None, [vp]),
    "cgd_depth_num_params": (i32, [vp]),
    "cgd_depth_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_depth_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_depth_finalize": (i32, [vp]),
    "cgd_depth_set_pos_embed": (i32, [vp, i32, i32, vp]),
    "cgd_depth_forward": (i32, [vp, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp]),
    "cgd_depth_debug_map": (i32, [vp, i32, vp, C.POINTER(i32), vp]),
    "cgd_depth_debug_stop": (i32, [vp, i32]),
    "cgd_op_relu_rows": (i32, [vp, vp, i32, vp, i32, i64, i32, vp]),
    "cgd_op_bilinear_up2x_ac": (i32, [vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv_transpose": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_op_depth_readout": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_op_depth_head_tail": (i32, [vp, vp, i32, vp, vp, vp, vp, i64, i32, f32, f32, f32, vp]),
    "cgd_op_resize_cubic": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, f32, i32, vp]),
    "cgd_classifier_manifest": (i32, [C.POINTER(ClassifierConfig), MANIFEST_CB, vp]),
    "cgd_classifier_create": (i32, [vp, C.POINTER(ClassifierConfig), C.POINTER(vp)]),
    "cgd_classifier_destroy": (None, [vp]),
    "cgd_classifier_num_params": (i32, [vp]),
    "cgd_classifier_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64)]),
    "cgd_classifier_set_param": (i32, [vp, C.c_char_p, vp, i64]),
    "cgd_classifier_finalize": (i32, [vp]),
    "cgd_classifier_forward": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_classifier_dgrad": (i32, [vp, f32, vp, i32, vp]),
    "cgd_op_attnpool_scratch_floats": (i64, [i32, i32, i32, i32, i32]),
    "cgd_op_attnpool_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_op_attnpool_bwd": (i32, [vp, vp, vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_aug_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_aug_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_aug_scratch_floats": (i64, [i32, i32, i32, i32]),
    "cgd_op_aug_sample_map": (i32, [vp, i32, i32, vp, vp, vp]),
    "cgd_cutouts_resize_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_resize_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_cutouts_resize_scratch_floats": (i64, [i32, i32, i32, i32]),
    "cgd_cutouts_resize_weights": (i32, [i32, i32, vp, vp, C.POINTER(i32)]),
    "cgd_spherical_loss": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp]),
    "cgd_directional_loss": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]),
    "cgd_spherical_loss_regions": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_directional_loss_regions": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_op_region_coverage": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_aesthetic_loss": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp]),
    "cgd_pmv_blend": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef), vp]),
    "cgd_guidance_part_blocks": (i32, [i32, i32, i32]),
    "cgd_guidance_combine": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef), f32, f32, f32, vp]),
    "cgd_grad_finish": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "cgd_scalars": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp]),
    "cgd_sample_update": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef), i32, vp]),
    "cgd_multistep_update": (i32, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp), vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef),
                                    C.POINTER(StepCoef), C.POINTER(Multistep), vp]),
    "cgd_dpmpp_update": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef), C.POINTER(Dpmpp), vp]),
    "cgd_abs_quantile_scratch_bytes": (i64, [i32, i64]),
    "cgd_abs_quantile_slice": (i32, []),
    "cgd_op_abs_quantile": (i32, [vp, vp, i32, i64, i64, f32, f32, f32, vp, vp, vp]),
    "cgd_dpmpp_threshold": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef), i64, f32, f32, f32, vp, vp, vp]),
    "cgd_dpmpp_update_thr": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(StepCoef), C.POINTER(Dpmpp), vp]),
    "cgd_masked_merge": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(MaskCoef), vp]),
    "cgd_ilvr_scratch_floats": (C.c_long, [i32, i32, i32, i32, i32]),
    "cgd_ilvr_refine": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp]),
    "cgd_frame_warp": (i32, [vp, vp, vp, i32, i32, i32, i32, C.POINTER(Warp), vp]),
    "cgd_frame_warp3d": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(Camera), vp]),
    "cgd_flow_levels": (i32, [i32, i32, i32, i32]),
    "cgd_flow_scratch_floats": (C.c_long, [i32, i32, i32, i32, i32]),
    "cgd_flow_estimate": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, C.POINTER(FlowParams), vp]),
    "cgd_op_flow_level": (i32, [vp, vp, vp, vp, i32, i32, vp, i32, i32, i32, C.POINTER(FlowParams), vp]),
    "cgd_frame_warp_flow": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(WarpFlow), vp]),
    "cgd_channel_stats": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "cgd_color_match": (i32, [vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, i32, vp]),
    "cgd_window_gather": (i32, [vp, vp, vp, C.POINTER(i32), i32, C.POINTER(i32), i32, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_window_merge": (i32, [vp, vp, vp, C.POINTER(i32), i32, C.POINTER(i32), i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_ddim_reverse_update": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, C.POINTER(ReverseCoef), vp]),
    "cgd_op_gemm": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, f32, i32, i32, vp]),
    "cgd_op_gemm_ex": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, f32, i32, i32, i32, i32, vp]),
    "cgd_op_pending": (i32, [vp, C.POINTER(i64)]),
    "cgd_op_gemm_gn_bwd_accepts": (i32, [i32] * 12),
    "cgd_op_gemm_gn_bwd": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp]),
    "cgd_op_plan": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32)]),
    "cgd_op_plan_conv": (i32, [i32] * 10 + [C.POINTER(i32)]),
    "cgd_op_pack_conv3x3_frag": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "cgd_set_hconv": (i32, [vp, i32, i32]),
    "cgd_op_conv3x3_s2": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv3x3_s2_dgrad": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv3x3_s2_accepts": (i32, [i32] * 9),
    "cgd_op_plan_conv_s2": (i32, [i32] * 7 + [C.POINTER(i32)]),
    "cgd_op_conv3x3_s2_packed": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv3x3_s2_dgrad_packed": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv3x3": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv3x3_ex": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp]),
    "cgd_op_pack_conv3x3_wino": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "cgd_op_conv3x3_wino": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cgd_set_wino": (i32, [vp, i32, i32]),
    "cgd_op_conv3x3_wino_ex": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp]),
    "cgd_op_new_pass": (i32, [vp]),
    "cgd_op_gn_record_merges": (i64, [vp]),
    "cgd_op_gn_records": (i32, [vp, vp, i32, i64, i32, i32, vp, i64, C.POINTER(i32), vp]),
    "cgd_op_gn_stats_offset": (i64, [i32, i32, i32]),
    "cgd_op_wconv_schedule": (i32, [i32, i32, C.POINTER(i32)]),
    "cgd_op_mfma_peak": (i32, [vp, i32, C.POINTER(C.c_double), vp]),
    "cgd_op_conv_in": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_op_conv_thin_out": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_op_sr_stem": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cgd_op_gn_scratch_floats": (i64, [i32, i32, i32]),
    "cgd_op_gn_fwd": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, i32, f32, vp, vp]),
    "cgd_op_gn_bwd": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp]),
    "cgd_op_ln_fwd": (i32, [vp, vp, vp, i32, i32, vp, vp, f32, vp, vp]),
    "cgd_op_ln_bwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp]),
    "cgd_op_pool2x2": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, vp]),
    "cgd_op_upsample2x": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, vp]),
    "cgd_op_act": (i32, [vp, vp, vp, vp, i64, i32, vp]),
    "cgd_op_attn_buf_floats": (i64, [i32, i32, i32, i32, i32]),
    "cgd_op_attn_buf_floats_ctx": (i64, [vp, i32, i32, i32, i32, i32, i32, i32]),
    "cgd_op_attn_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp), vp]),
    "cgd_op_attn_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp), vp]),
    "cgd_op_attn_fwd_causal": (i32, [vp, vp, vp, i32, i32, i32, i32, C.POINTER(vp), vp]),
    "cgd_op_attn_plan": (i32, [i32, i32, i32, i32, i32, i32, C.POINTER(i32)]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None


def load():
    """Load the shared library (once).  Raises if it is absent: there is no CPU or eager fallback."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The MI355X path has no fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class CgdError(RuntimeError):
    pass


class Context:
    """One per GPU; owns the split-K workspace and the error string."""

    def __init__(self, device=0, precision=None):
        import torch
        self.lib = load()
        if not torch.cuda.is_available():
            raise RuntimeError("cgd_mi355x needs an MI355X (gfx950) GPU visible to PyTorch-ROCm")
        h = vp()
        rc = self.lib.cgd_ctx_create(C.byref(h), int(device))
        if rc != 0:
            raise CgdError(f"cgd_ctx_create failed with status {rc} (is device {device} a gfx950?)")
        self.h = h
        self.device = int(device)
        self._nets = weakref.WeakSet()  # network handles created on this context (nets._Net._adopt)
        if precision is not None:
            self.set_precision(precision)
        tiles = os.environ.get("CGD_TILES")  # tuning only: "<large>,<small>" igemm tile codes (see cgd_set_tiles)
        if tiles:
            large, small = (int(v) for v in tiles.split(","))
            self.check(self.lib.cgd_set_tiles(self.h, large, small))
        hg = os.environ.get("CGD_HGEMM")  # tuning only: "<mode>,<min_m>,<min_chunks>" of the weight GEMM kernel
        if hg:
            self.check(self.lib.cgd_set_hgemm(self.h, *(int(v) for v in hg.split(","))))
        hv = os.environ.get("CGD_HCONV_VAR")  # tuning only: halo conv kernel variant (see cgd_set_hconv)
        if hv:
            self.check(self.lib.cgd_set_hconv(self.h, 1 + 16 * int(hv), 256))

    def check(self, rc):
        if rc != 0:
            what = {-1: "HIP runtime error", -2: "invalid argument or state", -3: "NULL handle or pointer", -4: "not a gfx950 device"}.get(rc, "error")
            msg = self.lib.cgd_last_error(self.h).decode() if rc in (-1, -2) else ""
            raise CgdError(f"{what} (status {rc})" + (f": {msg}" if msg else ""))

    def set_precision(self, mode):
        mode = {"f32": 0, "bf16x3": 1, "bf16": 2}.get(mode, mode)
        self.check(self.lib.cgd_set_precision(self.h, int(mode)))

    @property
    def precision(self):
        return self.lib.cgd_get_precision(self.h)

    def stream(self):
        """The caller's current HIP stream ON THE CONTEXT'S DEVICE (not on whatever device happens to be current)."""
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if getattr(self, "h", None):
            for net in list(self._nets):
                net.close()
            self.lib.cgd_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ptr(t):
    """Device pointer of a contiguous fp32/int tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "cgd_mi355x expects contiguous tensors"
    return t.data_ptr()


def stream_ptr(device=None):
    """Current HIP stream of `device` (default: the current device).  Product code uses Context.stream()."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream
