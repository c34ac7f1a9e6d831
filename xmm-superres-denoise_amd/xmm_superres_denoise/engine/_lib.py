"""ctypes binding of libxsd_hip.so (C ABI: include/xsd.h).  Fails loudly if the library is missing."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))          # .../xmm-superres-denoise_amd
LIB_PATH = os.environ.get("XSD_LIB") or os.path.join(_PKG_ROOT, "lib", "libxsd_hip.so")   # XSD_LIB: A/B builds
CSRC_DIR = os.path.join(_PKG_ROOT, "csrc")

_lib = None


class XsdError(RuntimeError):
    pass


class XsdConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("kind", "in_channels", "out_channels", "num_filters", "num_res_blocks", "num_upsample",
                 "memory_efficient", "reserved")]


class XsdTestOut(ctypes.Structure):      # xsd_test_out (include/xsd.h): one output chunk of xsd_test_conv3x3_ex and its fused epilogue
    _fields_ = [("p", ctypes.c_void_p), ("e1", ctypes.c_void_p), ("e2", ctypes.c_void_p), ("e3", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("a1", ctypes.c_float), ("s1", ctypes.c_float), ("a2", ctypes.c_float), ("s2", ctypes.c_float), ("s3", ctypes.c_float),
                ("slope", ctypes.c_float), ("mslope", ctypes.c_float), ("accumulate", ctypes.c_int32),
                ("bits_out", ctypes.c_void_p), ("bits_in", ctypes.c_void_p)]


class XsdTestGconvArgs(ctypes.Structure):      # xsd_test_gconv_args (include/xsd.h): the views and the fused epilogue of one generic-width conv
    _fields_ = [("x", ctypes.c_void_p), ("xbs", ctypes.c_int64), ("y", ctypes.c_void_p), ("ybs", ctypes.c_int64),
                ("a1", ctypes.c_float), ("e1", ctypes.c_void_p), ("e1bs", ctypes.c_int64), ("s1", ctypes.c_float), ("e1c", ctypes.c_int32),
                ("a2", ctypes.c_float), ("e2", ctypes.c_void_p), ("e2bs", ctypes.c_int64), ("s2", ctypes.c_float),
                ("slope", ctypes.c_float), ("accumulate", ctypes.c_int32), ("shuffle", ctypes.c_int32),
                ("skip", ctypes.c_void_p), ("skipbs", ctypes.c_int64), ("skipc", ctypes.c_int32),
                ("pre", ctypes.c_void_p), ("clamp01", ctypes.c_int32)]


class XsdSwGemmView(ctypes.Structure):      # xsd_sw_gemm_view (include/xsd.h): one launch of the Swin GEMM as the forwards describe theirs
    _fields_ = [("conv3", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("cin", ctypes.c_int32),
                ("N", ctypes.c_int32), ("a", ctypes.c_void_p), ("a_nchw", ctypes.c_int32), ("lda", ctypes.c_int64),
                ("imean", ctypes.c_void_p), ("irange", ctypes.c_float), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("act", ctypes.c_int32), ("slope", ctypes.c_float), ("res", ctypes.c_void_p), ("rbs", ctypes.c_int64), ("rps", ctypes.c_int64),
                ("omode", ctypes.c_int32), ("y", ctypes.c_void_p), ("ldy", ctypes.c_int64), ("r", ctypes.c_int32), ("omean", ctypes.c_void_p),
                ("orange", ctypes.c_float), ("math", ctypes.c_int32), ("rnchw", ctypes.c_int32), ("cH", ctypes.c_int32), ("cW", ctypes.c_int32),
                ("up2", ctypes.c_int32)]


class XsdRestormerConfig(ctypes.Structure):
    _fields_ = [("inp_channels", ctypes.c_int32), ("out_channels", ctypes.c_int32), ("dim", ctypes.c_int32),
                ("num_blocks", ctypes.c_int32 * 4), ("num_refinement_blocks", ctypes.c_int32), ("heads", ctypes.c_int32 * 4),
                ("bias", ctypes.c_int32), ("layernorm_bias_free", ctypes.c_int32), ("dual_pixel_task", ctypes.c_int32),
                ("ffn_expansion_factor", ctypes.c_double)]


class XsdSwinFIRConfig(ctypes.Structure):
    _fields_ = [("img_size", ctypes.c_int32 * 2), ("patch_size", ctypes.c_int32 * 2), ("in_chans", ctypes.c_int32),
                ("embed_dim", ctypes.c_int32), ("num_layers", ctypes.c_int32), ("depths", ctypes.c_int32 * 16),
                ("num_heads", ctypes.c_int32 * 16), ("window_size", ctypes.c_int32), ("qkv_bias", ctypes.c_int32), ("ape", ctypes.c_int32),
                ("patch_norm", ctypes.c_int32), ("upscale", ctypes.c_int32), ("upsampler", ctypes.c_int32),
                ("resi_connection", ctypes.c_int32), ("mlp_ratio", ctypes.c_double), ("qk_scale", ctypes.c_double),
                ("img_range", ctypes.c_double)]


class XsdSwinIRConfig(ctypes.Structure):      # the same fields as SwinFIR's; upsampler 0..3 and resi_connection 0 "1conv" / 1 "3conv"
    _fields_ = list(XsdSwinFIRConfig._fields_)


class XsdHATConfig(ctypes.Structure):
    _fields_ = [("img_size", ctypes.c_int32 * 2), ("patch_size", ctypes.c_int32 * 2), ("in_chans", ctypes.c_int32),
                ("embed_dim", ctypes.c_int32), ("num_layers", ctypes.c_int32), ("depths", ctypes.c_int32 * 16),
                ("num_heads", ctypes.c_int32 * 16), ("window_size", ctypes.c_int32), ("compress_ratio", ctypes.c_int32),
                ("squeeze_factor", ctypes.c_int32), ("qkv_bias", ctypes.c_int32), ("ape", ctypes.c_int32), ("patch_norm", ctypes.c_int32),
                ("upscale", ctypes.c_int32), ("upsampler", ctypes.c_int32), ("resi_connection", ctypes.c_int32),
                ("mlp_ratio", ctypes.c_double), ("qk_scale", ctypes.c_double), ("img_range", ctypes.c_double),
                ("conv_scale", ctypes.c_double), ("overlap_ratio", ctypes.c_double)]


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    if force:
        subprocess.check_call(["make", "-C", CSRC_DIR, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC_DIR, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XsdError(f"{LIB_PATH} not found: build it with `make -C {CSRC_DIR}` "
                       "(or __graft_entry__.build()). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp, fp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    L.xsd_last_error.restype = ctypes.c_char_p
    L.xsd_version.restype = ctypes.c_char_p
    L.xsd_create.argtypes = [ctypes.POINTER(XsdConfig), ctypes.POINTER(vp)]
    L.xsd_destroy.argtypes = [vp]
    L.xsd_destroy.restype = None
    L.xsd_param_count.argtypes = [vp]
    L.xsd_param_count.restype = i64
    L.xsd_pack_weights.argtypes = [vp, fp, vp]
    L.xsd_set_math.argtypes = [vp, i32]
    L.xsd_get_math.argtypes = [vp]
    L.xsd_forward.argtypes = [vp, fp, fp, i32, i32, i32, i32, vp]
    L.xsd_backward.argtypes = [vp, fp, fp, fp, vp]
    L.xsd_backward_num_stages.argtypes = [vp]
    L.xsd_backward_stage.argtypes = [vp, i32, fp, fp, fp, vp]
    L.xsd_grad_range.argtypes = [vp, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.xsd_l1_loss.argtypes = [vp, fp, fp, fp, fp, i64, vp]
    L.xsd_loss_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(vp)]
    L.xsd_loss_destroy.argtypes = [vp]
    L.xsd_loss_destroy.restype = None
    L.xsd_loss_eval.argtypes = [vp, fp, fp, fp, fp, i32, i32, i32, vp]
    L.xsd_loss_set_channels.argtypes = [vp, i32]
    L.xsd_ext_metrics_create.argtypes = [ctypes.POINTER(vp)]
    L.xsd_ext_metrics_destroy.argtypes = [vp]
    L.xsd_ext_metrics_destroy.restype = None
    L.xsd_ext_metrics_eval.argtypes = [vp, fp, fp, vp, i32, i32, i32, vp]
    L.xsd_fsim_create.argtypes = [ctypes.POINTER(vp)]
    L.xsd_fsim_destroy.argtypes = [vp]
    L.xsd_fsim_destroy.restype = None
    L.xsd_fsim_eval.argtypes = [vp, fp, fp, vp, i32, i32, i32, i32, vp]
    L.xsd_fsim_test_dft2.argtypes = [vp, fp, fp, i32, i32, i32, i32, vp]
    L.xsd_fsim_test_median.argtypes = [fp, fp, i32, i32, vp]
    L.xsd_ext_metrics_test_stage.argtypes = [vp, i32, i32, vp, i64, ctypes.POINTER(i32), vp]
    L.xsd_fsim_test_stage.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i32), vp]
    L.xsd_adam_step.argtypes = [vp, fp, fp, fp, fp, i64, i32, f32, f32, f32, f32, f32, vp]
    L.xsd_mask_pad_normalize.argtypes = [vp, i32, vp, fp, i32, i32, i32, i32, i32, f32, i32, vp]
    L.xsd_compose_input.argtypes = [vp, vp, vp, i32, i32, vp, fp, i32, i32, i32, i32, i32, i32, f32, i32, vp]
    L.xsd_compose_batch.argtypes = [vp, i32, i32, i64, i64, vp, vp, vp, vp, fp, i32, i32, i32, i32, i32, i32, f32, i32, vp]
    L.xsd_normalize.argtypes = [fp, fp, i64, f32, i32, i32, vp]
    L.xsd_image_upsample.argtypes = [fp, fp, i32, i32, i32, i32, vp]
    L.xsd_profile_enable.argtypes = [vp, i32]
    L.xsd_debug_stamps.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint64)]
    L.xsd_profile_read.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64),
                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.xsd_probe_mfma_stream.argtypes = [i32, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), vp]
    L.xsd_test_conv3x3.argtypes = [vp, ctypes.POINTER(vp), i32, fp, fp, ctypes.POINTER(vp), i32, f32, i32, i32, i32, vp]
    L.xsd_test_conv3x3_bwd.argtypes = [vp, ctypes.POINTER(vp), i32, fp, fp, ctypes.POINTER(vp), fp, fp, i32, i32, i32, vp]
    L.xsd_test_conv3x3_ex.argtypes = [vp, ctypes.POINTER(vp), i32, i32, fp, fp, ctypes.POINTER(XsdTestOut), i32, i32, ctypes.POINTER(f32), i32, i32, i32, vp]
    L.xsd_test_wgrad_ex.argtypes = [vp, ctypes.POINTER(vp), i32, ctypes.POINTER(vp), i32, i32, f32, i32, i32, i32, i32, i32, i32, fp, fp, i32, i32, i32, vp]
    ip = ctypes.POINTER(i32)
    L.xsd_test_wgrad_block.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), f32, fp, ctypes.POINTER(i64), ctypes.POINTER(i64), i32, i32, ip, i32, i32, i32, vp]
    L.xsd_test_edge_expand.argtypes = [vp, fp, i64, fp, i32, i32, i32, fp, fp, fp, f32, vp, i32, fp, i32, i32, i32, vp]
    L.xsd_test_edge_reduce.argtypes = [vp, fp, fp, i32, i32, i32, fp, fp, i64, fp, fp, i64, i32, fp, i32, i32, i32, vp]
    L.xsd_test_edge_wgrad.argtypes = [vp, fp, fp, i64, i32, fp, fp, i32, i32, ip, i32, i32, i32, vp]
    L.xsd_test_gconv.argtypes = [i32, i32, fp, i64, i32, ctypes.POINTER(XsdTestGconvArgs), i32, i32, i32, ip, vp]
    L.xsd_test_gwgrad.argtypes = [i32, i32, i64, fp, i64, fp, i64, fp, i32, i32, i32, ip, ip, vp]
    L.xsd_test_gop.argtypes = [i32, fp, i64, fp, i64, fp, i32, i32, i32, i32, f32, vp]
    L.xsd_test_gpack.argtypes = [i32, ip, ip, fp, fp, i64, fp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.xsd_loss_test_scale.argtypes = [vp, fp, fp, fp, fp, fp, i32, vp, ctypes.POINTER(f32), i32, i32, i32, vp]
    L.xsd_loss_test_pool2.argtypes = [fp, fp, fp, fp, i32, i32, i32, vp]
    L.xsd_test_clamp_bwd.argtypes = [fp, fp, fp, i64, vp]
    L.xsd_test_packed_region.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64), vp]
    L.xsd_test_pad_gather.argtypes = [vp, fp, fp, vp]
    L.xsd_test_add_channels.argtypes = [fp, fp, i32, i64, i32, vp]
    L.xsd_restormer_create.argtypes = [ctypes.POINTER(XsdRestormerConfig), ctypes.POINTER(vp)]
    L.xsd_restormer_destroy.argtypes = [vp]
    L.xsd_restormer_destroy.restype = None
    L.xsd_restormer_param_count.argtypes = [vp]
    L.xsd_restormer_param_count.restype = i64
    L.xsd_restormer_pack_weights.argtypes = [vp, fp, vp]
    L.xsd_restormer_forward.argtypes = [vp, fp, fp, i32, i32, i32, vp]
    L.xsd_swinfir_create.argtypes = [ctypes.POINTER(XsdSwinFIRConfig), ctypes.POINTER(vp)]
    L.xsd_swinfir_destroy.argtypes = [vp]
    L.xsd_swinfir_destroy.restype = None
    L.xsd_swinfir_param_count.argtypes = [vp]
    L.xsd_swinfir_param_count.restype = i64
    L.xsd_swinfir_pack_weights.argtypes = [vp, fp, vp]
    L.xsd_swinfir_forward.argtypes = [vp, fp, fp, i32, i32, i32, vp]
    L.xsd_swinfir_fft_supported.argtypes = [i32]
    L.xsd_swinfir_test_fft.argtypes = [vp, fp, fp, i32, i32, i32, i32, i32, vp]
    L.xsd_hat_create.argtypes = [ctypes.POINTER(XsdHATConfig), ctypes.POINTER(vp)]
    L.xsd_hat_destroy.argtypes = [vp]
    L.xsd_hat_destroy.restype = None
    L.xsd_hat_param_count.argtypes = [vp]
    L.xsd_hat_param_count.restype = i64
    L.xsd_hat_pack_weights.argtypes = [vp, fp, vp]
    L.xsd_hat_forward.argtypes = [vp, fp, fp, i32, i32, i32, vp]
    L.xsd_swinfir_set_math.argtypes = [vp, i32]
    L.xsd_swinfir_get_math.argtypes = [vp]
    L.xsd_hat_set_math.argtypes = [vp, i32]
    L.xsd_hat_get_math.argtypes = [vp]
    L.xsd_swinir_create.argtypes = [ctypes.POINTER(XsdSwinIRConfig), ctypes.POINTER(vp)]
    L.xsd_swinir_destroy.argtypes = [vp]
    L.xsd_swinir_destroy.restype = None
    L.xsd_swinir_param_count.argtypes = [vp]
    L.xsd_swinir_param_count.restype = i64
    L.xsd_swinir_pack_weights.argtypes = [vp, fp, vp]
    L.xsd_swinir_forward.argtypes = [vp, fp, fp, i32, i32, i32, vp]
    L.xsd_swinir_out_size.argtypes = [vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.xsd_swinir_set_math.argtypes = [vp, i32]
    L.xsd_swinir_get_math.argtypes = [vp]
    L.xsd_swinir_test_pad.argtypes = [fp, fp, i32, i32, i32, i32, i32, ctypes.POINTER(f32), f32, vp]
    L.xsd_swinir_test_nearest_conv.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, i32, f32, i32, vp]
    L.xsd_sw_test_gemm.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i64, i32, f32, i32, vp]
    L.xsd_sw_test_gemm_view.argtypes = [ctypes.POINTER(XsdSwGemmView), vp]
    L.xsd_swinir_test_gemm_view.argtypes = [ctypes.POINTER(XsdSwGemmView), vp]
    L.xsd_hat_test_ocab.argtypes = [fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    L.xsd_hat_test_channel_mean.argtypes = [fp, fp, i32, i64, i32, vp]
    L.xsd_sw_test_attention.argtypes = [fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    L.xsd_sw_test_layernorm.argtypes = [fp, fp, fp, fp, i64, i32, vp]
    L.xsd_hat_test_ca_combine.argtypes = [fp, fp, fp, fp, fp, fp, f32, i32, i64, i32, i32, fp, vp]
    L.xsd_restormer_test_pw.argtypes = [fp, i64, fp, i32, fp, i32, fp, fp, i32, fp, i64, i32, i32, i32, i64, vp]
    L.xsd_restormer_test_dw.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, i32, vp]
    L.xsd_restormer_test_attention.argtypes = [fp, fp, fp, fp, fp, i32, i32, i32, i64, vp]
    L.xsd_restormer_test_attention_wide.argtypes = [fp, fp, fp, fp, fp, i32, i32, i32, i64, vp]
    L.xsd_restormer_test_conv3.argtypes = [fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, vp]
    for n in ("linear", "conv3x3", "layernorm", "attention"):
        getattr(L, f"xsd_sw_op_{n}_scratch").restype = i64
    L.xsd_sw_op_linear_scratch.argtypes = [i64, i32, i32, i32, i64, i32]
    L.xsd_sw_op_linear_forward.argtypes = [fp, fp, fp, fp, fp, i64, i32, i32, i32, f32, i32, vp, i64, vp]
    L.xsd_sw_op_linear_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, i64, i32, i32, i32, f32, i32, i64, vp, i64, vp]
    L.xsd_sw_op_conv3x3_scratch.argtypes = [i32, i32, i32, i32, i32, i32, i64, i32]
    L.xsd_sw_op_conv3x3_forward.argtypes = [fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, f32, i32, vp, i64, vp]
    L.xsd_sw_op_conv3x3_backward.argtypes = [fp, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, f32, i32, i64, vp, i64, vp]
    L.xsd_sw_op_layernorm_forward.argtypes = [fp, fp, fp, fp, i64, i32, vp]
    L.xsd_sw_op_layernorm_scratch.argtypes = [i64, i32]
    L.xsd_sw_op_layernorm_backward.argtypes = [fp, fp, fp, fp, fp, fp, i64, i32, vp, i64, vp]
    L.xsd_sw_op_attention_forward.argtypes = [fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    L.xsd_sw_op_attention_scratch.argtypes = [i32, i32, i32, i32, i32, i32]
    L.xsd_sw_op_attention_backward.argtypes = [fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, f32, vp, i64, vp]
    _lib = L
    return L


# every symbol include/xsd.h declares (checked by tests/test_abi.py without a GPU)
ABI_SYMBOLS = [
    "xsd_last_error", "xsd_version", "xsd_create", "xsd_destroy", "xsd_param_count", "xsd_set_math", "xsd_get_math", "xsd_pack_weights",
    "xsd_forward", "xsd_backward", "xsd_backward_num_stages", "xsd_backward_stage", "xsd_grad_range",
    "xsd_l1_loss", "xsd_loss_create", "xsd_loss_destroy", "xsd_loss_eval", "xsd_loss_set_channels", "xsd_ext_metrics_create", "xsd_ext_metrics_destroy", "xsd_ext_metrics_eval", "xsd_ext_metrics_test_stage", "xsd_fsim_create", "xsd_fsim_destroy", "xsd_fsim_eval", "xsd_fsim_test_dft2", "xsd_fsim_test_median", "xsd_fsim_test_stage", "xsd_adam_step", "xsd_mask_pad_normalize", "xsd_compose_input", "xsd_compose_batch", "xsd_normalize", "xsd_image_upsample",
    "xsd_profile_enable", "xsd_profile_read", "xsd_probe_mfma_stream", "xsd_debug_stamps", "xsd_debug_persistent_grid", "xsd_debug_occupancy", "xsd_debug_residency_ms", "xsd_test_conv3x3", "xsd_test_conv3x3_bwd", "xsd_test_conv3x3_ex", "xsd_test_wgrad_ex", "xsd_test_wgrad_block",
    "xsd_test_edge_expand", "xsd_test_edge_reduce", "xsd_test_edge_wgrad", "xsd_test_gconv", "xsd_test_gwgrad", "xsd_test_gop", "xsd_test_gpack",
    "xsd_loss_test_scale", "xsd_loss_test_pool2", "xsd_test_clamp_bwd", "xsd_test_packed_region", "xsd_test_pad_gather", "xsd_test_add_channels",
    "xsd_restormer_create", "xsd_restormer_destroy", "xsd_restormer_param_count", "xsd_restormer_pack_weights", "xsd_restormer_forward",
    "xsd_swinfir_create", "xsd_swinfir_destroy", "xsd_swinfir_param_count", "xsd_swinfir_pack_weights", "xsd_swinfir_forward",
    "xsd_swinfir_fft_supported", "xsd_swinfir_test_fft", "xsd_swinfir_set_math", "xsd_swinfir_get_math", "xsd_sw_test_gemm",
    "xsd_sw_test_gemm_view", "xsd_swinir_test_gemm_view",
    "xsd_hat_create", "xsd_hat_destroy", "xsd_hat_param_count", "xsd_hat_pack_weights", "xsd_hat_forward", "xsd_hat_test_ocab",
    "xsd_hat_test_channel_mean", "xsd_hat_set_math", "xsd_hat_get_math",
    "xsd_sw_test_attention", "xsd_sw_test_layernorm", "xsd_hat_test_ca_combine",
    "xsd_swinir_create", "xsd_swinir_destroy", "xsd_swinir_param_count", "xsd_swinir_pack_weights", "xsd_swinir_forward",
    "xsd_swinir_out_size", "xsd_swinir_set_math", "xsd_swinir_get_math", "xsd_swinir_test_pad", "xsd_swinir_test_nearest_conv",
    "xsd_restormer_test_pw", "xsd_restormer_test_dw", "xsd_restormer_test_attention", "xsd_restormer_test_attention_wide", "xsd_restormer_test_conv3",
    "xsd_sw_op_linear_scratch", "xsd_sw_op_linear_forward", "xsd_sw_op_linear_backward", "xsd_sw_op_conv3x3_scratch", "xsd_sw_op_conv3x3_forward",
    "xsd_sw_op_conv3x3_backward", "xsd_sw_op_layernorm_forward", "xsd_sw_op_layernorm_scratch", "xsd_sw_op_layernorm_backward",
    "xsd_sw_op_attention_forward", "xsd_sw_op_attention_scratch", "xsd_sw_op_attention_backward",
]


def check(rc: int):
    if rc != 0:
        raise XsdError(f"libxsd_hip error {rc}: {load().xsd_last_error().decode()}")
