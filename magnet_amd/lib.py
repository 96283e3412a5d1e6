"""ctypes binding of libmagnet_hip.so (the C ABI in include/magnet_hip.h).

torch is used for device memory and streams only: every call passes `tensor.data_ptr()` and the
current HIP stream through the C boundary.  There is NO CPU fallback — if the library is missing,
or an argument lives on the CPU, the call raises.  torch must be imported before the library is
loaded so that libmagnet_hip.so binds to the same libamdhip64 (same SONAME) torch has loaded.

The binding is declared once: the constants, the argument-struct mirrors and `_PROTOS`, the prototype of every
entry point, which load() applies before it returns the handle.  tests/test_abi.py checks all three against the header.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch  # noqa: F401  (must precede CDLL: shares torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmagnet_hip.so")

# the enums and #defines of include/magnet_hip.h
FEAT_F32, FEAT_BF16 = 0, 1
# argument-error codes (positive return values; negative = -(hipError_t))
E_NULL, E_DIM, E_DTYPE, E_ALIGN, E_NODEVICE, E_SHAPE = 1, 2, 3, 4, 5, 6
MAX_CANDIDATES = 256
NLL_BLOCKS, NLL_MAX_ITER = 256, 16
BN_BLOCKS = 256
ACT_BASE, ACT_LEAKY_RELU, ACT_SILU = 0, 1, 2
TILING_FLAT, TILING_BM256, TILING_BM64 = 1, 2, 4
SPLITK_MAX, SPLITK_MIN_CHUNKS = 8, 2
METRICS_SIGMA, METRICS_VARIANCE, METRICS_NONE = 0, 1, 2
IMAGE_PREP_KMAX = 17                                             # taps per axis of magnet_image_prep_u8: downscale ratios up to 8


class MagnetError(RuntimeError):
    """code = the C ABI's return value when the error came from the library (None for host-side checks):
    E_SHAPE = "this kernel / output form does not take the shape" (the only condition callers may fall back on)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class MagnetCostVolumeArgs(ctypes.Structure):
    """Mirror of `struct MagnetCostVolumeArgs` (include/magnet_hip.h)."""
    _fields_ = [
        ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("F", ctypes.c_int32), ("D", ctypes.c_int32),
        ("h", ctypes.c_int32), ("w", ctypes.c_int32),
        ("kappa", ctypes.c_float), ("feat_dtype", ctypes.c_int32),
        ("ref_feat_cl", ctypes.c_void_p), ("src_feat_pad", ctypes.c_void_p),
        ("src_gmm_pad", ctypes.c_void_p), ("ref_gmm", ctypes.c_void_p),
        ("k_list", ctypes.c_void_p), ("d_volume", ctypes.c_void_p),
        ("poses", ctypes.c_void_p), ("is_valid", ctypes.c_void_p),
        ("intM", ctypes.c_void_p), ("rays", ctypes.c_void_p),
        ("cost", ctypes.c_void_p),
        ("path", ctypes.c_int32), ("stats", ctypes.c_void_p),
        ("cost_batch_stride", ctypes.c_int64),
        ("cost_hi", ctypes.c_void_p), ("cost_lo", ctypes.c_void_p), ("cost_ld", ctypes.c_int64),
        ("mode", ctypes.c_int32),
        ("gate_bits", ctypes.c_void_p),
        ("ray_params", ctypes.c_void_p),
        ("src_gmm_quad", ctypes.c_void_p),
        ("dev_flags", ctypes.c_uint32),
    ]


class MagnetConvArgs(ctypes.Structure):
    """Mirror of `struct MagnetConvArgs` (include/magnet_hip.h)."""
    _fields_ = [
        ("in_hi", ctypes.c_void_p), ("in_lo", ctypes.c_void_p), ("w_hi", ctypes.c_void_p), ("w_lo", ctypes.c_void_p),
        ("bias", ctypes.c_void_p), ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("out_f32", ctypes.c_void_p),
        ("rows", ctypes.c_int64),
        ("cin", ctypes.c_int32), ("cout_pad", ctypes.c_int32), ("taps", ctypes.c_int32), ("wp", ctypes.c_int32),
        ("relu", ctypes.c_int32), ("out_mode", ctypes.c_int32), ("in_ld", ctypes.c_int32),
        ("addend", ctypes.c_void_p), ("addend_ld", ctypes.c_int32),
        ("dil", ctypes.c_int32), ("out_ld", ctypes.c_int32),
        ("add_hi", ctypes.c_void_p), ("add_lo", ctypes.c_void_p), ("add_ld", ctypes.c_int32),
        ("border_hp", ctypes.c_int32), ("border_pad", ctypes.c_int32), ("repad", ctypes.c_int32),
        ("tail_w_hi", ctypes.c_void_p), ("tail_w_lo", ctypes.c_void_p), ("tail_bias", ctypes.c_void_p),
        ("tail_cout_pad", ctypes.c_int32),
        ("up_depth", ctypes.c_void_p), ("up_out", ctypes.c_void_p),
        ("up_npred", ctypes.c_int32), ("up_B", ctypes.c_int32), ("up_h", ctypes.c_int32), ("up_w", ctypes.c_int32),
        ("gu_in", ctypes.c_void_p), ("gu_out", ctypes.c_void_p),
    ]


class MagnetDepthMetricsArgs(ctypes.Structure):
    """Mirror of `struct MagnetDepthMetricsArgs` (include/magnet_hip.h)."""
    _fields_ = [("mu", ctypes.c_void_p), ("second", ctypes.c_void_p), ("gt", ctypes.c_void_p),
                ("mu_stride", ctypes.c_int64), ("second_stride", ctypes.c_int64),
                ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("kind", ctypes.c_int32),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float),
                ("crop", ctypes.c_int32), ("y0", ctypes.c_int32), ("y1", ctypes.c_int32), ("x0", ctypes.c_int32), ("x1", ctypes.c_int32),
                ("sums", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("work", ctypes.c_void_p)]


class MagnetNllArgs(ctypes.Structure):
    """Mirror of `struct MagnetNllArgs` (include/magnet_hip.h)."""
    _fields_ = [("preds", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("sums", ctypes.c_void_p),
                ("loss", ctypes.c_void_p), ("work", ctypes.c_void_p), ("grad_loss", ctypes.c_void_p), ("grad_preds", ctypes.c_void_p),
                ("gamma", ctypes.c_double),
                ("n_iter", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


class MagnetUpsampleBwdArgs(ctypes.Structure):
    """Mirror of `struct MagnetUpsampleBwdArgs` (include/magnet_hip.h)."""
    _fields_ = [("grad_up", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("grad_depth", ctypes.c_void_p), ("grad_mask", ctypes.c_void_p), ("work", ctypes.c_void_p),
                ("mask_sb", ctypes.c_int64), ("mask_sc", ctypes.c_int64), ("mask_sy", ctypes.c_int64), ("mask_sx", ctypes.c_int64),
                ("gm_sb", ctypes.c_int64), ("gm_sc", ctypes.c_int64), ("gm_sy", ctypes.c_int64), ("gm_sx", ctypes.c_int64),
                ("n_pred", ctypes.c_int32), ("B", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("k", ctypes.c_int32)]


class MagnetHeadDgradArgs(ctypes.Structure):
    """Mirror of `struct MagnetHeadDgradArgs` (include/magnet_hip.h)."""
    _fields_ = [("dout", ctypes.c_void_p), ("k0", ctypes.c_int32),
                ("wt_hi", ctypes.c_void_p), ("wt_lo", ctypes.c_void_p),
                ("h3_hi", ctypes.c_void_p), ("h2_hi", ctypes.c_void_p), ("h1_hi", ctypes.c_void_p),
                ("dout_hi", ctypes.c_void_p), ("dout_lo", ctypes.c_void_p),
                ("dh3_hi", ctypes.c_void_p), ("dh3_lo", ctypes.c_void_p), ("dh2_hi", ctypes.c_void_p), ("dh2_lo", ctypes.c_void_p),
                ("dh1_hi", ctypes.c_void_p), ("dh1_lo", ctypes.c_void_p),
                ("acc", ctypes.c_void_p), ("acc_hi", ctypes.c_void_p), ("acc_lo", ctypes.c_void_p), ("acc_mode", ctypes.c_int32),
                ("B", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("rows", ctypes.c_int64),
                ("grad_gmm", ctypes.c_void_p), ("gnet_out", ctypes.c_void_p), ("gmm_in", ctypes.c_void_p), ("gnet_ld", ctypes.c_int32)]


class MagnetWgradArgs(ctypes.Structure):
    """Mirror of `struct MagnetWgradArgs` (include/magnet_hip.h)."""
    _fields_ = [("dy_hi", ctypes.c_void_p), ("dy_lo", ctypes.c_void_p), ("x_hi", ctypes.c_void_p), ("x_lo", ctypes.c_void_p),
                ("dy_ld", ctypes.c_int64), ("x_ld", ctypes.c_int64), ("rows", ctypes.c_int64),
                ("cout", ctypes.c_int32), ("cin", ctypes.c_int32), ("taps", ctypes.c_int32), ("wp", ctypes.c_int32),
                ("grad_w", ctypes.c_void_p), ("grad_b", ctypes.c_void_p),
                ("cout_valid", ctypes.c_int32), ("cin_valid", ctypes.c_int32), ("cin_total", ctypes.c_int32), ("cin_dst", ctypes.c_int32),
                ("accumulate", ctypes.c_int32), ("work", ctypes.c_void_p)]


class MagnetBnTrainArgs(ctypes.Structure):
    """Mirror of `struct MagnetBnTrainArgs` (include/magnet_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("x_ld", ctypes.c_int64),
                ("N", ctypes.c_int32), ("hp", ctypes.c_int32), ("wp", ctypes.c_int32), ("pad", ctypes.c_int32), ("C", ctypes.c_int32),
                ("work", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p),
                ("running_mean", ctypes.c_void_p), ("running_var", ctypes.c_void_p), ("num_batches_tracked", ctypes.c_void_p),
                ("eps", ctypes.c_double), ("momentum", ctypes.c_double),
                ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("res_hi", ctypes.c_void_p), ("res_lo", ctypes.c_void_p), ("res_ld", ctypes.c_int64),
                ("relu", ctypes.c_int32),
                ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("out_f32", ctypes.c_void_p), ("out_ld", ctypes.c_int64)]


class MagnetWgradExArgs(ctypes.Structure):
    """Mirror of `struct MagnetWgradExArgs` (include/magnet_hip.h)."""
    _fields_ = [("base", MagnetWgradArgs), ("dil", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MagnetBnBwdArgs(ctypes.Structure):
    """Mirror of `struct MagnetBnBwdArgs` (include/magnet_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("x_ld", ctypes.c_int64),
                ("N", ctypes.c_int32), ("hp", ctypes.c_int32), ("wp", ctypes.c_int32), ("pad", ctypes.c_int32), ("C", ctypes.c_int32),
                ("relu", ctypes.c_int32),
                ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("g", ctypes.c_void_p), ("g_ld", ctypes.c_int64), ("work", ctypes.c_void_p),
                ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p),
                ("dx_hi", ctypes.c_void_p), ("dx_lo", ctypes.c_void_p), ("dx_ld", ctypes.c_int64)]


class MagnetSppBwdArgs(ctypes.Structure):
    """Mirror of `struct MagnetSppBwdArgs` (include/magnet_hip.h)."""
    _fields_ = [("g", ctypes.c_void_p), ("g_ld", ctypes.c_int64),
                ("N", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("pad", ctypes.c_int32), ("c_off", ctypes.c_int32),
                ("ph", ctypes.c_int32), ("pw", ctypes.c_int32),
                ("dq", ctypes.c_void_p), ("dpool", ctypes.c_void_p * 4), ("out", ctypes.c_void_p), ("out_ld", ctypes.c_int64)]


class MagnetConvExArgs(ctypes.Structure):
    """Mirror of `struct MagnetConvExArgs` (include/magnet_hip.h)."""
    _fields_ = [("base", MagnetConvArgs), ("act", ctypes.c_int32), ("act_slope", ctypes.c_float),
                ("tiling", ctypes.c_int32), ("tiles_out", ctypes.POINTER(ctypes.c_int64))]


class MagnetConvNchwArgs(ctypes.Structure):
    """Mirror of `struct MagnetConvNchwArgs` (include/magnet_hip.h)."""
    _fields_ = [("ex", MagnetConvExArgs), ("src", ctypes.c_void_p), ("src_c0", ctypes.c_int32), ("src_C", ctypes.c_int32)]


class MagnetFnetLossArgs(ctypes.Structure):
    """Mirror of `struct MagnetFnetLossArgs` (include/magnet_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("d", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("pred", ctypes.c_void_p),
                ("m", ctypes.c_void_p), ("rz", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("loss", ctypes.c_void_p),
                ("work", ctypes.c_void_p), ("grad_loss", ctypes.c_void_p), ("grad_x", ctypes.c_void_p),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float),
                ("B", ctypes.c_int32), ("D", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class MagnetDnetLossArgs(ctypes.Structure):
    """Mirror of `struct MagnetDnetLossArgs` (include/magnet_hip.h)."""
    _fields_ = [("depth", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("valid", ctypes.c_void_p),
                ("mask_sb", ctypes.c_int64), ("mask_sc", ctypes.c_int64), ("mask_sy", ctypes.c_int64), ("mask_sx", ctypes.c_int64),
                ("gm_sb", ctypes.c_int64), ("gm_sc", ctypes.c_int64), ("gm_sy", ctypes.c_int64), ("gm_sx", ctypes.c_int64),
                ("pred", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("loss", ctypes.c_void_p), ("work", ctypes.c_void_p),
                ("grad_loss", ctypes.c_void_p), ("grad_depth", ctypes.c_void_p), ("grad_mask", ctypes.c_void_p),
                ("B", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("k", ctypes.c_int32)]


class MagnetDnetNllArgs(ctypes.Structure):
    """Mirror of `struct MagnetDnetNllArgs` (include/magnet_hip.h)."""
    _fields_ = [("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("sums", ctypes.c_void_p),
                ("loss", ctypes.c_void_p), ("work", ctypes.c_void_p), ("grad_loss", ctypes.c_void_p), ("grad_pred", ctypes.c_void_p),
                ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


class MagnetGatherViewsArgs(ctypes.Structure):
    """Mirror of `struct MagnetGatherViewsArgs` (include/magnet_hip.h)."""
    _fields_ = [("slots", ctypes.c_void_p), ("n_slots", ctypes.c_int32),
                ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("F", ctypes.c_int32),
                ("feat_dtype", ctypes.c_int32),
                ("pool_feat", ctypes.c_void_p), ("pool_gmm", ctypes.c_void_p), ("pool_xd3_hi", ctypes.c_void_p), ("pool_xd3_lo", ctypes.c_void_p),
                ("ref_cl", ctypes.c_void_p), ("src_pad", ctypes.c_void_p), ("ref_gmm", ctypes.c_void_p), ("src_gmm", ctypes.c_void_p),
                ("gin_hi", ctypes.c_void_p), ("gin_lo", ctypes.c_void_p), ("gin_ld", ctypes.c_int64), ("gin_c_off", ctypes.c_int32)]


class MagnetScatterFramesArgs(ctypes.Structure):
    """Mirror of `struct MagnetScatterFramesArgs` (include/magnet_hip.h)."""
    _fields_ = [("slots", ctypes.c_void_p), ("n_slots", ctypes.c_int32),
                ("n", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("F", ctypes.c_int32), ("feat_dtype", ctypes.c_int32),
                ("feat", ctypes.c_void_p), ("gmm", ctypes.c_void_p), ("xd3_hi", ctypes.c_void_p), ("xd3_lo", ctypes.c_void_p),
                ("pool_feat", ctypes.c_void_p), ("pool_gmm", ctypes.c_void_p), ("pool_xd3_hi", ctypes.c_void_p), ("pool_xd3_lo", ctypes.c_void_p)]


class MagnetImagePrepArgs(ctypes.Structure):
    """Mirror of `struct MagnetImagePrepArgs` (include/magnet_hip.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("src_pitch", ctypes.c_int64), ("src_frame", ctypes.c_int64),
                ("coef_x", ctypes.c_void_p), ("bounds_x", ctypes.c_void_p), ("coef_y", ctypes.c_void_p), ("bounds_y", ctypes.c_void_p),
                ("lut", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("N", ctypes.c_int32), ("Hin", ctypes.c_int32), ("Win", ctypes.c_int32),
                ("crop_left", ctypes.c_int32), ("crop_top", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("Hout", ctypes.c_int32), ("Wout", ctypes.c_int32), ("kx", ctypes.c_int32), ("ky", ctypes.c_int32)]


class MagnetTrainPrepArgs(ctypes.Structure):
    """Mirror of `struct MagnetTrainPrepArgs` (include/magnet_hip.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("src_pitch", ctypes.c_int64), ("src_frame", ctypes.c_int64),
                ("coef_x", ctypes.c_void_p), ("bounds_x", ctypes.c_void_p), ("coef_y", ctypes.c_void_p), ("bounds_y", ctypes.c_void_p),
                ("luts", ctypes.c_void_p), ("frame_params", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("N", ctypes.c_int32), ("Hin", ctypes.c_int32), ("Win", ctypes.c_int32),
                ("crop_left", ctypes.c_int32), ("crop_top", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("Hres", ctypes.c_int32), ("Wres", ctypes.c_int32), ("Hout", ctypes.c_int32), ("Wout", ctypes.c_int32),
                ("kx", ctypes.c_int32), ("ky", ctypes.c_int32), ("n_luts", ctypes.c_int32)]


class MagnetDepthPrepArgs(ctypes.Structure):
    """Mirror of `struct MagnetDepthPrepArgs` (include/magnet_hip.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("src_pitch", ctypes.c_int64), ("src_frame", ctypes.c_int64),
                ("idx_x", ctypes.c_void_p), ("idx_y", ctypes.c_void_p), ("frame_params", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("N", ctypes.c_int32), ("Hin", ctypes.c_int32), ("Win", ctypes.c_int32),
                ("crop_left", ctypes.c_int32), ("crop_top", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("Hres", ctypes.c_int32), ("Wres", ctypes.c_int32), ("Hout", ctypes.c_int32), ("Wout", ctypes.c_int32),
                ("invalid_code", ctypes.c_int32), ("divisor", ctypes.c_float)]


class MagnetDwConvArgs(ctypes.Structure):
    """Mirror of `struct MagnetDwConvArgs` (include/magnet_hip.h)."""
    _fields_ = [("in_hi", ctypes.c_void_p), ("in_lo", ctypes.c_void_p), ("wgt", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("part", ctypes.c_void_p),
                ("N", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("c_pad", ctypes.c_int32),
                ("in_ld", ctypes.c_int32), ("out_ld", ctypes.c_int32), ("k", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("pad_top", ctypes.c_int32), ("pad_left", ctypes.c_int32), ("n_part", ctypes.c_int32)]


# (restype, argtypes) of every MAGNET_API declaration of include/magnet_hip.h, in header order; load() applies them all
_C, _L, _F, _I, _P, _S = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER
_PROTOS = {
    "magnet_version": (_C, []),
    "magnet_last_error": (ctypes.c_char_p, []),
    "magnet_device_count": (_C, []),
    "magnet_pack_features": (_C, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "magnet_pack_gmm": (_C, [_P, _P, _I, _I, _I, _P]),
    "magnet_pack_gmm_quad": (_C, [_P, _P, _I, _I, _I, _P]),
    "magnet_cost_volume_cw": (_C, [_S(MagnetCostVolumeArgs), _P]),
    "magnet_cost_volume_f_backward": (_C, [_S(MagnetCostVolumeArgs), _P, _P, _P, _P]),
    "magnet_make_rays": (_C, [_P, _P, _I, _I, _I, _P]),
    "magnet_relative_poses": (_C, [_P, _P, _P, _P, _I, _I, _P]),
    "magnet_cost_volume_f_backward_workspace": (_L, [_S(MagnetCostVolumeArgs)]),
    "magnet_cost_volume_f_backward_ws": (_C, [_S(MagnetCostVolumeArgs), _P, _P, _P, _P, _L, _P]),
    "magnet_gaussian_update": (_C, [_P, _P, _P, _I, _I, _P]),
    "magnet_upsample_depth": (_C, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "magnet_conv_mfma": (_C, [_S(MagnetConvArgs), _P]),
    "magnet_fnet_stem": (_C, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "magnet_space_to_depth": (_C, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "magnet_avgpool_cl": (_C, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "magnet_upsample_bilinear_cl": (_C, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "magnet_pack_split": (_C, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _P]),
    "magnet_gaussian_update_cl": (_C, [_P, _I, _P, _P, _I, _I, _I, _P]),
    "magnet_upsample_depth_cl": (_C, [_P, _P, _I, _P, _I, _I, _I, _P]),
    "magnet_upsample_depth_cl_n": (_C, [_P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "magnet_depth_metrics": (_C, [_P, _P, _P, _I, _I, _F, _F, _P]),
    "magnet_depth_metrics_crop": (_C, [_P, _P, _P, _I, _I, _I, _F, _F, _I, _I, _I, _I, _P]),
    "magnet_depth_metrics_workspace": (_L, [_I]),
    "magnet_depth_metrics_ex": (_C, [_S(MagnetDepthMetricsArgs), _P]),
    "magnet_nll_loss_forward": (_C, [_S(MagnetNllArgs), _P]),
    "magnet_nll_loss_backward": (_C, [_S(MagnetNllArgs), _P]),
    "magnet_upsample_depth_backward": (_C, [_S(MagnetUpsampleBwdArgs), _P]),
    "magnet_head_dgrad": (_C, [_S(MagnetHeadDgradArgs), _P]),
    "magnet_wgrad_workspace": (_L, [_S(MagnetWgradArgs)]),
    "magnet_wgrad": (_C, [_S(MagnetWgradArgs), _P]),
    "magnet_fnet_stem_raw": (_C, [_P, _P, _P, _I, _I, _I, _P]),
    "magnet_bn_train_stats": (_C, [_S(MagnetBnTrainArgs), _P]),
    "magnet_bn_train_apply": (_C, [_S(MagnetBnTrainArgs), _P]),
    "magnet_wgrad_ex_workspace": (_L, [_S(MagnetWgradExArgs)]),
    "magnet_wgrad_ex": (_C, [_S(MagnetWgradExArgs), _P]),
    "magnet_bn_train_backward": (_C, [_S(MagnetBnBwdArgs), _P]),
    "magnet_fnet_grad_pack": (_C, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "magnet_fnet_d2s_backward": (_C, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "magnet_spp_upsample_backward": (_C, [_S(MagnetSppBwdArgs), _P]),
    "magnet_spp_pool_backward": (_C, [_S(MagnetSppBwdArgs), _P]),
    "magnet_fnet_stem_wgrad": (_C, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "magnet_conv_mfma_ex": (_C, [_S(MagnetConvExArgs), _P]),
    "magnet_conv_mfma_nchw": (_C, [_S(MagnetConvNchwArgs), _P]),
    "magnet_conv_mfma_f16": (_C, [_S(MagnetConvExArgs), _P]),
    "magnet_conv_mfma_f16p": (_C, [_S(MagnetConvExArgs), _P]),
    "magnet_conv_mfma_splitk_workspace": (_L, [_S(MagnetConvExArgs), _I]),
    "magnet_conv_mfma_splitk": (_C, [_S(MagnetConvExArgs), _I, _P, _L, _P]),
    "magnet_conv_mfma_f16d": (_C, [_S(MagnetConvExArgs), _P]),
    "magnet_conv_mfma_f16d_splitk_workspace": (_L, [_S(MagnetConvExArgs), _I]),
    "magnet_conv_mfma_f16d_splitk": (_C, [_S(MagnetConvExArgs), _I, _P, _L, _P]),
    "magnet_conv_mfma_f16e": (_C, [_S(MagnetConvExArgs), _P]),
    "magnet_pack_f16": (_C, [_P, _P, _I, _I, _I, _I, _I, _I, _L, _P]),
    "magnet_planes_to_f16": (_C, [_P, _P, _I, _P, _I, _L, _I, _I, _P]),
    "magnet_fnet_stem_f16": (_C, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "magnet_space_to_depth_f16": (_C, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "magnet_avgpool_cl_f16": (_C, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "magnet_upsample_bilinear_cl_f16": (_C, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "magnet_conv_row_tiles": (_L, [_I, _I, _I, _I, _S(_I)]),
    "magnet_dnet_gauss_head": (_C, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "magnet_dnet_upsample_gauss": (_C, [_P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "magnet_enc_stem": (_C, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "magnet_dwconv_cl_parts": (_L, [_I, _I]),
    "magnet_dwconv_cl": (_C, [_S(MagnetDwConvArgs), _P]),
    "magnet_se_gate": (_C, [_P, _I, _L, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P]),
    "magnet_se_scale": (_C, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P]),
    "magnet_enc_stem_f16": (_C, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "magnet_dwconv_cl_f16": (_C, [_S(MagnetDwConvArgs), _P]),
    "magnet_se_scale_f16": (_C, [_P, _I, _P, _I, _I, _I, _I, _P, _I, _P]),
    "magnet_gather_views": (_C, [_S(MagnetGatherViewsArgs), _P]),
    "magnet_scatter_frames": (_C, [_S(MagnetScatterFramesArgs), _P]),
    "magnet_image_prep_u8": (_C, [_S(MagnetImagePrepArgs), _P]),
    "magnet_train_prep_u8": (_C, [_S(MagnetTrainPrepArgs), _P]),
    "magnet_depth_prep_u16": (_C, [_S(MagnetDepthPrepArgs), _P]),
    "magnet_fnet_loss_forward": (_C, [_S(MagnetFnetLossArgs), _P]),
    "magnet_fnet_loss_backward": (_C, [_S(MagnetFnetLossArgs), _P]),
    "magnet_bn_sync_moments": (_C, [_S(MagnetBnTrainArgs), _P, _P]),
    "magnet_bn_sync_merge": (_C, [_S(MagnetBnTrainArgs), _P, _I, _P, _P]),
    "magnet_bn_sync_backward_sums": (_C, [_S(MagnetBnBwdArgs), _P, _P]),
    "magnet_bn_sync_backward_apply": (_C, [_S(MagnetBnBwdArgs), _P, _I, _P, _P]),
    "magnet_dnet_loss_workspace": (_L, [_S(MagnetDnetLossArgs)]),
    "magnet_dnet_loss_forward": (_C, [_S(MagnetDnetLossArgs), _P]),
    "magnet_dnet_loss_backward": (_C, [_S(MagnetDnetLossArgs), _P]),
    "magnet_dnet_nll_forward": (_C, [_S(MagnetDnetNllArgs), _P]),
    "magnet_dnet_nll_backward": (_C, [_S(MagnetDnetNllArgs), _P]),
}
API_SYMBOLS = tuple(_PROTOS)

_lib = None


def use_dev_build():
    """tools/ only: bind to libmagnet_hip_dev.so (python -m magnet_amd.build --dev), the build that honours dev_flags and the
    MAGNET_* environment switches.  Must be called before the first load(); never called by the package itself."""
    global LIB_PATH
    if _lib is not None:
        raise MagnetError("use_dev_build() must be called before the library is loaded")
    LIB_PATH = os.path.join(_HERE, "libmagnet_hip_dev.so")


def load() -> ctypes.CDLL:
    """Load the library (once) and type every entry point.  Raises MagnetError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MagnetError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m magnet_amd.build` "
            "(or __graft_entry__.build()). magnet_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOS.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = load().magnet_last_error().decode("utf-8", "replace")
        raise MagnetError(f"{what} failed (rc={rc}): {msg}", code=rc)


def _dev(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise MagnetError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise MagnetError(f"{name} is on {t.device}; magnet_amd runs on the GPU only (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise MagnetError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise MagnetError(f"{name} must be contiguous")
    return t


def _bf16_ptr(t, name, contiguous=False):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.bfloat16 or (contiguous and not t.is_contiguous()):
        raise MagnetError(f"{name} must be a {'contiguous ' if contiguous else ''}bf16 GPU tensor")
    return t.data_ptr()


def _f16_ptr(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float16:
        raise MagnetError(f"{name} must be an fp16 GPU tensor")
    return t.data_ptr()


def _stream(t) -> ctypes.c_void_p:
    """The current HIP stream of a tensor's device (or of a torch.device)."""
    return ctypes.c_void_p(torch.cuda.current_stream(getattr(t, "device", t)).cuda_stream)


entry_log = None                # when set to a list: _launch appends the name of every entry point it calls (DNetMFMA.launch_log)


def _launch(name: str, on, *args):
    """Call the entry point `name` with `args` and, as its last argument, the current stream of `on` (a tensor or a
    torch.device), with that device current; a non-zero return raises MagnetError."""
    if entry_log is not None:
        entry_log.append(name)
    with torch.cuda.device(getattr(on, "device", on)):
        _check(getattr(load(), name)(*args, _stream(on)), name)


def _workspace(name: str, args, *more) -> int:
    """A `*_workspace` query: the bytes the call described by `args` (and `more`, the query's other arguments) needs; the library
    answers -(MAGNET_E_*) on bad arguments."""
    nbytes = int(getattr(load(), name)(ctypes.byref(args), *more))
    if nbytes < 0:
        _check(-nbytes, name)
    return nbytes


def feat_torch_dtype(feat_dtype: int):
    return torch.bfloat16 if feat_dtype == FEAT_BF16 else torch.float32


def feat_enum(dtype) -> int:
    if dtype in (torch.bfloat16, "bf16", "bfloat16", FEAT_BF16):
        return FEAT_BF16
    if dtype in (torch.float32, "fp32", "float32", FEAT_F32):
        return FEAT_F32
    raise MagnetError(f"unsupported feature storage dtype {dtype!r} (fp32 or bf16)")


def pack_features(feat_nchw: torch.Tensor, feat_dtype: int = FEAT_F32, pad: int = 0, out: torch.Tensor | None = None):
    """(N,F,h,w) fp32 NCHW -> (N,h+2*pad,w+2*pad,F) channel-last in fp32 or bf16 storage; pad=1 adds a
    one-texel zero border (the source-view layout of the matcher)."""
    x = _dev(feat_nchw, "feat_nchw", torch.float32)
    N, F, h, w = x.shape
    shape = (N, h + 2 * pad, w + 2 * pad, F)
    if out is None:
        out = torch.empty(shape, dtype=feat_torch_dtype(feat_dtype), device=x.device)
    else:
        _dev(out, "out", feat_torch_dtype(feat_dtype))
        if tuple(out.shape) != shape:
            raise MagnetError(f"out has shape {tuple(out.shape)}, expected {shape}")
    _launch("magnet_pack_features", x, x.data_ptr(), out.data_ptr(), N, F, h, w, feat_dtype, int(pad))
    return out


def _pack_gmm(name, channels, gmm_nchw, out):
    g = _dev(gmm_nchw, "gmm_nchw", torch.float32)
    N, two, h, w = g.shape
    if two != 2:
        raise MagnetError(f"gmm_nchw must be (N,2,h,w), got {tuple(g.shape)}")
    if out is None:
        out = torch.empty((N, h + 2, w + 2, channels), dtype=torch.float32, device=g.device)
    _launch(name, g, g.data_ptr(), _dev(out, "out", torch.float32).data_ptr(), N, h, w)
    return out


def pack_gmm(gmm_nchw: torch.Tensor, out: torch.Tensor | None = None):
    """(N,2,h,w) fp32 [mu,sigma] planes -> (N,h+2,w+2,2) interleaved with a zero border."""
    return _pack_gmm("magnet_pack_gmm", 2, gmm_nchw, out)


def pack_gmm_quad(gmm_nchw: torch.Tensor, out: torch.Tensor | None = None):
    """(N,2,h,w) fp32 [mu,sigma] planes -> (N,h+2,w+2,8): the zero-bordered map per quad origin in quad form
    (MagnetCostVolumeArgs.src_gmm_quad; the production matcher's bilinear (mu, sigma) samples are 3 fma each)."""
    return _pack_gmm("magnet_pack_gmm_quad", 8, gmm_nchw, out)


def cost_volume_cw(ref_feat_cl, src_feat_pad, src_gmm_pad, poses, is_valid, intM, rays, kappa,
                   ref_gmm=None, k_list=None, d_volume=None, out=None, path: int = 0, stats=None, out_split=None,
                   mode: int = 0, gate_bits=None, ray_params=None, src_gmm_quad=None, dev_flags: int = 0):
    """Launch the fused matching kernel.  All tensors on one GPU; see MagnetCostVolumeArgs.

    ref_feat_cl (B,h,w,F) from pack_features(pad=0); src_feat_pad (V*B,h+2,w+2,F) from
    pack_features(pad=1) (fp32 or bf16, same dtype); src_gmm_pad (V*B,h+2,w+2,2) from pack_gmm;
    poses (B,V,4,4), is_valid (B,V) int32, intM (B,3,3), rays (B,3,h*w).
    Either d_volume (B,D,h,w) or (ref_gmm (B,2,h,w), k_list: sequence of D python floats)."""
    r = _dev(ref_feat_cl, "ref_feat_cl")
    s = _dev(src_feat_pad, "src_feat_pad", r.dtype)
    fe = feat_enum(r.dtype)
    B, h, w, F = r.shape
    if s.shape[0] % B != 0 or tuple(s.shape[1:]) != (h + 2, w + 2, F):
        raise MagnetError(f"src_feat_pad shape {tuple(s.shape)} does not match ref_feat_cl {tuple(r.shape)} "
                          "(expected (V*B, h+2, w+2, F))")
    V = s.shape[0] // B
    a = MagnetCostVolumeArgs()
    a.B, a.V, a.F, a.h, a.w = B, V, F, h, w
    a.kappa = float(kappa)
    a.feat_dtype = fe
    a.ref_feat_cl, a.src_feat_pad = r.data_ptr(), s.data_ptr()
    a.mode = int(mode)
    if src_gmm_pad is None:
        if mode != 1 and src_gmm_quad is None:
            raise MagnetError("need src_gmm_pad (pack_gmm) or src_gmm_quad (pack_gmm_quad)")
        g = s                                                      # est_costvolume_F mode has no (mu,sigma) maps; or only the quad form is given
    else:
        g = _dev(src_gmm_pad, "src_gmm_pad", torch.float32)
        if tuple(g.shape) != (V * B, h + 2, w + 2, 2):
            raise MagnetError(f"src_gmm_pad shape {tuple(g.shape)}, expected {(V * B, h + 2, w + 2, 2)}")
        a.src_gmm_pad = g.data_ptr()
    keep = [r, s, g]
    kbuf = None
    if d_volume is not None:
        dv = _dev(d_volume, "d_volume", torch.float32)
        if dv.dim() != 4 or dv.shape[0] != B or tuple(dv.shape[2:]) != (h, w):
            raise MagnetError(f"d_volume shape {tuple(dv.shape)}, expected (B,D,h,w) = ({B},D,{h},{w})")
        D = dv.shape[1]
        a.d_volume = dv.data_ptr(); keep.append(dv)
    else:
        if k_list is None or (ref_gmm is None and mode != 1):
            raise MagnetError("need d_volume, or ref_gmm and k_list (mode 1: k_list = depth bins)")
        D = len(k_list)
        kbuf = (ctypes.c_double * D)(*[float(k) for k in k_list])
        a.k_list = ctypes.addressof(kbuf)
        if mode != 1:
            rg = _dev(ref_gmm, "ref_gmm", torch.float32)
            if tuple(rg.shape) != (B, 2, h, w):
                raise MagnetError(f"ref_gmm shape {tuple(rg.shape)}, expected {(B, 2, h, w)}")
            a.ref_gmm = rg.data_ptr(); keep.append(rg)
    a.D = D
    po = _dev(poses, "poses", torch.float32); iv = _dev(is_valid, "is_valid", torch.int32)
    K = _dev(intM, "intM", torch.float32)
    if rays is None and ray_params is None:
        raise MagnetError("need rays (B,3,h*w) or ray_params (B,8) float64")
    if rays is not None:
        ry = _dev(rays, "rays", torch.float32)
        if tuple(ry.shape) != (B, 3, h * w):
            raise MagnetError(f"rays shape {tuple(ry.shape)}, expected {(B, 3, h * w)}")
        a.rays = ry.data_ptr()
    else:
        ry = _dev(ray_params, "ray_params", torch.float64)                 # the kernel generates the rays (N4)
        if tuple(ry.shape) != (B, 8):
            raise MagnetError(f"ray_params shape {tuple(ry.shape)}, expected {(B, 8)}")
        a.ray_params = ry.data_ptr()
    if tuple(po.shape) != (B, V, 4, 4) or tuple(iv.shape) != (B, V) or tuple(K.shape) != (B, 3, 3):
        raise MagnetError("poses/is_valid/intM shape mismatch: "
                          f"{tuple(po.shape)} {tuple(iv.shape)} {tuple(K.shape)}")
    a.poses, a.is_valid, a.intM = po.data_ptr(), iv.data_ptr(), K.data_ptr()
    if out_split is not None:
        # (hi, lo, ld): split-bf16 planes of the conv kernel's zero-bordered channel-last buffer, written in place
        oh, ol, ld = out_split
        a.cost_hi, a.cost_lo, a.cost_ld = _bf16_ptr(oh, "out_split hi plane"), _bf16_ptr(ol, "out_split lo plane"), int(ld)
    elif out is None:
        out = torch.empty((B, D, h, w), dtype=torch.float32, device=r.device)
    else:
        # `out` may be the leading-D-channel slice of a larger (B, D+C, h, w) buffer (G-Net's input)
        if not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (B, D, h, w):
            raise MagnetError(f"out must be a float32 GPU tensor of shape {(B, D, h, w)}")
        if out.stride()[1:] != (h * w, w, 1) or (B > 1 and out.stride(0) < D * h * w):
            raise MagnetError(f"out strides {out.stride()} unsupported (need dense (D,h,w) frames)")
        a.cost_batch_stride = out.stride(0) if B > 1 else 0
    if out_split is None:
        a.cost = out.data_ptr()
    # `path` = 0..4; for the dev tools' convenience bits 8.. of the python argument are forwarded as dev_flags (ignored by the
    # product build of the library)
    a.path = int(path) & 0xff
    a.dev_flags = (int(path) >> 8) | int(dev_flags)
    if src_gmm_quad is not None:
        gq = _dev(src_gmm_quad, "src_gmm_quad", torch.float32)
        if tuple(gq.shape) != (V * B, h + 2, w + 2, 8):
            raise MagnetError(f"src_gmm_quad shape {tuple(gq.shape)}, expected {(V * B, h + 2, w + 2, 8)}")
        a.src_gmm_quad = gq.data_ptr(); keep.append(gq)
    if stats is not None:
        a.stats = _dev(stats, "stats").data_ptr()
    if gate_bits is not None:
        # debug output: (B,V,D,h,w) uint8 consistency-gate bits (zero it first: invalid views are not written)
        if not gate_bits.is_cuda or gate_bits.dtype != torch.uint8 or tuple(gate_bits.shape) != (B, V, D, h, w) \
                or not gate_bits.is_contiguous():
            raise MagnetError(f"gate_bits must be a contiguous uint8 GPU tensor of shape {(B, V, D, h, w)}")
        a.gate_bits = gate_bits.data_ptr()
    for t in (s, g, po, iv, K, ry):
        if t.device != r.device:
            raise MagnetError("all tensors must be on the same device")
    _launch("magnet_cost_volume_cw", r, ctypes.byref(a))
    return out


def cost_volume_f_backward(ref_feat_cl, src_feat_pad, poses, is_valid, intM, rays, d_center, grad_cost, path: int = 0,
                           stats=None, grad_ref=None, grad_src=None, workspace=None):
    """Gradients of the mode-1 volume (est_costvolume_F before its softmax) w.r.t. the two feature maps.

    Same tensors as the forward call (fp32 features) + grad_cost (B,D,h,w).  Returns
    (grad_ref_cl (B,h,w,F), grad_src_pad (V*B,h+2,w+2,F)), both fp32 channel-last.

    `path`: only its low byte selects the entry point.  Low byte 0 is magnet_cost_volume_f_backward_ws, the gather (deterministic;
    it stores every interior texel of grad_src_pad once and leaves the border alone, and falls back to the scatter kernels, which
    accumulate, when the workspace is short or the gather refuses the shape).  Any other low byte is
    magnet_cost_volume_f_backward, the scatter entry point: the LDS hash kernel when F % 32 == 0 and V <= 4, the per-item atomic
    kernel otherwise.  Bits 8 and up are forwarded as dev_flags exactly as cost_volume_cw does (the product build ignores them;
    the dev build: 0x1000 no gather, 0x2000 no gather and the per-item kernel, 0x4000 32-texel gather segments).

    `grad_ref` / `grad_src`: caller-owned output buffers of the shapes above (tests: views into guarded allocations).  The
    default is a fresh grad_ref and a zeroed grad_src; a caller's grad_src is used as it is (the scatter kernels add to it).
    `workspace`: a caller-owned uint8 buffer for the gather, or a function that is handed the number of bytes the library asks for
    and returns that buffer (it may be deliberately short: the call then takes the scatter fallback)."""
    r = _dev(ref_feat_cl, "ref_feat_cl", torch.float32)
    s = _dev(src_feat_pad, "src_feat_pad", torch.float32)
    B, h, w, F = r.shape
    if s.shape[0] % B != 0 or tuple(s.shape[1:]) != (h + 2, w + 2, F):
        raise MagnetError(f"src_feat_pad shape {tuple(s.shape)} does not match ref_feat_cl {tuple(r.shape)}")
    V = s.shape[0] // B
    D = len(d_center)
    g = _dev(grad_cost, "grad_cost", torch.float32)
    if tuple(g.shape) != (B, D, h, w):
        raise MagnetError(f"grad_cost shape {tuple(g.shape)}, expected {(B, D, h, w)}")
    po = _dev(poses, "poses", torch.float32); iv = _dev(is_valid, "is_valid", torch.int32)
    K = _dev(intM, "intM", torch.float32); ry = _dev(rays, "rays", torch.float32)
    if tuple(po.shape) != (B, V, 4, 4) or tuple(iv.shape) != (B, V) or tuple(K.shape) != (B, 3, 3) \
            or tuple(ry.shape) != (B, 3, h * w):
        raise MagnetError("poses/is_valid/intM/rays shape mismatch")
    a = MagnetCostVolumeArgs()
    a.B, a.V, a.F, a.D, a.h, a.w = B, V, F, D, h, w
    a.feat_dtype = FEAT_F32
    a.mode = 1
    a.path = int(path) & 0xff
    a.dev_flags = int(path) >> 8
    if stats is not None:
        a.stats = _dev(stats, "stats", torch.int32).data_ptr()       # [_, flushed texels, units merged in LDS, units sent to global atomics]
    a.ref_feat_cl, a.src_feat_pad = r.data_ptr(), s.data_ptr()
    kbuf = (ctypes.c_double * D)(*[float(k) for k in d_center])
    a.k_list = ctypes.addressof(kbuf)
    a.poses, a.is_valid, a.intM, a.rays = po.data_ptr(), iv.data_ptr(), K.data_ptr(), ry.data_ptr()
    grad_ref = torch.empty_like(r) if grad_ref is None else _dev(grad_ref, "grad_ref", torch.float32)
    grad_src = torch.zeros_like(s) if grad_src is None else _dev(grad_src, "grad_src", torch.float32)
    if grad_ref.shape != r.shape or grad_src.shape != s.shape:
        raise MagnetError(f"grad_ref / grad_src shapes {tuple(grad_ref.shape)} / {tuple(grad_src.shape)}, expected "
                          f"{tuple(r.shape)} / {tuple(s.shape)}")
    if grad_ref.device != r.device or grad_src.device != r.device:
        raise MagnetError("grad_ref / grad_src must be on the features' device")
    if a.path == 0:
        # gather path: deterministic, no atomics; workspace = projection terms + per-(view, bin, tile) bounding boxes
        if workspace is None or callable(workspace):
            nbytes = _workspace("magnet_cost_volume_f_backward_workspace", a)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=r.device) if workspace is None else workspace(nbytes)
        else:
            ws = workspace
        if ws.device != r.device:
            raise MagnetError("workspace must be on the features' device")
        nbytes = _dev(ws, "workspace", torch.uint8).numel()
        _launch("magnet_cost_volume_f_backward_ws", r, ctypes.byref(a), g.data_ptr(), grad_ref.data_ptr(), grad_src.data_ptr(),
                ws.data_ptr(), nbytes)
    else:
        _launch("magnet_cost_volume_f_backward", r, ctypes.byref(a), g.data_ptr(), grad_ref.data_ptr(), grad_src.data_ptr())
    return grad_ref, grad_src


def gaussian_update(gnet_out, gmm_in, out=None):
    """(B,2,h,w) G-Net output + previous [mu,sigma] -> new [mu,sigma] (MAGNET.py:60-69)."""
    o = _dev(gnet_out, "gnet_out", torch.float32); g = _dev(gmm_in, "gmm_in", torch.float32)
    if o.shape != g.shape or o.dim() != 4 or o.shape[1] != 2:
        raise MagnetError(f"gaussian_update: shapes {tuple(o.shape)} / {tuple(g.shape)}, expected (B,2,h,w)")
    if out is None:
        out = torch.empty_like(g)
    B, _, h, w = g.shape
    _launch("magnet_gaussian_update", g, o.data_ptr(), g.data_ptr(), _dev(out, "out", torch.float32).data_ptr(), B, h * w)
    return out


def upsample_depth(depth, up_mask, k: int, out=None):
    """Learned convex upsampling (MAGNET.py:15-27): (B,C,h,w),(B,9*k*k,h,w) -> (B,C,k*h,k*w)."""
    d = _dev(depth, "depth", torch.float32); m = _dev(up_mask, "up_mask", torch.float32)
    B, C, h, w = d.shape
    if tuple(m.shape) != (B, 9 * k * k, h, w):
        raise MagnetError(f"up_mask shape {tuple(m.shape)}, expected {(B, 9 * k * k, h, w)}")
    if out is None:
        out = torch.empty((B, C, k * h, k * w), dtype=torch.float32, device=d.device)
    _launch("magnet_upsample_depth", d, d.data_ptr(), m.data_ptr(), _dev(out, "out", torch.float32).data_ptr(), B, C, h, w, k)
    return out


# ---------------------------------------------------------------------------------------------------
# G-Net / mask-head convolutions on the matrix cores (include/magnet_hip.h: magnet_conv_mfma & friends)
# ---------------------------------------------------------------------------------------------------
# the routes of conv_mfma, by its `f16` value: (entry point, split-K entry point or None, workspace query or None); magnet_conv_mfma itself
# serves the default route when nothing needs the _ex struct.  A new route is one row here (and one case of launch_conv, conv_mfma.hip)
_CONV_ROUTES = {
    False: ("magnet_conv_mfma_ex", "magnet_conv_mfma_splitk", "magnet_conv_mfma_splitk_workspace"),
    True: ("magnet_conv_mfma_f16", None, None),
    "plane": ("magnet_conv_mfma_f16p", None, None),
    "wide": ("magnet_conv_mfma_f16d", "magnet_conv_mfma_f16d_splitk", "magnet_conv_mfma_f16d_splitk_workspace"),
    "enc": ("magnet_conv_mfma_f16e", None, None),
}


def conv_mfma(in_hi, in_lo, in_ld, cin, w_hi, w_lo, bias, taps, wp, relu, rows, out_hi=None, out_lo=None, out_f32=None,
              addend=None, dil=0, out_ld=0, add=None, border=None, repad=0, out_bf16=None, tail=None, upsample=None, gauss=None,
              leaky=None, tiling=None, f16=False, split_k=None, work=None, silu=False, src_nchw=None):
    """One convolution layer on the matrix cores.  in_hi/in_lo: bf16 tensors whose data_ptr is row 0 (possibly a
    channel-offset view of a wider buffer, `in_ld` = its row pitch in elements); weights (taps, cout_pad, cin) bf16.
    F-Net extras (include/magnet_hip.h): dil (3x3 dilation), out_ld (write a channel slice: out tensors may then be
    views), add = (hi, lo, ld) split-bf16 residual input, border = (hp, pad) zero the border outputs, repad (re-address
    interior rows to a grid with border repad-1), out_bf16 = single bf16 output plane.
    tail = (w_hi, w_lo, bias, cout_pad): the stack's three 1x1 successors fused into this launch (result in out_f32).
    upsample = (depths (n,B,2,h,w) fp32, outs (n,B,2,4h,4w) fp32): with tail cout_pad 144, the learned convex upsampling runs in
    the tail's last layer (models/MAGNET.py:15-27) and only `outs` is written.
    gauss = (gmm_in (B,2,h,w), gmm_out): with tail cout_pad 16 (G-Net's head) the Gaussian update of models/MAGNET.py:60-69 runs
    in the tail's last layer and only `gmm_out` is written.
    leaky = slope: LeakyReLU(slope) after bias instead of ReLU (magnet_conv_mfma_ex; relu must be False, no tail).
    silu = True: SiLU after bias / residual instead of ReLU (MAGNET_ACT_SILU, magnet_conv_mfma_ex only; relu must be False, no leaky, tail,
    f16 or split_k).
    tiling = TILING_* flags (magnet_conv_mfma_ex; tests and A/B runs).  Returns the number of row tiles launched when the launch went
    through magnet_conv_mfma_ex, else None.
    f16 = True: the single-plane fp16 operand format (magnet_conv_mfma_f16): in_hi / w_hi are fp16 tensors, in_lo / w_lo must be None;
    3x3 layers with cout_pad 128, a fused tail of 16 / 144 outputs or out_f32.  Always returns the row tile count.
    f16 = "plane": the same operand format, plane to plane (magnet_conv_mfma_f16p, the F-Net's launches): `add` = (fp16 plane, None, ld),
    the output is out_f16 (one fp16 plane, passed as out_hi with out_lo None), out_f32 or out_bf16; taps 1 / 4 / 9, cout_pad 32 / 64 /
    128, dil, border, repad and channel slices as in the default format; no tail, addend or leaky.
    split_k = S (2 .. SPLITK_MAX) with work = a float32 GPU tensor of at least conv_mfma_splitk_workspace(...) bytes: the split-K form
    (magnet_conv_mfma_splitk) of the plain bf16x3 layer, taps 1 / 9, cout_pad % 128 == 0, out_hi / out_lo or out_f32; not with f16, tail,
    addend or add.  Returns the row tile count.
    f16 = "wide": the same operand format, plane to plane at any cout_pad % 128 == 0 (magnet_conv_mfma_f16d, the D-Net decoder's plain
    layers): taps 1 / 9, relu or leaky, border, repad and channel slices; the output is out_f16 (passed as out_hi with out_lo None),
    out_f32 or the split-bf16 pair out_hi / out_lo; no tail, addend, add, dil or out_bf16.  split_k / work are allowed on this route
    (magnet_conv_mfma_f16d_splitk).  Returns the row tile count.
    f16 = "enc": the same operand format, plane to plane, for the EfficientNet encoder's 1x1 layers (magnet_conv_mfma_f16e): taps 1,
    cout_pad 32 / 64 / any multiple of 128, silu allowed, `add` = (fp16 plane, None, ld); the output is out_f16 (passed as out_hi with
    out_lo None) or out_f32; border, repad and channel slices; no relu, leaky, tail, addend, dil or out_bf16.  Returns the row tile count.
    src_nchw = (x (B, C, h, w) fp32 contiguous, c0): input channels [c0, c0 + C) with c0 + C == cin are read in place from x and split
    inside the kernel (magnet_conv_mfma_nchw: the fused-tail 3x3 launches on 256-row tiles under per-image tiling, nothing else); the
    planes hold channels [0, c0) and may be None when c0 == 0.  Returns the row tile count."""
    if src_nchw is not None:
        if f16 or split_k is not None or leaky is not None or silu:
            raise MagnetError("conv_mfma (src_nchw): the bf16x3 fused-tail launch only — not with f16, split_k, leaky or silu")
        _dev(src_nchw[0], "src_nchw", torch.float32)
        if src_nchw[0].dim() != 4:
            raise MagnetError("conv_mfma (src_nchw): src must be (B, C, h, w)")
    wide = isinstance(f16, str) and f16 == "wide"
    if split_k is not None:
        if (f16 and not wide) or tail is not None or addend is not None or add is not None:
            raise MagnetError("conv_mfma (split_k): the plain bf16x3 layer (or f16='wide') only — not with f16=True / 'plane', tail, addend or add")
        if isinstance(split_k, bool) or not isinstance(split_k, int):
            raise MagnetError(f"conv_mfma: split_k must be an int, got {split_k!r}")
        if not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous():
            raise MagnetError("conv_mfma (split_k): work must be a contiguous float32 GPU tensor")
    elif work is not None:
        raise MagnetError("conv_mfma: work goes with split_k")
    enc = isinstance(f16, str) and f16 == "enc"
    if silu and (relu or leaky is not None or tail is not None or (f16 and not enc) or split_k is not None):
        raise MagnetError("conv_mfma (silu): the bf16x3 layer (or f16='enc') without relu, leaky, tail or split_k")
    a = MagnetConvArgs()
    if f16 not in tuple(_CONV_ROUTES):
        raise MagnetError(f"conv_mfma: f16 must be False, True, 'plane', 'wide' or 'enc', got {f16!r}")
    entry, entry_splitk, _ = _CONV_ROUTES[f16]                          # the route, looked up once
    plane = isinstance(f16, str) and f16 == "plane"
    if wide and (tail is not None or addend is not None or add is not None or out_bf16 is not None or dil):
        raise MagnetError("conv_mfma (f16='wide'): the plain layer — no tail, addend, add, out_bf16 or dil")
    if plane and (tail is not None or addend is not None or out_lo is not None or (add is not None and add[1] is not None)):
        raise MagnetError("conv_mfma (f16='plane'): one fp16 plane per buffer — out_lo and add[1] must be None; no tail, no addend")
    if enc and (tail is not None or addend is not None or out_lo is not None or out_bf16 is not None or dil or relu or
                (add is not None and add[1] is not None)):
        raise MagnetError("conv_mfma (f16='enc'): one fp16 plane per buffer — out_lo and add[1] must be None; no relu, tail, addend, out_bf16 or dil")
    if f16:
        if in_lo is not None or w_lo is not None or (leaky is not None and not wide):
            raise MagnetError("conv_mfma (f16): one fp16 plane per operand — in_lo, w_lo and leaky (but for f16='wide') must be None")
        for t, n in ((in_hi, "in_hi"), (w_hi, "w_hi")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float16:
                raise MagnetError(f"conv_mfma (f16): {n} must be an fp16 GPU tensor")
    else:
        no_planes = src_nchw is not None and int(src_nchw[1]) == 0 and in_hi is None and in_lo is None
        for t, n in ((w_hi, "w_hi"), (w_lo, "w_lo")) if no_planes else ((in_hi, "in_hi"), (in_lo, "in_lo"), (w_hi, "w_hi"), (w_lo, "w_lo")):
            _bf16_ptr(t, f"conv_mfma: {n}")
    a.in_hi, a.w_hi = (in_hi.data_ptr() if in_hi is not None else None), w_hi.data_ptr()
    if not f16:
        a.in_lo, a.w_lo = (in_lo.data_ptr() if in_lo is not None else None), w_lo.data_ptr()
    a.bias = _dev(bias, "bias", torch.float32).data_ptr()
    a.rows, a.cin, a.cout_pad, a.taps, a.wp = int(rows), int(cin), int(w_hi.shape[1]), int(taps), int(wp)
    a.relu, a.in_ld = int(bool(relu)), int(in_ld)
    if addend is not None:
        a.addend, a.addend_ld = _dev(addend, "addend", torch.float32).data_ptr(), int(addend.shape[1])
    a.dil, a.out_ld, a.repad = int(dil), int(out_ld), int(repad)
    if add is not None and (plane or enc):
        a.add_hi, a.add_ld = _f16_ptr(add[0], "add (fp16 plane)"), int(add[2])
    elif add is not None:
        a.add_hi, a.add_lo, a.add_ld = _bf16_ptr(add[0], "add_hi"), _bf16_ptr(add[1], "add_lo"), int(add[2])
    if border is not None:
        a.border_hp, a.border_pad = int(border[0]), int(border[1])
    if tail is not None:
        a.tail_w_hi, a.tail_w_lo = _bf16_ptr(tail[0], "tail w_hi"), _bf16_ptr(tail[1], "tail w_lo")
        a.tail_bias, a.tail_cout_pad = _dev(tail[2], "tail bias", torch.float32).data_ptr(), int(tail[3])
    if gauss is not None:                                 # (gmm_in (B,2,h,w), gmm_out): Gaussian update behind G-Net's 16-channel fused tail
        gi, go = gauss
        if tail is None or gi.dim() != 4 or gi.shape[1] != 2 or go.shape != gi.shape:
            raise MagnetError("conv_mfma: gauss = (gmm_in (B,2,h,w), gmm_out (B,2,h,w)) with a fused tail")
        a.gu_in, a.gu_out = _dev(gi, "gmm_in", torch.float32).data_ptr(), _dev(go, "gmm_out", torch.float32).data_ptr()
        a.up_B, a.up_h, a.up_w = int(gi.shape[0]), int(gi.shape[2]), int(gi.shape[3])
        a.out_mode = 1
    elif upsample is not None:
        d, o = upsample
        if tail is None or d.dim() != 5 or d.shape[2] != 2 or tuple(o.shape) != (d.shape[0], d.shape[1], 2, 4 * d.shape[3], 4 * d.shape[4]):
            raise MagnetError("conv_mfma: upsample = (depths (n,B,2,h,w), outs (n,B,2,4h,4w)) with a fused tail")
        a.up_depth, a.up_out = _dev(d, "upsample depths", torch.float32).data_ptr(), _dev(o, "upsample outs", torch.float32).data_ptr()
        a.up_npred, a.up_B, a.up_h, a.up_w = int(d.shape[0]), int(d.shape[1]), int(d.shape[3]), int(d.shape[4])
        a.out_mode = 1
    elif out_f32 is not None:
        if not out_f32.is_cuda or out_f32.dtype != torch.float32:
            raise MagnetError("conv_mfma: out_f32 must be a float32 GPU tensor")
        a.out_mode, a.out_f32 = 1, out_f32.data_ptr()
    elif out_bf16 is not None:
        a.out_mode, a.out_hi = 2, _bf16_ptr(out_bf16, "out_bf16")
    elif plane or enc or (wide and out_lo is None):
        a.out_mode, a.out_hi = 3, _f16_ptr(out_hi, "out_hi (fp16 plane)")
    else:
        a.out_mode, a.out_hi, a.out_lo = 0, _bf16_ptr(out_hi, "out_hi"), _bf16_ptr(out_lo, "out_lo")
    if leaky is None and tiling is None and not f16 and split_k is None and not silu and src_nchw is None:
        _launch("magnet_conv_mfma", in_hi, ctypes.byref(a))
        return None
    tiles = ctypes.c_int64(0)
    if src_nchw is not None:
        src, c0 = src_nchw
        n = MagnetConvNchwArgs(ex=MagnetConvExArgs(base=a, act=ACT_BASE, tiling=int(tiling or 0), tiles_out=ctypes.pointer(tiles)),
                               src=src.data_ptr(), src_c0=int(c0), src_C=int(src.shape[1]))
        _launch("magnet_conv_mfma_nchw", src, ctypes.byref(n))
        return tiles.value
    x = MagnetConvExArgs(base=a, act=ACT_SILU if silu else (ACT_BASE if leaky is None else ACT_LEAKY_RELU), act_slope=float(leaky or 0.0),
                         tiling=int(tiling or 0), tiles_out=ctypes.pointer(tiles))
    more = () if split_k is None else (int(split_k), work.data_ptr(), work.numel() * 4)
    _launch(entry_splitk if more else entry, in_hi, ctypes.byref(x), *more)
    return tiles.value


def conv_mfma_splitk_workspace(rows, cin, cout_pad, taps, split_k, f16=False):
    """magnet_conv_mfma_splitk_workspace: the bytes of `work` for a split-K launch of this shape (split_k x rows x cout_pad fp32);
    MagnetError for a form the entry point refuses.  f16 = "wide": the query of magnet_conv_mfma_f16d_splitk (conv_mfma(f16="wide",
    split_k=...)).  Host arithmetic: needs the library, not a GPU."""
    if not (f16 is False or (isinstance(f16, str) and f16 == "wide")):
        raise MagnetError(f"conv_mfma_splitk_workspace: f16 must be False or 'wide', got {f16!r}")
    name = _CONV_ROUTES[f16][2]
    x = MagnetConvExArgs()
    x.base.rows, x.base.cin, x.base.cout_pad, x.base.taps, x.base.out_mode = int(rows), int(cin), int(cout_pad), int(taps), 1
    return _workspace(name, x, int(split_k))


def conv_row_tiles(n_img, h, wp, bm):
    """magnet_conv_row_tiles: (row tiles, tiles per image or 0 for flat tiling) of a launch over n_img zero-bordered (h + 2, wp) grids
    with bm-row tiles.  Host arithmetic: needs the library, not a GPU."""
    per = ctypes.c_int32(0)
    n = load().magnet_conv_row_tiles(int(n_img), int(h), int(wp), int(bm), ctypes.byref(per))
    return int(n), per.value


def _nchw_source(who, x_nchw):
    """The source of pack_split / pack_f16: a float32 GPU tensor (N,C,h,w) whose images are dense (a leading-channel slice of a
    wider NCHW tensor is).  Returns N, C, h, w and the in_img_stride argument: 0 (= dense) for one image, whose stride(0) is arbitrary."""
    if not x_nchw.is_cuda or x_nchw.dtype != torch.float32:
        raise MagnetError(f"{who}: input must be a float32 GPU tensor")
    N, C, h, w = x_nchw.shape
    if x_nchw.stride()[1:] != (h * w, w, 1):
        raise MagnetError(f"{who}: unsupported input strides {x_nchw.stride()}")
    return N, C, h, w, int(x_nchw.stride(0)) if N > 1 else 0


def pack_split(x_nchw, out_hi, out_lo, ctot, c_off):
    """fp32 (N,C,h,w) (dense, or a leading-channel slice of a wider NCHW tensor) -> interior of the split-bf16
    padded channel-last buffer (N,h+2,w+2,ctot), channels [c_off, c_off+C)."""
    N, C, h, w, img_stride = _nchw_source("pack_split", x_nchw)
    _launch("magnet_pack_split", x_nchw, x_nchw.data_ptr(), out_hi.data_ptr(), out_lo.data_ptr(), N, C, h, w, int(ctot), int(c_off), img_stride)


def pack_f16(x_nchw, out_f16, ctot, c_off):
    """fp32 (N,C,h,w) (dense, or a leading-channel slice of a wider NCHW tensor) -> channels [c_off, c_off+C) of the interior of the
    zero-bordered fp16 plane (N,h+2,w+2,ctot) of conv_mfma(f16=True).  Saturating round-to-nearest-even (include/magnet_hip.h)."""
    N, C, h, w, img_stride = _nchw_source("pack_f16", x_nchw)
    if not out_f16.is_cuda or out_f16.device != x_nchw.device or out_f16.dtype != torch.float16 or not out_f16.is_contiguous() or \
            out_f16.numel() < N * (h + 2) * (w + 2) * int(ctot):
        raise MagnetError(f"pack_f16: out_f16 must be a contiguous fp16 tensor on {x_nchw.device} with at least N (h+2) (w+2) ctot elements")
    _launch("magnet_pack_f16", x_nchw, x_nchw.data_ptr(), out_f16.data_ptr(), N, C, h, w, int(ctot), int(c_off), img_stride)


def planes_to_f16(in_hi, in_lo, out_f16, c0, c1):
    """Channels [c0, c1) of the split-bf16 planes in_hi / in_lo (rows, ld) -> the same channels of the fp16 plane out_f16 (rows, ld16):
    f16(hi + lo), every row.  c0, c1 multiples of 8."""
    for t, n in ((in_hi, "in_hi"), (in_lo, "in_lo")):
        _bf16_ptr(t, f"planes_to_f16: {n}", contiguous=True)
    if in_hi.dim() != 2 or in_lo.shape != in_hi.shape:
        raise MagnetError("planes_to_f16: in_hi / in_lo must be (rows, ld) planes of one shape")
    if not isinstance(out_f16, torch.Tensor) or out_f16.device != in_hi.device or out_f16.dtype != torch.float16 or out_f16.dim() != 2 or \
            not out_f16.is_contiguous() or out_f16.shape[0] != in_hi.shape[0]:
        raise MagnetError("planes_to_f16: out_f16 must be a contiguous fp16 (rows, ld16) plane on the inputs' device")
    _launch("magnet_planes_to_f16", in_hi, in_hi.data_ptr(), in_lo.data_ptr(), int(in_hi.shape[1]), out_f16.data_ptr(), int(out_f16.shape[1]),
            int(in_hi.shape[0]), int(c0), int(c1))


def gaussian_update_cl(gnet_out_pad, ld, gmm_in, h, w, out=None):
    g = _dev(gmm_in, "gmm_in", torch.float32)
    if out is None:
        out = torch.empty_like(g)
    _launch("magnet_gaussian_update_cl", g, _dev(gnet_out_pad, "gnet_out_pad", torch.float32).data_ptr(), int(ld), g.data_ptr(),
            out.data_ptr(), g.shape[0], h, w)
    return out


def upsample_depth_cl(depth, mask_pad, ld, out=None):
    d = _dev(depth, "depth", torch.float32)
    B, C, h, w = d.shape
    if C != 2:
        raise MagnetError("upsample_depth_cl: depth must be (B,2,h,w)")
    if out is None:
        out = torch.empty((B, 2, 4 * h, 4 * w), dtype=torch.float32, device=d.device)
    _launch("magnet_upsample_depth_cl", d, d.data_ptr(), _dev(mask_pad, "mask_pad", torch.float32).data_ptr(), int(ld), out.data_ptr(),
            B, h, w)
    return out


def upsample_depth_cl_n(depths, mask_pad, ld):
    """Every prediction of the refinement loop upsampled with the same mask in ONE launch (models/MAGNET.py:173): `depths` is a
    list of (B,2,h,w) tensors; returns the list of (B,2,4h,4w) outputs (contiguous slices of one buffer)."""
    if len(depths) == 1:
        return [upsample_depth_cl(depths[0], mask_pad, ld)]
    d = torch.stack([_dev(x, "depth", torch.float32) for x in depths])
    n, B, C, h, w = d.shape
    if C != 2:
        raise MagnetError("upsample_depth_cl_n: depths must be (B,2,h,w)")
    out = torch.empty((n, B, 2, 4 * h, 4 * w), dtype=torch.float32, device=d.device)
    _launch("magnet_upsample_depth_cl_n", d, d.data_ptr(), _dev(mask_pad, "mask_pad", torch.float32).data_ptr(), int(ld), out.data_ptr(),
            n, B, h, w)
    return [out[i] for i in range(n)]


def make_rays(ray_params, h: int, w: int):
    """(B,8) float64 GPU {fx, fy, cx, cy, sx, sy, left, top} -> unit_ray_array_2D (B,3,h*w) fp32 on the device, bit-identical to
    the loaders' host table (dataloader_scannet.py:139-147, dataloader_kitti.py:113-118)."""
    prm = _dev(ray_params, "ray_params", torch.float64)
    if prm.dim() != 2 or prm.shape[1] != 8:
        raise MagnetError(f"ray_params shape {tuple(prm.shape)}, expected (B, 8)")
    B = prm.shape[0]
    out = torch.empty((B, 3, h * w), dtype=torch.float32, device=prm.device)
    _launch("magnet_make_rays", prm, prm.data_ptr(), out.data_ptr(), B, int(h), int(w))
    return out


def relative_poses(ext_ref, ext_nghbr):
    """utils.data_preprocess on the device (utils/utils.py:72-98): float64 GPU extrinsics ext_ref (B,4,4), ext_nghbr (B,V,4,4) ->
    (poses (B,V,4,4) fp32, is_valid (B,V) int32), both on the device, ready for the matcher."""
    er = _dev(ext_ref, "ext_ref", torch.float64); en = _dev(ext_nghbr, "ext_nghbr", torch.float64)
    if er.dim() != 3 or tuple(er.shape[1:]) != (4, 4) or en.dim() != 4 or en.shape[0] != er.shape[0] or tuple(en.shape[2:]) != (4, 4):
        raise MagnetError(f"relative_poses: shapes {tuple(er.shape)} {tuple(en.shape)}, expected (B,4,4) and (B,V,4,4)")
    B, V = en.shape[:2]
    poses = torch.empty((B, V, 4, 4), dtype=torch.float32, device=er.device)
    valid = torch.empty((B, V), dtype=torch.int32, device=er.device)
    _launch("magnet_relative_poses", er, er.data_ptr(), en.data_ptr(), poses.data_ptr(), valid.data_ptr(), B, V)
    return poses, valid


# ---- F-Net non-GEMM layers (row N3) -------------------------------------------------------------------------------
def fnet_stem(img, wgt, bias, out_hi, out_lo):
    """(N,3,H,W) fp32 image -> 32-channel split planes (N,H2+2,W2+2,32): 3x3/s2 conv + folded BN + ReLU (F_psmnet.py:40)."""
    x = _dev(img, "img", torch.float32)
    N, C, H, W = x.shape
    if C != 3:
        raise MagnetError(f"fnet_stem: expected 3 input channels, got {C}")
    _launch("magnet_fnet_stem", x, x.data_ptr(), _dev(wgt, "wgt", torch.float32).data_ptr(), _dev(bias, "bias", torch.float32).data_ptr(),
            _bf16_ptr(out_hi, "out_hi"), _bf16_ptr(out_lo, "out_lo"), N, H, W)


def space_to_depth(in_hi, in_lo, out_hi, out_lo, N, C, H2, W2, opad):
    _launch("magnet_space_to_depth", in_hi, _bf16_ptr(in_hi, "in_hi"), _bf16_ptr(in_lo, "in_lo"), _bf16_ptr(out_hi, "out_hi"),
            _bf16_ptr(out_lo, "out_lo"), N, C, H2, W2, opad)


def avgpool_cl(in_hi, in_lo, ld, N, h, w, pad, k, C, out_hi, out_lo):
    _launch("magnet_avgpool_cl", in_hi, _bf16_ptr(in_hi, "in_hi"), _bf16_ptr(in_lo, "in_lo"), ld, N, h, w, pad, k, C,
            _bf16_ptr(out_hi, "out_hi"), _bf16_ptr(out_lo, "out_lo"))


def upsample_bilinear_cl(x, in_ld, ph, pw, C, out_hi, out_lo, out_ld, N, h, w, pad):
    _launch("magnet_upsample_bilinear_cl", x, _dev(x, "x", torch.float32).data_ptr(), in_ld, ph, pw, C, _bf16_ptr(out_hi, "out_hi"),
            _bf16_ptr(out_lo, "out_lo"), out_ld, N, h, w, pad)


# the same four on the single-plane fp16 format (FNetMFMA(precision="fp16")): one fp16 plane wherever the above take a (hi, lo) pair
def fnet_stem_f16(img, wgt, bias, out):
    x = _dev(img, "img", torch.float32)
    N, C, H, W = x.shape
    if C != 3:
        raise MagnetError(f"fnet_stem_f16: expected 3 input channels, got {C}")
    _launch("magnet_fnet_stem_f16", x, x.data_ptr(), _dev(wgt, "wgt", torch.float32).data_ptr(), _dev(bias, "bias", torch.float32).data_ptr(),
            _f16_ptr(out, "out"), N, H, W)


def space_to_depth_f16(x, out, N, C, H2, W2, opad):
    _launch("magnet_space_to_depth_f16", x, _f16_ptr(x, "in"), _f16_ptr(out, "out"), N, C, H2, W2, opad)


def avgpool_cl_f16(x, ld, N, h, w, pad, k, C, out):
    _launch("magnet_avgpool_cl_f16", x, _f16_ptr(x, "in"), ld, N, h, w, pad, k, C, _f16_ptr(out, "out"))


def upsample_bilinear_cl_f16(x, in_ld, ph, pw, C, out, out_ld, N, h, w, pad):
    _launch("magnet_upsample_bilinear_cl_f16", x, _dev(x, "x", torch.float32).data_ptr(), in_ld, ph, pw, C, _f16_ptr(out, "out"), out_ld,
            N, h, w, pad)


# ---- training step of g_net / mask_head (include/magnet_hip.h: magnet_nll_loss_*, magnet_upsample_depth_backward,
# ---- magnet_head_dgrad, magnet_wgrad; csrc/train_bwd.hip) -----------------------------------------------------------
def nll_loss_forward(preds, gt, mask, gamma: float):
    """preds (I,B,2,H,W) fp32, gt (B,H,W) fp32, mask (B,H,W) bool -> (loss 0-d fp32, sums (1+I) float64: count, per-iteration
    NLL sums).  Deterministic two-stage reduction on the device."""
    p = _dev(preds, "preds", torch.float32)
    g = _dev(gt, "gt", torch.float32)
    m = _dev(mask, "mask", torch.bool)
    I, B, C, H, W = p.shape
    if C != 2 or tuple(g.shape) != (B, H, W) or tuple(m.shape) != (B, H, W):
        raise MagnetError(f"nll_loss: shapes {tuple(p.shape)} {tuple(g.shape)} {tuple(m.shape)}, expected (I,B,2,H,W), (B,H,W), (B,H,W)")
    if not 1 <= I <= NLL_MAX_ITER:
        raise MagnetError(f"nll_loss: 1 <= n_iter <= {NLL_MAX_ITER}, got {I}")
    sums = torch.empty(1 + I, dtype=torch.float64, device=p.device)
    work = torch.empty(NLL_BLOCKS * (1 + I), dtype=torch.float64, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    a = MagnetNllArgs(preds=p.data_ptr(), gt=g.data_ptr(), mask=m.data_ptr(), sums=sums.data_ptr(), loss=loss.data_ptr(),
                      work=work.data_ptr(), gamma=float(gamma), n_iter=I, B=B, H=H, W=W)
    _launch("magnet_nll_loss_forward", p, ctypes.byref(a))
    return loss, sums


def nll_loss_backward(preds, gt, mask, sums, grad_loss, gamma: float):
    """d loss / d preds (I,B,2,H,W), scaled by the device scalar grad_loss (read on the device: no host sync)."""
    p = _dev(preds, "preds", torch.float32)
    gl = _dev(grad_loss.reshape(()), "grad_loss", torch.float32)
    I, B, _, H, W = p.shape
    out = torch.empty_like(p)
    a = MagnetNllArgs(preds=p.data_ptr(), gt=_dev(gt, "gt", torch.float32).data_ptr(), mask=_dev(mask, "mask", torch.bool).data_ptr(),
                      sums=_dev(sums, "sums", torch.float64).data_ptr(), grad_loss=gl.data_ptr(), grad_preds=out.data_ptr(),
                      gamma=float(gamma), n_iter=I, B=B, H=H, W=W)
    _launch("magnet_nll_loss_backward", p, ctypes.byref(a))
    return out


def _fnet_loss_args(raw, d, who):
    x = _dev(raw, "raw_volume", torch.float32)
    dc = _dev(d, "d_center", torch.float32)
    if x.dim() != 4 or dc.dim() != 1 or dc.shape[0] != x.shape[1] or dc.device != x.device:
        raise MagnetError(f"{who}: raw_volume {tuple(x.shape)} / d_center {tuple(dc.shape)}, expected (B,D,h,w) and (D) on one device")
    B, D, h, w = x.shape
    if not 1 <= D <= MAX_CANDIDATES:
        raise MagnetError(f"{who}: 1 <= D <= {MAX_CANDIDATES}, got {D}")
    return x, MagnetFnetLossArgs(x=x.data_ptr(), d=dc.data_ptr(), B=B, D=D, h=h, w=w)


def fnet_loss_forward(raw_volume, d_center, gt=None, min_depth: float = 0.0, max_depth: float = 0.0):
    """raw_volume (B,D,h,w) fp32 (the mode-1 matcher's output), d_center (D) fp32 on the device.  gt None -> pred (B,h,w), the expected
    depth sum_j softmax(raw)_j d_j.  gt (B,h,w) fp32 -> (loss 0-d fp32, pred, m, rz, sums (2) float64: valid count, sum |pred - gt|)
    with valid = gt > min_depth and not gt > max_depth; m, rz, sums are what fnet_loss_backward reads.  Deterministic reduction."""
    x, a = _fnet_loss_args(raw_volume, d_center, "fnet_loss_forward")
    B, D, h, w = x.shape
    pred = torch.empty((B, h, w), dtype=torch.float32, device=x.device)
    a.pred = pred.data_ptr()
    if gt is None:
        _launch("magnet_fnet_loss_forward", x, ctypes.byref(a))
        return pred
    g = _dev(gt, "gt", torch.float32)
    if tuple(g.shape) != (B, h, w) or g.device != x.device:
        raise MagnetError(f"fnet_loss_forward: gt shape {tuple(g.shape)}, expected {(B, h, w)} on {x.device}")
    m, rz = torch.empty_like(pred), torch.empty_like(pred)
    sums = torch.empty(2, dtype=torch.float64, device=x.device)
    work = torch.empty(NLL_BLOCKS * 2, dtype=torch.float64, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    a.gt, a.m, a.rz, a.sums, a.loss, a.work = g.data_ptr(), m.data_ptr(), rz.data_ptr(), sums.data_ptr(), loss.data_ptr(), work.data_ptr()
    a.min_depth, a.max_depth = float(min_depth), float(max_depth)
    _launch("magnet_fnet_loss_forward", x, ctypes.byref(a))
    return loss, pred, m, rz, sums


def fnet_loss_backward(raw_volume, d_center, gt, pred, m, rz, sums, grad_loss, min_depth: float, max_depth: float, out=None):
    """d loss / d raw_volume (B,D,h,w), scaled by the device scalar grad_loss (read on the device: no host sync).  Every element of the
    result is written (`out`: a contiguous fp32 buffer of that shape to write into)."""
    x, a = _fnet_loss_args(raw_volume, d_center, "fnet_loss_backward")
    B, D, h, w = x.shape
    gl = _dev(grad_loss.reshape(()), "grad_loss", torch.float32)
    if out is None:
        out = torch.empty_like(x)
    elif tuple(_dev(out, "out", torch.float32).shape) != tuple(x.shape):
        raise MagnetError(f"fnet_loss_backward: out shape {tuple(out.shape)}, expected {tuple(x.shape)}")
    for t, name in ((gt, "gt"), (pred, "pred"), (m, "m"), (rz, "rz")):
        if tuple(_dev(t, name, torch.float32).shape) != (B, h, w):
            raise MagnetError(f"fnet_loss_backward: {name} shape {tuple(t.shape)}, expected {(B, h, w)}")
    a.gt, a.pred, a.m, a.rz = gt.data_ptr(), pred.data_ptr(), m.data_ptr(), rz.data_ptr()
    a.sums, a.grad_loss, a.grad_x = _dev(sums, "sums", torch.float64).data_ptr(), gl.data_ptr(), out.data_ptr()
    a.min_depth, a.max_depth = float(min_depth), float(max_depth)
    _launch("magnet_fnet_loss_backward", x, ctypes.byref(a))
    return out


def _dnet_loss_args(depth, mask, gt, valid, mask_layout, who):
    """The checked operands of the fused DnetLoss tail and a MagnetDnetLossArgs with the inputs filled.  mask: NCHW (B,144,h,w)
    logits of any strides (a channel-last plane passes as it is: only the element strides differ), or with mask_layout = (element
    offset, sb, sc, sy, sx) contiguous fp32 storage addressed through it."""
    d = _dev(depth, "depth", torch.float32)
    if d.dim() != 4 or d.shape[1] != 2:
        raise MagnetError(f"{who}: depth {tuple(d.shape)}, expected (B,2,h,w)")
    B, _, h, w = d.shape
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.float32:
        raise MagnetError(f"{who}: mask must be a float32 GPU tensor (magnet_amd has no CPU fallback)")
    if mask_layout is None:
        if tuple(mask.shape) != (B, 144, h, w):
            raise MagnetError(f"{who}: mask shape {tuple(mask.shape)}, expected {(B, 144, h, w)}")
        mask_layout = (0,) + tuple(mask.stride())
    else:
        _dev(mask, "mask", torch.float32)
    g = _dev(gt, "gt", torch.float32)
    v = _dev(valid, "valid", torch.bool)
    if tuple(g.shape) != (B, 4 * h, 4 * w) or tuple(v.shape) != (B, 4 * h, 4 * w):
        raise MagnetError(f"{who}: gt {tuple(g.shape)} / valid {tuple(v.shape)}, expected {(B, 4 * h, 4 * w)}")
    if any(t.device != d.device for t in (mask, g, v)):
        raise MagnetError(f"{who}: depth, mask, gt and valid must be on one device")
    mo, sb, sc, sy, sx = mask_layout
    a = MagnetDnetLossArgs(depth=d.data_ptr(), mask=mask.data_ptr() + 4 * mo, gt=g.data_ptr(), valid=v.data_ptr(), mask_sb=sb, mask_sc=sc,
                           mask_sy=sy, mask_sx=sx, B=B, h=h, w=w, k=4)
    return d, a


def dnet_loss_forward(depth, mask, gt, valid, mask_layout=None, pred=True):
    """The fused tail of the stand-alone D-Net's training step: depth (B,2,h,w) fp32 raw head output [mu, v], mask the 144 logits
    per coarse pixel, gt (B,4h,4w) fp32, valid (B,4h,4w) bool -> (loss 0-d fp32, sums (2) float64: valid count and NLL sum,
    pred (B,2,4h,4w) [mu, var] or None with pred=False).  Deterministic reduction; nothing waits for the device."""
    d, a = _dnet_loss_args(depth, mask, gt, valid, mask_layout, "dnet_loss_forward")
    B, _, h, w = d.shape
    out = torch.empty((B, 2, 4 * h, 4 * w), dtype=torch.float32, device=d.device) if pred else None
    sums = torch.empty(2, dtype=torch.float64, device=d.device)
    loss = torch.empty((), dtype=torch.float32, device=d.device)
    work = torch.empty(_workspace("magnet_dnet_loss_workspace", a) // 8 + 1, dtype=torch.float64, device=d.device)
    a.pred, a.sums, a.loss, a.work = (out.data_ptr() if pred else None), sums.data_ptr(), loss.data_ptr(), work.data_ptr()
    _launch("magnet_dnet_loss_forward", d, ctypes.byref(a))
    return loss, sums, out


def dnet_loss_backward(depth, mask, gt, valid, sums, grad_loss, mask_layout=None, grad_mask=None, grad_mask_layout=None):
    """(grad_depth (B,2,h,w), grad_mask) of the fused tail, scaled by the device scalar grad_loss (read on the device: no host sync).
    grad_mask: by default a fresh tensor of the mask's shape and strides; or a preallocated contiguous fp32 buffer addressed by
    grad_mask_layout = (element offset, sb, sc, sy, sx).  All 144 channels of every pixel are written."""
    d, a = _dnet_loss_args(depth, mask, gt, valid, mask_layout, "dnet_loss_backward")
    gl = _dev(grad_loss.reshape(()), "grad_loss", torch.float32)
    if grad_mask is None:
        if mask_layout is not None:
            raise MagnetError("dnet_loss_backward: mask_layout needs grad_mask and grad_mask_layout")
        grad_mask = torch.empty_like(mask)                                  # preserve_format: the mask's own dense strides
        if not grad_mask.is_contiguous() and not grad_mask.is_contiguous(memory_format=torch.channels_last):
            grad_mask = torch.empty(mask.shape, dtype=torch.float32, device=d.device)
        grad_mask_layout = (0,) + tuple(grad_mask.stride())
    elif grad_mask_layout is None:
        raise MagnetError("dnet_loss_backward: grad_mask needs grad_mask_layout")
    else:
        _dev(grad_mask, "grad_mask", torch.float32)
    gd = torch.empty_like(d)
    work = torch.empty(_workspace("magnet_dnet_loss_workspace", a) // 8 + 1, dtype=torch.float64, device=d.device)
    go, gsb, gsc, gsy, gsx = grad_mask_layout
    a.gm_sb, a.gm_sc, a.gm_sy, a.gm_sx = gsb, gsc, gsy, gsx
    a.sums, a.work, a.grad_loss = _dev(sums, "sums", torch.float64).data_ptr(), work.data_ptr(), gl.data_ptr()
    a.grad_depth, a.grad_mask = gd.data_ptr(), grad_mask.data_ptr() + 4 * go
    _launch("magnet_dnet_loss_backward", d, ctypes.byref(a))
    return gd, grad_mask


def _dnet_nll_args(pred, gt, valid, who):
    p = _dev(pred, "pred", torch.float32)
    g = _dev(gt, "gt", torch.float32)
    v = _dev(valid, "valid", torch.bool)
    if p.dim() != 4 or p.shape[1] != 2 or tuple(g.shape) != (p.shape[0],) + tuple(p.shape[2:]) or tuple(v.shape) != tuple(g.shape):
        raise MagnetError(f"{who}: shapes {tuple(p.shape)} {tuple(g.shape)} {tuple(v.shape)}, expected (B,2,H,W), (B,H,W), (B,H,W)")
    B, _, H, W = p.shape
    return p, MagnetDnetNllArgs(pred=p.data_ptr(), gt=g.data_ptr(), valid=v.data_ptr(), B=B, H=H, W=W)


def dnet_nll_forward(pred, gt, valid):
    """The reference's own DnetLoss call: pred (B,2,H,W) fp32 [mu, var], gt (B,H,W) fp32, valid (B,H,W) bool -> (loss 0-d fp32,
    sums (2) float64: valid count, NLL sum); var < 1e-10 counts as 1e-10."""
    p, a = _dnet_nll_args(pred, gt, valid, "dnet_nll_forward")
    sums = torch.empty(2, dtype=torch.float64, device=p.device)
    work = torch.empty(NLL_BLOCKS * 2, dtype=torch.float64, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    a.sums, a.loss, a.work = sums.data_ptr(), loss.data_ptr(), work.data_ptr()
    _launch("magnet_dnet_nll_forward", p, ctypes.byref(a))
    return loss, sums


def dnet_nll_backward(pred, gt, valid, sums, grad_loss):
    """d loss / d pred (B,2,H,W) of dnet_nll_forward, scaled by the device scalar grad_loss; no var gradient where the clamp applied."""
    p, a = _dnet_nll_args(pred, gt, valid, "dnet_nll_backward")
    gl = _dev(grad_loss.reshape(()), "grad_loss", torch.float32)
    out = torch.empty_like(p)
    a.sums, a.grad_loss, a.grad_pred = _dev(sums, "sums", torch.float64).data_ptr(), gl.data_ptr(), out.data_ptr()
    _launch("magnet_dnet_nll_backward", p, ctypes.byref(a))
    return out


def upsample_depth_backward(grad_up, depths, mask, k: int, mask_layout=None, grad_mask=None, grad_mask_layout=None):
    """Backward of the convex upsampling for n predictions sharing one mask.  grad_up (n,B,2,kh,kw), depths (n,B,2,h,w) ->
    (grad_depths (n,B,2,h,w), grad_mask = the mask's gradient summed over the predictions).  mask: NCHW (B,9k^2,h,w) logits
    (layouts None: grad_mask is returned in that layout), or contiguous fp32 storage addressed by mask_layout = (element offset,
    sb, sc, sy, sx), with a preallocated contiguous grad_mask addressed by grad_mask_layout (the padded channel-last buffers of the
    HIP training path)."""
    gu = _dev(grad_up, "grad_up", torch.float32)
    d = _dev(depths, "depths", torch.float32)
    n, B, C, h, w = d.shape
    if C != 2 or tuple(gu.shape) != (n, B, 2, k * h, k * w):
        raise MagnetError(f"upsample_depth_backward: shapes {tuple(gu.shape)} / {tuple(d.shape)} (k = {k})")
    m = _dev(mask, "mask", torch.float32)
    if mask_layout is None:
        if tuple(m.shape) != (B, 9 * k * k, h, w):
            raise MagnetError(f"upsample_depth_backward: mask shape {tuple(m.shape)}, expected {(B, 9 * k * k, h, w)}")
        grad_mask = torch.zeros_like(m)
        mask_layout = grad_mask_layout = (0, 9 * k * k * h * w, h * w, w, 1)
    elif grad_mask is None or grad_mask_layout is None:
        raise MagnetError("upsample_depth_backward: mask_layout needs grad_mask and grad_mask_layout")
    gm = _dev(grad_mask, "grad_mask", torch.float32)
    gd = torch.empty_like(d)
    work = torch.empty(n * B * 2 * 9 * h * w, dtype=torch.float32, device=d.device)
    mo, msb, msc, msy, msx = mask_layout
    go, gsb, gsc, gsy, gsx = grad_mask_layout
    a = MagnetUpsampleBwdArgs(grad_up=gu.data_ptr(), depth=d.data_ptr(), mask=m.data_ptr() + 4 * mo, grad_depth=gd.data_ptr(),
                              grad_mask=gm.data_ptr() + 4 * go, work=work.data_ptr(), mask_sb=msb, mask_sc=msc, mask_sy=msy,
                              mask_sx=msx, gm_sb=gsb, gm_sc=gsc, gm_sy=gsy, gm_sx=gsx, n_pred=n, B=B, h=h, w=w, k=int(k))
    _launch("magnet_upsample_depth_backward", d, ctypes.byref(a))
    return gd, grad_mask


def head_dgrad(a: "MagnetHeadDgradArgs", device):
    _launch("magnet_head_dgrad", device, ctypes.byref(a))


def _wgrad_args(dy_hi, dy_lo, x_hi, x_lo, rows, wp, taps, cout, cin, grad_w, cin_dst, cout_valid, cin_valid, grad_b=None,
                accumulate=False):
    """MagnetWgradArgs of wgrad / wgrad_ex, without the workspace."""
    planes = [_bf16_ptr(t, n) for t, n in ((dy_hi, "dy_hi"), (dy_lo, "dy_lo"), (x_hi, "x_hi"), (x_lo, "x_lo"))]
    gw = _dev(grad_w, "grad_w", torch.float32)
    return MagnetWgradArgs(dy_hi=planes[0], dy_lo=planes[1], x_hi=planes[2], x_lo=planes[3],
                           dy_ld=dy_hi.stride(0), x_ld=x_hi.stride(0), rows=int(rows), cout=int(cout), cin=int(cin), taps=int(taps),
                           wp=int(wp), grad_w=gw.data_ptr(),
                           grad_b=_dev(grad_b, "grad_b", torch.float32).data_ptr() if grad_b is not None else None,
                           cout_valid=int(cout if cout_valid is None else cout_valid), cin_valid=int(cin if cin_valid is None else cin_valid),
                           cin_total=gw.shape[1], cin_dst=int(cin_dst), accumulate=int(bool(accumulate)))


def wgrad(dy_hi, dy_lo, x_hi, x_lo, rows, wp, taps, cout, cin, grad_w, cin_dst=0, cout_valid=None, cin_valid=None, grad_b=None,
          accumulate=False):
    """Weight (and bias) gradient of one convolution layer on the matrix cores.  dy_* (rows, dy_ld) and x_* (rows, x_ld) split
    bf16 planes of the zero-bordered grid (x_* may be a channel-offset view of a wider buffer); grad_w: the layer's
    nn.Conv2d-shaped fp32 gradient (Cout, Cin_total, kh, kw), written at input channels [cin_dst, cin_dst + cin_valid)."""
    a = _wgrad_args(dy_hi, dy_lo, x_hi, x_lo, rows, wp, taps, cout, cin, grad_w, cin_dst, cout_valid, cin_valid, grad_b, accumulate)
    work = torch.empty(max(_workspace("magnet_wgrad_workspace", a) // 4, 4), dtype=torch.float32, device=grad_w.device)
    a.work = work.data_ptr()
    _launch("magnet_wgrad", grad_w, ctypes.byref(a))


# ---- F-Net forward in training mode (include/magnet_hip.h: magnet_fnet_stem_raw, magnet_bn_train_*; csrc/train_fnet_fwd.hip) ----
def fnet_stem_raw(img, wgt, out):
    """(N,3,H,W) fp32 image, wgt (32, 27) fp32 -> the interior of `out`, the fp32 (N*(H2+2)*(W2+2), 32) channel-last grid:
    firstconv.0 without BatchNorm and ReLU."""
    x = _dev(img, "img", torch.float32)
    N, C, H, W = x.shape
    if C != 3:
        raise MagnetError(f"fnet_stem_raw: expected 3 input channels, got {C}")
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    o = _dev(out, "out", torch.float32)
    if o.numel() < N * (H2 + 2) * (W2 + 2) * 32:
        raise MagnetError("fnet_stem_raw: output grid too small")
    _launch("magnet_fnet_stem_raw", x, x.data_ptr(), _dev(wgt, "wgt", torch.float32).data_ptr(), o.data_ptr(), N, H, W)


def bn_train(x, grid, mean, invstd, work, gamma, beta, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None,
             res=None, relu=False, out=None, out_f32=None, stats=True):
    """One BatchNorm2d in training mode (magnet_bn_train_stats, then magnet_bn_train_apply).  x: fp32 (rows, x_ld) grid
    (possibly a channel-offset view), grid = (N, hp, wp, pad, C); res = (hi, lo) split residual views; out = (hi, lo) split
    planes (channel-slice views allowed) or out_f32 an fp32 (rows, ld) tensor.  momentum None: cumulative average."""
    N, hp, wp, pad, C = (int(v) for v in grid)
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < C:
        raise MagnetError("bn_train: x must be a (rows, >= C) float32 GPU tensor with unit channel stride")
    a = MagnetBnTrainArgs(x=x.data_ptr(), x_ld=x.stride(0), N=N, hp=hp, wp=wp, pad=pad, C=C,
                          work=_dev(work, "work", torch.float64).data_ptr(), mean=_dev(mean, "mean", torch.float32).data_ptr(),
                          invstd=_dev(invstd, "invstd", torch.float32).data_ptr(), eps=float(eps),
                          momentum=-1.0 if momentum is None else float(momentum),
                          gamma=_dev(gamma, "gamma", torch.float32).data_ptr(), beta=_dev(beta, "beta", torch.float32).data_ptr(),
                          relu=int(bool(relu)))
    if work.numel() < BN_BLOCKS * C * 2:
        raise MagnetError("bn_train: workspace too small")
    for t, n in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            setattr(a, n, _dev(t, n, torch.float32).data_ptr())
    if num_batches_tracked is not None:
        a.num_batches_tracked = _dev(num_batches_tracked, "num_batches_tracked", torch.int64).data_ptr()
    if res is not None:
        a.res_hi, a.res_lo, a.res_ld = _bf16_ptr(res[0], "res_hi"), _bf16_ptr(res[1], "res_lo"), res[0].stride(0)
    if out_f32 is not None:
        a.out_f32, a.out_ld = _dev(out_f32, "out_f32", torch.float32).data_ptr(), out_f32.stride(0)
    elif out is not None:
        a.out_hi, a.out_lo, a.out_ld = _bf16_ptr(out[0], "out_hi"), _bf16_ptr(out[1], "out_lo"), out[0].stride(0)
    rows = N * hp * wp
    if x.shape[0] < rows or (out_f32 is not None and out_f32.shape[0] < rows) or (out is not None and out[0].shape[0] < rows) or \
            (res is not None and res[0].shape[0] < rows):
        raise MagnetError(f"bn_train: a buffer holds fewer than the grid's {rows} rows")
    if stats:
        _launch("magnet_bn_train_stats", x, ctypes.byref(a))
    if out is not None or out_f32 is not None:
        _launch("magnet_bn_train_apply", x, ctypes.byref(a))


# ---- F-Net backward in training mode (include/magnet_hip.h; csrc/train_fnet_bwd.hip, csrc/train_bwd.hip) ----
def wgrad_ex(dy_hi, dy_lo, x_hi, x_lo, rows, wp, taps, cout, cin, grad_w, dil=1, cin_dst=0, cout_valid=None, cin_valid=None):
    """magnet_wgrad with dilation (taps 9), the space-to-depth 2x2 window (taps 4, grad_w (Cout, Cin, 2, 2)) or taps 1."""
    a = MagnetWgradExArgs(base=_wgrad_args(dy_hi, dy_lo, x_hi, x_lo, rows, wp, taps, cout, cin, grad_w, cin_dst, cout_valid, cin_valid),
                          dil=int(dil))
    for t, n in ((dy_hi, "dy"), (x_hi, "x")):
        if t.shape[0] < rows:
            raise MagnetError(f"wgrad_ex: {n} holds fewer than {rows} rows")
    work = torch.empty(max(_workspace("magnet_wgrad_ex_workspace", a) // 4, 4), dtype=torch.float32, device=grad_w.device)
    a.base.work = work.data_ptr()
    _launch("magnet_wgrad_ex", grad_w, ctypes.byref(a))


def _bn_bwd_args(who, x, grid, mean, invstd, gamma, beta, relu, g, work, dgamma=None, dbeta=None, dx=None):
    """The MagnetBnBwdArgs of one BatchNorm backward launch, with the buffer-size checks; dgamma / dbeta / dx as the launch takes them."""
    N, hp, wp, pad, C = (int(v) for v in grid)
    rows = N * hp * wp
    for t, n in ((x, "x"), (g, "g")):
        if not t.is_cuda or t.dtype != torch.float32 or t.stride(1) != 1 or t.shape[0] < rows or t.shape[1] < C:
            raise MagnetError(f"{who}: {n} must be a (>= {rows}, >= {C}) float32 GPU tensor with unit channel stride")
    if (dx is not None and dx[0].shape[0] < rows) or work.numel() < (BN_BLOCKS * 2 + 2) * C:
        raise MagnetError(f"{who}: dx or the workspace too small")
    a = MagnetBnBwdArgs(x=x.data_ptr(), x_ld=x.stride(0), N=N, hp=hp, wp=wp, pad=pad, C=C, relu=int(bool(relu)),
                        mean=_dev(mean, "mean", torch.float32).data_ptr(), invstd=_dev(invstd, "invstd", torch.float32).data_ptr(),
                        gamma=_dev(gamma, "gamma", torch.float32).data_ptr(), beta=_dev(beta, "beta", torch.float32).data_ptr(),
                        g=g.data_ptr(), g_ld=g.stride(0), work=_dev(work, "work", torch.float64).data_ptr())
    if dgamma is not None:
        a.dgamma, a.dbeta = _dev(dgamma, "dgamma", torch.float32).data_ptr(), _dev(dbeta, "dbeta", torch.float32).data_ptr()
    if dx is not None:
        a.dx_hi, a.dx_lo, a.dx_ld = _bf16_ptr(dx[0], "dx_hi"), _bf16_ptr(dx[1], "dx_lo"), dx[0].stride(0)
    return a


def bn_train_backward(x, grid, mean, invstd, gamma, beta, relu, g, dgamma, dbeta, dx, work):
    """BatchNorm2d backward (batch statistics).  x: the saved fp32 pre-BN grid; g: fp32 gradient grid (views allowed, unit channel
    stride); dx = (hi, lo) split planes written over the whole grid."""
    a = _bn_bwd_args("bn_train_backward", x, grid, mean, invstd, gamma, beta, relu, g, work, dgamma, dbeta, dx)
    _launch("magnet_bn_train_backward", x, ctypes.byref(a))


# ---- synchronised BatchNorm (include/magnet_hip.h: magnet_bn_sync_*): the launches before and after the caller's all-gather ----
def _f64_buf(t, name, numel):
    if _dev(t, name, torch.float64).numel() < numel:
        raise MagnetError(f"{name} holds fewer than {numel} doubles")
    return t.data_ptr()


def bn_sync_moments(x, grid, work, record):
    """This rank's (n, mean, M2) per channel over the interior of the grid (as bn_train's x and grid) -> record, fp64 (3, C)."""
    N, hp, wp, pad, C = (int(v) for v in grid)
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < C:
        raise MagnetError("bn_sync_moments: x must be a (rows, >= C) float32 GPU tensor with unit channel stride")
    if x.shape[0] < N * hp * wp:
        raise MagnetError(f"bn_sync_moments: x holds fewer than the grid's {N * hp * wp} rows")
    a = MagnetBnTrainArgs(x=x.data_ptr(), x_ld=x.stride(0), N=N, hp=hp, wp=wp, pad=pad, C=C, work=_f64_buf(work, "work", BN_BLOCKS * C * 2))
    _launch("magnet_bn_sync_moments", x, ctypes.byref(a), _f64_buf(record, "record", 3 * C))


def bn_sync_merge(records, C, mean, invstd, n_tot, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None):
    """records: fp64 (world, 3, C), the ranks' bn_sync_moments records in rank order -> the global mean, invstd (fp32 (C)) and
    n_tot (fp64, one element), and the running-statistics update of bn_train with the global count.  momentum None: cumulative."""
    C = int(C)
    if not isinstance(records, torch.Tensor) or records.dim() != 3 or tuple(records.shape[1:]) != (3, C):
        raise MagnetError(f"bn_sync_merge: records must be (world, 3, {C})")
    world = records.shape[0]
    a = MagnetBnTrainArgs(C=C, mean=_dev(mean, "mean", torch.float32).data_ptr(), invstd=_dev(invstd, "invstd", torch.float32).data_ptr(),
                          eps=float(eps), momentum=-1.0 if momentum is None else float(momentum))
    if mean.numel() < C or invstd.numel() < C:
        raise MagnetError("bn_sync_merge: mean / invstd hold fewer than C values")
    for t, n in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            if t.numel() < C:
                raise MagnetError(f"bn_sync_merge: {n} holds fewer than C values")
            setattr(a, n, _dev(t, n, torch.float32).data_ptr())
    if num_batches_tracked is not None:
        a.num_batches_tracked = _dev(num_batches_tracked, "num_batches_tracked", torch.int64).data_ptr()
    _launch("magnet_bn_sync_merge", records, ctypes.byref(a), _f64_buf(records, "records", world * 3 * C), world, _f64_buf(n_tot, "n_tot", 1))


def bn_sync_backward_sums(x, grid, mean, invstd, gamma, beta, relu, g, dgamma, dbeta, work, sums):
    """This rank's (sum g', sum g' xhat) per channel, xhat from the global mean / invstd -> sums, fp64 (2, C); dgamma / dbeta get
    the same local sums.  Arguments as bn_train_backward."""
    a = _bn_bwd_args("bn_sync_backward_sums", x, grid, mean, invstd, gamma, beta, relu, g, work, dgamma, dbeta)
    _launch("magnet_bn_sync_backward_sums", x, ctypes.byref(a), _f64_buf(sums, "sums", 2 * a.C))


def bn_sync_backward_apply(x, grid, mean, invstd, gamma, beta, relu, g, dx, work, sums, n_tot):
    """sums: fp64 (world, 2, C), the ranks' bn_sync_backward_sums in rank order; n_tot: bn_sync_merge's -> dx = (hi, lo) split
    planes over the whole grid of this rank."""
    a = _bn_bwd_args("bn_sync_backward_apply", x, grid, mean, invstd, gamma, beta, relu, g, work, dx=dx)
    if not isinstance(sums, torch.Tensor) or sums.dim() != 3 or tuple(sums.shape[1:]) != (2, a.C):
        raise MagnetError(f"bn_sync_backward_apply: sums must be (world, 2, {a.C})")
    world = sums.shape[0]
    _launch("magnet_bn_sync_backward_apply", x, ctypes.byref(a), _f64_buf(sums, "sums", world * 2 * a.C), world, _f64_buf(n_tot, "n_tot", 1))


def fnet_grad_pack(g_nchw, out_hi, out_lo, pad):
    g = _dev(g_nchw, "grad", torch.float32)
    N, C, h, w = g.shape
    ld = out_hi.shape[1]
    if out_hi.shape[0] < N * (h + 2 * pad) * (w + 2 * pad) or not out_hi.is_contiguous() or out_lo.shape != out_hi.shape:
        raise MagnetError("fnet_grad_pack: output planes too small")
    _launch("magnet_fnet_grad_pack", g, g.data_ptr(), _bf16_ptr(out_hi, "out_hi"), _bf16_ptr(out_lo, "out_lo"), N, C, h, w, int(pad), int(ld))


def fnet_d2s_backward(g_s, out, N, C, H2, W2, ipad):
    _launch("magnet_fnet_d2s_backward", g_s, _dev(g_s, "in", torch.float32).data_ptr(), _dev(out, "out", torch.float32).data_ptr(),
            N, C, H2, W2, ipad)


def spp_upsample_backward(g, c_off, N, h, w, pad, ph, pw, dq):
    a = MagnetSppBwdArgs(g=_dev(g, "g", torch.float32).data_ptr(), g_ld=g.stride(0), N=N, h=h, w=w, pad=pad, c_off=c_off, ph=ph, pw=pw,
                         dq=_dev(dq, "dq", torch.float32).data_ptr())
    _launch("magnet_spp_upsample_backward", g, ctypes.byref(a))


def spp_pool_backward(g, c_off, N, h, w, pad, dpools, out):
    a = MagnetSppBwdArgs(g=_dev(g, "g", torch.float32).data_ptr(), g_ld=g.stride(0), N=N, h=h, w=w, pad=pad, c_off=c_off,
                         out=_dev(out, "out", torch.float32).data_ptr(), out_ld=out.stride(0))
    for i, d in enumerate(dpools):
        a.dpool[i] = _dev(d, "dpool", torch.float32).data_ptr()
    _launch("magnet_spp_pool_backward", g, ctypes.byref(a))


def fnet_stem_wgrad(img, dz, grad_w, work):
    x = _dev(img, "img", torch.float32)
    N, _, H, W = x.shape
    _launch("magnet_fnet_stem_wgrad", x, x.data_ptr(), _bf16_ptr(dz[0], "dz_hi"), _bf16_ptr(dz[1], "dz_lo"),
            _dev(grad_w, "grad_w", torch.float32).data_ptr(), _dev(work, "work", torch.float64).data_ptr(), N, H, W)


# ---- the D-Net decoder (include/magnet_hip.h: magnet_conv_mfma_ex, magnet_dnet_gauss_head; csrc/dnet_kernels.hip) ----------------
def dnet_gauss_head(head_out, ld, N, h, w, pad, out):
    """Depth-head fp32 output (rows >= N*(h+2pad)*(w+2pad), ld) -> out (N,2,h,w) = [mu, sqrt(elu(v) + 1 + 1e-10)] (DNET.py:62-67)."""
    x = _dev(head_out, "head_out", torch.float32)
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) != ld or x.shape[0] < N * (h + 2 * pad) * (w + 2 * pad) or x.shape[1] < 2:
        raise MagnetError(f"dnet_gauss_head: head output {tuple(x.shape)} does not hold {N} ({h}+2*{pad}) x ({w}+2*{pad}) grids of pitch {ld}")
    o = _dev(out, "out", torch.float32)
    if tuple(o.shape) != (N, 2, h, w) or not o.is_contiguous():
        raise MagnetError(f"dnet_gauss_head: out must be a contiguous ({N}, 2, {h}, {w}) tensor")
    _launch("magnet_dnet_gauss_head", x, x.data_ptr(), int(ld), N, h, w, pad, o.data_ptr())


def check_dnet_upsample_gauss(head_out, head_ld, mask_out, mask_ld, N, h, w, out):
    """The shape / pitch / device rules of dnet_upsample_gauss (MagnetError); tensors on any device, nothing is launched."""
    N, h, w, head_ld, mask_ld = int(N), int(h), int(w), int(head_ld), int(mask_ld)
    if N <= 0 or h <= 0 or w <= 0:
        raise MagnetError(f"dnet_upsample_gauss: bad dims N={N} h={h} w={w}")
    if head_ld < 2 or head_ld % 2 or mask_ld < 144 or mask_ld % 4:
        raise MagnetError(f"dnet_upsample_gauss: head_ld {head_ld} must be even and >= 2, mask_ld {mask_ld} a multiple of 4 and >= 144")
    rows = N * (h + 2) * (w + 2)
    for t, name, ld, c in ((head_out, "head output", head_ld, 2), (mask_out, "mask logits", mask_ld, 144)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise MagnetError(f"dnet_upsample_gauss: {name} must be a float32 tensor")
        if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != ld or t.shape[0] < rows or t.shape[1] < c:
            raise MagnetError(f"dnet_upsample_gauss: {name} {tuple(t.shape)} does not hold {N} ({h}+2) x ({w}+2) grids of {c} channels at pitch {ld}")
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (N, 2, 4 * h, 4 * w) or not out.is_contiguous():
        raise MagnetError(f"dnet_upsample_gauss: out must be a contiguous float32 ({N}, 2, {4 * h}, {4 * w}) tensor")
    if head_out.device != out.device or mask_out.device != out.device:
        raise MagnetError("dnet_upsample_gauss: head output, mask logits and out must be on the same device")


def dnet_upsample_gauss(head_out, head_ld, mask_out, mask_ld, N, h, w, out):
    """The stand-alone D-Net's tail in one launch: depth-head fp32 output (rows >= N*(h+2)*(w+2), head_ld; channel 0 = mu, 1 = v) and
    mask-head logits (rows, mask_ld; channel n*16 + i*4 + j) -> out (N,2,4h,4w) = [up(mu), elu(up(v)) + 1 + 1e-10]
    (D_dense_depth.py:85-100 then DNET.py:55-60)."""
    check_dnet_upsample_gauss(head_out, head_ld, mask_out, mask_ld, N, h, w, out)
    x, m, o = _dev(head_out, "head_out", torch.float32), _dev(mask_out, "mask_out", torch.float32), _dev(out, "out", torch.float32)
    _launch("magnet_dnet_upsample_gauss", x, x.data_ptr(), int(head_ld), m.data_ptr(), int(mask_ld), int(N), int(h), int(w), o.data_ptr())
    return out


# ---- sequence inference (include/magnet_hip.h: magnet_gather_views, magnet_scatter_frames; csrc/frame_pool.hip; magnet_amd/sequence.py) -------------------
def gather_views(slots, B, V, pool_feat=None, pool_gmm=None, pool_xd3=None, ref_cl=None, src_pad=None, ref_gmm=None, src_gmm=None,
                 gin=None):
    """One launch from the frame pool into a step's input buffers through the device slot table `slots` ((1 + V) B int32: [b] the
    reference frame of window b, [B + v B + b] its view v; an entry outside [0, n_slots) stands for no frame and gives zeros).
    pool_feat (n_slots, h+2, w+2, F) fp32 / bf16, pool_gmm (n_slots, 2, h, w) fp32, pool_xd3 = (hi, lo) bf16 planes
    (n_slots, (h+2)(w+2), 256).  Destinations, each optional: ref_cl (B, h, w, F), src_pad (V B, h+2, w+2, F), ref_gmm (B, 2, h, w),
    src_gmm (V B, 2, h, w), gin = (hi, lo, ld, c_off): the reference frames' x_d3 into channels [c_off, c_off + 256) of the
    (B (h+2)(w+2), ld) planes of MAGNET.gnet_input_buffer()."""
    B, V = int(B), int(V)
    t = _dev(slots, "slots", torch.int32)
    if B <= 0 or V < 0 or tuple(t.shape) != ((1 + V) * B,):
        raise MagnetError(f"gather_views: slots has shape {tuple(t.shape)}, expected ({(1 + V) * B},) for B = {B}, V = {V}")
    a = MagnetGatherViewsArgs(slots=t.data_ptr(), B=B, V=V)
    used = [t]
    n_slots = h = w = None

    def geometry(n, hh, ww, what):
        nonlocal n_slots, h, w
        if n_slots is None:
            n_slots, h, w = int(n), int(hh), int(ww)
        elif (n_slots, h, w) != (int(n), int(hh), int(ww)):
            raise MagnetError(f"gather_views: {what} is for {n} slots of {hh} x {ww}, the other pool tensors for {n_slots} of {h} x {w}")

    def dest(x, name, dtype, shape):
        x = _dev(x, name, dtype)
        if tuple(x.shape) != shape:
            raise MagnetError(f"gather_views: {name} has shape {tuple(x.shape)}, expected {shape}")
        used.append(x)
        return x.data_ptr()

    if pool_feat is not None:
        f = _dev(pool_feat, "pool_feat")
        if f.dim() != 4 or f.shape[1] < 3 or f.shape[2] < 3:
            raise MagnetError(f"gather_views: pool_feat must be (n_slots, h+2, w+2, F), got {tuple(f.shape)}")
        geometry(f.shape[0], f.shape[1] - 2, f.shape[2] - 2, "pool_feat")
        a.pool_feat, a.F, a.feat_dtype = f.data_ptr(), int(f.shape[3]), feat_enum(f.dtype)
        used.append(f)
    else:
        a.F = 8                                                  # no feature destination: any valid width
    if pool_gmm is not None:
        g = _dev(pool_gmm, "pool_gmm", torch.float32)
        if g.dim() != 4 or g.shape[1] != 2:
            raise MagnetError(f"gather_views: pool_gmm must be (n_slots, 2, h, w), got {tuple(g.shape)}")
        geometry(g.shape[0], g.shape[2], g.shape[3], "pool_gmm")
        a.pool_gmm = g.data_ptr()
        used.append(g)
    if n_slots is None and pool_xd3 is not None:
        raise MagnetError("gather_views: the x_d3 planes do not carry h and w: pass pool_feat or pool_gmm with them")
    if n_slots is None:
        raise MagnetError("gather_views: no pool tensor given")
    R = (h + 2) * (w + 2)
    if pool_xd3 is not None:
        for x, name in zip(pool_xd3, ("pool_xd3 hi plane", "pool_xd3 lo plane")):
            x = _dev(x, name, torch.bfloat16)
            if tuple(x.shape) != (n_slots, R, 256):
                raise MagnetError(f"gather_views: {name} has shape {tuple(x.shape)}, expected {(n_slots, R, 256)}")
            used.append(x)
        a.pool_xd3_hi, a.pool_xd3_lo = pool_xd3[0].data_ptr(), pool_xd3[1].data_ptr()
    a.n_slots, a.h, a.w = n_slots, h, w
    if ref_cl is not None or src_pad is not None:
        if pool_feat is None:
            raise MagnetError("gather_views: ref_cl / src_pad need pool_feat")
        if ref_cl is not None:
            a.ref_cl = dest(ref_cl, "ref_cl", pool_feat.dtype, (B, h, w, a.F))
        if src_pad is not None:
            a.src_pad = dest(src_pad, "src_pad", pool_feat.dtype, (V * B, h + 2, w + 2, a.F))
    if ref_gmm is not None or src_gmm is not None:
        if pool_gmm is None:
            raise MagnetError("gather_views: ref_gmm / src_gmm need pool_gmm")
        if ref_gmm is not None:
            a.ref_gmm = dest(ref_gmm, "ref_gmm", torch.float32, (B, 2, h, w))
        if src_gmm is not None:
            a.src_gmm = dest(src_gmm, "src_gmm", torch.float32, (V * B, 2, h, w))
    if gin is not None:
        if pool_xd3 is None:
            raise MagnetError("gather_views: gin needs pool_xd3")
        ghi, glo, ld, c_off = gin
        ld, c_off = int(ld), int(c_off)
        if ld % 8 or c_off % 8 or c_off < 0 or c_off + 256 > ld:
            raise MagnetError(f"gather_views: gin pitch {ld} and channel offset {c_off} must be multiples of 8 with c_off + 256 <= pitch")
        a.gin_hi, a.gin_lo = dest(ghi, "gin hi plane", torch.bfloat16, (B * R, ld)), dest(glo, "gin lo plane", torch.bfloat16, (B * R, ld))
        a.gin_ld, a.gin_c_off = ld, c_off
    if any(x.device != t.device for x in used):
        raise MagnetError("gather_views: all tensors must be on the same device")
    _launch("magnet_gather_views", t, ctypes.byref(a))


def scatter_frames(slots, pool_feat=None, pool_gmm=None, pool_xd3=None, feat=None, gmm=None, xd3=None):
    """The inverse of gather_views, one launch: staged frame j of every source that is given goes to slot slots[j] of its pool tensor
    (`slots`: (n,) int32 on the device; an entry outside [0, n_slots) skips the frame; two entries naming one slot are the caller's
    error).  feat (n, h+2, w+2, F) in pool_feat's dtype, gmm (n, 2, h, w) fp32, xd3 = (hi, lo) bf16 planes (n, (h+2)(w+2), 256) — or
    (n (h+2)(w+2), 256), the staging planes as the D-Net writes them.  Whole frames are copied bit for bit, borders included; a source
    left out leaves its pool tensor untouched."""
    t = _dev(slots, "slots", torch.int32)
    if t.dim() != 1 or t.shape[0] < 1:
        raise MagnetError(f"scatter_frames: slots has shape {tuple(t.shape)}, expected (n,) with n >= 1")
    n = int(t.shape[0])
    a = MagnetScatterFramesArgs(slots=t.data_ptr(), n=n, F=8)
    used = [t]
    geom = None                                                  # (n_slots, h, w)
    if feat is not None:
        if pool_feat is None:
            raise MagnetError("scatter_frames: feat needs pool_feat")
        p = _dev(pool_feat, "pool_feat")
        if p.dim() != 4 or p.shape[1] < 3 or p.shape[2] < 3:
            raise MagnetError(f"scatter_frames: pool_feat must be (n_slots, h+2, w+2, F), got {tuple(p.shape)}")
        f = _dev(feat, "feat", p.dtype)
        if tuple(f.shape) != (n,) + tuple(p.shape[1:]):
            raise MagnetError(f"scatter_frames: feat has shape {tuple(f.shape)}, expected {(n,) + tuple(p.shape[1:])}")
        geom = (int(p.shape[0]), int(p.shape[1]) - 2, int(p.shape[2]) - 2)
        a.feat, a.pool_feat, a.F, a.feat_dtype = f.data_ptr(), p.data_ptr(), int(p.shape[3]), feat_enum(p.dtype)
        used += [p, f]
    if gmm is not None:
        if pool_gmm is None:
            raise MagnetError("scatter_frames: gmm needs pool_gmm")
        p = _dev(pool_gmm, "pool_gmm", torch.float32)
        if p.dim() != 4 or p.shape[1] != 2:
            raise MagnetError(f"scatter_frames: pool_gmm must be (n_slots, 2, h, w), got {tuple(p.shape)}")
        g = _dev(gmm, "gmm", torch.float32)
        if tuple(g.shape) != (n,) + tuple(p.shape[1:]):
            raise MagnetError(f"scatter_frames: gmm has shape {tuple(g.shape)}, expected {(n,) + tuple(p.shape[1:])}")
        here = (int(p.shape[0]), int(p.shape[2]), int(p.shape[3]))
        if geom is not None and geom != here:
            raise MagnetError(f"scatter_frames: pool_gmm is for {here[0]} slots of {here[1]} x {here[2]}, pool_feat for {geom[0]} of {geom[1]} x {geom[2]}")
        geom = here
        a.gmm, a.pool_gmm = g.data_ptr(), p.data_ptr()
        used += [p, g]
    if xd3 is not None:
        if pool_xd3 is None:
            raise MagnetError("scatter_frames: xd3 needs pool_xd3")
        if geom is None:
            raise MagnetError("scatter_frames: the x_d3 planes do not carry h and w: pass feat or gmm (and their pool tensor) with them")
        R = (geom[1] + 2) * (geom[2] + 2)
        for x, name in zip(tuple(pool_xd3) + tuple(xd3), ("pool_xd3 hi plane", "pool_xd3 lo plane", "xd3 hi plane", "xd3 lo plane")):
            x = _dev(x, name, torch.bfloat16)
            ok = ((geom[0], R, 256),) if name.startswith("pool") else ((n, R, 256), (n * R, 256))
            if tuple(x.shape) not in ok:
                raise MagnetError(f"scatter_frames: {name} has shape {tuple(x.shape)}, expected {ok[0]}")
            used.append(x)
        a.pool_xd3_hi, a.pool_xd3_lo, a.xd3_hi, a.xd3_lo = (x.data_ptr() for x in tuple(pool_xd3) + tuple(xd3))
    if geom is None:
        raise MagnetError("scatter_frames: no source given")
    a.n_slots, a.h, a.w = geom
    if any(x.device != t.device for x in used):
        raise MagnetError("scatter_frames: all tensors must be on the same device")
    _launch("magnet_scatter_frames", t, ctypes.byref(a))


# ---- image ingest (include/magnet_hip.h: magnet_image_prep_u8; csrc/image_prep.hip; magnet_amd/ingest.py) ------------------------------------------
def image_prep_u8(frames, out, crop, tables_x, tables_y, lut):
    """One launch: uint8 channel-last frames (N, Hin, Win, 3) (the last two dimensions dense, rows and frames through their strides)
    -> out (N, 3, Hout, Wout) fp32: crop = (left, top, width, height), PIL's 8-bit BILINEAR resize of the box to (Wout, Hout) through
    tables_x / tables_y = (coef (out size, k) int32, bounds (out size, 2) int32), or None for a pass whose size does not change, then
    out[n, c, y, x] = lut[c, v] with lut (3, 256) fp32.  magnet_amd.ingest.ImagePrep builds the tables and owns them."""
    f = frames
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
        raise MagnetError("image_prep_u8: frames must be a uint8 GPU tensor (N, Hin, Win, 3)")
    N, Hin, Win, _ = (int(v) for v in f.shape)
    if N < 1 or f.stride(3) != 1 or f.stride(2) != 3 or f.stride(1) < 3 * Win or (N > 1 and f.stride(0) < f.stride(1) * Hin):
        raise MagnetError(f"image_prep_u8: frames {tuple(f.shape)} with strides {tuple(f.stride())}: pixels must be dense and rows and frames must not overlap")
    o = _dev(out, "out", torch.float32)
    if o.dim() != 4 or o.shape[0] != N or o.shape[1] != 3:
        raise MagnetError(f"image_prep_u8: out has shape {tuple(o.shape)}, expected ({N}, 3, Hout, Wout)")
    Hout, Wout = int(o.shape[2]), int(o.shape[3])
    left, top, cw, ch = (int(v) for v in crop)
    lut = _dev(lut, "lut", torch.float32)
    if tuple(lut.shape) != (3, 256):
        raise MagnetError(f"image_prep_u8: lut has shape {tuple(lut.shape)}, expected (3, 256)")
    a = MagnetImagePrepArgs(src=f.data_ptr(), src_pitch=f.stride(1), src_frame=f.stride(0), lut=lut.data_ptr(), out=o.data_ptr(),
                            N=N, Hin=Hin, Win=Win, crop_left=left, crop_top=top, crop_w=cw, crop_h=ch, Hout=Hout, Wout=Wout)
    used = [f, o, lut]
    for axis, tables, n_in, n_out in (("x", tables_x, cw, Wout), ("y", tables_y, ch, Hout)):
        if (tables is None) != (n_in == n_out):
            raise MagnetError(f"image_prep_u8: the {axis} pass goes from {n_in} to {n_out} pixels: it takes tables exactly when the size changes")
        if tables is None:
            continue
        coef, bounds = _dev(tables[0], f"coef_{axis}", torch.int32), _dev(tables[1], f"bounds_{axis}", torch.int32)
        if coef.dim() != 2 or coef.shape[0] != n_out or tuple(bounds.shape) != (n_out, 2):
            raise MagnetError(f"image_prep_u8: coef_{axis} {tuple(coef.shape)} / bounds_{axis} {tuple(bounds.shape)}, expected ({n_out}, k) and ({n_out}, 2)")
        setattr(a, "coef_" + axis, coef.data_ptr()); setattr(a, "bounds_" + axis, bounds.data_ptr()); setattr(a, "k" + axis, int(coef.shape[1]))
        used += [coef, bounds]
    if any(x.device != f.device for x in used):
        raise MagnetError("image_prep_u8: all tensors must be on the same device")
    _launch("magnet_image_prep_u8", f, ctypes.byref(a))
    return out


# ---- training samples (magnet_train_prep_u8: csrc/image_prep.hip; magnet_depth_prep_u16: csrc/depth_prep.hip; ingest.TrainPrep) ----
def _frame_params(frame_params, N, who):
    r = _dev(frame_params, "frame_params", torch.int32)
    if tuple(r.shape) != (N, 4):
        raise MagnetError(f"{who}: frame_params has shape {tuple(r.shape)}, expected ({N}, 4) rows of (lut_index, flip, win_x, win_y)")
    return r


def _window(out, N, channels, res_hw, who):
    o = _dev(out, "out", torch.float32)
    if o.dim() != 4 or o.shape[0] != N or o.shape[1] != channels:
        raise MagnetError(f"{who}: out has shape {tuple(o.shape)}, expected ({N}, {channels}, Hout, Wout)")
    Hres, Wres = (int(v) for v in res_hw)
    if not (1 <= o.shape[2] <= Hres and 1 <= o.shape[3] <= Wres):
        raise MagnetError(f"{who}: the window {tuple(o.shape[2:])} of out is not inside the resized image {(Hres, Wres)}")
    return o, Hres, Wres


def train_prep_u8(frames, out, crop, res_hw, tables_x, tables_y, luts, frame_params):
    """One launch: image_prep_u8's crop and resize, to res_hw = (Hres, Wres), of uint8 frames (N, Hin, Win, 3); then per frame n, from
    frame_params[n] = (lut_index, flip, win_x, win_y) (int32 (N, 4) on the device), the (Hout, Wout) window at (win_x, win_y) of the
    horizontally flipped (flip != 0) resized image, looked up in luts[lut_index] ((L, 3, 256) fp32) -> out (N, 3, Hout, Wout) fp32.
    The tables are those of crop -> res_hw, present exactly when a size changes.  The device clamps the records into their ranges;
    ingest.TrainPrep validates them on the host."""
    f = frames
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
        raise MagnetError("train_prep_u8: frames must be a uint8 GPU tensor (N, Hin, Win, 3)")
    N, Hin, Win, _ = (int(v) for v in f.shape)
    if N < 1 or f.stride(3) != 1 or f.stride(2) != 3 or f.stride(1) < 3 * Win or (N > 1 and f.stride(0) < f.stride(1) * Hin):
        raise MagnetError(f"train_prep_u8: frames {tuple(f.shape)} with strides {tuple(f.stride())}: pixels must be dense and rows and frames must not overlap")
    o, Hres, Wres = _window(out, N, 3, res_hw, "train_prep_u8")
    left, top, cw, ch = (int(v) for v in crop)
    luts = _dev(luts, "luts", torch.float32)
    if luts.dim() != 3 or luts.shape[0] < 1 or tuple(luts.shape[1:]) != (3, 256):
        raise MagnetError(f"train_prep_u8: luts has shape {tuple(luts.shape)}, expected (L, 3, 256) with L >= 1")
    rec = _frame_params(frame_params, N, "train_prep_u8")
    a = MagnetTrainPrepArgs(src=f.data_ptr(), src_pitch=f.stride(1), src_frame=f.stride(0), luts=luts.data_ptr(), frame_params=rec.data_ptr(),
                            out=o.data_ptr(), N=N, Hin=Hin, Win=Win, crop_left=left, crop_top=top, crop_w=cw, crop_h=ch, Hres=Hres, Wres=Wres,
                            Hout=int(o.shape[2]), Wout=int(o.shape[3]), n_luts=int(luts.shape[0]))
    used = [f, o, luts, rec]
    for axis, tables, n_in, n_out in (("x", tables_x, cw, Wres), ("y", tables_y, ch, Hres)):
        if (tables is None) != (n_in == n_out):
            raise MagnetError(f"train_prep_u8: the {axis} pass goes from {n_in} to {n_out} pixels: it takes tables exactly when the size changes")
        if tables is None:
            continue
        coef, bounds = _dev(tables[0], f"coef_{axis}", torch.int32), _dev(tables[1], f"bounds_{axis}", torch.int32)
        if coef.dim() != 2 or coef.shape[0] != n_out or tuple(bounds.shape) != (n_out, 2):
            raise MagnetError(f"train_prep_u8: coef_{axis} {tuple(coef.shape)} / bounds_{axis} {tuple(bounds.shape)}, expected ({n_out}, k) and ({n_out}, 2)")
        setattr(a, "coef_" + axis, coef.data_ptr()); setattr(a, "bounds_" + axis, bounds.data_ptr()); setattr(a, "k" + axis, int(coef.shape[1]))
        used += [coef, bounds]
    if any(x.device != f.device for x in used):
        raise MagnetError("train_prep_u8: all tensors must be on the same device")
    _launch("magnet_train_prep_u8", f, ctypes.byref(a))
    return out


def depth_prep_u16(depth, out, crop, res_hw, idx_x, idx_y, frame_params, divisor, invalid_code=-1):
    """One launch: uint16 depth maps (N, Hin, Win) (the last dimension dense, rows and frames through their strides) -> out
    (N, 1, Hout, Wout) fp32: crop = (left, top, width, height), PIL's NEAREST resize of the box to res_hw through idx_x (Wres) / idx_y (Hres)
    int32 source indices (None for an axis whose size does not change), the frame's flip and window as train_prep_u8 (lut_index is
    ignored), a sample equal to invalid_code -> 0 (-1: none), then one correctly rounded fp32 division by `divisor`."""
    d = depth
    if not isinstance(d, torch.Tensor) or not d.is_cuda or d.dtype != torch.uint16 or d.dim() != 3:
        raise MagnetError("depth_prep_u16: depth must be a uint16 GPU tensor (N, Hin, Win)")
    N, Hin, Win = (int(v) for v in d.shape)
    if N < 1 or d.stride(2) != 1 or d.stride(1) < Win or (N > 1 and d.stride(0) < d.stride(1) * Hin):
        raise MagnetError(f"depth_prep_u16: depth {tuple(d.shape)} with strides {tuple(d.stride())}: pixels must be dense and rows and frames must not overlap")
    o, Hres, Wres = _window(out, N, 1, res_hw, "depth_prep_u16")
    left, top, cw, ch = (int(v) for v in crop)
    rec = _frame_params(frame_params, N, "depth_prep_u16")
    divisor = float(divisor)
    if not (math.isfinite(divisor) and divisor > 0.0):
        raise MagnetError(f"depth_prep_u16: divisor {divisor} must be finite and positive")
    a = MagnetDepthPrepArgs(src=d.data_ptr(), src_pitch=d.stride(1), src_frame=d.stride(0), frame_params=rec.data_ptr(), out=o.data_ptr(),
                            N=N, Hin=Hin, Win=Win, crop_left=left, crop_top=top, crop_w=cw, crop_h=ch, Hres=Hres, Wres=Wres,
                            Hout=int(o.shape[2]), Wout=int(o.shape[3]), invalid_code=int(invalid_code), divisor=divisor)
    used = [d, o, rec]
    for axis, idx, n_in, n_out in (("x", idx_x, cw, Wres), ("y", idx_y, ch, Hres)):
        if (idx is None) != (n_in == n_out):
            raise MagnetError(f"depth_prep_u16: the {axis} axis goes from {n_in} to {n_out} pixels: it takes an index table exactly when the size changes")
        if idx is None:
            continue
        t = _dev(idx, f"idx_{axis}", torch.int32)
        if tuple(t.shape) != (n_out,):
            raise MagnetError(f"depth_prep_u16: idx_{axis} has shape {tuple(t.shape)}, expected ({n_out},)")
        setattr(a, "idx_" + axis, t.data_ptr())
        used.append(t)
    if any(x.device != d.device for x in used):
        raise MagnetError("depth_prep_u16: all tensors must be on the same device")
    _launch("magnet_depth_prep_u16", d, ctypes.byref(a))
    return out


# ---- the D-Net's encoder (EfficientNet-B5): stem, depthwise convolution, squeeze-excite --------------------------------
def enc_stem(img, wgt, bias, out_hi, out_lo):
    """(N,3,H,W) fp32 image -> the interior of the 64-channel split planes (N,H2+2,W2+2,64), H2 = ceil(H/2): 3x3/s2 conv with TF "SAME"
    padding + folded BN + SiLU, 48 channels + 16 zero lanes.  wgt (48, 27), bias (48)."""
    x = _dev(img, "img", torch.float32)
    N, C, H, W = x.shape
    if C != 3:
        raise MagnetError(f"enc_stem: expected 3 input channels, got {C}")
    if tuple(wgt.shape) != (48, 27) or tuple(bias.shape) != (48,):
        raise MagnetError(f"enc_stem: wgt (48, 27) and bias (48,), got {tuple(wgt.shape)} / {tuple(bias.shape)}")
    rows = N * ((H + 1) // 2 + 2) * ((W + 1) // 2 + 2)
    for t, n in ((out_hi, "out_hi"), (out_lo, "out_lo")):
        _bf16_ptr(t, f"enc_stem: {n}", contiguous=True)
        if t.numel() < rows * 64:
            raise MagnetError(f"enc_stem: {n} holds {t.numel()} elements, needs {rows * 64}")
    _launch("magnet_enc_stem", x, x.data_ptr(), _dev(wgt, "wgt", torch.float32).data_ptr(), _dev(bias, "bias", torch.float32).data_ptr(),
            out_hi.data_ptr(), out_lo.data_ptr(), N, H, W)


def enc_stem_f16(img, wgt, bias, out_f16):
    """enc_stem on the single-plane fp16 format (magnet_enc_stem_f16): the interior of ONE fp16 plane (N,H2+2,W2+2,64)."""
    x = _dev(img, "img", torch.float32)
    N, C, H, W = x.shape
    if C != 3:
        raise MagnetError(f"enc_stem_f16: expected 3 input channels, got {C}")
    if tuple(wgt.shape) != (48, 27) or tuple(bias.shape) != (48,):
        raise MagnetError(f"enc_stem_f16: wgt (48, 27) and bias (48,), got {tuple(wgt.shape)} / {tuple(bias.shape)}")
    rows = N * ((H + 1) // 2 + 2) * ((W + 1) // 2 + 2)
    _f16_plane("enc_stem_f16: out_f16", out_f16, rows * 64)
    _launch("magnet_enc_stem_f16", x, x.data_ptr(), _dev(wgt, "wgt", torch.float32).data_ptr(), _dev(bias, "bias", torch.float32).data_ptr(),
            out_f16.data_ptr(), N, H, W)


def dwconv_parts(ho, wo) -> int:
    """magnet_dwconv_cl_parts: rows of the partial-sum scratch per image for an (ho, wo) output.  Host arithmetic: no GPU needed."""
    return int(load().magnet_dwconv_cl_parts(int(ho), int(wo)))


def _grid_planes(who, t, N, h, w, ld):
    """A plane of a zero-bordered (N, h+2, w+2, ld) grid: a bf16 GPU tensor that holds it at row pitch ld (its data_ptr is row 0)."""
    _bf16_ptr(t, who, contiguous=True)
    if t.numel() < N * (h + 2) * (w + 2) * ld:
        raise MagnetError(f"{who} holds {t.numel()} elements, needs {N * (h + 2) * (w + 2) * ld}")
    return t.data_ptr()


def _f16_plane(who, t, numel):
    """ONE fp16 plane of a zero-bordered grid: a contiguous fp16 GPU tensor of at least numel elements (its data_ptr is row 0)."""
    _f16_ptr(t, who)
    if not t.is_contiguous():
        raise MagnetError(f"{who} must be contiguous")
    if t.numel() < numel:
        raise MagnetError(f"{who} holds {t.numel()} elements, needs {numel}")
    return t.data_ptr()


def dwconv_cl(in_hi, in_lo, in_ld, N, h, w, c_pad, wgt, bias, k, stride, pad_top, pad_left, out_hi, out_lo, out_ld, part):
    """Depthwise k x k convolution + bias + SiLU on split planes, with the per-tile partial channel sums (include/magnet_hip.h):
    in (N,h+2,w+2,in_ld) -> interior of out (N,ho+2,wo+2,out_ld), ho = ceil(h / stride); wgt (k*k, c_pad) fp32, bias (c_pad);
    part (N, dwconv_parts(ho, wo), c_pad) fp32."""
    ho, wo = -(-int(h) // int(stride)), -(-int(w) // int(stride))
    n_part = dwconv_parts(ho, wo)
    a = MagnetDwConvArgs()
    a.in_hi, a.in_lo = (_grid_planes(f"dwconv_cl: {n}", t, N, h, w, in_ld) for t, n in ((in_hi, "in_hi"), (in_lo, "in_lo")))
    a.out_hi, a.out_lo = (_grid_planes(f"dwconv_cl: {n}", t, N, ho, wo, out_ld) for t, n in ((out_hi, "out_hi"), (out_lo, "out_lo")))
    if tuple(wgt.shape) != (k * k, c_pad) or tuple(bias.shape) != (c_pad,):
        raise MagnetError(f"dwconv_cl: wgt ({k * k}, {c_pad}) and bias ({c_pad},), got {tuple(wgt.shape)} / {tuple(bias.shape)}")
    a.wgt, a.bias = _dev(wgt, "wgt", torch.float32).data_ptr(), _dev(bias, "bias", torch.float32).data_ptr()
    if _dev(part, "part", torch.float32).numel() < N * n_part * c_pad:
        raise MagnetError(f"dwconv_cl: part holds {part.numel()} elements, needs {N * n_part * c_pad}")
    a.part = part.data_ptr()
    a.N, a.h, a.w, a.c_pad, a.in_ld, a.out_ld = int(N), int(h), int(w), int(c_pad), int(in_ld), int(out_ld)
    a.k, a.stride, a.pad_top, a.pad_left, a.n_part = int(k), int(stride), int(pad_top), int(pad_left), n_part
    _launch("magnet_dwconv_cl", in_hi, ctypes.byref(a))
    return n_part


def dwconv_cl_f16(in_f16, in_ld, N, h, w, c_pad, wgt, bias, k, stride, pad_top, pad_left, out_f16, out_ld, part):
    """dwconv_cl on the single-plane fp16 format (magnet_dwconv_cl_f16): in / out are ONE fp16 plane each; `part` holds the sums of the
    fp32 values before the fp16 store, as dwconv_cl's."""
    ho, wo = -(-int(h) // int(stride)), -(-int(w) // int(stride))
    n_part = dwconv_parts(ho, wo)
    a = MagnetDwConvArgs()
    a.in_hi = _f16_plane("dwconv_cl_f16: in_f16", in_f16, N * (h + 2) * (w + 2) * in_ld)
    a.out_hi = _f16_plane("dwconv_cl_f16: out_f16", out_f16, N * (ho + 2) * (wo + 2) * out_ld)
    if tuple(wgt.shape) != (k * k, c_pad) or tuple(bias.shape) != (c_pad,):
        raise MagnetError(f"dwconv_cl_f16: wgt ({k * k}, {c_pad}) and bias ({c_pad},), got {tuple(wgt.shape)} / {tuple(bias.shape)}")
    a.wgt, a.bias = _dev(wgt, "wgt", torch.float32).data_ptr(), _dev(bias, "bias", torch.float32).data_ptr()
    if _dev(part, "part", torch.float32).numel() < N * n_part * c_pad:
        raise MagnetError(f"dwconv_cl_f16: part holds {part.numel()} elements, needs {N * n_part * c_pad}")
    a.part = part.data_ptr()
    a.N, a.h, a.w, a.c_pad, a.in_ld, a.out_ld = int(N), int(h), int(w), int(c_pad), int(in_ld), int(out_ld)
    a.k, a.stride, a.pad_top, a.pad_left, a.n_part = int(k), int(stride), int(pad_top), int(pad_left), n_part
    _launch("magnet_dwconv_cl_f16", in_f16, ctypes.byref(a))
    return n_part


def se_gate(part, n_part, hw, w_reduce, b_reduce, w_expand_t, b_expand, C, R, gate):
    """part (N, n_part, c_pad) -> gate (N, c_pad) fp32: mean over hw, reduce FC + SiLU, expand FC + sigmoid; zero for channels >= C.
    w_reduce, w_expand_t (R, C) fp32; b_reduce (R,), b_expand (C,)."""
    g = _dev(gate, "gate", torch.float32)
    if g.dim() != 2:
        raise MagnetError(f"se_gate: gate must be (N, c_pad), got {tuple(g.shape)}")
    N, c_pad = g.shape
    if _dev(part, "part", torch.float32).numel() < N * int(n_part) * c_pad:
        raise MagnetError(f"se_gate: part holds {part.numel()} elements, needs {N * int(n_part) * c_pad}")
    for t, n, shape in ((w_reduce, "w_reduce", (R, C)), (w_expand_t, "w_expand_t", (R, C)), (b_reduce, "b_reduce", (R,)), (b_expand, "b_expand", (C,))):
        if tuple(_dev(t, n, torch.float32).shape) != shape:
            raise MagnetError(f"se_gate: {n} must be {shape}, got {tuple(t.shape)}")
    _launch("magnet_se_gate", g, part.data_ptr(), int(n_part), int(hw), w_reduce.data_ptr(), b_reduce.data_ptr(), w_expand_t.data_ptr(),
            b_expand.data_ptr(), int(C), int(R), int(c_pad), g.data_ptr(), int(N))


def se_scale(in_hi, in_lo, in_ld, gate, N, h, w, c_pad, out_hi, out_lo, out_ld):
    """out = split((hi + lo) * gate[n][c]) over the interior of the (N,h+2,w+2,.) grid, channels [0, c_pad); out may be the input."""
    g = _dev(gate, "gate", torch.float32)
    if tuple(g.shape) != (N, c_pad):
        raise MagnetError(f"se_scale: gate must be {(N, c_pad)}, got {tuple(g.shape)}")
    ih, il = (_grid_planes(f"se_scale: {n}", t, N, h, w, in_ld) for t, n in ((in_hi, "in_hi"), (in_lo, "in_lo")))
    oh, ol = (_grid_planes(f"se_scale: {n}", t, N, h, w, out_ld) for t, n in ((out_hi, "out_hi"), (out_lo, "out_lo")))
    _launch("magnet_se_scale", in_hi, ih, il, int(in_ld), g.data_ptr(), int(N), int(h), int(w), int(c_pad), oh, ol, int(out_ld))


def se_scale_f16(in_f16, in_ld, gate, N, h, w, c_pad, out_f16, out_ld):
    """se_scale on the single-plane fp16 format (magnet_se_scale_f16): out = f16(in * gate[n][c]); out may be the input."""
    g = _dev(gate, "gate", torch.float32)
    if tuple(g.shape) != (N, c_pad):
        raise MagnetError(f"se_scale_f16: gate must be {(N, c_pad)}, got {tuple(g.shape)}")
    i = _f16_plane("se_scale_f16: in_f16", in_f16, N * (h + 2) * (w + 2) * in_ld)
    o = _f16_plane("se_scale_f16: out_f16", out_f16, N * (h + 2) * (w + 2) * out_ld)
    _launch("magnet_se_scale_f16", in_f16, i, int(in_ld), g.data_ptr(), int(N), int(h), int(w), int(c_pad), o, int(out_ld))
