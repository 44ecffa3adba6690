"""ctypes binding of the C ABI declared in include/lama_hip.h.

``LamaLib()`` loads the in-tree ``lama_amd/lib/liblama_hip.so`` (built by ``lama_amd.build`` /
``__graft_entry__.build()``) and raises if it is missing: there is no CPU or eager-PyTorch fallback.
All entry points take raw device pointers (``tensor.data_ptr()``) and a ``hipStream_t``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
PAD_ZERO, PAD_REFLECT = 0, 1
PREC_F32, PREC_BF16X3, PREC_F16X3, PREC_F16 = 0, 1, 2, 3
CONV_COOPERATIVE = 1
CONV_DEFER_OUT = 2          # lama_winograd_conv3x3_fwd: the GEMM launch only (include/lama_hip.h)
CONV_SIBLINGS_SHIFT = 8     # (v109) bits 8..10: log2 of the number of sibling launches that share the chip with this one
DT_F32, DT_F16, DT_SPLIT16 = 0, 1, 2      # LAMA_DT_*
# LAMA_CONV_FAMILY_* of lama_conv2d_route_query (include/lama_hip.h)
(CONV_FAM_F32, CONV_FAM_GEMM1X1_WK, CONV_FAM_GEMM1X1_W4, CONV_FAM_GEMM1X1_WS, CONV_FAM_CONV_WR, CONV_FAM_CONVT2, CONV_FAM_STEM7, CONV_FAM_HEAD7,
 CONV_FAM_LDS) = range(9)


def conv_geo_wr(wmv, kg, ksc1, twlog, s2=0, coop=0, roll=0, fuse1=0, xs=0, ys=0) -> int:
    """LAMA_CONV_GEO_WR: the geometry word of a CONV_FAM_CONV_WR route."""
    return wmv | kg << 4 | ksc1 << 8 | twlog << 12 | s2 << 16 | coop << 17 | roll << 18 | fuse1 << 19 | xs << 20 | ys << 21


def conv_geo_lds(bm, bn, mode=0, trf=0) -> int:
    """The geometry word of a CONV_FAM_LDS route."""
    return bm | bn << 8 | mode << 20 | trf << 22
POOL_MAX, POOL_AVG_EXCLUDE_PAD = 0, 1      # lama_pool3x3_fwd mode
ABI_VERSION = 112      # LAMA_HIP_VERSION of include/lama_hip.h
PREC_NAMES = {'f32': PREC_F32, 'bf16x3': PREC_BF16X3, 'f16x3': PREC_F16X3, 'f16': PREC_F16}

_DEFAULT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'liblama_hip.so')


class LamaError(RuntimeError):
    """``code``: the numeric return value of the C entry point (LAMA_ERR_* < 0, hipError_t > 0) or None for host-side errors."""

    def __init__(self, msg: str = '', code=None):
        super().__init__(msg)
        self.code = code


class LamaRangeError(LamaError):
    """A weight or an activation left the range of the fp16 split (|x| <= 65504): re-run with PREC_BF16X3 / PREC_F32."""

F16_MAX = 65504.0
ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3      # include/lama_hip.h LAMA_ERR_*
JPEG_444, JPEG_420 = 0, 1      # include/lama_hip.h LAMA_JPEG_*
FFT_KIND_WINO64, FFT_KIND_IP64, FFT_KIND_IP128, FFT_KIND_TRACE64, FFT_KIND_SEQ, FFT_KIND_SIZED, FFT_KIND_GENERIC = range(7)   # LAMA_FFT_KIND_*


class Tensor4(C.Structure):
    """struct lama_tensor"""
    _fields_ = [('ptr', C.c_void_p), ('batch_stride', C.c_int64), ('C', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('dtype', C.c_int32)]


class Conv2dArgs(C.Structure):
    """struct lama_conv2d_args"""
    _fields_ = [('x', Tensor4), ('w_packed', C.c_void_p),
                ('kh', C.c_int32), ('kw', C.c_int32), ('stride', C.c_int32), ('pad', C.c_int32),
                ('pad_mode', C.c_int32), ('transposed', C.c_int32),
                ('x2', Tensor4), ('w2_packed', C.c_void_p), ('bias', C.c_void_p), ('act', C.c_int32),
                ('resid', Tensor4), ('y', Tensor4), ('batch', C.c_int32), ('precision', C.c_int32),
                ('range_flag', C.c_void_p), ('fuse1_w', C.c_void_p), ('fuse1_bias', C.c_void_p), ('fuse1_y', Tensor4),
                ('flags', C.c_int32)]


class Conv2dRectArgs(C.Structure):
    """struct lama_conv2d_rect_args"""
    _fields_ = [('x', Tensor4), ('w_packed', C.c_void_p), ('bias', C.c_void_p), ('act', C.c_int32), ('y', Tensor4), ('batch', C.c_int32),
                ('kh', C.c_int32), ('kw', C.c_int32), ('stride', C.c_int32), ('pad_h', C.c_int32), ('pad_w', C.c_int32),
                ('precision', C.c_int32), ('range_flag', C.c_void_p)]


class TailLists(C.Structure):
    """struct lama_tail_lists"""
    _fields_ = [('n_up', C.c_int32), ('head_rs', C.c_int32), ('up_mg', C.c_int32 * 4), ('head_list', C.c_void_p), ('head_count', C.c_void_p),
                ('up_list', C.c_void_p * 4), ('up_count', C.c_void_p * 4)]


def view(t: Optional[torch.Tensor], c0: int = 0, c: Optional[int] = None) -> Tensor4:
    """lama_tensor view of channels [c0, c0+c) of a contiguous fp32 / fp16 NCHW tensor (None -> absent)."""
    if t is None:
        return Tensor4(None, 0, 0, 0, 0, 0)
    if t.dtype not in (torch.float32, torch.float16) or t.dim() != 4 or not t.is_contiguous():
        raise LamaError(f'expected a contiguous fp32 / fp16 NCHW tensor, got {t.dtype} {tuple(t.shape)}')
    B, Ct, H, W = t.shape
    c = Ct - c0 if c is None else c
    if c0 < 0 or c <= 0 or c0 + c > Ct:
        raise LamaError('channel slice out of range')
    return Tensor4(t.data_ptr() + t.element_size() * c0 * H * W, Ct * H * W, c, H, W, DT_F16 if t.dtype == torch.float16 else DT_F32)


def view_split(t: torch.Tensor) -> Tensor4:
    """lama_tensor view of a whole contiguous fp32 [B, C, H, W] buffer that holds LAMA_DT_SPLIT16 parts (include/lama_hip.h: four bytes per
    logical element, per image [C / 8][hi | lo][H][W][8 halves]; no channel slices)."""
    if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() or t.shape[1] % 8 != 0:
        raise LamaError(f'expected a contiguous fp32-sized NCHW buffer with C % 8 == 0, got {t.dtype} {tuple(t.shape)}')
    B, Ct, H, W = t.shape
    return Tensor4(t.data_ptr(), Ct * H * W, Ct, H, W, DT_SPLIT16)


def _split16_part_dtype(precision: int) -> torch.dtype:
    if precision not in (PREC_F16X3, PREC_BF16X3):
        raise LamaError('LAMA_DT_SPLIT16 exists for PREC_F16X3 / PREC_BF16X3 only')
    return torch.float16 if precision == PREC_F16X3 else torch.bfloat16


def split16_pack(x: torch.Tensor, precision: int) -> torch.Tensor:
    """fp32 [B, C, H, W] -> the LAMA_DT_SPLIT16 image of it (an fp32-typed buffer of the same shape for view_split): hi = rne16(x),
    lo = rne16(x - hi) in the part type of ``precision``.  Host-side helper for tests and tools (torch ops on x's device)."""
    dt = _split16_part_dtype(precision)
    B, Ct, H, W = x.shape
    if Ct % 8 != 0:
        raise LamaError('LAMA_DT_SPLIT16 needs C % 8 == 0')
    x = x.float()
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt)
    parts = torch.stack((hi, lo), 0).view(torch.int16).view(2, B, Ct // 8, 8, H, W)
    return parts.permute(1, 2, 0, 4, 5, 3).contiguous().view(torch.float32).view(B, Ct, H, W)


def split16_unpack(buf: torch.Tensor, precision: int):
    """The (hi, lo) parts of a LAMA_DT_SPLIT16 buffer (as view_split takes it), each [B, C, H, W] in the part type of ``precision``."""
    dt = _split16_part_dtype(precision)
    B, Ct, H, W = buf.shape
    parts = buf.contiguous().view(torch.int16).view(B, Ct // 8, 2, H, W, 8).permute(2, 0, 1, 5, 3, 4).contiguous().view(2, B, Ct, H, W)
    return parts[0].view(dt), parts[1].view(dt)


class LamaLib:
    def __init__(self, path: Optional[str] = None, host_emulated: bool = False):
        """``host_emulated``: the library is the x86 build of the kernel sources (tests/hipemu) and takes HOST pointers; the
        real library takes device pointers only and every wrapper below refuses CPU tensors."""
        self.host_emulated = host_emulated
        path = path or _DEFAULT                   # (no environment variable chooses the library: tools pass a path -- use_library())
        if not os.path.exists(path):
            raise LamaError(f'{path} not found: build it with `python -m lama_amd.build` '
                            f'(hipcc --offload-arch=gfx950); lama_amd has no fallback path')
        self.path = path
        L = self._l = C.CDLL(path)
        i32, i64, vp, sz = C.c_int32, C.c_int64, C.c_void_p, C.c_size_t
        T = C.POINTER(Tensor4)
        L.lama_version.restype = C.c_int
        L.lama_error_string.restype = C.c_char_p
        L.lama_error_string.argtypes = [C.c_int]
        L.lama_conv2d_packed_weight_bytes.restype = i64
        L.lama_conv2d_packed_weight_bytes.argtypes = [i32] * 7
        L.lama_conv2d_pack_weight.restype = C.c_int
        L.lama_conv2d_pack_weight.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.lama_conv2d_fwd.restype = C.c_int
        L.lama_conv2d_fwd.argtypes = [vp, C.POINTER(Conv2dArgs)]
        L.lama_conv2d_list_fwd.restype, L.lama_conv2d_list_fwd.argtypes = C.c_int, [vp, C.POINTER(Conv2dArgs), vp, vp, i32]
        L.lama_conv2d_list_supported.restype, L.lama_conv2d_list_supported.argtypes = i32, [C.POINTER(Conv2dArgs), i32]
        L.lama_conv2d_route_query.restype = C.c_int
        L.lama_conv2d_route_query.argtypes = [C.POINTER(Conv2dArgs), i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.lama_tail_lists_workspace_bytes.restype, L.lama_tail_lists_workspace_bytes.argtypes = sz, [i32, i32, i32, C.POINTER(TailLists)]
        L.lama_tail_lists_build.restype, L.lama_tail_lists_build.argtypes = C.c_int, [vp, T, i32, C.POINTER(TailLists), vp, sz]
        L.lama_rfft2_fwd.restype = C.c_int
        L.lama_rfft2_fwd.argtypes = [vp, T, T, i32, vp, sz]
        L.lama_irfft2_fwd.restype = C.c_int
        L.lama_irfft2_fwd.argtypes = [vp, T, T, T, i32, vp, sz]
        L.lama_winograd_out_fwd.restype = C.c_int
        L.lama_winograd_out_fwd.argtypes = [vp, C.POINTER(Conv2dArgs), vp, sz]
        L.lama_rfft2_winograd_out_fwd.restype = C.c_int
        L.lama_rfft2_winograd_out_fwd.argtypes = [vp, T, T, i32, vp, sz, C.POINTER(Conv2dArgs), vp, sz]
        L.lama_rfft2_masked_fwd.restype = C.c_int
        L.lama_rfft2_masked_fwd.argtypes = [vp, T, T, T, i32, vp, sz]
        L.lama_irfft2_masked_fwd.restype = C.c_int
        L.lama_irfft2_masked_fwd.argtypes = [vp, T, T, T, T, i32, vp, sz]
        L.lama_fft_workspace_bytes.restype = sz
        L.lama_fft_workspace_bytes.argtypes = [i32] * 4
        L.lama_fft_route_query.restype = C.c_int
        L.lama_fft_route_query.argtypes = [T, T, T, T, i32, i32, vp, sz, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.lama_fourier_unit_workspace_bytes.restype = sz
        L.lama_fourier_unit_workspace_bytes.argtypes = [i32] * 4
        L.lama_fourier_unit_fwd.restype = C.c_int
        L.lama_fourier_unit_fwd.argtypes = [vp, T, vp, vp, T, i32, i32, i32, vp, sz, vp]
        L.lama_fourier_unit_winograd_out_fwd.restype = C.c_int
        L.lama_fourier_unit_winograd_out_fwd.argtypes = [vp, T, vp, vp, T, i32, i32, i32, vp, sz, vp, C.POINTER(Conv2dArgs), vp, sz]
        L.lama_fourier_unit_ex_fwd.restype = C.c_int
        L.lama_fourier_unit_ex_fwd.argtypes = [vp, T, vp, vp, T, i32, i32, i32, vp, sz, vp, i32, C.POINTER(Conv2dArgs), vp, sz]
        L.lama_mask_compose_fwd.restype = C.c_int
        L.lama_mask_compose_fwd.argtypes = [vp, T, T, T, i32]
        L.lama_blend_fwd.restype = C.c_int
        L.lama_blend_fwd.argtypes = [vp, T, T, T, T, i32]
        L.lama_quantize_u8_hwc_fwd.restype = C.c_int
        L.lama_quantize_u8_hwc_fwd.argtypes = [vp, T, vp, i32, i32, i32]
        L.lama_mask_compose_u8_fwd.restype = C.c_int
        L.lama_mask_compose_u8_fwd.argtypes = [vp, vp, vp, vp, T, i32, i32]
        L.lama_blend_quantize_u8_fwd.restype = C.c_int
        L.lama_blend_quantize_u8_fwd.argtypes = [vp, vp, vp, vp, T, vp, i32, i32]
        L.lama_resize_u8_fwd.restype = C.c_int
        L.lama_resize_u8_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.c_double, T, T, i32, i32]
        L.lama_paste_back_u8_fwd.restype = C.c_int
        L.lama_paste_back_u8_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, T, vp, i32, i32]
        L.lama_crop_compose_u8_fwd.restype = C.c_int
        L.lama_crop_compose_u8_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, T, i32, i32]
        L.lama_crop_paste_u8_fwd.restype = C.c_int
        L.lama_crop_paste_u8_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, T, vp, i32, i32]
        L.lama_crop_shrink_compose_u8_fwd.restype = C.c_int
        L.lama_crop_shrink_compose_u8_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, T, i32, i32]
        L.lama_crop_shrink_paste_u8_fwd.restype = C.c_int
        L.lama_crop_shrink_paste_u8_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, T, vp, i32, i32]
        L.lama_png_deflate_bound.restype, L.lama_png_deflate_bound.argtypes = sz, [i32] * 4
        L.lama_png_deflate_workspace_bytes.restype, L.lama_png_deflate_workspace_bytes.argtypes = C.c_int, [i32] * 5 + [C.POINTER(sz)]
        L.lama_png_deflate_u8_fwd.restype = C.c_int
        L.lama_png_deflate_u8_fwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, sz]
        L.lama_jpeg_scan_bound.restype, L.lama_jpeg_scan_bound.argtypes = sz, [i32] * 3
        L.lama_jpeg_scan_workspace_bytes.restype, L.lama_jpeg_scan_workspace_bytes.argtypes = C.c_int, [i32] * 4 + [C.POINTER(sz)]
        L.lama_jpeg_scan_u8_fwd.restype = C.c_int
        L.lama_jpeg_scan_u8_fwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, sz]
        L.lama_eval_ingest_u8_fwd.restype = C.c_int
        L.lama_eval_ingest_u8_fwd.argtypes = [vp, vp, vp, vp, C.POINTER(i32), i32, i32, i32, i32, C.c_float, C.c_float, T, T, vp, i32]
        L.lama_affine_act_fwd.restype = C.c_int
        L.lama_affine_act_fwd.argtypes = [vp, T, vp, vp, i32, T, i32]
        L.lama_reflect_pad_fwd.restype = C.c_int
        L.lama_reflect_pad_fwd.argtypes = [vp, T, i32, T, i32]
        f32, dp = C.c_float, C.POINTER(C.c_double)
        for name, args in (('lama_act_bwd', [vp, T, T, i32, T, i32]), ('lama_add_fwd', [vp, T, T, T, i32]),
                           ('lama_reflect_pad_bwd', [vp, T, T, i32, T, i32]), ('lama_reflect_pad_bwd_fused', [vp, T, T, T, i32, T, i32, T, T, i32, vp]),
                           ('lama_dgrad_ring_fwd', [vp, T, vp, i32, vp, i32]),
                           ('lama_gauss5_fwd', [vp, T, T, i32]),
                           ('lama_gauss5_bwd', [vp, T, T, i32]), ('lama_bilinear_fwd', [vp, T, T, i32]),
                           ('lama_bilinear_bwd', [vp, T, T, i32]), ('lama_threshold_fwd', [vp, T, f32, T, i32]),
                           ('lama_erode_fwd', [vp, T, vp, i32, i32, f32, T, i32]),
                           ('lama_l1_masked_fwd', [vp, T, T, T, f32, i32, vp, i32]),
                           ('lama_l1_masked_bwd', [vp, T, T, T, f32, i32, f32, i32, T, i32]),
                           ('lama_l1_masked_per_image_fwd', [vp, T, T, T, f32, i32, vp, i32]),
                           ('lama_l1_masked_per_image_bwd', [vp, T, T, T, f32, i32, vp, i32, T, i32]),
                           ('lama_adam_step', [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, i32])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        L.lama_dgrad_ring_bytes.restype, L.lama_dgrad_ring_bytes.argtypes = C.c_size_t, [i32, i32, i32, i32]
        L.lama_ssim_workspace_bytes.restype, L.lama_ssim_workspace_bytes.argtypes = C.c_size_t, [i32, i32, i32, i32]
        L.lama_ssim_fwd.restype, L.lama_ssim_fwd.argtypes = C.c_int, [vp, T, T, i32, i32, C.POINTER(C.c_float), vp, vp, C.c_size_t]
        L.lama_lpips_scale_fwd.restype, L.lama_lpips_scale_fwd.argtypes = C.c_int, [vp, T, T, T, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.lama_lpips_layer_workspace_bytes.restype, L.lama_lpips_layer_workspace_bytes.argtypes = C.c_size_t, [i32, i32, i32, i32]
        L.lama_lpips_layer_fwd.restype, L.lama_lpips_layer_fwd.argtypes = C.c_int, [vp, T, T, i32, vp, vp, T, T, vp, C.c_size_t]
        L.lama_fuse1_channel_order.restype, L.lama_fuse1_channel_order.argtypes = None, [C.POINTER(C.c_int32)]
        L.lama_winograd_packed_weight_bytes.restype, L.lama_winograd_packed_weight_bytes.argtypes = C.c_int64, [i32, i32, i32]
        L.lama_winograd_pack_weight.restype, L.lama_winograd_pack_weight.argtypes = C.c_int, [vp, vp, vp, i32, i32, i32, vp]
        L.lama_winograd_workspace_bytes.restype, L.lama_winograd_workspace_bytes.argtypes = C.c_size_t, [i32, i32, i32, i32]
        L.lama_winograd_supported.restype, L.lama_winograd_supported.argtypes = i32, [i32, i32, i32, i32, i32]
        L.lama_winograd_preferred.restype, L.lama_winograd_preferred.argtypes = i32, [i32, i32, i32, i32, i32, i32]
        L.lama_winograd_conv3x3_fwd.restype, L.lama_winograd_conv3x3_fwd.argtypes = C.c_int, [vp, C.POINTER(Conv2dArgs), vp, C.c_size_t]
        L.lama_multidilated_conv3x3_fwd.restype, L.lama_multidilated_conv3x3_fwd.argtypes = C.c_int, [vp, C.POINTER(Conv2dArgs), i32, i32]
        L.lama_conv2d_rect_packed_weight_bytes.restype, L.lama_conv2d_rect_packed_weight_bytes.argtypes = i64, [i32] * 5
        L.lama_conv2d_rect_pack_weight.restype, L.lama_conv2d_rect_pack_weight.argtypes = C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp]
        L.lama_conv2d_rect_fwd.restype, L.lama_conv2d_rect_fwd.argtypes = C.c_int, [vp, C.POINTER(Conv2dRectArgs)]
        L.lama_pool3x3_fwd.restype, L.lama_pool3x3_fwd.argtypes = C.c_int, [vp, T, T, i32, i32, i32, i32]
        L.lama_global_avgpool_fwd.restype, L.lama_global_avgpool_fwd.argtypes = C.c_int, [vp, T, vp, i32]
        L.lama_fid_input_fwd.restype, L.lama_fid_input_fwd.argtypes = C.c_int, [vp, T, T, T, i32, i32]
        L.lama_range_stats_workspace_bytes.restype, L.lama_range_stats_workspace_bytes.argtypes = sz, [i32] * 4
        L.lama_range_stats_fwd.restype, L.lama_range_stats_fwd.argtypes = C.c_int, [vp, T, i32, C.c_float, vp, vp, sz]
        L.lama_fourier_unit_workspace_views.restype, L.lama_fourier_unit_workspace_views.argtypes = C.c_int, [i32, i32, i32, i32, i32, vp, sz, T, T]
        L.lama_lfu_gather_fwd.restype, L.lama_lfu_gather_fwd.argtypes = C.c_int, [vp, T, T, i32]
        L.lama_lfu_tile_add_fwd.restype, L.lama_lfu_tile_add_fwd.argtypes = C.c_int, [vp, T, T, T, i32]
        del dp
        if L.lama_version() != ABI_VERSION:
            raise LamaError(f'{path}: ABI version {L.lama_version()} != {ABI_VERSION}')

    # -- helpers -------------------------------------------------------------------------------
    def check(self, rc: int, what: str):
        if rc != 0:
            raise LamaError(f'{what} failed: {self._l.lama_error_string(rc).decode()} (code {rc})', code=int(rc))

    @staticmethod
    def stream_of(t: torch.Tensor) -> int:
        return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0

    # -- conv ------------------------------------------------------------------------------------
    def pack_conv_weight(self, w: torch.Tensor, scale: Optional[torch.Tensor], stride: int = 1, transposed: bool = False,
                         precision: int = PREC_F32) -> torch.Tensor:
        """Reference-layout conv weight (+ folded BN scale) -> packed device buffer."""
        if not self.host_emulated and not w.is_cuda:
            raise LamaError('pack_conv_weight: the weights are on the CPU (e.g. after load_checkpoint(map_location="cpu")): move the '
                            'module to the GPU first (model.to("cuda")) -- the HIP kernels dereference device pointers only')
        w = w.contiguous().float()
        if scale is not None and scale.device != w.device:
            raise LamaError(f'pack_conv_weight: weight on {w.device} but BatchNorm scale on {scale.device}')
        if transposed:
            cin, cout, kh, kw = w.shape
        else:
            cout, cin, kh, kw = w.shape
        nbytes = self._l.lama_conv2d_packed_weight_bytes(cout, cin, kh, kw, stride, int(transposed), precision)
        if nbytes <= 0:
            raise LamaError(f'unsupported conv geometry {tuple(w.shape)} stride={stride} transposed={transposed}')
        if precision in (PREC_F16X3, PREC_F16) and w.numel():
            # the fp16 split of the WEIGHTS is checked here, once (activations: range_flag of lama_conv2d_args)
            ws = w if scale is None else w * (scale.float().view(1, -1, 1, 1) if transposed else scale.float().view(-1, 1, 1, 1))
            amax = float(ws.abs().max())
            if not amax <= F16_MAX:
                raise LamaRangeError(f'folded conv weight |w| max {amax:.3g} exceeds the fp16 split range ({F16_MAX}); use bf16x3 or f32')
        dst = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        sc = None if scale is None else scale.contiguous().float()
        self.check(self._l.lama_conv2d_pack_weight(self.stream_of(w), w.data_ptr(), None if sc is None else sc.data_ptr(),
                                                   cout, cin, kh, kw, stride, int(transposed), precision, dst.data_ptr()),
                   'lama_conv2d_pack_weight')
        if w.is_cuda:
            torch.cuda.current_stream(w.device).synchronize()  # w / sc may be temporaries
        return dst

    def conv2d(self, x: Tensor4, w_packed: torch.Tensor, y: Tensor4, batch: int, k: int, stride: int = 1, pad: int = 0,
               pad_mode: int = PAD_REFLECT, transposed: bool = False, bias: Optional[torch.Tensor] = None,
               act: int = ACT_NONE, resid: Optional[Tensor4] = None, x2: Optional[Tensor4] = None,
               w2_packed: Optional[torch.Tensor] = None, precision: int = PREC_F32, stream: int = 0,
               range_flag: Optional[torch.Tensor] = None, fuse1: Optional[tuple] = None, cooperative: bool = False, siblings_log2: int = 0,
               tile_list: Optional[tuple] = None, query: bool = False, route: bool = False):
        """``fuse1`` = (packed conv1 weights with the channel order of fuse1_channel_order(), BatchNorm shift [192], x1 view): the NEXT
        layer's SpectralTransform.conv1 in the epilogue of this (global-branch) launch -- lama_conv2d_args.fuse1_*.  ``siblings_log2`` (v109):
        this launch covers 1 / 2^n of a batch whose other parts run beside it (LAMA_CONV_SIBLINGS_*).  ``tile_list`` = (list, count, head_rs), the
        int32 tensors of ``tail_lists_alloc``: lama_conv2d_list_fwd, the launch over the listed work units only (LamaError with code ERR_UNSUPPORTED
        where the dedicated kernels do not take the shape); with ``query`` nothing is launched and the verdict is returned
        (lama_conv2d_list_supported).  ``route``: nothing is launched either; returns (code, family, geometry) of lama_conv2d_route_query
        for exactly these arguments (family and geometry are None unless code == 0)."""
        a = Conv2dArgs()
        a.x, a.w_packed = x, w_packed.data_ptr()
        a.kh = a.kw = k
        a.stride, a.pad, a.pad_mode, a.transposed = stride, pad, pad_mode, int(transposed)
        if x2 is not None:
            a.x2, a.w2_packed = x2, w2_packed.data_ptr()
        a.bias = None if bias is None else bias.data_ptr()
        a.act = act
        if resid is not None:
            a.resid = resid
        a.y, a.batch, a.precision = y, batch, precision
        a.range_flag = None if range_flag is None else range_flag.data_ptr()
        if fuse1 is not None:
            a.fuse1_w, a.fuse1_bias, a.fuse1_y = fuse1[0].data_ptr(), fuse1[1].data_ptr(), fuse1[2]
        a.flags = (CONV_COOPERATIVE if cooperative else 0) | (int(siblings_log2) << CONV_SIBLINGS_SHIFT)   # lama_conv2d_args.flags
        if route:
            fam, geo = C.c_int32(-1), C.c_int32(-1)
            rc = self._l.lama_conv2d_route_query(C.byref(a), -1 if tile_list is None else int(tile_list[2]), C.byref(fam), C.byref(geo))
            return (int(rc), fam.value, geo.value) if rc == 0 else (int(rc), None, None)
        if tile_list is not None:
            lst, cnt, head_rs = tile_list
            if query:
                return self._l.lama_conv2d_list_supported(C.byref(a), int(head_rs)) == 1
            self.check(self._l.lama_conv2d_list_fwd(stream, C.byref(a), lst.data_ptr(), cnt.data_ptr(), int(head_rs)), 'lama_conv2d_list_fwd')
            return None
        self.check(self._l.lama_conv2d_fwd(stream, C.byref(a)), 'lama_conv2d_fwd')

    # -- work lists of the sparse tail (lama_tail_lists_*) ------------------------------------------------
    def tail_lists_alloc(self, batch: int, H: int, W: int, head_rs: int, up_mg, device) -> dict:
        """The plan-owned buffers of lama_tail_lists_build for a [batch, ., H, W] head plane behind len(up_mg) upsamplings (up_mg[0] = Cout / 64 of
        the one that feeds the head): ``head`` and ``up[i]`` = (int32 list with room for every unit, int32 count [1]), the flag workspace and the
        argument block.  Zero-filled: an entry is a valid unit index before the first build."""
        n_up = len(up_mg)
        if n_up > 4 or H % (1 << n_up) or W % (1 << n_up) or head_rs < 8 or head_rs % 8:
            raise LamaError(f'tail lists: {n_up} upsamplings of a {H} x {W} plane, head_rs {head_rs}')

        def pair(n):
            return torch.zeros(n, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32, device=device)

        cd = lambda a, b: (a + b - 1) // b
        head = pair(batch * cd(W, 26) * cd(H, head_rs))
        up = [pair(batch * cd(H >> (i + 1), 4) * cd(W >> (i + 1), 32) * int(up_mg[i])) for i in range(n_up)]
        a = TailLists()
        a.n_up, a.head_rs = n_up, head_rs
        a.head_list, a.head_count = head[0].data_ptr(), head[1].data_ptr()
        for i in range(n_up):
            a.up_mg[i] = int(up_mg[i])
            a.up_list[i], a.up_count[i] = up[i][0].data_ptr(), up[i][1].data_ptr()
        nbytes = self._l.lama_tail_lists_workspace_bytes(batch, H, W, C.byref(a))
        if nbytes <= 0:
            raise LamaError(f'tail lists: unsupported geometry {batch} x {H} x {W}')
        ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=device)
        return dict(head=head, up=up, ws=ws, args=a, head_rs=head_rs, batch=batch, H=H, W=W)

    def tail_lists_build(self, mask: Tensor4, lists: dict, stream: int = 0):
        """lama_tail_lists_build: ``mask`` = the [batch, 1, H, W] view of channel 3 of the generator's input; fills ``lists`` (tail_lists_alloc)."""
        ws = lists['ws']
        self.check(self._l.lama_tail_lists_build(stream, C.byref(mask), lists['batch'], C.byref(lists['args']), ws.data_ptr(), ws.numel() * 4),
                   'lama_tail_lists_build')

    # -- Winograd F(2x2, 3x3) form of the stride-1 3x3 reflect conv (lama_winograd_*) -----------------
    def winograd_supported(self, cout: int, cin: int, H: int, W: int, precision: int) -> bool:
        return (precision in (PREC_F16X3, PREC_BF16X3) and self._l.lama_winograd_packed_weight_bytes(cout, cin, precision) > 0
                and self._l.lama_winograd_supported(cout, cin, H, W, precision) == 1)

    def winograd_preferred(self, batch: int, cout: int, cin: int, H: int, W: int, precision: int) -> bool:
        """(v110) supported AND expected to beat the direct kernel at this batch (the any-size geometry pays for whole rounds of workgroups)."""
        return self.winograd_supported(cout, cin, H, W, precision) and self._l.lama_winograd_preferred(batch, cout, cin, H, W, precision) == 1

    def winograd_workspace_bytes(self, batch: int, cout: int, H: int, W: int) -> int:
        return int(self._l.lama_winograd_workspace_bytes(batch, cout, H, W))

    def pack_winograd_weight(self, w: torch.Tensor, scale: Optional[torch.Tensor], precision: int) -> torch.Tensor:
        """Conv2d weight [Cout, Cin, 3, 3] (+ folded BN scale) -> packed U = G g G^T fragments (lama_winograd_pack_weight)."""
        if not self.host_emulated and not w.is_cuda:
            raise LamaError('pack_winograd_weight: the weights are on the CPU: move the module to the GPU first')
        w = w.contiguous().float()
        cout, cin, kh, kw = w.shape
        nbytes = self._l.lama_winograd_packed_weight_bytes(cout, cin, precision) if (kh, kw) == (3, 3) else -1
        if nbytes <= 0:
            raise LamaError(f'unsupported Winograd geometry {tuple(w.shape)} / precision {precision}', code=ERR_UNSUPPORTED)
        if precision == PREC_F16X3 and w.numel():
            ws = w if scale is None else w * scale.float().view(-1, 1, 1, 1)
            amax = float(ws.abs().sum(dim=(2, 3)).max())        # |U| <= sum |g| (the rows of G have absolute sum <= 1.5, squared 2.25 > needed)
            if not 2.25 * amax <= F16_MAX:
                raise LamaRangeError(f'transformed conv weight bound {2.25 * amax:.3g} exceeds the fp16 split range ({F16_MAX}); use bf16x3')
        dst = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        sc = None if scale is None else scale.contiguous().float()
        self.check(self._l.lama_winograd_pack_weight(self.stream_of(w), w.data_ptr(), None if sc is None else sc.data_ptr(), cout, cin,
                                                     precision, dst.data_ptr()), 'lama_winograd_pack_weight')
        if w.is_cuda:
            torch.cuda.current_stream(w.device).synchronize()
        return dst

    def winograd_conv3x3(self, x: Tensor4, w_packed: torch.Tensor, y: Tensor4, batch: int, ws: torch.Tensor, bias: Optional[torch.Tensor] = None,
                         act: int = ACT_NONE, resid: Optional[Tensor4] = None, precision: int = PREC_F16X3, stream: int = 0,
                         range_flag: Optional[torch.Tensor] = None, pad_mode: int = PAD_REFLECT, defer_out: bool = False, siblings_log2: int = 0):
        """``defer_out`` (v108): only the GEMM launch; returns the argument block the caller hands to ``winograd_out`` / ``rfft2_wino_out``
        (with the same workspace) before anything reads y."""
        a = Conv2dArgs()
        a.x, a.w_packed = x, w_packed.data_ptr()
        a.kh = a.kw = 3
        a.stride, a.pad, a.pad_mode, a.transposed = 1, 1, pad_mode, 0
        a.bias = None if bias is None else bias.data_ptr()
        a.act = act
        if resid is not None:
            a.resid = resid
        a.y, a.batch, a.precision = y, batch, precision
        a.range_flag = None if range_flag is None else range_flag.data_ptr()
        a.flags = (CONV_DEFER_OUT if defer_out else 0) | (int(siblings_log2) << CONV_SIBLINGS_SHIFT)
        self.check(self._l.lama_winograd_conv3x3_fwd(stream, C.byref(a), ws.data_ptr(), ws.numel() * ws.element_size()), 'lama_winograd_conv3x3_fwd')
        return a if defer_out else None

    def multidilated_conv3x3(self, x: Tensor4, w_packed: torch.Tensor, y: Tensor4, batch: int, groups: int, min_dilation: int = 1,
                             bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, resid: Optional[Tensor4] = None,
                             precision: int = PREC_F16X3, stream: int = 0, range_flag: Optional[torch.Tensor] = None):
        """(v112) lama_multidilated_conv3x3_fwd: ``groups`` dilated 3x3 reflect convs (dilation min_dilation * 2^j) over the channel chunks of x,
        summed, + bias, activation and residual in one launch.  ``w_packed``: ``pack_conv_weight`` of the group weights concatenated along Cin."""
        a = Conv2dArgs()
        a.x, a.w_packed = x, w_packed.data_ptr()
        a.kh = a.kw = 3
        a.stride, a.pad, a.pad_mode, a.transposed = 1, min_dilation, PAD_REFLECT, 0
        a.bias = None if bias is None else bias.data_ptr()
        a.act = act
        if resid is not None:
            a.resid = resid
        a.y, a.batch, a.precision = y, batch, precision
        a.range_flag = None if range_flag is None else range_flag.data_ptr()
        self.check(self._l.lama_multidilated_conv3x3_fwd(stream, C.byref(a), groups, min_dilation), 'lama_multidilated_conv3x3_fwd')

    def winograd_out(self, args: 'Conv2dArgs', ws: torch.Tensor, stream: int = 0):
        """The output transform a ``winograd_conv3x3(..., defer_out=True)`` call left out (lama_winograd_out_fwd)."""
        self.check(self._l.lama_winograd_out_fwd(stream, C.byref(args), ws.data_ptr(), ws.numel() * ws.element_size()), 'lama_winograd_out_fwd')

    def rfft2_wino_out(self, x: Tensor4, spec: Tensor4, batch: int, ws: Optional[torch.Tensor], wino_args: 'Conv2dArgs', wino_ws: torch.Tensor,
                       stream: int = 0):
        """rfft2 + the deferred Winograd output transform of the layer before in one launch (lama_rfft2_winograd_out_fwd; ERR_UNSUPPORTED where
        no kernel does it: the caller then runs the two separately)."""
        self.check(self._l.lama_rfft2_winograd_out_fwd(stream, C.byref(x), C.byref(spec), batch, None if ws is None else ws.data_ptr(),
                                                       0 if ws is None else ws.numel() * ws.element_size(), C.byref(wino_args), wino_ws.data_ptr(),
                                                       wino_ws.numel() * wino_ws.element_size()), 'lama_rfft2_winograd_out_fwd')

    def fuse1_channel_order(self) -> torch.Tensor:
        """Input-channel order of a conv1 weight that rides in another launch's epilogue (lama_fuse1_channel_order)."""
        buf = (C.c_int32 * 384)()
        self._l.lama_fuse1_channel_order(buf)
        return torch.tensor(list(buf), dtype=torch.long)

    # -- fft -------------------------------------------------------------------------------------
    def fft_workspace_bytes(self, b, c, h, w) -> int:
        return int(self._l.lama_fft_workspace_bytes(b, c, h, w))

    def fft_route_query(self, real: Tensor4, resid: Optional[Tensor4], spec: Tensor4, batch: int, inverse: bool, ws_addr: Optional[int] = None,
                        ws_bytes: int = 0, mask: Optional[Tensor4] = None):
        """(code, family, kind) of lama_fft_route_query: the return code ``rfft2`` / ``irfft2`` (``inverse``; with ``mask`` the masked entries) give
        for these views and this workspace ADDRESS, and on 0 the kernel family 1 .. 6 and FFT_KIND_* / threads per workgroup / 0.  Host only:
        nothing is launched, no pointer is dereferenced, so the addresses need not be real."""
        fam, kind = C.c_int32(-1), C.c_int32(-1)
        rc = self._l.lama_fft_route_query(C.byref(real), None if resid is None else C.byref(resid), C.byref(spec), None if mask is None else C.byref(mask),
                                          batch, int(bool(inverse)), ws_addr, ws_bytes, C.byref(fam), C.byref(kind))
        return (int(rc), None, None) if rc else (0, fam.value, kind.value)

    def rfft2(self, x: Tensor4, spec: Tensor4, batch: int, ws: Optional[torch.Tensor] = None, stream: int = 0, mask: Optional[Tensor4] = None):
        """``mask``: spec *= [mask > 0] in the same launch (lama_rfft2_masked_fwd; LamaError ERR_UNSUPPORTED where no kernel does it)."""
        if mask is not None:
            self.check(self._l.lama_rfft2_masked_fwd(stream, C.byref(x), C.byref(spec), C.byref(mask), batch,
                                                     None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * ws.element_size()),
                       'lama_rfft2_masked_fwd')
            return
        self.check(self._l.lama_rfft2_fwd(stream, C.byref(x), C.byref(spec), batch,
                                          None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * ws.element_size()),
                   'lama_rfft2_fwd')

    def irfft2(self, spec: Tensor4, resid: Optional[Tensor4], y: Tensor4, batch: int, ws: Optional[torch.Tensor] = None,
               stream: int = 0, mask: Optional[Tensor4] = None):
        if mask is not None:
            self.check(self._l.lama_irfft2_masked_fwd(stream, C.byref(spec), None if resid is None else C.byref(resid), C.byref(mask), C.byref(y), batch,
                                                      None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * ws.element_size()),
                       'lama_irfft2_masked_fwd')
            return
        self.check(self._l.lama_irfft2_fwd(stream, C.byref(spec), None if resid is None else C.byref(resid), C.byref(y), batch,
                                           None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * ws.element_size()),
                   'lama_irfft2_fwd')

    def fourier_unit_workspace_bytes(self, b, c, h, w) -> int:
        return int(self._l.lama_fourier_unit_workspace_bytes(b, c, h, w))

    def fourier_unit(self, x: Tensor4, w_packed: torch.Tensor, bias: torch.Tensor, y: Tensor4, batch: int, add_input: bool,
                     ws: torch.Tensor, precision: int = PREC_F32, stream: int = 0, range_flag: Optional[torch.Tensor] = None,
                     wino_out: Optional[tuple] = None, siblings_log2: int = 0):
        """``wino_out`` = (argument block of a ``winograd_conv3x3(..., defer_out=True)`` call, its workspace): that conv's output transform runs
        inside this FourierUnit's rfft2 launch (lama_fourier_unit_winograd_out_fwd, v108).  ``siblings_log2`` (v109): lama_fourier_unit_ex_fwd."""
        if siblings_log2:
            wa, wws = wino_out if wino_out is not None else (None, None)
            self.check(self._l.lama_fourier_unit_ex_fwd(stream, C.byref(x), w_packed.data_ptr(), bias.data_ptr(), C.byref(y), batch,
                                                        int(add_input), precision, ws.data_ptr(), ws.numel() * ws.element_size(),
                                                        None if range_flag is None else range_flag.data_ptr(), int(siblings_log2) << CONV_SIBLINGS_SHIFT,
                                                        None if wa is None else C.byref(wa), None if wws is None else wws.data_ptr(),
                                                        0 if wws is None else wws.numel() * wws.element_size()),
                       'lama_fourier_unit_ex_fwd')
            return
        if wino_out is not None:
            wa, wws = wino_out
            self.check(self._l.lama_fourier_unit_winograd_out_fwd(stream, C.byref(x), w_packed.data_ptr(), bias.data_ptr(), C.byref(y), batch,
                                                                  int(add_input), precision, ws.data_ptr(), ws.numel() * ws.element_size(),
                                                                  None if range_flag is None else range_flag.data_ptr(), C.byref(wa),
                                                                  wws.data_ptr(), wws.numel() * wws.element_size()),
                       'lama_fourier_unit_winograd_out_fwd')
            return
        self.check(self._l.lama_fourier_unit_fwd(stream, C.byref(x), w_packed.data_ptr(), bias.data_ptr(), C.byref(y), batch,
                                                 int(add_input), precision, ws.data_ptr(), ws.numel() * ws.element_size(),
                                                 None if range_flag is None else range_flag.data_ptr()),
                   'lama_fourier_unit_fwd')

    def fourier_unit_views(self, ws: torch.Tensor, b: int, c: int, h: int, w: int, dtype: int = DT_F32):
        """(spec_in, spec_out): the two [b, 2c, h, w/2+1] spectra a ``fourier_unit`` call on x [b, c, h, w] leaves inside its workspace ``ws`` --
        the operand of the spectral 1x1 and its BN + ReLU output (lama_fourier_unit_workspace_views: the library states the layout)."""
        si, so = Tensor4(), Tensor4()
        self.check(self._l.lama_fourier_unit_workspace_views(b, c, h, w, dtype, ws.data_ptr(), ws.numel() * ws.element_size(), C.byref(si),
                                                             C.byref(so)), 'lama_fourier_unit_workspace_views')
        return si, so

    # -- activation ranges (lama_range_stats_fwd) ------------------------------------------------------
    def range_stats_workspace_bytes(self, batch: int, c: int, h: int, w: int) -> int:
        return int(self._l.lama_range_stats_workspace_bytes(batch, c, h, w))

    def range_stats(self, x: Tensor4, batch: int, limit: float = F16_MAX, stream: int = 0, out: Optional[torch.Tensor] = None,
                    ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-channel range statistics of the view ``x`` over ``batch`` images: an int32 [C, 4] device tensor of lama_range_stats records --
        column 0 holds the BITS of abs_max (fp32), columns 1..3 n_nan, n_inf, n_over (uint32 bits); ``unpack_range_stats`` reads it on the
        host.  ``out`` (int32, at least 4 C elements, overwritten) and ``ws`` (the workspace) are allocated when absent -- a view carries no
        device, so on the other's device, or on the current GPU when neither is given."""
        if out is None:
            dev = ws.device if ws is not None else (torch.device('cpu') if self.host_emulated else torch.device('cuda', torch.cuda.current_device()))
            out = torch.empty(x.C, 4, dtype=torch.int32, device=dev)
        if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < 4 * x.C or (not self.host_emulated and not out.is_cuda):
            raise LamaError(f'range_stats: out is a contiguous device int32 tensor of at least 4 * C elements, got {tuple(out.shape)} {out.dtype}')
        if ws is None:
            ws = torch.empty(max(1, self.range_stats_workspace_bytes(batch, x.C, x.H, x.W) // 4), dtype=torch.int32, device=out.device)
        elif not self.host_emulated and not ws.is_cuda:
            raise LamaError('range_stats: the workspace must be a device tensor')
        self.check(self._l.lama_range_stats_fwd(stream, C.byref(x), batch, float(limit), out.data_ptr(), ws.data_ptr(),
                                                ws.numel() * ws.element_size()), 'lama_range_stats_fwd')
        return out

    # -- local Fourier unit (lfu.hip) ----------------------------------------------------------------
    def lfu_gather(self, x: Tensor4, y: Tensor4, batch: int, stream: int = 0):
        """y [B, 4q, h/2, h/2] = the four quadrants of x [B, q, h, h] stacked along the channels, row half fastest (ffc.py:152-155)."""
        self.check(self._l.lama_lfu_gather_fwd(stream, C.byref(x), C.byref(y), batch), 'lama_lfu_gather_fwd')

    def lfu_tile_add(self, a: Tensor4, xs: Tensor4, out: Tensor4, batch: int, stream: int = 0):
        """out = a + xs.repeat(1, 1, 2, 2) (ffc.py:156-161); ``out`` may be ``a``."""
        self.check(self._l.lama_lfu_tile_add_fwd(stream, C.byref(a), C.byref(xs), C.byref(out), batch), 'lama_lfu_tile_add_fwd')

    # -- elementwise -------------------------------------------------------------------------------
    def mask_compose(self, image: Tensor4, mask: Tensor4, out: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_mask_compose_fwd(stream, C.byref(image), C.byref(mask), C.byref(out), batch), 'lama_mask_compose_fwd')

    def blend(self, image: Tensor4, mask: Tensor4, pred: Tensor4, out: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_blend_fwd(stream, C.byref(image), C.byref(mask), C.byref(pred), C.byref(out), batch), 'lama_blend_fwd')

    def mask_compose_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, sizes, out: Tensor4, batch: int, binarize: bool = True, stream: int = 0):
        """(v110) u8 HWC image [B,Hp,Wp,3] + u8 mask [B,Hp,Wp] (+ int32 sizes [B,2] or None) -> the generator's input [B,4,Hp,Wp] fp32."""
        self.check(self._l.lama_mask_compose_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), None if sizes is None else sizes.data_ptr(),
                                                    C.byref(out), batch, int(bool(binarize))), 'lama_mask_compose_u8_fwd')

    def blend_quantize_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, sizes, pred: Tensor4, dst: torch.Tensor, batch: int,
                          binarize: bool = True, stream: int = 0):
        """(v110) blend (default.py:71) + u8 HWC quantisation (bin/predict.py:86-92) of the generator's output against the u8 operands."""
        self.check(self._l.lama_blend_quantize_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), None if sizes is None else sizes.data_ptr(),
                                                      C.byref(pred), dst.data_ptr(), batch, int(bool(binarize))), 'lama_blend_quantize_u8_fwd')

    @staticmethod
    def _u8_slot_operands(what: str, image_hwc: torch.Tensor, mask: torch.Tensor, batch: int, int32_arrays, out_hwc=None):
        """The operand checks of the entries that read a batch of u8 source slots: image slots [B,Hs,Ws,3] / mask slots [B,Hs,Ws], the
        ``int32_arrays`` (name, tensor, values per image) and, where the entry writes slots, ``out_hwc`` like the image slots."""
        if image_hwc.dim() != 4 or image_hwc.shape[3] != 3 or tuple(mask.shape) != tuple(image_hwc.shape[:3]) or image_hwc.shape[0] < batch:
            raise LamaError(f'{what}: image slots {tuple(image_hwc.shape)} / mask slots {tuple(mask.shape)}: [B,Hs,Ws,3] / [B,Hs,Ws] u8')
        if out_hwc is not None and tuple(out_hwc.shape) != tuple(image_hwc.shape):
            raise LamaError(f'{what}: out slots {tuple(out_hwc.shape)} != image slots {tuple(image_hwc.shape)}')
        u8 = [image_hwc, mask] + ([] if out_hwc is None else [out_hwc])
        for t, dt in [(t, torch.uint8) for t in u8] + [(t, torch.int32) for _, t, _ in int32_arrays]:
            if t.dtype != dt or not t.is_contiguous():
                raise LamaError(f'{what}: a contiguous {dt} tensor is needed, got {t.dtype}')
        if any(t.numel() < n * batch for _, t, n in int32_arrays):
            raise LamaError(f'{what}: ' + ', '.join(f'{name} is [B,{n}] int32' for name, _, n in int32_arrays))

    def resize_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, src_sizes: torch.Tensor, dst_sizes: torch.Tensor, factor: float,
                  out_image: Tensor4, out_mask: Tensor4, batch: int, binarize: bool = True, stream: int = 0):
        """lama_resize_u8_fwd: dataset.scale_factor on the device.  u8 HWC source slots [B,Hs,Ws,3] + u8 mask slots [B,Hs,Ws], int32 (h, w) per
        image of the source and of the scaled result [B,2] -> the loader's fp32 image [B,3,Hp,Wp] / mask [B,1,Hp,Wp] (/ 255, INTER_AREA /
        INTER_NEAREST, symmetric padding, mask > 0), bit-identical to ``predict.load_item``."""
        self._u8_slot_operands('resize_u8', image_hwc, mask, batch, [('src_sizes', src_sizes, 2), ('dst_sizes', dst_sizes, 2)])
        self.check(self._l.lama_resize_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), src_sizes.data_ptr(), dst_sizes.data_ptr(),
                                              int(image_hwc.shape[1]), int(image_hwc.shape[2]), float(factor), C.byref(out_image), C.byref(out_mask),
                                              batch, int(bool(binarize))), 'lama_resize_u8_fwd')

    def paste_back_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, src_sizes: torch.Tensor, dst_sizes: torch.Tensor, lowres: Tensor4,
                      out_hwc: torch.Tensor, batch: int, binarize: bool = True, stream: int = 0):
        """lama_paste_back_u8_fwd: the fp32 result ``lowres`` [B,3,Hp,Wp] of a ``scale_factor`` step (valid in [:dh, :dw] per image) resampled
        bilinearly to each image's source grid and pasted into the u8 source slots [B,Hs,Ws,3] wherever the u8 mask [B,Hs,Ws] is not 0 ->
        ``out_hwc`` [B,Hs,Ws,3] u8 (another buffer than ``image_hwc``).  Source pixels pass through byte for byte where the mask is 0."""
        self._u8_slot_operands('paste_back_u8', image_hwc, mask, batch, [('src_sizes', src_sizes, 2), ('dst_sizes', dst_sizes, 2)], out_hwc)
        self.check(self._l.lama_paste_back_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), src_sizes.data_ptr(), dst_sizes.data_ptr(),
                                                  int(image_hwc.shape[1]), int(image_hwc.shape[2]), C.byref(lowres), out_hwc.data_ptr(), batch,
                                                  int(bool(binarize))), 'lama_paste_back_u8_fwd')

    def crop_compose_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, src_sizes: torch.Tensor, rects: torch.Tensor, out: Tensor4, batch: int,
                        binarize: bool = True, stream: int = 0):
        """lama_crop_compose_u8_fwd: the generator's input [B,4,Hp,Wp] fp32 from the window ``rects`` [B,4] = (y0, x0, ch, cw) of each u8 source slot
        [B,Hs,Ws,3] / mask slot [B,Hs,Ws] -- what ``mask_compose_u8`` writes for the cropped arrays with sizes (ch, cw), bit for bit."""
        self._u8_slot_operands('crop_compose_u8', image_hwc, mask, batch, [('src_sizes', src_sizes, 2), ('rects', rects, 4)])
        self.check(self._l.lama_crop_compose_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), src_sizes.data_ptr(), rects.data_ptr(),
                                                    int(image_hwc.shape[1]), int(image_hwc.shape[2]), C.byref(out), batch, int(bool(binarize))),
                   'lama_crop_compose_u8_fwd')

    def crop_paste_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, src_sizes: torch.Tensor, rects: torch.Tensor, pred: Tensor4,
                      out_hwc: torch.Tensor, batch: int, binarize: bool = True, stream: int = 0):
        """lama_crop_paste_u8_fwd: ``out_hwc`` [B,Hs,Ws,3] u8 (another buffer than ``image_hwc``) = the source slots with, inside each window, the
        bytes ``blend_quantize_u8`` gives for the cropped arrays and the generator's output ``pred`` [B,3,Hp,Wp] of the window."""
        self._u8_slot_operands('crop_paste_u8', image_hwc, mask, batch, [('src_sizes', src_sizes, 2), ('rects', rects, 4)], out_hwc)
        self.check(self._l.lama_crop_paste_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), src_sizes.data_ptr(), rects.data_ptr(),
                                                  int(image_hwc.shape[1]), int(image_hwc.shape[2]), C.byref(pred), out_hwc.data_ptr(), batch,
                                                  int(bool(binarize))), 'lama_crop_paste_u8_fwd')

    def crop_shrink_compose_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, src_sizes: torch.Tensor, rects: torch.Tensor, shrinks: torch.Tensor,
                               out: Tensor4, batch: int, binarize: bool = True, stream: int = 0):
        """lama_crop_shrink_compose_u8_fwd (no counterpart in the reference): the generator's input [B,4,Hp,Wp] fp32 from the window ``rects`` of each
        u8 source slot, shrunk by the integer ``shrinks`` [B] = k (1 .. 16): k x k box means of the image (resize_u8's integer-shrink arithmetic),
        the MAX of each box's mask bytes, symmetric padding of the ceil(ch / k) x ceil(cw / k) planes."""
        self._u8_slot_operands('crop_shrink_compose_u8', image_hwc, mask, batch, [('src_sizes', src_sizes, 2), ('rects', rects, 4), ('shrinks', shrinks, 1)])
        self.check(self._l.lama_crop_shrink_compose_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), src_sizes.data_ptr(), rects.data_ptr(),
                                                           shrinks.data_ptr(), int(image_hwc.shape[1]), int(image_hwc.shape[2]), C.byref(out), batch,
                                                           int(bool(binarize))), 'lama_crop_shrink_compose_u8_fwd')

    def crop_shrink_paste_u8(self, image_hwc: torch.Tensor, mask: torch.Tensor, src_sizes: torch.Tensor, rects: torch.Tensor, shrinks: torch.Tensor,
                             lowres: Tensor4, out_hwc: torch.Tensor, batch: int, binarize: bool = True, stream: int = 0):
        """lama_crop_shrink_paste_u8_fwd: ``out_hwc`` [B,Hs,Ws,3] u8 (another buffer than ``image_hwc``) = the source slots with, inside each window
        and under the mask, the bytes ``paste_back_u8`` gives for the cropped arrays and ``lowres`` [B,3,Hp,Wp] (valid in [:ceil(ch / k),
        :ceil(cw / k)]): a k-fold bilinear upsampling of the generator's output."""
        self._u8_slot_operands('crop_shrink_paste_u8', image_hwc, mask, batch, [('src_sizes', src_sizes, 2), ('rects', rects, 4), ('shrinks', shrinks, 1)],
                               out_hwc)
        self.check(self._l.lama_crop_shrink_paste_u8_fwd(stream, image_hwc.data_ptr(), mask.data_ptr(), src_sizes.data_ptr(), rects.data_ptr(),
                                                         shrinks.data_ptr(), int(image_hwc.shape[1]), int(image_hwc.shape[2]), C.byref(lowres),
                                                         out_hwc.data_ptr(), batch, int(bool(binarize))), 'lama_crop_shrink_paste_u8_fwd')

    def png_deflate_bound(self, h: int, w: int, channels: int = 3, chunk_bytes: int = 0) -> int:
        """lama_png_deflate_bound: the most bytes the stream of one h x w image can take (0: empty, or arguments the encoder refuses)."""
        return int(self._l.lama_png_deflate_bound(int(h), int(w), int(channels), int(chunk_bytes)))

    def png_deflate_workspace_bytes(self, batch: int, Hs: int, Ws: int, channels: int = 3, chunk_bytes: int = 0) -> int:
        n = C.c_size_t(0)
        self.check(self._l.lama_png_deflate_workspace_bytes(int(batch), int(Hs), int(Ws), int(channels), int(chunk_bytes), C.byref(n)),
                   'lama_png_deflate_workspace_bytes')
        return int(n.value)

    def png_deflate_u8(self, image_hwc: torch.Tensor, sizes: torch.Tensor, out: torch.Tensor, out_stride: int, out_bytes: torch.Tensor,
                       workspace: torch.Tensor, batch: int, chunk_bytes: int = 0, stream: int = 0):
        """lama_png_deflate_u8_fwd: the zlib stream (Sub filter, literal-only dynamic Huffman chunks; tests/png_ref.py) of the h x w crop of every
        u8 slot of ``image_hwc`` [B,Hs,Ws,3] / [B,Hs,Ws,1] / [B,Hs,Ws], ``sizes`` = device int32 [B,2], into ``out`` (flat u8: slot j starts at
        byte j * ``out_stride``) and its length into ``out_bytes`` (int32 [B]; 0 for an empty slot).  Two launches, asynchronous, capturable."""
        if image_hwc.dim() not in (3, 4) or (image_hwc.dim() == 4 and image_hwc.shape[3] not in (1, 3)) or image_hwc.shape[0] < batch:
            raise LamaError(f'png_deflate_u8: image slots {tuple(image_hwc.shape)}: [B,Hs,Ws,3], [B,Hs,Ws,1] or [B,Hs,Ws] u8')
        for t, dt in ((image_hwc, torch.uint8), (out, torch.uint8), (workspace, torch.uint8), (sizes, torch.int32), (out_bytes, torch.int32)):
            if t.dtype != dt or not t.is_contiguous():
                raise LamaError(f'png_deflate_u8: a contiguous {dt} tensor is needed, got {t.dtype}')
            if not self.host_emulated and not t.is_cuda:
                raise LamaError('png_deflate_u8: every operand is a device tensor')
        if sizes.numel() < 2 * batch or out_bytes.numel() < batch or out.numel() < batch * int(out_stride):
            raise LamaError('png_deflate_u8: sizes [B,2] / out_bytes [B] int32, out of batch * out_stride bytes')
        c = 1 if image_hwc.dim() == 3 else int(image_hwc.shape[3])
        self.check(self._l.lama_png_deflate_u8_fwd(stream, image_hwc.data_ptr(), sizes.data_ptr(), int(image_hwc.shape[1]), int(image_hwc.shape[2]), c,
                                                   int(batch), int(chunk_bytes), out.data_ptr(), int(out_stride), out_bytes.data_ptr(),
                                                   workspace.data_ptr(), workspace.numel()), 'lama_png_deflate_u8_fwd')

    def jpeg_scan_bound(self, h: int, w: int, subsampling: int = 1) -> int:
        """lama_jpeg_scan_bound: the most bytes the scan of one h x w image can take (0: arguments the encoder refuses).  ``subsampling``:
        JPEG_420 (1) or JPEG_444 (0)."""
        return int(self._l.lama_jpeg_scan_bound(int(h), int(w), int(subsampling)))

    def jpeg_scan_workspace_bytes(self, batch: int, Hs: int, Ws: int, subsampling: int = 1) -> int:
        n = C.c_size_t(0)
        self.check(self._l.lama_jpeg_scan_workspace_bytes(int(batch), int(Hs), int(Ws), int(subsampling), C.byref(n)), 'lama_jpeg_scan_workspace_bytes')
        return int(n.value)

    def jpeg_scan_u8(self, image_hwc: torch.Tensor, sizes: torch.Tensor, out: torch.Tensor, out_stride: int, out_bytes: torch.Tensor,
                     workspace: torch.Tensor, batch: int, quality: int = 95, subsampling: int = 1, stream: int = 0):
        """lama_jpeg_scan_u8_fwd: the entropy-coded scan of a baseline JPEG (integer DCT, Annex K tables, one restart interval per MCU row;
        tests/jpeg_ref.py) of the h x w crop of every u8 slot of ``image_hwc`` [B,Hs,Ws,3], ``sizes`` = device int32 [B,2], into ``out`` (flat u8:
        slot j starts at byte j * ``out_stride``) and its length into ``out_bytes`` (int32 [B]; 0 for an empty slot, -(bytes needed) for a scan
        longer than ``out_stride``).  Three launches, asynchronous, capturable."""
        if image_hwc.dim() != 4 or image_hwc.shape[3] != 3 or image_hwc.shape[0] < batch:
            raise LamaError(f'jpeg_scan_u8: image slots {tuple(image_hwc.shape)}: [B,Hs,Ws,3] u8')
        for t, dt in ((image_hwc, torch.uint8), (out, torch.uint8), (workspace, torch.uint8), (sizes, torch.int32), (out_bytes, torch.int32)):
            if t.dtype != dt or not t.is_contiguous():
                raise LamaError(f'jpeg_scan_u8: a contiguous {dt} tensor is needed, got {t.dtype}')
            if not self.host_emulated and not t.is_cuda:
                raise LamaError('jpeg_scan_u8: every operand is a device tensor')
        if sizes.numel() < 2 * batch or out_bytes.numel() < batch or out.numel() < batch * int(out_stride):
            raise LamaError('jpeg_scan_u8: sizes [B,2] / out_bytes [B] int32, out of batch * out_stride bytes')
        self.check(self._l.lama_jpeg_scan_u8_fwd(stream, image_hwc.data_ptr(), sizes.data_ptr(), int(image_hwc.shape[1]), int(image_hwc.shape[2]),
                                                 int(batch), int(quality), int(subsampling), out.data_ptr(), int(out_stride), out_bytes.data_ptr(),
                                                 workspace.data_ptr(), workspace.numel()), 'lama_jpeg_scan_u8_fwd')

    def eval_ingest_u8(self, image_hwc: torch.Tensor, pred_hwc: torch.Tensor, mask: torch.Tensor, sizes, pad_mod: int,
                       out_image: Optional[torch.Tensor], out_pred: Optional[torch.Tensor], mask_sum: Optional[torch.Tensor], batch: int,
                       clamp=None, stream: int = 0):
        """lama_eval_ingest_u8_fwd: the evaluator's loader on the device.  u8 HWC ground truth / prediction slots [B,Hs,Ws,3] + u8 mask slots
        [B,Hs,Ws], ``sizes`` = a HOST sequence of (h, w) per image or None (every image fills its slot) -> fp32 ``out_image`` / ``out_pred``
        [B,3,Hp,Wp] (/ 255, symmetric padding to ``pad_mod``, ``clamp`` = (lo, hi) on the ground truth only) and ``mask_sum`` int64 [B], the
        exact sum of the padded u8 mask.  Shapes and codes: include/lama_hip.h."""
        if image_hwc.dim() != 4 or image_hwc.shape[3] != 3 or tuple(pred_hwc.shape) != tuple(image_hwc.shape) \
                or tuple(mask.shape) != tuple(image_hwc.shape[:3]) or image_hwc.shape[0] < batch:
            raise LamaError(f'eval_ingest_u8: image / prediction slots {tuple(image_hwc.shape)} / {tuple(pred_hwc.shape)}, mask slots '
                            f'{tuple(mask.shape)}: [B,Hs,Ws,3] / [B,Hs,Ws] u8')
        for t in (image_hwc, pred_hwc, mask):
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise LamaError(f'eval_ingest_u8: contiguous uint8 slots are needed, got {t.dtype}')
        if mask_sum is not None and (mask_sum.dtype != torch.int64 or not mask_sum.is_contiguous() or mask_sum.numel() < batch):
            raise LamaError('eval_ingest_u8: mask_sum is a contiguous int64 [B] tensor')
        for t in (image_hwc, pred_hwc, mask, out_image, out_pred, mask_sum):
            if t is not None and not self.host_emulated and not t.is_cuda:
                raise LamaError('eval_ingest_u8: the slots and the outputs are device tensors (there is no CPU path)')
        for t in (out_image, out_pred):
            if t is not None and t.shape[0] < batch:
                raise LamaError(f'eval_ingest_u8: output {tuple(t.shape)} holds fewer than {batch} images')
        hw = None
        if sizes is not None:
            flat = [int(v) for hw_ in sizes for v in hw_]
            if len(flat) != 2 * batch:
                raise LamaError(f'eval_ingest_u8: sizes holds {len(flat) // 2} (h, w) pairs for a batch of {batch}')
            hw = (C.c_int32 * len(flat))(*flat)
        lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
        self.check(self._l.lama_eval_ingest_u8_fwd(stream, image_hwc.data_ptr(), pred_hwc.data_ptr(), mask.data_ptr(), hw, int(image_hwc.shape[1]),
                                                   int(image_hwc.shape[2]), int(pad_mod), int(clamp is not None), lo, hi,
                                                   None if out_image is None else C.byref(view(out_image)),
                                                   None if out_pred is None else C.byref(view(out_pred)),
                                                   None if mask_sum is None else mask_sum.data_ptr(), batch), 'lama_eval_ingest_u8_fwd')

    def quantize_u8_hwc(self, src: Tensor4, dst: torch.Tensor, batch: int, crop_h: int, crop_w: int, stream: int = 0):
        self.check(self._l.lama_quantize_u8_hwc_fwd(stream, C.byref(src), dst.data_ptr(), batch, crop_h, crop_w), 'lama_quantize_u8_hwc_fwd')


    def affine_act(self, x: Tensor4, scale, shift, act: int, y: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_affine_act_fwd(stream, C.byref(x), None if scale is None else scale.data_ptr(),
                                               None if shift is None else shift.data_ptr(), act, C.byref(y), batch), 'lama_affine_act_fwd')

    def reflect_pad(self, x: Tensor4, pad: int, y: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_reflect_pad_fwd(stream, C.byref(x), pad, C.byref(y), batch), 'lama_reflect_pad_fwd')


    # -- refinement (include/lama_hip.h, last section) --------------------------------------------
    def act_bwd(self, g: Tensor4, y: Tensor4, act: int, gout: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_act_bwd(stream, C.byref(g), C.byref(y), act, C.byref(gout), batch), 'lama_act_bwd')

    def add(self, a: Tensor4, b: Tensor4, out: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_add_fwd(stream, C.byref(a), C.byref(b), C.byref(out), batch), 'lama_add_fwd')

    def reflect_pad_bwd_fused(self, gp: Tensor4, add1: Optional[Tensor4], add2: Optional[Tensor4], pad: int, mask_y: Optional[Tensor4], act: int,
                              g: Optional[Tensor4], gm: Optional[Tensor4], batch: int, stream: int = 0, ring: Optional[torch.Tensor] = None):
        """s = fold(gp) [+ add1] [+ add2]; g = s; gm = s * act'(mask_y) -- one pass (include/lama_hip.h, v108).  With ``ring`` (dgrad_ring), gp
        is the interior [B,C,H,W] of the padded plane."""
        r = lambda t: None if t is None else C.byref(t)    # noqa: E731
        self.check(self._l.lama_reflect_pad_bwd_fused(stream, C.byref(gp), r(add1), r(add2), pad, r(mask_y), act, r(g), r(gm), batch,
                                                      None if ring is None else ring.data_ptr()), 'lama_reflect_pad_bwd_fused')

    def dgrad_ring_bytes(self, b: int, cout: int, h: int, w: int) -> int:
        return int(self._l.lama_dgrad_ring_bytes(b, cout, h, w))

    @staticmethod
    def dgrad_ring_weight(w_dgrad: torch.Tensor) -> torch.Tensor:
        """w' [cout, cin, 3, 3] (the flipped, transposed weights of a 3x3 dgrad conv) -> [4][cin][3][cout] fp32 (include/lama_hip.h)."""
        wt = w_dgrad.detach().float().permute(1, 2, 3, 0)            # [cin][ky][kx][cout]
        return torch.stack([wt[:, 2], wt[:, 0], wt[:, :, 2], wt[:, :, 0]], 0).contiguous()

    def dgrad_ring(self, g: Tensor4, w_ring: torch.Tensor, cout: int, ring: torch.Tensor, batch: int, stream: int = 0):
        if ring.numel() * 4 < self.dgrad_ring_bytes(batch, cout, g.H, g.W) or tuple(w_ring.shape) != (4, g.C, 3, cout):
            raise LamaError('dgrad_ring: ring / weight buffer does not match the launch', ERR_BAD_ARG)
        self.check(self._l.lama_dgrad_ring_fwd(stream, C.byref(g), w_ring.data_ptr(), cout, ring.data_ptr(), batch), 'lama_dgrad_ring_fwd')

    def reflect_pad_bwd(self, gp: Tensor4, addend: Optional[Tensor4], pad: int, g: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_reflect_pad_bwd(stream, C.byref(gp), None if addend is None else C.byref(addend), pad, C.byref(g), batch),
                   'lama_reflect_pad_bwd')

    def ssim(self, img1: Tensor4, img2: Tensor4, batch: int, window1d, out: torch.Tensor, workspace: torch.Tensor, stream: int = 0):
        """Per-image SSIM (ssim.py:46-71, size_average=False) into out [batch] fp32; window1d = host sequence of the odd-length
        normalised 1-D gaussian; workspace = device buffer of at least ssim_workspace_bytes() bytes."""
        if not self.host_emulated and not (out.is_cuda and workspace.is_cuda):
            raise LamaError('ssim: out / workspace must be device tensors')
        w = (C.c_float * len(window1d))(*[float(v) for v in window1d])
        self.check(self._l.lama_ssim_fwd(stream, C.byref(img1), C.byref(img2), batch, len(window1d), w, out.data_ptr(), workspace.data_ptr(),
                                         workspace.numel() * workspace.element_size()), 'lama_ssim_fwd')

    def ssim_workspace_bytes(self, batch: int, c: int, h: int, w: int) -> int:
        return int(self._l.lama_ssim_workspace_bytes(batch, c, h, w))

    def lpips_scale(self, x0: Tensor4, x1: Tensor4, y: Tensor4, batch: int, shift, scale, normalize: bool = True, stream: int = 0):
        """lama_lpips_scale_fwd: ((2 x - 1) - shift) / scale of x0 | x1 ([batch,3,H,W] each) into the two halves of y [2 batch,3,H,W];
        shift / scale = host sequences of 3 floats."""
        sh, sc = (C.c_float * 3)(*[float(v) for v in shift]), (C.c_float * 3)(*[float(v) for v in scale])
        self.check(self._l.lama_lpips_scale_fwd(stream, C.byref(x0), C.byref(x1), C.byref(y), batch, int(bool(normalize)), sh, sc), 'lama_lpips_scale_fwd')

    def lpips_layer(self, f0: Tensor4, f1: Tensor4, batch: int, w: torch.Tensor, acc: torch.Tensor, workspace: torch.Tensor,
                    pool0: Optional[Tensor4] = None, pool1: Optional[Tensor4] = None, stream: int = 0):
        """lama_lpips_layer_fwd: acc[b] += the level's LPIPS term of (f0[b], f1[b]) under the head ``w`` [C]; pool0 / pool1 receive max_pool2d(f, 2, 2)
        from the same launch.  ``workspace``: device buffer of at least lpips_layer_workspace_bytes() bytes."""
        for name, t in (('w', w), ('acc', acc), ('workspace', workspace)):
            if not self.host_emulated and not t.is_cuda:
                raise LamaError(f'lpips_layer: {name} must be a device tensor')
        if w.dtype != torch.float32 or acc.dtype != torch.float32 or not w.is_contiguous() or not acc.is_contiguous() or w.numel() != f0.C or acc.numel() < batch:
            raise LamaError(f'lpips_layer: w is [C] fp32 and acc [batch] fp32, got {tuple(w.shape)} {w.dtype} / {tuple(acc.shape)} {acc.dtype}')
        self.check(self._l.lama_lpips_layer_fwd(stream, C.byref(f0), C.byref(f1), batch, w.data_ptr(), acc.data_ptr(),
                                                None if pool0 is None else C.byref(pool0), None if pool1 is None else C.byref(pool1),
                                                workspace.data_ptr(), workspace.numel() * workspace.element_size()), 'lama_lpips_layer_fwd')

    def lpips_layer_workspace_bytes(self, batch: int, c: int, h: int, w: int) -> int:
        return int(self._l.lama_lpips_layer_workspace_bytes(batch, c, h, w))

    # -- FID: Inception-v3 (new symbols in v112) ----------------------------------------------------------------
    def pack_conv_rect_weight(self, w: torch.Tensor, scale: Optional[torch.Tensor], precision: int = PREC_F16X3) -> torch.Tensor:
        """Conv2d weight [cout, cin, kh, kw] (+ folded BatchNorm scale) -> the packed device buffer of lama_conv2d_rect_fwd."""
        if not self.host_emulated and not w.is_cuda:
            raise LamaError('pack_conv_rect_weight: the weights are on the CPU: move the module to the GPU first')
        w = w.contiguous().float()
        if scale is not None and scale.device != w.device:
            raise LamaError(f'pack_conv_rect_weight: weight on {w.device} but BatchNorm scale on {scale.device}')
        cout, cin, kh, kw = w.shape
        nbytes = self._l.lama_conv2d_rect_packed_weight_bytes(cout, cin, kh, kw, precision)
        if nbytes <= 0:
            raise LamaError(f'unsupported rect conv geometry {tuple(w.shape)} / precision {precision}', code=ERR_UNSUPPORTED)
        if precision == PREC_F16X3 and w.numel():
            ws = w if scale is None else w * scale.float().view(-1, 1, 1, 1)
            amax = float(ws.abs().max())
            if not amax <= F16_MAX:
                raise LamaRangeError(f'folded conv weight |w| max {amax:.3g} exceeds the fp16 split range ({F16_MAX}); use bf16x3')
        dst = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        sc = None if scale is None else scale.contiguous().float()
        self.check(self._l.lama_conv2d_rect_pack_weight(self.stream_of(w), w.data_ptr(), None if sc is None else sc.data_ptr(), cout, cin, kh, kw,
                                                        precision, dst.data_ptr()), 'lama_conv2d_rect_pack_weight')
        if w.is_cuda:
            torch.cuda.current_stream(w.device).synchronize()  # w / sc may be temporaries
        return dst

    def conv2d_rect(self, x: Tensor4, w_packed: torch.Tensor, y: Tensor4, batch: int, kh: int, kw: int, stride: int = 1, pad_h: int = 0,
                    pad_w: int = 0, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, precision: int = PREC_F16X3, stream: int = 0,
                    range_flag: Optional[torch.Tensor] = None):
        """lama_conv2d_rect_fwd: zero-padded kh x kw convolution with per-axis padding; x / y may be channel-slice views."""
        a = Conv2dRectArgs()
        a.x, a.w_packed, a.y = x, w_packed.data_ptr(), y
        a.bias = None if bias is None else bias.data_ptr()
        a.act, a.batch, a.kh, a.kw, a.stride, a.pad_h, a.pad_w, a.precision = act, batch, kh, kw, stride, pad_h, pad_w, precision
        a.range_flag = None if range_flag is None else range_flag.data_ptr()
        self.check(self._l.lama_conv2d_rect_fwd(stream, C.byref(a)), 'lama_conv2d_rect_fwd')

    def pool3x3(self, x: Tensor4, y: Tensor4, batch: int, mode: int, stride: int, pad: int, stream: int = 0):
        """lama_pool3x3_fwd: POOL_MAX or POOL_AVG_EXCLUDE_PAD (count_include_pad=False) over a 3x3 window."""
        self.check(self._l.lama_pool3x3_fwd(stream, C.byref(x), C.byref(y), batch, mode, stride, pad), 'lama_pool3x3_fwd')

    def global_avgpool(self, x: Tensor4, y: torch.Tensor, batch: int, stream: int = 0):
        """lama_global_avgpool_fwd: [batch, C, h, w] -> y [batch, C] fp32 (fp64 sum, rounded once)."""
        if y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != batch * x.C or (not self.host_emulated and not y.is_cuda):
            raise LamaError(f'global_avgpool: y is a contiguous device [batch, C] fp32 tensor, got {tuple(y.shape)} {y.dtype}')
        self.check(self._l.lama_global_avgpool_fwd(stream, C.byref(x), y.data_ptr(), batch), 'lama_global_avgpool_fwd')

    def fid_input(self, pred: Tensor4, target: Tensor4, y: Tensor4, batch: int, resize: bool = True, stream: int = 0):
        """lama_fid_input_fwd: bilinear resize of pred | target to y's plane (resize) and 2 x - 1, into one [2 batch, 3, ., .] tensor."""
        self.check(self._l.lama_fid_input_fwd(stream, C.byref(pred), C.byref(target), C.byref(y), batch, int(bool(resize))), 'lama_fid_input_fwd')

    def gauss5(self, x: Tensor4, y: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_gauss5_fwd(stream, C.byref(x), C.byref(y), batch), 'lama_gauss5_fwd')

    def gauss5_bwd(self, gy: Tensor4, gx: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_gauss5_bwd(stream, C.byref(gy), C.byref(gx), batch), 'lama_gauss5_bwd')

    def bilinear(self, x: Tensor4, y: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_bilinear_fwd(stream, C.byref(x), C.byref(y), batch), 'lama_bilinear_fwd')

    def bilinear_bwd(self, gy: Tensor4, gx: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_bilinear_bwd(stream, C.byref(gy), C.byref(gx), batch), 'lama_bilinear_bwd')

    def threshold(self, x: Tensor4, thr: float, y: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_threshold_fwd(stream, C.byref(x), thr, C.byref(y), batch), 'lama_threshold_fwd')

    def erode(self, x: Tensor4, se: torch.Tensor, y: Tensor4, batch: int, max_val: float = 1e4, stream: int = 0):
        kh, kw = se.shape
        self.check(self._l.lama_erode_fwd(stream, C.byref(x), se.data_ptr(), kh, kw, max_val, C.byref(y), batch), 'lama_erode_fwd')

    def l1_masked(self, pred: Tensor4, target: Tensor4, mask: Tensor4, thr: float, select_ge: bool, accum: torch.Tensor, batch: int,
                  stream: int = 0):
        assert accum.dtype == torch.float64 and accum.numel() >= 2
        self.check(self._l.lama_l1_masked_fwd(stream, C.byref(pred), C.byref(target), C.byref(mask), thr, int(select_ge), accum.data_ptr(),
                                              batch), 'lama_l1_masked_fwd')

    def l1_masked_bwd(self, pred: Tensor4, target: Tensor4, mask: Tensor4, thr: float, select_ge: bool, scale: float, accumulate: bool,
                      g: Tensor4, batch: int, stream: int = 0):
        self.check(self._l.lama_l1_masked_bwd(stream, C.byref(pred), C.byref(target), C.byref(mask), thr, int(select_ge), scale,
                                              int(accumulate), C.byref(g), batch), 'lama_l1_masked_bwd')

    def l1_masked_per_image(self, pred: Tensor4, target: Tensor4, mask: Tensor4, thr: float, select_ge: bool, accum: torch.Tensor, batch: int,
                            stream: int = 0):
        """(v111) accum [batch, 2] float64 (zeroed by the caller) += per-image (sum |pred - target|, count)."""
        assert accum.dtype == torch.float64 and accum.is_contiguous() and accum.numel() >= 2 * batch
        self.check(self._l.lama_l1_masked_per_image_fwd(stream, C.byref(pred), C.byref(target), C.byref(mask), thr, int(select_ge),
                                                        accum.data_ptr(), batch), 'lama_l1_masked_per_image_fwd')

    def l1_masked_per_image_bwd(self, pred: Tensor4, target: Tensor4, mask: Tensor4, thr: float, select_ge: bool, accum: torch.Tensor,
                                accumulate: bool, g: Tensor4, batch: int, stream: int = 0):
        """(v111) g (+)= sign(pred - target) / n_b per image, n_b = accum[b, 1] as l1_masked_per_image left it."""
        assert accum.dtype == torch.float64 and accum.is_contiguous() and accum.numel() >= 2 * batch
        self.check(self._l.lama_l1_masked_per_image_bwd(stream, C.byref(pred), C.byref(target), C.byref(mask), thr, int(select_ge),
                                                        accum.data_ptr(), int(accumulate), C.byref(g), batch), 'lama_l1_masked_per_image_bwd')

    def adam_step(self, param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr: float, step: int,
                  beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, stream: int = 0):
        n = param.numel()
        for t_ in (param, grad, exp_avg, exp_avg_sq):
            if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() != n:
                raise LamaError('adam_step: contiguous fp32 tensors of one size expected')
        self.check(self._l.lama_adam_step(stream, param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n, lr,
                                          beta1, beta2, eps, step), 'lama_adam_step')


def unpack_range_stats(stats: torch.Tensor):
    """Host view of a ``LamaLib.range_stats`` result (int32 [..., 4], any device): (abs_max float32 [...], n_nan, n_inf, n_over uint32 [...])
    as numpy arrays.  One D2H copy when the tensor is on the device."""
    import numpy as np
    a = np.ascontiguousarray(stats.detach().cpu().numpy()).reshape(-1, 4)
    lead = tuple(stats.shape[:-1]) if stats.dim() > 1 else (a.shape[0],)
    u = a.view(np.uint32)
    return (a[:, 0].copy().view(np.float32).reshape(lead), u[:, 1].copy().reshape(lead), u[:, 2].copy().reshape(lead), u[:, 3].copy().reshape(lead))


_LIB: Optional[LamaLib] = None


def get_lib() -> LamaLib:
    """The process-wide HIP library (loaded on first use; raises LamaError if it was not built)."""
    global _LIB
    if _LIB is None:
        _LIB = LamaLib()
    return _LIB


def use_library(path: str) -> LamaLib:
    """Measurement tools only (tools/, bench.py --lib): make another build of the same ABI -- the profiling build, an A/B base -- the
    process-wide library.  Must be called before anything loaded the default one; the product never calls it and no environment variable
    selects a library."""
    global _LIB
    if _LIB is not None and os.path.abspath(_LIB.path) != os.path.abspath(path):
        raise LamaError(f'use_library({path}): {_LIB.path} is already loaded')
    if _LIB is None:
        _LIB = LamaLib(path)
    return _LIB
