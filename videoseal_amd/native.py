"""ctypes binding of libvideoseal_hip.so (the C-ABI declared in include/videoseal_hip.h).

This is the stub a maintainer of the reference would add to call the MI355X kernels
(INTEGRATION.md).  There is NO fallback: if the shared library is missing or an entry
point fails, the call raises -- the product path never silently runs on ATen / CPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional

import torch

from . import switches as SW

_HERE = os.path.dirname(os.path.abspath(__file__))
# VIDEOSEAL_LIB: another build of the same ABI (same-box A/B of two source trees, tools/ab_libs.sh); the default is the in-tree library
LIB_PATH = SW.path("VIDEOSEAL_LIB") or os.path.join(_HERE, "csrc", "libvideoseal_hip.so")

ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH, ACT_SILU = 0, 1, 2, 3, 4
PAD_ZERO, PAD_REFLECT = 0, 1
CONV_FORCE_F32, CONV_FORCE_SPLIT, CONV_TILE_HI, CONV_PRE = 0x10, 0x20, 0x40, 0x80
VIDEO_MODES = {"repeat": 0, "alternate": 1, "interpolate": 2}

EXPORTS = [
    "vs_version", "vs_arch", "vs_error_string", "vs_sizeof_conv_desc", "vs_sizeof_tail_desc", "vs_debug_set", "vs_debug_key", "vs_debug_get",
    "vs_model_create", "vs_model_destroy", "vs_model_workspace_bytes", "vs_model_embed", "vs_model_detect", "vs_model_set_nv12_color", "vs_nv12_default_color", "vs_conv_gemm", "vs_conv_plan", "vs_cnx_stage_plan", "vs_sizeof_conv_plan", "vs_sizeof_cnx_stage_plan", "vs_to_planes", "vs_to_planes_affine", "vs_layernorm_act", "vs_layernorm_patch2x2", "vs_stem_conv_ln", "vs_rmsnorm_act", "vs_vit_attention", "vs_dwconv7_ln", "vs_dwconv7_ln_planes", "vs_grn_scale", "vs_grn_scale_from_partials", "vs_grn_scale_from_straddle_partials", "vs_grn_apply",
    "vs_upcat2x", "vs_upconv_supported", "vs_upconv_gather_ln", "vs_cat2_scale", "vs_msg_pre", "vs_msg_pre_rows", "vs_upconv_fused_supported", "vs_upconv_fused_preferred", "vs_upconv_fused", "vs_im2col3x3", "vs_msg_latent", "vs_broadcast_channels", "vs_outc_tanh", "vs_pool_linear", "vs_resize_pre", "vs_resize_pre_u8",
    "vs_jnd_heatmap", "vs_embed_tail", "vs_aug_color_scratch_floats", "vs_aug_color", "vs_aug_color_chain", "vs_aug_crop_resize_color", "vs_aug_crop_flip", "vs_aug_warp", "vs_resize_nchw",
    "vs_gaussian_blur", "vs_median_filter", "vs_jpeg_workspace_bytes", "vs_jpeg_roundtrip", "vs_h264_proxy_workspace_bytes", "vs_h264_proxy_roundtrip",
    "vs_bn_partial_doubles", "vs_bn_batch_stats", "vs_bn_partial_sums", "vs_bn_finish_sums", "vs_scale_shift_act", "vs_aug_mask_blend", "vs_aug_add_scaled", "vs_aug_gather_frames", "vs_aug_window_average",
    "vs_gemm_wgrad_partial_floats", "vs_gemm_wgrad", "vs_conv3x3_wgrad", "vs_conv3x3_wgrad_supported", "vs_conv3x3_wgrad_partial_floats", "vs_pad_embed1", "vs_reflect_fold1", "vs_pack_conv", "vs_gaussian_blur_bwd", "vs_aug_warp_bwd", "vs_aug_gather_frames_bwd", "vs_aug_window_average_bwd", "vs_gelu_bwd", "vs_act_bwd", "vs_rmsnorm_act_bwd", "vs_vit_attention_bwd_scratch_floats", "vs_vit_attention_bwd", "vs_dwconv7", "vs_dwconv7_wgrad_partial_floats", "vs_dwconv7_wgrad", "vs_colreduce_partial_floats",
    "vs_layernorm_bwd", "vs_gelu_grn_bwd", "vs_patchify", "vs_unpatch", "vs_patchify_s", "vs_unpatch_s", "vs_col2im3x3_reflect", "vs_colmean", "vs_pool_gelu_bwd", "vs_matmul_small",
    "vs_bce_logits",
    "vs_bn_mean_rstd", "vs_bn_bwd_partial_floats", "vs_bn_relu_bwd_sums", "vs_bn_relu_bwd_apply", "vs_dilate2", "vs_im2col3x3_strided", "vs_upcat2x_bwd",
    "vs_msg_table_grad", "vs_outc_tanh_bwd", "vs_relu_bwd",
    "vs_resize_nchw_bwd", "vs_embed_tail_bwd", "vs_tail_key_reduce", "vs_aug_crop_flip_bwd", "vs_mask_mul", "vs_aug_color_bwd_scratch_floats",
    "vs_aug_color_bwd", "vs_clamp01_bwd", "vs_nhwc_to_nchw_scaled", "vs_percep_partial_doubles", "vs_percep_mse", "vs_percep_mse_grad",
    "vs_ssim_partial_doubles", "vs_ssim_stats", "vs_ssim_grad", "vs_avgpool2_pad", "vs_jnd_loss_partial_doubles", "vs_jnd_loss", "vs_jnd_loss_grad",
    "vs_split_block", "vs_check_finite", "vs_absmax", "vs_resblock_thin", "vs_resblock_thin_supported", "vs_cnx_block_supported", "vs_cnx_block_image_bytes", "vs_cnx_block",
    "vs_pixel_upgather_supported", "vs_pixel_upgather", "vs_pixel_upgather_bwd", "vs_pixel_linear", "vs_pixel_linear_bwd_partial_floats", "vs_pixel_linear_bwd",
    "vs_pixel_bce_partial_doubles", "vs_pixel_bce", "vs_pixel_vote",
    "vs_disc_input", "vs_disc_input_bwd", "vs_groupnorm_partial_doubles", "vs_groupnorm_lrelu", "vs_groupnorm_lrelu_bwd", "vs_conv4x4_wgrad_supported",
    "vs_conv4x4_wgrad_partial_floats", "vs_conv4x4_wgrad", "vs_conv4x4_n1", "vs_conv4x4_n1_bwd", "vs_conv4x4_n1_bias_grad", "vs_disc_loss",
    "vs_sizeof_tail_nv12_desc", "vs_resize_pre_nv12", "vs_embed_tail_nv12",
    "vs_sizeof_yuv420_surface", "vs_sizeof_tail_yuv420_desc", "vs_resize_pre_yuv420", "vs_embed_tail_yuv420", "vs_yuv420_default_color",
    "vs_model_embed_yuv420", "vs_model_detect_yuv420",
    "vs_sizeof_yuv_surface", "vs_sizeof_tail_yuv_desc", "vs_resize_pre_yuv", "vs_embed_tail_yuv", "vs_model_embed_yuv", "vs_model_detect_yuv",
    "vs_sizeof_rgb_surface", "vs_sizeof_tail_rgb_desc", "vs_resize_pre_rgb", "vs_embed_tail_rgb", "vs_model_embed_rgb", "vs_model_detect_rgb",
    "vs_resize_pre_images", "vs_embed_tail_images", "vs_images_plan",
    "vs_resize_pre_clips", "vs_embed_tail_clips", "vs_clips_plan", "vs_aggregate_clips",
    "vs_tail_energy_partial_doubles", "vs_embed_tail_energy", "vs_psnr_scale", "vs_embed_tail_scaled",
    "vs_model_embed_psnr", "vs_model_embed_psnr_workspace_bytes",
]

# the entry points of include/videoseal_regions.h (a header of its own: tests/test_host.py holds EXPORTS to what videoseal_hip.h declares)
REGION_EXPORTS = ["vs_embed_tail_regions", "vs_pixel_vote_regions_partial_doubles", "vs_pixel_vote_regions", "vs_label_boxes"]
REGIONS_MAX = 8                                              # VS_REGIONS_MAX
# the entry points of include/videoseal_lists_psnr.h (target PSNR on the image and clip lists; a header of its own for the same reason)
LIST_PSNR_EXPORTS = ["vs_tail_images_energy_partial_doubles", "vs_embed_tail_images_energy", "vs_embed_tail_images_scaled",
                     "vs_tail_clips_energy_partial_doubles", "vs_embed_tail_clips_energy", "vs_embed_tail_clips_scaled", "vs_psnr_scale_items"]
# the entry points of include/videoseal_half.h (float16 / bfloat16 surfaces; a header of its own for the same reason)
HALF_EXPORTS = ["vs_sizeof_half_surface", "vs_sizeof_tail_half_desc", "vs_resize_pre_half", "vs_embed_tail_half", "vs_model_embed_half",
                "vs_model_detect_half"]
# the entry points of include/videoseal_yuv_clips.h (lists of YUV clips; a header of its own for the same reason)
YUV_CLIPS_EXPORTS = ["vs_sizeof_yuv_clip_desc", "vs_sizeof_tail_yuv_clips_desc", "vs_sizeof_yuv_clips_group", "vs_resize_pre_yuv_clips",
                     "vs_embed_tail_yuv_clips", "vs_yuv_clips_plan"]
YUV_CLIPS_PER_LAUNCH = 16                                    # VS_YUV_CLIPS_PER_LAUNCH


class NativeError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """mirror of vs_conv_desc_t"""
    _fields_ = [
        ("inp", C.c_void_p), ("in_sb", C.c_int64), ("in_sy", C.c_int64), ("in_sx", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("SH", C.c_int32), ("SW", C.c_int32), ("PH", C.c_int32), ("PW", C.c_int32),
        ("pad_mode", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("wt", C.c_void_p), ("CinP", C.c_int32), ("N", C.c_int32),
        ("a_scale", C.c_void_p), ("a_scale_ld", C.c_int64), ("a_shift", C.c_void_p),
        ("bias", C.c_void_p), ("act", C.c_int32), ("n_store", C.c_int32),
        ("res", C.c_void_p), ("res_ld", C.c_int64),
        ("in2", C.c_void_p), ("in2_ld", C.c_int64), ("Cin2", C.c_int32), ("Cin2P", C.c_int32),
        ("wt2", C.c_void_p), ("bias2", C.c_void_p),
        ("out", C.c_void_p), ("out_ld", C.c_int64), ("out_coff", C.c_int32), ("tile_hint", C.c_int32),
        ("wt_split", C.c_void_p), ("wt2_split", C.c_void_p), ("wt_blk", C.c_void_p), ("wt2_blk", C.c_void_p),
        ("splitk_ws", C.c_void_p), ("splitk_ld", C.c_int64), ("split_k", C.c_int32), ("arith", C.c_int32),
        ("sumsq_part", C.c_void_p), ("in_pl", C.c_void_p), ("in2_pl", C.c_void_p), ("out_pl", C.c_void_p), ("a_mul", C.c_float), ("acc_mul", C.c_float), ("acc_mul2", C.c_float), ("grn_nchunk", C.c_int32), ("grn_part", C.c_void_p), ("grn_gamma", C.c_void_p), ("sumsq_hw", C.c_int32), ("reserved_", C.c_int32),
        ("bias_fs", C.c_int64), ("bias2_fs", C.c_int64),
    ]


class ConvPlan(C.Structure):
    """mirror of vs_conv_plan_t"""
    _fields_ = [(n, C.c_int32) for n in ("routes", "split_k", "tile_hint", "ws_slices", "grn_fold")]


class CnxStagePlan(C.Structure):
    """mirror of vs_cnx_stage_plan_t"""
    _fields_ = [(n, C.c_int32) for n in ("pl1", "pl2", "sk2", "tile1", "tile2", "pw2_narrow")]


# VS_ROUTE_* bits of ConvPlan.routes, VS_CNX_* flags of vs_cnx_stage_plan
ROUTE_GEMM_PC, ROUTE_PATCH, ROUTE_PATCH_PC, ROUTE_SMALL = 1, 2, 4, 8
CNX_NO_PLANES_GEMM, CNX_NO_PW2_SMALL_PC, CNX_NO_PW2_NARROW, CNX_GEMM_BIG, CNX_NO_SPLIT = 1, 2, 4, 8, 16


class TailDesc(C.Structure):
    """mirror of vs_tail_desc_t"""
    _fields_ = [
        ("imgs", C.c_void_p), ("out", C.c_void_p), ("preds_w", C.c_void_p),
        ("delta", C.c_void_p), ("hmap_lowres", C.c_void_p), ("taps43", C.c_void_p),
        ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("S_h", C.c_int32), ("S_w", C.c_int32), ("Cd", C.c_int32),
        ("step", C.c_int32), ("video_mode", C.c_int32), ("total_key", C.c_int32),
        ("attenuate", C.c_int32), ("clamp", C.c_int32), ("antialias", C.c_int32),
        ("scaling_i", C.c_float), ("scaling_w", C.c_float), ("io_u8", C.c_int32), ("variant", C.c_int32),
    ]


class TailNv12Desc(C.Structure):
    """mirror of vs_tail_nv12_desc_t: TailDesc's members, pitches / frame strides in bytes and the two colour affines"""
    _fields_ = TailDesc._fields_ + [
        ("src_pitch", C.c_int64), ("src_frame_stride", C.c_int64), ("dst_pitch", C.c_int64), ("dst_frame_stride", C.c_int64),
        ("yuv2rgb12", C.c_float * 12), ("rgb2yuv12", C.c_float * 12),
    ]


class Yuv420Surface(C.Structure):
    """mirror of vs_yuv420_surface_t: plane addresses, row pitches and frame strides in bytes, the format triple"""
    _fields_ = [
        ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3), ("frame_stride", C.c_int64 * 3),
        ("planar", C.c_int32), ("depth", C.c_int32), ("msb_aligned", C.c_int32), ("reserved_", C.c_int32),
    ]


class TailYuv420Desc(C.Structure):
    """mirror of vs_tail_yuv420_desc_t: two surfaces, then TailDesc's members from preds_w on and the two colour affines"""
    _fields_ = [("src", Yuv420Surface), ("dst", Yuv420Surface)] + TailDesc._fields_[2:] + [
        ("yuv2rgb12", C.c_float * 12), ("rgb2yuv12", C.c_float * 12),
    ]


def _fill_surface(s, planes, planar: bool, depth: int, msb: bool):
    """plane addresses, row pitches and frame strides in bytes and the format triple of device-resident planes: nothing is copied"""
    for i, p in enumerate(planes):
        s.plane[i] = ptr(p)
        s.pitch[i] = p.stride(1) * p.element_size()
        s.frame_stride[i] = p.stride(0) * p.element_size()
    s.planar, s.depth, s.msb_aligned = int(planar), depth, int(msb)
    return s


def yuv420_surface(planes, fmt: str) -> Yuv420Surface:
    """the surface of device-resident planes of a 4:2:0 format (videoseal_amd/yuv420.py), for the _yuv420 entry points"""
    from .yuv420 import fmt_info
    return _fill_surface(Yuv420Surface(), planes, *fmt_info(fmt))


class YuvSurface(C.Structure):
    """mirror of vs_yuv_surface_t: Yuv420Surface with the chroma format (420, 422, 444) as its last member"""
    _fields_ = Yuv420Surface._fields_[:-1] + [("chroma", C.c_int32)]


class TailYuvDesc(C.Structure):
    """mirror of vs_tail_yuv_desc_t: TailYuv420Desc on two YuvSurface"""
    _fields_ = [("src", YuvSurface), ("dst", YuvSurface)] + TailYuv420Desc._fields_[2:]


def yuv_surface(planes, fmt: str) -> YuvSurface:
    """the surface of device-resident planes of any of the ten formats (videoseal_amd/yuv.py)"""
    from .yuv import fmt_info
    planar, depth, msb, chroma = fmt_info(fmt)
    s = _fill_surface(YuvSurface(), planes, planar, depth, msb)
    s.chroma = chroma
    return s


class RgbSurface(C.Structure):
    """mirror of vs_rgb_surface_t: the first byte, row pitch and frame stride in bytes, the format (VS_RGB_*)"""
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_int64), ("frame_stride", C.c_int64), ("format", C.c_int32), ("reserved_", C.c_int32)]


class TailRgbDesc(C.Structure):
    """mirror of vs_tail_rgb_desc_t: two surfaces, then TailDesc's members from preds_w on"""
    _fields_ = [("src", RgbSurface), ("dst", RgbSurface)] + TailDesc._fields_[2:]


def rgb_surface(clip, fmt: str) -> RgbSurface:
    """the surface of a device-resident packed RGB clip (videoseal_amd/rgbpack.py): a strided view stays one, nothing is copied"""
    from .rgbpack import fmt_info
    s = RgbSurface()
    s.data = ptr(clip)
    s.pitch = clip.stride(1) * clip.element_size()
    s.frame_stride = clip.stride(0) * clip.element_size()
    s.format = fmt_info(fmt)[0]
    return s


class HalfSurface(C.Structure):
    """mirror of vs_half_surface_t: plane addresses (packed: one), row pitches and frame strides in bytes, element type, layout, components,
    value range (VS_HALF_*)"""
    _fields_ = [
        ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3), ("frame_stride", C.c_int64 * 3),
        ("elem", C.c_int32), ("layout", C.c_int32), ("components", C.c_int32), ("value_range", C.c_int32),
    ]


class TailHalfDesc(C.Structure):
    """mirror of vs_tail_half_desc_t: two surfaces, then TailDesc's members from preds_w on"""
    _fields_ = [("src", HalfSurface), ("dst", HalfSurface)] + TailDesc._fields_[2:]


def half_surface(clip, layout: str, value_range: str) -> HalfSurface:
    """the surface of a device-resident half clip (videoseal_amd/halfpix.py) in either memory form: a strided view stays one, nothing is copied"""
    from . import halfpix
    s = HalfSurface()
    form, comps = halfpix.memory_form(clip, layout)
    s.elem, s.layout, s.components, s.value_range = halfpix.DTYPES[clip.dtype], form, comps, halfpix.RANGES[value_range]
    es = clip.element_size()
    if form == halfpix.PLANAR:
        for i in range(3):
            s.plane[i] = ptr(clip) + i * clip.stride(1) * es
            s.pitch[i] = clip.stride(2) * es
            s.frame_stride[i] = clip.stride(0) * es
    else:
        s.plane[0] = ptr(clip)
        s.pitch[0] = clip.stride(1 if layout == "nhwc" else 2) * es
        s.frame_stride[0] = clip.stride(0) * es
    return s


IMAGES_PER_LAUNCH = 32                                       # VS_IMAGES_PER_LAUNCH
IMAGES_RESIZE, IMAGES_TAIL = 0, 1                            # VS_IMAGES_RESIZE / VS_IMAGES_TAIL: the pass a plan is for
IMAGES_FORM_TILE, IMAGES_FORM_STREAM128, IMAGES_FORM_STREAM64 = 0, 1, 2


class ImageDesc(C.Structure):
    """mirror of vs_image_desc_t: one image of a list, its own base pointer(s) and size"""
    _fields_ = [("img", C.c_void_p), ("out", C.c_void_p), ("preds_w", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32)]


class TailImagesDesc(C.Structure):
    """mirror of vs_tail_images_desc_t: the tail parameters every image shares and the list"""
    _fields_ = [
        ("images", C.POINTER(ImageDesc)), ("delta", C.c_void_p), ("hmap_lowres", C.c_void_p), ("taps43", C.c_void_p),
        ("n", C.c_int32), ("S_h", C.c_int32), ("S_w", C.c_int32), ("Cd", C.c_int32),
        ("attenuate", C.c_int32), ("clamp", C.c_int32), ("antialias", C.c_int32), ("io_u8", C.c_int32),
        ("scaling_i", C.c_float), ("scaling_w", C.c_float),
    ]


class ImagesGroup(C.Structure):
    """mirror of vs_images_group_t: one launch of the plan"""
    _fields_ = [("form", C.c_int32), ("count", C.c_int32), ("strip", C.c_int32), ("reserved_", C.c_int32),
                ("image", C.c_int32 * IMAGES_PER_LAUNCH), ("first_wg", C.c_int32 * (IMAGES_PER_LAUNCH + 1))]


def image_descs(imgs, outs=None, preds_w=None):
    """the HOST descriptor array of a list of device images (fp32 [3, H, W] or uint8 [H, W, 3], contiguous): addresses and sizes, nothing is copied"""
    arr = (ImageDesc * max(1, len(imgs)))()
    for i, t in enumerate(imgs):
        H, W = (t.shape[0], t.shape[1]) if t.dtype == torch.uint8 else (t.shape[-2], t.shape[-1])
        arr[i].img, arr[i].H, arr[i].W = ptr(t), H, W
        arr[i].out = ptr(outs[i]) if outs is not None else None
        arr[i].preds_w = ptr(preds_w[i]) if preds_w is not None else None
    return arr


def images_plan(sizes, kind: int, io_u8: bool, oh: int, ow: int, antialias: bool):
    """vs_images_plan on a list of (H, W): the launches as [(form, strip, [image indices], [first workgroups ..., grid])] (no GPU involved)"""
    L = lib()
    arr = (ImageDesc * max(1, len(sizes)))()
    for i, (H, W) in enumerate(sizes):
        arr[i].H, arr[i].W = H, W
    n = C.c_int(0)
    check(L.vs_images_plan(arr, len(sizes), kind, int(io_u8), oh, ow, int(antialias), None, 0, C.byref(n)), "vs_images_plan")
    groups = (ImagesGroup * max(1, n.value))()
    check(L.vs_images_plan(arr, len(sizes), kind, int(io_u8), oh, ow, int(antialias), groups, n.value, C.byref(n)), "vs_images_plan")
    return [(g.form, g.strip, list(g.image[:g.count]), list(g.first_wg[:g.count + 1])) for g in groups[:n.value]]


AGGREGATIONS = {"avg": 0, "squared_avg": 1, "l1norm_avg": 2, "l2norm_avg": 3}      # VS_AGG_*


class ClipDesc(C.Structure):
    """mirror of vs_clip_desc_t: one slot of a clip list -- a run of frames of one clip and where it sits in the processing-size tensors"""
    _fields_ = [("frames", C.c_void_p), ("out", C.c_void_p), ("preds_w", C.c_void_p), ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("first_frame", C.c_int32), ("first_key", C.c_int32)]


class TailClipsDesc(C.Structure):
    """mirror of vs_tail_clips_desc_t: vs_tail_images_desc_t's members over slots, then step and video_mode"""
    _fields_ = [
        ("clips", C.POINTER(ClipDesc)), ("delta", C.c_void_p), ("hmap_lowres", C.c_void_p), ("taps43", C.c_void_p),
        ("n", C.c_int32), ("S_h", C.c_int32), ("S_w", C.c_int32), ("Cd", C.c_int32),
        ("attenuate", C.c_int32), ("clamp", C.c_int32), ("antialias", C.c_int32), ("io_u8", C.c_int32),
        ("scaling_i", C.c_float), ("scaling_w", C.c_float), ("step", C.c_int32), ("video_mode", C.c_int32),
    ]


def clip_descs(slots, outs=None, preds_w=None):
    """the HOST descriptor array of a list of slots [(frames, first_frame, first_key)]: frames a device tensor fp32 [F, 3, H, W] or uint8
    [F, H, W, 3], contiguous; outs / preds_w: one tensor per slot or None.  Addresses and sizes, nothing is copied"""
    arr = (ClipDesc * max(1, len(slots)))()
    for i, (t, first_frame, first_key) in enumerate(slots):
        H, W = (t.shape[1], t.shape[2]) if t.dtype == torch.uint8 else (t.shape[-2], t.shape[-1])
        arr[i].frames, arr[i].F, arr[i].H, arr[i].W = ptr(t), t.shape[0], H, W
        arr[i].first_frame, arr[i].first_key = first_frame, first_key
        arr[i].out = ptr(outs[i]) if outs is not None else None
        arr[i].preds_w = ptr(preds_w[i]) if preds_w is not None else None
    return arr


def clips_plan(sizes, kind: int, io_u8: bool, oh: int, ow: int, antialias: bool):
    """vs_clips_plan on a list of (F, H, W): the launches as [(form, strip, [slot indices], [first workgroups ..., grid])] (no GPU involved)"""
    L = lib()
    arr = (ClipDesc * max(1, len(sizes)))()
    for i, (F_, H, W) in enumerate(sizes):
        arr[i].F, arr[i].H, arr[i].W = F_, H, W
    n = C.c_int(0)
    check(L.vs_clips_plan(arr, len(sizes), kind, int(io_u8), oh, ow, int(antialias), None, 0, C.byref(n)), "vs_clips_plan")
    groups = (ImagesGroup * max(1, n.value))()
    check(L.vs_clips_plan(arr, len(sizes), kind, int(io_u8), oh, ow, int(antialias), groups, n.value, C.byref(n)), "vs_clips_plan")
    return [(g.form, g.strip, list(g.image[:g.count]), list(g.first_wg[:g.count + 1])) for g in groups[:n.value]]


class YuvClipDesc(C.Structure):
    """mirror of vs_yuv_clip_desc_t: one slot of a list of YUV clips -- the surfaces of a run of frames of one clip and where it sits in the
    processing-size tensors"""
    _fields_ = [("src", YuvSurface), ("dst", YuvSurface), ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("first_frame", C.c_int32), ("first_key", C.c_int32)]


class TailYuvClipsDesc(C.Structure):
    """mirror of vs_tail_yuv_clips_desc_t: TailClipsDesc's members that apply to surfaces, then the two colour affines"""
    _fields_ = [
        ("clips", C.POINTER(YuvClipDesc)), ("delta", C.c_void_p), ("hmap_lowres", C.c_void_p), ("taps43", C.c_void_p),
        ("n", C.c_int32), ("S_h", C.c_int32), ("S_w", C.c_int32), ("Cd", C.c_int32),
        ("attenuate", C.c_int32), ("clamp", C.c_int32), ("antialias", C.c_int32),
        ("scaling_i", C.c_float), ("scaling_w", C.c_float), ("step", C.c_int32), ("video_mode", C.c_int32),
        ("yuv2rgb12", C.c_float * 12), ("rgb2yuv12", C.c_float * 12),
    ]


class YuvClipsGroup(C.Structure):
    """mirror of vs_yuv_clips_group_t: one launch of the plan"""
    _fields_ = [("form", C.c_int32), ("count", C.c_int32), ("strip", C.c_int32), ("reserved_", C.c_int32),
                ("slot", C.c_int32 * YUV_CLIPS_PER_LAUNCH), ("first_wg", C.c_int32 * (YUV_CLIPS_PER_LAUNCH + 1))]


def yuv_clip_descs(slots, outs=None):
    """the HOST descriptor array of a list of slots [(clip, first_frame, first_key)]: clip a yuv.Clip of device-resident planes at any pitch;
    outs: one clip per slot or None.  Addresses, pitches and sizes, nothing is copied"""
    arr = (YuvClipDesc * max(1, len(slots)))()
    for i, (c, first_frame, first_key) in enumerate(slots):
        arr[i].src = yuv_surface(c.planes, c.fmt)
        if outs is not None:
            arr[i].dst = yuv_surface(outs[i].planes, outs[i].fmt)
        arr[i].F, arr[i].H, arr[i].W = c.shape
        arr[i].first_frame, arr[i].first_key = first_frame, first_key
    return arr


def yuv_clips_plan(sizes, fmt: str, kind: int, oh: int, ow: int, antialias: bool):
    """vs_yuv_clips_plan on a list of (F, H, W) of format `fmt`: the launches as [(form, strip, [slot indices], [first workgroups ..., grid])]
    (no GPU involved)"""
    from .yuv import fmt_info
    L = lib()
    planar, depth, msb, chroma = fmt_info(fmt)
    arr = (YuvClipDesc * max(1, len(sizes)))()
    for i, (F_, H, W) in enumerate(sizes):
        arr[i].F, arr[i].H, arr[i].W = F_, H, W
        arr[i].src.planar, arr[i].src.depth, arr[i].src.msb_aligned, arr[i].src.chroma = int(planar), depth, int(msb), chroma
    n = C.c_int(0)
    check(L.vs_yuv_clips_plan(arr, len(sizes), kind, oh, ow, int(antialias), None, 0, C.byref(n)), "vs_yuv_clips_plan")
    groups = (YuvClipsGroup * max(1, n.value))()
    check(L.vs_yuv_clips_plan(arr, len(sizes), kind, oh, ow, int(antialias), groups, n.value, C.byref(n)), "vs_yuv_clips_plan")
    return [(g.form, g.strip, list(g.slot[:g.count]), list(g.first_wg[:g.count + 1])) for g in groups[:n.value]]


class ResblockThinDesc(C.Structure):
    """mirror of vs_resblock_thin_desc_t"""
    _fields_ = [
        ("x", C.c_void_p), ("x_ld", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
        ("w0_split", C.c_void_p), ("w1_split", C.c_void_p), ("wr_split", C.c_void_p),
        ("b0", C.c_void_p), ("b1", C.c_void_p), ("br", C.c_void_p),
        ("arith", C.c_int32), ("Cout", C.c_int32),
        ("a_mul", C.c_float), ("acc_mul0", C.c_float), ("acc_mul1", C.c_float), ("acc_mulr", C.c_float),
        ("out", C.c_void_p), ("out_ld", C.c_int64),
        ("outc_w", C.c_void_p), ("outc_b", C.c_void_p), ("out_ch", C.c_int32), ("use_tanh", C.c_int32), ("delta", C.c_void_p),
    ]


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load the shared library once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(or `make -C videoseal_amd/csrc`). There is no CPU/ATen fallback for the VideoSeal hot path.")
    L = C.CDLL(LIB_PATH)
    L.vs_version.restype = C.c_int
    L.vs_arch.restype = C.c_char_p
    L.vs_error_string.restype = C.c_char_p
    L.vs_error_string.argtypes = [C.c_int]
    P, I, I64, F = C.c_void_p, C.c_int, C.c_int64, C.c_float
    sig = {
        "vs_conv_gemm": [C.POINTER(ConvDesc), P],
        "vs_conv_plan": [C.POINTER(ConvDesc), I, I, C.POINTER(ConvPlan)],
        "vs_cnx_stage_plan": [I64, I, I, I, I, I, I, C.POINTER(CnxStagePlan)],
        "vs_to_planes": [P, I64, I, I64, F, P, P],
        "vs_to_planes_affine": [P, I64, I, I64, F, P, I64, P, I, P, P],
        "vs_layernorm_act": [P, I64, I, I64, P, P, F, I, P, I64, P],
        "vs_layernorm_patch2x2": [P, I, I, I, I, I64, P, P, F, P, P],
        "vs_stem_conv_ln": [P, I, I, I, I, P, P, P, P, F, I, P, I64, P],
        "vs_rmsnorm_act": [P, I64, I, I64, P, I, P, I64, P, I64, P],
        "vs_vit_attention": [P, I, I, I, I, I, I, P, P, P, P],
        "vs_dwconv7_ln": [P, I, I, I, I, I64, P, P, P, P, F, P, I64, P],
        "vs_dwconv7_ln_planes": [P, I, I, I, I, I64, P, P, P, P, F, F, I, P, P],
        "vs_grn_scale": [P, I, I, I, I64, P, P, P, P],
        "vs_grn_scale_from_partials": [P, I, I, I, P, P, I64, P],
        "vs_grn_scale_from_straddle_partials": [P, I, I, I, P, P, I64, P],
        "vs_grn_apply": [P, I, I, I, I64, P, I64, P, P],
        "vs_upcat2x": [P, I, I64, P, I, I64, F, I, I, I, P, I64, P],
        "vs_upconv_supported": [I],
        "vs_upconv_gather_ln": [P, I64, I, I, I, I, P, P, F, I, P, I64, P],
        "vs_cat2_scale": [P, I, I64, P, I, I64, F, I64, P, I64, P],
        "vs_msg_pre": [P, I, I, P, P],
        "vs_msg_pre_rows": [P, I64, I, I, P, P],
        "vs_upconv_fused_supported": [I, I, I],
        "vs_upconv_fused_preferred": [I, I, I],
        "vs_upconv_fused": [P, I, I64, P, I, I64, F, P, I, I, I, I, P, P, F, I, P, I64, I, F, F, P],
        "vs_im2col3x3": [P, I, I, I, I64, I, P, P],
        "vs_msg_latent": [P, P, I, I, I, P, P],
        "vs_broadcast_channels": [P, I, I, P, I, I, I64, I, P],
        "vs_outc_tanh": [P, I64, I, I, I64, P, P, I, I, P, P],
        "vs_pool_linear": [P, I, I, I, I64, P, P, I, P, P],
        "vs_resize_pre": [P, I, I, I, I, I, I, I, P, F, F, P, I, P, P],
        "vs_resize_pre_u8": [P, I, I, I, I, I, I, P, F, F, P, I, P, P],
        "vs_jnd_heatmap": [P, I, I, I, I64, I64, I64, I64, P, P, P],
        "vs_embed_tail": [C.POINTER(TailDesc), P],
        "vs_embed_tail_energy": [C.POINTER(TailDesc), P, P, P],
        "vs_psnr_scale": [P, I, I, I, I, F, F, P, P],
        "vs_embed_tail_scaled": [C.POINTER(TailDesc), P, P],
        "vs_nv12_default_color": [P, P],
        "vs_resize_pre_nv12": [P, I, I, I, I64, I64, P, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_nv12": [C.POINTER(TailNv12Desc), P],
        "vs_resize_pre_yuv420": [C.POINTER(Yuv420Surface), I, I, I, P, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_yuv420": [C.POINTER(TailYuv420Desc), P],
        "vs_yuv420_default_color": [I, P, P],
        "vs_resize_pre_yuv": [C.POINTER(YuvSurface), I, I, I, P, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_yuv": [C.POINTER(TailYuvDesc), P],
        "vs_resize_pre_rgb": [C.POINTER(RgbSurface), I, I, I, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_rgb": [C.POINTER(TailRgbDesc), P],
        "vs_resize_pre_half": [C.POINTER(HalfSurface), I, I, I, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_half": [C.POINTER(TailHalfDesc), P],
        "vs_resize_pre_images": [C.POINTER(ImageDesc), I, I, I, I, I, P, F, F, P, P, P],
        "vs_embed_tail_images": [C.POINTER(TailImagesDesc), P],
        "vs_images_plan": [C.POINTER(ImageDesc), I, I, I, I, I, I, C.POINTER(ImagesGroup), I, C.POINTER(C.c_int)],
        "vs_resize_pre_clips": [C.POINTER(ClipDesc), I, I, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_clips": [C.POINTER(TailClipsDesc), P],
        "vs_clips_plan": [C.POINTER(ClipDesc), I, I, I, I, I, I, C.POINTER(ImagesGroup), I, C.POINTER(C.c_int)],
        "vs_aggregate_clips": [P, I64, P, I, I, I, P, P],
        "vs_resize_pre_yuv_clips": [C.POINTER(YuvClipDesc), I, P, I, I, I, P, F, F, P, I, P, P],
        "vs_embed_tail_yuv_clips": [C.POINTER(TailYuvClipsDesc), P],
        "vs_yuv_clips_plan": [C.POINTER(YuvClipDesc), I, I, I, I, I, C.POINTER(YuvClipsGroup), I, C.POINTER(C.c_int)],
        "vs_aug_color": [P, P, I, I, I, I, F, P, P],
        "vs_aug_crop_flip": [P, P, I, I, I, I, I, I, I, I, P],
        "vs_aug_color_chain": [P, P, I, I, I, I, C.POINTER(C.c_int), C.POINTER(C.c_float), P, P],
        "vs_aug_crop_resize_color": [P, P, I, I, I, I, I, I, I, I, I, I, I, C.POINTER(C.c_int), C.POINTER(C.c_float), P],
        "vs_resize_nchw": [P, P, I, I, I, I, I, I, P],
        "vs_aug_warp": [P, P, I, I, I, I, I, I, P, I, P],
        "vs_gaussian_blur": [P, P, P, I, I, I, I, F, P],
        "vs_median_filter": [P, P, I, I, I, I, P],
        "vs_jpeg_roundtrip": [P, P, I, I, I, I, P, P],
        "vs_h264_proxy_roundtrip": [P, P, I, I, I, I, I, P, P],
        "vs_bn_batch_stats": [P, I64, I, I64, P, P, F, F, P, P, P, P, P, P],
        "vs_bn_partial_sums": [P, I64, I, I64, P, P, P],
        "vs_bn_finish_sums": [P, I, I64, P, P, F, F, P, P, P, P, P],
        "vs_scale_shift_act": [P, I64, I, I64, P, P, I, P, I64, P, I64, P],
        "vs_aug_mask_blend": [P, P, P, P, I, I, I, I, P],
        "vs_aug_add_scaled": [P, P, F, P, I64, P],
        "vs_aug_gather_frames": [P, P, P, I, I64, P],
        "vs_aug_window_average": [P, P, I, I64, I, F, P],
        "vs_gemm_wgrad": [P, I64, I, P, I64, I, I64, P, P, P],
        "vs_conv3x3_wgrad": [P, I64, I, P, I64, I, I, I, I, I, P, P, P],
        "vs_conv3x3_wgrad_supported": [I, I64, I],
        "vs_pad_embed1": [P, I, I, I, I64, P, P],
        "vs_reflect_fold1": [P, I, I, I, I64, P, P],
        "vs_pack_conv": [P, I, I, I, I, I, I, P, P],
        "vs_gaussian_blur_bwd": [P, P, P, I, I, I, I, F, P],
        "vs_aug_warp_bwd": [P, P, I, I, I, I, I, I, P, I, P, P],
        "vs_aug_gather_frames_bwd": [P, P, P, P, I, I64, P],
        "vs_aug_window_average_bwd": [P, P, I, I64, I, F, P],
        "vs_gelu_bwd": [P, I64, P, I64, I64, I, P, I64, P],
        "vs_act_bwd": [P, I64, P, I64, I64, I, I, P, I64, P],
        "vs_rmsnorm_act_bwd": [P, I64, I, I64, P, I, P, I64, P, I64, P, I64, P],
        "vs_vit_attention_bwd": [P, P, P, I, I, I, I, I, I, P, P, P, P, P, P, P],
        "vs_dwconv7": [P, I, I, I, I, I64, P, P, I, P, I64, P, I64, P],
        "vs_dwconv7_wgrad": [P, I64, P, I64, I, I, I, I, P, P, P],
        "vs_layernorm_bwd": [P, I64, P, I64, P, I64, I, F, P, I64, P, P, P, P, P],
        "vs_gelu_grn_bwd": [P, I64, P, I64, P, I, I, I, P, P, P, I64, P, P, P],
        "vs_patchify": [P, I, I, I, I64, I, P, P],
        "vs_unpatch": [P, I, I, I, I64, I, P, P],
        "vs_patchify_s": [P, I, I, I, I64, I, I, P, P],
        "vs_unpatch_s": [P, I, I, I, I64, I, I, P, P],
        "vs_col2im3x3_reflect": [P, I, I, I, I64, P, P],
        "vs_colmean": [P, I, I, I64, P, P],
        "vs_pool_gelu_bwd": [P, I64, P, I64, I, I, I, P, I64, P],
        "vs_matmul_small": [P, I64, P, I64, I, I, I, P, I64, P],
        "vs_bce_logits": [P, P, I, I, I, F, F, P, P, P],
        "vs_bn_mean_rstd": [P, I, I64, F, P, P, P],
        "vs_bn_relu_bwd_sums": [P, I64, P, I64, P, P, P, P, I, I64, I, P, P, P, P, P],
        "vs_bn_relu_bwd_apply": [P, I64, P, I64, P, P, P, P, I, P, I64, I, P, I64, P],
        "vs_dilate2": [P, I, I, I, I64, I, I, P, P],
        "vs_im2col3x3_strided": [P, I, I, I, I64, I, P, P],
        "vs_upcat2x_bwd": [P, I64, I, I, I, I, I, F, P, I64, P, I64, P],
        "vs_msg_table_grad": [P, P, I, I, I, P, P],
        "vs_outc_tanh_bwd": [P, P, I64, I, I, P, I, I, P, I64, P, P],
        "vs_relu_bwd": [P, I64, P, I64, I64, I, P, I64, P],
        "vs_resize_nchw_bwd": [P, P, I, I, I, I, I, I, P, P],
        "vs_embed_tail_bwd": [P, P, P, P, P, I, I, I, I, I, F, F, P, P],
        "vs_tail_key_reduce": [P, P, I, I, I, I, I, I, I, P, P],
        "vs_aug_crop_flip_bwd": [P, P, I, I, I, I, I, I, I, I, P],
        "vs_mask_mul": [P, P, P, I, I, I, I, I, P],
        "vs_aug_color_bwd": [P, P, P, I, I, I, I, F, P, P, P],
        "vs_clamp01_bwd": [P, P, P, I64, P],
        "vs_nhwc_to_nchw_scaled": [P, I, I, I, I, I64, F, P, P],
        "vs_percep_mse": [P, P, I, I, I, I, P, P, P],
        "vs_percep_mse_grad": [P, P, I, I, I, I, F, P, P],
        "vs_ssim_stats": [P, P, I, I, I, F, P, P, P, P],
        "vs_ssim_grad": [P, P, P, P, P, I, I, I, F, P, P, P],
        "vs_avgpool2_pad": [P, P, I, I, I, P, P, P],
        "vs_jnd_loss": [P, P, P, I, I, I, P, P, P],
        "vs_jnd_loss_grad": [P, P, P, I, I, I, F, P, P],
        "vs_split_block": [P, I, I64, I, I, F, P, P, P],
        "vs_check_finite": [P, I64, P, P],
        "vs_absmax": [P, I64, P, P],
        "vs_resblock_thin": [P, P],
        "vs_resblock_thin_supported": [I, I, I],
        "vs_cnx_block": [P, P, I, I64, I, I, F, F, P, I64, P, P, I64, P, I64, P, P],
        "vs_cnx_block_supported": [I, I64, I],
        "vs_pixel_upgather_supported": [I, I],
        "vs_pixel_upgather": [P, I64, I, I, I, I, I, P, P, F, I, P, I64, P],
        "vs_pixel_upgather_bwd": [P, I64, I, I, I, I, I, P, I64, P],
        "vs_pixel_linear": [P, I64, I, I64, I, P, P, I, I, P, P],
        "vs_pixel_linear_bwd": [P, P, P, I64, I, I64, I, P, I, P, I64, P, P, P, P],
        "vs_pixel_bce": [P, P, P, I, I, I, I64, F, F, F, P, P, P, P],
        "vs_pixel_vote": [P, I64, P, I, I, I64, F, P, P, P],
        "vs_embed_tail_regions": [C.POINTER(TailDesc), P, I, P],
        "vs_pixel_vote_regions": [P, I64, P, I, I, I, I, I, I, I, F, P, P, P, P, P],
        "vs_label_boxes": [P, I, I, I, I, P, P],
        "vs_embed_tail_images_energy": [C.POINTER(TailImagesDesc), P, P, P],
        "vs_embed_tail_images_scaled": [C.POINTER(TailImagesDesc), P, P],
        "vs_embed_tail_clips_energy": [C.POINTER(TailClipsDesc), P, P, I, P],
        "vs_embed_tail_clips_scaled": [C.POINTER(TailClipsDesc), P, I, P],
        "vs_psnr_scale_items": [P, P, P, I, I, F, F, P, P],
        "vs_disc_input": [P, I, I, I, P, P, P],
        "vs_disc_input_bwd": [P, I, I, I, P, P, P],
        "vs_groupnorm_lrelu": [P, I64, I, I, I, I, P, P, F, F, P, P, P, P, I64, P],
        "vs_groupnorm_lrelu_bwd": [P, I64, P, I64, I, I, I, I, P, P, P, P, F, P, P, I64, P, P, P],
        "vs_conv4x4_wgrad_supported": [I, I64, I],
        "vs_conv4x4_wgrad": [P, I64, I, P, I64, I, I, I, I, P, P, P],
        "vs_conv4x4_n1": [P, I64, I, I, I, P, P, P, P],
        "vs_conv4x4_n1_bwd": [P, I, I, I, I64, P, P, P],
        "vs_conv4x4_n1_bias_grad": [P, I64, P, P],
        "vs_disc_loss": [P, I64, P, I64, I, F, P, P, P, P],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L.vs_aug_color_scratch_floats.restype = C.c_int64
    L.vs_aug_color_scratch_floats.argtypes = [I, I, I]
    L.vs_jpeg_workspace_bytes.restype = C.c_int64
    L.vs_jpeg_workspace_bytes.argtypes = [I, I, I]
    L.vs_h264_proxy_workspace_bytes.restype = C.c_int64
    L.vs_h264_proxy_workspace_bytes.argtypes = [I, I, I]
    L.vs_vit_attention_bwd_scratch_floats.restype = C.c_int64
    L.vs_vit_attention_bwd_scratch_floats.argtypes = [I, I, I, I, I]
    for name in ("vs_aug_color_bwd_scratch_floats", "vs_percep_partial_doubles", "vs_ssim_partial_doubles", "vs_jnd_loss_partial_doubles"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [I, I, I]
    L.vs_tail_energy_partial_doubles.restype = C.c_int64
    L.vs_tail_energy_partial_doubles.argtypes = [I, I, I]
    L.vs_cnx_block_image_bytes.restype = C.c_int64
    L.vs_cnx_block_image_bytes.argtypes = [I]
    L.vs_bn_partial_doubles.restype = C.c_int64
    L.vs_bn_partial_doubles.argtypes = [I64, I64]
    for name, args in (("vs_gemm_wgrad_partial_floats", [I64, I, I]), ("vs_conv3x3_wgrad_partial_floats", [I, I64, I, I, I, I]), ("vs_dwconv7_wgrad_partial_floats", [I, I, I64]),
                       ("vs_colreduce_partial_floats", [I, I64, I64]), ("vs_bn_bwd_partial_floats", [I64, I64])):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = args
    L.vs_pixel_linear_bwd_partial_floats.restype = C.c_int64
    L.vs_pixel_linear_bwd_partial_floats.argtypes = [I64, I, I]
    L.vs_pixel_bce_partial_doubles.restype = C.c_int64
    L.vs_pixel_bce_partial_doubles.argtypes = [I, I, I64]
    L.vs_pixel_vote_regions_partial_doubles.restype = C.c_int64
    L.vs_pixel_vote_regions_partial_doubles.argtypes = [I, I, I64, I]
    L.vs_tail_images_energy_partial_doubles.restype = C.c_int64
    L.vs_tail_images_energy_partial_doubles.argtypes = [C.POINTER(ImageDesc), I, I, I, I, I]
    L.vs_tail_clips_energy_partial_doubles.restype = C.c_int64
    L.vs_tail_clips_energy_partial_doubles.argtypes = [C.POINTER(ClipDesc), I, I, I, I, I]
    L.vs_groupnorm_partial_doubles.restype = C.c_int64
    L.vs_groupnorm_partial_doubles.argtypes = [I, I, I]
    L.vs_conv4x4_wgrad_partial_floats.restype = C.c_int64
    L.vs_conv4x4_wgrad_partial_floats.argtypes = [I, I64, I, I, I, I]
    L.vs_sizeof_conv_desc.restype = C.c_int
    L.vs_sizeof_tail_desc.restype = C.c_int
    L.vs_sizeof_tail_nv12_desc.restype = C.c_int
    L.vs_sizeof_yuv420_surface.restype = L.vs_sizeof_tail_yuv420_desc.restype = C.c_int
    L.vs_sizeof_yuv_surface.restype = L.vs_sizeof_tail_yuv_desc.restype = C.c_int
    L.vs_sizeof_rgb_surface.restype = L.vs_sizeof_tail_rgb_desc.restype = C.c_int
    L.vs_sizeof_half_surface.restype = L.vs_sizeof_tail_half_desc.restype = C.c_int
    L.vs_sizeof_conv_plan.restype = L.vs_sizeof_cnx_stage_plan.restype = C.c_int
    if L.vs_version() != 3:
        raise NativeError(f"{LIB_PATH} has ABI version {L.vs_version()}, this binding is written for 3: rebuild (make -C videoseal_amd/csrc)")
    if L.vs_sizeof_conv_desc() != C.sizeof(ConvDesc) or L.vs_sizeof_tail_desc() != C.sizeof(TailDesc) or \
            L.vs_sizeof_tail_nv12_desc() != C.sizeof(TailNv12Desc) or L.vs_sizeof_conv_plan() != C.sizeof(ConvPlan) or \
            L.vs_sizeof_cnx_stage_plan() != C.sizeof(CnxStagePlan) or L.vs_sizeof_yuv420_surface() != C.sizeof(Yuv420Surface) or \
            L.vs_sizeof_tail_yuv420_desc() != C.sizeof(TailYuv420Desc) or L.vs_sizeof_yuv_surface() != C.sizeof(YuvSurface) or \
            L.vs_sizeof_tail_yuv_desc() != C.sizeof(TailYuvDesc) or L.vs_sizeof_rgb_surface() != C.sizeof(RgbSurface) or \
            L.vs_sizeof_tail_rgb_desc() != C.sizeof(TailRgbDesc) or L.vs_sizeof_half_surface() != C.sizeof(HalfSurface) or \
            L.vs_sizeof_tail_half_desc() != C.sizeof(TailHalfDesc):
        raise NativeError("ctypes mirrors of vs_conv_desc_t / vs_tail_desc_t / vs_tail_nv12_desc_t / vs_tail_yuv420_desc_t / vs_tail_yuv_desc_t / vs_tail_rgb_desc_t / vs_tail_half_desc_t / the plan structs are out of date with the shared library")
    _lib = L
    return L


ERR_UNSUPPORTED = -2      # VS_ERR_UNSUPPORTED: configuration outside what a kernel implements (callers with another form fall back to it)


def check(code: int, what: str) -> None:
    if code != 0:
        raise NativeError(f"{what} failed: {lib().vs_error_string(code).decode()} (code {code})")


@contextlib.contextmanager
def debug(name: str, value: int):
    """Development switch VS_DBG_<name> (csrc/vs_common.h) = value inside the block; 0 again -- the environment default, else the library's
    choice -- after it.  Process-global: tests and tools only."""
    L = lib()
    key = L.vs_debug_key(name.encode())
    if key < 0:
        raise NativeError(f"no development switch named {name!r} (VS_DBG_KEYS, csrc/vs_common.h)")
    check(L.vs_debug_set(key, int(value)), "vs_debug_set")
    try:
        yield
    finally:
        L.vs_debug_set(key, 0)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise NativeError("HIP kernels need device tensors (got a CPU tensor); move the model/inputs to cuda first")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def f32c(t: torch.Tensor) -> torch.Tensor:
    """contiguous float32 view/copy (plumbing)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()
