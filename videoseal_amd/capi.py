"""ctypes binding of the MODEL-LEVEL C-ABI (include/videoseal_hip.h: vs_model_create / vs_model_embed / vs_model_detect).

This is the stub a non-Python host would write in its own FFI: card numbers + the reference state_dict go in once, whole-path
calls take raw device pointers, a workspace and a stream.  The Python `Videoseal` class (model.py) drives the operator-level
entry points itself (per-shape tile tuning, hipGraph capture); `CModel` exists to exercise and document the C boundary."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import native as N
from .layout import ModelCfg


class ModelCfgC(C.Structure):
    """mirror of vs_model_cfg_t"""
    _fields_ = [("nbits", C.c_int32), ("hidden", C.c_int32), ("img_size", C.c_int32), ("in_ch", C.c_int32), ("out_ch", C.c_int32),
                ("yuv", C.c_int32), ("nlev", C.c_int32), ("zc", C.c_int32 * 8), ("num_blocks", C.c_int32), ("last_tanh", C.c_int32),
                ("depths", C.c_int32 * 4), ("dims", C.c_int32 * 4), ("stem_stride", C.c_int32), ("attenuate", C.c_int32),
                ("clamp", C.c_int32), ("scaling_w", C.c_float), ("scaling_i", C.c_float), ("arith", C.c_int32), ("reserved_", C.c_int32)]


class TensorC(C.Structure):
    """mirror of vs_tensor_t"""
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


def _bind(L):
    if getattr(L, "_model_api_bound", False):
        return
    P, I, I64 = C.c_void_p, C.c_int, C.c_int64
    L.vs_model_create.argtypes = [C.POINTER(ModelCfgC), C.POINTER(TensorC), I, C.POINTER(P)]
    L.vs_model_create.restype = I
    L.vs_model_destroy.argtypes = [P]
    L.vs_model_destroy.restype = None
    L.vs_model_workspace_bytes.argtypes = [P, I, I, I, I]
    L.vs_model_workspace_bytes.restype = I64
    L.vs_model_embed.argtypes = [P, P, P, I, I, I, I, I, I, I, I, I, P, P, P, I64, P]
    L.vs_model_embed.restype = I
    L.vs_model_embed_psnr_workspace_bytes.argtypes = [P, I, I, I, I]
    L.vs_model_embed_psnr_workspace_bytes.restype = I64
    L.vs_model_embed_psnr.argtypes = [P, P, P, I, I, I, I, I, I, I, I, I, C.c_float, I, C.c_float, P, P, P, P, I64, P]
    L.vs_model_embed_psnr.restype = I
    L.vs_model_detect.argtypes = [P, P, I, I, I, I, I, P, P, I64, P]
    L.vs_model_detect.restype = I
    L.vs_model_set_nv12_color.argtypes = [P, P, P]
    L.vs_model_set_nv12_color.restype = I
    L.vs_model_embed_yuv420.argtypes = [P, C.POINTER(N.Yuv420Surface), C.POINTER(N.Yuv420Surface), P, P, P, I, I, I, I, I, I, I, I, P, I64, P]
    L.vs_model_embed_yuv420.restype = I
    L.vs_model_detect_yuv420.argtypes = [P, C.POINTER(N.Yuv420Surface), P, I, I, I, I, P, P, I64, P]
    L.vs_model_detect_yuv420.restype = I
    L.vs_model_embed_yuv.argtypes = [P, C.POINTER(N.YuvSurface), C.POINTER(N.YuvSurface), P, P, P, I, I, I, I, I, I, I, I, P, I64, P]
    L.vs_model_embed_yuv.restype = I
    L.vs_model_detect_yuv.argtypes = [P, C.POINTER(N.YuvSurface), P, I, I, I, I, P, P, I64, P]
    L.vs_model_detect_yuv.restype = I
    L.vs_model_embed_rgb.argtypes = [P, C.POINTER(N.RgbSurface), C.POINTER(N.RgbSurface), P, I, I, I, I, I, I, I, I, P, I64, P]
    L.vs_model_embed_rgb.restype = I
    L.vs_model_detect_rgb.argtypes = [P, C.POINTER(N.RgbSurface), I, I, I, I, P, P, I64, P]
    L.vs_model_detect_rgb.restype = I
    L.vs_model_embed_half.argtypes = [P, C.POINTER(N.HalfSurface), C.POINTER(N.HalfSurface), P, I, I, I, I, I, I, I, I, P, I64, P]
    L.vs_model_embed_half.restype = I
    L.vs_model_detect_half.argtypes = [P, C.POINTER(N.HalfSurface), I, I, I, I, P, P, I64, P]
    L.vs_model_detect_half.restype = I
    L._model_api_bound = True


class CModel:
    """vs_model_t built from a ModelCfg and a reference-format state_dict (any device; copied to host fp32 for the call)."""

    def __init__(self, cfg: ModelCfg, state_dict: Dict[str, torch.Tensor], attenuate: bool = True, clamp: bool = True,
                 scaling_w: Optional[float] = None, scaling_i: Optional[float] = None):
        L = N.lib()
        _bind(L)
        if cfg.extractor != "convnext" or cfg.unet_norm != "batch":
            raise NotImplementedError("the model-level C-ABI covers the released cards (BatchNorm/ReLU U-Net + ConvNeXt-V2 extractor); "
                                      "the legacy videoseal_0.0 family runs through the operator-level entry points (videoseal_amd.engine)")
        if list(cfg.head_stages) != [1] or cfg.head_pixelwise or cfg.head_sigmoid:
            raise NotImplementedError("the model-level C-ABI passes [F, 1+nbits] rows of logits: extractors with up-scaling stages or a pixel-wise "
                                      "head run through the operator-level entry points (videoseal_amd.engine, csrc/pixel_head.hip)")
        self.cfg = cfg
        c = ModelCfgC()
        c.nbits, c.hidden, c.img_size, c.in_ch, c.out_ch, c.yuv = cfg.nbits, cfg.hidden, cfg.img_size, cfg.in_ch, cfg.out_ch, int(cfg.yuv)
        zc = cfg.zc
        c.nlev = len(zc) - 1
        for i, v in enumerate(zc):
            c.zc[i] = v
        c.num_blocks, c.last_tanh, c.stem_stride = cfg.num_blocks, int(cfg.last_tanh), cfg.stem_stride
        for i in range(4):
            c.depths[i], c.dims[i] = cfg.depths[i], cfg.dims[i]
        c.attenuate, c.clamp = int(attenuate), int(clamp)
        c.scaling_w = cfg.scaling_w if scaling_w is None else scaling_w
        c.scaling_i = cfg.scaling_i if scaling_i is None else scaling_i
        keep = []
        items = [(k, v) for k, v in state_dict.items() if v.dtype.is_floating_point]
        arr = (TensorC * len(items))()
        for i, (k, v) in enumerate(items):
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            arr[i].name, arr[i].data, arr[i].numel = k.encode(), t.data_ptr(), t.numel()
        h = C.c_void_p()
        N.check(L.vs_model_create(C.byref(c), arr, len(items), C.byref(h)), "vs_model_create")
        self._h, self._L = h, L
        self._ws: Optional[torch.Tensor] = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.vs_model_destroy(self._h)
            self._h = None

    def _workspace(self, frames, H, W, step) -> torch.Tensor:
        need = int(self._L.vs_model_workspace_bytes(self._h, frames, H, W, step))
        if need < 0:
            raise N.NativeError("vs_model_workspace_bytes failed")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        return self._ws

    def set_nv12_color(self, matrix: str = "bt709", full_range: bool = False) -> None:
        """colour choice of the NV12 clips (io_u8 = 2) of later calls; a fresh model reads BT.709 limited range"""
        from .nv12 import color_affine
        fwd, inv = color_affine(matrix, full_range)
        dec = (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)])
        enc = (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])
        N.check(self._L.vs_model_set_nv12_color(self._h, dec, enc), "vs_model_set_nv12_color")

    @staticmethod
    def _frames(imgs: torch.Tensor):
        """(contiguous frames, F, H, W, io_u8): fp32 NCHW -> 0, uint8 RGB24 [F,H,W,3] -> 1, uint8 NV12 [F,3H/2,W] -> 2"""
        if imgs.dtype == torch.uint8 and imgs.dim() == 3:
            from .nv12 import check_clip
            F_, H, W = check_clip(imgs)
            return imgs.contiguous(), F_, H, W, 2
        if imgs.dtype == torch.uint8:
            x = imgs.contiguous()
            return x, x.shape[0], x.shape[1], x.shape[2], 1
        x = N.f32c(imgs)
        return x, x.shape[0], x.shape[2], x.shape[3], 0

    def embed(self, imgs: torch.Tensor, msgs: torch.Tensor, *, step: int = 1, video_mode: int = 0, lowres_attenuation: bool = False,
              antialias: bool = True, want_preds_w: bool = False):
        x, F_, H, W, u8 = self._frames(imgs)           # uint8 clips (RGB24 [F,H,W,3] or NV12 [F,3H/2,W]) come back in their own format
        m = msgs.to(device=x.device, dtype=torch.int32).contiguous()
        out = torch.empty_like(x)
        pw = torch.empty(F_, self.cfg.out_ch, H, W, device=x.device) if want_preds_w else None
        ws = self._workspace(F_, H, W, step)
        N.check(self._L.vs_model_embed(self._h, N.ptr(x), N.ptr(m), m.shape[0], F_, H, W, step, video_mode, int(lowres_attenuation),
                                       int(antialias), int(u8), N.ptr(out), N.ptr(pw), N.ptr(ws), ws.numel(), N.stream()), "vs_model_embed")
        return (out, pw) if want_preds_w else out

    def embed_psnr(self, imgs: torch.Tensor, msgs: torch.Tensor, target_psnr: float, *, per_clip: bool = False,
                   max_scaling_w: Optional[float] = None, step: int = 1, video_mode: int = 0, lowres_attenuation: bool = False,
                   antialias: bool = True):
        """vs_model_embed_psnr on one chunk of fp32 NCHW or uint8 RGB24 frames -> (imgs_w, the strengths applied: fp32 [F] on the device)"""
        x, F_, H, W, u8 = self._frames(imgs)
        m = msgs.to(device=x.device, dtype=torch.int32).contiguous()
        out = torch.empty_like(x)
        scale = torch.empty(F_, device=x.device, dtype=torch.float32)
        need = int(self._L.vs_model_embed_psnr_workspace_bytes(self._h, F_, H, W, step))
        if need < 0:
            raise N.NativeError("vs_model_embed_psnr_workspace_bytes failed")
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        N.check(self._L.vs_model_embed_psnr(self._h, N.ptr(x), N.ptr(m), m.shape[0], F_, H, W, step, video_mode, int(lowres_attenuation),
                                            int(antialias), int(u8), float(target_psnr), int(per_clip), float(max_scaling_w or 0.0),
                                            N.ptr(out), None, N.ptr(scale), N.ptr(ws), ws.numel(), N.stream()), "vs_model_embed_psnr")
        return out, scale

    def embed_regions(self, *args, **kwargs):
        raise NotImplementedError("the model-level C-ABI (vs_model_*) has no region-wise entry point: label maps go through the operator-level "
                                  "entry points of include/videoseal_regions.h (Videoseal.embed_regions / decode_regions / detect_regions)")

    decode_regions = detect_regions = embed_regions

    def detect(self, imgs: torch.Tensor, antialias: bool = True) -> torch.Tensor:
        x, F_, H, W, u8 = self._frames(imgs)
        logits = torch.empty(F_, self.cfg.nbits + 1, device=x.device)
        ws = self._workspace(F_, H, W, 1)
        N.check(self._L.vs_model_detect(self._h, N.ptr(x), F_, H, W, int(antialias), int(u8), N.ptr(logits), N.ptr(ws), ws.numel(), N.stream()),
                "vs_model_detect")
        return logits

    @staticmethod
    def _yuv_color(depth: int, color):
        """(yuv2rgb12, rgb2yuv12) host arrays for `color` = (matrix, full_range), or (None, None) = the library's default at that depth"""
        if color is None:
            return None, None
        from .yuv import color_affine
        fwd, inv = color_affine(color[0], bool(color[1]), depth)
        return (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)]), (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])

    def _embed_yuv(self, module, surface, entry, planes, fmt, msgs, out_planes, color, step, video_mode, lowres_attenuation, antialias):
        """one body for embed_yuv420 and embed_yuv: `module` checks the format, `surface` makes the surface type of the library's
        entry point `entry`"""
        from .yuv import Clip
        F_, H, W = module.check_clip(planes, fmt)
        src = Clip(planes, fmt)
        dst = Clip(out_planes, fmt) if out_planes is not None else src.empty_like()
        m = msgs.to(device=src.device, dtype=torch.int32).contiguous()
        ws = self._workspace(F_, H, W, step)
        dec, enc = self._yuv_color(module.fmt_info(fmt)[1], color)
        sin, sout = surface(src.planes, fmt), surface(dst.planes, fmt)
        N.check(entry(self._h, C.byref(sin), C.byref(sout), dec, enc, N.ptr(m), m.shape[0], F_, H, W, step, video_mode, int(lowres_attenuation),
                      int(antialias), N.ptr(ws), ws.numel(), N.stream()), entry.__name__)
        return dst.planes

    def _detect_yuv(self, module, surface, entry, planes, fmt, color, antialias) -> torch.Tensor:
        from .yuv import Clip
        F_, H, W = module.check_clip(planes, fmt)
        src = Clip(planes, fmt)
        logits = torch.empty(F_, self.cfg.nbits + 1, device=src.device)
        ws = self._workspace(F_, H, W, 1)
        dec, _ = self._yuv_color(module.fmt_info(fmt)[1], color)
        sin = surface(src.planes, fmt)
        N.check(entry(self._h, C.byref(sin), dec, F_, H, W, int(antialias), N.ptr(logits), N.ptr(ws), ws.numel(), N.stream()), entry.__name__)
        return logits

    def embed_yuv420(self, planes, fmt: str, msgs: torch.Tensor, *, out_planes=None, color=None, step: int = 1, video_mode: int = 0,
                     lowres_attenuation: bool = False, antialias: bool = True):
        """vs_model_embed_yuv420 on device-resident planes (any pitches); `out_planes`: where the watermarked clip goes (default: a new
        packed clip).  `color` = (matrix, full_range) or None = NULL affines.  Returns the output planes."""
        from . import yuv420
        return self._embed_yuv(yuv420, N.yuv420_surface, self._L.vs_model_embed_yuv420, planes, fmt, msgs, out_planes, color, step, video_mode,
                               lowres_attenuation, antialias)

    def detect_yuv420(self, planes, fmt: str, *, color=None, antialias: bool = True) -> torch.Tensor:
        from . import yuv420
        return self._detect_yuv(yuv420, N.yuv420_surface, self._L.vs_model_detect_yuv420, planes, fmt, color, antialias)

    def embed_yuv(self, planes, fmt: str, msgs: torch.Tensor, *, out_planes=None, color=None, step: int = 1, video_mode: int = 0,
                  lowres_attenuation: bool = False, antialias: bool = True):
        """vs_model_embed_yuv on device-resident planes of any of the ten formats (yuv.py; any pitches); `out_planes`, `color` and the
        result as for embed_yuv420."""
        from . import yuv
        return self._embed_yuv(yuv, N.yuv_surface, self._L.vs_model_embed_yuv, planes, fmt, msgs, out_planes, color, step, video_mode,
                               lowres_attenuation, antialias)

    def detect_yuv(self, planes, fmt: str, *, color=None, antialias: bool = True) -> torch.Tensor:
        from . import yuv
        return self._detect_yuv(yuv, N.yuv_surface, self._L.vs_model_detect_yuv, planes, fmt, color, antialias)

    def embed_rgb(self, clip: torch.Tensor, fmt: str, msgs: torch.Tensor, *, out: Optional[torch.Tensor] = None, step: int = 1,
                  video_mode: int = 0, lowres_attenuation: bool = False, antialias: bool = True) -> torch.Tensor:
        """vs_model_embed_rgb on a device-resident packed RGB clip of format `fmt` (rgbpack.py; any pitch); `out`: where the watermarked clip
        goes (default: a new compact clip).  Returns the output clip."""
        from . import rgbpack
        F_, H, W = rgbpack.check_clip(clip, fmt)
        src = rgbpack.Clip(clip, fmt)
        if out is not None:
            rgbpack.check_clip(out, fmt, "out")
        dst = rgbpack.Clip(out, fmt) if out is not None else src.empty_like()
        m = msgs.to(device=src.device, dtype=torch.int32).contiguous()
        ws = self._workspace(F_, H, W, step)
        sin, sout = N.rgb_surface(src.tensor, fmt), N.rgb_surface(dst.tensor, fmt)
        N.check(self._L.vs_model_embed_rgb(self._h, C.byref(sin), C.byref(sout), N.ptr(m), m.shape[0], F_, H, W, step, video_mode,
                                           int(lowres_attenuation), int(antialias), N.ptr(ws), ws.numel(), N.stream()), "vs_model_embed_rgb")
        return dst.tensor

    def detect_rgb(self, clip: torch.Tensor, fmt: str, *, antialias: bool = True) -> torch.Tensor:
        from . import rgbpack
        F_, H, W = rgbpack.check_clip(clip, fmt)
        src = rgbpack.Clip(clip, fmt)
        logits = torch.empty(F_, self.cfg.nbits + 1, device=src.device)
        ws = self._workspace(F_, H, W, 1)
        sin = N.rgb_surface(src.tensor, fmt)
        N.check(self._L.vs_model_detect_rgb(self._h, C.byref(sin), F_, H, W, int(antialias), N.ptr(logits), N.ptr(ws), ws.numel(), N.stream()),
                "vs_model_detect_rgb")
        return logits

    def embed_half(self, clip: torch.Tensor, msgs: torch.Tensor, *, value_range: str = "unit", layout: str = "nchw", out: Optional[torch.Tensor] = None,
                   step: int = 1, video_mode: int = 0, lowres_attenuation: bool = False, antialias: bool = True) -> torch.Tensor:
        """vs_model_embed_half on a device-resident float16 / bfloat16 clip (halfpix.py; any pitch); `out`: where the watermarked clip goes
        (default: a new compact clip of the same memory form).  msgs [1, k], or [frames, k] with step = 1 (image mode).  Returns the output clip."""
        from . import halfpix
        F_, H, W = halfpix.check_clip(clip, layout, value_range)
        src = halfpix.Clip(clip, layout, value_range)
        if out is not None:
            halfpix.check_clip(out, layout, value_range, "out")
        dst = halfpix.Clip(out, layout, value_range) if out is not None else src.empty_like()
        m = msgs.to(device=src.device, dtype=torch.int32).contiguous()
        ws = self._workspace(F_, H, W, step)
        sin, sout = N.half_surface(src.tensor, layout, value_range), N.half_surface(dst.tensor, layout, value_range)
        N.check(self._L.vs_model_embed_half(self._h, C.byref(sin), C.byref(sout), N.ptr(m), m.shape[0], F_, H, W, step, video_mode,
                                            int(lowres_attenuation), int(antialias), N.ptr(ws), ws.numel(), N.stream()), "vs_model_embed_half")
        return dst.tensor

    def detect_half(self, clip: torch.Tensor, *, value_range: str = "unit", layout: str = "nchw", antialias: bool = True) -> torch.Tensor:
        from . import halfpix
        F_, H, W = halfpix.check_clip(clip, layout, value_range)
        logits = torch.empty(F_, self.cfg.nbits + 1, device=clip.device)
        ws = self._workspace(F_, H, W, 1)
        sin = N.half_surface(clip, layout, value_range)
        N.check(self._L.vs_model_detect_half(self._h, C.byref(sin), F_, H, W, int(antialias), N.ptr(logits), N.ptr(ws), ws.numel(), N.stream()),
                "vs_model_detect_half")
        return logits
