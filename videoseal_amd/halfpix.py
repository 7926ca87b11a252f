"""Half-precision RGB clips: the definitions of `Videoseal.embed_half` / `detect_half` as executable text (plain torch, any device).

Layout.  A clip is ONE tensor of dtype float16 or bfloat16; `layout` names its shape, the memory form is read from its strides:
    layout   shape              memory form      strides (elements)
    "nchw"   [F, 3, H, W]       planar           stride(3) == 1, row pitch stride(2) >= W, planes and frames kept apart
                                channels-last    stride(1) == 1, stride(3) == 3, row pitch stride(2) >= 3 W: the memory of a compact [F, H, W, 3]
    "nhwc"   [F, H, W, 3 | 4]   packed           component stride 1, pixel stride C, row pitch stride(1) >= C W, any frame stride
A strided view stays a view; nothing is copied.  With 4 components the fourth is alpha.

Rules, with `value_range` "unit" (stored value = component) or "signed" (stored value y, component v = y * 0.5 + 0.5):
    Decode   v = x.float() for unit, x.float() * 0.5 + 0.5 in fp32 for signed (the product is exact: one rounding, in the sum).  Decoded
             values are NOT clamped: a generator overshoots its range, and the fp32 path sees such values unclamped too.
    Encode   w = clamp(v, 0, 1), a negative zero counting as +0.0; the stored word is w.to(dtype) for unit, (w * 2 - 1).to(dtype) for signed: one fp32 rounding (w * 2 is
             exact), then round-to-nearest-even into the 16-bit type.  Results below 2^-14 are fp16 subnormals, not zero.
    Alpha    the alpha word of an output pixel is the source pixel's, bit for bit (NaN payloads included); it never enters arithmetic.
             Without a source (`like=None`) alpha is 1.0.
    Non-finite inputs are outside the contract, as they are for `embed`.
Round trip, by enumeration of all 65 536 words of each type (tests/test_halfpix_cpu.py): from_rgb(to_rgb(x)) returns the word unchanged for
    unit     every finite word in [0, 1] except -0.0, which comes back as +0.0: 15 361 fp16 words, 16 257 bf16 words; no word outside.
    signed   the finite words in [-1, 1] whose y * 0.5 + 0.5 is exact in fp32, i.e. whose y / 2 is a multiple of the fp32 spacing at the
             sum (2^-25 below 0.5, 2^-24 from 0.5 on); a smaller y / 2 is rounded away in the sum and the word comes back as a neighbour
             or as zero.  fp16: 29 697 of the 30 722 words of [-1, 1]; the 1 025 others are -0.0 and words of |y| <= 2^-13.  bf16, whose
             steps near zero are far finer than fp32's at 0.5: 4 481 of 32 514; the others have |y| < 2^-16.  ROUND_TRIP holds the counts.
Not supported: fp32 surfaces with a value range, planar alpha, big-endian words, premultiplied alpha.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import yuv as _yuv

DTYPES = {torch.float16: 0, torch.bfloat16: 1}            # VS_HALF_FP16 / VS_HALF_BF16
LAYOUTS = ("nchw", "nhwc")
RANGES = {"unit": 0, "signed": 1}                         # VS_HALF_UNIT / VS_HALF_SIGNED
PLANAR, PACKED = 0, 1                                     # VS_HALF_PLANAR / VS_HALF_PACKED

# words x with from_rgb(to_rgb(x)) == x bit for bit, of the 65 536 of each type: (dtype, value_range) -> count
ROUND_TRIP = {
    (torch.float16, "unit"): 15361, (torch.bfloat16, "unit"): 16257,
    (torch.float16, "signed"): 29697, (torch.bfloat16, "signed"): 4481,
}


def _check_names(layout: str, value_range: str) -> None:
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {list(LAYOUTS)}, got {layout!r}")
    if value_range not in RANGES:
        raise ValueError(f"value_range must be one of {sorted(RANGES)}, got {value_range!r}")


def memory_form(clip: torch.Tensor, layout: str) -> Tuple[int, int]:
    """(PLANAR | PACKED, components) of a checked clip"""
    if layout == "nhwc":
        return PACKED, clip.shape[3]
    W = clip.shape[3]
    if clip.stride(1) == 1 and (W == 1 or clip.stride(3) == 3) and not (clip.stride(3) == 1 and W > 1):
        return PACKED, 3
    return PLANAR, 3


def check_clip(clip: torch.Tensor, layout: str = "nchw", value_range: str = "unit", what: str = "clip") -> Tuple[int, int, int]:
    """(F, H, W) of a valid clip; ValueError with the reason otherwise"""
    _check_names(layout, value_range)
    if not torch.is_tensor(clip):
        raise ValueError(f"{what}: a half clip is one tensor")
    if clip.dtype not in DTYPES:
        raise ValueError(f"{what}: a half clip is a float16 or bfloat16 tensor, got {clip.dtype} (fp32 frames go to embed / detect, integer "
                         f"ones to embed_rgb / detect_rgb)")
    if clip.dim() != 4:
        raise ValueError(f"{what}: a half clip has four dimensions, got {tuple(clip.shape)}")
    if layout == "nchw":
        F_, C, H, W = clip.shape
        if C != 3:
            raise ValueError(f"{what}: an nchw clip has shape [F, 3, H, W], got {tuple(clip.shape)} (alpha travels in nhwc clips only)")
    else:
        F_, H, W, C = clip.shape
        if C not in (3, 4):
            raise ValueError(f"{what}: an nhwc clip has shape [F, H, W, 3 | 4], got {tuple(clip.shape)}")
    if H < 1 or W < 1:
        raise ValueError(f"{what}: a half clip needs H, W >= 1 (got {H} x {W})")
    if clip.numel() == 0:
        return F_, H, W
    sf = clip.stride(0)
    if layout == "nhwc" or memory_form(clip, layout)[0] == PACKED:
        sy, sx, sc = (clip.stride(1), clip.stride(2), clip.stride(3)) if layout == "nhwc" else (clip.stride(2), clip.stride(3), clip.stride(1))
        if sc != 1 or (W > 1 and sx != C):
            raise ValueError(f"{what}: the pixels of a row must be compact (component stride 1, pixel stride {C})")
        if H > 1 and sy < W * C:
            raise ValueError(f"{what}: the row pitch ({sy}) is shorter than a row ({W * C} elements)")
        if F_ > 1 and sf < (sy * (H - 1) if H > 1 else 0) + W * C:
            raise ValueError(f"{what}: frames overlap (frame stride {sf})")
        return F_, H, W
    sp, sy, sx = clip.stride(1), clip.stride(2), clip.stride(3)
    if W > 1 and sx != 1:
        raise ValueError(f"{what}: an nchw clip is planar (stride(3) == 1) or channels-last (stride(1) == 1, stride(3) == 3), got strides {tuple(clip.stride())}")
    if H > 1 and sy < W:
        raise ValueError(f"{what}: the row pitch ({sy}) is shorter than a row ({W} elements)")
    plane = (sy * (H - 1) if H > 1 else 0) + W
    if abs(sp) < plane:
        raise ValueError(f"{what}: planes overlap (plane stride {sp})")
    if F_ > 1:
        # frames apart: whole frames one after the other, or the frames of a plane interleaved below the plane stride
        if not (sf >= 2 * abs(sp) + plane or (plane <= sf and sf * (F_ - 1) + plane <= abs(sp))):
            raise ValueError(f"{what}: frames overlap (frame stride {sf})")
    return F_, H, W


def _pixels(clip: torch.Tensor, layout: str) -> torch.Tensor:
    """the clip as [F, H, W, C] (a view)"""
    return clip if layout == "nhwc" else clip.permute(0, 2, 3, 1)


def to_rgb(clip: torch.Tensor, layout: str = "nchw", value_range: str = "unit") -> torch.Tensor:
    """clip -> fp32 RGB [F, 3, H, W], contiguous: the component values, not clamped"""
    check_clip(clip, layout, value_range, "to_rgb")
    v = _pixels(clip, layout)[..., :3].permute(0, 3, 1, 2).float()
    if value_range == "signed":
        v = v * 0.5 + 0.5
    return v.contiguous()


def empty_like(clip: torch.Tensor, layout: str = "nchw", device=None) -> torch.Tensor:
    """an uninitialised compact clip of `clip`'s dtype, shape and memory form"""
    dev = clip.device if device is None else device
    if layout == "nhwc":
        return torch.empty(tuple(clip.shape), dtype=clip.dtype, device=dev)
    F_, C, H, W = clip.shape
    if clip.numel() and memory_form(clip, layout)[0] == PACKED:
        return torch.empty((F_, H, W, C), dtype=clip.dtype, device=dev).permute(0, 3, 1, 2)
    return torch.empty((F_, C, H, W), dtype=clip.dtype, device=dev)


def from_rgb(x01: torch.Tensor, like: Optional[torch.Tensor] = None, layout: str = "nchw", value_range: str = "unit",
             dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """fp32 RGB [F, 3, H, W] -> a compact clip: clamp to [0, 1], map to the stored range in fp32, round to nearest even.  `like` (a clip of the
    same layout and size) gives the dtype, the memory form and the alpha words; without it the result is planar / packed `dtype`, alpha 1.0"""
    _check_names(layout, value_range)
    if x01.dim() != 4 or x01.shape[1] != 3 or x01.dtype != torch.float32:
        raise ValueError("from_rgb wants fp32 [F, 3, H, W]")
    F_, _, H, W = x01.shape
    if like is not None:
        if tuple(check_clip(like, layout, value_range, "from_rgb: like")) != (F_, H, W):
            raise ValueError(f"from_rgb: `like` is {tuple(like.shape)} for frames {tuple(x01.shape)}")
        dtype = like.dtype
    elif dtype not in DTYPES:
        raise ValueError("from_rgb needs `like` or a dtype of float16 / bfloat16")
    w = x01.clamp(0.0, 1.0) + 0.0                           # (-0.0 + 0.0 = +0.0: the kernels' clamp returns +0.0 for every t <= 0)
    if value_range == "signed":
        w = w * 2.0 - 1.0
    w = w.to(dtype)                                         # [F, 3, H, W]
    if like is None:
        out = torch.empty((F_, H, W, 3) if layout == "nhwc" else (F_, 3, H, W), dtype=dtype, device=x01.device)
    else:
        out = empty_like(like, layout, device=x01.device)
    px = _pixels(out, layout)
    px[..., :3] = w.permute(0, 2, 3, 1)
    if px.shape[-1] == 4:                                   # the alpha words travel as integers: a NaN keeps its payload
        px.view(torch.int16)[..., 3] = like.to(x01.device).view(torch.int16)[..., 3]
    return out


class Clip(_yuv.Clip):
    """A half clip as the clip object `Videoseal._run_chunks` and the graph cache walk: yuv.Clip with ONE plane -- the tensor itself, in the
    caller's shape and strides -- and the layout and value range in its graph key.  A new clip (`empty_like`) is compact and keeps the
    memory form."""

    def __init__(self, clip: torch.Tensor, layout: str = "nchw", value_range: str = "unit", buf: torch.Tensor = None):
        _check_names(layout, value_range)
        self.planes = (clip,)
        self.layout, self.value_range, self.color, self.buf = layout, value_range, None, buf
        F_, H, W = (clip.shape[0], clip.shape[1], clip.shape[2]) if layout == "nhwc" else (clip.shape[0], clip.shape[2], clip.shape[3])
        self.shape = (F_, H, W)
        form, comps = memory_form(clip, layout) if clip.numel() else (PLANAR if layout == "nchw" else PACKED, clip.shape[1 if layout == "nchw" else 3])
        self.form, self.components = form, comps
        self.fmt = f"{'f16' if clip.dtype == torch.float16 else 'bf16'}.{value_range}.{'planar' if form == PLANAR else 'packed' + str(comps)}"

    tensor = property(lambda self: self.planes[0])
    graph_key = property(lambda self: (self.fmt, self.layout))

    def __getitem__(self, s) -> "Clip":
        if not isinstance(s, slice):
            raise TypeError("a clip is sliced by frame ranges")
        return Clip(self.planes[0][s], self.layout, self.value_range, self.buf[s] if self.buf is not None else None)

    def empty_like(self, device=None) -> "Clip":
        buf = empty_like(self.planes[0], self.layout, device)
        return Clip(buf, self.layout, self.value_range, buf)

    def contiguous(self) -> "Clip":
        return self                                         # (a strided view is a valid clip: nothing to compact)

    def to(self, device) -> "Clip":
        return Clip(self.planes[0].to(device), self.layout, self.value_range)


def clip(t: torch.Tensor, layout: str = "nchw", value_range: str = "unit") -> Clip:
    """the clip object of a checked tensor; ValueError for unknown names or a tensor that is no half clip"""
    check_clip(t, layout, value_range)
    return Clip(t, layout, value_range)
