"""YUV clips of every supported chroma format: the definitions of `Videoseal.embed_yuv` / `detect_yuv` as executable text (plain torch, any
device).  The four 4:2:0 formats are yuv420.py's, and every function here hands them to that module; this one adds 4:2:2 and 4:4:4.

Layout.  A clip is a tuple of plane tensors on one device; `fmt` is ffmpeg's pix_fmt name without the "le":
    fmt          dtype    planes                                        chroma
    "yuv422p"    uint8    (y [F, H, W], u [F, H, W/2], v [F, H, W/2])   4:2:2
    "yuv422p10"  uint16   as yuv422p; sample code = min(word, 1023)     4:2:2
    "nv16"       uint8    (y [F, H, W], uv [F, H, W])                   4:2:2   uv[..., 2j], uv[..., 2j+1] = Cb, Cr of block j of the row
    "p210"       uint16   as nv16; sample code = word >> 6              4:2:2   (the low 6 bits are ignored on input and zero on output)
    "yuv444p"    uint8    (y, u, v), each [F, H, W]                     4:4:4
    "yuv444p10"  uint16   as yuv444p; sample code = min(word, 1023)     4:4:4
    "nv12", "i420", "p010", "yuv420p10": see yuv420.py                   4:2:0
The size rule comes from the format: 4:2:0 needs H and W even, 4:2:2 needs W even and takes any H >= 1, 4:4:4 takes any H, W >= 1.
Everything else is as for the 4:2:0 clips: every plane has last stride 1 and its own row pitch and frame stride, int16 tensors are accepted
as the same bits as uint16, `planes_of` cuts the planes out of a packed per-frame buffer (Y, then U, then V -- or Y, then UV; 2HW samples
per frame for 4:2:2, 3HW for 4:4:4) and `pack` is its inverse.

Colour.  yuv420.color_affine: bt601 / bt709 / bt2020, limited / full range, depth 8 / 10, built and inverted in float64.
Chroma.  A block is 2 x 1 pixels (4:2:2: two neighbours of one row) or 1 x 1 (4:4:4).  Up: every pixel of a block uses the block's (Cb, Cr).
Down: the mean of the block's per-pixel chroma values (two for 4:2:2, the value itself for 4:4:4), then one rounding.
Range and rounding.  After decoding every RGB channel is clamped to [0, 1]; output codes are floor(clamp(v, 0, 2^depth - 1) + 0.5), v in code
units (p210 stores code << 6) -- one rounding, no intermediate RGB24.
Not supported: packed formats (yuyv422, uyvy422, v210), semi-planar 4:4:4 (nv24, p410), depth 12, any other chroma siting.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import yuv420
from .yuv420 import DEFAULT_COLOR, MATRICES, _as_words, _codes, _words, color_affine  # noqa: F401  (re-exported: one colour definition)

#            planar, depth, msb_aligned, chroma
FORMATS = {**{k: v + (420,) for k, v in yuv420.FORMATS.items()},
           "yuv422p": (True, 8, False, 422), "yuv422p10": (True, 10, False, 422), "nv16": (False, 8, False, 422), "p210": (False, 10, True, 422),
           "yuv444p": (True, 8, False, 444), "yuv444p10": (True, 10, False, 444)}
SHIFTS = {420: (1, 1), 422: (1, 0), 444: (0, 0)}            # chroma -> (sx, sy): a chroma sample serves (1 << sx) x (1 << sy) pixels


def fmt_info(fmt: str) -> Tuple[bool, int, bool, int]:
    """(planar, depth, msb_aligned, chroma) of `fmt`; ValueError for an unknown one"""
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    return FORMATS[fmt]


def is_420(fmt: str) -> bool:
    return fmt_info(fmt)[3] == 420


def fmt_dtype(fmt: str) -> torch.dtype:
    return torch.uint8 if fmt_info(fmt)[1] == 8 else torch.uint16


def plane_shapes(fmt: str, F_: int, H: int, W: int):
    """the shapes of the planes of an [F, H, W] clip"""
    planar, _, _, chroma = fmt_info(fmt)
    sx, sy = SHIFTS[chroma]
    if planar:
        return [(F_, H, W)] + [(F_, H >> sy, W >> sx)] * 2
    return [(F_, H, W), (F_, H >> sy, W)]


def frame_samples(fmt: str, H: int, W: int) -> int:
    """samples of one packed frame: 3HW/2, 2HW or 3HW"""
    return sum(s[1] * s[2] for s in plane_shapes(fmt, 1, H, W))


def _size_ok(chroma: int, H: int, W: int) -> bool:
    sx, sy = SHIFTS[chroma]
    return H % (1 << sy) == 0 and W % (1 << sx) == 0


def check_clip(planes: Sequence[torch.Tensor], fmt: str, what: str = "clip") -> Tuple[int, int, int]:
    """(F, H, W) of a valid clip; ValueError otherwise"""
    planar, depth, _, chroma = fmt_info(fmt)
    if chroma == 420:
        return yuv420.check_clip(planes, fmt, what)
    if not isinstance(planes, (tuple, list)) or len(planes) != (3 if planar else 2) or not all(torch.is_tensor(p) for p in planes):
        raise ValueError(f"{what}: {fmt} wants a tuple of {3 if planar else 2} plane tensors")
    planes = [_as_words(p) for p in planes]
    want = fmt_dtype(fmt)
    if any(p.dtype != want or p.dim() != 3 for p in planes):
        raise ValueError(f"{what}: {fmt} planes are {want} tensors [F, rows, samples]")
    if any(p.device != planes[0].device for p in planes):
        raise ValueError(f"{what}: the planes must be on one device")
    F_, H, W = planes[0].shape
    if not _size_ok(chroma, H, W):
        raise ValueError(f"{what}: a 4:2:2 clip needs an even W (got {H} x {W})")
    want_shapes = plane_shapes(fmt, F_, H, W)
    if any(tuple(p.shape) != s for p, s in zip(planes, want_shapes)):
        raise ValueError(f"{what}: a {fmt} clip with luma {tuple(planes[0].shape)} has chroma planes {want_shapes[1]}, got {[tuple(p.shape) for p in planes[1:]]}")
    if any(p.numel() > 0 and p.stride(2) != 1 for p in planes):
        raise ValueError(f"{what}: the last dimension of every plane must have stride 1")
    return F_, H, W


def planes_of(buf: torch.Tensor, fmt: str, H: int, W: int) -> Tuple[torch.Tensor, ...]:
    """plane views of a packed buffer with F leading and frame_samples(fmt, H, W) samples per frame: Y, then U, then V (or Y, then UV)"""
    chroma = fmt_info(fmt)[3]
    if chroma == 420:
        return yuv420.planes_of(buf, fmt, H, W)
    buf = _as_words(buf)
    if buf.dtype != fmt_dtype(fmt) or not _size_ok(chroma, H, W):
        raise ValueError(f"planes_of: {fmt} wants a {fmt_dtype(fmt)} buffer" + (" and an even W" if chroma == 422 else ""))
    F_, n = buf.shape[0], frame_samples(fmt, H, W)
    if buf.numel() != F_ * n or not buf.is_contiguous():
        raise ValueError(f"planes_of: want a contiguous buffer of {n} samples per frame")
    flat, out, at = buf.reshape(F_, n), [], 0
    for _, h, w in plane_shapes(fmt, F_, H, W):
        out.append(flat[:, at:at + h * w].view(F_, h, w))
        at += h * w
    return tuple(out)


def pack(planes: Sequence[torch.Tensor]) -> torch.Tensor:
    """contiguous [F, samples per frame] buffer holding the planes in order (the inverse of planes_of)"""
    return yuv420.pack(planes)


def to_rgb(planes: Sequence[torch.Tensor], fmt: str, matrix: str = "bt709", full_range: bool = False, dtype=torch.float32) -> torch.Tensor:
    """clip -> `dtype` RGB [F, 3, H, W], clamped to [0, 1]"""
    planar, depth, msb, chroma = fmt_info(fmt)
    if chroma == 420:
        return yuv420.to_rgb(planes, fmt, matrix, full_range, dtype)
    F_, H, W = check_clip(planes, fmt)
    sx, _ = SHIFTS[chroma]
    fwd, inv = color_affine(matrix, full_range, depth)
    m = torch.tensor(inv, dtype=dtype, device=planes[0].device)
    # the affine as A^-1 (code - offset), as yuv420.to_rgb: the offsets are subtracted exactly
    y = _codes(planes[0], depth, msb).to(dtype) - float(fwd[0, 3])
    if planar:
        c = torch.stack([_codes(planes[1], depth, msb), _codes(planes[2], depth, msb)], dim=-1).to(dtype)
    else:
        c = _codes(planes[1], depth, msb).reshape(F_, H, W // 2, 2).to(dtype)
    if sx:
        c = c.repeat_interleave(2, dim=2)
    cb, cr = c[..., 0] - float(fwd[1, 3]), c[..., 1] - float(fwd[2, 3])
    rgb = torch.stack([m[i, 0] * y + m[i, 1] * cb + m[i, 2] * cr for i in range(3)], dim=1)
    return rgb.clamp(0.0, 1.0)


def from_rgb(x01: torch.Tensor, fmt: str, matrix: str = "bt709", full_range: bool = False) -> Tuple[torch.Tensor, ...]:
    """RGB [F, 3, H, W] in [0, 1] (fp32 or float64) -> contiguous planes of `fmt`"""
    planar, depth, msb, chroma = fmt_info(fmt)
    if chroma == 420:
        return yuv420.from_rgb(x01, fmt, matrix, full_range)
    if x01.dim() != 4 or x01.shape[1] != 3 or not _size_ok(chroma, x01.shape[2], x01.shape[3]):
        raise ValueError("from_rgb wants [F, 3, H, W]" + (" with an even W" if chroma == 422 else ""))
    F_, _, H, W = x01.shape
    fwd, _ = color_affine(matrix, full_range, depth)
    m = torch.tensor(fwd, dtype=x01.dtype, device=x01.device)
    r, g, b = x01[:, 0], x01[:, 1], x01[:, 2]
    yuv = [m[i, 0] * r + m[i, 1] * g + m[i, 2] * b + m[i, 3] for i in range(3)]
    top = float((1 << depth) - 1)

    def words(v):
        return _words(torch.floor(v.clamp(0.0, top) + 0.5), depth, msb)
    if chroma == 444:
        return words(yuv[0]), words(yuv[1]), words(yuv[2])
    u, v = (c.reshape(F_, H, W // 2, 2).mean(dim=3) for c in (yuv[1], yuv[2]))
    if planar:
        return words(yuv[0]), words(u), words(v)
    return words(yuv[0]), words(torch.stack([u, v], dim=-1).reshape(F_, H, W))


class ClipYuv:
    """The planes of a 4:2:2 or 4:4:4 clip with the handful of tensor operations the model's chunk loop uses (slice by frames, move, copy),
    so that a clip walks `Videoseal._run_chunks` like a tensor does -- yuv420.Clip420 for the other chroma formats.  `color` = (matrix,
    full_range) travels with the clip."""

    def __init__(self, planes, fmt: str, color=DEFAULT_COLOR, buf: torch.Tensor = None):
        if is_420(fmt):
            raise ValueError("a 4:2:0 clip is a yuv420.Clip420 (yuv.clip makes the right one)")
        self.planes = tuple(_as_words(p) for p in planes)
        self.fmt, self.color, self.buf = fmt, (color[0], bool(color[1])), buf
        F_, H, W = self.planes[0].shape
        self.shape = (F_, H, W)

    dtype = property(lambda self: self.planes[0].dtype)
    device = property(lambda self: self.planes[0].device)
    graph_key = property(lambda self: (self.fmt, self.color))

    def dim(self) -> int:
        return 0            # (not a tensor: no frame layout of the tensor paths applies)

    def numel(self) -> int:
        return sum(p.numel() for p in self.planes)

    def __len__(self) -> int:
        return self.shape[0]

    def __getitem__(self, s) -> "ClipYuv":
        if not isinstance(s, slice):
            raise TypeError("a clip is sliced by frame ranges")
        return ClipYuv([p[s] for p in self.planes], self.fmt, self.color, self.buf[s] if self.buf is not None else None)

    def empty_like(self, device=None) -> "ClipYuv":
        """a new packed clip of the same format and size (the planes are views of one contiguous buffer, `buf`)"""
        F_, H, W = self.shape
        buf = torch.empty((F_, frame_samples(self.fmt, H, W)), dtype=self.dtype, device=self.device if device is None else device)
        return ClipYuv(planes_of(buf, self.fmt, H, W), self.fmt, self.color, buf)

    def contiguous(self) -> "ClipYuv":
        if self.buf is not None and self.buf.is_contiguous():
            return self
        return self.clone()

    def clone(self) -> "ClipYuv":
        return self.empty_like().copy_(self)

    def to(self, device) -> "ClipYuv":
        return ClipYuv([p.to(device) for p in self.planes], self.fmt, self.color)

    def copy_(self, other: "ClipYuv", non_blocking: bool = False) -> "ClipYuv":
        for d, s in zip(self.planes, other.planes):
            d.copy_(s, non_blocking=non_blocking)
        return self


def clip(planes, fmt: str, color=DEFAULT_COLOR):
    """the clip object of `planes`: yuv420.Clip420 for a 4:2:0 format, ClipYuv for the others"""
    return yuv420.Clip420(planes, fmt, color) if is_420(fmt) else ClipYuv(planes, fmt, color)
