"""Packed RGB clips: the definitions of `Videoseal.embed_rgb` / `detect_rgb` as executable text (plain torch, any device).

Layout.  A clip is ONE tensor; `fmt` is ffmpeg's pix_fmt name without the "le" (everything is little-endian):
    fmt                                dtype             shape           memory order of a pixel
    "rgb24", "bgr24"                   uint8             [F, H, W, 3]    R G B / B G R
    "rgba", "bgra", "argb", "abgr"     uint8             [F, H, W, 4]    R G B A / B G R A / A R G B / A B G R
    "rgb48", "bgr48"                   uint16            [F, H, W, 3]    words R G B / B G R
    "rgba64", "bgra64"                 uint16            [F, H, W, 4]    words R G B A / B G R A
    "x2rgb10", "x2bgr10"               int32 or uint32   [F, H, W]       one word: bits 31-30 X, 29-20 R (B), 19-10 G, 9-0 B (R)
int16 is accepted as the same bits as uint16 (as yuv.py does), uint32 as the same bits as int32.  The innermost dimensions are compact
(component stride 1, pixel stride C); the row pitch `stride(1)` is any value >= the row, the frame stride any value that keeps frames
apart: a pitched capture surface is a strided view, not a copy.

Rules, with top = 2^depth - 1 and depth 8, 16 or 10:
    Decode   component = float32(code) / float32(top), the IEEE quotient: `clip.float() / 255.0` for depth 8.
    Encode   floor(clamp(x, 0, 1) * float32(top)): the truncation of `(x * 255).byte()` (inference_streaming.py:31) at every depth.
             floor((c / top) * top) == c in fp32 for every code of the three depths, so an unwatermarked pixel comes back unchanged.
    Alpha    the alpha component (the two X bits) of an output pixel is the source pixel's, bit for bit; it never enters arithmetic.
             RGB is straight, not premultiplied.  Without a source (`like=None`) alpha is opaque (all ones) and X is 3.
Not supported: big-endian words, premultiplied alpha, packed YUV.  Half-float RGB (float16 / bfloat16) has a module of its own: halfpix.py.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import yuv as _yuv

#           id (VS_RGB_*), depth, components per pixel (0: the 10:10:10:2 word), where R, G, B sit (component index, or bit shift), alpha index
FORMATS = {
    "rgb24": (0, 8, 3, (0, 1, 2), None), "bgr24": (1, 8, 3, (2, 1, 0), None),
    "rgba": (2, 8, 4, (0, 1, 2), 3), "bgra": (3, 8, 4, (2, 1, 0), 3), "argb": (4, 8, 4, (1, 2, 3), 0), "abgr": (5, 8, 4, (3, 2, 1), 0),
    "rgb48": (6, 16, 3, (0, 1, 2), None), "bgr48": (7, 16, 3, (2, 1, 0), None),
    "rgba64": (8, 16, 4, (0, 1, 2), 3), "bgra64": (9, 16, 4, (2, 1, 0), 3),
    "x2rgb10": (10, 10, 0, (20, 10, 0), None), "x2bgr10": (11, 10, 0, (0, 10, 20), None),
}


def fmt_info(fmt: str) -> Tuple[int, int, int, Tuple[int, int, int], Optional[int]]:
    """(id, depth, components, (r, g, b) positions, alpha position) of `fmt`; ValueError for an unknown one"""
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    return FORMATS[fmt]


def fmt_dtype(fmt: str) -> torch.dtype:
    depth = fmt_info(fmt)[1]
    return {8: torch.uint8, 16: torch.uint16, 10: torch.int32}[depth]


def pixel_bytes(fmt: str) -> int:
    _, depth, comps, _, _ = fmt_info(fmt)
    return 4 if comps == 0 else comps * (depth // 8)


def _as_words(t: torch.Tensor) -> torch.Tensor:
    """int16 -> the same bits as uint16, uint32 -> the same bits as int32"""
    if torch.is_tensor(t) and t.dtype == torch.int16:
        return t.view(torch.uint16)
    if torch.is_tensor(t) and t.dtype == torch.uint32:
        return t.view(torch.int32)
    return t


def check_clip(clip: torch.Tensor, fmt: str, what: str = "clip") -> Tuple[int, int, int]:
    """(F, H, W) of a valid clip; ValueError with the reason otherwise"""
    _, depth, comps, _, _ = fmt_info(fmt)
    if not torch.is_tensor(clip):
        raise ValueError(f"{what}: {fmt} wants one tensor")
    clip = _as_words(clip)
    want = fmt_dtype(fmt)
    if clip.dtype != want:
        raise ValueError(f"{what}: a {fmt} clip is a {want} tensor, got {clip.dtype}")
    shape = "[F, H, W]" if comps == 0 else f"[F, H, W, {comps}]"
    if clip.dim() != (3 if comps == 0 else 4) or (comps and clip.shape[-1] != comps):
        raise ValueError(f"{what}: a {fmt} clip has shape {shape}, got {tuple(clip.shape)}")
    F_, H, W = clip.shape[:3]
    if H < 1 or W < 1:
        raise ValueError(f"{what}: a {fmt} clip needs H, W >= 1 (got {H} x {W})")
    if clip.numel() > 0:
        row = W * max(comps, 1)
        if (comps and clip.stride(3) != 1) or (W > 1 and clip.stride(2) != max(comps, 1)):
            raise ValueError(f"{what}: the pixels of a row must be compact (component stride 1, pixel stride {max(comps, 1)})")
        if H > 1 and clip.stride(1) < row:
            raise ValueError(f"{what}: the row pitch ({clip.stride(1)}) is shorter than a row ({row} elements)")
        if F_ > 1 and clip.stride(0) < (clip.stride(1) * (H - 1) if H > 1 else 0) + row:
            raise ValueError(f"{what}: frames overlap (frame stride {clip.stride(0)})")
    return F_, H, W


def _codes(clip: torch.Tensor, fmt: str):
    """stored words -> (int32 codes [F, H, W, 3] in R, G, B order, the words as int32 [F, H, W, C] or [F, H, W])"""
    _, depth, comps, pos, _ = fmt_info(fmt)
    clip = _as_words(clip)
    if comps == 0:
        w = clip.to(torch.int32)
        return torch.stack([(w >> p) & 0x3FF for p in pos], dim=-1), w
    w = clip.to(torch.int32) if depth == 8 else (clip.view(torch.int16).to(torch.int32) & 0xFFFF)
    return torch.stack([w[..., p] for p in pos], dim=-1), w


def to_rgb(clip: torch.Tensor, fmt: str, dtype=torch.float32) -> torch.Tensor:
    """clip -> `dtype` RGB [F, 3, H, W] in [0, 1]: code / top"""
    _, depth, _, _, _ = fmt_info(fmt)
    check_clip(clip, fmt, "to_rgb")
    codes, _ = _codes(clip, fmt)
    top = torch.tensor(float((1 << depth) - 1), dtype=dtype, device=clip.device)
    return (codes.to(dtype) / top).permute(0, 3, 1, 2).contiguous()


def from_rgb(x01: torch.Tensor, fmt: str, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RGB [F, 3, H, W] (fp32 or float64) -> a contiguous clip of `fmt`: floor(clamp(x, 0, 1) * top); alpha / X from `like` (a clip of the
    same format and size), opaque without it"""
    _, depth, comps, pos, apos = fmt_info(fmt)
    if x01.dim() != 4 or x01.shape[1] != 3:
        raise ValueError("from_rgb wants [F, 3, H, W]")
    F_, _, H, W = x01.shape
    top = (1 << depth) - 1
    c = torch.floor(x01.clamp(0.0, 1.0) * torch.tensor(float(top), dtype=x01.dtype, device=x01.device)).to(torch.int32)      # [F, 3, H, W]
    if like is not None:
        if tuple(check_clip(like, fmt, "from_rgb: like")) != (F_, H, W):
            raise ValueError(f"from_rgb: `like` is {tuple(like.shape)} for frames {tuple(x01.shape)}")
        _, lw = _codes(like.to(x01.device), fmt)
    if comps == 0:
        keep = (lw & ~((0x3FF << pos[0]) | (0x3FF << pos[1]) | (0x3FF << pos[2]))) if like is not None else torch.full((F_, H, W), -(1 << 30), dtype=torch.int32, device=x01.device)
        return (keep | (c[:, 0] << pos[0]) | (c[:, 1] << pos[1]) | (c[:, 2] << pos[2])).contiguous()
    w = torch.empty((F_, H, W, comps), dtype=torch.int32, device=x01.device)
    for i, p in enumerate(pos):
        w[..., p] = c[:, i]
    if apos is not None:
        w[..., apos] = lw[..., apos] if like is not None else top
    if depth == 8:
        return w.to(torch.uint8)
    w = torch.where(w >= 32768, w - 65536, w)          # the same 16 bits as a signed value
    return w.to(torch.int16).view(torch.uint16)


class Clip(_yuv.Clip):
    """A packed RGB clip as the clip object `Videoseal._run_chunks` and the graph cache walk: yuv.Clip with ONE plane -- the tensor itself --
    and nothing but the format in its graph key.  Slicing by frames, `to`, `copy_`, `clone` and `contiguous` are yuv.Clip's; a new clip
    (`empty_like`) is a compact tensor of the same shape."""

    def __init__(self, clip: torch.Tensor, fmt: str, buf: torch.Tensor = None):
        fmt_info(fmt)
        t = _as_words(clip)
        self.planes = (t,)
        self.fmt, self.color, self.buf = fmt, None, buf
        self.shape = tuple(t.shape[:3])

    tensor = property(lambda self: self.planes[0])
    graph_key = property(lambda self: (self.fmt,))

    def __getitem__(self, s) -> "Clip":
        if not isinstance(s, slice):
            raise TypeError("a clip is sliced by frame ranges")
        return Clip(self.planes[0][s], self.fmt, self.buf[s] if self.buf is not None else None)

    def empty_like(self, device=None) -> "Clip":
        t = self.planes[0]
        buf = torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device if device is None else device)
        return Clip(buf, self.fmt, buf)

    def to(self, device) -> "Clip":
        return Clip(self.planes[0].to(device), self.fmt)


def clip(t: torch.Tensor, fmt: str) -> Clip:
    """the clip object of a checked tensor; ValueError for an unknown `fmt` or a tensor that is no clip of it"""
    check_clip(t, fmt)
    return Clip(t, fmt)
