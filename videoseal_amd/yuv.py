"""YUV clips of every supported chroma format: the definitions of `Videoseal.embed_yuv` / `detect_yuv` (and of `embed_yuv420`, `embed_nv12`
and their detectors) as executable text (plain torch, any device).  yuv420.py and nv12.py are restrictions of this module to their formats.

Layout.  A clip is a tuple of plane tensors on one device; `fmt` is ffmpeg's pix_fmt name without the "le":
    fmt          dtype    planes                                            chroma
    "nv12"       uint8    (y [F, H, W], uv [F, H/2, W])                     4:2:0   uv[..., 2j], uv[..., 2j+1] = Cb, Cr of block j of the row
    "i420"       uint8    (y [F, H, W], u [F, H/2, W/2], v [F, H/2, W/2])   4:2:0
    "p010"       uint16   as nv12; sample code = word >> 6                  4:2:0   (the low 6 bits are ignored on input and zero on output)
    "yuv420p10"  uint16   as i420; sample code = min(word, 1023)            4:2:0
    "yuv422p"    uint8    (y [F, H, W], u [F, H, W/2], v [F, H, W/2])       4:2:2
    "yuv422p10"  uint16   as yuv422p; sample code = min(word, 1023)         4:2:2
    "nv16"       uint8    (y [F, H, W], uv [F, H, W])                       4:2:2   as nv12, one chroma row per luma row
    "p210"       uint16   as nv16; sample code = word >> 6                  4:2:2
    "yuv444p"    uint8    (y, u, v), each [F, H, W]                         4:4:4
    "yuv444p10"  uint16   as yuv444p; sample code = min(word, 1023)         4:4:4
The size rule comes from the format (`SHIFTS`): 4:2:0 needs H and W even, 4:2:2 needs W even and takes any H >= 1, 4:4:4 takes any H, W >= 1.
Every plane has last stride 1 and its own row pitch (>= the row) and frame stride: `AVFrame.data[i]` / `linesize[i]` map to strided views,
not copies.  int16 tensors are accepted as the same bits as uint16.  `planes_of` cuts the planes out of a packed per-frame buffer (Y, then
U, then V -- or Y, then UV: the byte order of ffmpeg's `rawvideo`; 3HW/2 samples per frame for 4:2:0, 2HW for 4:2:2, 3HW for 4:4:4) and
`pack` is its inverse.

Colour.  `matrix` is "bt601" (Kr, Kb = 0.299, 0.114), "bt709" (0.2126, 0.0722) or "bt2020" (0.2627, 0.0593), Kg = 1 - Kr - Kb:
    Y = Kr R + Kg G + Kb B,   Cb = (B - Y) / (2 (1 - Kb)),   Cr = (R - Y) / (2 (1 - Kr))
Codes at depth 8: limited range Y -> 16 + 219 Y, C -> 128 + 224 C; full range Y -> 255 Y, C -> 128 + 255 C.
Codes at depth 10: limited range Y -> 64 + 876 Y, C -> 512 + 896 C; full range Y -> 1023 Y, C -> 512 + 1023 C.
`color_affine` builds the forward 3 x 4 affine (RGB in [0, 1] -> code units) in float64 and inverts it in float64.

Chroma.  A block is 2 x 2 pixels (4:2:0), 2 x 1 (4:2:2: two neighbours of one row) or 1 x 1 (4:4:4).  Up: every pixel of a block uses the
block's (Cb, Cr).  Down: the mean of the block's per-pixel chroma values (four, two, or the value itself), then one rounding.
Range and rounding.  After decoding every RGB channel is clamped to [0, 1]; output codes are floor(clamp(v, 0, 2^depth - 1) + 0.5), v in code
units (p010 and p210 store code << 6) -- one rounding, no intermediate RGB24.
Not supported: packed formats (yuyv422, uyvy422, v210), semi-planar 4:4:4 (nv24, p410), depth 12, any other chroma siting.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
DEFAULT_COLOR = ("bt709", False)
#            planar, depth, msb_aligned, chroma
FORMATS = {"nv12": (False, 8, False, 420), "i420": (True, 8, False, 420), "p010": (False, 10, True, 420), "yuv420p10": (True, 10, False, 420),
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


def _size_rule(chroma: int) -> str:
    return {420: "even H and W", 422: "an even W", 444: "any H and W"}[chroma]


def color_affine(matrix: str = "bt709", full_range: bool = False, depth: int = 8) -> Tuple[np.ndarray, np.ndarray]:
    """(rgb2yuv, yuv2rgb): two float64 [3, 4] arrays.  rgb2yuv maps (R, G, B, 1) in [0, 1] to (Y, Cb, Cr) in code units of `depth`, yuv2rgb is
    its inverse (codes -> RGB in [0, 1], before the clamp)."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    if depth not in (8, 10):
        raise ValueError(f"depth must be 8 or 10, got {depth!r}")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y = np.array([kr, kg, kb], dtype=np.float64)
    cb = (np.array([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - kb))
    cr = (np.array([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - kr))
    if depth == 8:
        ys, cs, y0, c0 = (255.0, 255.0, 0.0, 128.0) if full_range else (219.0, 224.0, 16.0, 128.0)
    else:
        ys, cs, y0, c0 = (1023.0, 1023.0, 0.0, 512.0) if full_range else (876.0, 896.0, 64.0, 512.0)
    fwd = np.zeros((3, 4), dtype=np.float64)
    fwd[0, :3], fwd[0, 3] = ys * y, y0
    fwd[1, :3], fwd[1, 3] = cs * cb, c0
    fwd[2, :3], fwd[2, 3] = cs * cr, c0
    # inverse by cofactors, every product and sum in float64 and in this order: csrc/model_api.hip states the same expressions for
    # vs_yuv420_default_color, and tests/test_yuv420_cpu.py and tests/test_nv12_cpu.py hold them to the same bits
    a = [[float(fwd[i, j]) for j in range(3)] for i in range(3)]
    cof = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3]
            for j in range(3)] for i in range(3)]
    det = a[0][0] * cof[0][0] + a[0][1] * cof[0][1] + a[0][2] * cof[0][2]
    inv = np.zeros((3, 4), dtype=np.float64)
    for i in range(3):
        for j in range(3):
            inv[i, j] = cof[j][i] / det
        inv[i, 3] = -(inv[i, 0] * float(fwd[0, 3]) + inv[i, 1] * float(fwd[1, 3]) + inv[i, 2] * float(fwd[2, 3]))
    return fwd, inv


def _as_words(p: torch.Tensor) -> torch.Tensor:
    return p.view(torch.uint16) if torch.is_tensor(p) and p.dtype == torch.int16 else p


def check_clip(planes: Sequence[torch.Tensor], fmt: str, what: str = "clip") -> Tuple[int, int, int]:
    """(F, H, W) of a valid clip; ValueError otherwise"""
    planar, depth, _, chroma = fmt_info(fmt)
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
        raise ValueError(f"{what}: a {fmt} clip needs {_size_rule(chroma)} (got {H} x {W})")
    want_shapes = plane_shapes(fmt, F_, H, W)
    if any(tuple(p.shape) != s for p, s in zip(planes, want_shapes)):
        raise ValueError(f"{what}: a {fmt} clip with luma {tuple(planes[0].shape)} has chroma planes {want_shapes[1]}, got {[tuple(p.shape) for p in planes[1:]]}")
    if any(p.numel() > 0 and p.stride(2) != 1 for p in planes):
        raise ValueError(f"{what}: the last dimension of every plane must have stride 1")
    return F_, H, W


def planes_of(buf: torch.Tensor, fmt: str, H: int, W: int) -> Tuple[torch.Tensor, ...]:
    """plane views of a packed buffer with F leading and frame_samples(fmt, H, W) samples per frame: Y, then U, then V (or Y, then UV)"""
    chroma = fmt_info(fmt)[3]
    buf = _as_words(buf)
    if buf.dtype != fmt_dtype(fmt) or not _size_ok(chroma, H, W):
        raise ValueError(f"planes_of: {fmt} wants a {fmt_dtype(fmt)} buffer and {_size_rule(chroma)}")
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
    planes = [_as_words(p) for p in planes]
    return torch.cat([p.reshape(p.shape[0], -1) for p in planes], dim=1).contiguous()


def _codes(p: torch.Tensor, depth: int, msb: bool) -> torch.Tensor:
    """stored words -> int32 sample codes"""
    if depth == 8:
        return p.to(torch.int32)
    w = _as_words(p).view(torch.int16).to(torch.int32) & 0xFFFF
    return (w >> 6) if msb else w.clamp(max=1023)


def _words(code: torch.Tensor, depth: int, msb: bool) -> torch.Tensor:
    """integer-valued float codes -> stored words"""
    if depth == 8:
        return code.to(torch.uint8)
    w = code.to(torch.int32)
    if msb:
        w = w << 6
    w = torch.where(w >= 32768, w - 65536, w)          # the same 16 bits as a signed value
    return w.to(torch.int16).view(torch.uint16)


def to_rgb(planes: Sequence[torch.Tensor], fmt: str, matrix: str = "bt709", full_range: bool = False, dtype=torch.float32) -> torch.Tensor:
    """clip -> `dtype` RGB [F, 3, H, W], clamped to [0, 1]"""
    planar, depth, msb, chroma = fmt_info(fmt)
    F_, H, W = check_clip(planes, fmt)
    sx, sy = SHIFTS[chroma]
    fwd, inv = color_affine(matrix, full_range, depth)
    m = torch.tensor(inv, dtype=dtype, device=planes[0].device)
    # the affine as A^-1 (code - offset): the offsets are subtracted exactly, so no large constant is cancelled in fp32
    y = _codes(planes[0], depth, msb).to(dtype) - float(fwd[0, 3])
    if planar:
        c = torch.stack([_codes(planes[1], depth, msb), _codes(planes[2], depth, msb)], dim=-1).to(dtype)
    else:
        c = _codes(planes[1], depth, msb).reshape(F_, H >> sy, W >> 1, 2).to(dtype)
    if sy:
        c = c.repeat_interleave(2, dim=1)
    if sx:
        c = c.repeat_interleave(2, dim=2)
    cb, cr = c[..., 0] - float(fwd[1, 3]), c[..., 1] - float(fwd[2, 3])
    rgb = torch.stack([m[i, 0] * y + m[i, 1] * cb + m[i, 2] * cr for i in range(3)], dim=1)
    return rgb.clamp(0.0, 1.0)


def from_rgb(x01: torch.Tensor, fmt: str, matrix: str = "bt709", full_range: bool = False) -> Tuple[torch.Tensor, ...]:
    """RGB [F, 3, H, W] in [0, 1] (fp32 or float64) -> contiguous planes of `fmt`"""
    planar, depth, msb, chroma = fmt_info(fmt)
    if x01.dim() != 4 or x01.shape[1] != 3 or not _size_ok(chroma, x01.shape[2], x01.shape[3]):
        raise ValueError(f"from_rgb wants [F, 3, H, W], for {fmt} with {_size_rule(chroma)}")
    F_, _, H, W = x01.shape
    sx, sy = SHIFTS[chroma]
    fwd, _ = color_affine(matrix, full_range, depth)
    m = torch.tensor(fwd, dtype=x01.dtype, device=x01.device)
    r, g, b = x01[:, 0], x01[:, 1], x01[:, 2]
    yuv = [m[i, 0] * r + m[i, 1] * g + m[i, 2] * b + m[i, 3] for i in range(3)]
    top = float((1 << depth) - 1)

    def words(v):
        return _words(torch.floor(v.clamp(0.0, top) + 0.5), depth, msb)

    def down(c):            # [F, H, W, ...] -> the mean of every block [F, H >> sy, W >> sx, ...]
        return c.reshape(F_, H >> sy, 1 << sy, W >> sx, 1 << sx, *c.shape[3:]).mean(dim=(2, 4))
    if planar:
        return words(yuv[0]), words(down(yuv[1])), words(down(yuv[2]))
    # semi-planar (sx = 1): Cb and Cr are interleaved before the mean, so a row of the result is the row of the plane
    return words(yuv[0]), words(down(torch.stack([yuv[1], yuv[2]], dim=-1)).reshape(F_, H >> sy, W))


class Clip:
    """The planes of a clip with the handful of tensor operations the model's chunk loop uses (slice by frames, move, copy), so that a clip
    walks `Videoseal._run_chunks` like a tensor does.  `color` = (matrix, full_range) travels with the clip."""

    def __init__(self, planes, fmt: str, color=DEFAULT_COLOR, buf: torch.Tensor = None):
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

    def __getitem__(self, s) -> "Clip":
        if not isinstance(s, slice):
            raise TypeError("a clip is sliced by frame ranges")
        return Clip([p[s] for p in self.planes], self.fmt, self.color, self.buf[s] if self.buf is not None else None)

    def empty_like(self, device=None) -> "Clip":
        """a new packed clip of the same format and size (the planes are views of one contiguous buffer, `buf`)"""
        F_, H, W = self.shape
        buf = torch.empty((F_, frame_samples(self.fmt, H, W)), dtype=self.dtype, device=self.device if device is None else device)
        return Clip(planes_of(buf, self.fmt, H, W), self.fmt, self.color, buf)

    def contiguous(self) -> "Clip":
        if self.buf is not None and self.buf.is_contiguous():
            return self
        return self.clone()

    def clone(self) -> "Clip":
        return self.empty_like().copy_(self)

    def to(self, device) -> "Clip":
        return Clip([p.to(device) for p in self.planes], self.fmt, self.color)

    def copy_(self, other: "Clip", non_blocking: bool = False) -> "Clip":
        for d, s in zip(self.planes, other.planes):
            d.copy_(s, non_blocking=non_blocking)
        return self


ClipYuv = Clip            # (the name the 4:2:2 / 4:4:4 callers use; yuv420.Clip420 is the same class)


def clip(planes, fmt: str, color=DEFAULT_COLOR) -> Clip:
    """the clip object of `planes`; ValueError for an unknown `fmt`"""
    fmt_info(fmt)
    return Clip(planes, fmt, color)
