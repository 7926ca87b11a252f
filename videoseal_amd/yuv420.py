"""4:2:0 clips: the definitions of `Videoseal.embed_yuv420` / `detect_yuv420`.  The text lives in yuv.py (layout, colour, chroma, rounding,
the arithmetic and the clip class); this module is its restriction to the four 4:2:0 formats "nv12", "i420", "p010" and "yuv420p10" (H and
W even, 3HW/2 samples per packed frame), under the names and signatures the 4:2:0 callers use.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import yuv
from .yuv import DEFAULT_COLOR, MATRICES, _as_words, _codes, _words, color_affine  # noqa: F401  (re-exported: one colour definition)

#            planar, depth, msb_aligned
FORMATS = {k: v[:3] for k, v in yuv.FORMATS.items() if v[3] == 420}
Clip420 = yuv.Clip


def fmt_info(fmt: str) -> Tuple[bool, int, bool]:
    """(planar, depth, msb_aligned) of `fmt`; ValueError for an unknown one"""
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    return FORMATS[fmt]


def fmt_dtype(fmt: str) -> torch.dtype:
    fmt_info(fmt)
    return yuv.fmt_dtype(fmt)


def check_clip(planes: Sequence[torch.Tensor], fmt: str, what: str = "4:2:0 clip") -> Tuple[int, int, int]:
    """(F, H, W) of a valid clip; ValueError otherwise"""
    fmt_info(fmt)
    return yuv.check_clip(planes, fmt, what)


def planes_of(buf: torch.Tensor, fmt: str, H: int, W: int) -> Tuple[torch.Tensor, ...]:
    """plane views of a packed buffer [F, 3HW/2] (or any shape with F leading and 3HW/2 samples per frame): Y, then U, then V (or Y, then UV)"""
    fmt_info(fmt)
    return yuv.planes_of(buf, fmt, H, W)


def pack(planes: Sequence[torch.Tensor]) -> torch.Tensor:
    """contiguous [F, 3HW/2] buffer holding the planes in order (the inverse of planes_of)"""
    return yuv.pack(planes)


def to_rgb(planes: Sequence[torch.Tensor], fmt: str, matrix: str = "bt709", full_range: bool = False, dtype=torch.float32) -> torch.Tensor:
    """clip -> `dtype` RGB [F, 3, H, W], clamped to [0, 1]"""
    fmt_info(fmt)
    return yuv.to_rgb(planes, fmt, matrix, full_range, dtype)


def from_rgb(x01: torch.Tensor, fmt: str, matrix: str = "bt709", full_range: bool = False) -> Tuple[torch.Tensor, ...]:
    """RGB [F, 3, H, W] in [0, 1] (fp32 or float64) -> contiguous planes of `fmt`"""
    fmt_info(fmt)
    return yuv.from_rgb(x01, fmt, matrix, full_range)
