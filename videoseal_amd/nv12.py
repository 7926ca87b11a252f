"""NV12 frames: the definitions of `Videoseal.embed_nv12` / `detect_nv12` as executable text (plain torch, any device).

Layout.  A clip is uint8 [F, 3H/2, W] with H and W even.  Rows 0 .. H-1 of a frame are luma; rows H .. 3H/2-1 are the chroma plane:
bytes 2j and 2j+1 of chroma row i are Cb and Cr of the 2 x 2 pixel block (2i .. 2i+1, 2j .. 2j+1).  The last dimension has stride 1, the
row stride (pitch) may be any value >= W and the frame stride any value >= pitch * 3H/2: a pitched decoder surface is a strided view.

Colour.  `matrix` is "bt601" (Kr, Kb = 0.299, 0.114) or "bt709" (0.2126, 0.0722), Kg = 1 - Kr - Kb:
    Y = Kr R + Kg G + Kb B,   Cb = (B - Y) / (2 (1 - Kb)),   Cr = (R - Y) / (2 (1 - Kr))
Limited range codes: Y -> 16 + 219 Y, C -> 128 + 224 C; full range codes: Y -> 255 Y, C -> 128 + 255 C.  `color_affine` builds the forward
3 x 4 affine (RGB in [0, 1] -> code units) in float64 and inverts it in float64.

Chroma.  Up: every pixel of a 2 x 2 block uses that block's (Cb, Cr).  Down: the mean of the four per-pixel chroma values, then one rounding.
Range and rounding.  After NV12 -> RGB every channel is clamped to [0, 1]; output codes are floor(clamp(v, 0, 255) + 0.5), v in code units.

The arithmetic is yuv.py's for fmt "nv12" (depth 8) on the planes `clip[:, :H]` and `clip[:, H:]`; this module holds the single-buffer
layout and the two matrices of the NV12 entry points.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import yuv

MATRICES = {k: yuv.MATRICES[k] for k in ("bt601", "bt709")}
DEFAULT_COLOR = yuv.DEFAULT_COLOR


def _known(matrix: str) -> str:
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    return matrix


def color_affine(matrix: str = "bt709", full_range: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(rgb2yuv, yuv2rgb): two float64 [3, 4] arrays.  rgb2yuv maps (R, G, B, 1) in [0, 1] to (Y, Cb, Cr) in code units, yuv2rgb is its
    inverse (codes -> RGB in [0, 1], before the clamp)."""
    return yuv.color_affine(_known(matrix), full_range, 8)


def check_clip(clip: torch.Tensor, what: str = "NV12 clip") -> Tuple[int, int, int]:
    """(F, H, W) of a valid NV12 clip; ValueError otherwise"""
    if not torch.is_tensor(clip) or clip.dtype != torch.uint8 or clip.dim() != 3:
        raise ValueError(f"{what}: want a uint8 tensor [F, 3H/2, W]")
    F_, R, W = clip.shape
    if R % 3 or W % 2:            # (H = 2R/3: an odd H has no whole number of chroma rows)
        raise ValueError(f"{what}: H and W must be even (got {R} rows = 3H/2, W = {W})")
    if W > 0 and R > 0 and clip.stride(2) != 1:
        raise ValueError(f"{what}: the last dimension must have stride 1")
    return F_, R // 3 * 2, W


def planes(clip: torch.Tensor, what: str = "NV12 clip") -> Tuple[torch.Tensor, torch.Tensor]:
    """(y [F, H, W], uv [F, H/2, W]): the planes of a valid NV12 clip as views of it"""
    _, H, _ = check_clip(clip, what)
    return clip[:, :H], clip[:, H:]


def nv12_to_rgb(clip: torch.Tensor, matrix: str = "bt709", full_range: bool = False, dtype=torch.float32) -> torch.Tensor:
    """uint8 [F, 3H/2, W] -> `dtype` RGB [F, 3, H, W], clamped to [0, 1]"""
    return yuv.to_rgb(planes(clip), "nv12", _known(matrix), full_range, dtype)


def rgb_to_nv12(x01: torch.Tensor, matrix: str = "bt709", full_range: bool = False) -> torch.Tensor:
    """RGB [F, 3, H, W] in [0, 1] (fp32 or float64) -> contiguous uint8 [F, 3H/2, W]"""
    return torch.cat(yuv.from_rgb(x01, "nv12", _known(matrix), full_range), dim=1)
