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
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
DEFAULT_COLOR = ("bt709", False)


def color_affine(matrix: str = "bt709", full_range: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(rgb2yuv, yuv2rgb): two float64 [3, 4] arrays.  rgb2yuv maps (R, G, B, 1) in [0, 1] to (Y, Cb, Cr) in code units, yuv2rgb is its
    inverse (codes -> RGB in [0, 1], before the clamp)."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y = np.array([kr, kg, kb], dtype=np.float64)
    cb = (np.array([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - kb))
    cr = (np.array([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - kr))
    ys, cs, y0 = (255.0, 255.0, 0.0) if full_range else (219.0, 224.0, 16.0)
    fwd = np.zeros((3, 4), dtype=np.float64)
    fwd[0, :3], fwd[0, 3] = ys * y, y0
    fwd[1, :3], fwd[1, 3] = cs * cb, 128.0
    fwd[2, :3], fwd[2, 3] = cs * cr, 128.0
    # inverse by cofactors, every product and sum in float64 and in this order: csrc/model_api.hip states the same expressions for the
    # model-level C-ABI's default, and tests/test_nv12_cpu.py holds the two to the same bits
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


def nv12_to_rgb(clip: torch.Tensor, matrix: str = "bt709", full_range: bool = False, dtype=torch.float32) -> torch.Tensor:
    """uint8 [F, 3H/2, W] -> `dtype` RGB [F, 3, H, W], clamped to [0, 1]"""
    F_, H, W = check_clip(clip)
    fwd, inv = color_affine(matrix, full_range)
    m = torch.tensor(inv, dtype=dtype, device=clip.device)
    # the affine as A^-1 (code - offset): the offsets (16 or 0, 128, 128) are subtracted exactly, so no large constant is cancelled in fp32
    y = clip[:, :H, :].to(dtype) - float(fwd[0, 3])
    c = clip[:, H:, :].reshape(F_, H // 2, W // 2, 2).to(dtype)
    c = c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    cb, cr = c[..., 0] - float(fwd[1, 3]), c[..., 1] - float(fwd[2, 3])
    rgb = torch.stack([m[i, 0] * y + m[i, 1] * cb + m[i, 2] * cr for i in range(3)], dim=1)
    return rgb.clamp(0.0, 1.0)


def rgb_to_nv12(x01: torch.Tensor, matrix: str = "bt709", full_range: bool = False) -> torch.Tensor:
    """RGB [F, 3, H, W] in [0, 1] (fp32 or float64) -> contiguous uint8 [F, 3H/2, W]"""
    if x01.dim() != 4 or x01.shape[1] != 3 or x01.shape[2] % 2 or x01.shape[3] % 2:
        raise ValueError("rgb_to_nv12 wants [F, 3, H, W] with even H and W")
    F_, _, H, W = x01.shape
    fwd, _ = color_affine(matrix, full_range)
    m = torch.tensor(fwd, dtype=x01.dtype, device=x01.device)
    r, g, b = x01[:, 0], x01[:, 1], x01[:, 2]
    yuv = [m[i, 0] * r + m[i, 1] * g + m[i, 2] * b + m[i, 3] for i in range(3)]
    cbcr = torch.stack([yuv[1], yuv[2]], dim=-1)                                       # [F, H, W, 2]
    cbcr = cbcr.reshape(F_, H // 2, 2, W // 2, 2, 2).mean(dim=(2, 4)).reshape(F_, H // 2, W)
    v = torch.cat([yuv[0], cbcr], dim=1)
    return torch.floor(v.clamp(0.0, 255.0) + 0.5).to(torch.uint8)
