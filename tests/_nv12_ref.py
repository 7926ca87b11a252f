"""Independent float64 restatement of the NV12 definitions (numpy only; does not import videoseal_amd.nv12).

Clip: uint8 [F, 3H/2, W]; rows 0..H-1 luma, rows H..3H/2-1 interleaved CbCr of the 2 x 2 blocks.  Kr/Kb = 0.299/0.114 (bt601) or
0.2126/0.0722 (bt709); limited range Y -> 16 + 219 Y, C -> 128 + 224 C; full range Y -> 255 Y, C -> 128 + 255 C.  Chroma up: block value for
all four pixels; chroma down: mean of the four per-pixel values; RGB clamped to [0, 1] after decoding; codes = floor(clamp(v, 0, 255) + 0.5)."""
import numpy as np

PRESETS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
_K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def _scales(full_range):
    return (255.0, 255.0, 0.0) if full_range else (219.0, 224.0, 16.0)


def decode(clip, matrix="bt709", full_range=False, clamp=True):
    """uint8 [F, 3H/2, W] (numpy) -> float64 RGB [F, 3, H, W]; written from the inverse formulas, not from a matrix inverse"""
    clip = np.asarray(clip)
    F, R, W = clip.shape
    H = R // 3 * 2
    kr, kb = _K[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0 = _scales(full_range)
    y = (clip[:, :H].astype(np.float64) - y0) / ys
    ch = clip[:, H:].astype(np.float64).reshape(F, H // 2, W // 2, 2)
    ch = np.repeat(np.repeat(ch, 2, axis=1), 2, axis=2)
    cb = (ch[..., 0] - 128.0) / cs
    cr = (ch[..., 1] - 128.0) / cs
    r = y + 2.0 * (1.0 - kr) * cr
    b = y + 2.0 * (1.0 - kb) * cb
    g = (y - kr * r - kb * b) / kg
    rgb = np.stack([r, g, b], axis=1)
    return np.clip(rgb, 0.0, 1.0) if clamp else rgb


def encode_values(rgb, matrix="bt709", full_range=False):
    """float RGB [F, 3, H, W] -> float64 code values [F, 3H/2, W] BEFORE rounding (chroma after the 2 x 2 mean)"""
    rgb = np.asarray(rgb, dtype=np.float64)
    F, _, H, W = rgb.shape
    kr, kb = _K[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0 = _scales(full_range)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    y = kr * r + kg * g + kb * b
    cb = (b - y) / (2.0 * (1.0 - kb))
    cr = (r - y) / (2.0 * (1.0 - kr))
    c = np.stack([128.0 + cs * cb, 128.0 + cs * cr], axis=-1)                      # [F, H, W, 2]
    c = c.reshape(F, H // 2, 2, W // 2, 2, 2).mean(axis=(2, 4)).reshape(F, H // 2, W)
    return np.concatenate([y0 + ys * y, c], axis=1)


def round_codes(v):
    return np.floor(np.clip(v, 0.0, 255.0) + 0.5).astype(np.uint8)


def encode(rgb, matrix="bt709", full_range=False):
    return round_codes(encode_values(rgb, matrix, full_range))
