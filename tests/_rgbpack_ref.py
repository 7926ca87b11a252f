"""Packed RGB formats in float64 numpy: the reference of tests/test_rgbpack_cpu.py and tests/test_gpu_rgbpack.py, written from the format
table alone and independent of videoseal_amd.rgbpack (a plain helper module, no pytest in it).

A clip is one array: uint8 [F, H, W, 3 | 4], uint16 [F, H, W, 3 | 4] or uint32 [F, H, W] (bits 31-30 X, then three 10-bit fields).
decode: code / top in float64.  encode: floor(clip(x, 0, 1) * top) in float64, alpha / X from `like` or all ones."""
import numpy as np

#        numpy dtype, components (0: one 10:10:10:2 word), depth, index (or bit shift) of R, G, B, index of alpha
FORMATS = {
    "rgb24": (np.uint8, 3, 8, (0, 1, 2), None), "bgr24": (np.uint8, 3, 8, (2, 1, 0), None),
    "rgba": (np.uint8, 4, 8, (0, 1, 2), 3), "bgra": (np.uint8, 4, 8, (2, 1, 0), 3),
    "argb": (np.uint8, 4, 8, (1, 2, 3), 0), "abgr": (np.uint8, 4, 8, (3, 2, 1), 0),
    "rgb48": (np.uint16, 3, 16, (0, 1, 2), None), "bgr48": (np.uint16, 3, 16, (2, 1, 0), None),
    "rgba64": (np.uint16, 4, 16, (0, 1, 2), 3), "bgra64": (np.uint16, 4, 16, (2, 1, 0), 3),
    "x2rgb10": (np.uint32, 0, 10, (20, 10, 0), None), "x2bgr10": (np.uint32, 0, 10, (0, 10, 20), None),
}
IDS = {name: i for i, name in enumerate(FORMATS)}            # VS_RGB_* in the order of the header's table
EIGHT = ("rgb24", "bgr24", "rgba", "bgra", "argb", "abgr")
LAYOUTS = ("rgb24", "bgra", "rgb48", "rgba64", "x2rgb10")      # one format per kernel instantiation


def top_of(fmt):
    return (1 << FORMATS[fmt][2]) - 1


def pixel_bytes(fmt):
    dt, comps, _, _, _ = FORMATS[fmt]
    return 4 if comps == 0 else comps * np.dtype(dt).itemsize


def codes_of(clip, fmt):
    """integer codes [F, H, W, 3] in R, G, B order"""
    _, comps, _, pos, _ = FORMATS[fmt]
    c = np.asarray(clip)
    if comps == 0:
        w = c.astype(np.uint32).astype(np.int64)
        return np.stack([(w >> p) & 0x3FF for p in pos], axis=-1)
    return np.stack([c[..., p].astype(np.int64) for p in pos], axis=-1)


def alpha_of(clip, fmt):
    """the bits that are not colour: the alpha component, the two X bits, or None"""
    _, comps, _, _, apos = FORMATS[fmt]
    if comps == 0:
        return np.asarray(clip).astype(np.uint32) >> 30
    return None if apos is None else np.asarray(clip)[..., apos]


def decode(clip, fmt):
    """float64 RGB [F, 3, H, W]"""
    return np.ascontiguousarray((codes_of(clip, fmt).astype(np.float64) / float(top_of(fmt))).transpose(0, 3, 1, 2))


def encode_values(x, fmt):
    """float64 code VALUES clip(x, 0, 1) * top, [F, H, W, 3] in R, G, B order (before the floor)"""
    return np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0).transpose(0, 2, 3, 1) * float(top_of(fmt))


def encode(x, fmt, like=None, alpha=None):
    """[F, 3, H, W] -> a clip of `fmt`; alpha / X: from `like` (a clip), else `alpha` (an array of alpha codes / X values), else all ones"""
    dt, comps, depth, pos, apos = FORMATS[fmt]
    c = np.floor(encode_values(x, fmt)).astype(np.int64)
    F_, H, W, _ = c.shape
    if like is not None:
        alpha = alpha_of(like, fmt)
    if comps == 0:
        xb = np.full((F_, H, W), 3, dtype=np.int64) if alpha is None else np.asarray(alpha).astype(np.int64)
        return ((xb << 30) | (c[..., 0] << pos[0]) | (c[..., 1] << pos[1]) | (c[..., 2] << pos[2])).astype(np.uint32)
    out = np.zeros((F_, H, W, comps), dtype=dt)
    for i, p in enumerate(pos):
        out[..., p] = c[..., i]
    if apos is not None:
        out[..., apos] = top_of(fmt) if alpha is None else alpha
    return out


def random_alpha(fmt, F_, H, W, seed=3):
    """random alpha codes (or X values) for a clip of that size; None for a format without either"""
    _, comps, depth, _, apos = FORMATS[fmt]
    rng = np.random.default_rng(seed)
    if comps == 0:
        return rng.integers(0, 4, size=(F_, H, W))
    return None if apos is None else rng.integers(0, 1 << depth, size=(F_, H, W))


def convert(clip, src, dst):
    """the same colour codes (and alpha, where both have one) in another layout of the same depth"""
    assert FORMATS[src][2] == FORMATS[dst][2]
    c = codes_of(clip, src)
    dt, comps, depth, pos, apos = FORMATS[dst]
    a = alpha_of(clip, src)
    F_, H, W, _ = c.shape
    if comps == 0:
        xb = np.full((F_, H, W), 3, dtype=np.int64) if a is None else a.astype(np.int64)
        return ((xb << 30) | (c[..., 0] << pos[0]) | (c[..., 1] << pos[1]) | (c[..., 2] << pos[2])).astype(np.uint32)
    out = np.zeros((F_, H, W, comps), dtype=dt)
    for i, p in enumerate(pos):
        out[..., p] = c[..., i]
    if apos is not None:
        out[..., apos] = top_of(dst) if a is None else a
    return out
