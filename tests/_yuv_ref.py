"""Independent float64 restatement of the YUV definitions for every chroma format (numpy only; imports neither videoseal_amd.yuv nor
videoseal_amd.yuv420), by depth, layout and chroma subsampling.

A clip is a tuple of numpy planes.  fmt -> (planar, depth, msb_aligned, sx, sy): a chroma sample serves (1 << sx) x (1 << sy) pixels.
Interleaved layouts hold Cb, Cr of block j of a chroma row at samples 2j, 2j+1; depth 10 words: code = word >> 6 (msb) or min(word, 1023).
Kr/Kb = 0.299/0.114 (bt601), 0.2126/0.0722 (bt709), 0.2627/0.0593 (bt2020).  Depth 8: limited Y -> 16 + 219 Y, C -> 128 + 224 C, full
Y -> 255 Y, C -> 128 + 255 C.  Depth 10: limited Y -> 64 + 876 Y, C -> 512 + 896 C, full Y -> 1023 Y, C -> 512 + 1023 C.  Chroma up: the
block's value for each of its pixels; down: the mean of the block's per-pixel values; RGB clamped to [0, 1] after decoding; codes =
floor(clamp(v, 0, 2^depth - 1) + 0.5), msb-aligned formats store code << 6."""
import numpy as np

PRESETS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True), ("bt2020", False), ("bt2020", True)]
#           planar, depth, msb, sx, sy
FORMATS = {"nv12": (False, 8, False, 1, 1), "i420": (True, 8, False, 1, 1), "p010": (False, 10, True, 1, 1), "yuv420p10": (True, 10, False, 1, 1),
           "nv16": (False, 8, False, 1, 0), "yuv422p": (True, 8, False, 1, 0), "p210": (False, 10, True, 1, 0), "yuv422p10": (True, 10, False, 1, 0),
           "yuv444p": (True, 8, False, 0, 0), "yuv444p10": (True, 10, False, 0, 0)}
NEW = ("yuv422p", "yuv422p10", "nv16", "p210", "yuv444p", "yuv444p10")
_K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def _scales(full_range, depth):
    """(luma scale, chroma scale, luma offset, chroma offset)"""
    if depth == 8:
        return (255.0, 255.0, 0.0, 128.0) if full_range else (219.0, 224.0, 16.0, 128.0)
    return (1023.0, 1023.0, 0.0, 512.0) if full_range else (876.0, 896.0, 64.0, 512.0)


def codes_of(planes, fmt):
    """(Y [F,H,W], Cb, Cr [F, H >> sy, W >> sx]) integer sample codes of a clip"""
    planar, depth, msb, _, _ = FORMATS[fmt]
    p = [np.asarray(a).astype(np.int64) for a in planes]
    if depth == 10:
        p = [(a >> 6) if msb else np.minimum(a, 1023) for a in p]
    if planar:
        return p[0], p[1], p[2]
    return p[0], p[1][..., 0::2], p[1][..., 1::2]


def planes_from_codes(y, cb, cr, fmt):
    planar, depth, msb, _, _ = FORMATS[fmt]
    dt = np.uint8 if depth == 8 else np.uint16
    sh = 6 if msb else 0
    if planar:
        return tuple((np.asarray(a).astype(np.int64) << sh).astype(dt) for a in (y, cb, cr))
    uv = np.stack([cb, cr], axis=-1).reshape(cb.shape[0], cb.shape[1], 2 * cb.shape[2])
    return tuple((np.asarray(a).astype(np.int64) << sh).astype(dt) for a in (y, uv))


def convert(planes, src, dst):
    """the clip of format `dst` that holds the codes of `planes` (same depth, same chroma subsampling)"""
    assert FORMATS[src][1] == FORMATS[dst][1] and FORMATS[src][3:] == FORMATS[dst][3:]
    return planes_from_codes(*codes_of(planes, src), dst)


def replicate(planes, src420, dst):
    """the twin of a 4:2:0 clip in the 4:2:2 or 4:4:4 format `dst` of the same depth: every block's chroma replicated over the finer blocks"""
    assert FORMATS[src420][3:] == (1, 1) and FORMATS[src420][1] == FORMATS[dst][1]
    _, _, _, sx, sy = FORMATS[dst]
    y, cb, cr = codes_of(planes, src420)
    for axis, s in ((1, sy), (2, sx)):
        if s == 0:
            cb, cr = np.repeat(cb, 2, axis=axis), np.repeat(cr, 2, axis=axis)
    return planes_from_codes(y, cb, cr, dst)


def decode(planes, fmt, matrix="bt709", full_range=False, clamp=True):
    """clip -> float64 RGB [F, 3, H, W]; written from the inverse formulas, not from a matrix inverse"""
    _, depth, _, sx, sy = FORMATS[fmt]
    yc, cbc, crc = codes_of(planes, fmt)
    kr, kb = _K[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0, c0 = _scales(full_range, depth)
    y = (yc.astype(np.float64) - y0) / ys
    up = lambda a: np.repeat(np.repeat(a, 1 << sy, axis=1), 1 << sx, axis=2)        # noqa: E731
    cb = (up(cbc).astype(np.float64) - c0) / cs
    cr = (up(crc).astype(np.float64) - c0) / cs
    r = y + 2.0 * (1.0 - kr) * cr
    b = y + 2.0 * (1.0 - kb) * cb
    g = (y - kr * r - kb * b) / kg
    rgb = np.stack([r, g, b], axis=1)
    return np.clip(rgb, 0.0, 1.0) if clamp else rgb


def encode_values(rgb, fmt, matrix="bt709", full_range=False):
    """float RGB [F, 3, H, W] -> float64 code values (Y [F,H,W], Cb, Cr [F, H >> sy, W >> sx]) BEFORE rounding (chroma after the mean)"""
    _, depth, _, sx, sy = FORMATS[fmt]
    rgb = np.asarray(rgb, dtype=np.float64)
    F, _, H, W = rgb.shape
    kr, kb = _K[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0, c0 = _scales(full_range, depth)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    y = kr * r + kg * g + kb * b
    cb = (b - y) / (2.0 * (1.0 - kb))
    cr = (r - y) / (2.0 * (1.0 - kr))
    down = lambda a: a.reshape(F, H >> sy, 1 << sy, W >> sx, 1 << sx).mean(axis=(2, 4))           # noqa: E731
    return y0 + ys * y, down(c0 + cs * cb), down(c0 + cs * cr)


def round_codes(v, depth):
    return np.floor(np.clip(v, 0.0, float((1 << depth) - 1)) + 0.5).astype(np.int64)


def encode(rgb, fmt, matrix="bt709", full_range=False):
    depth = FORMATS[fmt][1]
    return planes_from_codes(*(round_codes(v, depth) for v in encode_values(rgb, fmt, matrix, full_range)), fmt)
