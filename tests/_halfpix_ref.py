"""numpy reference for half-precision clips, independent of videoseal_amd.halfpix (a plain helper module, no pytest hooks).

A clip is a uint16 array of stored words.  fp16 goes through numpy.float16, bf16 through integer arithmetic on the fp32 bits.  Decode and
encode work in float64 with ONE explicit rounding to fp32 where the definition has one (the sum of the signed decode, the difference of the
signed encode) and an explicit round-to-nearest-even into the 16-bit type."""
import numpy as np

TYPES = ("f16", "bf16")
RANGES = ("unit", "signed")


def words_to_f64(w, typ):
    """stored words (uint16) -> their values as float64, exact"""
    w = np.asarray(w, dtype=np.uint16)
    if typ == "f16":
        return w.view(np.float16).astype(np.float64)
    return (w.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def finite(w, typ):
    w = np.asarray(w, dtype=np.uint16)
    return (w & 0x7C00) != 0x7C00 if typ == "f16" else (w & 0x7F80) != 0x7F80


def _rne_f32(x64):
    """float64 -> the nearest fp32 (ties to even): numpy's conversion is IEEE"""
    return np.asarray(x64, dtype=np.float64).astype(np.float32)


def rne_words(v32, typ):
    """finite fp32 values -> the nearest 16-bit word, ties to even, written out"""
    v32 = np.asarray(v32, dtype=np.float32)
    if typ == "bf16":
        u = v32.view(np.uint32).astype(np.uint64)
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    # fp16: scale to the target's grid in float64 (exact), round half to even, rebuild
    a = np.abs(v32.astype(np.float64))
    sign = (v32.view(np.uint32) >> 16).astype(np.uint16) & 0x8000
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.clip(e, -14, 15)                                  # below 2^-14 the grid is the subnormal one: step 2^-24
    step = np.exp2(e - 10)
    q = np.rint(a / step)                                    # numpy's rint rounds half to even; a / step is exact (a power of two)
    val = q * step                                           # <= 65504 for the inputs of this module
    out = val.astype(np.float16).view(np.uint16)             # exact: val is on the fp16 grid
    return (out | sign).astype(np.uint16)


def decode(w, typ, rng):
    """stored words -> component values as fp32 (the definition's one rounding), in an array of float32"""
    y = words_to_f64(w, typ)
    if rng == "unit":
        return y.astype(np.float32)                          # exact
    return _rne_f32(y * 0.5 + 0.5)                           # float64 holds the sum exactly for every finite 16-bit word of |y| < 2^40 ...


def encode(v32, typ, rng):
    """fp32 component values -> stored words: clamp, map to the stored range with one fp32 rounding, RNE into the type"""
    w = np.clip(np.asarray(v32, dtype=np.float32).astype(np.float64), 0.0, 1.0)
    w = np.where(w == 0.0, 0.0, w)                           # a negative zero counts as +0.0
    if rng == "signed":
        w = _rne_f32(w * 2.0 - 1.0).astype(np.float64)       # exact in float64, one rounding to fp32
    return rne_words(w.astype(np.float32), typ)


def all_words():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def ulp(x, typ):
    """spacing of the 16-bit type at |x| (float64 array): 2^(floor(log2 |x|) - p) with p = 10 (f16, at least 2^-24) or 7 (bf16)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1e-300)))
    if typ == "f16":
        return np.exp2(np.maximum(e, -14) - 10)
    return np.exp2(np.maximum(e, -126) - 7)
