"""Packed RGB clips on the CPU: videoseal_amd/rgbpack.py (the definitions of embed_rgb / detect_rgb) against tests/_rgbpack_ref.py (float64
numpy, independent of it), the round-trip identities the kernels rely on, the refusals of check_clip, the clip object, and the C-ABI's
declarations, exports and struct sizes.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _rgbpack_ref as R  # noqa: E402

from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import rgbpack  # noqa: E402

NEW_EXPORTS = ("vs_sizeof_rgb_surface", "vs_sizeof_tail_rgb_desc", "vs_resize_pre_rgb", "vs_embed_tail_rgb", "vs_model_embed_rgb",
               "vs_model_detect_rgb")


def _t(a):
    """numpy clip -> torch (a uint32 word array as int32: the same bits)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def random_clip(fmt, F_=2, H=9, W=13, seed=0):
    dt, comps, depth, _, _ = R.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    if comps == 0:
        return rng.integers(0, 1 << 32, size=(F_, H, W), dtype=np.uint64).astype(np.uint32)
    return rng.integers(0, 1 << depth, size=(F_, H, W, comps)).astype(dt)


def test_format_tables_agree():
    assert tuple(rgbpack.FORMATS) == tuple(R.FORMATS)
    for fmt, (dt, comps, depth, pos, apos) in R.FORMATS.items():
        i, d, c, p, a = rgbpack.fmt_info(fmt)
        assert (i, d, c, tuple(p), a) == (R.IDS[fmt], depth, comps, pos, apos), fmt
        assert rgbpack.pixel_bytes(fmt) == R.pixel_bytes(fmt)
        assert rgbpack.fmt_dtype(fmt) == {np.uint8: torch.uint8, np.uint16: torch.uint16, np.uint32: torch.int32}[dt]
    with pytest.raises(ValueError, match="fmt must be one of"):
        rgbpack.fmt_info("rgb565")


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_definitions_against_float64(fmt):
    """to_rgb is the fp32 IEEE quotient of the float64 reference's codes; from_rgb on float64 frames gives the reference's words, alpha / X
    from `like` or opaque; on fp32 frames a code differs from the float64 one only where x * top lies within fp32 rounding of an integer"""
    clip = random_clip(fmt, seed=1)
    top = R.top_of(fmt)
    ref = R.decode(clip, fmt)                                              # float64 [F, 3, H, W]
    got = rgbpack.to_rgb(_t(clip), fmt)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape and got.is_contiguous()
    want32 = (R.codes_of(clip, fmt).astype(np.float32) / np.float32(top)).transpose(0, 3, 1, 2)
    assert np.array_equal(got.numpy(), want32)
    assert np.abs(got.numpy().astype(np.float64) - ref).max() <= 2.0 ** -24
    assert np.array_equal(rgbpack.to_rgb(_t(clip), fmt, dtype=torch.float64).numpy(), ref)
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.2, 1.2, size=ref.shape)                             # values outside [0, 1]: the clamp
    for like in (None, clip):
        want = R.encode(x, fmt, like=like)
        out = rgbpack.from_rgb(torch.from_numpy(x), fmt, like=None if like is None else _t(like))
        assert out.is_contiguous() and out.dtype == rgbpack.fmt_dtype(fmt)
        assert np.array_equal(_bytes(out).numpy(), _bytes(_t(want)).numpy()), (fmt, like is None)
        out32 = rgbpack.from_rgb(torch.from_numpy(x).float(), fmt, like=None if like is None else _t(like))
        c64, c32 = R.codes_of(want, fmt), R.codes_of(out32.numpy().view(clip.dtype), fmt)
        v = R.encode_values(x.astype(np.float32), fmt)
        near = np.abs(v - np.round(v)) <= top * 2.0 ** -22
        assert np.abs(c64 - c32).max() <= 1 and np.array_equal(c64[~near], c32[~near])
        a64, a32 = R.alpha_of(want, fmt), R.alpha_of(out32.numpy().view(clip.dtype), fmt)
        assert a64 is None or np.array_equal(a64, a32)
    if R.alpha_of(clip, fmt) is not None:                                  # opaque: all ones
        assert int(R.alpha_of(R.encode(x, fmt), fmt).min()) == (3 if R.FORMATS[fmt][1] == 0 else top)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_round_trip_is_exact_for_every_code(depth):
    """floor((c / top) * top) == c in fp32 for all 2^depth codes: an unwatermarked pixel comes back unchanged.  The quotient is the IEEE one
    (numpy and torch agree), and the Newton form the kernels use -- q = c * (1 / top), q + fma(-q, top, c) * (1 / top) -- reproduces it"""
    top = (1 << depth) - 1
    c = torch.arange(top + 1, dtype=torch.float32)
    q = c / torch.tensor(float(top), dtype=torch.float32)
    assert np.array_equal(q.numpy(), np.arange(top + 1, dtype=np.float32) / np.float32(top))
    assert torch.equal(torch.floor(q * float(top)), c)
    # the Newton step in float64 emulation of the two fused multiply-adds (each product is exact in float64, rounded once to fp32)
    r = np.float32(1.0) / np.float32(top)
    cn = np.arange(top + 1, dtype=np.float32)
    q0 = (cn * r).astype(np.float32)
    rem = (cn.astype(np.float64) - q0.astype(np.float64) * float(top)).astype(np.float32)
    newton = (q0.astype(np.float64) + rem.astype(np.float64) * np.float64(r)).astype(np.float32)
    assert np.array_equal(newton, q.numpy())
    fmt = {8: "rgb24", 10: "x2rgb10", 16: "rgb48"}[depth]
    n = top + 1
    codes = np.stack([np.arange(n), (n - 1) - np.arange(n), (np.arange(n) * 5 + 1) % n], axis=-1).reshape(1, 1, n, 3)       # every code in every position
    clip = R.encode(codes.transpose(0, 3, 1, 2) / float(top) + 1e-9, fmt)
    assert np.array_equal(R.codes_of(clip, fmt), codes)
    back = rgbpack.from_rgb(rgbpack.to_rgb(_t(clip), fmt), fmt, like=_t(clip))
    assert torch.equal(_bytes(back), _bytes(_t(clip)))


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_from_rgb_of_to_rgb_is_the_identity_on_random_words(fmt):
    clip = _t(random_clip(fmt, F_=3, H=17, W=29, seed=4))
    back = rgbpack.from_rgb(rgbpack.to_rgb(clip, fmt), fmt, like=clip)
    assert back.dtype == clip.dtype and back.shape == clip.shape and torch.equal(_bytes(back), _bytes(clip))
    if rgbpack.fmt_info(fmt)[1] == 16:                                     # int16 is the same bits
        assert torch.equal(rgbpack.to_rgb(clip.view(torch.int16), fmt), rgbpack.to_rgb(clip, fmt))
    if rgbpack.fmt_info(fmt)[2] == 0 and hasattr(torch, "uint32"):         # and so is uint32
        assert torch.equal(rgbpack.to_rgb(clip.view(torch.uint32), fmt), rgbpack.to_rgb(clip, fmt))


def test_check_clip_refusals_and_pitched_views():
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (3, 6, 10, 4), dtype=torch.uint8, generator=g)
    assert rgbpack.check_clip(u8, "bgra") == (3, 6, 10)
    assert rgbpack.check_clip(u8[..., :3].contiguous(), "rgb24") == (3, 6, 10)
    # a pitched surface with spare rows is a strided view, not a copy
    buf = torch.zeros(3, 9, 10 * 4 + 7, dtype=torch.uint8)
    view = buf[:, :6, :40].unflatten(-1, (10, 4))
    assert view.stride() == (9 * 47, 47, 4, 1) and rgbpack.check_clip(view, "rgba") == (3, 6, 10)
    assert torch.equal(rgbpack.to_rgb(view, "rgba"), torch.zeros(3, 3, 6, 10))
    w16 = torch.zeros(2, 4, 5, 3, dtype=torch.int16)
    assert rgbpack.check_clip(w16, "rgb48") == (2, 4, 5)
    x2 = torch.zeros(2, 4, 5, dtype=torch.int32)
    assert rgbpack.check_clip(x2, "x2bgr10") == (2, 4, 5)
    bad = [(u8, "rgb24", "shape"), (u8, "rgba64", "uint16"), (u8.float(), "rgba", "uint8"), (u8[0], "rgba", "shape"), (x2, "rgba", "uint8"),
           (w16, "x2rgb10", "int32"), (u8[..., :3], "rgb24", "compact"), (u8[:, :, ::2], "bgra", "compact"), (torch.as_strided(u8, (3, 6, 10, 4), (240, 30, 4, 1)), "argb", "pitch"),
           (u8[0:1].expand(3, 6, 10, 4), "abgr", "overlap"), (x2.transpose(1, 2), "x2rgb10", "compact"), (u8, "rgb565", "fmt must be one of"),
           ([u8], "rgba", "one tensor"), (u8[:, :0], "rgba", "H, W >= 1")]
    for clip, fmt, why in bad:
        with pytest.raises(ValueError, match=why):
            rgbpack.check_clip(clip, fmt, "test")
    assert rgbpack.check_clip(u8[:0], "rgba") == (0, 6, 10)                # an empty clip is a clip
    with pytest.raises(ValueError):
        rgbpack.from_rgb(torch.zeros(3, 3, 6, 9), "bgra", like=u8)         # `like` of another size
    with pytest.raises(ValueError):
        rgbpack.from_rgb(torch.zeros(3, 6, 10), "bgra")


def test_clip_object_walks_like_a_yuv_clip():
    """what Videoseal._run_chunks and the graph cache ask of a clip: slices by frames, empty_like, contiguous, to, copy_, clone, graph_key"""
    from videoseal_amd import yuv
    buf = torch.arange(4 * 7 * 52, dtype=torch.int16).reshape(4, 7, 52)
    view = buf[:, :5, :48].unflatten(-1, (6, 8))[..., :4]                  # not compact: refused
    with pytest.raises(ValueError):
        rgbpack.clip(view, "rgba64")
    view = buf[:, :5, :24].unflatten(-1, (6, 4))
    c = rgbpack.clip(view, "rgba64")
    assert isinstance(c, yuv.Clip) and c.shape == (4, 5, 6) and len(c) == 4 and c.dtype == torch.uint16 and c.graph_key == ("rgba64",)
    assert c.dim() == 0 and c.numel() == 4 * 5 * 6 * 4 and c.tensor.data_ptr() == view.data_ptr()
    s = c[1:3]
    assert isinstance(s, rgbpack.Clip) and s.shape == (2, 5, 6) and s.fmt == "rgba64" and s.tensor.data_ptr() == view[1:3].data_ptr()
    with pytest.raises(TypeError):
        c[0]
    e = c.empty_like()
    assert e.tensor.is_contiguous() and e.tensor.shape == view.shape and e.contiguous() is e
    e.copy_(c)
    assert torch.equal(e.tensor.view(torch.int16), view)
    k = c.contiguous()
    assert k is not c and k.tensor.is_contiguous() and torch.equal(k.tensor.view(torch.int16), view)
    e[2:4].copy_(c[0:2])
    assert torch.equal(e.tensor.view(torch.int16)[2:4], view[0:2])
    t = c.to("cpu")
    assert isinstance(t, rgbpack.Clip) and t.fmt == "rgba64" and torch.equal(t.tensor.view(torch.int16), view)
    assert rgbpack.clip(torch.zeros(1, 2, 3, dtype=torch.int32), "x2rgb10").graph_key != rgbpack.clip(torch.zeros(1, 2, 3, dtype=torch.int32), "x2bgr10").graph_key


def test_header_exports_and_struct_sizes():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    declared = set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", header))
    lib = N.lib()
    for sym in NEW_EXPORTS:
        assert sym in declared and sym in N.EXPORTS and hasattr(lib, sym), sym
    for fmt, i in R.IDS.items():
        assert re.search(rf"#define VS_RGB_{fmt.upper()} {i}\b", header), fmt
        assert rgbpack.fmt_info(fmt)[0] == i
    assert lib.vs_sizeof_rgb_surface() == C.sizeof(N.RgbSurface) == 32
    assert lib.vs_sizeof_tail_rgb_desc() == C.sizeof(N.TailRgbDesc)
    assert [f[0] for f in N.TailRgbDesc._fields_[2:]] == [f[0] for f in N.TailDesc._fields_[2:]]
    assert [f[0] for f in N.TailRgbDesc._fields_[2:]] == [f[0] for f in N.TailYuvDesc._fields_[2:-2]]      # vs_tail_yuv_desc_t without the colour arrays


def test_abi_version_stays_3():
    assert N.lib().vs_version() == 3


def test_c_level_refusals_need_no_gpu():
    """the checks of the two entry points come before any launch: they answer on a machine without a GPU (host pointers are never followed)"""
    lib = N.lib()
    buf = (C.c_ubyte * 4096)()
    other = (C.c_ubyte * 4096)()
    flt = (C.c_float * 16)()
    addr, oaddr, faddr = C.addressof(buf), C.addressof(other), C.addressof(flt)

    def surf(fmt=0, pitch=8 * 3, fs=8 * 3 * 4, data=addr):
        s = N.RgbSurface()
        s.data, s.pitch, s.frame_stride, s.format = data, pitch, fs, fmt
        return s

    def resize(s, B=1, H=4, W=8, oh=4, ow=4, dst=faddr):
        return lib.vs_resize_pre_rgb(C.byref(s), B, H, W, oh, ow, 1, dst, 1.0, 0.0, None, 1, None, None)
    assert lib.vs_resize_pre_rgb(None, 1, 4, 8, 4, 4, 1, faddr, 1.0, 0.0, None, 1, None, None) == -1
    assert resize(surf(data=None)) == -1
    assert resize(surf(), H=0) == -1 and resize(surf(), W=-1) == -1 and resize(surf(), oh=0) == -1 and resize(surf(), dst=None) == -1
    assert resize(surf(fmt=12)) == N.ERR_UNSUPPORTED and resize(surf(fmt=-1)) == N.ERR_UNSUPPORTED
    assert resize(surf(pitch=23)) == -1                                   # a pitch shorter than its row
    assert resize(surf(fmt=8, pitch=63)) == -1                            # ... of a 8-byte pixel
    assert resize(surf(fs=8 * 3 * 4 - 1), B=2) == -1                      # frames overlap

    def desc(**kw):
        d = N.TailRgbDesc()
        d.src, d.dst = surf(), surf(data=oaddr)
        d.delta, d.F, d.H, d.W, d.S_h, d.S_w, d.Cd, d.step, d.total_key, d.clamp = faddr, 1, 4, 8, 2, 2, 1, 1, 1, 1
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d
    tail = lambda d: lib.vs_embed_tail_rgb(C.byref(d), None)              # noqa: E731
    assert lib.vs_embed_tail_rgb(None, None) == -1
    assert tail(desc(delta=None)) == -1 and tail(desc(F=0)) == -1 and tail(desc(W=0)) == -1 and tail(desc(S_h=0)) == -1
    assert tail(desc(clamp=0)) == -1 and tail(desc(clamp=2)) == -1
    assert tail(desc(Cd=2)) == -1 and tail(desc(video_mode=3)) == -1
    d = desc()
    d.dst = surf()                                                        # dst.data == src.data
    assert tail(d) == -1
    d = desc()
    d.dst.pitch = 23
    assert tail(d) == -1
    d = desc()
    d.src.format = 12
    assert tail(d) == N.ERR_UNSUPPORTED
    d = desc()
    d.dst.format = 1                                                      # the two surfaces hold different formats
    assert tail(d) == N.ERR_UNSUPPORTED
    assert tail(desc(preds_w=faddr)) == N.ERR_UNSUPPORTED
    assert tail(desc(attenuate=2)) == N.ERR_UNSUPPORTED
    for variant in (2, 3, 5, -1):
        assert tail(desc(variant=variant)) == N.ERR_UNSUPPORTED
    assert tail(desc(variant=4, S_h=4)) == N.ERR_UNSUPPORTED              # the row-streaming form needs H >= 2 S_h
