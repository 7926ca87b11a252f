"""YUV helpers of every chroma format (videoseal_amd/yuv.py) against the independent float64 restatement of tests/_yuv_ref.py, and the public
surface of the path (exports, header, methods, the refusals that need no GPU).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle.inputs import synthetic_frames
from tests import _yuv_ref as R
from videoseal_amd import native, yuv, yuv420
from videoseal_amd.model import Videoseal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("smooth", "noise")
FMTS = tuple(R.FORMATS)
NEW = R.NEW
# shapes A - E of tests/test_gpu_yuv.py, and G (odd H and W) for 4:4:4
SHAPES = {"A": (5, 134, 202), "B": (6, 72, 88), "C": (3, 134, 522), "D": (2, 18, 34), "E": (3, 67, 202), "G": (2, 131, 259)}

# fp32 decode of in-gamut codes against float64: the bound of tests/test_yuv420_cpu.py and its reasoning (the decode is the same expression)
FP32_DECODE_BOUND = 3e-7


def _shape_ok(fmt, shape):
    _, _, _, sx, sy = R.FORMATS[fmt]
    _, H, W = SHAPES[shape]
    return H % (1 << sy) == 0 and W % (1 << sx) == 0


def _frames(kind, shape="C"):
    F_, H, W = SHAPES[shape]
    return 0.1 + 0.8 * synthetic_frames(F_, H, W, seed=5, kind=kind)


def _t(planes):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)) for p in planes)


def _np(planes, depth):
    return [g.view(torch.int16).numpy().view(np.uint16) if depth == 10 else g.numpy() for g in planes]


def _eq(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _random_words(fmt, shape, seed=11):
    """a clip of random stored words: every bit pattern of the word, the ignored low bits and the saturating range included"""
    planar, depth, msb, sx, sy = R.FORMATS[fmt]
    F_, H, W = SHAPES[shape]
    rng = np.random.default_rng(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    shapes = [(F_, H, W)] + ([(F_, H >> sy, W >> sx)] * 2 if planar else [(F_, H >> sy, W)])
    return tuple(rng.integers(0, top, s).astype(dt) for s in shapes)


def test_formats_table():
    assert set(yuv.FORMATS) == set(R.FORMATS) and len(yuv.FORMATS) == 10
    for fmt, (planar, depth, msb, sx, sy) in R.FORMATS.items():
        assert yuv.fmt_info(fmt) == (planar, depth, msb, {(1, 1): 420, (1, 0): 422, (0, 0): 444}[(sx, sy)])
        if (sx, sy) == (1, 1):
            assert yuv.fmt_info(fmt)[:3] == yuv420.fmt_info(fmt)
    # yuv420.py stays as it is: it does not know the new names
    assert set(yuv420.FORMATS) == {"nv12", "i420", "p010", "yuv420p10"}
    with pytest.raises(ValueError):
        yuv.fmt_info("yuyv422")
    with pytest.raises(ValueError):
        yuv420.fmt_info("yuv422p")


@pytest.mark.parametrize("kind", KINDS + ("words",))
@pytest.mark.parametrize("fmt", FMTS)
def test_helpers_agree_with_the_reference_to_the_last_code(fmt, kind):
    planar, depth, msb, sx, sy = R.FORMATS[fmt]
    shape = "C" if kind != "words" else ("G" if (sx, sy) == (0, 0) else "E" if sy == 0 else "D")
    for matrix, full_range in R.PRESETS:
        if kind == "words":                  # decode only: random words are no encoder's output
            want = _random_words(fmt, shape)
        else:
            x = _frames(kind, shape)
            want = R.encode(x.numpy(), fmt, matrix, full_range)
            got = yuv.from_rgb(x.double(), fmt, matrix, full_range)
            assert all(g.dtype == yuv.fmt_dtype(fmt) and g.is_contiguous() for g in got)
            assert _eq(got, _t(want)), (fmt, matrix, full_range)
            # fp32 arithmetic may only move a code whose float64 value lies on a rounding boundary (the windows of tests/test_yuv420_cpu.py)
            got32 = R.codes_of(_np(yuv.from_rgb(x, fmt, matrix, full_range), depth), fmt)
            for g, w, v in zip(got32, R.codes_of(want, fmt), R.encode_values(x.numpy(), fmt, matrix, full_range)):
                off = g != w
                tol = 1e-3 if depth == 8 else 4e-3
                assert np.all(np.abs(v[off] - np.floor(v[off]) - 0.5) < tol) and off.mean() < 2 * tol
        rgb_ref = R.decode(want, fmt, matrix, full_range)
        rgb64 = yuv.to_rgb(_t(want), fmt, matrix, full_range, dtype=torch.float64)
        rgb32 = yuv.to_rgb(_t(want), fmt, matrix, full_range)
        assert rgb64.shape == rgb_ref.shape
        assert np.abs(rgb64.numpy() - rgb_ref).max() < 1e-12
        if kind != "words":
            assert np.abs(rgb32.double().numpy() - rgb_ref).max() <= FP32_DECODE_BOUND
        else:               # out-of-gamut codes: values up to ~3 before the clamp, the bound scales with them
            assert np.abs(rgb32.double().numpy() - rgb_ref).max() <= 4 * FP32_DECODE_BOUND
            assert (rgb_ref == 0).any() and (rgb_ref == 1).any()            # the clamp is exercised


@pytest.mark.parametrize("fmt", tuple(f for f in FMTS if f not in NEW))
def test_a_420_format_is_yuv420s(fmt):
    x = _frames("noise", "D")
    c = yuv420.from_rgb(x, fmt, "bt601", True)
    assert _eq(yuv.from_rgb(x, fmt, "bt601", True), c)
    assert torch.equal(yuv.to_rgb(c, fmt, "bt601", True), yuv420.to_rgb(c, fmt, "bt601", True))
    assert isinstance(yuv.clip(c, fmt), yuv420.Clip420)
    assert yuv.check_clip(c, fmt) == yuv420.check_clip(c, fmt)


@pytest.mark.parametrize("fmt", NEW)
def test_planes_of_and_pack_round_trip(fmt):
    _, depth, _, sx, sy = R.FORMATS[fmt]
    F_, H, W = (3, 17, 33) if sx == 0 else (3, 17, 34)
    dt = yuv.fmt_dtype(fmt)
    n = yuv.frame_samples(fmt, H, W)
    assert n == (3 * H * W if sx == 0 else 2 * H * W)
    g = torch.Generator().manual_seed(3)
    buf = torch.randint(0, 256, (F_, n * (2 if dt == torch.uint16 else 1)), generator=g, dtype=torch.uint8).view(dt)
    planes = yuv.planes_of(buf, fmt, H, W)
    assert yuv.check_clip(planes, fmt) == (F_, H, W)
    assert all(p.stride(2) == 1 for p in planes)
    assert planes[0].data_ptr() == buf.data_ptr() and planes[1].data_ptr() == buf.data_ptr() + H * W * buf.element_size()
    if len(planes) == 3:
        assert planes[2].data_ptr() == planes[1].data_ptr() + planes[1][0].numel() * buf.element_size()
    back = yuv.pack(planes)
    assert back.is_contiguous() and torch.equal(back.view(torch.uint8), buf.view(torch.uint8))
    if dt == torch.uint16:
        assert _eq(yuv.planes_of(buf.view(torch.int16), fmt, H, W), planes)
    with pytest.raises(ValueError):
        yuv.planes_of(buf, fmt, H + 1, W)
    if sx == 1:
        with pytest.raises(ValueError):
            yuv.planes_of(torch.zeros((1, 2 * 4 * 5), dtype=dt), fmt, 4, 5)
    # the clip class walks like Clip420
    c = yuv.clip(planes, fmt, ("bt601", True))
    assert isinstance(c, yuv.ClipYuv) and c.shape == (F_, H, W) and len(c) == F_ and c.graph_key == (fmt, ("bt601", True))
    e = c.empty_like()
    assert e.buf.shape == (F_, n) and e.buf.is_contiguous() and e.copy_(c) is e and _eq(e.planes, planes)
    assert _eq(c[1:3].planes, tuple(p[1:3] for p in planes)) and c[1:3].shape == (2, H, W)
    assert _eq(c.to("cpu").contiguous().planes, planes) and c.clone().buf.data_ptr() != buf.data_ptr()


@pytest.mark.parametrize("kind", KINDS)
def test_layout_and_replication_twins_decode_to_the_same_bits(kind):
    x = _frames(kind, "A")
    for i, (matrix, full_range) in enumerate(R.PRESETS):
        p8 = R.encode(x.numpy(), "yuv422p", matrix, full_range)
        p10 = R.encode(x.numpy(), "yuv422p10", matrix, full_range)
        nv16, p210 = R.convert(p8, "yuv422p", "nv16"), R.convert(p10, "yuv422p10", "p210")
        low = tuple(p | np.uint16(0x15 + i) for p in p210)                   # p210 ignores its low six bits
        i420, q10 = R.encode(x.numpy(), "i420", matrix, full_range), R.encode(x.numpy(), "yuv420p10", matrix, full_range)
        for dt in (torch.float32, torch.float64):
            a = yuv.to_rgb(_t(p8), "yuv422p", matrix, full_range, dtype=dt)
            assert torch.equal(a, yuv.to_rgb(_t(nv16), "nv16", matrix, full_range, dtype=dt))
            b = yuv.to_rgb(_t(p10), "yuv422p10", matrix, full_range, dtype=dt)
            assert torch.equal(b, yuv.to_rgb(_t(p210), "p210", matrix, full_range, dtype=dt))
            assert torch.equal(b, yuv.to_rgb(_t(low), "p210", matrix, full_range, dtype=dt))
            # a 4:2:0 clip and its twins with replicated chroma
            c8, c10 = yuv420.to_rgb(_t(i420), "i420", matrix, full_range, dtype=dt), yuv420.to_rgb(_t(q10), "yuv420p10", matrix, full_range, dtype=dt)
            for dst in ("yuv422p", "nv16", "yuv444p"):
                assert torch.equal(c8, yuv.to_rgb(_t(R.replicate(i420, "i420", dst)), dst, matrix, full_range, dtype=dt))
            for dst in ("yuv422p10", "p210", "yuv444p10"):
                assert torch.equal(c10, yuv.to_rgb(_t(R.replicate(q10, "yuv420p10", dst)), dst, matrix, full_range, dtype=dt))
    big = tuple(torch.full((1, 1, 2), 4000, dtype=torch.int16).view(torch.uint16) for i in range(3))
    top = tuple(torch.full((1, 1, 2), 1023, dtype=torch.int16).view(torch.uint16) for i in range(3))
    assert torch.equal(yuv.to_rgb(big, "yuv444p10"), yuv.to_rgb(top, "yuv444p10"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_identity_on_the_cpu(shape, kind):
    """from_rgb(to_rgb(c)) == c in float64 and float32 for the six new formats, all three matrices, both ranges, smooth and noise frames:
    nothing is left out.  This grounds the GPU identity test."""
    x = _frames(kind, shape).numpy()
    for fmt in NEW:
        if not _shape_ok(fmt, shape):
            continue
        for matrix, full_range in R.PRESETS:
            c = R.encode(x, fmt, matrix, full_range)
            again = R.encode(R.decode(c, fmt, matrix, full_range), fmt, matrix, full_range)                    # the reference alone
            assert all(np.array_equal(a, b) for a, b in zip(again, c))
            for dt in (torch.float32, torch.float64):
                rgb = yuv.to_rgb(_t(c), fmt, matrix, full_range, dtype=dt)
                assert rgb.dtype == dt
                assert _eq(yuv.from_rgb(rgb, fmt, matrix, full_range), _t(c)), (shape, kind, fmt, matrix, full_range, dt)


def test_check_clip_refuses_malformed_clips():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)      # noqa: E731
    y, u, v = u8(2, 7, 12), u8(2, 7, 6), u8(2, 7, 6)
    assert yuv.check_clip((y, u, v), "yuv422p") == (2, 7, 12)
    assert yuv.check_clip((y, u8(2, 7, 12)), "nv16") == (2, 7, 12)
    assert yuv.check_clip((u8(2, 7, 11),) * 3, "yuv444p") == (2, 7, 11)
    assert yuv.check_clip((y.to(torch.int16), u.to(torch.int16), v.to(torch.int16)), "yuv422p10") == (2, 7, 12)
    for planes, fmt in (((u8(2, 7, 11), u8(2, 7, 5), u8(2, 7, 5)), "yuv422p"),           # odd W for 4:2:2
                        ((u8(2, 7, 11), u8(2, 7, 11)), "nv16"),
                        ((y, u), "yuv422p"), ((y, u, v), "nv16"), ((y, u, v), "yuv422p10"),      # plane count, dtype
                        ((y, u, v[:, :3]), "yuv422p"), ((y, u8(2, 4, 6), u8(2, 4, 6)), "yuv422p"), ((y, u, v), "yuv444p"),       # chroma shapes
                        ((y, u8(2, 7, 6)), "nv16"),
                        ((y, u, u8(2, 6, 7).transpose(1, 2)), "yuv422p"),               # last stride != 1
                        ((y, u, v.to("meta")), "yuv422p"),                               # mixed devices
                        (y, "yuv444p"), ((y, u, v), "yuyv422")):
        with pytest.raises(ValueError):
            yuv.check_clip(planes, fmt)


NEW_SYMBOLS = ("vs_sizeof_yuv_surface", "vs_sizeof_tail_yuv_desc", "vs_resize_pre_yuv", "vs_embed_tail_yuv", "vs_model_embed_yuv", "vs_model_detect_yuv")


def test_exports_are_listed_declared_and_built():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    declared = set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", header))
    lib = native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in native.EXPORTS and sym in declared and hasattr(lib, sym), sym
    assert "vs_yuv_surface_t" in header and "vs_tail_yuv_desc_t" in header
    for word in ("yuyv422", "uyvy422", "v210", "nv24", "p410", "depth 12"):          # what is out of scope is said in the header
        assert word in header, word
    assert lib.vs_version() == 3
    assert lib.vs_sizeof_yuv_surface() == ctypes.sizeof(native.YuvSurface)
    assert lib.vs_sizeof_tail_yuv_desc() == ctypes.sizeof(native.TailYuvDesc)


def _surface(planar, depth, msb, chroma, ptr=16):
    s = native.YuvSurface()
    s.planar, s.depth, s.msb_aligned, s.chroma = planar, depth, msb, chroma
    for i in range(3):
        s.plane[i], s.pitch[i], s.frame_stride[i] = ptr, 64, 64 * 64          # (never dereferenced: every call below is refused on the host)
    return s


KNOWN = {(p, d, m, c) for (p, d, m, c) in (tuple(int(v) for v in yuv.FORMATS[f]) for f in yuv.FORMATS)}


def test_c_level_refusals_that_need_no_gpu():
    lib = native.lib()
    UNS = native.ERR_UNSUPPORTED
    dec = (ctypes.c_float * 12)()
    out = ctypes.c_void_p(16)

    def resize(s, H, W):
        return lib.vs_resize_pre_yuv(ctypes.byref(s), 1, H, W, dec, 4, 4, 1, out, 1.0, 0.0, None, 1, None, None)
    assert lib.vs_embed_tail_yuv(None, None) == -1
    assert lib.vs_resize_pre_yuv(None, 1, 8, 8, None, 4, 4, 1, None, 1.0, 0.0, None, 1, None, None) == -1
    assert len(KNOWN) == 10
    # every (planar, depth, msb_aligned, chroma) outside the ten formats
    for planar in (0, 1, 2):
        for depth in (8, 10, 12):
            for msb in (0, 1):
                for chroma in (400, 411, 420, 422, 444):
                    if (planar, depth, msb, chroma) not in KNOWN:
                        assert resize(_surface(planar, depth, msb, chroma), 8, 8) == UNS, (planar, depth, msb, chroma)
    # the size rule comes from the format
    for fmt in yuv.FORMATS:
        planar, depth, msb, chroma = (int(v) for v in yuv.FORMATS[fmt])
        s = _surface(planar, depth, msb, chroma)
        if chroma != 444:
            assert resize(s, 8, 7) == -1                                                        # odd W: refused for 4:2:0 and 4:2:2
        if chroma == 420:
            assert resize(s, 7, 8) == -1                                                        # odd H: refused for 4:2:0 alone
        s.pitch[1 if planar == 0 else 2] = 3                                                    # a pitch shorter than its row
        assert resize(s, 8, 8) == -1, fmt
        s = _surface(planar, depth, msb, chroma)
        s.pitch[0] = 8 * (2 if depth == 10 else 1) - 1
        assert resize(s, 8, 8) == -1, fmt
    # the tail: refusals in front of any launch
    delta = ctypes.c_void_p(16)
    taps = (ctypes.c_float * 43)()

    def desc(src, dst, **kw):
        d = native.TailYuvDesc()
        d.src, d.dst = src, dst
        d.delta, d.taps43 = delta, ctypes.cast(taps, ctypes.c_void_p)
        d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = 1, 8, 8, 4, 4, 1
        d.step, d.video_mode, d.total_key, d.attenuate, d.clamp, d.antialias = 1, 0, 1, 0, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for fmt in yuv.FORMATS:
        f = tuple(int(v) for v in yuv.FORMATS[fmt])
        s = _surface(*f)
        assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, s, preds_w=ctypes.c_void_p(16))), None) == UNS, fmt
        assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, s, attenuate=2)), None) == UNS, fmt
        for variant in (2, 3, 5, -1):
            assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, s, variant=variant)), None) == UNS, (fmt, variant)
        for other in yuv.FORMATS:                                                  # two surfaces of different formats
            if other != fmt:
                o = _surface(*(int(v) for v in yuv.FORMATS[other]))
                assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, o)), None) == UNS, (fmt, other)
        if f[3] != 444:
            assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, s, W=7)), None) == -1, fmt
        if f[3] == 420:
            assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, s, H=7)), None) == -1, fmt
        assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, s, clamp=0)), None) == -1, fmt
        short = _surface(*f)
        short.pitch[0] = 7
        assert lib.vs_embed_tail_yuv(ctypes.byref(desc(s, short)), None) == -1, fmt
    # the 4:2:0 entry points go on refusing what they refused
    s420 = native.Yuv420Surface()
    s420.planar, s420.depth, s420.msb_aligned = 1, 8, 0
    assert lib.vs_resize_pre_yuv420(ctypes.byref(s420), 1, 7, 8, dec, 4, 4, 1, out, 1.0, 0.0, None, 1, None, None) == -1


def test_videoseal_has_both_methods():
    assert callable(getattr(Videoseal, "embed_yuv", None)) and callable(getattr(Videoseal, "detect_yuv", None))
    from videoseal_amd.capi import CModel
    assert callable(getattr(CModel, "embed_yuv", None)) and callable(getattr(CModel, "detect_yuv", None))
    from videoseal.models import Videoseal as Shim           # the reference's import path
    assert Shim.embed_yuv is Videoseal.embed_yuv and Shim.detect_yuv is Videoseal.detect_yuv
