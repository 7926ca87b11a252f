"""4:2:0 helpers (videoseal_amd/yuv420.py) against the independent float64 restatement of tests/_yuv420_ref.py, and the public surface of the
path (exports, header, methods).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle.inputs import synthetic_frames
from tests import _yuv420_ref as R
from videoseal_amd import native, nv12, yuv420
from videoseal_amd.model import Videoseal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("smooth", "noise")
FMTS = ("nv12", "i420", "p010", "yuv420p10")
SHAPES = {"A": (5, 134, 202), "B": (6, 72, 88), "C": (3, 134, 522), "D": (2, 18, 34)}

# fp32 decode of in-gamut codes against float64: the bound of tests/test_nv12_cpu.py and its reasoning.  to_rgb subtracts the offsets exactly
# at either depth (codes and offsets are integers below 2^10), the three products stay below 1 in magnitude for RGB in [0.1, 0.9], and the
# roundings (three products, one partial sum, the result, the fp32 coefficients) add up to at most 3.3e-7, 2.4e-7 on the worst channel.
FP32_DECODE_BOUND = 3e-7


def _frames(kind, shape="C"):
    F_, H, W = SHAPES[shape]
    return 0.1 + 0.8 * synthetic_frames(F_, H, W, seed=5, kind=kind)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _t(planes):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)) for p in planes)


def _eq(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_depth_8_affine_is_nv12s_bit_for_bit():
    for matrix, full_range in R.PRESETS[:4]:
        f8, i8 = yuv420.color_affine(matrix, full_range, 8)
        f0, i0 = nv12.color_affine(matrix, full_range)
        assert np.array_equal(_bits(f8), _bits(f0)) and np.array_equal(_bits(i8), _bits(i0))


def test_color_affine_is_an_inverse_pair():
    for depth in (8, 10):
        for matrix, full_range in R.PRESETS:
            fwd, inv = yuv420.color_affine(matrix, full_range, depth)
            assert fwd.dtype == np.float64 and inv.dtype == np.float64 and fwd.shape == (3, 4) and inv.shape == (3, 4)
            assert np.abs(inv[:, :3] @ fwd[:, :3] - np.eye(3)).max() < 1e-14
            assert np.abs(inv[:, :3] @ fwd[:, 3] + inv[:, 3]).max() < 1e-12
    fwd, _ = yuv420.color_affine("bt2020", False, 10)
    assert fwd[0, 3] == 64.0 and fwd[1, 3] == 512.0 and abs(fwd[0, :3].sum() - 876.0) < 1e-12 and abs(fwd[0, 0] - 876.0 * 0.2627) < 1e-12
    assert abs(fwd[1, 2] - 448.0) < 1e-12 and abs(fwd[2, 0] - 448.0) < 1e-12                # Cb(B = 1) = Cr(R = 1) = 0.5 -> 896 / 2
    fwd, _ = yuv420.color_affine("bt709", True, 10)
    assert fwd[0, 3] == 0.0 and abs(fwd[0, :3].sum() - 1023.0) < 1e-12 and abs(fwd[1, 2] - 511.5) < 1e-12
    with pytest.raises(ValueError):
        yuv420.color_affine("bt470", False, 8)
    with pytest.raises(ValueError):
        yuv420.color_affine("bt709", False, 12)
    with pytest.raises(ValueError):
        nv12.color_affine("bt2020", False)              # nv12.py keeps its two matrices


def _c_default(depth):
    dec, enc = (ctypes.c_float * 12)(), (ctypes.c_float * 12)()
    assert native.lib().vs_yuv420_default_color(depth, dec, enc) == 0
    return np.array(list(dec), dtype=np.float32).view(np.uint32), np.array(list(enc), dtype=np.float32).view(np.uint32)


def test_c_default_colour():
    lib = native.lib()
    dec, enc = (ctypes.c_float * 12)(), (ctypes.c_float * 12)()
    assert lib.vs_nv12_default_color(dec, enc) == 0
    d8, e8 = _c_default(8)
    assert np.array_equal(d8, np.array(list(dec), dtype=np.float32).view(np.uint32))
    assert np.array_equal(e8, np.array(list(enc), dtype=np.float32).view(np.uint32))
    d10, e10 = _c_default(10)
    fwd, inv = yuv420.color_affine("bt709", False, 10)
    assert np.array_equal(d10, inv.reshape(-1).astype(np.float32).view(np.uint32))
    assert np.array_equal(e10, fwd.reshape(-1).astype(np.float32).view(np.uint32))
    assert lib.vs_yuv420_default_color(12, dec, enc) == -1 and lib.vs_yuv420_default_color(10, None, enc) == -1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_helpers_agree_with_the_reference_to_the_last_code(fmt, kind):
    planar, depth, msb = R.FORMATS[fmt]
    x = _frames(kind)
    for matrix, full_range in R.PRESETS:
        want = R.encode(x.numpy(), fmt, matrix, full_range)
        got = yuv420.from_rgb(x.double(), fmt, matrix, full_range)
        assert all(g.dtype == yuv420.fmt_dtype(fmt) and g.is_contiguous() for g in got)
        assert _eq(got, _t(want)), (fmt, matrix, full_range)
        # fp32 arithmetic may only move a code whose float64 value lies on a rounding boundary (distance < 1e-3 of x.5 at depth 8; code
        # values are four times as large at depth 10, and so is an fp32 rounding of them)
        got32 = R.codes_of([g.view(torch.int16).numpy().view(np.uint16) if depth == 10 else g.numpy() for g in yuv420.from_rgb(x, fmt, matrix, full_range)], fmt)
        for g, w, v in zip(got32, R.codes_of(want, fmt), R.encode_values(x.numpy(), depth, matrix, full_range)):
            off = g != w
            tol = 1e-3 if depth == 8 else 4e-3
            assert np.all(np.abs(v[off] - np.floor(v[off]) - 0.5) < tol) and off.mean() < 2 * tol       # (the window holds 2 tol of all values)
        rgb_ref = R.decode(want, fmt, matrix, full_range)
        rgb64 = yuv420.to_rgb(_t(want), fmt, matrix, full_range, dtype=torch.float64)
        rgb32 = yuv420.to_rgb(_t(want), fmt, matrix, full_range)
        assert np.abs(rgb64.numpy() - rgb_ref).max() < 1e-12
        assert np.abs(rgb32.double().numpy() - rgb_ref).max() <= FP32_DECODE_BOUND


@pytest.mark.parametrize("fmt", FMTS)
def test_planes_of_and_pack_round_trip(fmt):
    F_, H, W = 3, 18, 34
    dt = yuv420.fmt_dtype(fmt)
    n = H * W * 3 // 2
    g = torch.Generator().manual_seed(3)
    buf = torch.randint(0, 256, (F_, n * (2 if dt == torch.uint16 else 1)), generator=g, dtype=torch.uint8).view(dt)
    planes = yuv420.planes_of(buf, fmt, H, W)
    assert yuv420.check_clip(planes, fmt) == (F_, H, W)
    assert all(p.data_ptr() >= buf.data_ptr() and p.stride(2) == 1 for p in planes)             # views, not copies
    assert planes[0].data_ptr() == buf.data_ptr() and planes[1].data_ptr() == buf.data_ptr() + H * W * buf.element_size()
    back = yuv420.pack(planes)
    assert back.is_contiguous() and torch.equal(back.view(torch.uint8), buf.view(torch.uint8))
    # the byte order of rawvideo: frame 1 starts right after frame 0's last plane
    flat = buf.view(torch.uint8).reshape(-1)
    assert torch.equal(planes[-1][0].contiguous().view(torch.uint8).reshape(-1)[-4:], flat[n * buf.element_size() - 4:n * buf.element_size()])
    # int16 carries the same bits
    if dt == torch.uint16:
        assert _eq(yuv420.planes_of(buf.view(torch.int16), fmt, H, W), planes)
    with pytest.raises(ValueError):
        yuv420.planes_of(buf, fmt, H + 1, W)


@pytest.mark.parametrize("kind", KINDS)
def test_layout_twins_decode_to_the_same_bits(kind):
    x = _frames(kind, "A")
    for i, (matrix, full_range) in enumerate(R.PRESETS):
        if matrix != "bt2020":
            i420 = R.encode(x.numpy(), "i420", matrix, full_range)
            y, uv = R.convert(i420, "i420", "nv12")
            clip = torch.from_numpy(np.concatenate([y, uv], axis=1))
            for dt in (torch.float32, torch.float64):
                assert torch.equal(yuv420.to_rgb(_t(i420), "i420", matrix, full_range, dtype=dt), nv12.nv12_to_rgb(clip, matrix, full_range, dtype=dt))
                assert torch.equal(yuv420.to_rgb(_t((y, uv)), "nv12", matrix, full_range, dtype=dt), nv12.nv12_to_rgb(clip, matrix, full_range, dtype=dt))
        p10 = R.encode(x.numpy(), "yuv420p10", matrix, full_range)
        p010 = R.convert(p10, "yuv420p10", "p010")
        assert np.array_equal(p010[0], p10[0].astype(np.uint16) << 6)
        low = tuple(p | np.uint16(0x15 + i) for p in p010)                   # p010 ignores its low six bits
        for dt in (torch.float32, torch.float64):
            a = yuv420.to_rgb(_t(p10), "yuv420p10", matrix, full_range, dtype=dt)
            assert torch.equal(a, yuv420.to_rgb(_t(p010), "p010", matrix, full_range, dtype=dt))
            assert torch.equal(a, yuv420.to_rgb(_t(low), "p010", matrix, full_range, dtype=dt))
    # yuv420p10 saturates a word above 1023
    big = tuple(torch.full((1, 2, 2) if i == 0 else (1, 1, 1), 4000, dtype=torch.int16).view(torch.uint16) for i in range(3))
    top = tuple(torch.full((1, 2, 2) if i == 0 else (1, 1, 1), 1023, dtype=torch.int16).view(torch.uint16) for i in range(3))
    assert torch.equal(yuv420.to_rgb(big, "yuv420p10"), yuv420.to_rgb(top, "yuv420p10"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_identity_on_the_cpu(shape, kind):
    """from_rgb(to_rgb(c)) == c in float64 and float32, depths 8 and 10, all three matrices, both ranges: nothing is left out"""
    x = _frames(kind, shape).numpy()
    for fmt in FMTS:
        for matrix, full_range in R.PRESETS:
            c = R.encode(x, fmt, matrix, full_range)
            again = R.encode(R.decode(c, fmt, matrix, full_range), fmt, matrix, full_range)                    # the reference alone
            assert all(np.array_equal(a, b) for a, b in zip(again, c))
            for dt in (torch.float32, torch.float64):
                rgb = yuv420.to_rgb(_t(c), fmt, matrix, full_range, dtype=dt)
                assert rgb.dtype == dt
                assert _eq(yuv420.from_rgb(rgb, fmt, matrix, full_range), _t(c)), (shape, kind, fmt, matrix, full_range, dt)


def test_check_clip_refuses_malformed_clips():
    y, u, v = (torch.zeros(2, 8, 12, dtype=torch.uint8), torch.zeros(2, 4, 6, dtype=torch.uint8), torch.zeros(2, 4, 6, dtype=torch.uint8))
    assert yuv420.check_clip((y, u, v), "i420") == (2, 8, 12)
    assert yuv420.check_clip((y.to(torch.int16), u.to(torch.int16), v.to(torch.int16)), "yuv420p10") == (2, 8, 12)
    for planes, fmt in (((y, u), "i420"), ((y, u, v), "nv12"), ((y, u, v), "yuv420p10"), ((y, u, v[:, :3]), "i420"), ((y[:, :7], u, v), "i420"),
                        ((y, u, v), "yuv444p"), ((y, u, torch.zeros(2, 6, 4, dtype=torch.uint8).transpose(1, 2)), "i420"), (y, "i420")):
        with pytest.raises(ValueError):
            yuv420.check_clip(planes, fmt)


def test_exports_are_listed_declared_and_built():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    declared = set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", header))
    lib = native.lib()
    for sym in ("vs_sizeof_yuv420_surface", "vs_sizeof_tail_yuv420_desc", "vs_resize_pre_yuv420", "vs_embed_tail_yuv420", "vs_yuv420_default_color",
                "vs_model_embed_yuv420", "vs_model_detect_yuv420"):
        assert sym in native.EXPORTS and sym in declared and hasattr(lib, sym), sym
    assert "vs_yuv420_surface_t" in header and "vs_tail_yuv420_desc_t" in header
    assert lib.vs_version() == 3
    assert lib.vs_sizeof_yuv420_surface() == ctypes.sizeof(native.Yuv420Surface)
    assert lib.vs_sizeof_tail_yuv420_desc() == ctypes.sizeof(native.TailYuv420Desc)
    # argument validation happens on the host before any launch
    assert lib.vs_embed_tail_yuv420(None, None) == -1
    assert lib.vs_resize_pre_yuv420(None, 1, 8, 8, None, 4, 4, 1, None, 1.0, 0.0, None, 1, None, None) == -1
    s = native.Yuv420Surface()
    s.planar, s.depth, s.msb_aligned = 1, 10, 1                     # no such format
    dec = (ctypes.c_float * 12)()
    out = ctypes.c_void_p(16)                                       # (never dereferenced: the format is refused first)
    assert lib.vs_resize_pre_yuv420(ctypes.byref(s), 1, 8, 8, dec, 4, 4, 1, out, 1.0, 0.0, None, 1, None, None) == native.ERR_UNSUPPORTED
    s.planar, s.depth, s.msb_aligned = 1, 8, 0
    assert lib.vs_resize_pre_yuv420(ctypes.byref(s), 1, 7, 8, dec, 4, 4, 1, out, 1.0, 0.0, None, 1, None, None) == -1         # odd H


def test_videoseal_has_both_methods():
    assert callable(getattr(Videoseal, "embed_yuv420", None)) and callable(getattr(Videoseal, "detect_yuv420", None))
    from videoseal_amd.capi import CModel
    assert callable(getattr(CModel, "embed_yuv420", None)) and callable(getattr(CModel, "detect_yuv420", None))
