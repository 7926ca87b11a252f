"""NV12 helpers (videoseal_amd/nv12.py) against the independent float64 restatement of tests/_nv12_ref.py, and the public surface of the
NV12 path (exports, header, methods).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from oracle.inputs import synthetic_frames
from tests import _nv12_ref as R
from videoseal_amd import native, nv12
from videoseal_amd.model import Videoseal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("smooth", "noise")


# fp32 decode of in-gamut codes against float64.  nv12_to_rgb subtracts the offsets exactly and sums three products, each below 1 in magnitude
# for RGB in [0.1, 0.9] (luma term <= 0.9, a chroma term <= 0.8): three products rounded to 2^-25 each, one partial sum below 2 (2^-24), the
# result in [0, 1] (2^-25), and the coefficients rounded to fp32 (2^-24 relative to terms whose magnitudes sum to at most 2.5):
# (3 + 2 + 1) * 2^-25 + 2.5 * 2^-24 = 3.3e-7 if every rounding aligns; the green channel, the only one with three terms, has chroma terms
# below 0.5 (2^-26 each, coefficients 1.45 * 2^-24), which brings the worst channel to 2.4e-7.  The bound asserted is 3e-7.
FP32_DECODE_BOUND = 3e-7


def _frames(kind):
    return 0.1 + 0.8 * synthetic_frames(5, 134, 522, seed=5, kind=kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("matrix,full_range", R.PRESETS)
def test_helpers_agree_with_the_reference_to_the_last_code(kind, matrix, full_range):
    x = _frames(kind)
    want = R.encode(x.numpy(), matrix, full_range)
    got = nv12.rgb_to_nv12(x.double(), matrix, full_range)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (5, 201, 522)
    assert np.array_equal(got.numpy(), want)
    got32 = nv12.rgb_to_nv12(x, matrix, full_range)
    # fp32 arithmetic may only move a code whose float64 value lies on a rounding boundary (distance < 1e-3 of x.5)
    v = R.encode_values(x.numpy(), matrix, full_range)
    off = got32.numpy() != want
    assert np.all(np.abs(v[off] - np.floor(v[off]) - 0.5) < 1e-3) and off.mean() < 1e-4
    rgb_ref = R.decode(want, matrix, full_range)
    rgb64 = nv12.nv12_to_rgb(torch.from_numpy(want), matrix, full_range, dtype=torch.float64)
    rgb32 = nv12.nv12_to_rgb(torch.from_numpy(want), matrix, full_range)
    assert np.abs(rgb64.numpy() - rgb_ref).max() < 1e-12
    assert np.abs(rgb32.double().numpy() - rgb_ref).max() <= FP32_DECODE_BOUND


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("matrix,full_range", R.PRESETS)
def test_identity_on_the_cpu(kind, matrix, full_range):
    c = torch.from_numpy(R.encode(_frames(kind).numpy(), matrix, full_range))
    assert np.array_equal(R.encode(R.decode(c.numpy(), matrix, full_range), matrix, full_range), c.numpy())      # the reference alone
    raw = R.decode(c.numpy(), matrix, full_range, clamp=False)
    assert raw.min() >= 0.0 and raw.max() <= 1.0, "a converted sample leaves [0, 1]"
    rgbs = {}
    for dt in (torch.float32, torch.float64):
        rgb = rgbs[dt] = nv12.nv12_to_rgb(c, matrix, full_range, dtype=dt)
        assert rgb.dtype == dt
        assert torch.equal(nv12.rgb_to_nv12(rgb.clamp(0, 1), matrix, full_range), c)
    assert (rgbs[torch.float32].double() - rgbs[torch.float64]).abs().max().item() <= FP32_DECODE_BOUND


def test_color_affine_is_an_inverse_pair():
    for matrix, full_range in R.PRESETS:
        fwd, inv = nv12.color_affine(matrix, full_range)
        assert fwd.dtype == np.float64 and inv.dtype == np.float64 and fwd.shape == (3, 4) and inv.shape == (3, 4)
        assert np.abs(inv[:, :3] @ fwd[:, :3] - np.eye(3)).max() < 1e-14
        assert np.abs(inv[:, :3] @ fwd[:, 3] + inv[:, 3]).max() < 1e-12
    with pytest.raises(ValueError):
        nv12.color_affine("bt2020", False)


def test_exports_are_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    declared = set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", header))
    for sym in ("vs_resize_pre_nv12", "vs_embed_tail_nv12", "vs_sizeof_tail_nv12_desc", "vs_model_set_nv12_color", "vs_nv12_default_color"):
        assert sym in native.EXPORTS and sym in declared, sym
    assert "vs_tail_nv12_desc_t" in header
    assert hasattr(native, "TailNv12Desc")
    lib = native.lib()
    assert lib.vs_sizeof_tail_nv12_desc() == __import__("ctypes").sizeof(native.TailNv12Desc)
    # argument validation happens on the host before any launch
    assert lib.vs_embed_tail_nv12(None, None) == -1
    assert lib.vs_resize_pre_nv12(None, 1, 8, 8, 8, 96, None, 4, 4, 1, None, 1.0, 0.0, None, 1, None, None) == -1


def test_c_default_colour_equals_color_affine_bit_for_bit():
    """the model-level C-ABI's default (BT.709 limited range, built in C++) is the pair of 12 floats `color_affine` gives, to the last bit"""
    import ctypes
    lib = native.lib()
    dec, enc = (ctypes.c_float * 12)(), (ctypes.c_float * 12)()
    assert lib.vs_nv12_default_color(dec, enc) == 0
    fwd, inv = nv12.color_affine("bt709", False)
    assert np.array_equal(np.array(list(dec), dtype=np.float32).view(np.uint32), inv.reshape(-1).astype(np.float32).view(np.uint32))
    assert np.array_equal(np.array(list(enc), dtype=np.float32).view(np.uint32), fwd.reshape(-1).astype(np.float32).view(np.uint32))
    assert lib.vs_nv12_default_color(None, enc) == -1


def test_videoseal_has_both_methods():
    assert callable(getattr(Videoseal, "embed_nv12", None)) and callable(getattr(Videoseal, "detect_nv12", None))
