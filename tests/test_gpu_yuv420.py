"""I420, P010 and yuv420p10 clips on the HIP path: vs_resize_pre_yuv420 / vs_embed_tail_yuv420, Videoseal.embed_yuv420 / detect_yuv420, the
model-level C-ABI.

References: tests/_yuv420_ref.py (float64 numpy, independent of videoseal_amd.yuv420), the NV12 entry points (layouts that hold the same
codes must give the same bits) and the project's own fp32 entry points.  Every plane is a strided view of its own poisoned buffer between
GUARD bands; the pitch differs per plane and is odd where the caller can express it (an 8-bit plane anywhere, a 16-bit plane at the C level).
  A = 5 x 134 x 202: chroma width 101 and chroma height 67 are odd          B = 6 x 72 x 88: up-resize of the watermark below 2 x
  C = 3 x 134 x 522: three 256-column tiles, a ragged last one, 8 : 1 resize   D = 2 x 18 x 34: a chroma row shorter than one 16-byte
  load, a frame smaller than one tile
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from oracle.weights import make_state_dict, tiny_spec  # noqa: E402
from tests import _yuv420_ref as R  # noqa: E402
from tests._guards import GUARD  # noqa: E402
from tests._util import assert_decisions  # noqa: E402
from tests._model import TOL_IMG, TOL_LOGIT, make_model  # noqa: E402

from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import yuv420  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 134, 202, 7), "B": (6, 72, 88, 0), "C": (3, 134, 522, 3), "D": (2, 18, 34, 1)}       # F, H, W, spare rows per frame
PADS = {"A": (54, 7, 12), "B": (0, 3, 8), "C": (1, 5, 2), "D": (13, 1, 6)}       # bytes between a row's end and the next row, per plane
S = 64                                                                          # img_size of the tiny models


@pytest.fixture(scope="module")
def tiny():
    s = tiny_spec()
    sd = make_state_dict(s, seed=3)
    return s, sd, make_model(s, sd)


@pytest.fixture(scope="module")
def tinyc():
    s = tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16)
    sd = make_state_dict(s, seed=4)
    return s, sd, make_model(s, sd)


def _t(planes):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)) for p in planes)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _np(planes):
    return tuple(p.cpu().contiguous().view(torch.uint8).numpy().view(np.uint16 if p.element_size() == 2 else np.uint8) for p in planes)


class Pitched:
    """a clip whose planes are strided views of their own poisoned device buffers.  `bviews`: the planes as bytes [F, R, row bytes] (what the
    C level sees: any pitch); `views`: the same memory as tensors of the planes' dtype (16-bit planes need `even` pads for that)"""

    def __init__(self, planes, shape, poison=0xA5, even=False, extra=0, fill=True):
        spare = SHAPES[shape][3]
        self.bufs, self.bviews, self.views, self.masks = [], [], [], []
        for p, pad in zip(planes, PADS[shape]):
            F_, R_, W = p.shape
            es = p.element_size()
            rowb = W * es
            pitch = rowb + (pad + extra) * (2 if (even and es == 2) else 1)
            n = F_ * (R_ + spare) * pitch
            buf = torch.full((GUARD + n + GUARD,), poison, dtype=torch.uint8, device="cuda")
            bv = buf[GUARD:GUARD + n].view(F_, R_ + spare, pitch)[:, :R_, :rowb]
            if fill:
                bv.copy_(p.contiguous().view(torch.uint8).view(F_, R_, rowb).cuda())
            m = torch.ones(F_, R_ + spare, pitch, dtype=torch.bool, device="cuda")
            m[:, :R_, :rowb] = False
            g = torch.ones(GUARD, dtype=torch.bool, device="cuda")
            self.bufs.append(buf)
            self.bviews.append(bv)
            self.views.append(bv if es == 1 else (bv.view(torch.uint16) if pitch % 2 == 0 else None))
            self.masks.append(torch.cat([g, m.flatten(), g]))
        self.views = tuple(self.views)

    def surface(self, fmt):
        planar, depth, msb = R.FORMATS[fmt]
        s = N.Yuv420Surface()
        for i, bv in enumerate(self.bviews):
            s.plane[i], s.pitch[i], s.frame_stride[i] = bv.data_ptr(), bv.stride(1), bv.stride(0)
        s.planar, s.depth, s.msb_aligned = int(planar), depth, int(msb)
        return s

    def planes_cpu(self, fmt):
        dt = np.uint8 if R.FORMATS[fmt][1] == 8 else np.uint16
        return tuple(np.ascontiguousarray(bv.cpu().numpy()).view(dt) for bv in self.bviews)


def frames_of(shape, kind="smooth", seed=5, lo=0.0, hi=1.0):
    F_, H, W, _ = SHAPES[shape]
    return lo + (hi - lo) * synthetic_frames(F_, H, W, seed=seed, kind=kind)


def clip_of(shape, fmt, preset, **kw):
    return R.encode(frames_of(shape, **kw).numpy(), fmt, *preset)


def random_clip(shape, fmt, seed=9):
    """uniformly random words: most (Y, Cb, Cr) triples are out of gamut, p010's low six bits are non-zero, yuv420p10 words pass 1023"""
    F_, H, W, _ = SHAPES[shape]
    planar, depth, _ = R.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    shapes = [(F_, H, W)] + ([(F_, H // 2, W // 2)] * 2 if planar else [(F_, H // 2, W)])
    return tuple(rng.integers(0, top, size=s).astype(dt) for s in shapes)


def aff(preset, depth):
    fwd, inv = yuv420.color_affine(preset[0], preset[1], depth)
    return (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)]), (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])


YMAT = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]


def _resize_outputs(F_, want_rgb, want_y, y_step):
    rgb = torch.full((F_, S, S, 4), float("nan"), device="cuda") if want_rgb else None
    key = torch.full(((F_ + y_step - 1) // y_step, S, S, 4), float("nan"), device="cuda") if want_y else None
    return rgb, key


def call_resize(pc: Pitched, fmt, shape, preset, aa, want_rgb=True, want_y=True, y_step=2, form=None, strip=0):
    """form "tile" keeps the tile kernel, `strip` sets the strip height of the row-streaming one (development switches RESIZE_FORM, RESIZE_STRIP)"""
    F_, H, W, _ = SHAPES[shape]
    rgb, key = _resize_outputs(F_, want_rgb, want_y, y_step)
    surf = pc.surface(fmt)
    with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", int(strip)):
        N.check(N.lib().vs_resize_pre_yuv420(C.byref(surf), F_, H, W, aff(preset, R.FORMATS[fmt][1])[0], S, S, int(aa), N.ptr(rgb), 2.0, -1.0,
                                             N.ptr(key), y_step, (C.c_float * 3)(*YMAT), None), "vs_resize_pre_yuv420")
        torch.cuda.synchronize()
    return rgb, key


def call_resize_nv12(planes, shape, preset, aa, y_step=2, form=None, strip=0):
    """the NV12 entry point on the one-buffer clip [F, 3H/2, W] at an odd pitch"""
    F_, H, W, spare = SHAPES[shape]
    clip = torch.from_numpy(np.concatenate(planes, axis=1))
    pitch = W + 2 * PADS[shape][0] + 1
    n = F_ * (H * 3 // 2 + spare) * pitch
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:GUARD + n].view(F_, H * 3 // 2 + spare, pitch)[:, :H * 3 // 2, :W]
    view.copy_(clip.cuda())
    rgb, key = _resize_outputs(F_, True, True, y_step)
    with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", int(strip)):
        N.check(N.lib().vs_resize_pre_nv12(view.data_ptr(), F_, H, W, view.stride(1), view.stride(0), aff(preset, 8)[0], S, S, int(aa), N.ptr(rgb),
                                           2.0, -1.0, N.ptr(key), y_step, (C.c_float * 3)(*YMAT), None), "vs_resize_pre_nv12")
        torch.cuda.synchronize()
    return rgb, key


FORMS = (("tile", 0), (None, 0), (None, 5), (None, 22))


# ---------------------------------------------------------------------------------------------------- 1. layout equivalence, bit for bit
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_resize_layout_twins_give_the_same_bits(shape, aa):
    """i420 through vs_resize_pre_yuv420 against its interleaved twin through vs_resize_pre_nv12, yuv420p10 against p010 (words shifted by
    6): dst_rgb and dst_y torch.equal in the tile form, the row-streaming form and at odd strip heights; smooth and random clips, the presets
    in turn"""
    for i, (form, strip) in enumerate(FORMS):
        for j, rnd in enumerate((False, True)):
            preset = R.PRESETS[(2 * i + j) % 6]
            i420 = random_clip(shape, "i420", seed=11 + i) if rnd else clip_of(shape, "i420", preset, seed=11 + i)
            want = call_resize_nv12(R.convert(i420, "i420", "nv12"), shape, preset, aa, form=form, strip=strip)
            got = call_resize(Pitched(_t(i420), shape), "i420", shape, preset, aa, form=form, strip=strip)
            via = call_resize(Pitched(_t(R.convert(i420, "i420", "nv12")), shape), "nv12", shape, preset, aa, form=form, strip=strip)
            for w, g, v in zip(want, got, via):
                assert torch.equal(w, g) and torch.equal(w, v), (shape, aa, form, strip, preset, rnd)
            p10 = clip_of(shape, "yuv420p10", preset, seed=11 + i)
            if rnd:
                p10 = tuple(np.minimum(p, 1023).astype(np.uint16) for p in random_clip(shape, "yuv420p10", seed=11 + i))
            a = call_resize(Pitched(_t(p10), shape), "yuv420p10", shape, preset, aa, form=form, strip=strip)
            b = call_resize(Pitched(_t(R.convert(p10, "yuv420p10", "p010")), shape), "p010", shape, preset, aa, form=form, strip=strip)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (shape, aa, form, strip, preset, rnd)
            assert not torch.isnan(a[0]).any() and not torch.isnan(a[1]).any() and torch.all(a[0][..., 3] == 0) and torch.all(a[1][..., 1:] == 0)


def _nv12_tensor(planes):
    return torch.from_numpy(np.concatenate(planes, axis=1)).cuda()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_embed_and_detect_layout_twins_give_the_same_bits(which, shape, tiny, tinyc):
    """embed_yuv420(i420) re-interleaved equals embed_nv12, embed_yuv420(yuv420p10) shifted by 6 equals embed_yuv420(p010), fmt="nv12" gives
    embed_nv12's bits; lowres on / off, the three video modes, attenuation on / off, step_size 2, both tail variants; the logits of
    detect_yuv420 are torch.equal too"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    F_, H, W, _ = SHAPES[shape]
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    att0 = model.attenuation
    model.chunk_size, model.step_size = 2, 2
    try:
        for i, (lowres, mode, att) in enumerate(itertools.product((True, False), ("repeat", "alternate", "interpolate"), (True, False))):
            preset = R.PRESETS[i % 4]                        # (embed_nv12 knows the two older matrices)
            any_preset = R.PRESETS[i % 6]
            kw = dict(lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])
            kw10 = dict(lowres_attenuation=lowres, matrix=any_preset[0], full_range=any_preset[1])
            model.video_mode = mode
            model.attenuation = att0 if att else None
            i420 = clip_of(shape, "i420", preset, seed=20 + i)
            nv = R.convert(i420, "i420", "nv12")
            p10 = clip_of(shape, "yuv420p10", any_preset, seed=20 + i)
            p010 = R.convert(p10, "yuv420p10", "p010")
            for variant in (0, 1):
                model._engine().tail_variant = variant
                want = model.embed_nv12(_nv12_tensor(nv), msgs, **kw)["imgs_w"]
                out = model.embed_yuv420(Pitched(_t(i420), shape).views, "i420", msgs, **kw)
                assert out["imgs_w"].is_contiguous() and out["imgs_w"].shape == (F_, H * W * 3 // 2) and out["planes_w"][1].shape == (F_, H // 2, W // 2)
                assert all(p.data_ptr() >= out["imgs_w"].data_ptr() for p in out["planes_w"])
                got = R.convert(_np(out["planes_w"]), "i420", "nv12")
                assert np.array_equal(np.concatenate(got, axis=1), want.cpu().numpy()), (which, shape, lowres, mode, att, variant)
                via = model.embed_yuv420(Pitched(_t(nv), shape).views, "nv12", msgs, **kw)["imgs_w"]
                assert torch.equal(via.view(F_, H * 3 // 2, W), want)
                a = model.embed_yuv420(Pitched(_t(p10), shape, even=True).views, "yuv420p10", msgs, **kw10)["planes_w"]
                b = model.embed_yuv420(Pitched(_t(p010), shape, even=True).views, "p010", msgs, **kw10)["planes_w"]
                assert all(np.array_equal(x, y) for x, y in zip(R.convert(_np(a), "yuv420p10", "p010"), _np(b))), (which, shape, lowres, mode, att, variant)
                assert all(int((y & 63).max()) == 0 for y in _np(b))
            model._engine().tail_variant = 0
            if i % 3 == 0:
                for aa in (True, False):
                    it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
                    dk = dict(interpolation=it, matrix=preset[0], full_range=preset[1])
                    want = model.detect_nv12(_nv12_tensor(nv), **dk)["preds"]
                    assert torch.equal(model.detect_yuv420(Pitched(_t(i420), shape).views, "i420", **dk)["preds"], want)
                    assert torch.equal(model.detect_yuv420(Pitched(_t(nv), shape).views, "nv12", **dk)["preds"], want)
                    dk = dict(interpolation=it, matrix=any_preset[0], full_range=any_preset[1])
                    assert torch.equal(model.detect_yuv420(Pitched(_t(p10), shape, even=True).views, "yuv420p10", **dk)["preds"],
                                       model.detect_yuv420(Pitched(_t(p010), shape, even=True).views, "p010", **dk)["preds"])
    finally:
        model._engine().tail_variant = 0
        model.attenuation = att0
        model.video_mode = "repeat"


# ---------------------------------------------------------------------------------------------------- 2. 10 bits against float64
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_resize_pre_p010_against_float64_interpolate(shape, aa):
    """max |delta| < 2e-6, the bound tests/test_gpu_kernels.py::test_resize_pre and the NV12 test hold this kernel body to; a smooth clip and a
    uniformly random-word clip (out-of-gamut triples: the clamp; non-zero low bits), at odd byte pitches, the presets in turn"""
    worst = 0.0
    for i, preset in enumerate(R.PRESETS):
        clip = random_clip(shape, "p010", seed=9 + i) if i % 2 else clip_of(shape, "p010", preset)
        x = R.decode(clip, "p010", *preset)
        ref = F.interpolate(torch.from_numpy(x), size=(S, S), mode="bilinear", align_corners=False, antialias=aa)       # float64
        ref_rgb = (ref * 2.0 - 1.0).permute(0, 2, 3, 1)
        ref_y = ((YMAT[0] * ref[:, 0] + YMAT[1] * ref[:, 1] + YMAT[2] * ref[:, 2]) * 2.0 - 1.0)[::2]
        rgb, key = call_resize(Pitched(_t(clip), shape), "p010", shape, preset, aa)
        e_rgb = (rgb[..., :3].cpu().double() - ref_rgb).abs().max().item()
        e_y = (key[..., 0].cpu().double() - ref_y).abs().max().item()
        worst = max(worst, e_rgb, e_y)
        print(f"resize_pre p010 {shape} antialias={aa} {preset}: max |delta| rgb {e_rgb:.2e}, y {e_y:.2e}")
        assert e_rgb < 2e-6 and e_y < 2e-6, (shape, aa, preset, e_rgb, e_y)
    raw = R.decode(random_clip("A", "p010"), "p010", "bt709", False, clamp=False)
    assert raw.min() < -0.1 and raw.max() > 1.1               # the clamp is exercised
    assert int((random_clip("A", "p010")[0] & 63).max()) > 0   # and so are the ignored bits


def _composition(model, planes, fmt, msgs, preset, lowres):
    rgb = yuv420.to_rgb(_t(planes), fmt, *preset).cuda()                               # fp32
    w = model.embed(rgb, msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
    return w, R.encode_values(w.cpu().double().numpy(), R.FORMATS[fmt][1], *preset)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_embed_p010_equals_the_composition(which, shape, tiny, tinyc):
    """every output code lies within 0.5 + 1023 * TOL_IMG of the float64 code value of the fp32 composition to_rgb -> embed -> encode_values,
    and the clip changed"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    att0 = model.attenuation
    model.chunk_size, model.step_size = 2, 2
    worst = 0.0
    try:
        for i, (lowres, mode, att) in enumerate(itertools.product((True, False), ("repeat", "alternate", "interpolate"), (True, False))):
            preset = R.PRESETS[i % 6]
            model.video_mode = mode
            model.attenuation = att0 if att else None
            clip = clip_of(shape, "p010", preset, seed=20 + i)
            _, v = _composition(model, clip, "p010", msgs, preset, lowres)
            for variant in (0, 1):
                model._engine().tail_variant = variant
                out = model.embed_yuv420(Pitched(_t(clip), shape, even=True).views, "p010", msgs, lowres_attenuation=lowres, matrix=preset[0],
                                         full_range=preset[1])["planes_w"]
                model._engine().tail_variant = 0
                assert all(p.dtype == torch.uint16 and p.is_cuda for p in out)
                for g, want in zip(R.codes_of(_np(out), "p010"), v):
                    err = np.abs(g.astype(np.float64) - want).max()
                    worst = max(worst, err)
                    assert err <= 0.5 + 1023 * TOL_IMG, (which, shape, lowres, mode, att, preset, variant, err)
                assert not np.array_equal(_np(out)[0], clip[0])
    finally:
        model._engine().tail_variant = 0
        model.attenuation = att0
        model.video_mode = "repeat"
    print(f"embed_yuv420 p010 {which} {shape}: max |code - v| = {worst:.4f}")


@pytest.mark.parametrize("fmt", ["p010", "yuv420p10", "i420"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_detect_yuv420(shape, fmt, tiny):
    spec, sd, model = tiny
    F_ = SHAPES[shape][0]
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    for i, preset in enumerate(R.PRESETS):
        clip = clip_of(shape, fmt, preset, seed=40 + i) if i % 2 == 0 else random_clip(shape, fmt, seed=40 + i)
        aa = i % 3 != 0
        it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
        got = model.detect_yuv420(Pitched(_t(clip), shape, even=True).views, fmt, interpolation=it, matrix=preset[0], full_range=preset[1])["preds"]
        want = model.detect(yuv420.to_rgb(_t(clip), fmt, *preset).cuda(), is_video=True, interpolation=it)["preds"]
        assert got.shape == (F_, spec.nbits + 1)
        assert (got - want).abs().max().item() < TOL_LOGIT
        assert_decisions(got, want, what=f"detect_yuv420 {fmt} {shape} {preset}", min_sure=0.99)
    # end to end: the watermarked clip through detect_yuv420
    msgs = synthetic_msgs(1, spec.nbits, seed=9)
    preset = R.PRESETS[4]
    kw = dict(matrix=preset[0], full_range=preset[1])
    w = model.embed_yuv420(Pitched(_t(clip_of(shape, fmt, preset)), shape, even=True).views, fmt, msgs, **kw)["planes_w"]
    got = model.detect_yuv420(w, fmt, **kw)["preds"]
    want = model.detect(yuv420.to_rgb(tuple(p.cpu() for p in w), fmt, *preset).cuda(), is_video=True)["preds"]
    assert (got - want).abs().max().item() < TOL_LOGIT
    assert_decisions(got, want, what=f"detect_yuv420 of embed_yuv420 {fmt} {shape}", min_sure=0.99)


# ---------------------------------------------------------------------------------------------------- 3. 10 bits keep what 8 bits drop
def test_ten_bits_keep_what_eight_bits_drop(tiny):
    """one clip (shape A, smooth), embed_yuv420(p010) and embed_nv12 of the same RGB frames, each against the unrounded fp32 composition in
    normalised units (code / scale): by the rounding rule the errors are <= 0.5 / 876 + TOL_IMG and about 0.5 / 219"""
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=12)
    preset = ("bt709", False)
    x = frames_of("A", seed=14).numpy()
    errs = {}
    for fmt, (ys, cs) in (("p010", (876.0, 896.0)), ("nv12", (219.0, 224.0))):
        clip = R.encode(x, fmt, *preset)
        _, v = _composition(model, clip, fmt, msgs, preset, True)
        if fmt == "nv12":
            out = model.embed_nv12(_nv12_tensor(clip), msgs)["imgs_w"].cpu().numpy()
            H = SHAPES["A"][1]
            got = R.codes_of((out[:, :H], out[:, H:]), "nv12")
        else:
            got = R.codes_of(_np(model.embed_yuv420(Pitched(_t(clip), "A", even=True).views, fmt, msgs)["planes_w"]), fmt)
        errs[fmt] = max(np.abs(g - want).max() / sc for g, want, sc in zip(got, v, (ys, cs, cs)))
    print(f"normalised max error: 10-bit {errs['p010']:.3e}, 8-bit {errs['nv12']:.3e}")
    assert errs["p010"] <= 0.5 / 876 + TOL_IMG
    assert errs["p010"] < errs["nv12"]


# ---------------------------------------------------------------------------------------------------- 4. chroma is left alone
@pytest.mark.parametrize("fmt", ["p010", "yuv420p10"])
@pytest.mark.parametrize("lowres", [True, False])
@pytest.mark.parametrize("shape", ["A", "C"])
def test_yuv_embedder_leaves_chroma_alone(shape, lowres, fmt, tiny):
    """the yuv embedder adds one value to R, G and B alike: wherever the fp32 composition clamps none of a block's 12 values the block's
    (Cb, Cr) come back exactly.  Catches swapped Cb / Cr or U / V, a chroma row or pitch off by one, a tile starting on an odd row."""
    spec, sd, model = tiny
    F_, H, W, _ = SHAPES[shape]
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=8)
    for preset in (R.PRESETS[2], R.PRESETS[1], R.PRESETS[4]):
        clip = clip_of(shape, fmt, preset, kind="noise", seed=31, lo=0.3, hi=0.7)
        rgb = yuv420.to_rgb(_t(clip), fmt, *preset)
        w = model.embed(rgb.cuda(), msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"].cpu()
        inside = ((w > 0) & (w < 1) & (rgb > 0) & (rgb < 1)).all(dim=1)                             # [F, H, W]: no channel clamped
        blocks = inside.reshape(F_, H // 2, 2, W // 2, 2).all(dim=4).all(dim=2).numpy()             # [F, H/2, W/2]
        assert blocks.mean() >= 0.99
        yin, cbin, crin = R.codes_of(clip, fmt)
        for variant in (0, 1):                        # row-streaming tail, tile tail
            model._engine().tail_variant = variant
            try:
                out = model.embed_yuv420(Pitched(_t(clip), shape, even=True).views, fmt, msgs, lowres_attenuation=lowres, matrix=preset[0],
                                         full_range=preset[1])["planes_w"]
            finally:
                model._engine().tail_variant = 0
            yo, cbo, cro = R.codes_of(_np(out), fmt)
            assert np.array_equal(cbin[blocks], cbo[blocks]) and np.array_equal(crin[blocks], cro[blocks]), (preset, variant)
            assert not np.array_equal(yo, yin)               # luma carries the watermark


# ---------------------------------------------------------------------------------------------------- 5. identity
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("shape", ["A", "C", "D"])
def test_identity_without_a_watermark(shape, kind, tiny):
    """scaling_w = 0, attenuation off: output words equal input words, all four formats, the six presets in turn, both tail variants"""
    spec, sd, model = tiny
    x = (0.1 + 0.8 * frames_of(shape, kind=kind)).numpy()
    att0, sw0 = model.attenuation, model.blender.scaling_w
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    try:
        model.attenuation = None
        model.blender.scaling_w = 0.0
        for k, fmt in enumerate(("nv12", "i420", "p010", "yuv420p10")):
            for j, variant in enumerate((0, 1)):
                for i in range(3):
                    preset = R.PRESETS[(2 * i + j + k) % 6]
                    clip = R.encode(x, fmt, *preset)
                    model._engine().tail_variant = variant
                    out = model.embed_yuv420(Pitched(_t(clip), shape, even=True).views, fmt, matrix=preset[0], full_range=preset[1])["planes_w"]
                    assert all(np.array_equal(a, b) for a, b in zip(_np(out), clip)), (shape, kind, fmt, preset, variant)
    finally:
        model._engine().tail_variant = 0
        model.attenuation, model.blender.scaling_w = att0, sw0


# ---------------------------------------------------------------------------------------------------- 6. red zones
def call_tail(src: Pitched, dst: Pitched, fmt, shape, preset, eng, delta, hm, variant):
    F_, H, W, _ = SHAPES[shape]
    d = N.TailYuv420Desc()
    d.src, d.dst = src.surface(fmt), dst.surface(fmt)
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(eng.taps43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, 1
    d.step, d.video_mode, d.total_key = 2, 2, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = 1, 1, 1
    d.scaling_i, d.scaling_w = 1.0, 0.2
    d.variant = variant
    d.yuv2rgb12, d.rgb2yuv12 = aff(preset, R.FORMATS[fmt][1])
    N.check(N.lib().vs_embed_tail_yuv420(C.byref(d), None), "vs_embed_tail_yuv420")
    torch.cuda.synchronize()


@pytest.mark.parametrize("full_jnd", [True, False])
@pytest.mark.parametrize("fmt", ["i420", "p010"])
@pytest.mark.parametrize("shape", ["A", "C", "D"])
def test_red_zones_and_pitch_padding(shape, fmt, full_jnd, tiny):
    """source and destination planes between guard bands with poisoned pitch padding (odd byte pitches, 16-bit planes included): the source
    is unchanged, no byte of a destination plane outside its rows' payload is written, and the value of the source padding reaches no result"""
    spec, sd, model = tiny
    eng = model._engine()
    preset = R.PRESETS[4]
    F_, H, W, _ = SHAPES[shape]
    clip = clip_of(shape, fmt, preset, kind="noise", seed=50)
    g = torch.Generator().manual_seed(51)
    delta = torch.tanh(torch.randn((F_ + 1) // 2, 1, S, S, generator=g)).cuda()
    hm = None if full_jnd else torch.rand(F_ * S * S, generator=g).cuda()
    results = []
    # (padding poison, tail form, strip height of the row-streaming tail): every combination gives the same bytes, except that the tile form
    # evaluates the full-resolution heat-map tap by tap (held to the composition above, not bit for bit here)
    for poison, variant, strip in ((0xA5, 0, 0), (0x3C, 0, 0), (0xA5, 0, 4), (0x3C, 0, 20)) + (() if full_jnd else ((0xA5, 1, 0),)):
        src = Pitched(_t(clip), shape, poison)
        keep = [b.clone() for b in src.bufs]
        dst = Pitched(_t(clip), shape, 0x5A, extra=4, fill=False)
        with torch.cuda.device(eng.dev), N.debug("TAIL_STRIP", strip):
            rgb, key = call_resize(src, fmt, shape, preset, True)
            call_tail(src, dst, fmt, shape, preset, eng, delta, hm, variant)
        assert all(torch.equal(a, b) for a, b in zip(src.bufs, keep))                            # the source is read only
        for buf, mask in zip(dst.bufs, dst.masks):
            assert torch.all(buf[mask] == 0x5A)                                                  # guards, pitch padding, spare rows
        out = dst.planes_cpu(fmt)
        assert not np.array_equal(out[0], clip[0])
        results.append([rgb, key] + [torch.from_numpy(o.astype(np.int32)) for o in out])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a.cpu(), b.cpu())


# ---------------------------------------------------------------------------------------------------- 7. graphs
def test_p010_graph_replay_matches_eager(tiny):
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 8, 2, "repeat"          # (detect walks a clip in chunk_size frames: one chunk)
    outs = {}
    n0 = len(model._graphs)
    try:
        for use in (False, True):
            model.use_graphs = use
            res = []
            for seed in (1, 2, 3):
                pc = Pitched(_t(clip_of("A", "p010", R.PRESETS[2], seed=seed)), "A", even=True)
                msgs = synthetic_msgs(1, spec.nbits, seed=seed)
                w = model.embed_yuv420(pc.views, "p010", msgs)
                res.append((w["imgs_w"], model.detect_yuv420(w["planes_w"], "p010")["preds"]))
            outs[use] = res
    finally:
        model.use_graphs = False
    assert len(model._graphs) == n0 + 2           # one embed graph + one detect graph, reused for the 3 clips
    for (w0, p0), (w1, p1) in zip(outs[False], outs[True]):
        assert torch.equal(w0.view(torch.uint8), w1.view(torch.uint8)) and torch.equal(p0, p1)
    # another colour choice is another graph, and so is another format of the same size
    model.use_graphs = True
    try:
        planes = yuv420.planes_of(outs[True][0][0], "p010", SHAPES["A"][1], SHAPES["A"][2])
        model.detect_yuv420(planes, "p010", matrix="bt2020", full_range=True)
        assert len(model._graphs) == n0 + 3
        model.detect_yuv420(planes, "p010", matrix="bt2020", full_range=True)
        assert len(model._graphs) == n0 + 3
    finally:
        model.use_graphs = False


# ---------------------------------------------------------------------------------------------------- 8. model-level C-ABI
@pytest.mark.parametrize("fmt", ["i420", "p010", "yuv420p10"])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_model_level_c_api_yuv420(which, fmt, tiny, tinyc):
    """vs_model_embed_yuv420 / vs_model_detect_yuv420 equal embed_yuv420 / detect_yuv420: words equal, logits within 1e-4 (the bound of the
    RGB24 and NV12 twins); NULL affines (the default colour) and an explicit bt2020 limited pair; pitched input and output surfaces"""
    from tests._model import cfg_of
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny if which == "tiny" else tinyc
    cm = CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=33)
    model.chunk_size, model.step_size, model.video_mode = 3, 2, "repeat"
    for color in (None, ("bt2020", False)):
        preset = color or ("bt709", False)
        clip = clip_of("B", fmt, preset, seed=60)
        for lowres in (True, False):
            src = Pitched(_t(clip), "B", even=True)
            py = model.embed_yuv420(src.views, fmt, msgs, lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])["planes_w"]
            dst = Pitched(_t(clip), "B", 0x5A, even=True, extra=3, fill=False)
            c = cm.embed_yuv420(src.views, fmt, msgs, out_planes=dst.views, color=color, step=2, lowres_attenuation=lowres)
            assert all(_same(a, b) for a, b in zip(py, c)), (which, fmt, color, lowres)
            for buf, mask in zip(dst.bufs, dst.masks):
                assert torch.all(buf[mask] == 0x5A)
            packed = cm.embed_yuv420(tuple(p.contiguous() for p in src.views), fmt, msgs, color=color, step=2, lowres_attenuation=lowres)
            assert all(_same(a, b) for a, b in zip(py, packed))
        lp = model.detect_yuv420(py, fmt, matrix=preset[0], full_range=preset[1])["preds"]
        assert (cm.detect_yuv420(dst.views, fmt, color=color) - lp).abs().max().item() < 1e-4


def test_c_level_refusals():
    lib = N.lib()
    clip = clip_of("D", "i420", R.PRESETS[2])
    pc = Pitched(_t(clip), "D")
    F_, H, W, _ = SHAPES["D"]
    rgb, _ = _resize_outputs(F_, True, False, 1)
    dec = aff(R.PRESETS[2], 8)[0]
    for planar, depth, msb in ((1, 10, 1), (0, 10, 0), (1, 12, 0), (0, 8, 1)):
        s = pc.surface("i420")
        s.planar, s.depth, s.msb_aligned = planar, depth, msb
        assert lib.vs_resize_pre_yuv420(C.byref(s), F_, H, W, dec, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == N.ERR_UNSUPPORTED
    s = pc.surface("i420")
    assert lib.vs_resize_pre_yuv420(C.byref(s), F_, H - 1, W, dec, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == -1
    assert lib.vs_resize_pre_yuv420(C.byref(s), F_, H, W - 1, dec, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == -1
    s.pitch[1] = W // 2 - 1                                       # a pitch shorter than the row
    assert lib.vs_resize_pre_yuv420(C.byref(s), F_, H, W, dec, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == -1
    d = N.TailYuv420Desc()
    d.src, d.dst = pc.surface("i420"), pc.surface("i420")
    delta = torch.zeros(1, 1, S, S, device="cuda")
    d.delta, d.F, d.H, d.W, d.S_h, d.S_w, d.Cd, d.step, d.total_key, d.clamp = N.ptr(delta), F_, H, W, S, S, 1, 2, 1, 1
    d.yuv2rgb12, d.rgb2yuv12 = aff(R.PRESETS[2], 8)
    d.attenuate = 2
    assert lib.vs_embed_tail_yuv420(C.byref(d), None) == N.ERR_UNSUPPORTED
    d.attenuate = 0
    d.preds_w = N.ptr(delta)
    assert lib.vs_embed_tail_yuv420(C.byref(d), None) == N.ERR_UNSUPPORTED
    d.preds_w = None
    d.variant = 2
    assert lib.vs_embed_tail_yuv420(C.byref(d), None) == N.ERR_UNSUPPORTED
    d.variant = 0
    d.dst.depth, d.dst.msb_aligned = 10, 1                        # the two surfaces hold different formats
    assert lib.vs_embed_tail_yuv420(C.byref(d), None) == N.ERR_UNSUPPORTED
    d.dst = pc.surface("i420")
    d.H = H - 1
    assert lib.vs_embed_tail_yuv420(C.byref(d), None) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 9. errors, empty and host-resident clips
def test_errors_empty_and_host_clips(tiny):
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=3)
    y, u, v = (p.cuda() for p in _t(clip_of("B", "i420", R.PRESETS[2])))
    y10, uv10 = (p.cuda() for p in _t(clip_of("B", "p010", R.PRESETS[2])))
    tr = torch.zeros(6, 44, 36, dtype=torch.uint8, device="cuda").transpose(1, 2)                  # [6, 36, 44] with a last stride of 44
    bad = [((y[:, :71], u, v), "i420"), ((y[:, :, :87], u, v), "i420"), ((y.float(), u, v), "i420"), ((y10, uv10), "nv12"), ((y, u, v), "yuv420p10"),
           ((y, u[:, :35], v), "i420"), ((y, u), "i420"), ((y, u, tr), "i420"), ((y, u, v.cpu()), "i420"), ((y, u, v), "yuv422p"), (y, "i420")]
    for planes, fmt in bad:
        with pytest.raises(ValueError):
            model.embed_yuv420(planes, fmt, msgs)
        with pytest.raises(ValueError):
            model.detect_yuv420(planes, fmt)
    with pytest.raises(ValueError):
        model.detect_yuv420((y, u, v), "i420", matrix="bt470")
    with pytest.raises(ValueError):
        model.detect_nv12(torch.zeros(2, 108, 88, dtype=torch.uint8, device="cuda"), matrix="bt2020")       # the NV12 methods keep their two matrices
    clamp0 = model.clamp
    try:
        model.clamp = False
        with pytest.raises(NotImplementedError):
            model.embed_yuv420((y, u, v), "i420", msgs)
    finally:
        model.clamp = clamp0
    e = model.embed_yuv420((y[:0], u[:0], v[:0]), "i420", msgs)
    assert e["imgs_w"].shape == (0, 72 * 88 * 3 // 2) and e["imgs_w"].dtype == torch.uint8 and e["msgs"].shape[0] == 0 and len(e["planes_w"]) == 3
    assert model.detect_yuv420((y10[:0], uv10[:0]), "p010")["preds"].shape == (0, spec.nbits + 1)
    # int16 planes are the same bits
    a = model.embed_yuv420((y10, uv10), "p010", msgs)["imgs_w"]
    b = model.embed_yuv420((y10.view(torch.int16), uv10.view(torch.int16)), "p010", msgs)["imgs_w"]
    assert a.dtype == torch.uint16 and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a host-resident clip moves chunk by chunk and comes back on the host with the same words
    for planes, fmt in (((y, u, v), "i420"), ((y10, uv10), "p010")):
        dev = model.embed_yuv420(planes, fmt, msgs)
        host = model.embed_yuv420(tuple(p.cpu() for p in planes), fmt, msgs)
        assert not host["imgs_w"].is_cuda and torch.equal(host["imgs_w"].view(torch.uint8), dev["imgs_w"].cpu().view(torch.uint8))
        assert all(not p.is_cuda for p in host["planes_w"])
        assert torch.equal(model.detect_yuv420(tuple(p.cpu() for p in planes), fmt)["preds"], model.detect_yuv420(planes, fmt)["preds"].cpu())


def test_pixelwise_detector_is_refused(tiny, monkeypatch):
    spec, sd, model = tiny
    monkeypatch.setattr(type(model), "pixelwise", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        model.detect_yuv420(tuple(p.cuda() for p in _t(clip_of("B", "i420", R.PRESETS[2]))), "i420")
