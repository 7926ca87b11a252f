"""NV12 frames on the HIP path: vs_resize_pre_nv12 / vs_embed_tail_nv12, Videoseal.embed_nv12 / detect_nv12.

The reference is tests/_nv12_ref.py (float64 numpy, independent of videoseal_amd.nv12) and the project's own fp32 entry points.  Every clip
is a strided view of a larger, poisoned buffer:
  A = 5 x 134 x 202, pitch 256, frame stride > pitch * 201: chroma width 101 and chroma height 67 are odd
  B = 6 x 72 x 88, pitch 88: up-resize of the watermark below 2 x
  C = 3 x 134 x 522, pitch 523: odd pitch (unaligned rows), three 256-column tiles with a ragged last one, an 8 x down-scale in the resize
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
from tests import _nv12_ref as R  # noqa: E402
from tests._guards import GUARD  # noqa: E402
from tests._util import assert_decisions  # noqa: E402
from tests._model import TOL_IMG, TOL_LOGIT, make_model  # noqa: E402

from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import nv12  # noqa: E402
from videoseal_amd.yuv420 import Clip420  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 134, 202, 256, 7), "B": (6, 72, 88, 88, 0), "C": (3, 134, 522, 523, 3)}       # F, H, W, pitch, spare rows per frame
S = 64                                                                                          # img_size of the tiny models


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


def pitched(clip: torch.Tensor, pitch: int, spare: int, poison: int = 0xA5):
    """(buffer, view): `clip` [F, R, W] as a strided view (row stride `pitch`, `spare` unused rows after every frame) of a poisoned device
    buffer with GUARD bytes on either side"""
    F_, R_, W = clip.shape
    n = F_ * (R_ + spare) * pitch
    buf = torch.full((GUARD + n + GUARD,), poison, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:GUARD + n].view(F_, R_ + spare, pitch)[:, :R_, :W]
    view.copy_(clip.cuda())
    return buf, view


def padding_mask(F_, R_, W, pitch, spare):
    m = torch.ones(F_, R_ + spare, pitch, dtype=torch.bool, device="cuda")
    m[:, :R_, :W] = False
    return torch.cat([torch.ones(GUARD, dtype=torch.bool, device="cuda"), m.flatten(), torch.ones(GUARD, dtype=torch.bool, device="cuda")])


def clip_of(shape: str, preset, kind="smooth", seed=5, lo=0.0, hi=1.0) -> torch.Tensor:
    F_, H, W, _, _ = SHAPES[shape]
    x = lo + (hi - lo) * synthetic_frames(F_, H, W, seed=seed, kind=kind)
    return torch.from_numpy(R.encode(x.numpy(), *preset))


def random_clip(shape: str, seed=9) -> torch.Tensor:
    F_, H, W, _, _ = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (F_, H * 3 // 2, W), generator=g, dtype=torch.uint8)          # most (Y, Cb, Cr) triples are out of gamut


def call_resize(view, preset, aa, want_rgb, want_y, ymat, y_step=2, form=None, strip=0):
    """form "tile" keeps the tile kernel, `strip` sets the strip height of the row-streaming one (development switches RESIZE_FORM and RESIZE_STRIP)"""
    lib = N.lib()
    F_, R_, W = view.shape
    H = R_ // 3 * 2
    _, inv = nv12.color_affine(*preset)
    dec = (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)])
    rgb = torch.full((F_, S, S, 4), float("nan"), device="cuda") if want_rgb else None
    nk = (F_ + y_step - 1) // y_step
    key = torch.full((nk, S, S, 4), float("nan"), device="cuda") if want_y else None
    ym = (C.c_float * 3)(*ymat)
    with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", int(strip)):
        N.check(lib.vs_resize_pre_nv12(view.data_ptr(), F_, H, W, view.stride(1), view.stride(0), dec, S, S, int(aa), N.ptr(rgb), 2.0, -1.0,
                                       N.ptr(key), y_step, ym, None), "vs_resize_pre_nv12")
        torch.cuda.synchronize()
    return rgb, key


# ---------------------------------------------------------------------------------------------------- 1. vs_resize_pre_nv12
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_resize_pre_nv12_against_float64_interpolate(shape, aa):
    """max |delta| < 2e-6, the bound tests/test_gpu_kernels.py::test_resize_pre holds the fp32 kernel to; all four presets, dst_rgb and dst_y
    each alone and both, a uniformly random clip (out-of-gamut bytes: the clamp) next to a smooth one"""
    F_, H, W, pitch, spare = SHAPES[shape]
    ymat = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]
    worst = 0.0
    for preset in R.PRESETS:
        for clip in (clip_of(shape, preset), random_clip(shape)):
            x = R.decode(clip.numpy(), *preset)
            ref = F.interpolate(torch.from_numpy(x), size=(S, S), mode="bilinear", align_corners=False, antialias=aa)       # float64
            ref_rgb = (ref * 2.0 - 1.0).permute(0, 2, 3, 1)
            ref_y = ((ymat[0] * ref[:, 0] + ymat[1] * ref[:, 1] + ymat[2] * ref[:, 2]) * 2.0 - 1.0)[::2]
            buf, view = pitched(clip, pitch, spare)
            got = {}
            for want_rgb, want_y in ((True, False), (False, True), (True, True)):
                rgb, key = call_resize(view, preset, aa, want_rgb, want_y, ymat)
                if want_rgb:
                    assert torch.all(rgb[..., 3] == 0)
                    e = (rgb[..., :3].cpu().double() - ref_rgb).abs().max().item()
                    worst = max(worst, e)
                    assert e < 2e-6, (shape, aa, preset, "rgb", e)
                    assert got.setdefault("rgb", rgb).equal(rgb)                   # alone and together: the same bits
                if want_y:
                    assert torch.all(key[..., 1:] == 0)
                    e = (key[..., 0].cpu().double() - ref_y).abs().max().item()
                    worst = max(worst, e)
                    assert e < 2e-6, (shape, aa, preset, "y", e)
                    assert got.setdefault("y", key).equal(key)
            # the forms agree bit for bit: tile kernel, row-streaming kernel (A and B admit it) at its own and at odd strip heights
            for form, strip in (("tile", 0), (None, 5), (None, 22)):
                rgb, key = call_resize(view, preset, aa, True, True, ymat, form=form, strip=strip)
                assert rgb.equal(got["rgb"]) and key.equal(got["y"]), (shape, aa, preset, form, strip)
    print(f"resize_pre_nv12 {shape} antialias={aa}: max |delta| = {worst:.2e}")


def test_resize_pre_nv12_random_clip_is_out_of_gamut():
    raw = R.decode(random_clip("A").numpy(), "bt709", False, clamp=False)
    assert raw.min() < -0.1 and raw.max() > 1.1           # the clamp is exercised by the random clips of the test above


# ---------------------------------------------------------------------------------------------------- 2. embed_nv12 against the composition
def _composition_values(model, clip, msgs, preset, lowres):
    rgb = nv12.nv12_to_rgb(clip, *preset).cuda()                                        # fp32
    w = model.embed(rgb, msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
    return w, R.encode_values(w.cpu().double().numpy(), *preset)


@pytest.mark.parametrize("shape", ["A", "B", "C"])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_embed_nv12_equals_the_composition(which, shape, tiny, tinyc):
    """every output code lies within 0.5 + 255 * TOL_IMG of the float64 code value of the fp32 composition; lowres on / off, the three
    video modes, attenuation on / off, step_size 2 (F = 5 and F = 3 are no multiples of it), the presets in turn"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    F_, H, W, pitch, spare = SHAPES[shape]
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    att0 = model.attenuation
    model.chunk_size, model.step_size = 2, 2
    worst = 0.0
    try:
        for i, (lowres, mode, att) in enumerate(itertools.product((True, False), ("repeat", "alternate", "interpolate"), (True, False))):
            preset = R.PRESETS[i % 4]
            model.video_mode = mode
            model.attenuation = att0 if att else None
            clip = clip_of(shape, preset, seed=20 + i)
            buf, view = pitched(clip, pitch, spare)
            _, v = _composition_values(model, clip, msgs, preset, lowres)
            outs = []
            for variant in (0, 1):                    # default (the row-streaming tail where it applies: A and C) and the tile kernel
                model._engine().tail_variant = variant
                out = model.embed_nv12(view, msgs, lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])["imgs_w"]
                model._engine().tail_variant = 0
                assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == view.shape and out.is_cuda
                err = np.abs(out.cpu().numpy().astype(np.float64) - v).max()
                worst = max(worst, err)
                assert err <= 0.5 + 255 * TOL_IMG, (which, shape, lowres, mode, att, preset, variant, err)
                assert not torch.equal(out.cpu(), clip)        # the watermark is there
                outs.append(out)
            if lowres or not att:                     # without the full-resolution heat-map both forms evaluate the same expressions
                assert torch.equal(outs[0], outs[1]), (which, shape, lowres, mode, att)
    finally:
        model._engine().tail_variant = 0
        model.attenuation = att0
        model.video_mode = "repeat"
    print(f"embed_nv12 {which} {shape}: max |code - v| = {worst:.4f}")


# ---------------------------------------------------------------------------------------------------- 3. chroma is left alone
@pytest.mark.parametrize("lowres", [True, False])
@pytest.mark.parametrize("shape", ["A", "C"])
def test_yuv_embedder_leaves_chroma_alone(shape, lowres, tiny):
    """the yuv embedder adds one value to R, G and B alike: wherever the fp32 composition clamps none of a block's 12 values the block's
    (Cb, Cr) come back exactly.  Catches swapped Cb / Cr, a chroma row or pitch off by one, a tile starting on an odd row."""
    spec, sd, model = tiny
    F_, H, W, pitch, spare = SHAPES[shape]
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=8)
    for preset in (R.PRESETS[2], R.PRESETS[1]):
        clip = clip_of(shape, preset, kind="noise", seed=31, lo=0.3, hi=0.7)
        buf, view = pitched(clip, pitch, spare)
        rgb = nv12.nv12_to_rgb(clip, *preset)
        w = model.embed(rgb.cuda(), msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"].cpu()
        inside = ((w > 0) & (w < 1) & (rgb > 0) & (rgb < 1)).all(dim=1)                             # [F, H, W]: no channel clamped
        blocks = inside.reshape(F_, H // 2, 2, W // 2, 2).all(dim=4).all(dim=2)                      # [F, H/2, W/2]
        assert blocks.float().mean().item() >= 0.99
        cin = clip[:, H:].reshape(F_, H // 2, W // 2, 2)
        for variant in (0, 1):                        # row-streaming tail, tile tail
            model._engine().tail_variant = variant
            try:
                out = model.embed_nv12(view, msgs, lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])["imgs_w"].cpu()
            finally:
                model._engine().tail_variant = 0
            cout = out[:, H:].reshape(F_, H // 2, W // 2, 2)
            assert torch.equal(cin[blocks], cout[blocks]), (preset, variant)
            assert not torch.equal(out[:, :H], clip[:, :H])          # luma carries the watermark


# ---------------------------------------------------------------------------------------------------- 4. identity
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("shape", ["A", "C"])
def test_identity_without_a_watermark(shape, kind, tiny):
    spec, sd, model = tiny
    F_, H, W, pitch, spare = SHAPES[shape]
    x = (0.1 + 0.8 * synthetic_frames(5, 134, 522, seed=5, kind=kind))[:F_, :, :H, :W]
    att0, sw0 = model.attenuation, model.blender.scaling_w
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    try:
        model.attenuation = None
        model.blender.scaling_w = 0.0
        for preset in R.PRESETS:
            clip = torch.from_numpy(R.encode(x.numpy(), *preset))
            buf, view = pitched(clip, pitch, spare)
            for variant in (0, 1):
                model._engine().tail_variant = variant
                out = model.embed_nv12(view, matrix=preset[0], full_range=preset[1])["imgs_w"]
                assert torch.equal(out.cpu(), clip), (shape, kind, preset, variant)
    finally:
        model._engine().tail_variant = 0
        model.attenuation, model.blender.scaling_w = att0, sw0


# ---------------------------------------------------------------------------------------------------- 5. detect_nv12
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_detect_nv12(shape, tiny):
    spec, sd, model = tiny
    F_, H, W, pitch, spare = SHAPES[shape]
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    for i, preset in enumerate(R.PRESETS):
        clip = clip_of(shape, preset, seed=40 + i) if i % 2 == 0 else random_clip(shape, seed=40 + i)
        buf, view = pitched(clip, pitch, spare)
        for aa in (True, False):
            it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
            got = model.detect_nv12(view, interpolation=it, matrix=preset[0], full_range=preset[1])["preds"]
            want = model.detect(nv12.nv12_to_rgb(clip, *preset).cuda(), is_video=True, interpolation=it)["preds"]
            assert got.shape == (F_, spec.nbits + 1)
            assert (got - want).abs().max().item() < TOL_LOGIT
            assert_decisions(got, want, what=f"detect_nv12 {shape} {preset}", min_sure=0.99)
    # end to end: the watermarked NV12 clip through detect_nv12
    msgs = synthetic_msgs(1, spec.nbits, seed=9)
    buf, view = pitched(clip_of(shape, R.PRESETS[2]), pitch, spare)
    w = model.embed_nv12(view, msgs)["imgs_w"]
    got = model.detect_nv12(w)["preds"]
    want = model.detect(nv12.nv12_to_rgb(w.cpu()).cuda(), is_video=True)["preds"]
    assert (got - want).abs().max().item() < TOL_LOGIT
    assert_decisions(got, want, what=f"detect_nv12 of embed_nv12 {shape}", min_sure=0.99)


# ---------------------------------------------------------------------------------------------------- 6. red zones
@pytest.mark.parametrize("full_jnd", [True, False])
@pytest.mark.parametrize("shape", ["A", "C"])
def test_red_zones_and_pitch_padding(shape, full_jnd, tiny):
    """source and destination between guard bands with poisoned pitch padding: no byte outside the W columns of a destination row is
    written, and the value of the source's padding bytes reaches no result"""
    spec, sd, model = tiny
    eng = model._engine()
    color = ("bt709", False)
    F_, H, W, pitch, spare = SHAPES[shape]
    clip = clip_of(shape, R.PRESETS[2], kind="noise", seed=50)
    g = torch.Generator().manual_seed(51)
    delta = torch.tanh(torch.randn((F_ + 1) // 2, 1, S, S, generator=g)).cuda()
    hm = None if full_jnd else torch.rand(F_ * S * S, generator=g).cuda()
    dpitch = pitch + 5
    pad = padding_mask(F_, H * 3 // 2, W, dpitch, spare)
    results = []
    # (padding poison, tail form, strip height of the row-streaming tail): every combination gives the same bytes, except that the tile form
    # evaluates the full-resolution heat-map tap by tap (compared against the composition in the test above, not bit for bit here)
    for poison, variant, strip in ((0xA5, 0, 0), (0x3C, 0, 0), (0xA5, 0, 4), (0x3C, 0, 20)) + (() if full_jnd else ((0xA5, 1, 0),)):
        eng.tail_variant = variant
        sbuf, sview = pitched(clip, pitch, spare, poison)
        keep = sbuf.clone()
        dbuf, dview = pitched(torch.zeros_like(clip), dpitch, spare, 0x5A)
        with torch.cuda.device(eng.dev), N.debug("TAIL_STRIP", strip):
            src, dst = (Clip420(nv12.planes(v), "nv12", color) for v in (sview, dview))      # the planes are views of the pitched buffers
            rgb, key = eng.resize_pre(src, (S, S), True, want_rgb=True, want_key=True, key_step=2, tag="t.nv12")
            res = [rgb.t.clone(), key.t.clone()]
            eng.embed_tail(src, dst, delta, step=2, video_mode=2, hmap_low=hm, attenuate=True, clamp=True, antialias=True,
                           scaling_i=1.0, scaling_w=0.2)
        torch.cuda.synchronize()
        eng.tail_variant = 0
        assert torch.equal(sbuf, keep)                                        # the source is read only
        assert torch.all(dbuf[pad] == 0x5A)                                   # guards, pitch padding and spare rows of the destination
        assert not torch.equal(dview.cpu(), clip)
        results.append(res + [dview.clone()])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


def call_tail(sview, dview, delta, hm, eng, preset, variant, frame_strides=None):
    """vs_embed_tail_nv12 on two single-buffer views; returns the entry point's code.  variant 1 = the tile kernel, 4 = the row-streaming one"""
    F_, R_, W = sview.shape
    fwd, inv = nv12.color_affine(*preset)
    d = N.TailNv12Desc()
    d.imgs, d.out, d.preds_w = sview.data_ptr(), dview.data_ptr(), None
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(eng.taps43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, R_ // 3 * 2, W, delta.shape[-2], delta.shape[-1], delta.shape[1]
    d.step, d.video_mode, d.total_key = 2, 2, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = 1, 1, 1
    d.scaling_i, d.scaling_w = 1.0, 0.2
    d.variant = variant
    d.src_pitch, d.dst_pitch = sview.stride(1), dview.stride(1)
    d.src_frame_stride, d.dst_frame_stride = frame_strides or (sview.stride(0), dview.stride(0))
    d.yuv2rgb12 = (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)])
    d.rgb2yuv12 = (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])
    with torch.cuda.device(eng.dev):
        rc = N.lib().vs_embed_tail_nv12(C.byref(d), N.stream())
        torch.cuda.synchronize()
    return rc


def test_misaligned_chroma_plane_and_unequal_pitches(tiny):
    """The single-buffer entry points place the chroma plane at base + H * pitch.  2 x 74 x 88 with source pitch 91 and destination pitch 93:
    H * pitch is 14 resp. 2 past a multiple of 16, so neither chroma plane starts on a 16-byte boundary, and the two buffers disagree on
    every row's alignment.  vs_resize_pre_nv12 (tile and row-streaming form) against float64 interpolation (2e-6, the bound of section 1),
    vs_embed_tail_nv12 (both forms, full-resolution and low-resolution heat-map) against the fp32 tail on the decoded clip (0.5 +
    255 * TOL_IMG, the bound of section 2); no padding or spare byte of either buffer changes."""
    spec, sd, model = tiny
    eng = model._engine()
    F_, H, W, spitch, dpitch, spare = 2, 74, 88, 91, 93, 2
    assert (H * spitch) % 16 == 14 and (H * dpitch) % 16 == 2
    preset = R.PRESETS[2]
    x = synthetic_frames(F_, H, W, seed=70, kind="noise")
    clip = torch.from_numpy(R.encode(x.numpy(), *preset))
    sbuf, sview = pitched(clip, spitch, spare)
    keep = sbuf.clone()
    # resize
    ymat = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]
    ref = F.interpolate(torch.from_numpy(R.decode(clip.numpy(), *preset)), size=(S, S), mode="bilinear", align_corners=False, antialias=True)
    ref_rgb = (ref * 2.0 - 1.0).permute(0, 2, 3, 1)
    ref_y = ((ymat[0] * ref[:, 0] + ymat[1] * ref[:, 1] + ymat[2] * ref[:, 2]) * 2.0 - 1.0)[::2]
    got = [call_resize(sview, preset, True, True, True, ymat, form=form) for form in ("tile", None)]
    for rgb, key in got:
        e_rgb, e_y = (rgb[..., :3].cpu().double() - ref_rgb).abs().max().item(), (key[..., 0].cpu().double() - ref_y).abs().max().item()
        print(f"resize_pre_nv12 pitch 91: max |delta| rgb {e_rgb:.2e}, y {e_y:.2e}")
        assert e_rgb < 2e-6 and e_y < 2e-6
    assert got[0][0].equal(got[1][0]) and got[0][1].equal(got[1][1])
    # tail: the watermark at 32 x 32, so that the row-streaming form applies (an up-scale by >= 2 in both directions)
    g = torch.Generator().manual_seed(71)
    delta = torch.tanh(torch.randn(1, 1, 32, 32, generator=g)).cuda()
    pad = padding_mask(F_, H * 3 // 2, W, dpitch, spare)
    rgb = nv12.nv12_to_rgb(clip, *preset).cuda()
    for hm in (None, torch.rand(F_ * 32 * 32, generator=g).cuda()):
        w = torch.empty_like(rgb)
        with torch.cuda.device(eng.dev):
            eng.embed_tail(rgb, w, delta, step=2, video_mode=2, hmap_low=hm, attenuate=True, clamp=True, antialias=True, scaling_i=1.0, scaling_w=0.2)
        v = R.encode_values(w.cpu().double().numpy(), *preset)
        outs = []
        for variant in (1, 4):
            dbuf, dview = pitched(torch.zeros_like(clip), dpitch, spare, 0x5A)
            assert call_tail(sview, dview, delta, hm, eng, preset, variant) == 0
            err = np.abs(dview.cpu().numpy().astype(np.float64) - v).max()
            print(f"embed_tail_nv12 pitch 91 -> 93, variant {variant}, {'full' if hm is None else 'low-resolution'} heat-map: max |code - v| = {err:.4f}")
            assert err <= 0.5 + 255 * TOL_IMG
            assert torch.all(dbuf[pad] == 0x5A)
            assert not torch.equal(dview.cpu(), clip)
            outs.append(dview.clone())
        if hm is not None:                            # without the full-resolution heat-map both forms evaluate the same expressions
            assert torch.equal(outs[0], outs[1])
    assert torch.equal(sbuf, keep)                    # the source is read only


# ---------------------------------------------------------------------------------------------------- 7. graphs
def test_nv12_graph_replay_matches_eager(tiny):
    spec, sd, model = tiny
    F_, H, W, pitch, spare = SHAPES["A"]
    model.chunk_size, model.step_size, model.video_mode = 8, 2, "repeat"          # (detect walks a clip in chunk_size frames: one chunk)
    outs = {}
    n0 = len(model._graphs)
    try:
        for use in (False, True):
            model.use_graphs = use
            res = []
            for seed in (1, 2, 3):
                buf, view = pitched(clip_of("A", R.PRESETS[2], seed=seed), pitch, spare)
                msgs = synthetic_msgs(1, spec.nbits, seed=seed)
                w = model.embed_nv12(view, msgs)["imgs_w"]
                res.append((w, model.detect_nv12(w)["preds"]))
            outs[use] = res
    finally:
        model.use_graphs = False
    assert len(model._graphs) == n0 + 2           # one embed graph + one detect graph, reused for the 3 clips
    for (w0, p0), (w1, p1) in zip(outs[False], outs[True]):
        assert torch.equal(w0, w1) and torch.equal(p0, p1)
    # another colour choice is another graph
    model.use_graphs = True
    try:
        model.detect_nv12(outs[True][0][0], matrix="bt601", full_range=True)
    finally:
        model.use_graphs = False
    assert len(model._graphs) == n0 + 3


# ---------------------------------------------------------------------------------------------------- 8. model-level C-ABI
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_model_level_c_api_nv12(which, tiny, tinyc):
    """vs_model_embed / vs_model_detect with io_u8 = 2 on a contiguous clip equal embed_nv12 / detect_nv12: codes equal, logits within 1e-4
    (the bound of the RGB24 twin in tests/test_gpu_e2e.py::test_model_level_c_api); default colour and vs_model_set_nv12_color"""
    from tests._model import cfg_of
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny if which == "tiny" else tinyc
    cm = CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=33)
    model.chunk_size, model.step_size, model.video_mode = 3, 2, "repeat"
    for preset in (R.PRESETS[2], R.PRESETS[1]):
        clip = clip_of("B", preset, seed=60).cuda()
        if preset != R.PRESETS[2]:
            cm.set_nv12_color(*preset)
        for lowres in (True, False):
            py = model.embed_nv12(clip, msgs, lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])["imgs_w"]
            c = cm.embed(clip, msgs, step=2, lowres_attenuation=lowres)
            assert c.dtype == torch.uint8 and c.shape == clip.shape and torch.equal(c, py)
        lp = model.detect_nv12(py, matrix=preset[0], full_range=preset[1])["preds"]
        assert (cm.detect(py) - lp).abs().max().item() < 1e-4
    # the RGB24 and fp32 formats are untouched by the NV12 colour choice
    imgs = synthetic_frames(6, 72, 88, seed=33)
    u8 = (imgs * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    assert torch.equal(cm.embed(u8, msgs, step=2, lowres_attenuation=True), CModel(cfg_of(spec), sd).embed(u8, msgs, step=2, lowres_attenuation=True))


# ---------------------------------------------------------------------------------------------------- 9. errors, empty and host-resident clips
def test_errors_empty_and_host_clips(tiny):
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    ok = clip_of("B", R.PRESETS[2]).cuda()
    msgs = synthetic_msgs(1, spec.nbits, seed=3)
    transposed = torch.zeros(6, 90, 108, dtype=torch.uint8, device="cuda").transpose(1, 2)      # [6, 108, 90] with a last stride of 108
    for bad in (ok[:, :107], ok[:, :, :87], ok.float(), transposed, ok[0]):          # odd H, odd W, fp32, transposed, rank 2
        with pytest.raises(ValueError):
            model.embed_nv12(bad, msgs)
        with pytest.raises(ValueError):
            model.detect_nv12(bad)
    with pytest.raises(ValueError):
        model.detect_nv12(ok, matrix="bt2020")
    e = model.embed_nv12(ok[:0], msgs)
    assert e["imgs_w"].shape == (0, 108, 88) and e["imgs_w"].dtype == torch.uint8 and e["msgs"].shape[0] == 0
    assert model.detect_nv12(ok[:0])["preds"].shape == (0, spec.nbits + 1)
    # a host-resident clip moves chunk by chunk and comes back on the host with the same codes
    dev = model.embed_nv12(ok, msgs)["imgs_w"]
    host = model.embed_nv12(ok.cpu(), msgs)["imgs_w"]
    assert not host.is_cuda and torch.equal(host, dev.cpu())
    assert torch.equal(model.detect_nv12(ok.cpu())["preds"], model.detect_nv12(ok)["preds"].cpu())


def test_frame_stride_must_hold_the_whole_buffer(tiny):
    """a frame of a single-buffer clip is pitch * (3H/2 - 1) + W bytes.  frame_stride = pitch * H holds the luma plane and the chroma plane
    each on its own (the rule of the plane entry points) but lets the chroma rows of a frame overlap the luma rows of the next: both entry
    points answer VS_ERR_BAD_ARG (-1), for the source and for the destination, before any launch"""
    spec, sd, model = tiny
    eng = model._engine()
    F_, H, W, pitch = 2, 8, 16, 16
    whole, planes_only = pitch * (H * 3 // 2), pitch * H
    src = torch.zeros(F_, H * 3 // 2, W, dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    dec = (C.c_float * 12)(*[float(v) for v in nv12.color_affine()[1].reshape(-1)])
    rgb = torch.zeros(F_, 4, 4, 4, device="cuda")

    def resize(frame_stride):
        return N.lib().vs_resize_pre_nv12(src.data_ptr(), F_, H, W, pitch, frame_stride, dec, 4, 4, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None)
    delta = torch.zeros(1, 1, 4, 4, device="cuda")
    hm = torch.ones(F_ * 16, device="cuda")
    assert resize(planes_only) == -1
    assert call_tail(src, dst, delta, hm, eng, nv12.DEFAULT_COLOR, 0, frame_strides=(planes_only, whole)) == -1
    assert call_tail(src, dst, delta, hm, eng, nv12.DEFAULT_COLOR, 0, frame_strides=(whole, planes_only)) == -1
    assert resize(whole) == 0 and call_tail(src, dst, delta, hm, eng, nv12.DEFAULT_COLOR, 0, frame_strides=(whole, whole)) == 0
    torch.cuda.synchronize()


def test_pixelwise_detector_is_refused(tiny, monkeypatch):
    spec, sd, model = tiny
    monkeypatch.setattr(type(model), "pixelwise", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        model.detect_nv12(clip_of("B", R.PRESETS[2]).cuda())
