"""4:2:2 and 4:4:4 clips on the HIP path: vs_resize_pre_yuv / vs_embed_tail_yuv, Videoseal.embed_yuv / detect_yuv, the model-level C-ABI.

References: tests/_yuv_ref.py (float64 numpy, independent of videoseal_amd.yuv), the 4:2:0 entry points (a 4:2:0 clip and its twin with every
block's chroma replicated decode to the same RGB, so they must give the same bits wherever only RGB matters) and the project's own fp32 entry
points.  Every plane is a strided view of its own poisoned buffer between GUARD bands; the pitch differs per plane and is odd where the caller
can express it (an 8-bit plane anywhere, a 16-bit plane at the C level).
  A = 5 x 134 x 202: 4:2:2 chroma width 101 is odd                          B = 6 x 72 x 88: up-resize of the watermark below 2 x
  C = 3 x 134 x 522: three 256-column tiles, a ragged last one, 8 : 1 resize   D = 2 x 18 x 34: a chroma row shorter than one 16-byte load,
  a frame smaller than one tile      E = 3 x 67 x 202: odd H, tile forms      G = 2 x 131 x 259 (4:4:4 only): odd H and W, row-streaming
  forms (H, W >= 2 S), a partial last piece in every row
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
from tests import _yuv_ref as R  # noqa: E402
from tests._guards import GUARD  # noqa: E402
from tests._util import assert_decisions  # noqa: E402
from tests._model import TOL_IMG, TOL_LOGIT, make_model  # noqa: E402

from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import yuv  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 134, 202, 7), "B": (6, 72, 88, 0), "C": (3, 134, 522, 3), "D": (2, 18, 34, 1), "E": (3, 67, 202, 5),
          "G": (2, 131, 259, 2)}                                                 # F, H, W, spare rows per frame
PADS = {"A": (54, 7, 12), "B": (0, 3, 8), "C": (1, 5, 2), "D": (13, 1, 6), "E": (9, 5, 3), "G": (11, 2, 7)}       # bytes after a row's end, per plane
S = 64                                                                          # img_size of the tiny models
EVEN = ("A", "B", "C", "D")                                                     # shapes a 4:2:0 clip can have
F422 = ("yuv422p", "yuv422p10", "nv16", "p210")
F444 = ("yuv444p", "yuv444p10")
TWINS8, TWINS10 = ("yuv422p", "nv16", "yuv444p"), ("yuv422p10", "p210", "yuv444p10")


def shapes_of(fmt, names="ABCDEG"):
    """the shapes of `names` that `fmt` can have"""
    _, _, _, sx, sy = R.FORMATS[fmt]
    return [n for n in names if SHAPES[n][1] % (1 << sy) == 0 and SHAPES[n][2] % (1 << sx) == 0]


def cases(fmts, names="ABCDEG"):
    return [(f, n) for f in fmts for n in shapes_of(f, names)]


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


def depth_of(fmt):
    return R.FORMATS[fmt][1]


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

    def surface(self, fmt, old=False):
        """vs_yuv_surface_t of the planes; old: vs_yuv420_surface_t (a 4:2:0 format through the _yuv420 entry points)"""
        planar, depth, msb, sx, sy = R.FORMATS[fmt]
        s = N.Yuv420Surface() if old else N.YuvSurface()
        for i, bv in enumerate(self.bviews):
            s.plane[i], s.pitch[i], s.frame_stride[i] = bv.data_ptr(), bv.stride(1), bv.stride(0)
        s.planar, s.depth, s.msb_aligned = int(planar), depth, int(msb)
        if not old:
            s.chroma = {(1, 1): 420, (1, 0): 422, (0, 0): 444}[(sx, sy)]
        return s

    def planes_cpu(self, fmt):
        dt = np.uint8 if depth_of(fmt) == 8 else np.uint16
        return tuple(np.ascontiguousarray(bv.cpu().numpy()).view(dt) for bv in self.bviews)


def frames_of(shape, kind="smooth", seed=5, lo=0.0, hi=1.0):
    F_, H, W, _ = SHAPES[shape]
    return lo + (hi - lo) * synthetic_frames(F_, H, W, seed=seed, kind=kind)


def clip_of(shape, fmt, preset, **kw):
    return R.encode(frames_of(shape, **kw).numpy(), fmt, *preset)


def random_clip(shape, fmt, seed=9):
    """uniformly random words: most (Y, Cb, Cr) triples are out of gamut, msb-aligned words carry non-zero low bits, the others pass 1023"""
    F_, H, W, _ = SHAPES[shape]
    planar, depth, _, sx, sy = R.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    shapes = [(F_, H, W)] + ([(F_, H >> sy, W >> sx)] * 2 if planar else [(F_, H >> sy, W)])
    return tuple(rng.integers(0, top, size=s).astype(dt) for s in shapes)


def aff(preset, depth):
    fwd, inv = yuv.color_affine(preset[0], preset[1], depth)
    return (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)]), (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])


YMAT = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]
FORMS = (("tile", 0), (None, 0), (None, 5), (None, 22))


def call_resize(pc: Pitched, fmt, shape, preset, aa, y_step=2, form=None, strip=0, old=False):
    """vs_resize_pre_yuv (old: vs_resize_pre_yuv420).  form "tile" keeps the tile kernel, `strip` sets the strip height of the row-streaming
    one (development switches RESIZE_FORM, RESIZE_STRIP)"""
    F_, H, W, _ = SHAPES[shape]
    rgb = torch.full((F_, S, S, 4), float("nan"), device="cuda")
    key = torch.full(((F_ + y_step - 1) // y_step, S, S, 4), float("nan"), device="cuda")
    surf = pc.surface(fmt, old)
    fn = N.lib().vs_resize_pre_yuv420 if old else N.lib().vs_resize_pre_yuv
    with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", int(strip)):
        N.check(fn(C.byref(surf), F_, H, W, aff(preset, depth_of(fmt))[0], S, S, int(aa), N.ptr(rgb), 2.0, -1.0, N.ptr(key), y_step,
                   (C.c_float * 3)(*YMAT), None), "vs_resize_pre_yuv")
        torch.cuda.synchronize()
    return rgb, key


# ---------------------------------------------------------------------------------------------------- 1. replication twins, bit for bit
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("shape", EVEN)
def test_resize_replication_twins_give_the_same_bits(shape, aa):
    """a 4:2:0 clip through vs_resize_pre_yuv420 against its 4:2:2 and 4:4:4 twins (every block's chroma replicated) through
    vs_resize_pre_yuv: dst_rgb and dst_y torch.equal in the tile form, the row-streaming form and at odd strip heights; smooth and
    random-word clips, planar and interleaved originals, the presets in turn.  A 4:2:0 surface through vs_resize_pre_yuv gives the same."""
    for i, (form, strip) in enumerate(FORMS):
        for j, rnd in enumerate((False, True)):
            preset = R.PRESETS[(2 * i + j) % 6]
            kw = dict(form=form, strip=strip)
            for src, other, twins in (("i420", "nv12", TWINS8), ("yuv420p10", "p010", TWINS10)):
                clip = random_clip(shape, src, seed=11 + i) if rnd else clip_of(shape, src, preset, seed=11 + i)
                if (i + j) % 2:                                            # the interleaved original holds the same codes
                    orig, ofmt = R.convert(clip, src, other), other
                else:
                    orig, ofmt = clip, src
                want = call_resize(Pitched(_t(orig), shape), ofmt, shape, preset, aa, old=True, **kw)
                assert not torch.isnan(want[0]).any() and not torch.isnan(want[1]).any()
                via = call_resize(Pitched(_t(orig), shape), ofmt, shape, preset, aa, **kw)
                assert torch.equal(via[0], want[0]) and torch.equal(via[1], want[1]), (shape, aa, form, strip, ofmt)
                for dst in twins:
                    got = call_resize(Pitched(_t(R.replicate(clip, src, dst)), shape), dst, shape, preset, aa, **kw)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (shape, aa, form, strip, preset, rnd, dst)


@pytest.mark.parametrize("shape", EVEN)
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_embed_and_detect_replication_twins(which, shape, tiny, tinyc):
    """the luma plane of embed_yuv(twin) equals the luma plane of embed_yuv420(original) word for word, detect_yuv(twin) is torch.equal to
    detect_yuv420(original); lowres on / off, the three video modes, attenuation on / off, step_size 2, both tail variants; the twin formats
    and the original's layout in turn, smooth and random-word clips.  A 4:2:0 fmt through embed_yuv / detect_yuv equals the _yuv420 methods."""
    spec, sd, model = tiny if which == "tiny" else tinyc
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    att0 = model.attenuation
    model.chunk_size, model.step_size = 2, 2
    try:
        for i, (lowres, mode, att) in enumerate(itertools.product((True, False), ("repeat", "alternate", "interpolate"), (True, False))):
            preset = R.PRESETS[i % 6]
            kw = dict(lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])
            model.video_mode = mode
            model.attenuation = att0 if att else None
            pairs = []
            for src, other, twins, k in (("i420", "nv12", TWINS8, i), ("yuv420p10", "p010", TWINS10, i + 1)):
                clip = random_clip(shape, src, seed=20 + i) if i % 4 == 3 else clip_of(shape, src, preset, seed=20 + i)
                orig, ofmt = (R.convert(clip, src, other), other) if i % 2 else (clip, src)
                pairs.append((orig, ofmt, R.replicate(clip, src, twins[k % 3]), twins[k % 3]))
            for variant in (0, 1):
                model._engine().tail_variant = variant
                for orig, ofmt, twin, tfmt in pairs:
                    want = model.embed_yuv420(Pitched(_t(orig), shape, even=True).views, ofmt, msgs, **kw)
                    got = model.embed_yuv(Pitched(_t(twin), shape, even=True).views, tfmt, msgs, **kw)
                    gy, wy = _np(got["planes_w"])[0], _np(want["planes_w"])[0]
                    if R.FORMATS[ofmt][2] != R.FORMATS[tfmt][2]:            # p010 / p210 words are the other layout's words << 6
                        gy, wy = (a >> 6 if R.FORMATS[f][2] else a for a, f in ((gy, tfmt), (wy, ofmt)))
                        assert all(int((p & 63).max()) == 0 for p, f in ((_np(got["planes_w"])[0], tfmt), (_np(want["planes_w"])[0], ofmt)) if R.FORMATS[f][2])
                    assert np.array_equal(gy, wy), (which, shape, lowres, mode, att, variant, ofmt, tfmt)
                    assert got["imgs_w"].is_contiguous() and got["imgs_w"].shape == (SHAPES[shape][0], yuv.frame_samples(tfmt, *SHAPES[shape][1:3]))
                    if variant == 0 and i % 4 == 0:
                        via = model.embed_yuv(Pitched(_t(orig), shape, even=True).views, ofmt, msgs, **kw)
                        assert _same(via["imgs_w"], want["imgs_w"]) and torch.equal(via["msgs"], want["msgs"])
            model._engine().tail_variant = 0
            if i % 3 == 0:
                for aa in (True, False):
                    it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
                    dk = dict(interpolation=it, matrix=preset[0], full_range=preset[1])
                    for orig, ofmt, twin, tfmt in pairs:
                        want = model.detect_yuv420(Pitched(_t(orig), shape, even=True).views, ofmt, **dk)["preds"]
                        assert torch.equal(model.detect_yuv(Pitched(_t(twin), shape, even=True).views, tfmt, **dk)["preds"], want), (ofmt, tfmt)
                        assert torch.equal(model.detect_yuv(Pitched(_t(orig), shape, even=True).views, ofmt, **dk)["preds"], want), ofmt
    finally:
        model._engine().tail_variant = 0
        model.attenuation = att0
        model.video_mode = "repeat"


# ---------------------------------------------------------------------------------------------------- 2. layout twins
@pytest.mark.parametrize("shape", shapes_of("nv16"))
def test_layout_twins_give_the_same_bits(shape, tiny):
    """nv16 against yuv422p, p210 against yuv422p10 (words shifted by 6): resize outputs, embed words and logits equal bit for bit, p210
    output has zero low bits"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    att0 = model.attenuation
    model.chunk_size, model.step_size = 2, 2
    try:
        for i, (form, strip) in enumerate(FORMS):
            for j, rnd in enumerate((False, True)):
                preset = R.PRESETS[(2 * i + j) % 6]
                for pl, il in (("yuv422p", "nv16"), ("yuv422p10", "p210")):
                    clip = random_clip(shape, pl, seed=13 + i) if rnd else clip_of(shape, pl, preset, seed=13 + i)
                    if rnd and pl == "yuv422p10":
                        clip = tuple(np.minimum(p, 1023).astype(np.uint16) for p in clip)
                    twin = R.convert(clip, pl, il)
                    if il == "p210":
                        assert np.array_equal(twin[0], clip[0].astype(np.uint16) << 6)
                    a = call_resize(Pitched(_t(clip), shape), pl, shape, preset, i % 2 == 0, form=form, strip=strip)
                    b = call_resize(Pitched(_t(twin), shape), il, shape, preset, i % 2 == 0, form=form, strip=strip)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (shape, form, strip, preset, rnd, pl)
                    assert not torch.isnan(a[0]).any() and torch.all(a[0][..., 3] == 0) and torch.all(a[1][..., 1:] == 0)
        for i, (lowres, mode, att) in enumerate(itertools.product((True, False), ("repeat", "alternate", "interpolate"), (True, False))):
            preset = R.PRESETS[(i + 1) % 6]
            kw = dict(lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])
            model.video_mode = mode
            model.attenuation = att0 if att else None
            pl, il = (("yuv422p", "nv16"), ("yuv422p10", "p210"))[i % 2]
            clip = clip_of(shape, pl, preset, seed=23 + i)
            twin = R.convert(clip, pl, il)
            for variant in (0, 1):
                model._engine().tail_variant = variant
                a = model.embed_yuv(Pitched(_t(clip), shape, even=True).views, pl, msgs, **kw)["planes_w"]
                b = model.embed_yuv(Pitched(_t(twin), shape, even=True).views, il, msgs, **kw)["planes_w"]
                assert all(np.array_equal(x, y) for x, y in zip(R.convert(_np(a), pl, il), _np(b))), (shape, lowres, mode, att, variant, pl)
                if il == "p210":
                    assert all(int((y & 63).max()) == 0 for y in _np(b))
            model._engine().tail_variant = 0
            if i % 4 == 0:
                dk = dict(matrix=preset[0], full_range=preset[1])
                assert torch.equal(model.detect_yuv(Pitched(_t(clip), shape, even=True).views, pl, **dk)["preds"],
                                   model.detect_yuv(Pitched(_t(twin), shape, even=True).views, il, **dk)["preds"])
    finally:
        model._engine().tail_variant = 0
        model.attenuation = att0
        model.video_mode = "repeat"


# ---------------------------------------------------------------------------------------------------- 3. against float64
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("fmt,shape", cases(("yuv444p10", "p210")))
def test_resize_pre_against_float64_interpolate(fmt, shape, aa):
    """max |delta| < 2e-6, the bound tests/test_gpu_kernels.py::test_resize_pre and the 4:2:0 tests hold this kernel body to; a smooth clip and
    a uniformly random-word clip (out-of-gamut triples: the clamp; p210's low bits, yuv444p10 words above 1023), at odd byte pitches, the
    presets and the forms in turn"""
    for i, preset in enumerate(R.PRESETS):
        clip = random_clip(shape, fmt, seed=9 + i) if i % 2 else clip_of(shape, fmt, preset)
        x = R.decode(clip, fmt, *preset)
        ref = F.interpolate(torch.from_numpy(x), size=(S, S), mode="bilinear", align_corners=False, antialias=aa)       # float64
        ref_rgb = (ref * 2.0 - 1.0).permute(0, 2, 3, 1)
        ref_y = ((YMAT[0] * ref[:, 0] + YMAT[1] * ref[:, 1] + YMAT[2] * ref[:, 2]) * 2.0 - 1.0)[::2]
        form, strip = FORMS[i % 4]
        rgb, key = call_resize(Pitched(_t(clip), shape), fmt, shape, preset, aa, form=form, strip=strip)
        e_rgb = (rgb[..., :3].cpu().double() - ref_rgb).abs().max().item()
        e_y = (key[..., 0].cpu().double() - ref_y).abs().max().item()
        print(f"resize_pre {fmt} {shape} antialias={aa} {preset} {form} {strip}: max |delta| rgb {e_rgb:.2e}, y {e_y:.2e}")
        assert e_rgb < 2e-6 and e_y < 2e-6, (fmt, shape, aa, preset, e_rgb, e_y)
    raw = R.decode(random_clip(shape, fmt), fmt, "bt709", False, clamp=False)
    assert raw.min() < -0.1 and raw.max() > 1.1               # the clamp is exercised
    words = random_clip(shape, fmt)[0]
    assert int((words & 63).max()) > 0 if fmt == "p210" else int(words.max()) > 1023       # and so are the ignored bits / the saturation


# ---------------------------------------------------------------------------------------------------- 4. embed equals the composition
def _composition(model, planes, fmt, msgs, preset, lowres):
    rgb = yuv.to_rgb(_t(planes), fmt, *preset).cuda()                               # fp32
    w = model.embed(rgb, msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
    return R.encode_values(w.cpu().double().numpy(), fmt, *preset)


@pytest.mark.parametrize("fmt,shape", cases(("yuv422p10", "yuv444p10", "yuv444p")))
def test_embed_equals_the_composition(fmt, shape, tiny):
    """every output code lies within 0.5 + (2^depth - 1) * TOL_IMG of the float64 code value of the fp32 composition to_rgb -> embed ->
    encode_values (the rule and the constant of the p010 test), and the clip changed"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    att0 = model.attenuation
    model.chunk_size, model.step_size = 2, 2
    top = (1 << depth_of(fmt)) - 1
    worst = 0.0
    try:
        for i, (lowres, mode, att) in enumerate(itertools.product((True, False), ("repeat", "alternate", "interpolate"), (True, False))):
            preset = R.PRESETS[i % 6]
            model.video_mode = mode
            model.attenuation = att0 if att else None
            clip = clip_of(shape, fmt, preset, seed=20 + i)
            v = _composition(model, clip, fmt, msgs, preset, lowres)
            for variant in (0, 1):
                model._engine().tail_variant = variant
                out = model.embed_yuv(Pitched(_t(clip), shape, even=True).views, fmt, msgs, lowres_attenuation=lowres, matrix=preset[0],
                                      full_range=preset[1])["planes_w"]
                model._engine().tail_variant = 0
                assert all(p.dtype == yuv.fmt_dtype(fmt) and p.is_cuda for p in out)
                for g, want in zip(R.codes_of(_np(out), fmt), v):
                    assert g.shape == want.shape
                    err = np.abs(g.astype(np.float64) - want).max()
                    worst = max(worst, err)
                    assert err <= 0.5 + top * TOL_IMG, (fmt, shape, lowres, mode, att, preset, variant, err)
                assert not np.array_equal(_np(out)[0], clip[0])
    finally:
        model._engine().tail_variant = 0
        model.attenuation = att0
        model.video_mode = "repeat"
    print(f"embed_yuv {fmt} {shape}: max |code - v| = {worst:.4f}")


@pytest.mark.parametrize("fmt,shape", cases(("yuv422p10", "yuv444p10", "yuv444p")))
def test_detect_yuv(fmt, shape, tiny):
    spec, sd, model = tiny
    F_ = SHAPES[shape][0]
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    for i, preset in enumerate(R.PRESETS):
        clip = clip_of(shape, fmt, preset, seed=40 + i) if i % 2 == 0 else random_clip(shape, fmt, seed=40 + i)
        aa = i % 3 != 0
        it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
        got = model.detect_yuv(Pitched(_t(clip), shape, even=True).views, fmt, interpolation=it, matrix=preset[0], full_range=preset[1])["preds"]
        want = model.detect(yuv.to_rgb(_t(clip), fmt, *preset).cuda(), is_video=True, interpolation=it)["preds"]
        assert got.shape == (F_, spec.nbits + 1)
        assert (got - want).abs().max().item() < TOL_LOGIT
        assert_decisions(got, want, what=f"detect_yuv {fmt} {shape} {preset}", min_sure=0.99)
    # end to end: the watermarked clip through detect_yuv
    msgs = synthetic_msgs(1, spec.nbits, seed=9)
    preset = R.PRESETS[4]
    kw = dict(matrix=preset[0], full_range=preset[1])
    w = model.embed_yuv(Pitched(_t(clip_of(shape, fmt, preset)), shape, even=True).views, fmt, msgs, **kw)["planes_w"]
    got = model.detect_yuv(w, fmt, **kw)["preds"]
    want = model.detect(yuv.to_rgb(tuple(p.cpu() for p in w), fmt, *preset).cuda(), is_video=True)["preds"]
    assert (got - want).abs().max().item() < TOL_LOGIT
    assert_decisions(got, want, what=f"detect_yuv of embed_yuv {fmt} {shape}", min_sure=0.99)


# ---------------------------------------------------------------------------------------------------- 5. chroma is left alone
@pytest.mark.parametrize("lowres", [True, False])
@pytest.mark.parametrize("fmt,shape", cases(("yuv422p10", "p210", "yuv444p10", "yuv422p"), "ACEG"))
def test_yuv_embedder_leaves_chroma_alone(fmt, shape, lowres, tiny):
    """the yuv embedder adds one value to R, G and B alike: wherever the fp32 composition clamps none of a block's values the block's
    (Cb, Cr) come back exactly (blocks are 2 x 1 or 1 x 1).  Catches swapped Cb / Cr or U / V, a chroma row or pitch off by one, a 4:2:2
    kernel that indexes chroma at row >> 1."""
    spec, sd, model = tiny
    F_, H, W, _ = SHAPES[shape]
    sx = R.FORMATS[fmt][3]
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=8)
    for preset in (R.PRESETS[2], R.PRESETS[1], R.PRESETS[4]):
        clip = clip_of(shape, fmt, preset, kind="noise", seed=31, lo=0.3, hi=0.7)
        rgb = yuv.to_rgb(_t(clip), fmt, *preset)
        w = model.embed(rgb.cuda(), msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"].cpu()
        inside = ((w > 0) & (w < 1) & (rgb > 0) & (rgb < 1)).all(dim=1)                             # [F, H, W]: no channel clamped
        blocks = inside.reshape(F_, H, W >> sx, 1 << sx).all(dim=3).numpy()                         # [F, H, W >> sx]
        assert blocks.mean() >= 0.99
        yin, cbin, crin = R.codes_of(clip, fmt)
        for variant in (0, 1):                        # row-streaming tail, tile tail
            model._engine().tail_variant = variant
            try:
                out = model.embed_yuv(Pitched(_t(clip), shape, even=True).views, fmt, msgs, lowres_attenuation=lowres, matrix=preset[0],
                                      full_range=preset[1])["planes_w"]
            finally:
                model._engine().tail_variant = 0
            yo, cbo, cro = R.codes_of(_np(out), fmt)
            assert np.array_equal(cbin[blocks], cbo[blocks]) and np.array_equal(crin[blocks], cro[blocks]), (preset, variant)
            assert not np.array_equal(yo, yin)               # luma carries the watermark


# ---------------------------------------------------------------------------------------------------- 6. identity
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("shape", ["A", "C", "D", "E", "G"])
def test_identity_without_a_watermark(shape, kind, tiny):
    """scaling_w = 0, attenuation off: output words equal input words, the six formats, the six presets in turn, both tail variants
    (tests/test_yuv_cpu.py::test_identity_on_the_cpu grounds it: the definitions are the identity on these clips, noise frames included)"""
    spec, sd, model = tiny
    x = (0.1 + 0.8 * frames_of(shape, kind=kind)).numpy()
    att0, sw0 = model.attenuation, model.blender.scaling_w
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    try:
        model.attenuation = None
        model.blender.scaling_w = 0.0
        for k, fmt in enumerate(R.NEW):
            if shape not in shapes_of(fmt):
                continue
            for j, variant in enumerate((0, 1)):
                for i in range(3):
                    preset = R.PRESETS[(2 * i + j + k) % 6]
                    clip = R.encode(x, fmt, *preset)
                    model._engine().tail_variant = variant
                    out = model.embed_yuv(Pitched(_t(clip), shape, even=True).views, fmt, matrix=preset[0], full_range=preset[1])["planes_w"]
                    assert all(np.array_equal(a, b) for a, b in zip(_np(out), clip)), (shape, kind, fmt, preset, variant)
    finally:
        model._engine().tail_variant = 0
        model.attenuation, model.blender.scaling_w = att0, sw0


# ---------------------------------------------------------------------------------------------------- 7. red zones
def call_tail(src: Pitched, dst: Pitched, fmt, shape, preset, eng, delta, hm, variant):
    F_, H, W, _ = SHAPES[shape]
    d = N.TailYuvDesc()
    d.src, d.dst = src.surface(fmt), dst.surface(fmt)
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(eng.taps43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, 1
    d.step, d.video_mode, d.total_key = 2, 2, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = 1, 1, 1
    d.scaling_i, d.scaling_w = 1.0, 0.2
    d.variant = variant
    d.yuv2rgb12, d.rgb2yuv12 = aff(preset, depth_of(fmt))
    N.check(N.lib().vs_embed_tail_yuv(C.byref(d), None), "vs_embed_tail_yuv")
    torch.cuda.synchronize()


@pytest.mark.parametrize("full_jnd", [True, False])
@pytest.mark.parametrize("fmt,shape", cases(("yuv422p", "p210", "yuv444p10"), "ACDEG"))
def test_red_zones_and_pitch_padding(fmt, shape, full_jnd, tiny):
    """source and destination planes between guard bands with poisoned pitch padding (odd byte pitches, 16-bit planes included) and spare
    rows: the source is unchanged, no byte of a destination plane outside its rows' payload is written, and two padding poisons, the tile
    form and several strip heights give the same bytes"""
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


# ---------------------------------------------------------------------------------------------------- 8. graphs
def test_yuv444p10_graph_replay_matches_eager(tiny):
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 8, 2, "repeat"          # (detect walks a clip in chunk_size frames: one chunk)
    outs = {}
    n0 = len(model._graphs)
    try:
        for use in (False, True):
            model.use_graphs = use
            res = []
            for seed in (1, 2, 3):
                pc = Pitched(_t(clip_of("A", "yuv444p10", R.PRESETS[2], seed=seed)), "A", even=True)
                msgs = synthetic_msgs(1, spec.nbits, seed=seed)
                w = model.embed_yuv(pc.views, "yuv444p10", msgs)
                res.append((w["imgs_w"], model.detect_yuv(w["planes_w"], "yuv444p10")["preds"]))
            outs[use] = res
    finally:
        model.use_graphs = False
    assert len(model._graphs) == n0 + 2           # one embed graph + one detect graph, reused for the 3 clips
    for (w0, p0), (w1, p1) in zip(outs[False], outs[True]):
        assert torch.equal(w0.view(torch.uint8), w1.view(torch.uint8)) and torch.equal(p0, p1)
    # another colour choice is another graph, and so is another format of the same size
    model.use_graphs = True
    try:
        H, W = SHAPES["A"][1:3]
        planes = yuv.planes_of(outs[True][0][0], "yuv444p10", H, W)
        model.detect_yuv(planes, "yuv444p10", matrix="bt2020", full_range=True)
        assert len(model._graphs) == n0 + 3
        model.detect_yuv(planes, "yuv444p10", matrix="bt2020", full_range=True)
        assert len(model._graphs) == n0 + 3
        p422 = tuple(p.cuda() for p in _t(clip_of("A", "yuv422p10", R.PRESETS[2])))
        model.detect_yuv(p422, "yuv422p10")
        assert len(model._graphs) == n0 + 4
        model.detect_yuv(tuple(p.cuda() for p in _t(R.convert(_np(p422), "yuv422p10", "p210"))), "p210")
        assert len(model._graphs) == n0 + 5
    finally:
        model.use_graphs = False


# ---------------------------------------------------------------------------------------------------- 9. model-level C-ABI
@pytest.mark.parametrize("fmt,shape", [("yuv422p", "B"), ("p210", "E"), ("yuv444p10", "G"), ("yuv444p", "B"), ("i420", "B")])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_model_level_c_api_yuv(which, fmt, shape, tiny, tinyc):
    """vs_model_embed_yuv / vs_model_detect_yuv equal embed_yuv / detect_yuv: words equal, logits within 1e-4 (the bound of the RGB24, NV12 and
    4:2:0 twins); NULL affines (the default colour) and an explicit bt2020 limited pair; pitched input and output surfaces, poison intact"""
    from tests._model import cfg_of
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny if which == "tiny" else tinyc
    cm = CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=33)
    model.chunk_size, model.step_size, model.video_mode = 3, 2, "repeat"
    for color in (None, ("bt2020", False)):
        preset = color or ("bt709", False)
        clip = clip_of(shape, fmt, preset, seed=60)
        for lowres in (True, False):
            src = Pitched(_t(clip), shape, even=True)
            py = model.embed_yuv(src.views, fmt, msgs, lowres_attenuation=lowres, matrix=preset[0], full_range=preset[1])["planes_w"]
            dst = Pitched(_t(clip), shape, 0x5A, even=True, extra=3, fill=False)
            c = cm.embed_yuv(src.views, fmt, msgs, out_planes=dst.views, color=color, step=2, lowres_attenuation=lowres)
            assert all(_same(a, b) for a, b in zip(py, c)), (which, fmt, color, lowres)
            for buf, mask in zip(dst.bufs, dst.masks):
                assert torch.all(buf[mask] == 0x5A)
            packed = cm.embed_yuv(tuple(p.contiguous() for p in src.views), fmt, msgs, color=color, step=2, lowres_attenuation=lowres)
            assert all(_same(a, b) for a, b in zip(py, packed))
        lp = model.detect_yuv(py, fmt, matrix=preset[0], full_range=preset[1])["preds"]
        assert (cm.detect_yuv(dst.views, fmt, color=color) - lp).abs().max().item() < 1e-4


def test_c_level_refusals():
    lib = N.lib()
    UNS = N.ERR_UNSUPPORTED
    clip = clip_of("D", "yuv422p", R.PRESETS[2])
    pc = Pitched(_t(clip), "D")
    F_, H, W, _ = SHAPES["D"]
    rgb = torch.zeros((F_, S, S, 4), device="cuda")
    dec = aff(R.PRESETS[2], 8)[0]

    def resize(s, H_, W_):
        return lib.vs_resize_pre_yuv(C.byref(s), F_, H_, W_, dec, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None)
    for planar, depth, msb, chroma in ((1, 10, 1, 422), (0, 10, 0, 422), (1, 12, 0, 444), (0, 8, 1, 422), (0, 8, 0, 444), (0, 10, 1, 444), (1, 8, 0, 411),
                                       (1, 8, 0, 0), (2, 8, 0, 422)):
        s = pc.surface("yuv422p")
        s.planar, s.depth, s.msb_aligned, s.chroma = planar, depth, msb, chroma
        assert resize(s, H, W) == UNS, (planar, depth, msb, chroma)
    s = pc.surface("yuv422p")
    assert resize(s, H, W - 1) == -1                                # 4:2:2: W even
    s.chroma = 420
    assert resize(s, H - 1, W) == -1                                # 4:2:0: H even too
    s = pc.surface("yuv422p")
    s.pitch[1] = W // 2 - 1                                         # a pitch shorter than the row
    assert resize(s, H, W) == -1
    d = N.TailYuvDesc()
    d.src, d.dst = pc.surface("yuv422p"), pc.surface("yuv422p")
    delta = torch.zeros(1, 1, S, S, device="cuda")
    d.delta, d.F, d.H, d.W, d.S_h, d.S_w, d.Cd, d.step, d.total_key, d.clamp = N.ptr(delta), F_, H, W, S, S, 1, 2, 1, 1
    d.yuv2rgb12, d.rgb2yuv12 = aff(R.PRESETS[2], 8)
    d.attenuate = 2
    assert lib.vs_embed_tail_yuv(C.byref(d), None) == UNS
    d.attenuate = 0
    d.preds_w = N.ptr(delta)
    assert lib.vs_embed_tail_yuv(C.byref(d), None) == UNS
    d.preds_w = None
    d.variant = 2
    assert lib.vs_embed_tail_yuv(C.byref(d), None) == UNS
    d.variant = 0
    d.dst.chroma = 444                                              # the two surfaces hold different formats
    assert lib.vs_embed_tail_yuv(C.byref(d), None) == UNS
    d.dst = pc.surface("yuv422p")
    d.dst.depth, d.dst.msb_aligned = 10, 1
    assert lib.vs_embed_tail_yuv(C.byref(d), None) == UNS
    d.dst = pc.surface("yuv422p")
    d.W = W - 1
    assert lib.vs_embed_tail_yuv(C.byref(d), None) == -1
    # the 4:2:0 entry points go on refusing a surface that is none of theirs, and odd sizes
    s420 = pc.surface("yuv422p", old=True)
    assert lib.vs_resize_pre_yuv420(C.byref(s420), F_, H - 1, W, dec, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 10. errors, empty and host-resident clips
def test_errors_empty_and_host_clips(tiny):
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=3)
    y, u, v = (p.cuda() for p in _t(clip_of("B", "yuv422p", R.PRESETS[2])))
    y10, uv10 = (p.cuda() for p in _t(clip_of("B", "p210", R.PRESETS[2])))
    q = tuple(p.cuda() for p in _t(clip_of("G", "yuv444p10", R.PRESETS[2])))
    tr = torch.zeros(6, 44, 72, dtype=torch.uint8, device="cuda").transpose(1, 2)                  # [6, 72, 44] with a last stride of 72
    bad = [((y[:, :, :87], u, v), "yuv422p"), ((y.float(), u, v), "yuv422p"), ((y10, uv10), "nv16"), ((y, u, v), "yuv422p10"),
           ((y, u[:, :35], v), "yuv422p"), ((y, u), "yuv422p"), ((y, u, tr), "yuv422p"), ((y, u, v.cpu()), "yuv422p"), ((y, u, v), "yuv444p"),
           ((y, u, v), "yuyv422"), ((y, u, v), "i420"), (y, "yuv444p")]
    for planes, fmt in bad:
        with pytest.raises(ValueError):
            model.embed_yuv(planes, fmt, msgs)
        with pytest.raises(ValueError):
            model.detect_yuv(planes, fmt)
    with pytest.raises(ValueError):
        model.detect_yuv((y, u, v), "yuv422p", matrix="bt470")
    with pytest.raises(ValueError):
        model.embed_yuv420((y, u, v), "yuv422p", msgs)                                          # embed_yuv420 goes on refusing the new names
    clamp0 = model.clamp
    try:
        model.clamp = False
        with pytest.raises(NotImplementedError):
            model.embed_yuv((y, u, v), "yuv422p", msgs)
    finally:
        model.clamp = clamp0
    e = model.embed_yuv((y[:0], u[:0], v[:0]), "yuv422p", msgs)
    assert e["imgs_w"].shape == (0, 72 * 88 * 2) and e["imgs_w"].dtype == torch.uint8 and e["msgs"].shape[0] == 0 and len(e["planes_w"]) == 3
    assert model.detect_yuv((y10[:0], uv10[:0]), "p210")["preds"].shape == (0, spec.nbits + 1)
    # int16 planes are the same bits
    a = model.embed_yuv((y10, uv10), "p210", msgs)["imgs_w"]
    b = model.embed_yuv((y10.view(torch.int16), uv10.view(torch.int16)), "p210", msgs)["imgs_w"]
    assert a.dtype == torch.uint16 and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a host-resident clip moves chunk by chunk and comes back on the host with the same words
    for planes, fmt in (((y, u, v), "yuv422p"), ((y10, uv10), "p210"), (q, "yuv444p10")):
        dev = model.embed_yuv(planes, fmt, msgs)
        host = model.embed_yuv(tuple(p.cpu() for p in planes), fmt, msgs)
        assert not host["imgs_w"].is_cuda and torch.equal(host["imgs_w"].view(torch.uint8), dev["imgs_w"].cpu().view(torch.uint8))
        assert all(not p.is_cuda for p in host["planes_w"])
        assert torch.equal(model.detect_yuv(tuple(p.cpu() for p in planes), fmt)["preds"], model.detect_yuv(planes, fmt)["preds"].cpu())


def test_pixelwise_detector_is_refused(tiny, monkeypatch):
    spec, sd, model = tiny
    monkeypatch.setattr(type(model), "pixelwise", property(lambda self: True))
    with pytest.raises(NotImplementedError, match="detect_yuv"):
        model.detect_yuv(tuple(p.cuda() for p in _t(clip_of("B", "yuv422p", R.PRESETS[2]))), "yuv422p")
