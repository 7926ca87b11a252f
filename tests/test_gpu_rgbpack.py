"""Packed RGB clips on the HIP path: vs_resize_pre_rgb / vs_embed_tail_rgb, Videoseal.embed_rgb / detect_rgb, the model-level C-ABI.

References: tests/_rgbpack_ref.py (float64 numpy, independent of videoseal_amd.rgbpack), the project's own fp32 entry points on the decoded
frames (the packed kernels evaluate the same expressions in the same order between decode and encode: torch.equal), embed_u8 / detect_u8 on
the contiguous RGB24 clip, and the CPU oracle in float64.  Every clip is a strided view of a poisoned device buffer between GUARD bands: spare
rows per frame, a byte pitch that is odd wherever the caller can express it (an 8-bit clip anywhere, every clip at the C level) and a base
address one byte (at the tensor level: one element) past a 16-byte boundary.
  A = 5 x 134 x 202: general case                                          B = 6 x 72 x 88: watermark up-resize below 2 x, tile forms
  C = 3 x 134 x 522: three 256-column tiles with a ragged last one, 8 : 1 resize   D = 2 x 18 x 34: an rgb24 row of 102 bytes, a frame
  smaller than a tile      E = 3 x 67 x 202: odd H       G = 2 x 131 x 259: odd H and W, row-streaming forms, a partial last piece in
  every row                H = 1 x 3 x 5: a row shorter than one piece
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import videoseal_ref as O  # noqa: E402
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from oracle.weights import make_state_dict, tiny_spec  # noqa: E402
from tests import _rgbpack_ref as R  # noqa: E402
from tests._guards import GUARD, _guarded, _guards_intact  # noqa: E402
from tests._util import assert_decisions  # noqa: E402
from tests._model import TOL_IMG, TOL_LOGIT, cfg_of, make_model  # noqa: E402

from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import rgbpack  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 134, 202, 7), "B": (6, 72, 88, 0), "C": (3, 134, 522, 3), "D": (2, 18, 34, 1), "E": (3, 67, 202, 5), "G": (2, 131, 259, 2),
          "H": (1, 3, 5, 2)}                                                     # F, H, W, spare rows per frame
PADS = {"A": 54, "B": 0, "C": 1, "D": 13, "E": 9, "G": 11, "H": 6}               # bytes (tensor level: elements) after a row's end
S = 64                                                                          # img_size of the tiny models
NAMES = "ABCDEGH"
STREAMS = ("A", "C", "G")                                                       # H, W >= 2 S: the row-streaming tail applies
FMTS = list(R.FORMATS)
MODES = ("repeat", "alternate", "interpolate")
ATTS = ("off", "lowres", "full")


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


def _t(a):
    """numpy clip -> CPU tensor (a uint32 word array as int32: the same bits)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)


def _np(t, fmt):
    """tensor clip (any device) -> numpy of the reference's dtype"""
    return t.cpu().contiguous().view(torch.uint8).numpy().view(R.FORMATS[fmt][0]).reshape(tuple(t.shape))


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu())


def frames_of(shape, kind="smooth", seed=5, lo=0.0, hi=1.0):
    F_, H, W, _ = SHAPES[shape]
    return lo + (hi - lo) * synthetic_frames(F_, H, W, seed=seed, kind=kind)


def clip_of(shape, fmt, seed=5, kind="smooth", lo=0.0, hi=1.0):
    """a picture in `fmt` with random alpha words / X bits"""
    F_, H, W, _ = SHAPES[shape]
    return R.encode(frames_of(shape, kind, seed, lo, hi).double().numpy(), fmt, alpha=R.random_alpha(fmt, F_, H, W, seed=seed + 1))


def random_clip(shape, fmt, seed=9):
    F_, H, W, _ = SHAPES[shape]
    dt, comps, depth, _, _ = R.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    if comps == 0:
        return rng.integers(0, 1 << 32, size=(F_, H, W), dtype=np.uint64).astype(np.uint32)
    return rng.integers(0, 1 << depth, size=(F_, H, W, comps)).astype(dt)


class Pitched:
    """a clip as a strided view of a poisoned device buffer.  `bview`: its rows as bytes [F, H, row bytes] (what the C level sees: odd pitch,
    base one byte past a 16-byte boundary); `view`: the same memory as a tensor of the clip's dtype and shape (level "torch": pitch and base
    offset are whole elements; an 8-bit clip keeps the odd pitch and the one-byte offset)"""

    def __init__(self, clip, shape, poison=0xA5, level="torch", extra=0, fill=True):
        clip = _t(clip) if isinstance(clip, np.ndarray) else clip
        spare, pad = SHAPES[shape][3], PADS[shape] + extra
        F_, H, W = clip.shape[:3]
        es = clip.element_size()
        rowb = clip[0, 0].numel() * es
        unit = 1 if (level == "c" or es == 1) else es
        pitch = rowb + pad * unit
        if unit == 1 and pitch % 2 == 0:
            pitch += 1
        n = F_ * (H + spare) * pitch
        self.buf = torch.full((GUARD + unit + n + GUARD,), poison, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.bview = self.buf[GUARD + unit:GUARD + unit + n].view(F_, H + spare, pitch)[:, :H, :rowb]
        assert self.bview.data_ptr() % 16 == unit and self.bview.stride(1) == pitch
        if fill:
            self.bview.copy_(clip.contiguous().view(torch.uint8).reshape(F_, H, rowb).cuda())
        m = torch.ones(F_, H + spare, pitch, dtype=torch.bool, device="cuda")
        m[:, :H, :rowb] = False
        g = torch.ones(GUARD + unit, dtype=torch.bool, device="cuda")
        self.mask = torch.cat([g, m.flatten(), g[:GUARD]])
        self.view = None
        if unit == es:
            v = self.bview if es == 1 else self.bview.view(clip.dtype)
            self.view = v if clip.dim() == 3 else v.unflatten(-1, (W, clip.shape[3]))
            assert tuple(self.view.shape) == tuple(clip.shape)
        self.dtype, self.shape = clip.dtype, tuple(clip.shape)

    def surface(self, fmt):
        s = N.RgbSurface()
        s.data, s.pitch, s.frame_stride, s.format = self.bview.data_ptr(), self.bview.stride(1), self.bview.stride(0), R.IDS[fmt]
        return s

    def intact(self, poison):
        return bool(torch.all(self.buf[self.mask] == poison))

    def cpu(self):
        return self.bview.cpu().contiguous().view(self.dtype).reshape(self.shape)


YMAT = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]
FORMS = (("tile", 0), (None, 0), (None, 5), (None, 22))


def call_resize(pc: Pitched, fmt, oh, ow, aa, mul=2.0, add=-1.0, y_step=2, form=None, strip=0):
    """vs_resize_pre_rgb; form "tile" keeps the tile kernel, `strip` sets the strip height of the row-streaming one"""
    F_, H, W = pc.shape[:3]
    rgb_buf, rgb = _guarded(torch.full((F_, oh, ow, 4), float("nan")).cuda(), -7.0)
    key_buf, key = _guarded(torch.full(((F_ + y_step - 1) // y_step, oh, ow, 4), float("nan")).cuda(), -7.0)
    surf = pc.surface(fmt)
    with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", int(strip)):
        N.check(N.lib().vs_resize_pre_rgb(C.byref(surf), F_, H, W, oh, ow, int(aa), N.ptr(rgb), mul, add, N.ptr(key), y_step,
                                          (C.c_float * 3)(*YMAT), None), "vs_resize_pre_rgb")
        torch.cuda.synchronize()
    assert _guards_intact(rgb_buf, -7.0) and _guards_intact(key_buf, -7.0)
    return rgb, key


def call_tail(src: Pitched, dst: Pitched, fmt, eng, delta, hm, variant, step=2, mode=2, scaling_w=0.2):
    F_, H, W = src.shape[:3]
    d = N.TailRgbDesc()
    d.src, d.dst = src.surface(fmt), dst.surface(fmt)
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(eng.taps43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, delta.shape[1]
    d.step, d.video_mode, d.total_key = step, mode, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = 1, 1, 1
    d.scaling_i, d.scaling_w = 1.0, scaling_w
    d.variant = variant
    N.check(N.lib().vs_embed_tail_rgb(C.byref(d), None), "vs_embed_tail_rgb")
    torch.cuda.synchronize()


class settings:
    """video mode, attenuation (off / lowres / full) and tail variant of a model for the block; restored afterwards"""

    def __init__(self, model, mode="repeat", att="lowres", variant=0, chunk=2, step=2):
        self.model, self.new = model, (mode, att, variant, chunk, step)

    def __enter__(self):
        m = self.model
        self.old = (m.video_mode, m.attenuation, m._engine().tail_variant, m.chunk_size, m.step_size)
        mode, att, variant, chunk, step = self.new
        m.video_mode, m.chunk_size, m.step_size = mode, chunk, step
        if att == "off":
            m.attenuation = None
        m._engine().tail_variant = variant
        return att == "lowres"

    def __exit__(self, *exc):
        m = self.model
        m.video_mode, m.attenuation, _, m.chunk_size, m.step_size = self.old
        m._engine().tail_variant = self.old[2]


def variants_of(shape):
    return (1, 4) if shape in STREAMS else (1,)


# ---------------------------------------------------------------------------------------------------- 1. exact decode
@pytest.mark.parametrize("fmt", ["rgb24", "bgr24", "argb", "x2rgb10", "x2bgr10", "rgb48", "bgra64"])
def test_decode_is_the_ieee_quotient_for_every_code(fmt):
    """an identity-size vs_resize_pre_rgb (oh = H, ow = W, no antialias, mul 1, add 0) of a clip holding every code returns
    float32(code) / float32(top) bit for bit: all 256 / 1024 / 65536 codes in each of the three component positions, the tile form and the
    row-streaming form, at the C level (odd pitch, odd base address)"""
    top = R.top_of(fmt)
    n = top + 1
    side = int(round(n ** 0.5))
    assert side * side == n
    codes = np.stack([np.arange(n), (n - 1) - np.arange(n), (np.arange(n) * 5 + 1) % n], axis=-1)
    assert all(len(set(codes[:, i])) == n for i in range(3))
    codes = codes.reshape(1, side, side, 3)
    clip = R.encode((codes.astype(np.float64) + 0.25).transpose(0, 3, 1, 2) / float(top), fmt, alpha=R.random_alpha(fmt, 1, side, side))
    assert np.array_equal(R.codes_of(clip, fmt), codes)
    want = torch.from_numpy(codes.astype(np.float32) / np.float32(top))
    for form in ("tile", None):
        pc = Pitched(clip, "H", level="c")
        rgb, key = call_resize(pc, fmt, side, side, False, mul=1.0, add=0.0, y_step=1, form=form)
        assert torch.equal(rgb[..., :3].cpu(), want), (fmt, form)
        assert torch.all(rgb[..., 3] == 0)


# ---------------------------------------------------------------------------------------------------- 2. same bits as the fp32 path
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
@pytest.mark.parametrize("fmt", FMTS)
def test_embed_rgb_gives_the_bits_of_the_fp32_path(fmt, which, tiny, tinyc):
    """embed_rgb(clip) is torch.equal to from_rgb(embed(to_rgb(clip).cuda())['imgs_w'], like=clip): the three video modes x attenuation off /
    low-res / full-res, Cd = 1 (tiny) and 3 (tinyc), tail_variant 1 everywhere and 4 where the row-streaming form applies, set on the engine
    for both sides; the seven shapes in turn, smooth pictures and random words"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    k = FMTS.index(fmt)
    for i, (mode, att) in enumerate(itertools.product(MODES, ATTS)):
        shape = NAMES[(i + k) % len(NAMES)]
        clip = random_clip(shape, fmt, seed=20 + i) if i % 4 == 3 else clip_of(shape, fmt, seed=20 + i)
        x = rgbpack.to_rgb(_t(clip), fmt).cuda()
        for variant in variants_of(shape):
            with settings(model, mode, att, variant) as lowres:
                got = model.embed_rgb(Pitched(clip, shape).view, fmt, msgs, lowres_attenuation=lowres)
                w = model.embed(x, msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
            want = rgbpack.from_rgb(w, fmt, like=_t(clip))
            out = got["imgs_w"]
            assert out.is_contiguous() and out.is_cuda and out.dtype == _t(clip).dtype and out.shape == _t(clip).shape
            assert _same(out, want), (fmt, which, shape, mode, att, variant, int((_np(out, fmt) != _np(want, fmt)).sum()))
            assert got["msgs"].shape == (SHAPES[shape][0], spec.nbits)
            if i % 4 != 3 and shape in STREAMS:           # (a frame of 15 pixels may well keep all its 8-bit codes)
                assert not np.array_equal(R.codes_of(_np(out, fmt), fmt), R.codes_of(clip, fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_detect_rgb_gives_the_bits_of_the_fp32_path(fmt, tiny):
    """detect_rgb(clip) is torch.equal to detect(to_rgb(clip)) -- the division on the CPU, as tests/test_gpu_e2e.py::test_uint8_rgb24_clip_path
    notes --, both antialias values, the seven shapes"""
    spec, sd, model = tiny
    k = FMTS.index(fmt)
    with settings(model):
        for i, shape in enumerate(NAMES):
            clip = random_clip(shape, fmt, seed=40 + i) if (i + k) % 3 == 2 else clip_of(shape, fmt, seed=40 + i)
            x = rgbpack.to_rgb(_t(clip), fmt).cuda()
            for aa in (True, False):
                it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
                got = model.detect_rgb(Pitched(clip, shape).view, fmt, interpolation=it)["preds"]
                want = model.detect(x, is_video=True, interpolation=it)["preds"]
                assert got.shape == (SHAPES[shape][0], spec.nbits + 1) and torch.equal(got, want), (fmt, shape, aa)


@pytest.mark.parametrize("fmt", R.LAYOUTS)
def test_resize_forms_agree(fmt):
    """tile form, row-streaming form and odd strip heights of vs_resize_pre_rgb: the same bits (shapes A, C, G at the C level)"""
    for shape in ("A", "C", "G"):
        clip = random_clip(shape, fmt, seed=3)
        for aa in (True, False):
            res = [call_resize(Pitched(clip, shape, level="c"), fmt, S, S, aa, form=f, strip=s) for f, s in FORMS]
            assert not torch.isnan(res[0][0]).any() and not torch.isnan(res[0][1]).any()
            for other in res[1:]:
                assert torch.equal(other[0], res[0][0]) and torch.equal(other[1], res[0][1]), (fmt, shape, aa)


# ---------------------------------------------------------------------------------------------------- 3. same bytes as embed_u8
@pytest.mark.parametrize("shape", list(NAMES))
def test_rgb24_equals_embed_u8(shape, tiny):
    """embed_rgb(fmt='rgb24', tail_variant = 1) equals embed_u8 on the contiguous clip, detect_rgb equals detect_u8, and vs_embed_tail_rgb
    equals vs_embed_tail(io_u8 = 1) at the C level"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=5)
    clip = _t(clip_of(shape, "rgb24", seed=6))
    for mode, att in (("repeat", "lowres"), ("interpolate", "full"), ("alternate", "off")):
        with settings(model, mode, att, 1) as lowres:
            got = model.embed_rgb(Pitched(clip, shape).view, "rgb24", msgs, lowres_attenuation=lowres)["imgs_w"]
            want = model.embed_u8(clip.cuda(), msgs, lowres_attenuation=lowres)["imgs_w"]
            assert torch.equal(got, want), (shape, mode, att)
            assert torch.equal(model.detect_rgb(Pitched(got, shape).view, "rgb24")["preds"], model.detect_u8(want)["preds"])
    eng = model._engine()
    F_, H, W, _ = SHAPES[shape]
    g = torch.Generator().manual_seed(51)
    delta = torch.tanh(torch.randn((F_ + 1) // 2, 1, S, S, generator=g)).cuda()
    for full in (True, False):
        hm = None if full else torch.rand(F_ * S * S, generator=g).cuda()
        dst = Pitched(clip, shape, 0x5A, level="c", fill=False)
        with torch.cuda.device(eng.dev):
            call_tail(Pitched(clip, shape, level="c"), dst, "rgb24", eng, delta, hm, 1)
            src8, out8 = clip.cuda(), torch.empty_like(clip, device="cuda")
            d = N.TailDesc()
            d.imgs, d.out, d.delta, d.hmap_lowres = N.ptr(src8), N.ptr(out8), N.ptr(delta), N.ptr(hm)
            d.taps43 = C.cast(eng.taps43, C.c_void_p)
            d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, 1
            d.step, d.video_mode, d.total_key = 2, 2, delta.shape[0]
            d.attenuate, d.clamp, d.antialias, d.io_u8, d.variant = 1, 1, 1, 1, 1
            d.scaling_i, d.scaling_w = 1.0, 0.2
            N.check(N.lib().vs_embed_tail(C.byref(d), None), "vs_embed_tail")
            torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), out8.cpu()) and (shape == "H" or not torch.equal(out8.cpu(), clip)), (shape, full)


# ---------------------------------------------------------------------------------------------------- 4. order and depth twins
@pytest.mark.parametrize("shape", ["A", "D", "G"])
def test_order_and_depth_twins(shape, tiny):
    """one picture in the six 8-bit layouts: equal RGB bytes after embed_rgb and torch.equal logits (a swapped R / B or an alpha read as colour
    would show); its rgb48 twin with words 257 * code: bit-identical resize output and logits (257 c / 65535 = c / 255 exactly: a division
    that is not correctly rounded would show)"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=8)
    F_, H, W, _ = SHAPES[shape]
    base = clip_of(shape, "rgb24", seed=12)
    with settings(model, "interpolate", "full", 0) as lowres:
        ref_codes, ref_logits, ref_rs = None, None, None
        for fmt in R.EIGHT:
            clip = R.convert(base, "rgb24", fmt)
            if R.FORMATS[fmt][4] is not None:
                clip[..., R.FORMATS[fmt][4]] = R.random_alpha(fmt, F_, H, W, seed=4)
            out = model.embed_rgb(Pitched(clip, shape).view, fmt, msgs, lowres_attenuation=lowres)["imgs_w"]
            codes = R.codes_of(_np(out, fmt), fmt)
            logits = model.detect_rgb(Pitched(clip, shape).view, fmt)["preds"]
            rs = call_resize(Pitched(clip, shape, level="c"), fmt, S, S, True)
            if ref_codes is None:
                ref_codes, ref_logits, ref_rs = codes, logits, rs
                assert not np.array_equal(codes, R.codes_of(base, "rgb24"))
            assert np.array_equal(codes, ref_codes) and torch.equal(logits, ref_logits), (shape, fmt)
            assert torch.equal(rs[0], ref_rs[0]) and torch.equal(rs[1], ref_rs[1]), (shape, fmt)
        for fmt16, fmt8 in (("rgb48", "rgb24"), ("bgra64", "bgra")):
            twin = (R.convert(base, "rgb24", fmt8).astype(np.uint16) * 257).astype(np.uint16)
            rs = call_resize(Pitched(twin, shape, level="c"), fmt16, S, S, True)
            assert torch.equal(rs[0], ref_rs[0]) and torch.equal(rs[1], ref_rs[1]), (shape, fmt16)
            assert torch.equal(model.detect_rgb(Pitched(twin, shape).view, fmt16)["preds"], ref_logits), (shape, fmt16)


# ---------------------------------------------------------------------------------------------------- 5. alpha / X
@pytest.mark.parametrize("fmt", ["rgba", "bgra", "argb", "abgr", "rgba64", "bgra64", "x2rgb10", "x2bgr10"])
def test_alpha_and_x_bits_travel_untouched(fmt, tiny):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=9)
    for shape, variant in (("G", 4), ("G", 1), ("D", 1), ("H", 1)):
        clip = clip_of(shape, fmt, seed=14, lo=0.2, hi=0.8)
        with settings(model, "repeat", "full", variant) as lowres:
            out = _np(model.embed_rgb(Pitched(clip, shape).view, fmt, msgs, lowres_attenuation=lowres)["imgs_w"], fmt)
        a_in, a_out = R.alpha_of(clip, fmt), R.alpha_of(out, fmt)
        assert len(np.unique(a_in)) > 1 and np.array_equal(a_in, a_out), (fmt, shape, variant)
        assert shape != "G" or not np.array_equal(R.codes_of(out, fmt), R.codes_of(clip, fmt))         # ... and RGB changed


# ---------------------------------------------------------------------------------------------------- 6. identity
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("fmt", FMTS)
def test_identity_without_a_watermark(fmt, kind, tiny):
    """scaling_w = 0, attenuation off: output words equal input words (tests/test_rgbpack_cpu.py grounds it: floor((c / top) * top) == c for
    every code), both variants, random words among the clips"""
    spec, sd, model = tiny
    sw0 = model.blender.scaling_w
    try:
        model.blender.scaling_w = 0.0
        for shape in ("A", "D", "G", "H"):
            clip = clip_of(shape, fmt, kind=kind, seed=17) if shape != "D" else random_clip(shape, fmt, seed=17)
            for variant in variants_of(shape):
                with settings(model, "repeat", "off", variant):
                    out = model.embed_rgb(Pitched(clip, shape).view, fmt)["imgs_w"]
                assert _same(out, _t(clip)), (fmt, kind, shape, variant)
    finally:
        model.blender.scaling_w = sw0


# ---------------------------------------------------------------------------------------------------- 7. against the CPU oracle
@pytest.mark.parametrize("shape", ["A", "G"])
@pytest.mark.parametrize("fmt", ["bgra", "rgba64", "x2bgr10"])
def test_against_the_cpu_oracle_in_float64(fmt, shape, tiny):
    """every output code c satisfies |c - top * v| <= 1 + top * TOL_IMG with v = oracle.videoseal_ref.embed_video in float64 on to_rgb(clip);
    detect_rgb of the output within TOL_LOGIT of the oracle's float64 detector on the same words, decisions equal where the oracle is sure"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=11)
    sd64 = {k_: (v.double() if v.dtype.is_floating_point else v) for k_, v in sd.items()}
    clip = clip_of(shape, fmt, seed=19)
    top = R.top_of(fmt)
    x64 = rgbpack.to_rgb(_t(clip), fmt, dtype=torch.float64)
    assert np.array_equal(x64.numpy(), R.decode(clip, fmt))
    ref = O.embed_video(sd64, spec, x64, msgs, chunk_size=2, step_size=2, lowres_attenuation=True)["imgs_w"]
    with settings(model, "repeat", "lowres", 0) as lowres:
        out = model.embed_rgb(Pitched(clip, shape).view, fmt, msgs, lowres_attenuation=lowres)["imgs_w"]
        preds = model.detect_rgb(out, fmt)["preds"].cpu()
    codes = R.codes_of(_np(out, fmt), fmt).astype(np.float64)
    err = np.abs(codes - top * ref.numpy().transpose(0, 2, 3, 1)).max()
    print(f"embed_rgb {fmt} {shape}: max |c - top * v| = {err:.4f} (bound {1 + top * TOL_IMG:.4f})")
    assert err <= 1 + top * TOL_IMG, (fmt, shape, err)
    assert np.array_equal(R.alpha_of(_np(out, fmt), fmt), R.alpha_of(clip, fmt))
    # the oracle's detector in float64 on the frames OUR detector saw: the decoded output words (the oracle's own frames are not quantised
    # to the clip's depth: at 8 bits that alone moves a logit by 4e-2)
    pref = O.detect(sd64, spec, rgbpack.to_rgb(out.cpu(), fmt, dtype=torch.float64))["preds"].float()
    lerr = (preds - pref).abs().max().item()
    print(f"detect_rgb {fmt} {shape}: max |logit - oracle| = {lerr:.2e}")
    assert lerr < TOL_LOGIT
    assert_decisions(preds, pref, what=f"detect_rgb {fmt} {shape}", min_sure=0.99)


# ---------------------------------------------------------------------------------------------------- 8. red zones
@pytest.mark.parametrize("full_jnd", [True, False])
@pytest.mark.parametrize("fmt", R.LAYOUTS)
def test_red_zones_and_pitch_padding(fmt, full_jnd, tiny):
    """source and destination between guard bands with poisoned pitch padding (odd byte pitches and base addresses, 16- and 32-bit words
    included) and spare rows: the source is unchanged, no byte of the destination outside its rows' payload is written, two source poisons,
    several strip heights (and, with the low-resolution heat-map, the tile form) give the same bytes; the resize's destinations keep their
    guards (call_resize checks them)"""
    spec, sd, model = tiny
    eng = model._engine()
    for shape in ("C", "D", "G", "H"):
        F_, H, W, _ = SHAPES[shape]
        clip = clip_of(shape, fmt, kind="noise", seed=50)
        g = torch.Generator().manual_seed(51)
        delta = torch.tanh(torch.randn((F_ + 1) // 2, 1, S, S, generator=g)).cuda()
        hm = None if full_jnd else torch.rand(F_ * S * S, generator=g).cuda()
        results = []
        # (the tile form evaluates the full-resolution heat-map tap by tap: held to the fp32 path above, not bit for bit against the other form)
        runs = ((0xA5, 0, 0), (0x3C, 0, 0), (0xA5, 0, 4), (0x3C, 0, 20), (0xA5, 1, 0), (0x3C, 1, 0))
        for poison, variant, strip in runs:
            src = Pitched(clip, shape, poison, level="c")
            keep = src.buf.clone()
            dst = Pitched(clip, shape, 0x5A, level="c", extra=4, fill=False)
            with torch.cuda.device(eng.dev), N.debug("TAIL_STRIP", strip):
                rgb, key = call_resize(src, fmt, S, S, True)
                call_tail(src, dst, fmt, eng, delta, hm, variant)
            assert torch.equal(src.buf, keep)                                                        # the source is read only
            assert dst.intact(0x5A), (fmt, shape, variant, strip)                                    # guards, pitch padding, spare rows
            out = dst.cpu()
            assert shape == "H" or not _same(out, _t(clip))
            results.append((variant, [rgb.cpu(), key.cpu(), out.view(torch.uint8) if out.dtype != torch.uint8 else out]))
        for variant, other in results[1:]:
            first = results[0][1] if (variant == 0 or not full_jnd or shape not in STREAMS) else results[4][1]
            for a, b in zip(first, other):
                assert torch.equal(a, b), (fmt, shape, variant)


# ---------------------------------------------------------------------------------------------------- 9. graphs
def test_rgba64_graph_replay_matches_eager(tiny):
    spec, sd, model = tiny
    outs = {}
    n0 = len(model._graphs)
    with settings(model, "repeat", "lowres", 0, chunk=8, step=2):
        try:
            for use in (False, True):
                model.use_graphs = use
                res = []
                for seed in (1, 2, 3):
                    pc = Pitched(clip_of("A", "rgba64", seed=seed), "A")
                    msgs = synthetic_msgs(1, spec.nbits, seed=seed)
                    w = model.embed_rgb(pc.view, "rgba64", msgs)["imgs_w"]
                    res.append((w, model.detect_rgb(w, "rgba64")["preds"]))
                outs[use] = res
            assert len(model._graphs) == n0 + 2           # one embed graph + one detect graph, reused for the 3 clips
            for (w0, p0), (w1, p1) in zip(outs[False], outs[True]):
                assert _same(w0, w1) and torch.equal(p0, p1)
            # the graph is keyed by the format: the same words read as bgra64 are another graph
            model.detect_rgb(outs[True][0][0], "bgra64")
            assert len(model._graphs) == n0 + 3
            model.detect_rgb(outs[True][1][0], "bgra64")
            assert len(model._graphs) == n0 + 3
        finally:
            model.use_graphs = False


# ---------------------------------------------------------------------------------------------------- 10. refusals
def test_c_level_refusals():
    lib = N.lib()
    UNS = N.ERR_UNSUPPORTED
    clip = clip_of("D", "bgra")
    pc, other = Pitched(clip, "D", level="c"), Pitched(clip, "D", level="c")
    F_, H, W, _ = SHAPES["D"]
    rgb = torch.zeros((F_, S, S, 4), device="cuda")

    def resize(s, H_=H, W_=W, dst=N.ptr(rgb)):
        return lib.vs_resize_pre_rgb(C.byref(s), F_, H_, W_, S, S, 1, dst, 1.0, 0.0, None, 1, None, None)
    s = pc.surface("bgra")
    for f in (-1, 12, 99):
        s.format = f
        assert resize(s) == UNS
    s = pc.surface("bgra")
    assert resize(s, H_=0) == -1 and resize(s, W_=0) == -1 and resize(s, dst=None) == -1
    assert lib.vs_resize_pre_rgb(None, F_, H, W, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == -1
    s.pitch = W * 4 - 1
    assert resize(s) == -1                                                     # a pitch shorter than its row
    s = pc.surface("bgra")
    s.data = None
    assert resize(s) == -1
    delta = torch.zeros(1, 1, S, S, device="cuda")

    def desc():
        d = N.TailRgbDesc()
        d.src, d.dst = pc.surface("bgra"), other.surface("bgra")
        d.delta, d.F, d.H, d.W, d.S_h, d.S_w, d.Cd, d.step, d.total_key, d.clamp = N.ptr(delta), F_, H, W, S, S, 1, 2, 1, 1
        return d
    tail = lambda d: lib.vs_embed_tail_rgb(C.byref(d), None)                   # noqa: E731
    for name, value, code in (("attenuate", 2, UNS), ("preds_w", N.ptr(delta), UNS), ("variant", 2, UNS), ("variant", 3, UNS), ("variant", 4, UNS),
                              ("clamp", 0, -1), ("delta", None, -1), ("F", 0, -1), ("S_w", 0, -1), ("Cd", 2, -1), ("video_mode", 3, -1)):
        d = desc()
        setattr(d, name, value)
        assert tail(d) == code, (name, value)                                  # (variant 4: D is too small for the row-streaming form)
    d = desc()
    d.dst.format = R.IDS["rgba"]                                               # the two surfaces hold different formats
    assert tail(d) == UNS
    d = desc()
    d.src.format = d.dst.format = 12
    assert tail(d) == UNS
    d = desc()
    d.dst = pc.surface("bgra")                                                 # dst.data == src.data: the JND reads a halo of the source
    assert tail(d) == -1
    d = desc()
    d.dst.pitch = W * 4 - 1
    assert tail(d) == -1
    d = desc()
    d.src.data = None
    assert tail(d) == -1
    assert lib.vs_embed_tail_rgb(None, None) == -1
    torch.cuda.synchronize()
    assert pc.intact(0xA5) and other.intact(0xA5) and _same(other.cpu(), _t(clip))       # nothing was launched


def test_python_refusals_empty_and_host_clips(tiny, monkeypatch):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=3)
    with settings(model):
        bgra = _t(clip_of("B", "bgra")).cuda()
        w64 = _t(clip_of("B", "rgba64")).cuda()
        x2 = _t(clip_of("G", "x2rgb10")).cuda()
        bad = [(bgra, "rgb24"), (bgra, "rgba64"), (bgra.float(), "bgra"), (bgra[0], "bgra"), (bgra[..., :3], "rgb24"), (bgra[:, :, ::2], "bgra"),
               (w64, "rgba"), (x2, "bgra"), (x2.transpose(1, 2), "x2rgb10"), (bgra, "rgb565"), ((bgra,), "bgra"), (bgra[0:1].expand(6, 72, 88, 4), "bgra")]
        for clip, fmt in bad:
            with pytest.raises(ValueError):
                model.embed_rgb(clip, fmt, msgs)
            with pytest.raises(ValueError):
                model.detect_rgb(clip, fmt)
        with pytest.raises(AssertionError, match="Message should be unique"):
            model.embed_rgb(bgra, "bgra", synthetic_msgs(2, spec.nbits, seed=3))
        clamp0 = model.clamp
        try:
            model.clamp = False
            with pytest.raises(NotImplementedError):
                model.embed_rgb(bgra, "bgra", msgs)
        finally:
            model.clamp = clamp0
        e = model.embed_rgb(bgra[:0], "bgra", msgs)
        assert e["imgs_w"].shape == (0, 72, 88, 4) and e["imgs_w"].dtype == torch.uint8 and e["msgs"].shape[0] == 0
        assert model.detect_rgb(w64[:0], "rgba64")["preds"].shape == (0, spec.nbits + 1)
        # int16 words are the same bits, and come back as int16
        a = model.embed_rgb(w64, "rgba64", msgs)["imgs_w"]
        b = model.embed_rgb(w64.view(torch.int16), "rgba64", msgs)["imgs_w"]
        assert a.dtype == torch.uint16 and b.dtype == torch.int16 and _same(a, b)
        # a host-resident clip moves chunk by chunk and comes back on the host with the same words
        for clip, fmt in ((bgra, "bgra"), (w64, "rgba64"), (x2, "x2rgb10")):
            dev = model.embed_rgb(clip, fmt, msgs)["imgs_w"]
            host = model.embed_rgb(clip.cpu(), fmt, msgs)["imgs_w"]
            assert not host.is_cuda and host.dtype == clip.dtype and _same(host, dev)
            assert torch.equal(model.detect_rgb(clip.cpu(), fmt)["preds"], model.detect_rgb(clip, fmt)["preds"].cpu())
        monkeypatch.setattr(type(model), "pixelwise", property(lambda self: True))
        with pytest.raises(NotImplementedError, match="detect_rgb"):
            model.detect_rgb(bgra, "bgra")


# ---------------------------------------------------------------------------------------------------- 11. model-level C-ABI
@pytest.mark.parametrize("fmt,shape", [("bgra", "B"), ("x2rgb10", "G"), ("rgb48", "E")])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_model_level_c_api_rgb(which, fmt, shape, tiny, tinyc):
    """vs_model_embed_rgb / vs_model_detect_rgb equal embed_rgb / detect_rgb: words equal, logits within 1e-4 (the bound of the RGB24, NV12 and
    YUV twins); pitched input and output surfaces, poison intact"""
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny if which == "tiny" else tinyc
    cm = CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=33)
    clip = clip_of(shape, fmt, seed=60)
    with settings(model, "repeat", "lowres", 0, chunk=3, step=2):
        for lowres in (True, False):
            src = Pitched(clip, shape)
            py = model.embed_rgb(src.view, fmt, msgs, lowres_attenuation=lowres)["imgs_w"]
            dst = Pitched(clip, shape, 0x5A, extra=3, fill=False)
            c = cm.embed_rgb(src.view, fmt, msgs, out=dst.view, step=2, lowres_attenuation=lowres)
            assert _same(py, c), (which, fmt, lowres)
            assert dst.intact(0x5A)
            assert _same(py, cm.embed_rgb(src.view.contiguous(), fmt, msgs, step=2, lowres_attenuation=lowres))
        lp = model.detect_rgb(py, fmt)["preds"]
        assert (cm.detect_rgb(dst.view, fmt) - lp).abs().max().item() < 1e-4
    lib = N.lib()
    s_in, s_out = N.rgb_surface(src.view, fmt), N.rgb_surface(dst.view, fmt)
    s_out.format = (s_in.format + 1) % 12
    mi = msgs.to(device="cuda", dtype=torch.int32)
    ws = cm._workspace(SHAPES[shape][0], SHAPES[shape][1], SHAPES[shape][2], 2)
    args = (N.ptr(mi), 1, SHAPES[shape][0], SHAPES[shape][1], SHAPES[shape][2], 2, 0, 1, 1, N.ptr(ws), ws.numel(), None)
    assert lib.vs_model_embed_rgb(cm._h, C.byref(s_in), C.byref(s_out), *args) == N.ERR_UNSUPPORTED
    assert lib.vs_model_embed_rgb(cm._h, C.byref(s_in), C.byref(s_in), *args) == -1
