"""Half-precision clips on the HIP path: vs_resize_pre_half / vs_embed_tail_half, Videoseal.embed_half / detect_half.

References: videoseal_amd.halfpix (the torch definition, itself held to tests/_halfpix_ref.py by tests/test_halfpix_cpu.py), the project's own
fp32 entry points on the decoded frames (the half kernels evaluate the same expressions in the same order between decode and encode:
torch.equal on the raw 16-bit words) and the CPU oracle in float64.  Every clip is a strided view of a poisoned device buffer between GUARD
bands: spare rows per frame (and plane), a pitch that is odd in elements (odd in bytes at the C level) and a base address one element (at the C
level for packed pixels and planes alike: one byte) past a 16-byte boundary.
  A = 5 x 134 x 202: general case                                          B = 6 x 72 x 88: watermark up-resize below 2 x, tile forms
  C = 3 x 134 x 522: three 256-column tiles with a ragged last one        D = 2 x 18 x 34: a frame smaller than a tile
  E = 3 x 67 x 202: odd H       G = 2 x 131 x 259: odd H and W, row-streaming forms, a partial last piece      H = 1 x 3 x 5: a row shorter
  than a piece
Memory forms: "planar" and "cl" (channels-last) are layout "nchw", "nhwc3" and "nhwc4" are layout "nhwc".
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
from tests import _halfpix_ref as R  # noqa: E402
from tests._guards import GUARD, _guarded, _guards_intact  # noqa: E402
from tests._model import TOL_IMG, cfg_of, make_model  # noqa: E402

from videoseal_amd import halfpix  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 134, 202, 7), "B": (6, 72, 88, 0), "C": (3, 134, 522, 3), "D": (2, 18, 34, 1), "E": (3, 67, 202, 5), "G": (2, 131, 259, 2),
          "H": (1, 3, 5, 2)}                                                     # F, H, W, spare rows per frame (and plane)
PADS = {"A": 54, "B": 0, "C": 1, "D": 13, "E": 9, "G": 11, "H": 6}               # bytes (tensor level: elements) after a row's end
S = 64                                                                          # img_size of the tiny models
NAMES = "ABCDEGH"
STREAMS = ("A", "C", "G")                                                       # H, W >= 2 S: the row-streaming tail applies
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
FORMS = ("planar", "cl", "nhwc3", "nhwc4")
LAYOUT = {"planar": "nchw", "cl": "nchw", "nhwc3": "nhwc", "nhwc4": "nhwc"}
MODES = ("repeat", "alternate", "interpolate")
ATTS = ("off", "lowres", "full")
GRID = list(itertools.product(R.TYPES, R.RANGES, FORMS))


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


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def random_alpha(F_, H, W, seed=1):
    """alpha words: anything, NaN and Inf bit patterns included"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-32768, 32768, (F_, H, W), generator=g, dtype=torch.int32).to(torch.int16)
    a.view(-1)[:6] = torch.tensor([0x7E01, 0x7C00, -1, -1024, 0x7FC1, 0x7F80], dtype=torch.int16)       # NaN (payload), +Inf, NaN, -Inf as fp16; NaN, +Inf as bf16
    return a


def pack(x01, typ, rng, form, alpha_seed=1):
    """component values fp32 [F, 3, H, W] (not clamped: stored as they are, rounded to the type) -> a compact CPU clip in `form`"""
    y = (x01 * 2.0 - 1.0) if rng == "signed" else x01
    w = y.to(DT[typ])
    return arrange(w, form, alpha_seed)


def arrange(w, form, alpha_seed=1):
    """stored words [F, 3, H, W] -> the compact clip of `form` (nchw forms: the [F, 3, H, W] view of it)"""
    F_, _, H, W = w.shape
    if form == "planar":
        return w.contiguous()
    px = w.permute(0, 2, 3, 1).contiguous()
    if form == "nhwc4":
        px = torch.cat([px, random_alpha(F_, H, W, alpha_seed).view(w.dtype)[..., None]], dim=-1).contiguous()
    return px.permute(0, 3, 1, 2) if form == "cl" else px


def smooth(shape, seed=5, lo=0.0, hi=1.0):
    F_, H, W, _ = SHAPES[shape]
    return lo + (hi - lo) * synthetic_frames(F_, H, W, seed=seed)


def wild(shape, typ, seed=9):
    """component values overshooting [0, 1] by up to 25 % on both sides, signed zeros, a dark frame whose components lie in (0, 2^-14), an
    all-black frame where the clip has a third one, random finite words elsewhere (magnitude below 2: larger ones overflow nothing in the
    shell, but the tiny networks' split arithmetic is not the subject here)"""
    F_, H, W, _ = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(F_, 3, H, W, generator=g) * 1.5 - 0.25
    words = torch.randint(-32768, 32768, (F_, 3, H, W), generator=g, dtype=torch.int32).to(torch.int16).view(DT[typ]).float()
    ok = torch.isfinite(words) & (words.abs() < 2.0)
    pick = torch.rand(F_, 3, H, W, generator=g) < 0.3
    x = torch.where(pick & ok, words, x)
    z = torch.rand(F_, 3, H, W, generator=g)
    x = torch.where(z < 0.02, torch.zeros(()), x)
    x = torch.where((z >= 0.02) & (z < 0.04), -torch.zeros(()), x)
    x[0] = torch.rand(3, H, W, generator=g) * (2.0 ** -14) * 0.999 + 2.0 ** -26            # the dark frame
    if F_ >= 3:
        x[2] = 0.0
    return x


class Pitched:
    """a clip as a strided view of a poisoned device buffer.  level "torch": `view` is a tensor of the clip's dtype, shape and layout whose
    pitch is odd in elements and whose base lies one element past a 16-byte boundary; level "c": the pitch is odd in bytes and the base one
    byte past (only `surface()` can express that).  Planes of a planar clip are [H + spare] rows each, one after the other inside a frame."""

    def __init__(self, clip, form, shape, poison=0xA5, level="torch", extra=0, fill=True):
        self.form, self.layout = form, LAYOUT[form]
        px = clip if self.layout == "nhwc" else (clip.permute(0, 2, 3, 1) if form == "cl" else clip)
        spare, pad = SHAPES[shape][3], PADS[shape] + extra
        es = 2
        if form == "planar":
            F_, P, H, W = px.shape
            rowb = W * es
        else:
            F_, H, W, Cc = px.shape
            P, rowb = 1, W * Cc * es
        unit = 1 if level == "c" else es
        pitch = rowb + pad * unit
        if (pitch // unit) % 2 == 0:
            pitch += unit
        n = F_ * P * (H + spare) * pitch
        self.buf = torch.full((GUARD + unit + n + GUARD,), poison, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.bview = self.buf[GUARD + unit:GUARD + unit + n].view(F_, P, H + spare, pitch)[:, :, :H, :rowb]
        assert self.bview.data_ptr() % 16 == unit and self.bview.stride(2) == pitch
        if fill:
            self.bview.copy_(px.contiguous().view(torch.uint8).reshape(F_, P, H, rowb).cuda())
        m = torch.ones(F_, P, H + spare, pitch, dtype=torch.bool, device="cuda")
        m[:, :, :H, :rowb] = False
        g = torch.ones(GUARD + unit, dtype=torch.bool, device="cuda")
        self.mask = torch.cat([g, m.flatten(), g[:GUARD]])
        self.view = None
        if unit == es:
            v = self.bview.view(clip.dtype)                                     # [F, P, H, W (x C)]
            if form == "planar":
                self.view = v
            else:
                v = v[:, 0].unflatten(-1, (W, Cc))
                self.view = v.permute(0, 3, 1, 2) if form == "cl" else v
            assert tuple(self.view.shape) == tuple(clip.shape)
        self.dtype, self.shape, self.dims, self.comps = clip.dtype, tuple(clip.shape), (F_, H, W), (3 if form == "planar" else Cc)

    def surface(self, rng):
        s = N.HalfSurface()
        b = self.bview
        s.elem, s.value_range = halfpix.DTYPES[self.dtype], halfpix.RANGES[rng]
        s.layout, s.components = (halfpix.PLANAR if self.form == "planar" else halfpix.PACKED), self.comps
        for i in range(3 if self.form == "planar" else 1):
            s.plane[i], s.pitch[i], s.frame_stride[i] = b.data_ptr() + i * b.stride(1), b.stride(2), b.stride(0)
        return s

    def intact(self, poison):
        return bool(torch.all(self.buf[self.mask] == poison))

    def cpu(self):
        F_, H, W = self.dims
        w = self.bview.cpu().contiguous().view(self.dtype)
        if self.form == "planar":
            return w.reshape(self.shape)
        w = w.reshape(F_, H, W, self.comps)
        return w.permute(0, 3, 1, 2) if self.form == "cl" else w


YMAT = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]
RS_FORMS = (("tile", 0), (None, 0), (None, 5), (None, 22))


def call_resize(pc: Pitched, rng, oh, ow, aa, mul=2.0, add=-1.0, y_step=2, form=None, strip=0):
    """vs_resize_pre_half; form "tile" keeps the tile kernel, `strip` sets the strip height of the row-streaming one"""
    F_, H, W = pc.dims
    rgb_buf, rgb = _guarded(torch.full((F_, oh, ow, 4), float("nan")).cuda(), -7.0)
    key_buf, key = _guarded(torch.full(((F_ + y_step - 1) // y_step, oh, ow, 4), float("nan")).cuda(), -7.0)
    surf = pc.surface(rng)
    with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", int(strip)):
        N.check(N.lib().vs_resize_pre_half(C.byref(surf), F_, H, W, oh, ow, int(aa), N.ptr(rgb), mul, add, N.ptr(key), y_step,
                                           (C.c_float * 3)(*YMAT), None), "vs_resize_pre_half")
        torch.cuda.synchronize()
    assert _guards_intact(rgb_buf, -7.0) and _guards_intact(key_buf, -7.0)        # the red zones of the low-resolution outputs
    return rgb, key


def call_tail(src: Pitched, dst: Pitched, rng, eng, delta, hm, variant, step=2, mode=2, scaling_w=0.2):
    F_, H, W = src.dims
    d = N.TailHalfDesc()
    d.src, d.dst = src.surface(rng), dst.surface(rng)
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(eng.taps43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, delta.shape[1]
    d.step, d.video_mode, d.total_key = step, mode, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = 1, 1, 1
    d.scaling_i, d.scaling_w = 1.0, scaling_w
    d.variant = variant
    N.check(N.lib().vs_embed_tail_half(C.byref(d), None), "vs_embed_tail_half")
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
@pytest.mark.parametrize("form", ["planar", "nhwc3", "nhwc4"])
@pytest.mark.parametrize("typ", R.TYPES)
def test_decode_is_exact_for_every_finite_word(typ, form):
    """an identity-size vs_resize_pre_half (oh = H, ow = W, no antialias, mul 1, add 0) of a 256 x 256 frame holding every 16-bit word (the
    non-finite ones replaced by zero) in each of the three component positions returns halfpix.to_rgb: the tile form and the row-streaming
    form, both value ranges, at the C level (odd pitch, odd base address).  Compared as bits, except that a decoded -0.0 (the one word the
    filter's `0 + 1 * v` turns into +0.0, as it does on the fp32 path) is compared as a value."""
    w = R.all_words()
    w = np.where(R.finite(w, typ), w, 0).astype(np.uint16)
    planes = np.stack([w, w[::-1], np.roll(w, 12345)]).reshape(1, 3, 256, 256)
    words = torch.from_numpy(np.ascontiguousarray(planes).view(np.int16)).view(DT[typ])
    clip = arrange(words, form)
    for rng in R.RANGES:
        want = halfpix.to_rgb(clip, LAYOUT[form], rng).permute(0, 2, 3, 1).contiguous()
        assert np.array_equal(want.numpy()[..., 0].reshape(-1).view(np.uint32), R.decode(w, typ, rng).view(np.uint32))
        for f in ("tile", None):
            pc = Pitched(clip, form, "H", level="c")
            rgb, _ = call_resize(pc, rng, 256, 256, False, mul=1.0, add=0.0, y_step=1, form=f)
            got = rgb[..., :3].cpu()
            assert torch.equal(got, want), (typ, form, rng, f)
            nz = want != 0
            assert torch.equal(got.view(torch.int32)[nz], want.view(torch.int32)[nz]), (typ, form, rng, f)
            assert torch.all(rgb[..., 3] == 0)


# ---------------------------------------------------------------------------------------------------- 2. same bits as the fp32 path
def _fp32_path(model, clip, layout, rng, msgs, is_video, lowres):
    x = halfpix.to_rgb(clip, layout, rng).cuda()
    w = model.embed(x, msgs, is_video=is_video, lowres_attenuation=lowres)["imgs_w"]
    return halfpix.from_rgb(w, like=clip.cuda(), layout=layout, value_range=rng)


@pytest.mark.parametrize("which", ["tiny", "tinyc"])
@pytest.mark.parametrize("typ,rng,form", GRID)
def test_embed_half_gives_the_bits_of_the_fp32_path(typ, rng, form, which, tiny, tinyc):
    """embed_half(x) is torch.equal (on the raw words) to from_rgb(embed(to_rgb(x))['imgs_w'], like=x): the three video modes x attenuation
    off / low-res / full-res, Cd = 1 (tiny) and 3 (tinyc), tail_variant 1 everywhere and 4 where the row-streaming form applies, set on the
    engine for both sides; the seven shapes in turn; smooth pictures, the wild clip (overshoot, signed zeros, a dark frame of fp16
    subnormals, an all-black frame, random words); image mode with a message per frame"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    msgs = synthetic_msgs(1, spec.nbits, seed=7)
    k = GRID.index((typ, rng, form))
    layout = LAYOUT[form]
    for i, (mode, att) in enumerate(itertools.product(MODES, ATTS)):
        shape = NAMES[(i + k) % len(NAMES)]
        x01 = wild(shape, typ, seed=20 + i) if i % 3 == 2 else smooth(shape, seed=20 + i)
        clip = pack(x01, typ, rng, form, alpha_seed=i)
        for variant in variants_of(shape):
            with settings(model, mode, att, variant) as lowres:
                got = model.embed_half(Pitched(clip, form, shape).view, msgs, value_range=rng, layout=layout, lowres_attenuation=lowres)
                want = _fp32_path(model, clip, layout, rng, msgs, True, lowres)
            out = got["imgs_w"]
            assert out.is_cuda and out.dtype == DT[typ] and out.shape == clip.shape and out.stride() == clip.stride()
            assert _same(out, want), (typ, rng, form, which, shape, mode, att, variant, int((_bits(out) != _bits(want)).sum()))
            assert got["msgs"].shape == (SHAPES[shape][0], spec.nbits)
            if i % 3 != 2 and shape in STREAMS:
                assert not _same(out, clip)
    # image mode: a message row per frame, the embedder on every frame, no preds_w
    shape = NAMES[k % len(NAMES)]
    F_ = SHAPES[shape][0]
    mf = synthetic_msgs(F_, spec.nbits, seed=8)
    clip = pack(wild(shape, typ, seed=3) if k % 2 else smooth(shape, seed=3), typ, rng, form)
    with settings(model, "repeat", "full", 1, chunk=2) as lowres:
        got = model.embed_half(Pitched(clip, form, shape).view, mf, is_video=False, value_range=rng, layout=layout, lowres_attenuation=lowres)
        want = _fp32_path(model, clip, layout, rng, mf, False, lowres)
    assert set(got) == {"imgs_w", "msgs"} and torch.equal(got["msgs"], mf)
    assert got["imgs_w"].stride() == clip.stride() and _same(got["imgs_w"], want), (typ, rng, form, which, shape, "image mode")


def test_dark_frame_keeps_its_fp16_subnormals(tiny):
    """a unit-range fp16 frame whose components lie in (0, 2^-14), no watermark: the words come back (a conversion that flushes subnormals
    would return zeros); with the watermark the result still equals the fp32 path (test above) and holds subnormal words"""
    spec, sd, model = tiny
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 131, 259, generator=g) * (2.0 ** -14) * 0.99 + 2.0 ** -24
    clip = x.to(torch.float16)
    assert torch.all((clip > 0) & (clip < 2.0 ** -14))
    sw0 = model.blender.scaling_w
    try:
        model.blender.scaling_w = 0.0
        for variant in (1, 4):
            with settings(model, "repeat", "off", variant):
                out = model.embed_half(Pitched(clip, "planar", "G").view)["imgs_w"]
            assert _same(out, clip), variant
    finally:
        model.blender.scaling_w = sw0


# ---------------------------------------------------------------------------------------------------- 3. detect
@pytest.mark.parametrize("typ,rng,form", GRID)
def test_detect_half_gives_the_bits_of_the_fp32_path(typ, rng, form, tiny):
    """detect_half(x) is torch.equal to detect(to_rgb(x)): both antialias values, both is_video values, the seven shapes"""
    spec, sd, model = tiny
    k = GRID.index((typ, rng, form))
    layout = LAYOUT[form]
    with settings(model):
        for i, shape in enumerate(NAMES):
            clip = pack(wild(shape, typ, seed=40 + i) if (i + k) % 3 == 2 else smooth(shape, seed=40 + i), typ, rng, form)
            x = halfpix.to_rgb(clip, layout, rng).cuda()
            for aa in (True, False):
                it = {"mode": "bilinear", "align_corners": False, "antialias": aa}
                is_video = bool((i + int(aa)) % 2)
                got = model.detect_half(Pitched(clip, form, shape).view, is_video=is_video, value_range=rng, layout=layout, interpolation=it)["preds"]
                want = model.detect(x, is_video=is_video, interpolation=it)["preds"]
                assert got.shape == (SHAPES[shape][0], spec.nbits + 1) and torch.equal(got, want), (typ, rng, form, shape, aa, is_video)


# ---------------------------------------------------------------------------------------------------- 4. forms agree
@pytest.mark.parametrize("form", ["planar", "nhwc3", "nhwc4"])
@pytest.mark.parametrize("typ", R.TYPES)
def test_resize_forms_agree(typ, form):
    """tile form, row-streaming form and odd strip heights of vs_resize_pre_half: the same bits (shapes A, C, G at the C level)"""
    for j, shape in enumerate(("A", "C", "G")):
        rng = R.RANGES[j % 2]
        clip = pack(wild(shape, typ, seed=3), typ, rng, form)
        for aa in (True, False):
            res = [call_resize(Pitched(clip, form, shape, level="c"), rng, S, S, aa, form=f, strip=s) for f, s in RS_FORMS]
            assert not torch.isnan(res[0][0]).any() and not torch.isnan(res[0][1]).any()
            for other in res[1:]:
                assert torch.equal(other[0], res[0][0]) and torch.equal(other[1], res[0][1]), (typ, form, shape, aa)


# ---------------------------------------------------------------------------------------------------- 5. alpha
@pytest.mark.parametrize("typ", R.TYPES)
def test_alpha_travels_untouched(typ, tiny):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=9)
    for j, (shape, variant) in enumerate((("G", 4), ("G", 1), ("D", 1), ("H", 1))):
        rng = R.RANGES[j % 2]
        clip = pack(smooth(shape, seed=14, lo=0.2, hi=0.8), typ, rng, "nhwc4", alpha_seed=j)
        with settings(model, "repeat", "full", variant) as lowres:
            out = model.embed_half(Pitched(clip, "nhwc4", shape).view, msgs, value_range=rng, layout="nhwc", lowres_attenuation=lowres)["imgs_w"]
        a_in, a_out = _bits(clip)[..., 3], _bits(out)[..., 3]
        assert len(torch.unique(a_in)) > 1 and torch.equal(a_in, a_out), (typ, shape, variant)
        assert shape != "G" or not torch.equal(_bits(out)[..., :3], _bits(clip)[..., :3])               # ... and RGB changed


# ---------------------------------------------------------------------------------------------------- 6. identity
@pytest.mark.parametrize("typ,rng,form", GRID)
def test_identity_without_a_watermark(typ, rng, form, tiny):
    """scaling_w = 0, attenuation off: the output is from_rgb(to_rgb(x), like=x); for unit-range clips with values in [0, 1] (no -0.0: it
    encodes as +0.0) it is x's own words"""
    spec, sd, model = tiny
    layout = LAYOUT[form]
    sw0 = model.blender.scaling_w
    try:
        model.blender.scaling_w = 0.0
        for shape in ("A", "D", "G", "H"):
            x01 = wild(shape, typ, seed=17) if shape in ("A", "D") else smooth(shape, seed=17)
            clip = pack(x01, typ, rng, form)
            want = halfpix.from_rgb(halfpix.to_rgb(clip, layout, rng), like=clip, layout=layout, value_range=rng)
            for variant in variants_of(shape):
                with settings(model, "repeat", "off", variant):
                    out = model.embed_half(Pitched(clip, form, shape).view, value_range=rng, layout=layout)["imgs_w"]
                assert _same(out, want), (typ, rng, form, shape, variant)
                if rng == "unit" and shape in ("G", "H"):
                    assert _same(out, clip)
    finally:
        model.blender.scaling_w = sw0


# ---------------------------------------------------------------------------------------------------- 7. against the CPU oracle
@pytest.mark.parametrize("shape", ["A", "G"])
@pytest.mark.parametrize("typ,rng,form", [("f16", "unit", "planar"), ("bf16", "signed", "cl"), ("f16", "signed", "nhwc4"), ("bf16", "unit", "nhwc3")])
def test_against_the_cpu_oracle_in_float64(typ, rng, form, shape, tiny):
    """with y the value of oracle.videoseal_ref.embed_video (float64, on to_rgb(clip).double()) mapped to the stored range and g = 1 (unit) or
    2 (signed), every stored output o satisfies |float(o) - y| <= ulp_dtype(max(|o|, |y|)) / 2 + g * TOL_IMG"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=11)
    sd64 = {k_: (v.double() if v.dtype.is_floating_point else v) for k_, v in sd.items()}
    layout = LAYOUT[form]
    clip = pack(smooth(shape, seed=19), typ, rng, form)
    x64 = halfpix.to_rgb(clip, layout, rng).double()
    ref = O.embed_video(sd64, spec, x64, msgs, chunk_size=2, step_size=2, lowres_attenuation=True)["imgs_w"].clamp(0.0, 1.0)
    with settings(model, "repeat", "lowres", 0) as lowres:
        out = model.embed_half(Pitched(clip, form, shape).view, msgs, value_range=rng, layout=layout, lowres_attenuation=lowres)["imgs_w"]
    px = out.cpu() if layout == "nhwc" else out.cpu().permute(0, 2, 3, 1)
    o = R.words_to_f64(_bits(px[..., :3]).numpy().view(np.uint16), typ)
    y = ref.permute(0, 2, 3, 1).numpy()
    g = 1.0
    if rng == "signed":
        y, g = y * 2.0 - 1.0, 2.0
    bound = R.ulp(np.maximum(np.abs(o), np.abs(y)), typ) / 2 + g * TOL_IMG
    err = np.abs(o - y)
    print(f"embed_half {typ} {rng} {form} {shape}: max |o - y| = {err.max():.3e}, max (|o - y| - ulp / 2) = {(err - (bound - g * TOL_IMG)).max():.3e} "
          f"(allowed {g * TOL_IMG:.1e})")
    assert np.all(err <= bound), (typ, rng, form, shape, float((err - bound).max()))


# ---------------------------------------------------------------------------------------------------- 8. red zones
@pytest.mark.parametrize("full_jnd", [True, False])
@pytest.mark.parametrize("typ,form", [("f16", "planar"), ("bf16", "nhwc3"), ("f16", "nhwc4"), ("bf16", "planar")])
def test_red_zones_and_pitch_padding(typ, form, full_jnd, tiny):
    """source and destination between guard bands with poisoned pitch padding (odd byte pitches and base addresses) and spare rows: the source
    is unchanged, no byte of the destination outside its rows' payload is written, two source poisons and several strip heights give the
    same words; the resize's destinations keep their guards (call_resize checks them)"""
    spec, sd, model = tiny
    eng = model._engine()
    for j, shape in enumerate(("C", "D", "G", "H")):
        rng = R.RANGES[j % 2]
        F_, H, W, _ = SHAPES[shape]
        clip = pack(wild(shape, typ, seed=50), typ, rng, form)
        g = torch.Generator().manual_seed(51)
        delta = torch.tanh(torch.randn((F_ + 1) // 2, 1, S, S, generator=g)).cuda()
        hm = None if full_jnd else torch.rand(F_ * S * S, generator=g).cuda()
        results = []
        runs = ((0xA5, 0, 0), (0x3C, 0, 0), (0xA5, 0, 4), (0x3C, 0, 20), (0xA5, 1, 0), (0x3C, 1, 0))
        for poison, variant, strip in runs:
            src = Pitched(clip, form, shape, poison, level="c")
            keep = src.buf.clone()
            dst = Pitched(clip, form, shape, 0x5A, level="c", extra=4, fill=False)
            with torch.cuda.device(eng.dev), N.debug("TAIL_STRIP", strip):
                rgb, key = call_resize(src, rng, S, S, True)
                call_tail(src, dst, rng, eng, delta, hm, variant)
            assert torch.equal(src.buf, keep)                                                        # the source is read only
            assert dst.intact(0x5A), (typ, form, shape, variant, strip)                              # guards, pitch padding, spare rows
            out = dst.cpu()
            assert shape == "H" or not _same(out, clip)
            results.append((variant, [rgb.cpu(), key.cpu(), _bits(out)]))
        for variant, other in results[1:]:
            first = results[0][1] if (variant == 0 or not full_jnd or shape not in STREAMS) else results[4][1]
            for a, b in zip(first, other):
                assert torch.equal(a, b), (typ, form, shape, variant)


# ---------------------------------------------------------------------------------------------------- 9. graphs
def test_graph_replay_matches_eager(tiny):
    spec, sd, model = tiny
    outs = {}
    n0 = len(model._graphs)
    with settings(model, "repeat", "lowres", 0, chunk=8, step=2):
        try:
            for use in (False, True):
                model.use_graphs = use
                res = []
                for seed in (1, 2, 3):
                    pc = Pitched(pack(smooth("A", seed=seed), "bf16", "signed", "planar"), "planar", "A")
                    msgs = synthetic_msgs(1, spec.nbits, seed=seed)
                    w = model.embed_half(pc.view, msgs, value_range="signed")["imgs_w"]
                    res.append((w, model.detect_half(w, value_range="signed")["preds"]))
                outs[use] = res
            assert len(model._graphs) == n0 + 2           # one embed graph + one detect graph, reused for the 3 clips
            for (w0, p0), (w1, p1) in zip(outs[False], outs[True]):
                assert _same(w0, w1) and torch.equal(p0, p1)
            model.detect_half(outs[True][0][0], value_range="unit")           # the graph is keyed by the value range
            assert len(model._graphs) == n0 + 3
        finally:
            model.use_graphs = False


# ---------------------------------------------------------------------------------------------------- 10. refusals
def test_c_level_refusals():
    lib = N.lib()
    UNS = N.ERR_UNSUPPORTED
    F_, H, W, _ = SHAPES["D"]
    rgb = torch.zeros((F_, S, S, 4), device="cuda")
    delta = torch.zeros(1, 1, S, S, device="cuda")
    for form in ("planar", "nhwc4"):
        clip = pack(smooth("D"), "f16", "unit", form)
        pc, other = Pitched(clip, form, "D", level="c"), Pitched(clip, form, "D", level="c")
        rowb = W * 2 * (1 if form == "planar" else 4)

        def resize(s, H_=H, W_=W, dst=N.ptr(rgb)):
            return lib.vs_resize_pre_half(C.byref(s), F_, H_, W_, S, S, 1, dst, 1.0, 0.0, None, 1, None, None)
        for name, value in (("elem", 2), ("elem", -1), ("layout", 2), ("value_range", 2), ("components", 2), ("components", 5),
                            ("components", 4 if form == "planar" else 1)):
            s = pc.surface("unit")
            setattr(s, name, value)
            assert resize(s) == UNS, (form, name, value)
        s = pc.surface("unit")
        assert resize(s, H_=0) == -1 and resize(s, W_=0) == -1 and resize(s, dst=None) == -1
        assert lib.vs_resize_pre_half(None, F_, H, W, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, None) == -1
        s.pitch[0] = rowb - 1
        assert resize(s) == -1                                                     # a pitch shorter than its row
        for i in range(3 if form == "planar" else 1):
            s = pc.surface("unit")
            s.plane[i] = None
            assert resize(s) == -1

        def desc():
            d = N.TailHalfDesc()
            d.src, d.dst = pc.surface("unit"), other.surface("unit")
            d.delta, d.F, d.H, d.W, d.S_h, d.S_w, d.Cd, d.step, d.total_key, d.clamp = N.ptr(delta), F_, H, W, S, S, 1, 2, 1, 1
            return d
        tail = lambda d: lib.vs_embed_tail_half(C.byref(d), None)                  # noqa: E731
        for name, value, code in (("attenuate", 2, UNS), ("preds_w", N.ptr(delta), UNS), ("variant", 2, UNS), ("variant", 4, UNS),
                                  ("clamp", 0, -1), ("delta", None, -1), ("F", 0, -1), ("H", 0, -1), ("W", 0, -1), ("S_w", 0, -1), ("Cd", 2, -1),
                                  ("video_mode", 3, -1)):
            d = desc()
            setattr(d, name, value)
            assert tail(d) == code, (form, name, value)
        for name, value in (("elem", 1), ("value_range", 1), ("layout", 1 if form == "planar" else 0), ("components", 3 if form == "nhwc4" else 4)):
            d = desc()
            setattr(d.dst, name, value)                                            # source and destination of different formats
            assert tail(d) == UNS, (form, name)
        d = desc()
        d.src.elem = d.dst.elem = 7
        assert tail(d) == UNS
        d = desc()
        d.dst = pc.surface("unit")                                                 # the destination is the source
        assert tail(d) == -1
        d = desc()
        d.dst.pitch[0] = rowb - 1
        assert tail(d) == -1
        d = desc()
        d.src.plane[0] = None
        assert tail(d) == -1
        assert lib.vs_embed_tail_half(None, None) == -1
        torch.cuda.synchronize()
        assert pc.intact(0xA5) and other.intact(0xA5) and _same(other.cpu(), clip)         # nothing was launched


def test_python_refusals_empty_and_host_clips(tiny, monkeypatch):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=3)
    with settings(model):
        x = pack(smooth("B"), "f16", "unit", "planar").cuda()
        p4 = pack(smooth("B"), "bf16", "signed", "nhwc4").cuda()
        for clip, kw in ((x.float(), {}), ((x * 255).to(torch.uint8), {}), (x.double(), {})):
            with pytest.raises(ValueError, match="embed_rgb"):
                model.embed_half(clip, msgs, **kw)
            with pytest.raises(ValueError, match="detect_rgb"):
                model.detect_half(clip, **kw)
        bad = [(x, dict(layout="nchw4")), (x, dict(value_range="full")), (x, dict(layout="nhwc")), (p4, dict(layout="nchw")),
               (p4.permute(0, 3, 1, 2), {}), (x[0], {}), (x[:, :, :, ::2], {}), (x[0:1].expand(6, 3, 72, 88), {})]
        for clip, kw in bad:
            with pytest.raises(ValueError):
                model.embed_half(clip, msgs, **kw)
            with pytest.raises(ValueError):
                model.detect_half(clip, **kw)
        with pytest.raises(AssertionError, match="Message should be unique"):
            model.embed_half(x, synthetic_msgs(2, spec.nbits, seed=3))
        with pytest.raises(ValueError, match="rows"):
            model.embed_half(x, synthetic_msgs(2, spec.nbits, seed=3), is_video=False)
        clamp0 = model.clamp
        try:
            model.clamp = False
            for iv in (True, False):
                with pytest.raises(NotImplementedError, match="clamp=True"):
                    model.embed_half(x, None, is_video=iv)
        finally:
            model.clamp = clamp0
        labels = torch.ones(6, 72, 88, dtype=torch.uint8, device="cuda")
        with pytest.raises(NotImplementedError, match="half-precision"):
            model.embed_regions(x, labels, msgs)
        with pytest.raises(NotImplementedError, match="half-precision"):
            model.embed_psnr(x, 40.0, msgs)
        with pytest.raises(NotImplementedError, match="half-precision"):
            model.embed_images([x[0], x[1]])
        with pytest.raises(NotImplementedError, match="half-precision"):
            model.embed_clips([x])
        with pytest.raises(NotImplementedError, match="one clip"):
            model.embed_half([x], msgs)
        e = model.embed_half(p4[:0], msgs, value_range="signed", layout="nhwc")
        assert e["imgs_w"].shape == (0, 72, 88, 4) and e["imgs_w"].dtype == torch.bfloat16 and e["msgs"].shape[0] == 0
        assert model.detect_half(x[:0])["preds"].shape == (0, spec.nbits + 1)
        # a host-resident clip moves chunk by chunk and comes back on the host with the same words
        for clip, kw in ((x, {}), (p4, dict(value_range="signed", layout="nhwc")), (x.contiguous(memory_format=torch.channels_last), {})):
            dev = model.embed_half(clip, msgs, **kw)["imgs_w"]
            host = model.embed_half(clip.cpu(), msgs, **kw)["imgs_w"]
            assert not host.is_cuda and host.dtype == clip.dtype and host.stride() == dev.stride() and _same(host, dev)
            assert torch.equal(model.detect_half(clip.cpu(), **kw)["preds"], model.detect_half(clip, **kw)["preds"].cpu())
        monkeypatch.setattr(type(model), "pixelwise", property(lambda self: True))
        with pytest.raises(NotImplementedError, match="detect_half"):
            model.detect_half(x)


# ---------------------------------------------------------------------------------------------------- 12. model-level C-ABI
@pytest.mark.parametrize("typ,rng,form,shape", [("f16", "unit", "planar", "B"), ("bf16", "signed", "planar", "G"), ("f16", "signed", "nhwc4", "E"),
                                                ("bf16", "unit", "cl", "A")])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_model_level_c_api_half(which, typ, rng, form, shape, tiny, tinyc):
    """vs_model_embed_half / vs_model_detect_half equal embed_half / detect_half: words equal, logits within 1e-4 (the bound of the packed RGB,
    NV12 and YUV twins); pitched input and output surfaces, poison intact; image mode with a message per frame"""
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny if which == "tiny" else tinyc
    cm = CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=33)
    layout = LAYOUT[form]
    kw = dict(value_range=rng, layout=layout)
    clip = pack(smooth(shape, seed=60), typ, rng, form)
    with settings(model, "repeat", "lowres", 0, chunk=3, step=2):
        for lowres in (True, False):
            src = Pitched(clip, form, shape)
            py = model.embed_half(src.view, msgs, lowres_attenuation=lowres, **kw)["imgs_w"]
            dst = Pitched(clip, form, shape, 0x5A, extra=3, fill=False)
            c = cm.embed_half(src.view, msgs, out=dst.view, step=2, lowres_attenuation=lowres, **kw)
            assert _same(py, c), (which, typ, rng, form, lowres)
            assert dst.intact(0x5A)
            assert _same(py, cm.embed_half(clip.cuda(), msgs, step=2, lowres_attenuation=lowres, **kw))
        lp = model.detect_half(py, **kw)["preds"]
        assert (cm.detect_half(dst.view, **kw) - lp).abs().max().item() < 1e-4
    F_, H, W, _ = SHAPES[shape]
    mf = synthetic_msgs(F_, spec.nbits, seed=34)
    with settings(model, "repeat", "full", 0, chunk=F_):
        py = model.embed_half(src.view, mf, is_video=False, lowres_attenuation=False, **kw)["imgs_w"]
        assert _same(py, cm.embed_half(src.view, mf, step=1, lowres_attenuation=False, **kw))
    lib = N.lib()
    s_in, s_out = N.half_surface(src.view, layout, rng), N.half_surface(dst.view, layout, rng)
    s_out.value_range = 1 - s_in.value_range
    mi = msgs.to(device="cuda", dtype=torch.int32)
    ws = cm._workspace(F_, H, W, 2)
    args = (N.ptr(mi), 1, F_, H, W, 2, 0, 1, 1, N.ptr(ws), ws.numel(), None)
    assert lib.vs_model_embed_half(cm._h, C.byref(s_in), C.byref(s_out), *args) == N.ERR_UNSUPPORTED
    assert lib.vs_model_embed_half(cm._h, C.byref(s_in), C.byref(s_in), *args) == -1
    torch.cuda.synchronize()
    assert dst.intact(0x5A)
