"""fp64 envelopes of the image-domain forward kernels on structured hard frames (tests/_img_ref.py: formulas, frames, cases, metric;
tests/test_img_contract_cpu.py: the metric bites).  vs_resize_pre / vs_resize_pre_u8 in every kernel form, vs_jnd_heatmap, vs_embed_tail,
the colour ops alone, chained and as the epilogue of vs_aug_crop_resize_color, vs_resize_nchw, vs_gaussian_blur, vs_median_filter, vs_aug_warp and
the pointwise / temporal ops, called through the C ABI: per (case, frame kind)  max |got - ref64| / max |ref64|  against the formula in float64,
at most IMG_FP64_MARGIN times what the same formula costs in float32 on the CPU.  Inputs sit between NaN bands (bytes: 0xFF), outputs are
pre-filled with a sentinel between -7.0 bands: the bands must be intact and no sentinel may be left.  Every figure is printed as an IMG-ENVELOPE
line; profiles/img_fp64_envelope.txt is such a run on an MI355X."""
import contextlib
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _envelope as E  # noqa: E402
from tests import _img_ref as R  # noqa: E402
from tests._guards import _guarded, _guards_intact  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd.native import TailDesc  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = 77.25                   # pre-fill of every output: no kernel under test can produce it (all outputs lie in [-4, 4])
F32, F64 = torch.float32, torch.float64


def _in(t):
    """(buffer, view) of a float input between NaN bands, of a uint8 input between 0xFF bands"""
    return _guarded(t.to(DEV), NAN if t.dtype.is_floating_point else 255)


def _out(*shape, dtype=F32):
    """(buffer, view) of an output pre-filled with the sentinel between -7.0 bands (bytes: 0xA5 between 0x5A bands)"""
    if dtype == torch.uint8:
        return _guarded(torch.full(shape, 0xA5, dtype=dtype, device=DEV), 0x5A)
    return _guarded(torch.full(shape, SENT, dtype=dtype, device=DEV), -7.0)


def _done(outs, ins=()):
    """after the launch: every band intact, every output element written; returns the outputs on the CPU"""
    torch.cuda.synchronize()
    for buf, view in ins:
        assert _guards_intact(buf, NAN if buf.dtype.is_floating_point else 255), "a band around an input changed"
    res = []
    for buf, view in outs:
        assert _guards_intact(buf, -7.0 if buf.dtype.is_floating_point else 0x5A), "a kernel wrote outside its output"
        v = view.cpu()
        assert not (v == SENT).any() if v.dtype.is_floating_point else True, "an output element was not written"
        res.append(v)
    return res


@contextlib.contextmanager
def _switch(sw):
    """development switches {name: value} for the calls inside the block"""
    with contextlib.ExitStack() as stack:
        for k, v in sw.items():
            stack.enter_context(N.debug(k, v))
        yield


def _nchw(t):
    """[B, oh, ow, 4] NHWC(4) -> ([B, 3, oh, ow], channel 3)"""
    return t[..., :3].permute(0, 3, 1, 2), t[..., 3]


# ------------------------------------------------------------------------------------------------------------------------ vs_resize_pre
YM = (C.c_float * 3)(*R.YMAT)


def _resize_pre_lines(x, u8, H, W, oh, ow, aa, sw, rows):
    """one frame kind through vs_resize_pre (or _u8): rgb + Y key frames, then rgb key frames; appends (output, kind, hip, yard) to rows"""
    L = N.lib()
    B = x.shape[0]
    src = x if u8 is None else u8
    want64 = R.resize_pre(x, (oh, ow), aa, 2.0, -1.0, 2, R.YMAT, F64)
    want32 = R.resize_pre(x, (oh, ow), aa, 2.0, -1.0, 2, R.YMAT, F32)
    krgb64 = R.resize_pre(x, (oh, ow), aa, 2.0, -1.0, 2, None, F64)[1]
    krgb32 = R.resize_pre(x, (oh, ow), aa, 2.0, -1.0, 2, None, F32)[1]
    got = {}
    for ymat in (YM, None):
        xin, rgb, key = _in(src), _out(B, oh, ow, 4), _out((B + 1) // 2, oh, ow, 4)
        with _switch(sw):
            if u8 is None:
                N.check(L.vs_resize_pre(N.ptr(xin[1]), B, 3, H, W, oh, ow, aa, N.ptr(rgb[1]), 2.0, -1.0, N.ptr(key[1]), 2, ymat, N.stream()), "vs_resize_pre")
            else:
                N.check(L.vs_resize_pre_u8(N.ptr(xin[1]), B, H, W, oh, ow, aa, N.ptr(rgb[1]), 2.0, -1.0, N.ptr(key[1]), 2, ymat, N.stream()), "vs_resize_pre_u8")
            g_rgb, g_key = _done([rgb, key], [xin])
        c, pad = _nchw(g_rgb)
        assert (pad == 0).all()
        if ymat is not None:
            assert (g_key[..., 1:] == 0).all()
            got["rgb"], got["key-y"] = c, g_key[..., 0][:, None]
        else:
            assert torch.equal(c, got["rgb"])          # the rgb output does not depend on the key mode
            k, pad = _nchw(g_key)
            assert (pad == 0).all()
            got["key-rgb"] = k
    for name, r64, r32 in (("rgb", want64[0], want32[0]), ("key-y", want64[1], want32[1]), ("key-rgb", krgb64, krgb32)):
        rows.setdefault(name, []).append((E.frame_err(got[name], r64), E.frame_err(r32, r64)))


def _emit(case, rows, kinds):
    for name, figs in rows.items():
        R.envelope(f"{case} {name}", [(k, h, y) for k, (h, y) in zip(kinds, figs)])


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=[c[0] for c in R.RESIZE_CASES])
def test_resize_pre_fp64_envelope(case):
    """every form of vs_resize_pre (row-streaming <128> / <64> with scalar and 16-byte loads, strips of 1, 7 and 80 rows, the staged and the
    unstaged tile kernel, 128 taps, up-scales, one input row) on noise, checkerboard, constant, ramp and impulse frames; rgb and key outputs,
    key_step 2, both key modes"""
    tag, H, W, oh, ow, aa, sw = case
    rows = {}
    fr = R.hard_frames(H, W)
    for kind, x in fr.items():
        _resize_pre_lines(x, None, H, W, oh, ow, aa, sw, rows)
    _emit(f"resize_pre {tag} {H}x{W}->{oh}x{ow} aa={aa}", rows, list(fr))


@pytest.mark.parametrize("aa", [0, 1])
def test_resize_pre_identity_size_is_bit_equal_to_the_affine_map(aa):
    H, W = R.RESIZE_IDENTITY
    L = N.lib()
    for kind, x in R.hard_frames(H, W).items():
        xin, rgb = _in(x), _out(2, H, W, 4)
        N.check(L.vs_resize_pre(N.ptr(xin[1]), 2, 3, H, W, H, W, aa, N.ptr(rgb[1]), 2.0, -1.0, None, 1, None, N.stream()), "vs_resize_pre")
        (g,) = _done([rgb], [xin])
        assert torch.equal(_nchw(g)[0], x * 2.0 - 1.0), kind


def test_resize_pre_single_channel_fp64_envelope():
    """C = 1: the tile kernel, channels 1-3 of the output zero"""
    H, W, oh, ow = 93, 118, 29, 37
    L = N.lib()
    lines = []
    for kind, x3 in R.hard_frames(H, W).items():
        x = x3[:, :1].contiguous()
        r64, r32 = R.resize_ref(x, (oh, ow), 1)
        xin, rgb = _in(x), _out(2, oh, ow, 4)
        N.check(L.vs_resize_pre(N.ptr(xin[1]), 2, 1, H, W, oh, ow, 1, N.ptr(rgb[1]), 2.0, -1.0, None, 1, None, N.stream()), "vs_resize_pre")
        (g,) = _done([rgb], [xin])
        assert (g[..., 1:] == 0).all()
        lines.append((kind, E.frame_err(g[..., 0][:, None], r64 * 2 - 1), E.frame_err(r32 * 2 - 1, r64 * 2 - 1)))
    R.envelope(f"resize_pre C=1 {H}x{W}->{oh}x{ow} aa=1 rgb", lines)


@pytest.mark.parametrize("H,W,oh,ow,aa", R.RESIZE_U8_CASES)
def test_resize_pre_u8_fp64_envelope(H, W, oh, ow, aa):
    """RGB24 frames (the five kinds quantised to bytes): these row pitches and window starts take the staging path through byte misalignments 0-3;
    reference from u8 / 255 in float64"""
    rows = {}
    fr = R.hard_frames(H, W)
    for kind, x in fr.items():
        u8 = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        xq = u8.permute(0, 3, 1, 2).double() / 255
        _resize_pre_lines(xq, u8, H, W, oh, ow, aa, {}, rows)
    _emit(f"resize_pre_u8 {H}x{W}->{oh}x{ow} aa={aa}", rows, list(fr))


# ------------------------------------------------------------------------------------------------------------------------ vs_jnd_heatmap
T43 = (C.c_float * 43)(*[float(v) for v in R.JND_TAPS])


def _jnd_launch(x, nhwc=False):
    B, _, H, W = x.shape
    src = x.permute(0, 2, 3, 1).contiguous() if nhwc else x
    st = (3 * H * W, 1, 3 * W, 3) if nhwc else (3 * H * W, H * W, W, 1)
    xin, hm = _in(src), _out(B, 1, H, W)
    N.check(N.lib().vs_jnd_heatmap(N.ptr(xin[1]), B, H, W, *st, T43, N.ptr(hm[1]), N.stream()), "vs_jnd_heatmap")
    return _done([hm], [xin])[0]


@pytest.mark.parametrize("H,W,nhwc", [(h, w, False) for h, w in R.JND_SHAPES] + [(70, 101, True)])
def test_jnd_heatmap_fp64_envelope(H, W, nhwc):
    """noise, checkerboard, flat, black and frames on the la = 127 jump; a frame smaller than a tile's halo, a tile edge on the frame edge, NCHW and
    NHWC strides.  A pixel whose float64 la is within 127 x 2^-18 of the jump may match either branch, every other pixel its own"""
    lines = []
    for kind, x in R.jnd_frames(H, W).items():
        own, other, amb, y32 = R.jnd_ref(x)
        assert float(amb.float().mean()) <= R.JND_SHARE          # condition on the reference alone
        got = _jnd_launch(x, nhwc)
        lines.append((kind, E.cand_err(got, own, other, amb), E.cand_err(y32, own, other, amb)))
    R.envelope(f"jnd_heatmap {H}x{W}{' nhwc strides' if nhwc else ''}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_embed_tail
def _tail_launch(imgs, delta, hm_low, cfg, Cd, S, want_pw, variant, io_u8=False):
    Fn, _, H, W = imgs.shape
    src = (imgs * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() if io_u8 else imgs
    xin = _in(src)
    out = _out(Fn, H, W, 3, dtype=torch.uint8) if io_u8 else _out(Fn, 3, H, W)
    pw = _out(Fn, Cd, H, W) if want_pw else None
    din = _in(delta)
    hin = _in(hm_low) if hm_low is not None else None
    d = TailDesc()
    d.imgs, d.out, d.preds_w = N.ptr(xin[1]), N.ptr(out[1]), (N.ptr(pw[1]) if want_pw else None)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(din[1]), (N.ptr(hin[1]) if hin else None), C.cast(T43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = Fn, H, W, S, S, Cd
    d.step, d.video_mode, d.total_key = cfg["step"], cfg["mode"], cfg["total_key"]
    d.attenuate, d.clamp, d.antialias = cfg["attenuate"], cfg["clamp"], cfg["aa"]
    d.scaling_i, d.scaling_w, d.io_u8, d.variant = cfg["si"], cfg["sw"], int(io_u8), variant
    N.check(N.lib().vs_embed_tail(C.byref(d), N.stream()), "vs_embed_tail")
    res = _done([out] + ([pw] if want_pw else []), [xin, din] + ([hin] if hin else []))
    return res[0], (res[1] if want_pw else None)


def _tail_case(case):
    tag, Fn, H, W, S, Cd, low, want_pw, cfg = case
    delta, hm = R.tail_inputs(Fn, Cd, S, cfg["step"])
    return delta, (hm if low else None), dict(cfg, total_key=cfg["total_key"] or delta.shape[0])


@pytest.mark.parametrize("case", R.TAIL_CASES, ids=[c[0] for c in R.TAIL_CASES])
def test_embed_tail_fp64_envelope(case):
    """variants 1 (43-tap JND), 2 (separable stencils on 16-row tiles) and 4 (row-streaming where it applies), each held to the float64 tail, not
    to each other: key-frame expansion in the three video modes, low-resolution heat-map, full JND in both orders of operations, preds_w, Cd 1 / 3,
    both clamps, staged and unstaged taps, a down-resized delta, frames smaller than a tile; noise, flat and jump frames"""
    tag, Fn, H, W, S, Cd, low, want_pw, _ = case
    delta, hm, cfg = _tail_case(case)
    rows = {}
    kinds = []
    for kind, imgs in R.tail_frames(Fn, H, W).items():
        own, other, amb, y32 = R.tail_ref(imgs, delta, hm, cfg)
        assert float(amb.float().mean()) <= R.JND_SHARE
        kinds.append(kind)
        for variant in (1, 2, 4):
            got, gpw = _tail_launch(imgs, delta, hm, cfg, Cd, S, want_pw, variant)
            rows.setdefault(f"v{variant} out", []).append((E.cand_err(got, own[0], other[0], amb), E.cand_err(y32[0], own[0], other[0], amb)))
            if want_pw:
                rows.setdefault(f"v{variant} preds_w", []).append((E.cand_err(gpw, own[1], other[1], amb), E.cand_err(y32[1], own[1], other[1], amb)))
    _emit(f"embed_tail {tag} F={Fn} {H}x{W} S={S} Cd={Cd}", rows, kinds)


def test_embed_tail_u8_bytes_are_within_one_level_of_the_float64_tail():
    """io_u8 on the first configuration: every output byte is trunc(255 ref64) or, where 255 ref64 is within 255 x margin x yardstick of an integer,
    one level beside it (a pixel in the band of the JND jump may take either branch's byte)"""
    case = R.TAIL_CASES[0]
    tag, Fn, H, W, S, Cd, low, want_pw, _ = case
    delta, hm, cfg = _tail_case(case)
    for kind, imgs in R.tail_frames(Fn, H, W).items():
        imgs = ((imgs * 255).round().to(torch.uint8).float() / 255.0)          # the fp32 value the kernel reads: float(u) / 255.0f
        own, other, amb, y32 = R.tail_ref(imgs, delta, hm, cfg)
        yard = max(E.cand_err(y32[0], own[0], other[0], amb), E.U32) * float(own[0].abs().max())
        got = _tail_launch(imgs, delta, hm, cfg, Cd, S, False, 0, io_u8=True)[0].permute(0, 3, 1, 2).double()

        def ok(ref):
            v = 255 * ref
            near = (v - v.round()).abs() <= 255 * R.IMG_FP64_MARGIN * yard
            return (got == v.floor()) | (near & ((got - v.floor()).abs() <= 1))
        good = ok(own[0]) | (amb & ok(other[0]))
        print(f"IMG-U8 embed_tail io_u8 {kind}: {int((got != (255 * own[0]).floor()).sum())} of {got.numel()} bytes beside trunc(255 ref64), {int((~good).sum())} unexplained")
        assert good.all(), (kind, int((~good).sum()))


# ------------------------------------------------------------------------------------------------------------------------ colour ops
def _ops(ops):
    return (C.c_int * len(ops))(*[o for o, _ in ops]), (C.c_float * len(ops))(*[f for _, f in ops])


def _color_launch(x, ops, chain):
    L = N.lib()
    Fn, _, H, W = x.shape
    xin, out = _in(x), _out(Fn, 3, H, W)
    n = int(L.vs_aug_color_scratch_floats(Fn, H, W))
    sbuf, scr = _guarded(torch.full((n,), NAN, device=DEV), -7.0)
    if chain:
        oa, fa = _ops(ops)
        N.check(L.vs_aug_color_chain(N.ptr(xin[1]), N.ptr(out[1]), Fn, H, W, len(ops), oa, fa, N.ptr(scr), N.stream()), "vs_aug_color_chain")
    else:
        N.check(L.vs_aug_color(N.ptr(xin[1]), N.ptr(out[1]), Fn, H, W, ops[0][0], ops[0][1], N.ptr(scr), N.stream()), "vs_aug_color")
    (g,) = _done([out], [xin])
    assert _guards_intact(sbuf, -7.0)
    return g


@pytest.fixture(scope="module")
def colour_inputs():
    g = torch.Generator().manual_seed(9)
    noise = torch.rand(3, 3, 300, 300, generator=g) * torch.tensor([1.0, 0.7, 0.4]).view(3, 1, 1, 1)          # each frame a different mean
    return {"pixels": R.hard_pixels(), "noise300": noise}          # 300 x 300 > 65536 pixels: the strided branch of the contrast partial sums


@pytest.mark.parametrize("name,op,f", R.COLOR_CASES, ids=[f"{n}{f:g}" for n, _, f in R.COLOR_CASES])
def test_colour_op_fp64_envelope(colour_inputs, name, op, f):
    """vs_aug_color and a one-op vs_aug_color_chain on random, grey, tied, nearly grey, corner and nearly black / white pixels"""
    lines = []
    for kind, x in colour_inputs.items():
        if kind == "noise300" and op != R.OP_CONTRAST:
            continue
        r64, r32 = R.color_op(x, op, f, F64), R.color_op(x, op, f, F32)
        got = _color_launch(x, [(op, f)], False)
        assert torch.equal(_color_launch(x, [(op, f)], True), got)
        lines.append((kind, E.frame_err(got, r64), E.frame_err(r32, r64)))
    R.envelope(f"aug_color {name} factor {f:g}", lines)


def test_colour_chain_fp64_envelope(colour_inputs):
    """the chain of four ops (contrast first: it needs the mean of its input) held to the float64 chain"""
    lines = []
    for kind, x in colour_inputs.items():
        r64, r32 = R.color_chain(x, R.COLOR_CHAIN, F64), R.color_chain(x, R.COLOR_CHAIN, F32)
        lines.append((kind, E.frame_err(_color_launch(x, R.COLOR_CHAIN, True), r64), E.frame_err(r32, r64)))
    R.envelope("aug_color_chain contrast>brightness>saturation>hue", lines)


# ------------------------------------------------------------------------------------------------------------------------ plane resizes
def _crc_launch(x, crop, oh, ow, aa, ops, tile):
    L = N.lib()
    Fn, _, H, W = x.shape
    i0, j0, ch, cw = crop
    xin, out = _in(x), _out(Fn, 3, oh, ow)
    oa, fa = _ops(ops) if ops else (None, None)
    with _switch({"CROP_RESIZE_FORM": 1} if tile else {}):
        rc = L.vs_aug_crop_resize_color(N.ptr(xin[1]), N.ptr(out[1]), Fn, H, W, i0, j0, ch, cw, oh, ow, aa, len(ops), oa, fa, N.stream())
        if rc == N.ERR_UNSUPPORTED:          # the tile's source window does not fit the LDS: callers take the separate launches
            torch.cuda.synchronize()
            return None
        N.check(rc, "vs_aug_crop_resize_color")
        return _done([out], [xin])[0]


@pytest.mark.parametrize("case", R.PLANE_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}x{c[4]}-aa{c[5]}" for c in R.PLANE_CASES])
def test_plane_resizes_fp64_envelope(case):
    """vs_resize_nchw (both tap branches) and vs_aug_crop_resize_color in its streaming and its tile form, without and with the colour epilogue: the
    shapes of vs_resize_pre as planes, crops with j0 at residues 0-3 on a width-128 frame, a crop that ends on the frame's edge, 200 x 12 -> 16 x 3"""
    H, W, crop, oh, ow, aa = case
    L = N.lib()
    crop = crop or (0, 0, H, W)
    i0, j0, ch, cw = crop
    rows, kinds = {}, []
    for kind, x in R.hard_frames(H, W).items():
        kinds.append(kind)
        xc = x[:, :, i0:i0 + ch, j0:j0 + cw].contiguous()
        r64, r32 = R.resize_ref(xc, (oh, ow), aa)
        e64, e32 = R.color_chain(r64, R.CROP_CHAIN, F64), R.color_chain(r32, R.CROP_CHAIN, F32)
        xin, out = _in(xc), _out(2, 3, oh, ow)
        N.check(L.vs_resize_nchw(N.ptr(xin[1]), N.ptr(out[1]), 6, ch, cw, oh, ow, aa, N.stream()), "vs_resize_nchw")
        (g,) = _done([out], [xin])
        rows.setdefault("resize_nchw", []).append((E.frame_err(g, r64), E.frame_err(r32, r64)))
        for form, tile in (("crc stream", False), ("crc tile", True)):
            g = _crc_launch(x, crop, oh, ow, aa, [], tile)
            if g is None:
                continue
            rows.setdefault(form, []).append((E.frame_err(g, r64), E.frame_err(r32, r64)))
            g = _crc_launch(x, crop, oh, ow, aa, R.CROP_CHAIN, tile)
            rows.setdefault(form + "+colour", []).append((E.frame_err(g, e64), E.frame_err(e32, e64)))
    _emit(f"planes {H}x{W} crop {crop} -> {oh}x{ow} aa={aa}", rows, kinds)


# ------------------------------------------------------------------------------------------------------------------------ blur / median
@pytest.mark.parametrize("k", R.BLUR_KS)
def test_gaussian_blur_fp64_envelope(k):
    """k = 3, 9, 17, 33 on 93 x 118 and on the smallest legal frames (k / 2 + 1 rows or columns: the reflection reaches the far edge)"""
    L = N.lib()
    for H, W in ((93, 118), (k // 2 + 1, 40), (40, k // 2 + 1)):
        lines = []
        for kind, x in R.hard_frames(H, W).items():
            r64, r32 = R.gaussian_blur(x, k, F64), R.gaussian_blur(x, k, F32)
            xin, tmp, out = _in(x), _out(2, 3, H, W), _out(2, 3, H, W)
            N.check(L.vs_gaussian_blur(N.ptr(xin[1]), N.ptr(tmp[1]), N.ptr(out[1]), 6, H, W, k, R.blur_sigma(k), N.stream()), "vs_gaussian_blur")
            _, g = _done([tmp, out], [xin])
            lines.append((kind, E.frame_err(g, r64), E.frame_err(r32, r64)))
        R.envelope(f"gaussian_blur k={k} {H}x{W}", lines)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_median_filter_equals_the_float64_selection(k):
    L = N.lib()
    for H, W in ((93, 118), (5, 7)):
        for kind in ("noise", "checker", "impulse"):
            x = R.hard_frames(H, W)[kind]
            xin, out = _in(x), _out(2, 3, H, W)
            N.check(L.vs_median_filter(N.ptr(xin[1]), N.ptr(out[1]), 6, H, W, k, N.stream()), "vs_median_filter")
            (g,) = _done([out], [xin])
            assert torch.equal(g.double(), R.median_filter(x, k)), (k, H, W, kind)


# ------------------------------------------------------------------------------------------------------------------------ vs_aug_warp
def _warp_launch(x, kind, coeffs, oh, ow, bilinear):
    P, H, W = x.shape
    xin, out = _in(x), _out(P, oh, ow)
    co = (C.c_float * len(coeffs))(*coeffs)
    N.check(N.lib().vs_aug_warp(N.ptr(xin[1]), N.ptr(out[1]), P, H, W, oh, ow, kind, co, bilinear, N.stream()), "vs_aug_warp")
    return _done([out], [xin])[0]


def _warp_cases():
    out = [(f"rotate {a}", H, W, H, W, 0, R.rotate_coeffs(a, H, W), R.ROT_SHARE) for H, W in R.ROT_SHAPES for a in R.ROT_ANGLES]
    out += [(f"rotate 90 expand", H, W) + R.rot90_size(H, W) + (0, R.rotate_coeffs(90, H, W), 1.0) for H, W in R.ROT90_SHAPES]
    out += [(f"perspective {s}", H, W, H, W, 1, R.perspective_coeffs(*R.perspective_points(W, H, s)), R.ROT_SHARE) for H, W, s in R.PERSP_CASES]
    out.append(("exact half-pixel shift", R.HALF_PIXEL_SHIFT[1], R.HALF_PIXEL_SHIFT[2], R.HALF_PIXEL_SHIFT[1], R.HALF_PIXEL_SHIFT[2], 0, R.HALF_PIXEL_SHIFT[0], 0.0))
    return out


WARP_CASES = _warp_cases()


@pytest.mark.parametrize("case", WARP_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in WARP_CASES])
def test_warp_nearest_exact_or_candidate(case):
    """nearest: a pixel whose float64 source coordinate is farther than max(H, W) 2^-20 px from every .5 boundary equals the float64-chosen source
    pixel (zero off the frame); a pixel within the band equals one of the at most four neighbouring choices.  The quarter turn of the odd x even
    frame is all ties (candidate rule only), of the even x even frame an exact permutation; the dyadic half-pixel shift has exact ties and no band"""
    tag, H, W, oh, ow, kind, co, share = case
    exact_ties = tag.startswith("exact")
    for fk in ("noise", "checker", "impulse"):
        x = R.hard_frames(H, W)[fk].reshape(6, H, W)
        cand, amb = R.nearest_candidates(x.double(), kind, co, oh, ow, delta=0.0 if exact_ties else None)
        assert float(amb.float().mean()) <= share           # condition on the reference alone
        got = _warp_launch(x, kind, co, oh, ow, 0)
        bad = R.nearest_check(got.double(), cand)
        print(f"IMG-NEAREST {tag} {H}x{W} {fk}: ambiguous share {float(amb.float().mean()):.4f}, {bad} pixels outside their candidates")
        assert bad == 0, (tag, fk, bad)
        if tag.startswith("rotate 90") and H % 2 == 0:          # even x even: an exact pixel permutation, no pixel in the band
            assert not amb.any() and torch.equal(got, torch.rot90(x, 1, dims=(-2, -1)))


@pytest.mark.parametrize("case", [c for c in WARP_CASES if not c[0].startswith(("rotate 90", "exact"))], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_warp_bilinear_fp64_envelope(case):
    """bilinear (affine and perspective grids): the yardstick is the fp32 grid + ATen grid_sample on the CPU; the checkerboard is its hardest frame"""
    tag, H, W, oh, ow, kind, co, _ = case
    lines = []
    for fk, x4 in R.hard_frames(H, W).items():
        x = x4.reshape(6, H, W)
        r64, r32 = R.warp_bilinear(x, kind, co, oh, ow, F64), R.warp_bilinear(x, kind, co, oh, ow, F32)
        lines.append((fk, E.frame_err(_warp_launch(x, kind, co, oh, ow, 1), r64), E.frame_err(r32, r64)))
    R.envelope(f"aug_warp bilinear {tag} {H}x{W}", lines)


# ------------------------------------------------------------------------------------------------------------------------ pointwise / temporal
def _same(got, want, what):
    """bit equality, with the count, the size and the place of the differences in the message"""
    if not torch.equal(got, want):
        ne = (got != want).flatten()
        first = int(ne.nonzero()[0])
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, max |diff| {float(d.max()):.3e}, first at flat index {first}: "
                             f"got {float(got.flatten()[first])!r} want {float(want.flatten()[first])!r}")


@pytest.mark.parametrize("H,W", R.POINT_PLANES)
def test_pointwise_ops_equal_the_written_out_fp32_expression(H, W):
    """vs_aug_mask_blend, vs_aug_add_scaled, vs_aug_window_average, vs_aug_crop_flip, vs_aug_gather_frames: bit for bit the fp32 expression ATen
    evaluates (every product rounded before the add); a plane of 11 pixels, 93 x 118, and 1025 x 1024 (the grid-stride loop's second pass)"""
    L = N.lib()
    g = torch.Generator().manual_seed(H + W)
    big = H * W > 1 << 20
    Fn, Cc = (1, 1) if big else (2, 3)
    a, b = torch.rand(Fn, Cc, H, W, generator=g), torch.rand(Fn, Cc, H, W, generator=g)
    m = torch.rand(Fn, 1, H, W, generator=g)
    ai, bi, mi, out = _in(a), _in(b), _in(m), _out(Fn, Cc, H, W)
    N.check(L.vs_aug_mask_blend(N.ptr(ai[1]), N.ptr(bi[1]), N.ptr(mi[1]), N.ptr(out[1]), Fn, Cc, H, W, N.stream()), "vs_aug_mask_blend")
    (got,) = _done([out], [ai, bi, mi])
    _same(got, a * m + b * (1 - m), "vs_aug_mask_blend")
    nz = torch.randn(Fn, Cc, H, W, generator=g)
    ni, out = _in(nz), _out(Fn, Cc, H, W)
    N.check(L.vs_aug_add_scaled(N.ptr(ai[1]), N.ptr(ni[1]), 0.1, N.ptr(out[1]), a.numel(), N.stream()), "vs_aug_add_scaled")
    (got,) = _done([out], [ai, ni])
    _same(got, a + nz * torch.tensor(0.1, dtype=F32), "vs_aug_add_scaled")
    # crop windows partly outside the frame (zero fill), flip on and off
    planes = a.reshape(Fn * Cc, H, W)
    for i0, j0, h, w in ((-2, -3, H + 3, W + 5), (H // 2, W // 3, H, W), (0, 1, max(H - 1, 1), max(W - 2, 1))):
        for flip in (0, 1):
            out = _out(Fn * Cc, h, w)
            N.check(L.vs_aug_crop_flip(N.ptr(ai[1]), N.ptr(out[1]), Fn * Cc, H, W, i0, j0, h, w, flip, N.stream()), "vs_aug_crop_flip")
            (got,) = _done([out], [ai])
            _same(got, R.crop_flip(planes, i0, j0, h, w, flip), f"vs_aug_crop_flip {(i0, j0, h, w, flip)}")
    # temporal ops: F = 5 frames, half windows 0, 1 and 4 (wider than the clip); gathers with repeated and dropped frames
    clip = torch.rand(5, Cc, H, W, generator=g)
    ci = _in(clip)
    for hw, alpha in ((0, 0.4), (1, 1.0), (4, 0.6)):
        out = _out(5, Cc, H, W)
        N.check(L.vs_aug_window_average(N.ptr(ci[1]), N.ptr(out[1]), 5, Cc * H * W, hw, alpha, N.stream()), "vs_aug_window_average")
        (got,) = _done([out], [ci])
        _same(got, R.window_average(clip, hw, alpha), f"vs_aug_window_average {(hw, alpha)}")
    idx = torch.tensor([4, 4, 0, 2, 2, 1, 3], dtype=torch.int32)
    out = _out(7, Cc, H, W)
    idd = idx.to(DEV)
    N.check(L.vs_aug_gather_frames(N.ptr(ci[1]), N.ptr(idd), N.ptr(out[1]), 7, Cc * H * W, N.stream()), "vs_aug_gather_frames")
    (got,) = _done([out], [ci])
    _same(got, clip[idx.long()], "vs_aug_gather_frames")


def test_add_scaled_past_2_to_the_24_elements():
    """n = 2^24 + 5: more elements than the 65536 x 256 threads of the largest grid, and an index that an fp32 counter could not hold"""
    L = N.lib()
    n = (1 << 24) + 5
    g = torch.Generator().manual_seed(1)
    x, nz = torch.rand(n, generator=g), torch.randn(n, generator=g)
    xi, ni, out = _in(x), _in(nz), _out(n)
    N.check(L.vs_aug_add_scaled(N.ptr(xi[1]), N.ptr(ni[1]), 0.25, N.ptr(out[1]), n, N.stream()), "vs_aug_add_scaled")
    (got,) = _done([out], [xi, ni])
    _same(got, x + nz * 0.25, "vs_aug_add_scaled")
