"""fp64 envelopes of the image-domain adjoint kernels (csrc/bwd_shell.hip) on hard upstream gradients, hard frames and gates
(tests/_img_bwd_ref.py: formulas, cases, metric, bands; tests/test_img_bwd_contract_cpu.py: the metric bites).  Every kernel is called through the
C ABI: per (case, kind)  max |got - ref64| / max |ref64|  against float64 autograd of the tests/_img_ref.py formula, at most IMG_BWD_FP64_MARGIN
times what the same autograd costs in float32 on the CPU.  Inputs sit between NaN bands, outputs are pre-filled with a sentinel between -7.0 bands:
the bands must be intact and no sentinel may be left.  Every figure is printed as an IMG-BWD-ENVELOPE line; profiles/img_bwd_fp64_envelope.txt is
such a run on an MI355X."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _envelope as E  # noqa: E402
from tests import _img_bwd_ref as B  # noqa: E402
from tests import _img_ref as R  # noqa: E402
from tests._guards import _guarded, _guards_intact  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = 77.25                   # pre-fill of every output: no kernel under test produces it
F32, F64 = torch.float32, torch.float64


def _in(t):
    return _guarded(t.to(DEV).contiguous(), NAN if t.dtype.is_floating_point else 255)


def _out(*shape):
    return _guarded(torch.full(shape, SENT, dtype=F32, device=DEV), -7.0)


def _done(outs, ins=()):
    """after the launch: every band intact, every output element written; returns the outputs on the CPU"""
    torch.cuda.synchronize()
    for buf, view in ins:
        assert _guards_intact(buf, NAN if buf.dtype.is_floating_point else 255), "a band around an input changed"
    res = []
    for buf, view in outs:
        assert _guards_intact(buf, -7.0), "a kernel wrote outside its output"
        v = view.cpu()
        assert not (v == SENT).any(), "an output element was not written"
        res.append(v)
    return res


def _same(got, want, what):
    if not torch.equal(got, want):
        ne = (got != want).flatten()
        first = int(ne.nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at flat index {first}: "
                             f"got {float(got.flatten()[first])!r} want {float(want.flatten()[first])!r}")


# ------------------------------------------------------------------------------------------------------------------------ vs_resize_nchw_bwd
def _resize_bwd(dy, H, W, aa):
    P = dy.numel() // (dy.shape[-2] * dy.shape[-1])
    oh, ow = dy.shape[-2:]
    di, dx, tmp = _in(dy), _out(*dy.shape[:-2], H, W), _out(P, oh, W)
    N.check(N.lib().vs_resize_nchw_bwd(N.ptr(di[1]), N.ptr(dx[1]), P, H, W, oh, ow, aa, N.ptr(tmp[1]), N.stream()), "vs_resize_nchw_bwd")
    return _done([dx, tmp], [di])[0]


@pytest.mark.parametrize("case", B.RESIZE_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resize_bwd_fp64_envelope(case):
    """the transposes of the plane cases: block tails in both directions, 128 taps, up-scales where one input collects a dozen outputs and the
    source clamps at 0, one input row, 12.5 : 1; noise, constant, checkerboard, ramp and impulse gradients"""
    H, W, oh, ow, aa = case
    lines = []
    for kind, dy in B.hard_dy((2, 3, oh, ow)).items():
        r64, r32 = B.adjoint_pair(lambda t, dt: R.resize(t, (oh, ow), aa, dt), torch.zeros(2, 3, H, W), dy)
        lines.append((kind, E.frame_err(_resize_bwd(dy, H, W, aa), r64), E.frame_err(r32, r64)))
    B.envelope(f"resize_bwd {H}x{W}<-{oh}x{ow} aa={aa}", lines)


@pytest.mark.parametrize("aa", [0, 1])
def test_resize_bwd_identity_size_is_bit_equal_to_dy(aa):
    H, W = R.RESIZE_IDENTITY
    for kind, dy in B.hard_dy((2, 3, H, W)).items():
        _same(_resize_bwd(dy, H, W, aa), dy, f"identity resize adjoint aa={aa} {kind}")


# ------------------------------------------------------------------------------------------------------------------------ vs_gaussian_blur_bwd
@pytest.mark.parametrize("k", R.BLUR_KS)
def test_gaussian_blur_bwd_fp64_envelope(k):
    """one axis at r + 1 rows or columns (both reflection folds land on the same pixels) with a generic axis wider than a 32 x 8 block, and 33 x 47"""
    for H, W in B.BLUR_BWD_SHAPES[k]:
        lines = []
        for kind, dy in B.hard_dy((2, 3, H, W)).items():
            r64, r32 = B.adjoint_pair(lambda t, dt: R.gaussian_blur(t, k, dt), torch.zeros(2, 3, H, W), dy)
            di, tmp, dx = _in(dy), _out(2, 3, H, W), _out(2, 3, H, W)
            N.check(N.lib().vs_gaussian_blur_bwd(N.ptr(di[1]), N.ptr(tmp[1]), N.ptr(dx[1]), 6, H, W, k, R.blur_sigma(k), N.stream()), "vs_gaussian_blur_bwd")
            _, g = _done([tmp, dx], [di])
            lines.append((kind, E.frame_err(g, r64), E.frame_err(r32, r64)))
        B.envelope(f"gaussian_blur_bwd k={k} {H}x{W}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_aug_warp_bwd
def _warp_bwd(dy, H, W, kind, co, bilinear):
    P, oh, ow = dy.shape
    di, dx = _in(dy), _out(P, H, W)
    inv = B.warp_inverse(kind, co, H, W, oh, ow)
    N.check(N.lib().vs_aug_warp_bwd(N.ptr(di[1]), N.ptr(dx[1]), P, H, W, oh, ow, kind, (C.c_float * len(co))(*co), bilinear, (C.c_float * 9)(*inv),
                                    N.stream()), "vs_aug_warp_bwd")
    return _done([dx], [di])[0]


PERSP = [(f"perspective {s}", R.perspective_coeffs(*R.perspective_points(W, H, s)), H, W) for H, W, s in R.PERSP_CASES] + [
    ("perspective zoom", *B.ZOOM_PERSP), ("perspective whole", *B.WHOLE_PERSP)]


@pytest.mark.parametrize("case", PERSP, ids=[f"{c[0]}-{c[2]}x{c[3]}" for c in PERSP])
def test_warp_bwd_bilinear_fp64_envelope(case):
    """perspective, bilinear: the cases of the forward family, a 2.5 x zoom (an input pixel collects some 25 outputs) and a perspective whose
    horizon crosses the input (the search's `whole` fallback), against float64 autograd of grid_sample on the float64 grid"""
    tag, co, H, W = case
    if tag.endswith("whole"):
        assert 0 < B.warp_adjoint32(torch.zeros(1, H, W), 1, co, H, W, 1)[1] < H * W          # the fallback runs, on part of the frame
    lines = []
    for kind, dy4 in B.hard_dy((2, 3, H, W)).items():
        dy = dy4.reshape(6, H, W)
        r64, r32 = B.adjoint_pair(lambda t, dt: R.warp_bilinear(t, 1, co, H, W, dt), torch.zeros(6, H, W), dy)
        lines.append((kind, E.frame_err(_warp_bwd(dy, H, W, 1, co, 1), r64), E.frame_err(r32, r64)))
    B.envelope(f"aug_warp_bwd bilinear {tag} {H}x{W}", lines)


def _nearest_cases():
    out = [(f"rotate {a}", H, W, H, W, 0, R.rotate_coeffs(a, H, W)) for H, W in R.ROT_SHAPES for a in R.ROT_ANGLES]
    out += [(f"rotate {a} expand", H, W) + R.rot90_size(H, W) + (0, R.rotate_coeffs(a, H, W)) for H, W in R.ROT90_SHAPES for a in (90, -90)]
    out += [(tag, H, W, H, W, 1, co) for tag, co, H, W in PERSP[-2:]]
    return out


NEAREST = _nearest_cases()


@pytest.mark.parametrize("case", NEAREST, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in NEAREST])
def test_warp_bwd_nearest_is_the_scatter_of_the_forward_choices(case):
    """nearest: no rounding tie is excluded or guessed.  The HIP forward (held to candidate sets by the forward family) warps an index image --
    pixel number + 1 as an exact float, 0 = off the frame -- and dx must be the sum of dy over the output pixels that chose the pixel: float64
    sum = reference, fp32 sum = yardstick.  A contributor missed by the search box is an error of order 1."""
    tag, H, W, oh, ow, kind, co = case
    L = N.lib()
    ii, io = _in(torch.arange(1, H * W + 1, dtype=F32).view(1, H, W)), _out(1, oh, ow)
    N.check(L.vs_aug_warp(N.ptr(ii[1]), N.ptr(io[1]), 1, H, W, oh, ow, kind, (C.c_float * len(co))(*co), 0, N.stream()), "vs_aug_warp")
    index = _done([io], [ii])[0][0] - 1
    assert (index >= 0).any()
    lines = []
    for name, dy4 in B.hard_dy((2, 3, oh, ow)).items():
        dy = dy4.reshape(6, oh, ow)
        r64, r32 = B.scatter_adjoint(dy, index, H, W, F64), B.scatter_adjoint(dy, index, H, W, F32)
        lines.append((name, E.frame_err(_warp_bwd(dy, H, W, kind, co, 0), r64), E.frame_err(r32, r64)))
    B.envelope(f"aug_warp_bwd nearest {tag} {H}x{W}", lines)


# ------------------------------------------------------------------------------------------------------------------------ embed tail
def _tail_bwd(imgs, preds, hm, d_out, d_preds, cfg):
    Fn, Cd, H, W = preds.shape
    ins = [_in(imgs), _in(preds)] + [_in(t) for t in (hm, d_out, d_preds) if t is not None]
    opt = iter(ins[2:])
    p = [N.ptr(next(opt)[1]) if t is not None else None for t in (hm, d_out, d_preds)]
    g = _out(Fn, Cd, H, W)
    N.check(N.lib().vs_embed_tail_bwd(N.ptr(ins[0][1]), N.ptr(ins[1][1]), p[0], p[1], p[2], Fn, H, W, Cd, cfg["clamp"], cfg["si"], cfg["sw"],
                                      N.ptr(g[1]), N.stream()), "vs_embed_tail_bwd")
    return _done([g], ins)[0]


def _key_chain(g_full, hm_low, Fn, Cd, S, cfg):
    """(vs_resize_nchw_bwd where the frame differs from S) -> vs_tail_key_reduce"""
    H, W = g_full.shape[-2:]
    g_low = _resize_bwd(g_full, S, S, cfg["aa"]) if (H, W) != (S, S) else g_full
    gi, hi, dd = _in(g_low), (_in(hm_low) if hm_low is not None else None), _out(cfg["total_key"], Cd, S, S)
    N.check(N.lib().vs_tail_key_reduce(N.ptr(gi[1]), N.ptr(hi[1]) if hi else None, Fn, Cd, S, S, cfg["step"], cfg["mode"], cfg["total_key"], N.ptr(dd[1]),
                                       N.stream()), "vs_tail_key_reduce")
    return _done([dd], [gi] + ([hi] if hi else []))[0]


@pytest.mark.parametrize("case", B.TAIL_BWD_CASES, ids=[c[0] for c in B.TAIL_BWD_CASES])
def test_embed_tail_bwd_fp64_envelope(case):
    """vs_embed_tail_bwd with only d_out, only d_preds and both, on noise, flat, jump and saturated frames (blocks of exactly 0 and 1, a zero key
    frame, sw = 3): an exact bound passes the gradient, a flagged element may match either side of its gate.  Then its output through
    vs_resize_nchw_bwd and vs_tail_key_reduce against the float64 adjoint of expansion x heat-map x resize applied to those very values, and
    vs_tail_key_reduce alone on the five gradient kinds: Cd 1 and 3, the three video modes, F not a multiple of step, total_key clamping"""
    tag, Fn, H, W, S, Cd, low, full, _ = case
    rows = {}
    for kind in B.TAIL_KINDS:
        imgs, delta, hm_low, hm, cfg, preds = B.tail_bwd_inputs(case, kind)
        d_out, d_preds = B.tail_dy(case, kind)
        amb = B.tail_flags(preds, imgs, hm, cfg)
        share = float(amb.float().mean())
        print(f"IMG-BWD-FLAGGED embed_tail_bwd {tag} {kind}: share {share:.5f}")
        assert share <= B.FLAG_SHARE
        ambg = amb if Cd == 3 else amb.any(1, keepdim=True)
        own = B.adjoint(lambda t, dt: B.tail_out(t, imgs, hm, cfg, dt), preds, d_out, F64)
        y32 = B.adjoint(lambda t, dt: B.tail_out(t, imgs, hm, cfg, dt), preds, d_out, F32)
        other = B.tail_point_adjoint(preds, imgs, hm, d_out, None, cfg, F64, flip=amb)
        for combo, do, dp in (("out", d_out, None), ("preds", None, d_preds), ("both", d_out, d_preds)):
            got = _tail_bwd(imgs, preds, hm, do, dp, cfg)
            if do is None:
                _same(got, d_preds, f"{tag} {kind}: only d_preds")
                continue
            add = 0 if dp is None else dp.double()
            rows.setdefault(f"g {combo}", []).append((B.masked_err(got, own + add, other + add, ambg), B.masked_err(y32.double() + add, own + add, other + add, ambg)))
        fn = lambda t, dt: B.tail_linear(t, Fn, H, W, cfg, hm_low, dt)          # noqa: E731
        r64, r32 = B.adjoint_pair(fn, delta, got)
        rows.setdefault("chain", []).append((E.frame_err(_key_chain(got, hm_low, Fn, Cd, S, cfg), r64), E.frame_err(r32, r64)))
    for name, figs in rows.items():
        B.envelope(f"embed_tail_bwd {tag} F={Fn} {H}x{W} Cd={Cd} {name}", [(k, h, y) for k, (h, y) in zip(B.TAIL_KINDS, figs)])
    lines = []
    for kind, g in B.hard_dy((Fn, Cd, S, S)).items():
        r64, r32 = B.adjoint_pair(lambda t, dt: B.tail_linear(t, Fn, S, S, cfg, hm_low, dt), delta, g)
        lines.append((kind, E.frame_err(_key_chain(g, hm_low, Fn, Cd, S, cfg), r64), E.frame_err(r32, r64)))
    B.envelope(f"tail_key_reduce {tag} F={Fn} Cd={Cd}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_aug_color_bwd
def _color_bwd(x, dy, op, f):
    L = N.lib()
    Fn, _, H, W = x.shape
    xi, di, dx = _in(x), _in(dy), _out(Fn, 3, H, W)
    means = None
    if op == R.OP_CONTRAST:          # the per-frame grey means of the forward pass: the last F floats of vs_aug_color's scratch
        fs = torch.empty(int(L.vs_aug_color_scratch_floats(Fn, H, W)), device=DEV)
        fo = torch.empty(Fn, 3, H, W, device=DEV)
        N.check(L.vs_aug_color(N.ptr(xi[1]), N.ptr(fo), Fn, H, W, op, f, N.ptr(fs), N.stream()), "vs_aug_color")
        means = fs[-Fn:].clone()
    scr = torch.empty(int(L.vs_aug_color_bwd_scratch_floats(Fn, H, W)) + 2, device=DEV, dtype=F64).view(F32)
    N.check(L.vs_aug_color_bwd(N.ptr(xi[1]), N.ptr(di[1]), N.ptr(dx[1]), Fn, H, W, op, f, N.ptr(means) if means is not None else None, N.ptr(scr),
                               N.stream()), "vs_aug_color_bwd")
    return _done([dx], [xi, di])[0]


@pytest.mark.parametrize("name,op,f", B.COLOR_BWD_CASES, ids=[f"{n}{f:g}" for n, _, f in B.COLOR_BWD_CASES])
def test_colour_bwd_fp64_envelope(name, op, f):
    """every colour op on hard_pixels, one line per band of rows: random, grey, tied, nearly grey, corner and nearly black / white pixels.  Exact
    gates (black and white channels, dyadic factors) have one answer; flagged elements of brightness / saturation may match either side; flagged
    hue pixels (a sector boundary or a p / q / t gate within its band) are left out, at most 0.5 % of a band; contrast has no flagged element,
    on hard_pixels and on three 300 x 300 frames of different means (the strided pass of its masked sums)"""
    x, changed = B.hue_pixels(f) if op == R.OP_HUE else (R.hard_pixels(), [])
    sets = [("pixels", x, B.pixel_bands(x.shape[-2]))]
    if op == R.OP_CONTRAST:
        sets.append(("frames300", B.contrast_frames(), None))
    for sname, xs, bands in sets:
        for kind, dy in B.hard_dy(tuple(xs.shape)).items():
            own, other, amb, keep, y32 = B.color_ref(xs, dy, op, f)
            flagged = amb if amb is not None else (~keep if keep is not None else None)
            got = _color_bwd(xs, dy, op, f)
            if bands is None:          # one line per frame
                hip = [(f"frame {i}", B.masked_err(got[i], own[i])) for i in range(xs.shape[0])]
                yard = [(f"frame {i}", B.masked_err(y32[i], own[i])) for i in range(xs.shape[0])]
                assert not flagged.any()
            else:
                hip, yard = B.band_lines(got, own, bands, other, amb, keep), B.band_lines(y32, own, bands, other, amb, keep)
                for band, rows in bands if flagged is not None else ():
                    share = float(flagged[:, :, rows].float().mean())
                    assert share <= (0.0 if op == R.OP_CONTRAST else B.FLAG_SHARE), (band, share)
                    if share:
                        print(f"IMG-BWD-FLAGGED aug_color_bwd {name} {f:g} {kind} {band}: share {share:.5f}")
            B.envelope(f"aug_color_bwd {name} factor {f:g} {sname} dy={kind}",
                       [(b + ("*" if b in changed else ""), h, y) for (b, h), (_, y) in zip(hip, yard)])


# ------------------------------------------------------------------------------------------------------------------------ vs_percep_mse
@pytest.mark.parametrize("yuv", [0, 1], ids=["mse", "yuv"])
@pytest.mark.parametrize("Fn,H,W", B.PERCEP_SHAPES)
def test_percep_mse_fp64_envelope(Fn, H, W, yuv):
    """loss and gradient; 3 x 300 x 300 pixels exceed the 1024 blocks of the partial sums (their second grid-stride pass); differences of order
    1e-7 on a 0.9 background; an identical pair gives loss and gradient exactly 0"""
    L = N.lib()
    lines = []
    for kind in ("noise", "tiny", "same"):
        a, b = B.percep_inputs(Fn, H, W, kind)
        ai, bi, d = _in(a), _in(b), _out(Fn, 3, H, W)
        part = torch.full((int(L.vs_percep_partial_doubles(Fn, H, W)),), NAN, dtype=F64, device=DEV)
        loss = _out(1)
        N.check(L.vs_percep_mse(N.ptr(ai[1]), N.ptr(bi[1]), Fn, H, W, yuv, N.ptr(part), N.ptr(loss[1]), N.stream()), "vs_percep_mse")
        N.check(L.vs_percep_mse_grad(N.ptr(ai[1]), N.ptr(bi[1]), Fn, H, W, yuv, 1.0, N.ptr(d[1]), N.stream()), "vs_percep_mse_grad")
        gl, gd = _done([loss, d], [ai, bi])
        if kind == "same":
            assert float(gl) == 0.0 and not gd.any()
            continue
        l64, l32 = B.percep(a, b, yuv, F64), B.percep(a, b, yuv, F32)
        r64, r32 = B.adjoint_pair(lambda t, dt: B.percep(a, t, yuv, dt), b, torch.ones(()))
        lines.append((f"{kind} loss", E.frame_err(gl.view(()), l64), E.frame_err(l32, l64)))
        lines.append((f"{kind} grad", E.frame_err(gd, r64), E.frame_err(r32, r64)))
    B.envelope(f"percep_mse {'yuv' if yuv else 'mse'} {Fn}x3x{H}x{W}", lines)


# ------------------------------------------------------------------------------------------------------------------------ temporal ops
@pytest.mark.parametrize("hw,alpha", [(1, 0.6), (3, 1.0)])
def test_window_average_bwd_fp64_envelope(hw, alpha):
    """F = 5, half windows 1 and 3 (wider than the clip: every window is clipped on both sides)"""
    lines = []
    for kind, dy in B.hard_dy((5, 3, 33, 47)).items():
        r64, r32 = B.adjoint_pair(lambda t, dt: R.window_average(t, hw, alpha), torch.zeros(5, 3, 33, 47), dy)
        di, dx = _in(dy), _out(5, 3, 33, 47)
        N.check(N.lib().vs_aug_window_average_bwd(N.ptr(di[1]), N.ptr(dx[1]), 5, 3 * 33 * 47, hw, alpha, N.stream()), "vs_aug_window_average_bwd")
        lines.append((kind, E.frame_err(_done([dx], [di])[0], r64), E.frame_err(r32, r64)))
    B.envelope(f"window_average_bwd F=5 half window {hw} alpha {alpha}", lines)


def test_gather_frames_bwd_sums_repeated_sources_and_zeroes_unused_ones():
    """source 2 copied three times, sources 1 and 4 never: their dx is written as zeros over the sentinel"""
    idx = [2, 2, 0, 2, 3]
    lists = [[o for o, f in enumerate(idx) if f == s] for s in range(5)]
    start = torch.tensor([0] + [sum(len(l) for l in lists[:s + 1]) for s in range(5)], dtype=torch.int32, device=DEV)
    outs = torch.tensor([o for l in lists for o in l], dtype=torch.int32, device=DEV)
    lines = []
    for kind, dy in B.hard_dy((5, 3, 33, 47)).items():
        r64, r32 = B.adjoint_pair(lambda t, dt: t[idx], torch.zeros(5, 3, 33, 47), dy)
        di, dx = _in(dy), _out(5, 3, 33, 47)
        N.check(N.lib().vs_aug_gather_frames_bwd(N.ptr(di[1]), N.ptr(start), N.ptr(outs), N.ptr(dx[1]), 5, 3 * 33 * 47, N.stream()), "vs_aug_gather_frames_bwd")
        got = _done([dx], [di])[0]
        assert not got[1].any() and not got[4].any()
        lines.append((kind, E.frame_err(got, r64), E.frame_err(r32, r64)))
    B.envelope("gather_frames_bwd 5 <- [2, 2, 0, 2, 3]", lines)


# ------------------------------------------------------------------------------------------------------------------------ exact operations
@pytest.mark.parametrize("H,W", R.POINT_PLANES)
def test_exact_adjoints_equal_their_definition_bit_for_bit(H, W):
    """vs_mask_mul, vs_aug_crop_flip_bwd, vs_clamp01_bwd, vs_nhwc_to_nchw_scaled on a plane of 11 pixels, 93 x 118 and 1025 x 1024 (the grid-stride
    loop's second pass); the clamp's gate on exact bounds, their neighbours and values outside"""
    L = N.lib()
    g = torch.Generator().manual_seed(3 * H + W)
    Fn, Cc = (1, 1) if H * W > 1 << 20 else (2, 3)
    dy, m = torch.randn(Fn, Cc, H, W, generator=g), torch.rand(Fn, 1, H, W, generator=g)
    di, mi = _in(dy), _in(m)
    for comp, want in ((0, dy * m), (1, dy * (1 - m))):
        dx = _out(Fn, Cc, H, W)
        N.check(L.vs_mask_mul(N.ptr(di[1]), N.ptr(mi[1]), N.ptr(dx[1]), Fn, Cc, H, W, comp, N.stream()), "vs_mask_mul")
        _same(_done([dx], [di, mi])[0], want, f"vs_mask_mul complement {comp}")
    one = torch.ones(())
    vals = torch.tensor([0.0, 1.0, -0.0, float(torch.nextafter(one, 2 * one)), float(torch.nextafter(one, 0 * one)), -1e-45, 1e-45, -0.5, 1.5, 0.5])
    x = torch.rand(Fn, Cc, H, W, generator=g) * 1.5 - 0.25
    x.view(-1)[torch.randperm(x.numel(), generator=g)[: x.numel() // 2]] = vals[torch.randint(0, 10, (x.numel() // 2,), generator=g)]
    xi, dx = _in(x), _out(Fn, Cc, H, W)
    N.check(L.vs_clamp01_bwd(N.ptr(xi[1]), N.ptr(di[1]), N.ptr(dx[1]), x.numel(), N.stream()), "vs_clamp01_bwd")
    _same(_done([dx], [xi, di])[0], torch.where((x >= 0) & (x <= 1), dy, torch.zeros(())), "vs_clamp01_bwd")
    src = torch.randn(Fn, H, W, 4, generator=g)
    si = _in(src)
    for mul in (2.0, -0.3):
        dst = _out(Fn, 3, H, W)
        N.check(L.vs_nhwc_to_nchw_scaled(N.ptr(si[1]), Fn, H, W, 3, 4, mul, N.ptr(dst[1]), N.stream()), "vs_nhwc_to_nchw_scaled")
        _same(_done([dst], [si])[0], (src[..., :3] * torch.tensor(mul, dtype=F32)).permute(0, 3, 1, 2), f"vs_nhwc_to_nchw_scaled {mul}")
    P = Fn * Cc
    for i0, j0, h, w in ((-2, -3, H + 3, W + 5), (H // 2, W // 3, H, W), (0, 1, max(H - 1, 1), max(W - 2, 1))):
        for flip in (0, 1):
            dyc = torch.randn(P, h, w, generator=g)
            want = B.adjoint(lambda t, dt: R.crop_flip(t, i0, j0, h, w, flip), torch.zeros(P, H, W), dyc, F32)
            ci, dx = _in(dyc), _out(P, H, W)
            N.check(L.vs_aug_crop_flip_bwd(N.ptr(ci[1]), N.ptr(dx[1]), P, H, W, i0, j0, h, w, flip, N.stream()), "vs_aug_crop_flip_bwd")
            _same(_done([dx], [ci])[0], want, f"vs_aug_crop_flip_bwd {(i0, j0, h, w, flip)}")
