"""fp64 envelopes of the loss and discriminator kernels (csrc/ssim.hip, vs_percep_mse*, vs_bce_logits, vs_pixel_bce, csrc/disc.hip) on hard frame
pairs, logits and activations (tests/_loss_ref.py: formulas, cases, metric; tests/test_loss_contract_cpu.py: the metric bites).  Every kernel is
called through the C ABI: per (case, kind, quantity) the error against the float64 formula (float64 autograd for the gradients), at most
LOSS_FP64_MARGIN times what the same formula costs in float32 on the CPU.  Inputs sit between NaN bands (int32 messages between poisoned words),
outputs are pre-filled with a sentinel between -7.0 bands, every workspace has exactly the size its contract function returns, between bands: the
bands must be intact and no sentinel may be left.  Every figure is printed as a LOSS-ENVELOPE line; profiles/loss_fp64_envelope.txt is such a
run on an MI355X."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import _envelope as E  # noqa: E402
from tests import _img_bwd_ref as B  # noqa: E402
from tests import _img_ref as R  # noqa: E402
from tests import _loss_ref as Q  # noqa: E402
from tests._guards import _guarded, _guards_intact, scratch  # noqa: E402
from videoseal_amd import autograd as AG  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = 2.0 ** 120              # pre-fill of every output: no kernel under test produces it (a small dyadic value can be the sum of a checkerboard)
F32, F64 = torch.float32, torch.float64
WIN = (C.c_float * 11)(*Q.win11(F32).tolist())


def _in(t):
    return _guarded(t.to(DEV).contiguous(), NAN if t.dtype.is_floating_point else 255)


def _out(*shape, dtype=F32):
    return _guarded(torch.full(shape, SENT, dtype=dtype, device=DEV), -7.0)


def _ws(nelem, dtype=F64):
    """a workspace of exactly the contract's size, NaN-filled, between bands"""
    return scratch(int(nelem), dtype, NAN, DEV)


def _done(outs, ins=(), wss=()):
    """after the launch: every band intact, every output element written; returns the outputs on the CPU"""
    torch.cuda.synchronize()
    for buf, view in ins:
        assert _guards_intact(buf, NAN if buf.dtype.is_floating_point else 255), "a band around an input changed"
    for buf, view in wss:
        assert _guards_intact(buf, -7.0), "a kernel wrote outside its workspace"
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


def test_the_window_is_the_one_the_engine_passes():
    assert list(WIN) == list(AG._win11())


# ------------------------------------------------------------------------------------------------------------------------ vs_ssim_stats / vs_ssim_grad
def _ssim_stats(x, y):
    L = N.lib()
    P, (H, W) = x.shape[0] * x.shape[1], x.shape[-2:]
    xi, yi, out, ws = _in(x), _in(y), _out(2, P, dtype=F64), _ws(L.vs_ssim_partial_doubles(P, H, W))
    N.check(L.vs_ssim_stats(N.ptr(xi[1]), N.ptr(yi[1]), P, H, W, 1.0, WIN, N.ptr(ws[1]), N.ptr(out[1]), N.stream()), "vs_ssim_stats")
    o = _done([out], [xi, yi], [ws])[0]
    return o[0].view(x.shape[:2]), o[1].view(x.shape[:2])


def _ssim_grad(x, y, gs, gc, gco):
    P, (H, W) = x.shape[0] * x.shape[1], x.shape[-2:]
    ins = [_in(t) for t in (x, y, gs, gc)] + ([_in(gco)] if gco is not None else [])
    d = _out(*x.shape)
    N.check(N.lib().vs_ssim_grad(*[N.ptr(i[1]) for i in ins[:4]], N.ptr(ins[4][1]) if gco is not None else None, P, H, W, 1.0, WIN, N.ptr(d[1]),
                                 N.stream()), "vs_ssim_grad")
    return _done([d], ins)[0]


def _ssim_case(Fn, H, W):
    gs, gc, gco = Q.ssim_coeffs(H, W, 3 * Fn)
    lines, scale = [], None
    for kind, (x, y) in Q.hard_pairs(H, W, Fn).items():
        (s64, c64), (s32, c32) = Q.ssim_stats(x, y, F64), E.one_thread(lambda: Q.ssim_stats(x, y, F32))
        s, c = _ssim_stats(x, y)
        lines.append(Q.line(f"{kind} ssim", s, s64, s32, scalar=True))
        lines.append(Q.line(f"{kind} cs", c, c64, c32, scalar=True))
        for tag, co in (("grad", None), ("grad+coarse", gco)):
            g64, g32 = (Q.grad_of(lambda t: Q.ssim_target(x, t, gs, gc, co, dt), y, dt) for dt in (F64, F32))
            scale = scale or float(g64.abs().max())
            lines.append(Q.line(f"{kind} {tag}", _ssim_grad(x, y, gs, gc, co), g64, g32, scale, zero=kind == "identical" and co is None))
    Q.envelope(f"ssim {Fn}x3x{H}x{W}", lines)


@pytest.mark.parametrize("H,W", Q.SSIM_SHAPES, ids=lambda v: str(v))
def test_ssim_stats_and_grad_fp64_envelope(H, W):
    """per plane the means of the SSIM and contrast-structure maps, and d / dy of their random combination without and with the pooled gradient of
    a coarser level, on every pair kind: against the reference's own unshifted formula in float64, the same in float32 as the yardstick.  The
    gradient of the identical pair is zero in exact arithmetic: absolute errors on the `noise` kind's scale"""
    _ssim_case(2, H, W)


def test_ssim_stats_and_grad_fp64_envelope_at_the_full_row_counts():
    """513 narrow planes: enough workgroups that pick_rows keeps STATS_ROWS = 96 and GRAD_ROWS = 128 (the chunks of full-size frames: a workgroup's
    shift is taken over 106 and 148 rows, a black bar and the picture in one chunk)"""
    _ssim_case(*Q.SSIM_MANY_PLANES)


@pytest.mark.parametrize("H,W", Q.SSIM_SHAPES, ids=lambda v: str(v))
def test_avgpool2_pad_fp64_envelope(H, W):
    """every shape has an odd side: the padded zeros are counted"""
    lines = []
    for kind, (x, y) in Q.hard_pairs(H, W).items():
        xi, yi = _in(x), _in(y)
        xo, yo = _out(2, 3, (H + 1) // 2, (W + 1) // 2), _out(2, 3, (H + 1) // 2, (W + 1) // 2)
        N.check(N.lib().vs_avgpool2_pad(N.ptr(xi[1]), N.ptr(yi[1]), 6, H, W, N.ptr(xo[1]), N.ptr(yo[1]), N.stream()), "vs_avgpool2_pad")
        gx, gy = _done([xo, yo], [xi, yi])
        lines.append(Q.line(f"{kind} x", gx, Q.pool2(x.double()), Q.pool2(x), 1.0))
        lines.append(Q.line(f"{kind} y", gy, Q.pool2(y.double()), Q.pool2(y), 1.0))
    Q.envelope(f"avgpool2_pad 2x3x{H}x{W}", lines)


@pytest.mark.parametrize("H,W", Q.MS_SHAPES, ids=lambda v: str(v))
def test_msssim_and_ssim_loss_chain_fp64_envelope(H, W):
    """autograd.msssim_loss (five levels of vs_ssim_stats / vs_avgpool2_pad, vs_ssim_grad from the coarsest level up) and ssim_loss: loss and
    gradient against the float64 formula.  On `inverse` the relu gate closes: loss and gradient are exactly 0"""
    lines, scale = [], {}
    for kind in Q.MS_KINDS:
        x, y = (t[:1] for t in Q.hard_pairs(H, W)[kind])
        for name, hip, ref in (("msssim", AG.msssim_loss, Q.msssim_loss), ("ssim", AG.ssim_loss, Q.ssim_loss)):
            yg = y.to(DEV).requires_grad_(True)
            loss = hip(x.to(DEV), yg)
            loss.backward()
            l64, l32 = ref(x, y, F64), E.one_thread(lambda: ref(x, y, F32))
            g64, g32 = (Q.grad_of(lambda t: ref(x, t, dt), y, dt) for dt in (F64, F32))
            scale.setdefault(name, float(g64.abs().max()))
            lines.append(Q.line(f"{kind} {name} loss", loss, l64, l32, 1.0, scalar=True))
            lines.append(Q.line(f"{kind} {name} grad", yg.grad, g64, g32, scale[name]))
    Q.envelope(f"loss chain 1x3x{H}x{W}", lines)


# ------------------------------------------------------------------------------------------------------------------------ mse / yuv / jnd
@pytest.mark.parametrize("Fn,H,W", Q.PERCEP_SHAPES)
def test_percep_mse_and_jnd_loss_fp64_envelope(Fn, H, W):
    """vs_percep_mse / _grad (mse and yuv) and vs_jnd_loss / vs_jnd_loss_grad with the heat-map of the float64 _img_ref formula, fed to both sides as
    fp32; the identical pair: mse and its gradient exactly 0, the JND gradient exactly 0 (sign(0) = 0)"""
    L = N.lib()
    lines, scale = [], {}
    for kind, (x, y) in Q.hard_pairs(H, W, Fn).items():
        xi, yi = _in(x), _in(y)
        for yuv in (0, 1):
            nm = "yuv" if yuv else "mse"
            ws, loss, d = _ws(L.vs_percep_partial_doubles(Fn, H, W)), _out(1), _out(Fn, 3, H, W)
            N.check(L.vs_percep_mse(N.ptr(xi[1]), N.ptr(yi[1]), Fn, H, W, yuv, N.ptr(ws[1]), N.ptr(loss[1]), N.stream()), "vs_percep_mse")
            N.check(L.vs_percep_mse_grad(N.ptr(xi[1]), N.ptr(yi[1]), Fn, H, W, yuv, 1.0, N.ptr(d[1]), N.stream()), "vs_percep_mse_grad")
            gl, gd = _done([loss, d], [xi, yi], [ws])
            g64, g32 = (Q.grad_of(lambda t: Q.percep(x, t, yuv, dt), y, dt) for dt in (F64, F32))
            scale.setdefault(nm, float(g64.abs().max()))
            lines.append(Q.line(f"{kind} {nm} loss", gl.view(()), Q.percep(x, y, yuv, F64), Q.percep(x, y, yuv, F32), 1.0, scalar=True))
            lines.append(Q.line(f"{kind} {nm} grad", gd, g64, g32, scale[nm]))
        hm = R.jnd(x, F64)[0].to(F32)
        hi, ws, loss, d = _in(hm), _ws(L.vs_jnd_loss_partial_doubles(Fn, H, W)), _out(1), _out(Fn, 3, H, W)
        N.check(L.vs_jnd_loss(N.ptr(xi[1]), N.ptr(yi[1]), N.ptr(hi[1]), Fn, H, W, N.ptr(ws[1]), N.ptr(loss[1]), N.stream()), "vs_jnd_loss")
        N.check(L.vs_jnd_loss_grad(N.ptr(xi[1]), N.ptr(yi[1]), N.ptr(hi[1]), Fn, H, W, 1.0, N.ptr(d[1]), N.stream()), "vs_jnd_loss_grad")
        gl, gd = _done([loss, d], [xi, yi, hi], [ws])
        g64, g32 = (Q.grad_of(lambda t: Q.jnd_loss(x, t, hm, dt), y, dt) for dt in (F64, F32))
        scale.setdefault("jnd", float(g64.abs().max()))
        lines.append(Q.line(f"{kind} jnd loss", gl.view(()), Q.jnd_loss(x, y, hm, F64), Q.jnd_loss(x, y, hm, F32), 1.0, scalar=True))
        lines.append(Q.line(f"{kind} jnd grad", gd, g64, g32, scale["jnd"]))
        if kind == "identical":
            assert not gd.any()
    Q.envelope(f"percep / jnd {Fn}x3x{H}x{W}", lines)


# ------------------------------------------------------------------------------------------------------------------------ decoding losses
@pytest.mark.parametrize("Bn,k", Q.BCE_SHAPES)
def test_bce_logits_fp64_envelope(Bn, k):
    """loss and gradient at temperatures 0.1, 1 and 10, one message row and one per frame; logits on the hinge kink, far in both tails (exp
    overflows, sigmoid saturates) and one-sided; column 0 of the gradient is exactly 0"""
    L = N.lib()
    for T in Q.BCE_TEMPS:
        for rows in sorted({1, Bn}):
            msgs = Q.hard_msgs(rows, k)
            lines, scale = [], None
            for kind, p in Q.hard_logits((Bn, k + 1)).items():
                pi, mi, d, loss = _in(p), _in(msgs), _out(Bn, k + 1), _out(1)
                N.check(L.vs_bce_logits(N.ptr(pi[1]), N.ptr(mi[1]), rows, Bn, k, T, 0.5, N.ptr(d[1]), N.ptr(loss[1]), N.stream()), "vs_bce_logits")
                gd, gl = _done([d, loss], [pi, mi])
                assert not gd[:, 0].any()
                g64, g32 = (0.5 * Q.grad_of(lambda t: Q.bce_logits(t, msgs, T, dt), p, dt) for dt in (F64, F32))
                scale = scale or float(g64.abs().max())
                lines.append(Q.line(f"{kind} loss", gl.view(()), Q.bce_logits(p, msgs, T, F64), Q.bce_logits(p, msgs, T, F32), 1.0, scalar=True))
                lines.append(Q.line(f"{kind} grad", gd, g64, g32, scale))
            Q.envelope(f"bce_logits B={Bn} k={k} T={T:g} msg_rows={rows}", lines)


@pytest.mark.parametrize("Bn,K,HW", Q.PIXEL_BCE_SHAPES)
def test_pixel_bce_fp64_envelope(Bn, K, HW):
    """detection and masked decoding loss and w_det d det + w_dec d dec; frame 0's mask selects a single pixel, frame 1's everything"""
    L = N.lib()
    masks = Q.pixel_masks(Bn, HW)
    w_det, w_dec = 0.5, 2.0
    for T in Q.BCE_TEMPS:
        for rows in (1, Bn):
            msgs = Q.hard_msgs(rows, K - 1)
            lines, scale = [], None
            for kind, p in Q.hard_logits((Bn, K, HW)).items():
                pi, ki, mi, d, loss, ws = _in(p), _in(masks), _in(msgs), _out(Bn, K, HW), _out(2), _ws(L.vs_pixel_bce_partial_doubles(Bn, K, HW))
                N.check(L.vs_pixel_bce(N.ptr(pi[1]), N.ptr(ki[1]), N.ptr(mi[1]), rows, Bn, K, HW, T, w_det, w_dec, N.ptr(d[1]), N.ptr(ws[1]),
                                       N.ptr(loss[1]), N.stream()), "vs_pixel_bce")
                gd, gl = _done([d, loss], [pi, ki, mi], [ws])

                def tot(t, dt):
                    det, dec = Q.pixel_bce(t, masks, msgs, T, dt)
                    return w_det * det + w_dec * dec
                g64, g32 = (Q.grad_of(lambda t: tot(t, dt), p, dt) for dt in (F64, F32))
                scale = scale or float(g64.abs().max())
                l64, l32 = Q.pixel_bce(p, masks, msgs, T, F64), Q.pixel_bce(p, masks, msgs, T, F32)
                lines.append(Q.line(f"{kind} detect", gl[0], l64[0], l32[0], 1.0, scalar=True))
                lines.append(Q.line(f"{kind} decode", gl[1], l64[1], l32[1], 1.0, scalar=True))
                lines.append(Q.line(f"{kind} grad", gd, g64, g32, scale))
            Q.envelope(f"pixel_bce B={Bn} K={K} HW={HW} T={T:g} msg_rows={rows}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_disc_loss
def _disc_loss(real, fake, hinge, gscale, grads):
    ins = ([_in(real)] if real is not None else []) + [_in(fake)]
    dr = _out(*real.shape) if grads and real is not None else None
    df = _out(*fake.shape) if grads else None
    out = _out(4)
    N.check(N.lib().vs_disc_loss(N.ptr(ins[0][1]) if real is not None else None, real.numel() if real is not None else 0, N.ptr(ins[-1][1]), fake.numel(),
                                 hinge, gscale, N.ptr(dr[1]) if dr else None, N.ptr(df[1]) if df else None, N.ptr(out[1]), N.stream()), "vs_disc_loss")
    return _done([o for o in (out, dr, df) if o is not None], ins)


@pytest.mark.parametrize("shape", [(3, 1, 7, 9), (5, 1, 9, 11)], ids=lambda v: "x".join(map(str, v)))
def test_disc_loss_fp64_envelope(shape):
    """the hinge loss and -mean(fake), their gradients (times gscale) and the two logit means; 189 logits (fewer than the 256 threads) and 495;
    with and without the gradient outputs; the generator's form with and without `real`.  A gradient at the exact kink is exactly 0"""
    gscale = 0.25
    lines, scale = [], {}
    for kind, t in Q.hard_logits(shape).items():
        real, fake = t, -t.flip(0)
        # hinge
        out, dr, df = _disc_loss(real, fake, 1, gscale, True)
        _same(_disc_loss(real, fake, 1, gscale, False)[0], out, f"{kind}: out without gradient outputs")
        l64, l32 = Q.disc_loss(real, fake, 1, F64), Q.disc_loss(real, fake, 1, F32)
        assert out[3] == 0
        mag = float(t.double().abs().mean())          # the logit means can cancel (`large` sums to 0): absolute errors over mean |logit|
        lines.append(Q.line(f"{kind} hinge loss", out[0], l64[0], l32[0], 1.0, scalar=True))
        for i, nm in ((1, "mean real"), (2, "mean fake")):
            lines.append(Q.line(f"{kind} hinge {nm}", out[i], l64[i], l32[i], mag=mag))
        for nm, got, wrt in (("dreal", dr, 0), ("dfake", df, 1)):
            g64, g32 = (gscale * Q.grads_of(lambda r, f: Q.disc_loss(r, f, 1, dt)[0], (real, fake), dt)[wrt] for dt in (F64, F32))
            scale.setdefault(nm, float(g64.abs().max()))
            lines.append(Q.line(f"{kind} hinge {nm}", got, g64, g32, scale[nm]))
        assert not dr[real == 1].any() and not df[fake == -1].any(), "a gradient at the exact kink"
        if kind == "one-sided":
            assert out[0] == 0 and not dr.any() and not df.any()
        # the generator's term: n_real = 0 and real = NULL, then with real (only its mean is used)
        for r in (None, real):
            out, *rest = _disc_loss(r, fake, 0, gscale, True)
            l64, l32 = Q.disc_loss(r, fake, 0, F64), Q.disc_loss(r, fake, 0, F32)
            g64, g32 = (gscale * Q.grad_of(lambda f: Q.disc_loss(None, f, 0, dt)[0], fake, dt) for dt in (F64, F32))
            tag = "gen" if r is None else "gen+real"
            lines.append(Q.line(f"{kind} {tag} loss", out[0], l64[0], l32[0], mag=mag))
            lines.append(Q.line(f"{kind} {tag} mean fake", out[2], l64[2], l32[2], mag=mag))
            lines.append(Q.line(f"{kind} {tag} dfake", rest[-1], g64, g32, 1.0))
            if r is None:
                assert out[1] == 0 and out[3] == 0
            else:
                lines.append(Q.line(f"{kind} {tag} mean real", out[1], l64[1], l32[1], mag=mag))
    Q.envelope(f"disc_loss {'x'.join(map(str, shape))}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_groupnorm_lrelu
@pytest.mark.parametrize("Cc,Bn,H,W", Q.GN_CASES)
def test_groupnorm_lrelu_fp64_envelope(Cc, Bn, H, W):
    """out, mean, rstd, dx, dgamma, dbeta with ld = C + 4 on noise and on groups of mean 30 / std 0.5, a constant group, one with a 4e3 outlier
    and one of magnitude 1e-3; noise and checkerboard upstream gradients; the pad columns of out and dx are zero"""
    L = N.lib()
    ld, HW = Cc + 4, H * W
    gamma, beta = Q.gn_params(Cc)
    for kind, x in Q.hard_acts(Bn, Cc, H, W, 4).items():
        lines = []
        xi, gi, bi = _in(Q.nhwc(x, ld)), _in(gamma), _in(beta)
        ws, mean, rstd, out = _ws(L.vs_groupnorm_partial_doubles(Bn, HW, Cc)), _out(Bn, 4, dtype=F64), _out(Bn, 4, dtype=F64), _out(Bn, H, W, ld)
        N.check(L.vs_groupnorm_lrelu(N.ptr(xi[1]), ld, Bn, HW, Cc, 4, N.ptr(gi[1]), N.ptr(bi[1]), Q.GN_EPS, Q.SLOPE, N.ptr(ws[1]), N.ptr(mean[1]),
                                     N.ptr(rstd[1]), N.ptr(out[1]), ld, N.stream()), "vs_groupnorm_lrelu")
        gm, gr, go = _done([mean, rstd, out], [xi, gi, bi], [ws])
        assert not go[..., Cc:].any(), "pad columns of out"
        (m64, r64), (m32, r32) = Q.gn_stats(x, F64), Q.gn_stats(x, F32)
        o64, o32 = Q.gn_lrelu(x, gamma, beta, 4, F64), E.one_thread(lambda: Q.gn_lrelu(x, gamma, beta, 4, F32))
        lines += [Q.line("mean", gm, m64, m32, scalar=True), Q.line("rstd", gr, r64, r32, scalar=True),
                  Q.line("out", go[..., :Cc].permute(0, 3, 1, 2), o64, o32)]
        for dk in ("noise", "checker"):
            dy = B.hard_dy((Bn, Cc, H, W))[dk]
            di, ws = _in(Q.nhwc(dy, ld)), _ws(L.vs_groupnorm_partial_doubles(Bn, HW, Cc))
            dx, dg, db = _out(Bn, H, W, ld), _out(Cc), _out(Cc)
            N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(di[1]), ld, N.ptr(xi[1]), ld, Bn, HW, Cc, 4, N.ptr(gi[1]), N.ptr(bi[1]), N.ptr(mean[1]), N.ptr(rstd[1]),
                                             Q.SLOPE, N.ptr(ws[1]), N.ptr(dx[1]), ld, N.ptr(dg[1]), N.ptr(db[1]), N.stream()), "vs_groupnorm_lrelu_bwd")
            gx, gg, gb = _done([dx, dg, db], [di, xi, gi, bi], [ws])
            assert not gx[..., Cc:].any(), "pad columns of dx"
            r64s, r32s = (Q.grads_of(lambda a, b, c: Q.gn_lrelu(a, b, c, 4, dt), (x, gamma, beta), dt, dy) for dt in (F64, F32))
            for nm, got, a, b in zip(("dx", "dgamma", "dbeta"), (gx[..., :Cc].permute(0, 3, 1, 2), gg, gb), r64s, r32s):
                lines.append(Q.line(f"dy={dk} {nm}", got, a, b, 1.0))
        Q.envelope(f"groupnorm_lrelu C={Cc} {Bn}x{H}x{W} {kind}", lines)


def test_plain_leaky_relu_is_bit_equal_on_exact_zeros():
    """groups = 0 on noise and on 0.0, -0.0 and +- the smallest subnormal: out = leaky_relu(x), dx = dy * (x > 0 ? 1 : slope), bit for bit"""
    L = N.lib()
    Bn, Cc, H, W = 2, 16, 5, 7
    ld = Cc + 4
    dy = B.hard_dy((Bn, Cc, H, W))["noise"]
    for kind, x in Q.hard_acts(Bn, Cc, H, W, 0).items():
        xi, di, out, dx = _in(Q.nhwc(x, ld)), _in(Q.nhwc(dy, ld)), _out(Bn, H, W, ld), _out(Bn, H, W, ld)
        N.check(L.vs_groupnorm_lrelu(N.ptr(xi[1]), ld, Bn, H * W, Cc, 0, None, None, Q.GN_EPS, Q.SLOPE, None, None, None, N.ptr(out[1]), ld, N.stream()),
                "vs_groupnorm_lrelu")
        N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(di[1]), ld, N.ptr(xi[1]), ld, Bn, H * W, Cc, 0, None, None, None, None, Q.SLOPE, None, N.ptr(dx[1]), ld,
                                         None, None, N.stream()), "vs_groupnorm_lrelu_bwd")
        go, gx = _done([out, dx], [xi, di])
        assert not go[..., Cc:].any() and not gx[..., Cc:].any()
        _same(go[..., :Cc].permute(0, 3, 1, 2), F.leaky_relu(x, Q.SLOPE), f"leaky_relu {kind}")
        _same(gx[..., :Cc].permute(0, 3, 1, 2), dy * torch.where(x > 0, 1.0, Q.SLOPE), f"leaky_relu backward {kind}")


# ------------------------------------------------------------------------------------------------------------------------ 4 x 4 convolutions
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ld,ci,n", Q.WGRAD_PAIRS)
def test_conv4x4_wgrad_fp64_envelope(ld, ci, n, stride):
    """every (row stride, channels, outputs) of the three configurations at both strides, on 3 x 23 x 19 and on a 2 x 4 x 5 map (fewer output
    pixels than one 16-pixel step): noise activations against every upstream kind, mean-30 group activations against noise, checkerboard and
    ramp; two runs are bit-identical; the gradients of the image's pad channels are zero"""
    L = N.lib()
    assert L.vs_conv4x4_wgrad_supported(n, ld, stride)
    for Bn, H, W in Q.WGRAD_MAPS:
        Ho, Wo = Q.conv_out(H, W, stride)
        dys = B.hard_dy((Bn, n, Ho, Wo))
        lines = []
        for xk, x in Q.hard_acts(Bn, ci, H, W, 4).items():
            xi = _in(Q.nhwc(x, ld))
            for dk in B.DY_KINDS if xk == "noise" else ("noise", "checker", "ramp"):
                dy = dys[dk]
                dyl = 1 if n == 1 else n + 4
                di = _in(dy.permute(0, 2, 3, 1).contiguous() if n == 1 else Q.nhwc(dy, dyl))
                runs = []
                for _ in range(2):
                    ws, dw = _ws(L.vs_conv4x4_wgrad_partial_floats(n, ld, Bn, H, W, stride), F32), _out(n, 16 * ld)
                    N.check(L.vs_conv4x4_wgrad(N.ptr(di[1]), dyl, n, N.ptr(xi[1]), ld, Bn, H, W, stride, N.ptr(ws[1]), N.ptr(dw[1]), N.stream()),
                            "vs_conv4x4_wgrad")
                    runs.append(_done([dw], [di, xi], [ws])[0])
                _same(runs[1], runs[0], "second run")
                got = runs[0].view(n, 4, 4, ld)
                assert not got[..., ci:].any(), "gradients of the pad channels"
                g64, g32 = Q.conv_wgrad(x, dy, n, stride, F64), Q.conv_wgrad(x, dy, n, stride, F32)
                lines.append(Q.line(f"{dk}/{xk}", got[..., :ci].permute(0, 3, 1, 2), g64, g32, 1.0))
        Q.envelope(f"conv4x4_wgrad ld={ld} ci={ci} n={n} s={stride} {Bn}x{H}x{W}", lines)


@pytest.mark.parametrize("ld", Q.N1_LDS)
def test_conv4x4_n1_forward_and_backward_fp64_envelope(ld):
    """the last layer (ld channels -> 1 logit, stride 1) with and without its bias, and its backward-data on every upstream kind; 2 x 6 x 7 and a
    1 x 2 x 2 map whose single 4 x 4 window hangs over every edge"""
    L = N.lib()
    w, bias = Q.conv_weights(1, ld), torch.tensor([0.3])
    wi, bi = _in(Q.taps_first(w, ld)), _in(bias)
    for Bn, H, W in Q.N1_MAPS:
        lines = []
        for xk, x in Q.hard_acts(Bn, ld, H, W, 4).items():
            xi = _in(Q.nhwc(x, ld))
            for tag, b in (("bias", bias), ("no bias", None)):
                out = _out(Bn, H - 1, W - 1)
                N.check(L.vs_conv4x4_n1(N.ptr(xi[1]), ld, Bn, H, W, N.ptr(wi[1]), N.ptr(bi[1]) if b is not None else None, N.ptr(out[1]), N.stream()),
                        "vs_conv4x4_n1")
                got = _done([out], [xi, wi, bi])[0]
                lines.append(Q.line(f"{xk} {tag}", got[:, None], Q.conv4x4(x, w, b, 1, F64), Q.conv4x4(x, w, b, 1, F32), 1.0))
        for dk, dy in B.hard_dy((Bn, 1, H - 1, W - 1)).items():
            di, dx = _in(dy), _out(Bn, H, W, ld)
            N.check(L.vs_conv4x4_n1_bwd(N.ptr(di[1]), Bn, H, W, ld, N.ptr(wi[1]), N.ptr(dx[1]), N.stream()), "vs_conv4x4_n1_bwd")
            got = _done([dx], [di, wi])[0]
            g64, g32 = (Q.grad_of(lambda t: Q.conv4x4(t, w, None, 1, dt), torch.zeros(Bn, ld, H, W), dt, dy) for dt in (F64, F32))
            lines.append(Q.line(f"dy={dk} dx", got.permute(0, 3, 1, 2), g64, g32, 1.0))
        Q.envelope(f"conv4x4_n1 ld={ld} {Bn}x{H}x{W}", lines)


@pytest.mark.parametrize("shape", Q.BIAS_MAPS, ids=lambda v: "x".join(map(str, v)))
def test_conv4x4_n1_bias_grad_fp64_envelope(shape):
    """the sum of every upstream kind times 0.1: checkerboards cancel down to one element per odd plane, ramps to rounding residue, so the
    errors are absolute ones over the sum of the magnitudes"""
    lines = []
    for dk in B.DY_KINDS:
        dy = Q.bias_dy(shape, dk)
        di, db = _in(dy), _out(1)
        N.check(N.lib().vs_conv4x4_n1_bias_grad(N.ptr(di[1]), dy.numel(), N.ptr(db[1]), N.stream()), "vs_conv4x4_n1_bias_grad")
        lines.append(Q.line(f"{dk} db", _done([db], [di])[0].view(()), Q.bias_grad(dy, F64), Q.bias_grad(dy, F32), mag=float(dy.double().abs().sum())))
    Q.envelope(f"conv4x4_n1_bias_grad {'x'.join(map(str, shape))}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_disc_input
@pytest.mark.parametrize("input_nc", [1, 3])
def test_disc_input_and_its_adjoint_fp64_envelope(input_nc):
    """the frames of every pair kind -> the rows of layer 1 (RGB, or Y = 0.299 r + 0.587 g + 0.114 b), and the adjoint on every upstream kind"""
    L = N.lib()
    H, W = Q.DISC_INPUT_SHAPE
    mi = _in(torch.tensor(Q.Y_ROW, dtype=F32)) if input_nc == 1 else None
    m0 = N.ptr(mi[1]) if mi else None
    lines = []
    for kind, (x, _) in Q.hard_pairs(H, W).items():
        xi, rows = _in(x), _out(2, H, W, 4)
        N.check(L.vs_disc_input(N.ptr(xi[1]), 2, H, W, m0, N.ptr(rows[1]), N.stream()), "vs_disc_input")
        got = _done([rows], [xi] + ([mi] if mi else []))[0]
        assert not got[..., input_nc:].any()
        lines.append(Q.line(f"{kind} rows", got, Q.disc_input(x, input_nc, F64), Q.disc_input(x, input_nc, F32), 1.0))
    for dk, d4 in B.hard_dy((2, 4, H, W)).items():
        d = d4.permute(0, 2, 3, 1).contiguous()
        di, dimgs = _in(d), _out(2, 3, H, W)
        N.check(L.vs_disc_input_bwd(N.ptr(di[1]), 2, H, W, m0, N.ptr(dimgs[1]), N.stream()), "vs_disc_input_bwd")
        got = _done([dimgs], [di] + ([mi] if mi else []))[0]
        g64, g32 = (Q.grad_of(lambda t: Q.disc_input(t, input_nc, dt), torch.zeros(2, 3, H, W), dt, d) for dt in (F64, F32))
        lines.append(Q.line(f"dy={dk} dimgs", got, g64, g32, 1.0))
    Q.envelope(f"disc_input input_nc={input_nc} 2x3x{H}x{W}", lines)
