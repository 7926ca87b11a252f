"""The envelope of tests/test_gpu_loss_envelope.py has teeth: on the very inputs the GPU file uses, a seeded defect applied to the float32 formula
(tests/_loss_ref.py) falls outside max(yardstick, 2^-24) x 8 on the kind it is named for -- no LOSS_FP64_MARGIN up to the cap admits it -- while
the unmodified float32 formula is its own yardstick (ratio 1 by construction) and finite on every kind of every case; and the hard inputs hold
what they promise.  Nothing here needs a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _envelope as E
from tests import _img_bwd_ref as B
from tests import _img_ref as R
from tests import _loss_ref as Q

F32, F64 = torch.float32, torch.float64


def _teeth(tag, rows, named):
    """rows: (name, defect's error, yardstick's error) as _loss_ref.line returns them, the defect in the kernel's place.  Prints every row;
    the yardstick must be finite; the defect must be outside at the cap on every kind of `named`"""
    hit = []
    for name, bad, yard in rows:
        print(f"TEETH {tag:<44s} {name:<24s} yardstick {yard:.3e}  defect {bad:.3e}  ratio {bad / max(yard, E.U32):9.3g}")
        assert math.isfinite(yard), (tag, name)
        assert not E.outside(yard, yard)
        if E.outside(bad, yard):
            hit.append(name.split()[0])
    assert set(named) <= set(hit), (tag, named, hit)


def _finite(*ts):
    return all(bool(torch.isfinite(torch.as_tensor(t)).all()) for t in ts)


# ------------------------------------------------------------------------------------------------------------------------ hard inputs
def test_hard_inputs_hold_what_they_promise():
    p = Q.hard_pairs(35, 139)
    assert all(x.dtype == F32 and float(x.min()) >= 0 and float(x.max()) <= 1 and float(y.min()) >= 0 and float(y.max()) <= 1 for x, y in p.values())
    assert not p["dark"][0].any() and float(p["dark"][1].max()) < 0.02 and float(p["dark"][1].max()) > 0
    x, y = p["dark-bars"]
    assert not x[:, :, :8].any() and not x[:, :, -8:].any() and x[:, :, 8:-8].all() and (y[:, :, :8] == 0).any() and (y[:, :, :8] > 0).any()
    assert torch.equal(*p["identical"]) and bool((p["white"][0] == 1).all()) and bool((p["flat"][0] == 0.75).all())
    assert set(p["checker"][0].unique().tolist()) == {0.0, 1.0} and torch.equal(p["inverse"][1], 1 - p["inverse"][0])
    assert not p["impulse"][1].any() and p["impulse"][0][0, 0, 0, 0] == 0.5 and float(p["impulse"][0].max()) < 1
    lg = Q.hard_logits((3, 7, 9))
    k = lg["kink"].flatten()
    n = k.numel()
    assert int((k == 1).sum()) == n // 3 and int((k == -1).sum()) == n // 3
    rest = k[(k != 1) & (k != -1)]
    assert bool(((rest.abs() - 1).abs() <= 2 * 2.0 ** -23).all()) and (rest > 1).any() and ((rest < 1) & (rest > 0)).any() and (rest < -1).any()
    assert set(lg["large"].flatten().tolist()) == set(torch.tensor(Q.LARGE).tolist()) and float(lg["one-sided"].min()) > 1
    for kind, t in lg.items():          # the hinge terms of `one-sided` are inactive in both precisions
        assert _finite(t)
    assert not F.relu(1 - lg["one-sided"]).any() and not F.relu(1 + (-lg["one-sided"])).any()
    for C, Bn, H, W in Q.GN_CASES:
        x = Q.hard_acts(Bn, C, H, W, 4)["groups"]
        xg = x.view(Bn, 4, -1)
        var = xg.double().var(2, unbiased=False)
        for f in range(Bn):
            assert float(var[f, (f + 1) % 4]) == 0.0 and float(xg[f, (f + 2) % 4].max()) == 4e3 and float(xg[f, (f + 3) % 4].abs().max()) < 0.01
            assert abs(float(xg[f, f % 4].mean()) - 30) < 0.1
        gamma, beta = Q.gn_params(C)
        # no normalised value on the LeakyReLU kink: xhat gamma + beta in fp32 from a float64 xhat is within 3 x 2^-24 (|xhat gamma| + |beta|) < 1e-6
        # of the float64 value where the two terms cancel (|beta| < 1), so its side is the same
        for kind, xk in Q.hard_acts(Bn, C, H, W, 4).items():
            assert float(Q.gn_pre(xk, gamma, beta, F64).abs().min()) > 1e-6, (C, kind)
    z = Q.hard_acts(2, 16, 5, 7, 0)["zeros"].flatten()
    assert z[0] == 0 and not torch.signbit(z[0]) and z[1] == 0 and torch.signbit(z[1]) and z[2] == Q.SUBNORMAL and z[3] == -Q.SUBNORMAL
    assert z[2] > 0 and z[2] * 0.5 == 0          # the smallest subnormal, kept by the host


# ------------------------------------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("H,W", Q.SSIM_SHAPES, ids=lambda v: str(v))
def test_ssim_references_are_finite_and_the_shifted_moments_fall_outside_on_dark_frames(H, W):
    """the suspected defect itself: the moments of x - 0.5 in fp32.  On `dark` and `dark-bars` E[x'^2] - mu'^2 is 0.25 - 0.25 against C2 = 9e-4"""
    gs, gc, gco = Q.ssim_coeffs(H, W)
    pairs = Q.hard_pairs(H, W)
    rows, grows, scale = [], [], None
    for kind, (x, y) in pairs.items():
        r64, y32, bad = Q.ssim_stats(x, y, F64), Q.ssim_stats(x, y, F32), Q.ssim_stats(x, y, F32, shift=0.5)
        assert _finite(*r64, *y32)
        rows.append(Q.line(f"{kind} ssim", bad[0], r64[0], y32[0], scalar=True))
        rows.append(Q.line(f"{kind} cs", bad[1], r64[1], y32[1], scalar=True))
        g64, g32, gbad = (Q.grad_of(lambda t: Q.ssim_target(x, t, gs, gc, None, dt, sh), y, dt) for dt, sh in ((F64, None), (F32, None), (F32, 0.5)))
        assert _finite(g64, g32)
        scale = scale or float(g64.abs().max())
        grows.append(Q.line(f"{kind} grad", gbad, g64, g32, scale, zero=kind == "identical"))
    # `dark-bars` is dark only where an 11-row window fits inside a bar of H / 4 rows; every other window holds noise rows, whose variance is far above C2
    named = ["dark", "dark-bars"] if H // 4 >= 11 else ["dark"]
    _teeth(f"ssim stats {H}x{W}, moments of x - 0.5", rows, named)
    _teeth(f"ssim grad {H}x{W}, moments of x - 0.5", grows, named)


@pytest.mark.parametrize("H,W", Q.MS_SHAPES, ids=lambda v: str(v))
def test_msssim_references_are_finite_and_a_missing_relu_falls_outside_on_inverse(H, W):
    rows = []
    for kind in Q.MS_KINDS:
        x, y = (t[:1] for t in Q.hard_pairs(H, W)[kind])
        l64, l32, lbad = (Q.msssim_loss(x, y, dt, relu) for dt, relu in ((F64, True), (F32, True), (F32, False)))
        g64, g32 = (Q.grad_of(lambda t: Q.msssim_loss(x, t, dt), y, dt) for dt in (F64, F32))
        assert _finite(l64, l32, g64, g32), kind
        rows.append(Q.line(f"{kind} loss", lbad, l64, l32, 1.0, scalar=True))
    assert float(Q.msssim_loss(*(t[:1] for t in Q.hard_pairs(H, W)["inverse"]), F64)) == 0.0          # the gate closes: cs ~ -1 at level 0
    _teeth(f"msssim {H}x{W} without relu", rows, ["inverse"])


# ------------------------------------------------------------------------------------------------------------------------ mse / yuv / jnd
@pytest.mark.parametrize("Fn,H,W", Q.PERCEP_SHAPES)
def test_percep_and_jnd_references_are_finite_and_sign0_falls_outside_on_identical(Fn, H, W):
    rows, scale = [], None
    for kind, (x, y) in Q.hard_pairs(H, W, Fn).items():
        hm = R.jnd(x, F64)[0].to(F32)
        g64, g32 = (Q.grad_of(lambda t: Q.jnd_loss(x, t, hm, dt), y, dt) for dt in (F64, F32))
        assert _finite(hm, g64, g32, Q.jnd_loss(x, y, hm, F64), *(Q.percep(x, y, yuv, dt) for yuv in (0, 1) for dt in (F64, F32)))
        scale = scale or float(g64.abs().max())
        assert E.frame_err(Q.jnd_grad32(x, y, hm), g64) <= 4 * max(E.frame_err(g32, g64), E.U32) or not g64.any()          # the closed form is the formula
        rows.append(Q.line(f"{kind} grad", Q.jnd_grad32(x, y, hm, sign0=1.0), g64, g32, scale))
    _teeth(f"jnd grad {Fn}x3x{H}x{W}, sign(0) = 1", rows, ["identical"])


# ------------------------------------------------------------------------------------------------------------------------ decoding losses
@pytest.mark.parametrize("Bn,k", Q.BCE_SHAPES)
def test_bce_references_are_finite_and_the_unstable_form_is_no_defect_in_fp32(Bn, k):
    """`sigmoid(z) - m` as `-(1 - sigmoid(z))`: in fp32 both are the same number (sigmoid(20) is 1.0), float32 autograd is equally far from the
    float64 gradient at z = 20 (2e-9 of max |g|, below 2^-24), so the `large` kind cannot tell them apart: dropped as a seeded defect, pinned here"""
    for T in Q.BCE_TEMPS:
        for rows_ in (1, Bn):
            msgs = Q.hard_msgs(rows_, k)
            for kind, p in Q.hard_logits((Bn, k + 1)).items():
                l64, l32 = Q.bce_logits(p, msgs, T, F64), Q.bce_logits(p, msgs, T, F32)
                g64, g32 = (Q.grad_of(lambda t: Q.bce_logits(t, msgs, T, dt), p, dt) for dt in (F64, F32))
                assert _finite(l64, l32, g64, g32) and not g64[:, 0].any()
                e = [E.frame_err(Q.bce_grad32(p, msgs, T, unstable=u), g64) for u in (False, True)]
                assert not E.outside(e[0], E.frame_err(g32, g64)) and not E.outside(e[1], E.frame_err(g32, g64)), (T, kind, e)


@pytest.mark.parametrize("Bn,K,HW", Q.PIXEL_BCE_SHAPES)
def test_pixel_bce_references_are_finite(Bn, K, HW):
    masks = Q.pixel_masks(Bn, HW)
    assert int(masks[0].sum()) == 1 and bool((masks[1] == 1).all())
    for kind, p in Q.hard_logits((Bn, K, HW)).items():
        for T in Q.BCE_TEMPS:
            msgs = Q.hard_msgs(Bn, K - 1)
            g = Q.grad_of(lambda t: sum(Q.pixel_bce(t, masks, msgs, T, F64)), p, F64)
            assert _finite(*Q.pixel_bce(p, masks, msgs, T, F64), *Q.pixel_bce(p, masks, msgs, T, F32), g)
            assert not g[0, 1:][:, masks[0] == 0].any()          # unselected pixels carry no decoding gradient


# ------------------------------------------------------------------------------------------------------------------------ discriminator loss
def test_hinge_gate_ge_falls_outside_on_kink():
    lg = Q.hard_logits((3, 1, 7, 9))
    rows = []
    for kind, t in lg.items():
        real, fake = t, -t.flip(0)
        l64, l32 = Q.disc_loss(real, fake, 1, F64), Q.disc_loss(real, fake, 1, F32)
        assert _finite(*l64, *l32)
        g64 = [0.25 * Q.grad_of(lambda v: Q.disc_loss(*((v, fake) if i == 0 else (real, v)), 1, F64)[0], (real, fake)[i], F64) for i in (0, 1)]
        g32 = [0.25 * Q.grad_of(lambda v: Q.disc_loss(*((v, fake) if i == 0 else (real, v)), 1, F32)[0], (real, fake)[i], F32) for i in (0, 1)]
        good, bad = Q.hinge_grads32(real, fake, 0.25), Q.hinge_grads32(real, fake, 0.25, ge=True)
        for i, nm in enumerate(("dreal", "dfake")):
            assert not E.outside(*Q.line("", good[i], g64[i], g32[i], 1.0)[1:])
            rows.append(Q.line(f"{kind} {nm}", bad[i], g64[i], g32[i], 1.0))
        if kind == "kink":
            assert not g64[0][real == 1].any() and not g64[1][fake == -1].any() and g64[0].any()
        if kind == "one-sided":
            assert float(l64[0]) == 0 and not g64[0].any() and not g64[1].any()
    _teeth("hinge gate >=", rows, ["kink"])


# ------------------------------------------------------------------------------------------------------------------------ GroupNorm + LeakyReLU
@pytest.mark.parametrize("C,Bn,H,W", Q.GN_CASES)
def test_groupnorm_naive_variance_falls_outside_on_the_mean_30_groups(C, Bn, H, W):
    gamma, beta = Q.gn_params(C)
    rows = []
    for kind, x in Q.hard_acts(Bn, C, H, W, 4).items():
        o64, (m64, r64) = Q.gn_lrelu(x, gamma, beta, 4, F64), Q.gn_stats(x, F64)
        o32, (m32, r32) = E.one_thread(lambda: Q.gn_lrelu(x, gamma, beta, 4, F32)), Q.gn_stats(x, F32)
        assert _finite(o64, m64, r64, o32, m32, r32)
        good, bad = Q.gn_lrelu32(x, gamma, beta), Q.gn_lrelu32(x, gamma, beta, naive_var=True)
        assert not E.outside(E.frame_err(good[2], o64), E.frame_err(o32, o64))
        rows.append(Q.line(f"{kind} rstd", bad[1], r64, r32, scalar=True))
        rows.append(Q.line(f"{kind} out", bad[2], o64, o32))
        dy = B.hard_dy((Bn, C, H, W))["noise"]
        for wrt in (x, gamma, beta):          # the gradients exist and are finite in both precisions
            for dt in (F64, F32):
                ins = [x, gamma, beta]
                f = lambda t: Q.gn_lrelu(*[t if v is wrt else v.to(dt) for v in ins], 4, dt)          # noqa: E731
                assert _finite(Q.grad_of(f, wrt, dt, dy))
    _teeth(f"groupnorm C={C}, variance as E[x^2] - mean^2", rows, ["groups"])


def test_leaky_relu_derivative_1_at_zero_falls_outside_on_zeros():
    rows = []
    for kind, x in Q.hard_acts(2, 16, 5, 7, 0).items():
        dy = B.hard_dy((2, 16, 5, 7))["noise"]
        g64, g32 = (Q.grad_of(lambda t: Q.gn_lrelu(t, None, None, 0, dt), x, dt, dy) for dt in (F64, F32))
        assert torch.equal(Q.lrelu_bwd32(x, dy), g32)
        rows.append(Q.line(f"{kind} dx", Q.lrelu_bwd32(x, dy, at_zero=1.0), g64, g32))
    _teeth("leaky_relu, derivative 1 at 0", rows, ["zeros"])


# ------------------------------------------------------------------------------------------------------------------------ 4 x 4 convolutions
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ld,ci,n", [Q.WGRAD_PAIRS[1], Q.WGRAD_PAIRS[2], Q.WGRAD_PAIRS[5]])
def test_wgrad_without_the_last_output_row_falls_outside(ld, ci, n, stride):
    for Bn, H, W in Q.WGRAD_MAPS:
        Ho, Wo = Q.conv_out(H, W, stride)
        rows = []
        for xk, x in Q.hard_acts(Bn, ci, H, W, 4).items():
            for kind, dy in B.hard_dy((Bn, n, Ho, Wo)).items():
                g64, g32 = Q.conv_wgrad(x, dy, n, stride, F64), Q.conv_wgrad(x, dy, n, stride, F32)
                assert _finite(g64, g32)
                rows.append(Q.line(f"{kind}/{xk}", Q.conv_wgrad(x, dy, n, stride, F32, drop_last_row=True), g64, g32))
        _teeth(f"wgrad ld={ld} ci={ci} n={n} s={stride} {Bn}x{H}x{W}, last row dropped", rows, ["noise/noise", "ones/groups", "checker/groups", "ramp/noise"])


def test_n1_references_are_finite_and_a_cancelling_bias_sum_falls_outside_on_checker():
    for ld in Q.N1_LDS:
        for Bn, H, W in Q.N1_MAPS:
            w, bias = Q.conv_weights(1, ld), torch.tensor([0.3])
            for xk, x in Q.hard_acts(Bn, ld, H, W, 4).items():
                assert _finite(Q.conv4x4(x, w, bias, 1, F64), Q.conv4x4(x, w, bias, 1, F32))
            for kind, dy in B.hard_dy((Bn, 1, H - 1, W - 1)).items():
                assert _finite(*(Q.grad_of(lambda t: Q.conv4x4(t, w, None, 1, dt), torch.zeros(Bn, ld, H, W), dt, dy) for dt in (F64, F32)))
    rows = []
    n = Q.BIAS_MAPS[-1]
    for kind in B.DY_KINDS:
        dy = Q.bias_dy(n, kind)
        rows.append(Q.line(f"{kind} db", Q.bias_grad_cancelling32(dy), Q.bias_grad(dy, F64), Q.bias_grad(dy, F32), mag=float(dy.double().abs().sum())))
    _teeth(f"bias gradient n={n}, positives first", rows, ["checker"])


@pytest.mark.parametrize("input_nc", [1, 3])
def test_disc_input_references_are_finite(input_nc):
    H, W = Q.DISC_INPUT_SHAPE
    for kind, (x, _) in Q.hard_pairs(H, W).items():
        r64, r32 = Q.disc_input(x, input_nc, F64), Q.disc_input(x, input_nc, F32)
        assert _finite(r64, r32) and r64.shape == (2, H, W, 4) and not r64[..., input_nc:].any()
