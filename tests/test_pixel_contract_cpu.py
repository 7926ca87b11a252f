"""The envelope of tests/test_gpu_pixel_envelope.py (and the per-frame bias cases of tests/test_gpu_frame_bias_envelope.py) stands on firm ground
and has teeth.
  * The float64 references of tests/_pixel_ref.py are the torch modules' and the oracle's: nn.Upsample + ReflectionPad2d + Conv2d + LayerNorm +
    GELU for the Upsample group (and autograd for its adjoint), Conv2d 1x1 with autograd for the per-pixel linear layer's dx / dw / db.
  * The yardstick alone is finite on every case and has ratio 1 by construction, so the GPU file cannot fail for the reference's own sake; the
    case that stands for the 512-workgroup cap is at it; the vote inputs hold every pair of special logit and special mask value.
  * Seeded fp32 emulations of defects fall outside  8 x max(yardstick, floor)  on these very cases -- no PIXEL_MARGIN up to the cap admits them:
    tanh-GELU, unbiased variance, a dropped last row of a 32-row tile in dw, partials of empty workgroups left as NaN, y (1 - y) omitted behind the
    sigmoid, the frame index as row >> log2 in place of row / HW on a frame that is no power of two (in dw and in a per-frame bias).
  * vs_conv_plan sizes the K-slice workspace of the ragged 3x3 + second-phase case of tests/test_gpu_frame_bias_envelope.py with the slice of the
    second phase (it was one slice short there: the kernel wrote past the workspace).
Nothing here needs a GPU."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import videoseal_ref as O
from tests import _envelope as E
from tests import _pixel_ref as R
from tests import _split_ref as S
from videoseal_amd import native as N

D = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))
    assert err <= tol, err


# ------------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("f,H,W", [(2, 2, 2), (4, 3, 5), (2, 2, 9), (4, 2, 2)])
def test_upgather_is_the_upsample_group_of_the_modules_and_of_the_oracle(f, H, W):
    g = torch.Generator().manual_seed(10 + f + H + W)
    B, Ci, Co = 2, 5, 8
    v = torch.randn(B, Ci, H, W, dtype=D, generator=g)
    conv = nn.Conv2d(Ci, Co, 3, bias=False).double()
    ln = nn.LayerNorm(Co, eps=R.LN_EPS).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Co, Ci, 3, 3, dtype=D, generator=g) / 7)
        ln.weight.copy_(1 + 0.3 * torch.randn(Co, dtype=D, generator=g))
        ln.bias.copy_(0.3 * torch.randn(Co, dtype=D, generator=g))
    z = torch.einsum("bihw,oikl->bhwklo", v, conv.weight.detach()).reshape(B, H, W, 9 * Co).requires_grad_()
    raw = R.up_gather(z, H, W, Co, f)
    stage = nn.Sequential(nn.Upsample(scale_factor=f, mode="bilinear", align_corners=False), nn.ReflectionPad2d(1), conv)
    want = stage(v).detach().permute(0, 2, 3, 1)
    _close(raw.detach(), want)
    out = R.up_norm(raw.detach(), ln.weight.detach(), ln.bias.detach())
    _close(out, nn.GELU()(ln(want)).detach())
    sd = {"p.upsample_block.2.weight": conv.weight.detach(), "p.upsample_block.3.weight": ln.weight.detach(), "p.upsample_block.3.bias": ln.bias.detach()}
    _close(out, O.upsample_block(sd, "p", v, f, F.gelu).permute(0, 2, 3, 1))
    # the adjoint is autograd's, and <A z, d> = <z, A^T d>
    d = torch.randn(raw.shape, dtype=D, generator=g)
    raw.backward(d)
    adj = R.up_gather_adjoint(d, H, W, Co, f)
    _close(adj, z.grad)
    lhs, rhs = float((raw.detach() * d).sum()), float((z.detach() * adj).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # the bilinear weights are exact in fp32 (multiples of 1 / (2 f)), as the kernel's own
    assert torch.equal(R.up_axis(H, f, torch.float32).double(), R.up_axis(H, f))


@pytest.mark.parametrize("sig", [False, True])
def test_linear_is_conv2d_1x1_and_its_autograd(sig):
    g = torch.Generator().manual_seed(20)
    B, C, K, H, W = 2, 8, 5, 3, 7
    conv = nn.Conv2d(C, K, 1).double()
    x = torch.randn(B, C, H, W, dtype=D, generator=g, requires_grad=True)
    out = conv(x)
    out = torch.sigmoid(out) if sig else out
    dp = torch.randn(B, K, H, W, dtype=D, generator=g)
    out.backward(dp)
    rows = x.detach().permute(0, 2, 3, 1).reshape(-1, C)
    w = conv.weight.detach().view(K, C)
    y = R.lin_fwd(rows, w, conv.bias.detach(), sig, B)
    _close(y, out.detach().view(B, K, H * W))
    dx, dw, db = R.lin_bwd(dp.view(B, K, H * W), y if sig else None, rows, w)
    _close(dx, x.grad.permute(0, 2, 3, 1).reshape(-1, C))
    _close(dw, conv.weight.grad.view(K, C))
    _close(db, conv.bias.grad)


def test_the_cap_case_is_at_the_workgroup_cap():
    C, K, H, W, sig, pad = R.LIN_CAP
    rows = R.LIN_B * H * W
    assert rows == 132098
    assert R.lin_plan(rows, R.lin_partial_floats(rows, K, C), K, C) == (512, 288, 459)
    for case in R.LIN_CASES:
        c, k, h, w = case[:4]
        nb, rpb, first_empty = R.lin_plan(R.LIN_B * h * w, R.lin_partial_floats(R.LIN_B * h * w, k, c), k, c)
        assert (first_empty < nb) == (case == R.LIN_CAP)


def test_vote_inputs_hold_every_special_pair_and_the_reference_is_the_metrics_rule():
    for (B, K, HW) in R.VOTE_CASES:
        for thr in R.VOTE_THRESHOLDS:
            x, m = R.vote_inputs(B, K, HW, thr)
            t = torch.tensor(thr)
            inf = torch.tensor(float("inf"))
            mm = m[:, None, :].expand_as(x)
            for lv in (t, torch.nextafter(t, -inf), torch.nextafter(t, inf)):
                for sel in (mm == 0, mm == 0.3, mm.abs() == 2.0 ** -149):
                    assert bool(((x == lv) & sel).any()), (B, K, HW, thr, float(lv))
            assert bool(((m == 0) & torch.signbit(m)).any()) and bool(((x == 0) & torch.signbit(x)).any())
            votes, nsel = R.vote_ref(x, m, thr)
            assert torch.equal(nsel, m.bool().sum(-1)) and torch.equal(votes, ((x > thr) & m.bool()[:, None]).sum(-1))
            assert int(((x == t) & (mm != 0)).sum()) > 0 and int(nsel.sum()) < B * HW
            assert torch.equal(R.vote_ref(x, None, thr)[1], torch.full((B,), HW))


# ------------------------------------------------------------------------------------------------------------------------ the yardstick alone
def _finite_and_inside(err):
    assert math.isfinite(err), err
    assert not E.outside(err, err) and not E.outside(err, err, 1.0)


@pytest.mark.parametrize("case", R.LIN_CASES, ids=R.lin_name)
def test_linear_yardsticks_are_finite(case):
    r64, r32, P = R.lin_fwd_ref(case)
    _finite_and_inside(R.group_err(r32, r64, -1) if P is None else R.units(r32, r64, P))
    if P is not None:
        assert bool((P == 0).any()), "no output without a non-zero term"
    for kind in R.DP_KINDS:
        t64, t32, Ps = R.lin_bwd_ref(case, kind)
        for a, b, p, n in zip(t32, t64, Ps, R.lin_bwd_terms(case)):
            _finite_and_inside(R.units(a, b, p, n))
        assert bool((Ps[0] == 0).any())
    dp = R.lin_dpreds(case, "positive")
    assert float(dp.min()) >= 0 and float(R.lin_dpreds(case, "cancelling").min()) < 0


@pytest.mark.parametrize("case", R.UP_CASES, ids=R.up_name)
def test_upgather_yardsticks_are_finite_and_the_constant_frame_is_exact(case):
    ref = R.up_ref(case)
    for key in ("raw", "adj"):
        r64, r32, P = ref[key]
        _finite_and_inside(R.units(r32, r64, P))
        assert bool((P == 0).any())
    o64, o32 = ref["out"]
    for name, hip, yard in R.up_class_rows("px", o32, o64, o32):
        _finite_and_inside(yard)
    # every pixel of the constant frame: 9 x 30.25 on every channel, variance exactly 0, also in fp32
    r64, r32, _ = ref["raw"]
    assert torch.equal(r64[1], torch.full_like(r64[1], 272.25)) and torch.equal(r32[1].double(), r64[1])
    lb = R.up_inputs(case)[2]
    assert torch.equal(o32[1], F.gelu(lb).expand_as(o32[1]))


@pytest.mark.parametrize("case", R.MM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_matmul_yardstick_is_finite(case):
    r64, r32, P = R.mm_ref(case)
    _finite_and_inside(R.units(r32, r64, P))
    assert case[1] == 1 or bool((P == 0).any())


# ------------------------------------------------------------------------------------------------------------------------ seeded defects
@pytest.mark.parametrize("defect", ["tanh_gelu", "unbiased"])
@pytest.mark.parametrize("case", R.UP_CASES, ids=R.up_name)
def test_a_wrong_gelu_or_variance_falls_outside(case, defect):
    Co, f, H, W, pad = case
    z, lw, lb, _ = R.up_inputs(case)
    o64, o32 = R.up_ref(case)["out"]
    bad = E.one_thread(lambda: R.up_norm(R.up_gather(z, H, W, Co, f), lw, lb, **{defect: True}))
    rows = R.up_class_rows("px", bad, o64, o32)
    assert any(E.outside(err, yard) for _, err, yard in rows), rows


@pytest.mark.parametrize("kind", R.DP_KINDS)
@pytest.mark.parametrize("case", R.LIN_CASES, ids=R.lin_name)
def test_a_dropped_tile_row_or_a_wrong_frame_index_in_dw_falls_outside(case, kind):
    C, K, H, W, sig, pad = case
    rows = R.LIN_B * H * W
    x = R.lin_inputs(case)[0]
    (dx64, dw64, db64), (dx32, dw32, db32), (Px, Pw, Pb) = R.lin_bwd_ref(case, kind)
    nb, rpb, first_empty = R.lin_plan(rows, R.lin_partial_floats(rows, K, C), K, C)
    y = R.lin_y(case)
    d = R.lin_dlogit(R.lin_dpreds(case, kind), y)
    nx, nw, nb_ = R.lin_bwd_terms(case)
    units_x, units_w, units_b = (lambda t: R.units(t, dx64, Px, nx)), (lambda t: R.units(t, dw64, Pw, nw)), (lambda t: R.units(t, db64, Pb, nb_))
    yard_w, yard_b = units_w(dw32), units_b(db32)
    # the emulated partition itself (no defect) is inside
    dw, db = E.one_thread(lambda: R.lin_wgrad_emulated(d, x, nb, rpb))
    assert not E.outside(units_w(dw), yard_w, 1.0) and not E.outside(units_b(db), yard_b, 1.0)
    dw, db = E.one_thread(lambda: R.lin_wgrad_emulated(d, x, nb, rpb, drop_tile_last_row=True))
    assert E.outside(units_w(dw), yard_w, 1.0) and E.outside(units_b(db), yard_b, 1.0)
    if (H * W) & (H * W - 1):                              # a frame that is no power of two: all of these
        (_, dw, db) = R.lin_bwd_ref(case, kind, shift_frame=True)[1]
        assert E.outside(units_w(dw), yard_w, 1.0) and E.outside(units_b(db), yard_b, 1.0)
    if sig:
        (dx, dw, db) = R.lin_bwd_ref(case, kind, no_yprime=True)[1]
        assert E.outside(units_x(dx), units_x(dx32), 1.0) and E.outside(units_w(dw), yard_w, 1.0)


def test_nan_partials_of_empty_workgroups_fall_outside():
    C, K, H, W, sig, pad = R.LIN_CAP
    rows = R.LIN_B * H * W
    x = R.lin_inputs(R.LIN_CAP)[0]
    (dx64, dw64, db64), (dx32, dw32, db32), (Px, Pw, Pb) = R.lin_bwd_ref(R.LIN_CAP, "positive")
    nb, rpb, first_empty = R.lin_plan(rows, R.lin_partial_floats(rows, K, C), K, C)
    d = R.lin_dlogit(R.lin_dpreds(R.LIN_CAP, "positive"), None)
    dw, db = E.one_thread(lambda: R.lin_wgrad_emulated(d, x, nb, rpb, nan_empty=True))
    assert E.outside(R.units(dw, dw64, Pw), R.units(dw32, dw64, Pw), 1.0) and E.outside(R.units(db, db64, Pb), R.units(db32, db64, Pb), 1.0)


def test_a_shifted_frame_index_in_a_per_frame_bias_falls_outside():
    """35-row frames (B = 3, 5 x 7): frame = row >> 5 gives rows 32..34 of frame 0 the vector of frame 1 (and so on); in the split family's units"""
    B, H, W, K, Co = 3, 5, 7, 32, 64
    a, w = S.hard_act(B, K, H, W, 9100), S.hard_weights(Co, K, 1, 9101)
    bias = torch.stack([S.hard_bias(Co, 9102 + i) for i in range(B)])
    r = S.ideal(a, w, 3)
    b4 = bias.double()[:, :, None, None]
    Sv, P = r.S + b4, r.P + b4.abs()
    good = E.one_thread(lambda: r.ref32 + bias[:, :, None, None])
    row = torch.arange(B * H * W)
    wrong = bias[(row >> 5).clamp_max(B - 1)].view(B, H * W, Co).permute(0, 2, 1).reshape(B, Co, H, W)
    bad = E.one_thread(lambda: r.ref32 + wrong)
    yard = float(S.units(good, Sv, P).max())
    assert not E.outside(yard, yard, 1.0) and E.outside(float(S.units(bad, Sv, P).max()), yard, 1.0)


# ------------------------------------------------------------------------------------------------------------------------ the K-slice workspace
@pytest.mark.parametrize("H,W", [(24, 40), (16, 16), (13, 21)])
def test_the_plan_counts_the_second_phase_slice_on_ragged_frames_too(H, W):
    """the wave-specialised 3x3 kernel, named by its tile, runs on any frame size and writes slice `split_k` for its 1x1 second phase: the
    workspace vs_conv_plan sizes must hold split_k + 1 slices whether or not the frame is a whole number of 8 x 16 tiles (the pointer fields are
    flags to the plan: it never dereferences them)"""
    B, Cin, Co, Cin2, sk = 3, 32, 192, 16, 2
    fake = 1 << 16
    d = N.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.CinP, d.N, d.n_store = B, H, W, Cin, Cin, Co, Co
    d.KH, d.KW, d.SH, d.SW, d.PH, d.PW, d.Ho, d.Wo = 3, 3, 1, 1, 1, 1, H, W
    d.in_sx, d.in_sy, d.in_sb = Cin, W * Cin, H * W * Cin
    d.wt_split, d.wt_blk, d.in2, d.wt2, d.wt2_blk, d.Cin2P = fake, fake, fake, fake, fake, Cin2
    d.tile_hint, d.split_k = N.CONV_TILE_HI | 0, sk
    p = N.ConvPlan()
    assert N.lib().vs_conv_plan(ctypes.byref(d), 0, 0, ctypes.byref(p)) == 0
    assert (p.split_k, p.ws_slices, p.tile_hint) == (sk, sk + 1, N.CONV_TILE_HI | 0)
    d.in2 = d.wt2 = d.wt2_blk = None                     # without a second phase: the K slices alone
    assert N.lib().vs_conv_plan(ctypes.byref(d), 0, 0, ctypes.byref(p)) == 0 and p.ws_slices == sk
