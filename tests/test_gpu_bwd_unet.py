"""GPU tests of the U-Net backward (csrc/bwd_unet.hip, videoseal_amd.training.EmbedderBackward).  Unit level: every kernel against torch
autograd of the same op on the GPU.  End to end: all `embedder.unet.*` gradients against autograd through the oracle's functional U-Net
(CPU, fp32) for a random d(delta).

The U-Net is piecewise linear in its ReLUs: a forward that differs in the last bits flips a few of the ~10^7 ReLU decisions and moves the
gradient discretely -- the CPU oracle run in fp32 and in fp64 already differs by up to 1.3 % of a tensor's largest element on the VideoSeal 1.0
U-Net (median 0.27 %; /tmp-free reproduction: tests/tools/relu_flip_sensitivity.py).  The comparison therefore runs the oracle's autograd WITH THE
RELU DECISIONS OF THE HIP FORWARD (read back from the operands the backward keeps): every remaining difference is arithmetic, and the
tolerance is tight.  The unconstrained comparison is kept with the tolerance the fp32-vs-fp64 experiment justifies."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import videoseal_ref as R  # noqa: E402
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from oracle.weights import make_state_dict, spec_from_card, tiny_spec  # noqa: E402
from tests._cases import CARDS  # noqa: E402
from tests._envelope import ENV_SHAPES, bwd_envelope as envelope, cpu_autograd, group_err, hard_matrix  # noqa: E402
from tests._gpu import _lib, _MaskedF, _padded, _rand, hip_relu_masks  # noqa: E402
from tests._model import make_model  # noqa: E402

from videoseal_amd import native as N  # noqa: E402


def _nhwc(t, ld):
    C = t.shape[1]
    return _padded(t.detach().permute(0, 2, 3, 1).reshape(-1, C), ld).contiguous()


@pytest.mark.parametrize("rows,C,ld", [(300, 8, 8), (1000, 20, 20), (70, 6, 8), (5000, 64, 64)])
def test_bn_relu_bwd(rows, C, ld):
    L, st = _lib()
    raw = (_rand(rows, C, seed=1) * 1.5 + 0.2).requires_grad_(True)
    gam, bet = (_rand(C, seed=2) * 0.5 + 1).requires_grad_(True), _rand(C, seed=3, scale=0.3).requires_grad_(True)
    y = F.relu(F.batch_norm(raw, None, None, gam, bet, training=True, eps=1e-5))
    dy = _rand(rows, C, seed=4)
    y.backward(dy)
    ra, dya = _padded(raw.detach(), ld), _padded(dy, ld)
    part = torch.empty(int(L.vs_bn_partial_doubles(rows, ld)), dtype=torch.float64, device="cuda")
    sums = torch.empty(2 * ld + 1, dtype=torch.float64, device="cuda")
    N.check(L.vs_bn_partial_sums(N.ptr(ra), rows, C, ld, N.ptr(part), N.ptr(sums), st), "vs_bn_partial_sums")
    v = torch.zeros(4, ld, device="cuda")
    gp, bp = _padded(gam.detach()[None], ld)[0].contiguous(), _padded(bet.detach()[None], ld)[0].contiguous()
    N.check(L.vs_bn_finish_sums(N.ptr(sums), C, ld, N.ptr(gp), N.ptr(bp), 1e-5, 0.1, None, None, N.ptr(v[0]), N.ptr(v[1]), st), "vs_bn_finish_sums")
    N.check(L.vs_bn_mean_rstd(N.ptr(sums), C, ld, 1e-5, N.ptr(v[2]), N.ptr(v[3]), st), "vs_bn_mean_rstd")
    rd = raw.detach().double()
    assert (v[2][:C].double() - rd.mean(0)).abs().max() < 1e-6
    assert (v[3][:C].double() - 1 / torch.sqrt(rd.var(0, unbiased=False) + 1e-5)).abs().max() < 1e-5
    ldp = (C + 3) // 4 * 4
    bpart = torch.empty(int(L.vs_bn_bwd_partial_floats(rows, ldp)), device="cuda")
    bsums = torch.empty(2 * ldp + 1, dtype=torch.float64, device="cuda")
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    N.check(L.vs_bn_relu_bwd_sums(N.ptr(ra), ld, N.ptr(dya), ld, N.ptr(v[2]), N.ptr(v[3]), N.ptr(v[0]), N.ptr(v[1]), 1, rows, C, N.ptr(bpart), N.ptr(bsums),
                                  N.ptr(dg), N.ptr(db), st), "vs_bn_relu_bwd_sums")
    assert float(bsums[-1]) == rows
    dx = torch.full((rows, ld), 7.0, device="cuda")
    N.check(L.vs_bn_relu_bwd_apply(N.ptr(ra), ld, N.ptr(dya), ld, N.ptr(v[2]), N.ptr(v[3]), N.ptr(v[0]), N.ptr(v[1]), 1, N.ptr(bsums), rows, C, N.ptr(dx),
                                   ld, st), "vs_bn_relu_bwd_apply")
    assert (dx[:, :C] - raw.grad).abs().max() <= 5e-5 * raw.grad.abs().max()
    assert (dx[:, C:] == 0).all()
    assert (dg - gam.grad).abs().max() <= 5e-5 * gam.grad.abs().max()
    assert (db - bet.grad).abs().max() <= 5e-5 * bet.grad.abs().max()


@pytest.mark.parametrize("rows,C,ld", ENV_SHAPES)
def test_bn_relu_bwd_chain_fp64_envelope(rows, C, ld):
    """vs_bn_partial_sums -> vs_bn_finish_sums / vs_bn_mean_rstd -> vs_bn_relu_bwd_sums -> vs_bn_relu_bwd_apply on hard channels (mean 30 and
    std 0.5: E[x^2] - mean^2 cancels four digits; a constant channel: variance 0; a single 4e3 outlier; a channel of magnitude 1e-3, below
    sqrt(eps)) against float64 autograd of relu(batch_norm(training=True)) on the CPU, per channel (see tests/test_gpu_bwd.py for the metric
    and the yardstick).
    ReLU decisions: an element whose float64 pre-activation lies within the fp32 rounding of raw * scale + shift of zero -- tau = 4 U (|raw *
    scale| + |mean * scale| + |beta|): scale, shift and the multiply-add each round once -- may legitimately fall on either side, so such
    elements are left out of the dx comparison; at most 0.1 % of the elements may be (ATen's fp32 run flips none on these inputs).  beta of
    the constant channel, whose pre-activation IS beta, is set away from zero."""
    L, st = _lib()
    g = torch.Generator().manual_seed(60)
    raw = hard_matrix(rows, C, 61, "cols")
    gam, bet, dy = 1 + 0.5 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g), torch.randn(rows, C, generator=g)
    bet[1] = 0.25

    def autograd(dt):
        rr, gg, bb = (t.to(dt).requires_grad_(True) for t in (raw, gam, bet))
        pre = F.batch_norm(rr, None, None, gg, bb, training=True, eps=1e-5)
        F.relu(pre).backward(dy.to(dt))
        return rr.grad, gg.grad, bb.grad, pre.detach()
    r64, r32 = cpu_autograd(autograd)
    rd = raw.double()
    mean64, var64 = rd.mean(0), rd.var(0, unbiased=False)
    rstd64 = 1 / torch.sqrt(var64 + 1e-5)
    sc64 = gam.double() * rstd64
    tau = 4 * 2.0 ** -24 * ((rd * sc64).abs() + (mean64 * sc64).abs() + bet.double().abs())
    keep = (r64[3].abs() > tau).double()
    assert 1 - float(keep.mean()) <= 1e-3
    assert torch.equal(r32[3] > 0, r64[3] > 0)                   # the yardstick itself takes every ReLU decision of the reference
    ra, dya = _padded(raw.cuda(), ld), _padded(dy.cuda(), ld)
    part = torch.empty(int(L.vs_bn_partial_doubles(rows, ld)), dtype=torch.float64, device="cuda")
    sums = torch.empty(2 * ld + 1, dtype=torch.float64, device="cuda")
    N.check(L.vs_bn_partial_sums(N.ptr(ra), rows, C, ld, N.ptr(part), N.ptr(sums), st), "vs_bn_partial_sums")
    v = torch.zeros(4, ld, device="cuda")
    gp, bp = _padded(gam.cuda()[None], ld)[0].contiguous(), _padded(bet.cuda()[None], ld)[0].contiguous()
    N.check(L.vs_bn_finish_sums(N.ptr(sums), C, ld, N.ptr(gp), N.ptr(bp), 1e-5, 0.1, None, None, N.ptr(v[0]), N.ptr(v[1]), st), "vs_bn_finish_sums")
    N.check(L.vs_bn_mean_rstd(N.ptr(sums), C, ld, 1e-5, N.ptr(v[2]), N.ptr(v[3]), st), "vs_bn_mean_rstd")
    ldp = (C + 3) // 4 * 4
    bpart = torch.empty(int(L.vs_bn_bwd_partial_floats(rows, ldp)), device="cuda")
    bsums = torch.empty(2 * ldp + 1, dtype=torch.float64, device="cuda")
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    N.check(L.vs_bn_relu_bwd_sums(N.ptr(ra), ld, N.ptr(dya), ld, N.ptr(v[2]), N.ptr(v[3]), N.ptr(v[0]), N.ptr(v[1]), 1, rows, C, N.ptr(bpart), N.ptr(bsums),
                                  N.ptr(dg), N.ptr(db), st), "vs_bn_relu_bwd_sums")
    dx = torch.full((rows, ld), 7.0, device="cuda")
    N.check(L.vs_bn_relu_bwd_apply(N.ptr(ra), ld, N.ptr(dya), ld, N.ptr(v[2]), N.ptr(v[3]), N.ptr(v[0]), N.ptr(v[1]), 1, N.ptr(bsums), rows, C, N.ptr(dx),
                                   ld, st), "vs_bn_relu_bwd_apply")
    assert (dx[:, C:] == 0).all()
    # the forward statistics: mean and rstd are single correctly-rounded-or-nearly values, the yardstick is one fp32 rounding (2^-24, the floor)
    envelope(f"bn_relu_bwd chain rows={rows} C={C} ld={ld}", [
        ("mean/chan", group_err(v[2][:C], mean64, None), 0.0),
        ("rstd/chan", group_err(v[3][:C], rstd64, None), 0.0),
        ("dx/chan", group_err(dx[:, :C], r64[0], 0, keep), group_err(r32[0], r64[0], 0, keep)),
        ("dgamma/ch", group_err(dg, r64[1], None), group_err(r32[1], r64[1], None)),
        ("dbeta/ch", group_err(db, r64[2], None), group_err(r32[2], r64[2], None))])


@pytest.mark.parametrize("B,H,W,C,ld", [(2, 8, 8, 4, 4), (1, 9, 7, 6, 8), (2, 5, 6, 8, 8)])
def test_stride2_conv_adjoint_pieces(B, H, W, C, ld):
    """vs_dilate2 (+ the flipped conv, here through F.conv2d) and vs_im2col3x3_strided against autograd of conv2d(stride=2, padding=1)"""
    L, st = _lib()
    Co = 5
    x = _rand(B, C, H, W, seed=5).requires_grad_(True)
    w = _rand(Co, C, 3, 3, seed=6).requires_grad_(True)
    y = F.conv2d(x, w, stride=2, padding=1)
    dy = _rand(*y.shape, seed=7)
    y.backward(dy)
    Ho, Wo = y.shape[-2:]
    dya = _nhwc(dy, 8)
    dil = torch.full((B * H * W, 8), 7.0, device="cuda")
    N.check(L.vs_dilate2(N.ptr(dya), B, Ho, Wo, 8, H, W, N.ptr(dil), st), "vs_dilate2")
    dil_nchw = dil.view(B, H, W, 8)[..., :Co].permute(0, 3, 1, 2)
    dx = F.conv2d(dil_nchw, w.detach().flip(2, 3).permute(1, 0, 2, 3), padding=1)
    assert (dx - x.grad).abs().max() < 3e-5
    xa = _nhwc(x, ld)
    cols = torch.full((B * Ho * Wo, 9 * ld), 7.0, device="cuda")
    N.check(L.vs_im2col3x3_strided(N.ptr(xa), B, H, W, ld, 2, N.ptr(cols), st), "vs_im2col3x3_strided")
    dw = (dya[:, :Co].t() @ cols).view(Co, 3, 3, ld)[..., :C].permute(0, 3, 1, 2)
    assert (dw - w.grad).abs().max() <= 3e-5 * w.grad.abs().max()


@pytest.mark.parametrize("B,H,W,C1,C2", [(2, 4, 5, 4, 8), (1, 1, 3, 4, 4), (2, 7, 3, 8, 4), (1, 2, 2, 4, 4)])
def test_upcat2x_bwd(B, H, W, C1, C2):
    L, st = _lib()
    x, sk = _rand(B, C1, H, W, seed=8).requires_grad_(True), _rand(B, C2, H, W, seed=9).requires_grad_(True)
    s = 2 ** -0.5
    y = F.interpolate(torch.cat([x, sk * s], 1), scale_factor=2, mode="bilinear", align_corners=False)
    dy = _rand(*y.shape, seed=10)
    y.backward(dy)
    # forward of the existing kernel first (the adjoint must match ITS tap convention)
    xa, ska = _nhwc(x, C1), _nhwc(sk, C2)
    cat = torch.empty(B * 4 * H * W, C1 + C2, device="cuda")
    N.check(L.vs_upcat2x(N.ptr(xa), C1, C1, N.ptr(ska), C2, C2, s, B, H, W, N.ptr(cat), C1 + C2, st), "vs_upcat2x")
    assert (cat - _nhwc(y, C1 + C2)).abs().max() < 2e-6
    dya = _nhwc(dy, C1 + C2)
    dx, dsk = torch.full((B * H * W, C1), 7.0, device="cuda"), torch.full((B * H * W, C2), 7.0, device="cuda")
    N.check(L.vs_upcat2x_bwd(N.ptr(dya), C1 + C2, B, H, W, C1, C2, s, N.ptr(dx), C1, N.ptr(dsk), C2, st), "vs_upcat2x_bwd")
    assert (dx - _nhwc(x.grad, C1)).abs().max() < 2e-5
    assert (dsk - _nhwc(sk.grad, C2)).abs().max() < 2e-5


def test_msg_table_outc_and_relu_adjoints():
    L, st = _lib()
    # message table
    Bm, nbits, hidden = 3, 7, 12
    table = _rand(2 * nbits, hidden, seed=11).requires_grad_(True)
    msgs = (torch.rand(Bm, nbits, generator=torch.Generator().manual_seed(12)) > 0.5).cuda()
    rows_sel = 2 * torch.arange(nbits, device="cuda")[None] + msgs.long()
    lat = table[rows_sel].sum(1)
    dlat = _rand(Bm, hidden, seed=13)
    lat.backward(dlat)
    dt = torch.empty(2 * nbits, hidden, device="cuda")
    N.check(L.vs_msg_table_grad(N.ptr(dlat), N.ptr(msgs.to(torch.int32).contiguous()), Bm, nbits, hidden, N.ptr(dt), st), "vs_msg_table_grad")
    assert (dt - table.grad).abs().max() < 1e-6
    # output conv + tanh
    B, HW, C, oc = 2, 30, 8, 3
    x = _rand(B, HW, C, seed=14).requires_grad_(True)
    w, b = _rand(oc, C, seed=15).requires_grad_(True), _rand(oc, seed=16).requires_grad_(True)
    delta = torch.tanh(F.linear(x, w, b)).permute(0, 2, 1).contiguous()                  # planar [B][oc][HW]
    dd = _rand(B, oc, HW, seed=17)
    delta.backward(dd)
    dx = torch.full((B * HW, C), 7.0, device="cuda")
    dv = torch.empty(B * HW, 4, device="cuda")
    N.check(L.vs_outc_tanh_bwd(N.ptr(delta.detach()), N.ptr(dd), HW, B, C, N.ptr(w.detach().contiguous()), oc, 1, N.ptr(dx), C, N.ptr(dv), st),
            "vs_outc_tanh_bwd")
    assert (dx - x.grad.reshape(-1, C)).abs().max() < 1e-5
    assert (dv[:, :oc].t() @ x.detach().reshape(-1, C) - w.grad).abs().max() < 1e-4
    assert (dv[:, :oc].sum(0) - b.grad).abs().max() < 1e-4 and (dv[:, oc:] == 0).all()
    # ReLU
    z, dy = _rand(50, 6, seed=18), _rand(50, 6, seed=19)
    za, dya = _padded(z, 8), _padded(dy, 8)
    dz = torch.full((50, 8), 7.0, device="cuda")
    N.check(L.vs_relu_bwd(N.ptr(za), 8, N.ptr(dya), 8, 50, 6, N.ptr(dz), 8, st), "vs_relu_bwd")
    assert torch.equal(dz[:, :6], dy * (z > 0)) and (dz[:, 6:] == 0).all()


def _embedder_case(spec, sd, n, seed, masked=True):
    import ctypes as C
    from videoseal_amd.model import _msgs_i32
    from videoseal_amd.training import EmbedderBackward
    S = spec.img_size
    imgs = synthetic_frames(n, S, S, seed=seed)
    x01 = imgs if not spec.yuv else (0.299 * imgs[:, 0:1] + 0.587 * imgs[:, 1:2] + 0.114 * imgs[:, 2:3])
    x01 = x01[:, : spec.in_ch].contiguous()
    msgs = synthetic_msgs(n, spec.nbits, seed=seed)
    dd = torch.randn(n, spec.out_ch, S, S, generator=torch.Generator().manual_seed(seed)) * 1e-3
    names = [k for k, v in sd.items() if k.startswith("embedder.unet.") and v.dtype.is_floating_point and "running" not in k]
    # HIP
    model = make_model(spec, sd).train()
    eng = model._engine()
    xd = x01.cuda()
    key = eng.new_act("t.emb.in", n, S, S, spec.in_ch, 4)
    ymat = (C.c_float * 3)(1.0, 0.0, 0.0) if spec.in_ch == 1 else None
    N.check(eng.lib.vs_resize_pre(N.ptr(xd), n, spec.in_ch, S, S, S, S, 0, None, 1.0, 0.0, N.ptr(key.t), 1, ymat, N.stream()), "vs_resize_pre")
    eb = EmbedderBackward(model)
    delta, saved = eb.forward_keep(eng, key, _msgs_i32(msgs, eng.dev))
    grads = eb.backward(eng, saved, dd.cuda())
    torch.cuda.synchronize()
    # oracle: autograd through the functional U-Net with batch-statistics BatchNorm (and, masked, the HIP forward's ReLU decisions)
    sdg = {k: v.clone() for k, v in sd.items()}
    for k in names:
        sdg[k].requires_grad_(True)
    real_F = R.F
    try:
        if masked:
            R.F = _MaskedF(hip_relu_masks(model, saved))
        ref = R.embedder_forward(sdg, spec, x01, msgs, {})
        if masked:
            assert R.F.i == len(R.F.masks)
    finally:
        R.F = real_F
    ref.backward(dd)
    assert (delta.cpu() - ref.detach()).abs().max() < 2e-5
    errs = []
    for k in names:
        rf = sdg[k].grad
        if rf is None:
            continue
        assert k in grads, k
        got = grads[k].reshape(rf.shape).cpu()
        errs.append((float((got - rf).abs().max() / rf.abs().max().clamp_min(1e-12)), k))
    missing = [k for k in names if sdg[k].grad is not None and k not in grads]
    assert not missing, missing
    errs.sort(reverse=True)
    print(f"{'masked' if masked else 'free'}: worst relative gradient errors over {len(errs)} tensors: {[(round(e, 6), k) for e, k in errs[:4]]}; "
          f"median {errs[len(errs) // 2][0]:.2e}")
    return errs


def test_embedder_backward_tiny_matches_oracle_autograd():
    spec = tiny_spec()
    errs = _embedder_case(spec, make_state_dict(spec, seed=3), 3, 51)
    assert errs[0][0] < 2e-4, errs[:5]            # same ReLU decisions: what is left is fp32 arithmetic


def test_embedder_backward_vs10_matches_oracle_autograd():
    spec = spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml"))
    errs = _embedder_case(spec, make_state_dict(spec, seed=0), 2, 52)
    assert errs[0][0] < 5e-4, errs[:5]


def test_embedder_backward_unconstrained_within_the_relu_flip_noise():
    """without sharing the ReLU decisions the oracle itself moves by ~1 % (fp32 vs fp64 on the CPU): median and worst bounds of that order"""
    spec = tiny_spec()
    errs = _embedder_case(spec, make_state_dict(spec, seed=3), 3, 51, masked=False)
    assert errs[len(errs) // 2][0] < 1e-2 and errs[0][0] < 8e-2, errs[:5]


@pytest.mark.parametrize("rows,C,act", [(300, 16, "silu"), (77, 64, "silu"), (50, 128, "relu"), (9, 384, "silu"), (40, 24, "gelu")])
def test_rmsnorm_act_bwd_and_act_bwd(rows, C, act):
    """ChanRMSNorm + activation of the legacy U-Net (common.py:172-179: F.normalize(x, dim=1) * sqrt(C) * gamma, then the activation) and the
    plain activation derivative, against torch autograd"""
    L, st = N.lib(), N.stream()
    fn = {"silu": F.silu, "relu": F.relu, "gelu": F.gelu}[act]
    code = {"silu": N.ACT_SILU, "relu": N.ACT_RELU, "gelu": N.ACT_GELU}[act]
    g = torch.Generator().manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 1.5).cuda().requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).cuda().requires_grad_(True)
    dy = torch.randn(rows, C, generator=g).cuda()
    y = fn(F.normalize(x, dim=1) * (C ** 0.5) * gamma)
    y.backward(dy)
    xd, gd = x.detach().contiguous(), gamma.detach().contiguous()
    dx = torch.full((rows, C), 7.0, device="cuda")
    term = torch.full((rows, C), 7.0, device="cuda")
    N.check(L.vs_rmsnorm_act_bwd(N.ptr(xd), rows, C, C, N.ptr(gd), code, N.ptr(dy), C, N.ptr(dx), C, N.ptr(term), C, st), "vs_rmsnorm_act_bwd")
    assert (dx - x.grad).abs().max() <= 2e-5 * x.grad.abs().max()
    dg = term.double().sum(0)
    assert (dg - gamma.grad.double()).abs().max() <= 2e-5 * gamma.grad.abs().max()
    z = torch.randn(rows, C, generator=g).cuda().requires_grad_(True)
    fn(z).backward(dy)
    zd = z.detach().contiguous()
    dz = torch.full((rows, C), 7.0, device="cuda")
    N.check(L.vs_act_bwd(N.ptr(zd), C, N.ptr(dy), C, rows, C, code, N.ptr(dz), C, st), "vs_act_bwd")
    assert (dz - z.grad).abs().max() <= 2e-6 * z.grad.abs().max() + 1e-7


@pytest.mark.parametrize("rows,C,ld,act", [(37, 20, 20, "silu"), (301, 132, 160, "gelu"), (67, 1100, 1100, "relu")])
def test_rmsnorm_act_bwd_fp64_envelope(rows, C, ld, act):
    """vs_rmsnorm_act_bwd on hard rows (mean 30 and std 0.5: the projection g - n (n . g) removes the dominant common component; a constant
    row; a single 4e3 outlier that carries the norm alone; a row of magnitude 1e-3) against float64 autograd on the CPU, per row for dx and per
    channel for d gamma (the column sums of `term`, summed in float64 like the caller does).  The entry point requires C % 4 == 0: 18 and 130
    of the other envelope tests become 20 and 132.  The ReLU case has no ambiguous decision: the sign of u = n sqrt(C) gamma is the sign of
    x * gamma in any precision."""
    L, st = N.lib(), N.stream()
    fn = {"silu": F.silu, "relu": F.relu, "gelu": F.gelu}[act]
    code = {"silu": N.ACT_SILU, "relu": N.ACT_RELU, "gelu": N.ACT_GELU}[act]
    g = torch.Generator().manual_seed(62)
    x = hard_matrix(rows, C, 63, "rows")
    gamma, dy = 1 + 0.3 * torch.randn(C, generator=g), torch.randn(rows, C, generator=g)

    def autograd(dt):
        xx, gg = x.to(dt).requires_grad_(True), gamma.to(dt).requires_grad_(True)
        fn(F.normalize(xx, dim=1) * (C ** 0.5) * gg).backward(dy.to(dt))
        return xx.grad, gg.grad
    r64, r32 = cpu_autograd(autograd)
    xa, dya, gd = _padded(x.cuda(), ld), _padded(dy.cuda(), ld), gamma.cuda()
    dx = torch.full((rows, ld), 7.0, device="cuda")
    term = torch.full((rows, ld), 7.0, device="cuda")
    N.check(L.vs_rmsnorm_act_bwd(N.ptr(xa), rows, C, ld, N.ptr(gd), code, N.ptr(dya), ld, N.ptr(dx), ld, N.ptr(term), ld, st), "vs_rmsnorm_act_bwd")
    assert (dx[:, C:] == 0).all() and (term[:, C:] == 0).all()
    envelope(f"rmsnorm_act_bwd {act} rows={rows} C={C} ld={ld}", [
        ("dx/row", group_err(dx[:, :C], r64[0], 1), group_err(r32[0], r64[0], 1)),
        ("dgamma/ch", group_err(term[:, :C].double().sum(0), r64[1], None), group_err(r32[1], r64[1], None))])
