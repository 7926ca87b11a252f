"""The PatchGAN discriminator on the HIP path (csrc/disc.hip, videoseal_amd/discriminator.py, training.GeneratorStep / DiscriminatorStep) against
the float64 run of the unmodified reference (tests/golden/disc_ops.npz, disc_step.npz; tests/golden/make_golden_disc.py).

Tolerance.  The yardstick is the reference, never the code under test: per quantity the fixture holds `e`, what the reference's OWN float32 run
loses against its float64 run, in five measures (tests/_disc_util.errors).  The HIP result, compared with the same float64 values, gets
max(4 e, floor) with the floors of tests/test_gpu_ssim.py: 2e-7 absolute on a loss or statistic, 2e-5 of max |g| on a gradient element, 2e-5 of
the norm on an L2 error.  Derived, as there: |norm - norm64| <= L, the L2 bound of the whole tensor (triangle inequality; the sub-sample's bound
scaled by sqrt(n / n_sub)); sum and the +-1 projection: 4 x max(the reference's own error of that quantity, L).  Where the float64 gradient is
exactly 0 (max |g| = 0) the floors are taken relative to 1 / (B h w of the logit map).  The operator tests that need no fixture compare with
float64 torch on the host at the same floors.  With VS_DISC_PARITY_OUT=<file> the measured errors are written there (profiles/disc_parity.json
is such a run)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _disc_util as U
from tests._util import load_golden
from tests._guards import _guarded, _guards_intact

from videoseal_amd import native as N
from videoseal_amd.discriminator import GN_EPS, SLOPE, NLayerDiscriminator, disc_loss_raw, generator_disc_loss
from videoseal_amd.engine import Act, ConvW, pack_conv, pack_conv_bwd

pytestmark = pytest.mark.gpu

OPS = load_golden("disc_ops")
STEPS = load_golden("disc_step")
MEASURED = {}
GEMMS = ("f16x2", "f32", "bf16x3")        # the module's default, then the fp32 MFMA path and the exact 3 x bf16 split: there the error seen is the new kernels'


def _record(key, **kw):
    MEASURED.setdefault(key, {}).update({k: (float(v) if np.ndim(v) == 0 else [float(x) for x in v]) for k, v in kw.items()})
    path = os.environ.get("VS_DISC_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _bounds(stats, sub, e, zero_scale=0.0):
    n, gmax, nrm = stats[3], stats[5], stats[0]
    if n == 1:                                   # a loss or a statistic
        b = max(4 * e[0], 2e-7)
        return np.array([b, b, b, b, b])
    if gmax == 0.0:
        gmax, nrm = zero_scale, zero_scale * math.sqrt(n)
    nsub = math.sqrt(float((sub ** 2).sum())) if stats[5] > 0 else zero_scale * math.sqrt(sub.size)
    E, Ls = max(4 * e[0], 2e-5 * gmax), max(4 * e[1], 2e-5 * nsub)
    L = max(4 * e[1] * math.sqrt(n / sub.size), 4 * e[2], 2e-5 * nrm)
    return np.array([E, Ls, L, 4 * max(e[3], L), 4 * max(e[4], L)])


def _check(case_name, key, t, zero_scale=0.0, tag=""):
    sub, stats, e = OPS[f"{case_name}/{key}.sub"], OPS[f"{case_name}/{key}.stats"], OPS[f"{case_name}/{key}.e"]
    assert t.numel() == int(stats[3]), (key, tuple(t.shape), stats[3])
    err = U.errors(key, t, sub, stats)
    bound = _bounds(stats, sub, e, zero_scale)
    print(f"{case_name}{tag} {key}: err {err} reference fp32 {e} bound {bound}")
    _record(f"{case_name}{tag}/{key}", err=err, e_ref=e, bound=bound)
    assert (err <= bound).all(), (case_name, key, err.tolist(), bound.tolist())


def _host_check(what, got, ref64, scalar=False):
    """against a float64 host value at the floors alone"""
    got, ref64 = got.detach().double().cpu().flatten(), ref64.detach().double().cpu().flatten()
    d = got - ref64
    emax, el2 = float(d.abs().max()), float(d.norm())
    bmax = 2e-7 if scalar else 2e-5 * float(ref64.abs().max())
    bl2 = 2e-7 if scalar else 2e-5 * float(ref64.norm())
    print(f"{what}: max err {emax:.3e} (bound {bmax:.3e}), L2 err {el2:.3e} (bound {bl2:.3e})")
    _record(what, err=[emax, el2], bound=[bmax, bl2])
    assert emax <= bmax and el2 <= bl2, (what, emax, bmax, el2, bl2)


def _nhwc(x, ld):
    B, C, H, W = x.shape
    t = torch.zeros(B, H, W, ld)
    t[..., :C] = x.permute(0, 2, 3, 1)
    return t


def _disc(case, hinge_seed=None, gemm=NLayerDiscriminator.gemm):
    d = NLayerDiscriminator(input_nc=case[1], ndf=U.NDF, n_layers=case[0])
    d.load_state_dict(U.state_dict(case[0], case[1], hinge=hinge_seed is not None, hinge_seed=hinge_seed or 0), strict=True)
    d.gemm = gemm
    return d.cuda()


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("C,B,H,W", [(64, 2, 9, 13), (128, 3, 7, 10), (256, 2, 5, 11)])
def test_groupnorm_lrelu_forward_and_backward_between_red_zones(C, B, H, W):
    """vs_groupnorm_lrelu / _bwd with ld > C against float64 torch (group_norm + leaky_relu); every operand between poisoned guard areas, the outputs
    between sentinels.  H * W is no multiple of the 64-row chunk and more than one chunk; the affine parameters are random."""
    L, st = N.lib(), N.stream
    g = torch.Generator().manual_seed(C + H)
    ld = C + 4
    x = 1.5 * torch.randn(B, C, H, W, generator=g) + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(B, C, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yn = F.group_norm(xr, 4, gr, br, GN_EPS)
    assert float(yn.detach().abs().min()) > 1e-6, "a normalised value on the LeakyReLU kink: change the seed"
    yr = F.leaky_relu(yn, SLOPE)
    yr.backward(dy.double())
    nan = float("nan")
    xb, xd = _guarded(_nhwc(x, ld).cuda(), nan)
    db, dd = _guarded(_nhwc(dy, ld).cuda(), nan)
    gb, gd = _guarded(gamma.cuda(), nan)
    bb, bd = _guarded(beta.cuda(), nan)
    ob, od = _guarded(torch.full((B, H, W, ld), 7.0, device="cuda"), 5.0)
    dxb, dxd = _guarded(torch.full((B, H, W, ld), 7.0, device="cuda"), 5.0)
    mb, md = _guarded(torch.zeros(4 * B, device="cuda", dtype=torch.float64), 5.0)
    rb, rd = _guarded(torch.zeros(4 * B, device="cuda", dtype=torch.float64), 5.0)
    dgb, dgd = _guarded(torch.zeros(C, device="cuda"), 5.0)
    dbb, dbd = _guarded(torch.zeros(C, device="cuda"), 5.0)
    part = torch.empty(int(L.vs_groupnorm_partial_doubles(B, H * W, C)), device="cuda", dtype=torch.float64)
    N.check(L.vs_groupnorm_lrelu(N.ptr(xd), ld, B, H * W, C, 4, N.ptr(gd), N.ptr(bd), GN_EPS, SLOPE, N.ptr(part), N.ptr(md), N.ptr(rd), N.ptr(od), ld,
                                 st()), "vs_groupnorm_lrelu")
    N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(dd), ld, N.ptr(xd), ld, B, H * W, C, 4, N.ptr(gd), N.ptr(bd), N.ptr(md), N.ptr(rd), SLOPE, N.ptr(part),
                                     N.ptr(dxd), ld, N.ptr(dgd), N.ptr(dbd), st()), "vs_groupnorm_lrelu_bwd")
    torch.cuda.synchronize()
    for buf, fill in ((xb, nan), (db, nan), (gb, nan), (bb, nan), (ob, 5.0), (dxb, 5.0), (mb, 5.0), (rb, 5.0), (dgb, 5.0), (dbb, 5.0)):
        assert _guards_intact(buf, fill)
    assert bool((od[..., C:] == 0).all()) and bool((dxd[..., C:] == 0).all()), "pad columns are written as zeros"
    xg = x.double().view(B, 4, -1)
    _host_check(f"gn{C}.mean", md.view(B, 4), xg.mean(2))
    _host_check(f"gn{C}.rstd", rd.view(B, 4), 1 / torch.sqrt(xg.var(2, unbiased=False) + GN_EPS))
    _host_check(f"gn{C}.out", od[..., :C], yr.permute(0, 2, 3, 1))
    _host_check(f"gn{C}.dx", dxd[..., :C], xr.grad.permute(0, 2, 3, 1))
    _host_check(f"gn{C}.dgamma", dgd, gr.grad)
    _host_check(f"gn{C}.dbeta", dbd, br.grad)
    # the plain LeakyReLU form of layer 1
    N.check(L.vs_groupnorm_lrelu(N.ptr(xd), ld, B, H * W, C, 0, None, None, GN_EPS, SLOPE, None, None, None, N.ptr(od), ld, st()), "vs_groupnorm_lrelu")
    N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(dd), ld, N.ptr(xd), ld, B, H * W, C, 0, None, None, None, None, SLOPE, None, N.ptr(dxd), ld, None, None, st()),
            "vs_groupnorm_lrelu_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(ob, 5.0) and _guards_intact(dxb, 5.0)
    assert torch.equal(od[..., :C].cpu(), F.leaky_relu(x, SLOPE).permute(0, 2, 3, 1))
    assert torch.equal(dxd[..., :C].cpu(), (dy * torch.where(x > 0, 1.0, SLOPE)).permute(0, 2, 3, 1))


# every (input row stride, output channels) pair of the three configurations, each at both strides
WGRAD_PAIRS = [(4, 1, 32), (4, 3, 32), (32, 32, 64), (64, 64, 128), (128, 128, 256), (128, 128, 1), (256, 256, 1)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ld,ci,n", WGRAD_PAIRS)
def test_conv4x4_wgrad_matches_float64_autograd(ld, ci, n, stride):
    """vs_conv4x4_wgrad straight from the NHWC image against the float64 weight gradient of F.conv2d(padding=1): odd maps, a row count that is no
    multiple of the 16-pixel step, several pixel slices; operands between red zones; two runs are bit-identical"""
    L = N.lib()
    B, H, W = 3, 23, 19
    g = torch.Generator().manual_seed(ld * 7 + n + stride)
    x = torch.randn(B, ci, H, W, generator=g)
    Ho, Wo = (H - 2) // stride + 1, (W - 2) // stride + 1
    dy = torch.randn(B, n, Ho, Wo, generator=g)
    w = torch.zeros(n, ci, 4, 4, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, stride, 1).backward(dy.double())
    assert L.vs_conv4x4_wgrad_supported(n, ld, stride)
    nan = float("nan")
    dyl = 1 if n == 1 else n + 4
    xb, xd = _guarded(_nhwc(x, ld).cuda(), nan)
    yb, yd = _guarded((dy.permute(0, 2, 3, 1).contiguous() if n == 1 else _nhwc(dy, dyl)).cuda(), nan)
    part = torch.empty(int(L.vs_conv4x4_wgrad_partial_floats(n, ld, B, H, W, stride)), device="cuda")
    outs = []
    for _ in range(2):
        wb, wd = _guarded(torch.full((n, 16 * ld), 7.0, device="cuda"), 5.0)
        N.check(L.vs_conv4x4_wgrad(N.ptr(yd), dyl, n, N.ptr(xd), ld, B, H, W, stride, N.ptr(part), N.ptr(wd), N.stream()), "vs_conv4x4_wgrad")
        torch.cuda.synchronize()
        assert _guards_intact(wb, 5.0) and _guards_intact(xb, nan) and _guards_intact(yb, nan)
        outs.append(wd.clone())
    assert torch.equal(outs[0], outs[1])
    got = outs[0].view(n, 4, 4, ld)
    assert bool((got[..., ci:] == 0).all()), "pad channels of the image are zero, so are their gradients"
    _host_check(f"wgrad ld{ld} ci{ci} n{n} s{stride}", got[..., :ci].permute(0, 3, 1, 2), w.grad)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("ci,co,H,W", [(32, 64, 19, 25), (1, 32, 38, 50), (3, 32, 40, 56), (64, 128, 20, 28)])
def test_stride2_backward_data_is_the_adjoint_of_the_forward(ci, co, H, W, gemm):
    """<A x, y> = <x, A^T y> in double on the host to 1e-5 relative, with no reference at all: A = the stride-2 4 x 4 convolution (vs_conv_gemm),
    A^T = zero-dilated gradient + the same kernel on flipped weights with padding 2 (NLayerDiscriminator._bwd_data); odd and even maps"""
    d = NLayerDiscriminator(input_nc=3, ndf=32, n_layers=2)
    d.gemm = gemm
    d.cuda()
    eng = d.engine()
    g = torch.Generator().manual_seed(ci + H)
    B, ld = 2, (ci + 3) // 4 * 4
    x = torch.randn(B, ci, H, W, generator=g)
    w = (0.05 * torch.randn(co, ci, 4, 4, generator=g)).cuda()
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    y = torch.randn(B, co, Ho, Wo, generator=g)
    xa = Act(_nhwc(x, ld).cuda().flatten(), B, H, W, ci, ld)
    p, cp = pack_conv(w, ld)
    ax = Act(torch.empty(B * Ho * Wo * co, device="cuda"), B, Ho, Wo, co, co)
    eng.conv(xa, ConvW(p, None, co, 4, 4, cp), ax, stride=2, pad=1)
    ya = Act(_nhwc(y, co).cuda().flatten(), B, Ho, Wo, co, co)
    pb, cpb = pack_conv_bwd(w, co)
    aty = NLayerDiscriminator._bwd_data(eng, ya, ConvW(pb, None, ci, 4, 4, cpb), 2, H, W, ci, "t")
    torch.cuda.synchronize()
    lhs = float((ax.t.double().cpu().view(B, Ho, Wo, co) * y.double().permute(0, 2, 3, 1)).sum())
    rhs = float((aty.t.double().cpu().view(B, H, W, ld)[..., :ci] * x.double().permute(0, 2, 3, 1)).sum())
    scale = float(ax.t.double().norm().cpu()) * float(y.double().norm())
    print(f"adjoint {ci}->{co} {H}x{W} {gemm}: <Ax,y> {lhs:.9e} <x,ATy> {rhs:.9e} rel {abs(lhs - rhs) / scale:.2e}")
    _record(f"adjoint {ci}->{co} {H}x{W} {gemm}", err=abs(lhs - rhs) / scale, bound=1e-5)
    assert abs(lhs - rhs) <= 1e-5 * scale
    # and A itself against float64 conv2d: the pairing above cannot see an error that A and A^T share
    _host_check(f"conv s2 {ci}->{co} {H}x{W} {gemm}", ax.t.view(B, Ho, Wo, co), F.conv2d(x.double(), w.double().cpu(), None, 2, 1).permute(0, 2, 3, 1))


@pytest.mark.parametrize("input_nc", [1, 3])
def test_input_pass_and_its_adjoint(input_nc):
    L = N.lib()
    B, H, W = 2, 13, 21
    g = torch.Generator().manual_seed(input_nc)
    imgs = torch.rand(B, 3, H, W, generator=g)
    M = U.state_dict(2, 1)["rgb2yuv.M"]
    m0 = M[0].contiguous().cuda() if input_nc == 1 else None
    rb, rows = _guarded(torch.full((B, H, W, 4), 7.0, device="cuda"), 5.0)
    N.check(L.vs_disc_input(N.ptr(imgs.cuda()), B, H, W, N.ptr(m0), N.ptr(rows), N.stream()), "vs_disc_input")
    d = torch.randn(B, H, W, 4, generator=g)
    db, dimgs = _guarded(torch.full((B, 3, H, W), 7.0, device="cuda"), 5.0)
    N.check(L.vs_disc_input_bwd(N.ptr(d.cuda()), B, H, W, N.ptr(m0), N.ptr(dimgs), N.stream()), "vs_disc_input_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(rb, 5.0) and _guards_intact(db, 5.0)
    if input_nc == 1:
        y = torch.einsum("bchw,c->bhw", imgs.double(), M[0].double())
        _host_check("input y", rows[..., 0], y)
        assert bool((rows[..., 1:] == 0).all())
        _host_check("input y adjoint", dimgs, d[..., 0].double()[:, None] * M[0].double()[None, :, None, None])
    else:
        assert torch.equal(rows[..., :3].cpu(), imgs.permute(0, 2, 3, 1)) and bool((rows[..., 3] == 0).all())
        assert torch.equal(dimgs.cpu(), d[..., :3].permute(0, 3, 1, 2))


def test_disc_loss_values_gradients_and_masks():
    g = torch.Generator().manual_seed(3)
    real, fake = 1.5 * torch.randn(3, 1, 7, 9, generator=g), 1.5 * torch.randn(3, 1, 7, 9, generator=g) - 0.2
    rr, fr = real.double().requires_grad_(True), fake.double().requires_grad_(True)
    (0.5 * (F.relu(1 - rr).mean() + F.relu(1 + fr).mean())).backward()
    out, dr, df = disc_loss_raw(real.cuda(), fake.cuda(), hinge=True, gscale=0.25)
    ref = 0.5 * (F.relu(1 - real.double()).mean() + F.relu(1 + fake.double()).mean())
    _host_check("hinge loss", out[:3], torch.stack([ref, real.double().mean(), fake.double().mean()]), scalar=True)
    _host_check("hinge d real", dr, 0.25 * rr.grad)
    _host_check("hinge d fake", df, 0.25 * fr.grad)
    lf = fake.cuda().requires_grad_(True)
    loss = generator_disc_loss(lf)
    (3.0 * loss).backward()
    _host_check("generator term", loss, -fake.double().mean(), scalar=True)
    _host_check("generator term d fake", lf.grad, torch.full_like(fake, -3.0 / fake.numel()).double())


# ------------------------------------------------------------------------------------------------ network
def _acts(d, S):
    """fixture key -> tensor for every layer output of one forward (rows are NHWC, as the fixture stores them)"""
    out = {}
    for li, (ci, gi, _) in enumerate(d._plan):
        out[f"fwd.conv{ci}"] = S["layers"][li]["z"].t
        nxt = S["layers"][li + 1]["x"] if li + 1 < len(d._plan) else S["last_x"]
        out[f"fwd.act{ci + 1 if gi is None else gi + 1}"] = nxt.t
    return out


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("case", U.CASES, ids=U.case_name)
def test_network_matches_the_reference(case, gemm):
    name = U.case_name(case)
    meta = OPS["meta"]["cases"][name]
    tag = "" if gemm == NLayerDiscriminator.gemm else "@" + gemm
    real, fake, dl = U.frames(case, meta["seed"], 0), U.frames(case, meta["seed"], 1), U.dlogits(case)
    h, w = U.logit_hw(case)
    d = _disc(case, gemm=gemm)
    # forward: every layer's output, the logits
    with torch.cuda.device(0):
        logits, S = d._forward(real.cuda(), True)
    for k, t in _acts(d, S).items():
        _check(name, k, t, tag=tag)
    _check(name, f"fwd.conv{d._last}", logits, tag=tag)
    _check(name, "logits", logits, tag=tag)
    # a seeded d logits: d imgs and every parameter; two backward passes over one forward give identical results
    x = real.cuda().requires_grad_(True)
    lg = d(x)
    assert lg.grad_fn is not None and tuple(lg.shape) == (case[2], 1, h, w)
    lg.backward(dl.cuda(), retain_graph=True)
    first = {k: p.grad.clone() for k, p in d.named_parameters()}
    first_x = x.grad.clone()
    d.zero_grad(set_to_none=True)
    x.grad = None
    lg.backward(dl.cuda())
    assert torch.equal(first_x, x.grad) and all(torch.equal(first[k], p.grad) for k, p in d.named_parameters())
    _check(name, "rand.dimgs", x.grad, tag=tag)
    for k, p in d.named_parameters():
        _check(name, "rand.grad." + k, p.grad, tag=tag)
    # the generator term with every parameter frozen: d imgs only
    d.zero_grad(set_to_none=True)
    for p in d.parameters():
        p.requires_grad_(False)
    x = real.cuda().requires_grad_(True)
    loss = generator_disc_loss(d(x))
    loss.backward()
    assert [k for k, p in d.named_parameters() if p.grad is None] == meta["no_grad_gen"]
    _check(name, "gen.loss", loss, tag=tag)
    _check(name, "gen.dimgs", x.grad, tag=tag)
    # a mixed state: parameters with requires_grad = False receive None, the others their gradient
    for k, p in d.named_parameters():
        p.requires_grad_(k.endswith(".bias"))
    d(real.cuda()).backward(dl.cuda())
    for k, p in d.named_parameters():
        assert (p.grad is None) == (not k.endswith(".bias")), k
        if p.grad is not None:
            assert torch.equal(p.grad, first[k]), k


@pytest.mark.parametrize("case", U.CASES, ids=U.case_name)
def test_hinge_update_matches_the_reference(case):
    """real and fake frames as one batch of 2 B through the network with the scaled last layer (logits on both sides of +-1: both masks of the hinge
    loss are exercised), vs_disc_loss, one backward"""
    name = U.case_name(case)
    meta = OPS["meta"]["cases"][name]
    real, fake = U.frames(case, meta["seed"], 0), U.frames(case, meta["seed"], 1)
    h, w = U.logit_hw(case)
    B = case[2]
    d = _disc(case, hinge_seed=meta["hinge_seed"])
    logits = d(torch.cat([real, fake]).cuda())
    out, dr, df = disc_loss_raw(logits[:B], logits[B:], hinge=True)
    logits.backward(torch.cat([dr, df]))
    _check(name, "hinge.logits_real", logits[:B])
    _check(name, "hinge.logits_fake", logits[B:])
    _check(name, "hinge.loss", out[0])
    _check(name, "hinge.mean_real", out[1])
    _check(name, "hinge.mean_fake", out[2])
    for k, p in d.named_parameters():
        _check(name, "hinge.grad." + k, p.grad, zero_scale=1.0 / (B * h * w))


# ------------------------------------------------------------------------------------------------ the two training steps
def _step_setup(meta, monkeypatch):
    from oracle.inputs import synthetic_frames, synthetic_msgs
    from oracle.weights import make_state_dict, tiny_spec
    from tests._model import make_model
    from videoseal_amd import augmentation as G
    monkeypatch.setenv("VIDEOSEAL_CONV", "bf16x3")            # the embedder and the extractor on the exact split as well
    spec = tiny_spec()
    model = make_model(spec, make_state_dict(spec, seed=3))
    model.augmenter = G.Augmenter(masks={"kind": "none"}, augs={"identity": 1}, augs_params={}, num_augs=1)
    model.train()
    vid = meta["mode"] == "vid"
    if vid:
        model.step_size = meta["step"]
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"]).cuda()
    msgs = synthetic_msgs(1 if vid else meta["n"], spec.nbits, seed=meta["seed"])
    masks = torch.ones(meta["n"], 1, meta["h"], meta["w"]).cuda()
    disc = NLayerDiscriminator(input_nc=1, ndf=U.NDF, n_layers=2)
    disc.load_state_dict(U.state_dict(2, 1), strict=True)
    return model, disc.cuda(), imgs, msgs, masks, vid


def _check_step(name, meta, log, grads):
    for k, v in meta["log"].items():
        bound = max(4 * meta["log_e"][k], 2e-7)
        err = abs(float(log[k]) - v)
        print(f"{name} {k}: {float(log[k]):.9g} vs {v:.9g}: err {err:.3e} reference fp32 {meta['log_e'][k]:.3e} bound {bound:.3e}")
        _record(f"step/{name}/{k}", err=err, e_ref=meta["log_e"][k], bound=bound)
    names = [str(k) for k in STEPS[f"{name}/grad_names"]]
    stats, es = STEPS[f"{name}/grad_stats"], STEPS[f"{name}/grad_e"]
    assert sorted(grads) == sorted(names), sorted(set(grads) ^ set(names))[:6]
    worst, fails = 0.0, []
    for i, k in enumerate(names):
        _, got = U.summary(k, grads[k])
        n, nrm = stats[i][3], stats[i][0]
        L = max(4 * es[i][2], 4 * es[i][1] * math.sqrt(n / len(range(0, int(n), int(stats[i][4])))), 2e-5 * nrm)
        bound = np.array([L, 4 * max(es[i][3], L), 4 * max(es[i][4], L)])
        err = np.abs(got[:3] - stats[i][:3])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        if (err > bound).any():
            fails.append((k, err.tolist(), bound.tolist()))
    _record(f"step/{name}/grads", worst_err_over_bound=worst, tensors=len(names), failing=len(fails))
    print(f"{name}: worst gradient-summary error / bound {worst:.3f} over {len(names)} tensors")
    for k, v in meta["log"].items():
        assert abs(float(log[k]) - v) <= max(4 * meta["log_e"][k], 2e-7), (name, k, float(log[k]), v)
    assert not fails, fails[:4]


GEN_CASES = [k for k, m in STEPS["meta"]["cases"].items() if m["optimizer_idx"] == 0]
DISC_CASES = [k for k, m in STEPS["meta"]["cases"].items() if m["optimizer_idx"] == 1]


@pytest.mark.parametrize("name", GEN_CASES)
def test_generator_step_with_the_adversarial_term(name, monkeypatch):
    """Measured on an MI355X (profiles/disc_parity.json, keys step/*): see the figures there."""
    from videoseal_amd.training import GeneratorStep
    meta = STEPS["meta"]["cases"][name]
    model, disc, imgs, msgs, masks, vid = _step_setup(meta, monkeypatch)
    kw = meta["loss_kw"]
    step = GeneratorStep(model, percep_loss=kw["percep_loss"], percep_weight=kw["percep_weight"], decode_weight=kw["decode_weight"],
                         balanced=meta["balanced"], disc_weight=kw["disc_weight"], disc_start=meta["disc_start"], disc_num_layers=kw["disc_num_layers"],
                         disc_in_channels=kw["disc_in_channels"], discriminator=disc)
    torch.manual_seed(meta["torch_seed"])
    _, log, _ = step.step(imgs, masks, msgs, is_video=vid, global_step=meta["global_step"])
    assert list(log) == ["total_loss", "loss_percep", "loss_disc", "loss_decode", "scale_percep", "scale_disc", "scale_decode"]
    assert all(p.grad is None for p in disc.parameters()) and all(p.requires_grad for p in disc.parameters())
    if meta["global_step"] < meta["disc_start"]:
        assert float(log["scale_disc"]) == 0.0
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    first = {k: g.clone() for k, g in grads.items()}
    model.zero_grad(set_to_none=True)
    torch.manual_seed(meta["torch_seed"])
    step.step(imgs, masks, msgs, is_video=vid, global_step=meta["global_step"])
    assert all(torch.equal(first[k], p.grad) for k, p in model.named_parameters() if p.grad is not None), "the same step twice: bit-identical gradients"
    _check_step(name, meta, log, first)


@pytest.mark.parametrize("name", DISC_CASES)
def test_discriminator_step(name, monkeypatch):
    from videoseal_amd.training import DiscriminatorStep
    meta = STEPS["meta"]["cases"][name]
    model, disc, imgs, msgs, masks, vid = _step_setup(meta, monkeypatch)
    torch.manual_seed(meta["torch_seed"])
    outputs = model(imgs, masks, msgs, is_video=vid)
    step = DiscriminatorStep(disc, disc_start=meta["disc_start"])
    d_loss, log = step.step(imgs, outputs["imgs_w"], global_step=meta["global_step"])
    assert list(log) == ["disc_loss", "disc_factor", "logits_real", "logits_fake"]
    assert all(p.grad is None for p in model.parameters()), "the discriminator step leaves the embedder and the detector untouched"
    if meta["global_step"] < meta["disc_start"]:
        assert log["disc_factor"] == 0.0 and float(d_loss) == 0.0
    first = {"disc." + k: p.grad.clone() for k, p in disc.named_parameters()}
    disc.zero_grad(set_to_none=True)
    step.step(imgs, outputs["imgs_w"], global_step=meta["global_step"])
    assert all(torch.equal(first["disc." + k], p.grad) for k, p in disc.named_parameters())
    _check_step(name, meta, log, first)
