"""fp64 envelopes of the LOSS AND DISCRIMINATOR kernels (csrc/ssim.hip: vs_ssim_stats, vs_ssim_grad, vs_avgpool2_pad, vs_jnd_loss / _grad;
csrc/bwd_shell.hip: vs_percep_mse / _grad; csrc/bwd_ops.hip: vs_bce_logits; csrc/pixel_head.hip: vs_pixel_bce; csrc/disc.hip: vs_disc_loss,
vs_groupnorm_lrelu / _bwd, vs_conv4x4_wgrad, vs_conv4x4_n1 / _bwd / _bias_grad, vs_disc_input / _bwd): formulas, hard frame pairs, logits and
activations, cases, the metric and the margin shared by tests/test_loss_contract_cpu.py (the envelope has teeth; no GPU) and
tests/test_gpu_loss_envelope.py (every kernel against it).

As in tests/_img_bwd_ref.py: every formula is written from the reference's definition (losses/ssim.py, losses/perceptual.py, losses/yuvloss.py,
losses/jndloss.py, losses/videosealloss.py, modules/discriminator.py) and takes its dtype as a parameter; the reference is the formula in float64
on the CPU from the same fp32 values the kernel receives, gradients by float64 autograd; the yardstick is the same formula (and the same autograd)
in float32 on one thread.  The SSIM yardstick is the reference's own unshifted E[x^2] - mu^2: it restates nothing of the code under test.
One line per (case, kind, quantity), so that noise's larger yardstick cannot hide a structured kind:
  tensors   max |got - ref64| / max(max |ref64|, tiny)                                    (_envelope.frame_err)
  scalars   max over the values of |got - ref64| / max(|ref64|, tiny)                     (losses, per-plane statistics, group statistics)
  zeros     where the exact result is zero (gradients of an identical pair, of inactive hinge terms, mse of identical frames): if the float32
            formula gives exact zeros too the kernel must (the line says `=0`), else both absolute errors are divided by max |g64| of the same
            shape's `noise` kind (the line says `/noise`)
  means     a mean or sum of signed terms (the logit means and -mean(fake) of vs_disc_loss, the bias gradient) can cancel to nothing, where an
            error relative to the result is 100 % for any answer: both absolute errors over the mean (summed) magnitude of the terms (`/mag`)
A kernel may exceed the yardstick by LOSS_FP64_MARGIN."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import _img_bwd_ref as B
from tests._envelope import TINY, check_rows, frame_err, one_thread

# Twice the largest ratio hip / max(yardstick, 2^-24) measured on an MI355X over every line of tests/test_gpu_loss_envelope.py
# (profiles/loss_fp64_envelope.txt lists them), never more than 8: a kernel that needs more has a defect.
LOSS_FP64_MARGIN = 5.008       # 2 x 2.504, the largest ratio measured: vs_ssim_stats, mean SSIM of a plane on 11 x 11 (a 1 x 1 map), `dark` (1391 lines)
F32, F64 = torch.float32, torch.float64
envelope = functools.partial(check_rows, "LOSS-ENVELOPE", 58, "cpu-fp32", LOSS_FP64_MARGIN)

SLOPE, GN_EPS = 0.2, 1e-5      # modules/discriminator.py: LeakyReLU(0.2), GroupNorm's default eps
K1, K2 = 0.01, 0.03            # losses/ssim.py:68
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)          # losses/ssim.py:223
Y_ROW = (0.299, 0.587, 0.114)  # row 0 of the rgb2yuv matrix (data/transforms.py:46)


# ------------------------------------------------------------------------------------------------------------------------ metric
def scalar_err(got, ref):
    """max over the values of |got - ref64| / max(|ref64|, tiny)"""
    got, ref = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / ref.abs().clamp_min(TINY)).max())


def line(name, got, r64, y32, scale=None, zero=False, scalar=False, mag=None):
    """one envelope row (name, error of `got`, error of the yardstick `y32`).  zero: the exact result is zero although float64 autograd leaves
    rounding residue; an all-zero r64 is treated the same; scale: max |g64| of the same shape's `noise` kind.  mag: for a mean or sum of signed
    terms, which may cancel to nothing (an error relative to it would be 100 % for any answer): both absolute errors divided by `mag`, the mean
    (or summed) magnitude of the terms; the line says `/mag`"""
    got, r64, y32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, y32))
    if mag is not None:
        assert mag > 0, name
        return (name + " /mag", float((got - r64).abs().max()) / mag, float((y32 - r64).abs().max()) / mag)
    if zero or not r64.any():
        if not y32.any():
            return (name + " =0", 0.0 if not got.any() else math.inf, 0.0)
        assert scale is not None and scale > 0, name
        return (name + " /noise", float((got - r64).abs().max()) / scale, float((y32 - r64).abs().max()) / scale)
    err = scalar_err if scalar else frame_err
    return (name, err(got, r64), err(y32, r64))


def grads_of(fn, ts, dt, up=None):
    """d <fn(*ts in dt), up> / d ts by autograd; the float32 yardstick on one thread (its summation order must not depend on the host)"""
    def run():
        tl = [t.detach().to(dt).requires_grad_(True) for t in ts]
        return torch.autograd.grad(fn(*tl), tl, None if up is None else up.to(dt))
    return run() if dt == F64 else one_thread(run)


def grad_of(fn, t, dt, up=None):
    return grads_of(fn, (t,), dt, up)[0]


# ------------------------------------------------------------------------------------------------------------------------ hard inputs
PAIR_KINDS = ("noise", "dark", "dark-bars", "white", "flat", "checker", "inverse", "ramp", "impulse", "identical")


def hard_pairs(H, W, Fn=2):
    """{kind: (x, y)} [Fn, 3, H, W] float32 in [0, 1], fixed seeds.  noise: uniform, y = x + 0.05 randn; dark: x = 0, y = |2e-3 randn|; dark-bars:
    noise whose rows [: H / 4] and [-H / 4 :] are exactly 0, y = x + 2e-3 randn; white: x = 1, y = 1 - |1e-3 randn|; flat: 0.75 and
    0.75 + 1e-3 randn; checker: the 0 / 1 checkerboard, y = x + 0.01 randn; inverse: checkerboard and 1 - x (SSIM ~ -1: the relu gate of
    MS-SSIM); ramp: horizontal 0 -> 1, y = x + 1e-3 randn; impulse: the lattice of _img_bwd_ref.hard_dy (halved: the plane factors stay below 1)
    against 0; identical: noise and itself, bit for bit (the exact gradient is 0).  Every y is clamped to [0, 1]."""
    g = torch.Generator().manual_seed(4100 + 131 * H + W)
    shape = (Fn, 3, H, W)
    rn = lambda s: s * torch.randn(shape, generator=g)          # noqa: E731
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    noise = torch.rand(shape, generator=g)
    out = {"noise": (noise, noise + rn(0.05))}
    out["dark"] = (torch.zeros(shape), rn(2e-3).abs())
    bars = torch.rand(shape, generator=g)
    bars[:, :, : H // 4] = 0.0
    bars[:, :, H - H // 4:] = 0.0
    out["dark-bars"] = (bars, bars + rn(2e-3))
    out["white"] = (torch.ones(shape), 1 - rn(1e-3).abs())
    out["flat"] = (torch.full(shape, 0.75), 0.75 + rn(1e-3))
    ck = ((yy + xx) % 2).float().expand(shape).contiguous()
    out["checker"] = (ck, ck + rn(0.01))
    out["inverse"] = (ck, 1 - ck)
    ramp = (xx.float() / max(W - 1, 1)).expand(shape).contiguous()
    out["ramp"] = (ramp, ramp + rn(1e-3))
    out["impulse"] = (0.5 * B.hard_dy(shape)["impulse"], torch.zeros(shape))
    ident = torch.rand(shape, generator=g)
    out["identical"] = (ident, ident.clone())
    assert tuple(out) == PAIR_KINDS
    return {k: (x.contiguous(), y.clamp(0, 1).contiguous()) for k, (x, y) in out.items()}


LOGIT_KINDS = ("noise", "kink", "large", "one-sided")
LARGE = (0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)


def hard_logits(shape, seed=0):
    """{kind: float32 `shape`}.  noise: 1.5 randn; kink: a third of the elements exactly +1, a third exactly -1, the rest 1 or 2 ulp beside
    +-1 on either side (the hinge gates 1 - real > 0 and 1 + fake > 0 at and around their kink); large: the values of LARGE in turn (exp
    overflows beyond 88, sigmoid saturates beyond 17, 1e-8 is below the ulp of log 2); one-sided: 1.5 + |randn| (as `real`, and negated as
    `fake`, every hinge term is inactive: loss and gradients are exactly 0)"""
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator().manual_seed(5200 + 7 * n + seed)
    one = torch.ones(())
    up1, dn1 = torch.nextafter(one, 2 * one), torch.nextafter(one, 0 * one)
    near = torch.stack([up1, torch.nextafter(up1, 2 * one), dn1, torch.nextafter(dn1, 0 * one)])
    i = torch.arange(n)
    kink = torch.where(i % 3 == 0, one, torch.where(i % 3 == 1, -one, near[(i // 3) % 4] * (1 - 2 * ((i // 12) % 2)).float()))
    out = {"noise": 1.5 * torch.randn(n, generator=g), "kink": kink[torch.randperm(n, generator=g)] if n > 2 else kink,
           "large": torch.tensor(LARGE)[(i + seed) % len(LARGE)], "one-sided": 1.5 + torch.randn(n, generator=g).abs()}
    return {k: v.reshape(shape).contiguous() for k, v in out.items()}


def hard_msgs(rows, k, seed=0):
    """[rows, k] int32 message bits"""
    g = torch.Generator().manual_seed(5300 + 17 * rows + k + seed)
    return torch.randint(0, 2, (rows, k), generator=g, dtype=torch.int32)


SUBNORMAL = 2.0 ** -149
ZERO_VALUES = (0.0, -0.0, SUBNORMAL, -SUBNORMAL)


def hard_acts(Bn, C, H, W, groups, seed=0):
    """{kind: [Bn, C, H, W] float32}.  groups = 4: `noise` (1.5 randn + 0.3) and `groups`, the group analogue of _envelope.hard_matrix: every
    (frame, group of C / 4 channels) has mean 30 and std 0.5, except, in frame f, group (f + 1) % 4: constant 30.25 (variance exactly 0), group
    (f + 2) % 4: one 4e3 outlier, group (f + 3) % 4: magnitude 1e-3.  A channel count below 4 has fewer groups (the convolution inputs).
    groups = 0 (the plain LeakyReLU form): `noise` and `zeros`: noise with 0.0, -0.0, 2^-149 and -2^-149 at the flat positions 4 j + (0, 1, 2, 3)
    for j % 5 == 0"""
    g = torch.Generator().manual_seed(6100 + 131 * C + 7 * H + W + seed)
    out = {"noise": 1.5 * torch.randn(Bn, C, H, W, generator=g) + 0.3}
    if groups:
        x = 30.0 + 0.5 * torch.randn(Bn, C, H, W, generator=g)
        grp = (torch.arange(C) * 4) // C
        for f in range(Bn):
            c0 = grp == (f + 1) % 4
            x[f, c0] = 30.25
            c1 = (grp == (f + 2) % 4).nonzero().flatten()
            if len(c1):
                x[f, c1[len(c1) // 2], H // 2, W // 2] = 4e3
            c2 = grp == (f + 3) % 4
            x[f, c2] = 1e-3 * torch.randn(int(c2.sum()), H, W, generator=g)
        out["groups"] = x
    else:
        z = out["noise"].clone().flatten()
        for j in range(0, z.numel() // 4, 5):
            z[4 * j: 4 * j + 4] = torch.tensor(ZERO_VALUES)
        out["zeros"] = z.view(Bn, C, H, W)
    return out


def nhwc(x, ld):
    """[B, C, H, W] -> the rows [B, H, W, ld] a kernel reads, pad columns zero"""
    Bn, C, H, W = x.shape
    t = torch.zeros(Bn, H, W, ld, dtype=x.dtype)
    t[..., :C] = x.permute(0, 2, 3, 1)
    return t


# ------------------------------------------------------------------------------------------------------------------------ SSIM / MS-SSIM
# (H, W) of the P = 2 x 3 planes.  csrc/ssim.hip: a workgroup holds NT = 128 map columns (statistics) or GRAD_TW = 118 gradient columns (adjoint);
# rows per chunk: pick_rows halves STATS_ROWS = 96 / GRAD_ROWS = 128 down to STATS_ROWS_MIN = 24 / GRAD_ROWS_MIN = 32 while strips * P * chunks < 1024,
# which at P = 6 holds for every frame below some 8000 rows: every case of SSIM_SHAPES runs with rows = 24 / 32.  The un-halved counts need
# strips * P * chunks >= 1024: SSIM_MANY_PLANES reaches them with 513 narrow planes instead of a frame no test could afford.
SSIM_MANY_PLANES = (171, 139, 11)          # (F, H, W): one strip; 129 map rows = 96 + 33, 139 gradient rows = 128 + 11: 513 * 1 * 2 = 1026 workgroups at the full counts
SSIM_SHAPES = [
    (11, 11),          # a 1 x 1 map
    (11, 257),         # one map row; 247 map columns: two strips, the second short
    (59, 11),          # one map column; 49 map rows: three chunks of 24, the last a single row
    (35, 138),         # the map's 128th column is the last: exactly one strip of NT; H - 10 = 25: one row past STATS_ROWS_MIN
    (35, 139),         # the map's 129th column: a second strip of one column
    (33, 118),         # exactly one GRAD_TW strip, GRAD_ROWS_MIN + 1 rows: a second chunk of one gradient row
    (65, 119),         # the 119th gradient column: a second strip of one column; three chunks of 32 rows
    (97, 150),         # several chunks of both kernels at once (87 map rows: 4 chunks; 97 gradient rows: 4 chunks), two strips of both
]
MS_SHAPES = [(161, 163), (176, 162)]          # levels 161 -> 81 -> 41 -> 21 -> 11 (a 1 x 1 map, every level odd: every pooling pads); even / mixed
MS_KINDS = ("noise", "dark-bars", "flat", "inverse")


def win11(dt):
    """losses/ssim.py:16-30: the 11-tap window, sigma 1.5, built in fp32 and cast"""
    c = torch.arange(11, dtype=F32) - 11 // 2
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dt)


def _filt(t, w):
    """gaussian_filter (losses/ssim.py:33-59): 'valid', per channel, along H first, then along W"""
    C = t.shape[1]
    k = w.view(1, 1, 1, 11).repeat(C, 1, 1, 1)
    return F.conv2d(F.conv2d(t, k.transpose(2, 3), groups=C), k, groups=C)


def ssim_stats(x, y, dt, shift=None):
    """(mean SSIM map, mean contrast-structure map) [F, C] of losses/ssim.py:82-107, data_range 1.  DEFECT: shift = c: the variances from the
    moments of x - c, with the terms the window's sum (1 - 1e-8) leaves behind restored -- the same function in exact arithmetic"""
    X, Y, w = x.to(dt), y.to(dt), win11(dt)
    C1, C2 = K1 ** 2, K2 ** 2
    mu1, mu2 = _filt(X, w), _filt(Y, w)
    if shift is None:
        s1, s2, s12 = _filt(X * X, w) - mu1.pow(2), _filt(Y * Y, w) - mu2.pow(2), _filt(X * Y, w) - mu1 * mu2
    else:
        S = float(win11(F32).double().sum()) ** 2
        c, k1, k2 = (torch.tensor(v, dtype=F64).to(dt) for v in (shift, shift * (1 - S), shift * shift * S * (1 - S)))
        Xs, Ys = X - c, Y - c
        m1, m2 = _filt(Xs, w), _filt(Ys, w)
        s1 = (_filt(Xs * Xs, w) - m1 * m1) + (2 * k1 * m1 + k2)
        s2 = (_filt(Ys * Ys, w) - m2 * m2) + (2 * k1 * m2 + k2)
        s12 = (_filt(Xs * Ys, w) - m1 * m2) + (k1 * (m1 + m2) + k2)
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ss = ((2 * mu1 * mu2 + C1) / (mu1.pow(2) + mu2.pow(2) + C1)) * cs
    return ss.flatten(2).mean(-1), cs.flatten(2).mean(-1)


def pool2(t):
    """losses/ssim.py:237-238: avg_pool2d(2, padding = side % 2), the padded zeros counted"""
    return F.avg_pool2d(t, kernel_size=2, padding=[s % 2 for s in t.shape[2:]])


def ssim_target(x, y, g_ssim, g_cs, g_coarse, dt, shift=None):
    """sum_p (g_ssim[p] mean SSIM_p + g_cs[p] mean cs_p) [+ <g_coarse, pool2(y)>]: what vs_ssim_grad differentiates with respect to y"""
    s, c = ssim_stats(x, y, dt, shift)
    T = (g_ssim.to(dt).view_as(s) * s).sum() + (g_cs.to(dt).view_as(c) * c).sum()
    if g_coarse is None:
        return T
    pooled = pool2(y.to(dt))
    return T + (g_coarse.to(dt).view_as(pooled) * pooled).sum()


def ssim_loss(x, y, dt, shift=None):
    """losses/ssim.py:282-291: -mean over frames and channels"""
    return -ssim_stats(x, y, dt, shift)[0].mean()


def msssim_loss(x, y, dt, relu=True):
    """losses/ssim.py:230-246, 325-334: -mean(prod_l relu(f_l) ^ w_l), f = cs at the first four levels, SSIM at the fifth.  DEFECT: relu = False"""
    gate = torch.relu if relu else (lambda t: t)
    X, Y = x.to(dt), y.to(dt)
    f = []
    for lv in range(len(MS_WEIGHTS)):
        s, c = ssim_stats(X, Y, dt)
        if lv < len(MS_WEIGHTS) - 1:
            f.append(gate(c))
            X, Y = pool2(X), pool2(Y)
    f.append(gate(s))
    wts = torch.tensor(MS_WEIGHTS, dtype=dt)
    return -torch.prod(torch.stack(f, 0) ** wts.view(-1, 1, 1), dim=0).mean()


def ssim_coeffs(H, W, P=6):
    """(g_ssim [P], g_cs [P], g_coarse [P, ceil(H / 2), ceil(W / 2)]) float32: the random upstream gradients of vs_ssim_grad"""
    g = torch.Generator().manual_seed(4300 + 131 * H + W)
    return (torch.rand(P, generator=g) - 0.5, torch.rand(P, generator=g) - 0.5, torch.rand(P, (H + 1) // 2, (W + 1) // 2, generator=g) - 0.5)


# ------------------------------------------------------------------------------------------------------------------------ mse / yuv / jnd
PERCEP_SHAPES = [(2, 23, 141), (1, 5, 7)]          # (F, H, W): an odd plane wider than a wave; one tiny frame


def percep(x, y, yuv, dt):
    """losses/perceptual.py:20-28, yuvloss.py:11-27: mean((T (y - x))^2)"""
    return B.percep(x, y, yuv, dt)


def jnd_loss(x, y, hm, dt):
    """losses/jndloss.py:27-31: mean((|y - x| - h)^2), the heat-map h [F, 1, H, W] passed in (broadcast over the channels)"""
    e = (y.to(dt) - x.to(dt)).abs() - hm.to(dt)
    return one_thread(lambda: (e * e).mean())


def jnd_grad32(x, y, hm, sign0=0.0):
    """fp32 closed form 2 (|d| - h) sign(d) / N.  DEFECT: sign0 = 1 (torch's abs has derivative 0 at 0, and clamped or identical pixels give d = 0)"""
    d = y - x
    sg = torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, sign0))
    return torch.tensor(2.0 / d.numel(), dtype=F32) * (d.abs() - hm) * sg


# ------------------------------------------------------------------------------------------------------------------------ decoding losses
BCE_SHAPES = [(3, 16), (300, 7), (1, 1)]          # (B, k): more rows than the 256 threads of the one workgroup; a single logit
BCE_TEMPS = (0.1, 1.0, 10.0)
PIXEL_BCE_SHAPES = [(3, 5, 7 * 9), (2, 3, 16 * 20)]          # (B, K, HW): HW % 4 != 0 (the scalar kernel) and HW % 4 == 0 (16-byte stores), > 256 pixels


def _bce(z, t):
    return F.binary_cross_entropy_with_logits(z, t, reduction="none")


def bce_logits(preds, msgs, temperature, dt):
    """videosealloss.py:147-153: BCE-with-logits of preds[:, 1:] / T against the bits, mean over B k; msgs [1 | B, k]"""
    z = preds.to(dt)[:, 1:] / temperature
    return one_thread(lambda: _bce(z, msgs.to(dt).expand_as(z)).mean())


def bce_grad32(preds, msgs, temperature, unstable=False):
    """fp32 closed form (sigmoid(z) - m) / (T B k), column 0 zero.  unstable: for m = 1 as -(1 - sigmoid(z)) -- in fp32 the same number:
    sigmoid(20) is already 1.0, and autograd's own sigmoid(z) - m is no better, so the `large` kind cannot tell them apart (see the contract test)"""
    z = preds[:, 1:] / temperature
    m = msgs.float().expand_as(z)
    sg = torch.sigmoid(z)
    d = torch.where(m > 0, -(1 - sg), sg) if unstable else sg - m
    g = torch.zeros_like(preds)
    g[:, 1:] = d / (temperature * z.numel())
    return g


def pixel_masks(Bn, HW, seed=0):
    """[Bn, HW] float32 0 / 1: frame 0 selects a single pixel, frame 1 everything, any further frame a random half"""
    g = torch.Generator().manual_seed(5400 + HW + seed)
    m = (torch.rand(Bn, HW, generator=g) < 0.5).float()
    m[0] = 0.0
    m[0, HW // 3] = 1.0
    if Bn > 1:
        m[1] = 1.0
    return m


def pixel_bce(preds, masks, msgs, temperature, dt):
    """(detection, decoding) of videosealloss.py:137-167 on preds [B, K, HW]: mean BCE-with-logits of channel 0 against the mask; mean over the
    selected pixels (mask != 0) and the K - 1 bits of BCE-with-logits of channels 1.. / T against the bits"""
    p, m = preds.to(dt), masks.to(dt)

    def run():
        det = _bce(p[:, 0], m).mean()
        z = p[:, 1:] / temperature
        t = msgs.to(dt).expand(p.shape[0], -1)[:, :, None].expand_as(z)
        sel = (masks != 0)[:, None].expand_as(z)
        return det, (_bce(z, t) * sel).sum() / sel.sum()
    return one_thread(run)


# ------------------------------------------------------------------------------------------------------------------------ discriminator loss
def disc_loss(real, fake, hinge, dt):
    """(loss, mean real, mean fake): videosealloss.py:16-23 (hinge) or :134 (-mean(fake), the generator's term; real may be None)"""
    f = fake.to(dt)
    r = real.to(dt) if real is not None else None

    def run():
        loss = 0.5 * (torch.mean(F.relu(1.0 - r)) + torch.mean(F.relu(1.0 + f))) if hinge else -f.mean()
        return loss, (r.mean() if r is not None and r.numel() else torch.zeros((), dtype=dt)), f.mean()
    return one_thread(run)


def hinge_grads32(real, fake, gscale, ge=False):
    """fp32 closed form of gscale * d hinge: -0.5 gscale / n_r where 1 - real > 0, 0.5 gscale / n_f where 1 + fake > 0.  DEFECT: ge = `>=`"""
    on = (lambda t: t >= 0) if ge else (lambda t: t > 0)
    gr, gf = torch.tensor(-0.5 * gscale / real.numel(), dtype=F32), torch.tensor(0.5 * gscale / fake.numel(), dtype=F32)
    return torch.where(on(1 - real), gr, 0.0), torch.where(on(1 + fake), gf, 0.0)


# ------------------------------------------------------------------------------------------------------------------------ GroupNorm + LeakyReLU
GN_CASES = [(64, 2, 9, 13), (256, 2, 5, 11), (16, 1, 3, 23)]          # (C, B, H, W), all with ld = C + 4: two 64-row chunks with a tail; one chunk; C / 4 = 4


def gn_params(C):
    g = torch.Generator().manual_seed(6200 + C)
    return 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g) + 0.05


def gn_pre(x, gamma, beta, dt):
    """GroupNorm(4, C) (biased variance, eps 1e-5) with its affine, before the LeakyReLU"""
    return F.group_norm(x.to(dt), 4, gamma.to(dt), beta.to(dt), GN_EPS)


def gn_lrelu(x, gamma, beta, groups, dt):
    """modules/discriminator.py:118-132: GroupNorm(4, C) + LeakyReLU(0.2); groups = 0: the plain LeakyReLU of the first layer"""
    return F.leaky_relu(gn_pre(x, gamma, beta, dt) if groups else x.to(dt), SLOPE)


def gn_stats(x, dt):
    """(mean, 1 / sqrt(biased variance + eps)) [B, 4]"""
    xg = x.to(dt).reshape(x.shape[0], 4, -1)
    return one_thread(lambda: (xg.mean(2), 1 / torch.sqrt(xg.var(2, unbiased=False) + GN_EPS)))


def gn_lrelu32(x, gamma, beta, naive_var=False):
    """fp32 restatement (mean, rstd, out).  DEFECT: naive_var = the variance as E[x^2] - mean^2 in fp32"""
    Bn, C = x.shape[:2]
    xg = x.reshape(Bn, 4, -1)

    def run():
        m = xg.mean(2, keepdim=True)
        var = ((xg * xg).mean(2, keepdim=True) - m * m).clamp_min(0) if naive_var else xg.var(2, unbiased=False, keepdim=True)
        rs = 1 / torch.sqrt(var + GN_EPS)
        y = ((xg - m) * rs).view_as(x) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
        return m[..., 0], rs[..., 0], F.leaky_relu(y, SLOPE)
    return one_thread(run)


def lrelu_bwd32(x, dy, at_zero=SLOPE):
    """dy * (x > 0 ? 1 : slope).  DEFECT: at_zero = 1 (derivative 1 at exactly 0)"""
    return dy * torch.where(x > 0, 1.0, torch.where(x == 0, at_zero, SLOPE))


# ------------------------------------------------------------------------------------------------------------------------ 4 x 4 convolutions
# every (input row stride, input channels, output channels) of the three configurations (WGRAD_PAIRS of tests/test_gpu_disc.py)
WGRAD_PAIRS = [(4, 1, 32), (4, 3, 32), (32, 32, 64), (64, 64, 128), (128, 128, 256), (128, 128, 1), (256, 256, 1)]
WGRAD_MAPS = [(3, 23, 19), (2, 4, 5)]          # (B, H, W): odd maps, several pixel slices, no multiple of the 16-pixel step; less than one step
N1_LDS = (128, 256)
N1_MAPS = [(2, 6, 7), (1, 2, 2)]               # (B, H, W): 60 logits; a single logit whose 4 x 4 window hangs over every edge
BIAS_MAPS = [(2, 5, 6), (1, 1, 1), (3, 23, 19)]          # the logits of the two maps, and odd planes beyond the 256 threads (a checkerboard plane sums to one element)


def conv4x4(x, w, bias, stride, dt):
    """modules/discriminator.py:107-137: Conv2d(kernel 4, stride, padding 1)"""
    return one_thread(lambda: F.conv2d(x.to(dt), w.to(dt), None if bias is None else bias.to(dt), stride, 1))


def conv_out(H, W, stride):
    return (H - 2) // stride + 1, (W - 2) // stride + 1


def conv_wgrad(x, dy, n, stride, dt, drop_last_row=False):
    """d <conv4x4(x, w), dy> / d w [n, ci, 4, 4] by autograd.  DEFECT: drop_last_row = without the last output row"""
    if drop_last_row:
        dy = dy.clone()
        dy[:, :, -1] = 0.0
    return grad_of(lambda w: conv4x4(x, w, None, stride, dt), torch.zeros(n, x.shape[1], 4, 4), dt, dy)


def conv_weights(n, ci, seed=0):
    g = torch.Generator().manual_seed(6300 + 131 * n + ci + seed)
    return 0.05 * torch.randn(n, ci, 4, 4, generator=g)


def taps_first(w, ld):
    """[n, ci, 4, 4] -> [n, 16 * ld] in the kernels' (tap, channel) order, pad channels zero"""
    n, ci = w.shape[:2]
    t = torch.zeros(n, 4, 4, ld, dtype=w.dtype)
    t[..., :ci] = w.permute(0, 2, 3, 1)
    return t.reshape(n, 16 * ld)


def bias_dy(shape, kind):
    """the upstream gradient of the last layer's bias, flat: a kind of hard_dy on the logit map, times 0.1 (non-dyadic: a sum in fp32 rounds)"""
    return (B.hard_dy(shape)[kind].flatten() * torch.tensor(0.1, dtype=F32)).contiguous()


def bias_grad(dy, dt):
    return one_thread(lambda: dy.to(dt).sum())


def bias_grad_cancelling32(dy):
    """DEFECT: every positive element first, then every negative one, one running fp32 sum (element by element: ATen's cumsum is no such sum)"""
    s = torch.zeros((), dtype=F32)
    for v in torch.cat([dy[dy > 0], dy[dy <= 0]]):
        s = s + v
    return s


# ------------------------------------------------------------------------------------------------------------------------ discriminator input
DISC_INPUT_SHAPE = (13, 21)


def disc_input(imgs, input_nc, dt):
    """modules/discriminator.py:146-147 as rows [B, H, W, 4]: (r, g, b, 0), or (Y, 0, 0, 0) with Y = 0.299 r + 0.587 g + 0.114 b"""
    x = imgs.to(dt).permute(0, 2, 3, 1)
    if input_nc == 1:
        x = (x * torch.tensor(Y_ROW, dtype=F32).to(dt)).sum(-1, keepdim=True)
    return F.pad(x, (0, 4 - x.shape[-1]))
