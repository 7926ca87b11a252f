"""fp64 envelopes of the small fp32 kernels that hold the U-Net and the extractor head together (csrc/net_ops.hip, csrc/bwd_unet.hip, parts of
csrc/bwd_ops.hip): formulas, hard inputs, cases and metrics shared by tests/test_unet_contract_cpu.py (the references agree with independent
implementations, seeded defects fall outside; no GPU) and tests/test_gpu_unet_envelope.py (every kernel against them, between red zones).

The rule and its helpers are tests/_envelope.py's.  References are the modelled project's formulas written out in float64 on the CPU from the same
fp32 input values (unet.py:24-39, 166, 186-197; common.py:45-52; msg_processor.py:88-115; pixel_decoder.py:76-79; nn.BatchNorm2d's training
branch); the yardstick is the same formula in float32 through ATen on one thread.  Two metrics:
    sums and dot products (pool + linear, message latent / table / border classes, the 1x1 output conv and its adjoint, the x2 bilinear and its
    adjoint, the reflection adjoints): the error in units of 2^-24 * sum |terms| (`units`, floor 1); an output whose terms are all zero must be
    reproduced exactly
    BatchNorm's folded scale / shift / running statistics and the scale-shift-activation that applies them: per channel, max |got - ref| /
    max |ref| (`group_err`, floor 2^-24), one row per channel CLASS of the hard channels (`class_rows`), each against its own yardstick
A plain CPU module: torch and the standard library only."""
import functools
import math

import torch
import torch.nn.functional as F

from tests._envelope import ENV_SHAPES, U32, check_rows, check_units, group_err, hard_matrix, one_thread

# Twice the largest ratio measured on an MI355X over every case of tests/test_gpu_unet_envelope.py (profiles/unet_fp64_envelope.txt lists them),
# never more than 8: a kernel that needs more has a defect.
UNET_MARGIN = 3.97             # 2 x 1.987, the largest ratio measured: `shift` of the outlier channel, vs_bn_batch_stats at rows = 301, C = 130 (1.2e-7 against ATen's 3.9e-8)
WIDTH = 74
envelope = functools.partial(check_rows, "UNET-ENVELOPE", WIDTH, "aten-fp32", UNET_MARGIN)
envelope_units = functools.partial(check_units, "UNET-ENVELOPE", WIDTH, UNET_MARGIN)
BN_EPS = 1e-5

F64, F32 = torch.float64, torch.float32


def f32(v):
    """the fp32 value a `float` kernel argument holds, as a python float"""
    return float(torch.tensor(v, dtype=F32))


def both(fn):
    """(float64 reference, fp32 yardstick) of fn(dtype), ATen on one thread"""
    return one_thread(lambda: (fn(F64), fn(F32)))


def units(got, ref, mag):
    """worst |got - ref| in units of 2^-24 * mag (mag = sum of the magnitudes of the terms of each output); where mag is zero the output has no
    non-zero term and must be exactly zero (inf otherwise)"""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    d = (got - ref).abs()
    u = torch.where(mag > 0, d / (U32 * mag.clamp_min(1e-300)), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(u.max())


CHANNEL_CLASSES = ("mean30", "const", "outlier", "tiny")          # hard_matrix(..., "cols"): every channel but 1, 2, 3 | channel 1 | 2 | 3


def class_channels(C):
    return {"mean30": [c for c in range(C) if c not in (1, 2, 3)], "const": [1], "outlier": [2], "tiny": [3]}


def class_rows(name, got, r64, r32, dim, keep=None):
    """envelope rows of a [rows, C] (dim = 0: a channel is a group) or [C] (dim = None) result, one per channel class, each against the yardstick of
    its OWN class: the fp32 yardstick differs by orders of magnitude between the classes (on the constant channel x * scale is about 1e4 and
    cancels against shift to beta: an unfused fp32 multiply-add loses 1e-4 .. 2e-3 there, 1e-6 on the mean-30 channels), and the worst class must
    not set the bound of the others"""
    got, r64, r32 = got.detach().cpu(), r64.detach().cpu(), r32.detach().cpu()
    out = []
    for cls, ch in class_channels(got.shape[-1]).items():
        k = None if keep is None else keep[..., ch]
        out.append((f"{name}/{cls}", group_err(got[..., ch], r64[..., ch], dim, k), group_err(r32[..., ch], r64[..., ch], dim, k)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ hard inputs
FRAME_KINDS = ("noise", "const", "checker", "ramp", "impulse")


def frames(kind, B, C, H, W, seed=0):
    """[B, C, H, W] float32 of one kind (those of tests/_img_ref.py, for any channel count): noise = mean 30 / std 0.5 (the shifted activations of
    the other families), const = 30.25 and 0.3 by channel parity, checker = 0 / 1 by pixel parity (inverted on odd channels), ramp = a plane
    through the map different per channel, impulse = zero but single ones (first / last row and column by channel, a 3 x 2 lattice)"""
    g = torch.Generator().manual_seed(2100 + 131 * H + 17 * W + C + seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    c = torch.arange(C).view(1, C, 1, 1)
    if kind == "noise":
        return 30.0 + 0.5 * torch.randn(B, C, H, W, generator=g)
    if kind == "const":
        return torch.where(c % 2 == 0, torch.tensor(30.25), torch.tensor(0.3)).expand(B, C, H, W).contiguous()
    if kind == "checker":
        return ((yy + xx).view(1, 1, H, W) + c) .remainder(2).float().expand(B, C, H, W).contiguous()
    if kind == "ramp":
        rx, ry = xx.float() / max(W - 1, 1), yy.float() / max(H - 1, 1)
        a = torch.rand(C, generator=g).view(1, C, 1, 1)
        return (a * rx + (1 - a) * ry + 0.1 * c).expand(B, C, H, W).contiguous()
    if kind == "impulse":
        x = torch.zeros(B, C, H, W)
        for ch in range(C):
            k = ch % 5
            if k == 0:
                x[:, ch, 0] = 1.0
            elif k == 1:
                x[:, ch, -1] = 1.0
            elif k == 2:
                x[:, ch, :, 0] = 1.0
            elif k == 3:
                x[:, ch, :, -1] = 1.0
            else:
                x[:, ch, ::3, ::2] = 0.75
        return x
    raise ValueError(kind)


def nhwc(x, ld=None):
    """[B, C, H, W] -> [B H W, ld] with zero pad lanes"""
    B, C, H, W = x.shape
    ld = ld or C
    t = torch.zeros(B * H * W, ld, dtype=x.dtype)
    t[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    return t


def nchw(rows, B, H, W):
    """[B H W, C] -> [B, C, H, W]"""
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def padded(t, ld):
    """[..., C] -> [..., ld] with zero pad lanes"""
    out = torch.zeros(t.shape[:-1] + (ld,), dtype=t.dtype)
    out[..., : t.shape[-1]] = t
    return out


def saturated_delta(shape, seed=0):
    """tanh outputs in (-1, 1) and ON its ends: uniform values, then in turn elements exactly +1, exactly -1, 1 - k ulp and -(1 - k ulp) for
    k = 1, 2, 3 (ulp = 2^-24 below 1) -- where 1 - d^2 cancels all but a few bits -- and exactly 0"""
    g = torch.Generator().manual_seed(2200 + seed)
    d = (1.6 * torch.rand(shape, generator=g) - 0.8).flatten()
    special = [1.0, -1.0, 0.0] + [s * (1.0 - k * 2.0 ** -24) for k in (1, 2, 3) for s in (1.0, -1.0)]
    for i in range((d.numel() + 1) // 2):
        d[2 * i] = special[i % len(special)]
    return d.view(shape)


def relu_z(rows, C, seed=0):
    """pre-activations for the ReLU decision: randn, and in turn +0, -0, +-denormals (2^-149, 2^-127) and +-2^-24-sized values, +-2^-30"""
    g = torch.Generator().manual_seed(2300 + seed)
    z = torch.randn(rows * C, generator=g)
    special = [0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -127, 2.0 ** -24, -2.0 ** -24, 2.0 ** -30, -2.0 ** -30]
    for i in range(z.numel() // 2):
        z[2 * i] = special[i % len(special)]
    return z.view(rows, C)


# ------------------------------------------------------------------------------------------------------------------------ BatchNorm (batch statistics)
# (rows, C, ld): the shared shapes + n = 1 (the variance is not divided by n - 1) + one row past a 2048-row chunk (ld 8: G = 2, 128 row lanes) +
# G = 5 / 51 row lanes / chunks of 816 rows, one row past + two grid columns of 64 float4 groups, the second partly empty
BN_SHAPES = ENV_SHAPES + [(1, 4, 4), (2049, 6, 8), (817, 18, 20), (65, 260, 260)]
BN_MOMENTA = (0.1, 1.0)


def bn_inputs(rows, C):
    """x = hard channels (mean 30 / std 0.5; channel 1 constant; channel 2 one 4e3 outlier; channel 3 of magnitude 1e-3, below sqrt(eps)), gamma,
    beta and non-trivial previous running statistics (positive, so that the update never cancels)"""
    g = torch.Generator().manual_seed(2400 + rows + C)
    x = hard_matrix(rows, C, 2401 + rows + C, "cols") if rows > 1 else 30.0 + 0.5 * torch.randn(1, C, generator=g)
    gamma, beta = 1 + 0.5 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    return x, gamma, beta, 0.5 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g)


def bn_fold(x, gamma, beta, rmean, rvar, momentum, eps=BN_EPS, *, biased_running=False, seq32_mean=False):
    """(scale, shift, running_mean', running_var') of nn.BatchNorm2d's training branch over the rows of x [rows, C], in x's dtype: biased variance
    for the normalisation, momentum update with the UNBIASED variance (the variance itself for a single row, where torch refuses to train).
    DEFECTS for the teeth test: biased_running = running_var from the biased variance; seq32_mean = the mean that `shift` uses summed row by
    row in fp32 (behind a 4e3 outlier every later row loses its low bits)"""
    n = x.shape[0]
    mean, var = x.mean(0), x.var(0, unbiased=False)
    scale = gamma / torch.sqrt(var + eps)
    m_shift = mean
    if seq32_mean:
        s = torch.zeros_like(mean)
        for r in range(n):
            s = s + x[r]
        m_shift = s / n
    shift = beta - m_shift * scale
    unb = var if (n == 1 or biased_running) else var * (n / (n - 1))
    return scale, shift, (1 - momentum) * rmean + momentum * mean, (1 - momentum) * rvar + momentum * unb


def bn_ref(x, gamma, beta, rmean, rvar, momentum, **defect):
    return both(lambda dt: bn_fold(x.to(dt), gamma.to(dt), beta.to(dt), rmean.to(dt), rvar.to(dt), momentum, **(defect if dt == F32 else {})))


BN_NAMES = ("sc", "sh", "rm", "rv")               # scale, shift, running mean, running variance: one row per channel class each


# ------------------------------------------------------------------------------------------------------------------------ scale-shift-activation
ACTS = (0, 1, 2, 3, 4)                      # none, ReLU, GELU (erf), tanh, SiLU: every code vs_apply_act tells apart
SSA_SHAPES = [(1, 4, 8, 12, 16), (7, 20, 24, 20, 28), (301, 132, 136, 140, 132)]          # rows, C, ld, add_ld, out_ld: the three strides differ


def act_fn(act):
    return {0: lambda v: v, 1: F.relu, 2: F.gelu, 3: torch.tanh, 4: F.silu}[act]


def ssa_inputs(rows, C):
    """x = the hard channels, scale / shift = their folded float64 BatchNorm rounded to fp32 (x * scale and shift cancel from 60 to O(1)), add"""
    g = torch.Generator().manual_seed(2500 + rows + C)
    x = hard_matrix(max(rows, 8), C, 2501 + rows + C, "cols")
    gamma, beta = 1 + 0.5 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    sc, sh, _, _ = bn_fold(x.double(), gamma.double(), beta.double(), torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64), 0.1)
    return x[:rows].contiguous(), sc.float(), sh.float(), torch.randn(rows, C, generator=g)


def ssa(x, scale, shift, act, add, *, tanh_gelu=False, gain=None):
    """act(x * scale + shift) (+ add).  DEFECTS for the teeth test: tanh_gelu = the tanh approximation in place of the erf GELU (off by up to 5e-4);
    gain = the result times a constant next to 1 (3e-5: about 500 ulp)"""
    v = x * scale + shift
    y = F.gelu(v, approximate="tanh") if (tanh_gelu and act == 2) else act_fn(act)(v)
    if gain is not None:
        y = y * gain
    return y if add is None else y + add


def ssa_ref(x, scale, shift, act, add, **defect):
    return both(lambda dt: ssa(x.to(dt), scale.to(dt), shift.to(dt), act, None if add is None else add.to(dt), **(defect if dt == F32 else {})))


CHAIN_SHAPES = ENV_SHAPES[:2] + [(817, 20, 20)]


def chain_inputs(rows, C):
    """the hard channels, gamma and beta of tests/test_gpu_bwd_unet.py's backward chain (same seeds: ATen's fp32 run takes every ReLU decision of
    the float64 reference on them) and the residual branch `add`; beta of the constant channel, whose pre-activation IS beta, is away from zero"""
    g = torch.Generator().manual_seed(60)
    x = hard_matrix(rows, C, 61, "cols")
    gamma, beta, add = 1 + 0.5 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g), torch.randn(rows, C, generator=g)
    beta[1] = 0.25
    return x, gamma, beta, add


def bn_relu_add(x, gamma, beta, add, eps=BN_EPS):
    """(relu(batch_norm(x)) + add, the pre-activation) of a train-mode ResnetBlock (unet.py:30, 38-39) through F.batch_norm"""
    pre = F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps)
    return F.relu(pre) + add, pre


def relu_gate(x, gamma, beta, pre64):
    """mask of the elements whose float64 pre-activation is further from zero than tau = 4 U (|x scale| + |mean scale| + |beta|): scale, shift and
    the multiply-add each round once, so the others may legitimately fall on either side of the ReLU (tests/test_gpu_bwd_unet.py)"""
    xd = x.double()
    sc = gamma.double() / torch.sqrt(xd.var(0, unbiased=False) + BN_EPS)
    tau = 4 * U32 * ((xd * sc).abs() + (xd.mean(0) * sc).abs() + beta.double().abs())
    return (pre64.abs() > tau).double()


# ------------------------------------------------------------------------------------------------------------------------ x2 bilinear of the concat
# (B, H, W, C1, C2, ld1, ld2, out_ld, skip_scale): H = 1 / W = 1 maps, 2 x 2, an odd map with more than one block; each ld larger than its
# channel count once
UPCAT_CASES = [(1, 1, 1, 4, 4, 4, 4, 8, 2 ** -0.5), (2, 1, 5, 4, 8, 8, 8, 12, 1.0), (2, 6, 1, 8, 4, 8, 8, 12, 2 ** -0.5),
               (2, 7, 9, 24, 8, 24, 8, 36, 2 ** -0.5), (1, 2, 2, 4, 4, 4, 4, 8, 1.0)]


def bilinear2x(v, clamp=True):
    """x2 bilinear, align_corners = False, written out per axis (ATen's upsample_bilinear2d: source index (Y + 0.5) / 2 - 0.5, clamped at 0; taps
    i0 = floor, i1 = min(i0 + 1, n - 1)).  clamp = False is the DEFECT of the teeth test: the first row / column extrapolates with weights
    1.25 / -0.25"""
    def axis(t, dim):
        n = t.shape[dim]
        src = (torch.arange(2 * n, dtype=t.dtype) + 0.5) * 0.5 - 0.5
        if clamp:
            src = src.clamp_min(0)
        i0 = src.floor().clamp(0, n - 1).long()
        i1 = (i0 + 1).clamp_max(n - 1)
        f = src - i0.to(t.dtype)
        shape = [1] * t.dim()
        shape[dim] = 2 * n
        return t.index_select(dim, i0) * (1 - f).view(shape) + t.index_select(dim, i1) * f.view(shape)
    return axis(axis(v, 2), 3)


def upcat(x, skip, s, *, no_clamp=False):
    """[B, C1 + C2, 2H, 2W]: unet.py:186-187 + common.py:46.  DEFECT no_clamp: see bilinear2x"""
    v = torch.cat((x, skip * s), 1)
    return bilinear2x(v, clamp=False) if no_clamp else F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)


def upcat_ref(x, skip, s, **defect):
    s = f32(s)
    return both(lambda dt: upcat(x.to(dt), skip.to(dt), s, **(defect if dt == F32 else {})))


def upcat_mag(x, skip, s):
    """sum of the magnitudes of the (at most four) terms of every output: the same interpolation (non-negative weights) of |cat|"""
    return upcat(x.double().abs(), skip.double().abs(), abs(f32(s)))


def upcat_bwd(dhi, C1, s):
    """(dx, dskip) [B, C, H, W]: autograd of `upcat` for the upstream gradient dhi [B, C1 + C2, 2H, 2W]"""
    B, C, H2, W2 = dhi.shape
    x = torch.zeros(B, C1, H2 // 2, W2 // 2, dtype=dhi.dtype, requires_grad=True)
    sk = torch.zeros(B, C - C1, H2 // 2, W2 // 2, dtype=dhi.dtype, requires_grad=True)
    upcat(x, sk, s).backward(dhi)
    return x.grad, sk.grad


def upcat_bwd_ref(dhi, C1, s):
    s = f32(s)
    return both(lambda dt: upcat_bwd(dhi.to(dt), C1, s))


# ------------------------------------------------------------------------------------------------------------------------ 1x1 output conv + tanh
OUTC_CASES = [(1, 1, 1, 1, 4), (2, 257, 6, 3, 8), (1, 257, 16, 4, 16), (2, 1, 130, 2, 132), (1, 257, 130, 4, 132)]    # B, rows per frame, C, Cout, ld


def outc_inputs(B, rpf, C, Cout):
    """x [rows, C]: channel 0 of mean 30 / std 0.5, the others randn; the bias cancels the shift of channel 0 (w[o][0] * 30 + bias[o] = 0 to fp32
    rounding); the other channels of row r are scaled by |linspace(-12, 12)[r]|, so that the pre-activations spread over [-12, 12]: tanh saturates"""
    g = torch.Generator().manual_seed(2600 + rpf + C + Cout)
    rows = B * rpf
    x = torch.randn(rows, C, generator=g)
    x[:, 0] = 30.0 + 0.5 * torch.randn(rows, generator=g)
    w = torch.randn(Cout, C, generator=g) / math.sqrt(C)
    bias = -30.0 * w[:, 0]
    spread = torch.linspace(-12.0, 12.0, rows).view(rows, 1) if rows > 1 else torch.ones(1, 1)
    x[:, 1:] = x[:, 1:] * (spread.abs().clamp_min(0.05) / 3)          # three standard deviations reach 12
    return x, w, bias


def outc(x, w, bias, use_tanh):
    """[rows, Cout]: unet.py:166, 194-196"""
    v = x @ w.t() + bias
    return torch.tanh(v) if use_tanh else v


def outc_ref(x, w, bias, use_tanh):
    return both(lambda dt: outc(x.to(dt), w.to(dt), bias.to(dt), use_tanh))


def outc_mag(x, w, bias, use_tanh):
    """first-order size of one fp32 rounding per term: (sum |x w| + |bias|) tanh'(v) + |tanh(v)|"""
    xd, wd, bd = x.double(), w.double(), bias.double()
    S = xd.abs() @ wd.abs().t() + bd.abs()
    if not use_tanh:
        return S
    t = torch.tanh(xd @ wd.t() + bd)
    return S * (1 - t * t) + t.abs()


def outc_bwd(delta, ddelta, w, use_tanh, *, linear_defect=False):
    """(dv [rows, Cout], dx [rows, C]) of the kernel's own contract: dv = d delta * (1 - delta^2) from the GIVEN delta, dx = W^T dv.
    DEFECT linear_defect: 1 - delta in place of 1 - delta^2"""
    if use_tanh:
        dv = ddelta * ((1 - delta) if linear_defect else (1 - delta * delta))
    else:
        dv = ddelta
    return dv, dv @ w


def outc_bwd_ref(delta, ddelta, w, use_tanh, **defect):
    return both(lambda dt: outc_bwd(delta.to(dt), ddelta.to(dt), w.to(dt), use_tanh, **(defect if dt == F32 else {})))


def outc_bwd_mag(delta, ddelta, w, use_tanh):
    """(terms of dv: |d delta| (1 + delta^2), terms of dx: the same through |W|)"""
    dd, d = ddelta.double().abs(), delta.double()
    mv = dd * (1 + d * d) if use_tanh else dd
    return mv, mv @ w.double().abs()


# ------------------------------------------------------------------------------------------------------------------------ pool + linear
# (B, HW, C, ld, N, one-hot weights?): the 8 x 8 map of VideoSeal's head, the 31 x 31 of ChunkySeal's, a 32 x 32 with ld > C, a single pixel, the
# branch above 1024 channels, and ld odd (= C): the scalar pooling path
POOL_CASES = [(3, 64, 76, 76, 33, False), (2, 961, 96, 96, 5, False), (2, 961, 96, 96, 5, True), (2, 1024, 96, 100, 257, False), (1, 1, 4, 4, 1, False),
              (1, 16, 1028, 1028, 3, False), (2, 961, 75, 75, 5, True)]


def pool_inputs(B, HW, C, N, onehot):
    g = torch.Generator().manual_seed(2700 + HW + C + N)
    x = torch.stack([hard_matrix(max(HW, 8), max(C, 4), 2701 + HW + C + b, "cols")[:HW, :C] for b in range(B)])
    w = torch.randn(N, C, generator=g) / 8
    bias = 0.1 * torch.randn(N, generator=g)
    if onehot:                      # output n IS the pooled mean of channel n (the first N channels include all four hard kinds)
        w, bias = torch.eye(N, C), torch.zeros(N)
    return x.contiguous(), w, bias


def pool_linear(x, w, bias, *, seq32=False):
    """[B, N]: pixel_decoder.py:76-79 (AdaptiveAvgPool2d(1) + Linear) on x [B, HW, C].  DEFECT seq32: the rows added one by one in fp32"""
    if seq32:
        s = torch.zeros_like(x[:, 0])
        for r in range(x.shape[1]):
            s = s + x[:, r]
        pooled = s / x.shape[1]
    else:
        pooled = x.mean(1)
    return pooled @ w.t() + bias


def pool_ref(x, w, bias, **defect):
    return both(lambda dt: pool_linear(x.to(dt), w.to(dt), bias.to(dt), **(defect if dt == F32 else {})))


def pool_mag(x, w, bias):
    return x.double().abs().mean(1) @ w.double().abs().t() + bias.double().abs()


# ------------------------------------------------------------------------------------------------------------------------ message latent, table gradient
MSG_CASES = [(1, 1, 1), (3, 15, 24), (3, 40, 24), (2, 256, 260), (2, 1000, 24), (2, 1000, 300), (2, 1024, 300)]          # Bm, nbits, hidden
MSG_TABLES = ("randn", "shifted")
MSG_GRAD_CASES = [(1, 1, 1), (3, 7, 12), (64, 16, 130)]


def msg_table(kind, nbits, hidden):
    g = torch.Generator().manual_seed(2800 + nbits + hidden)
    t = torch.randn(2 * nbits, hidden, generator=g)
    return 3.0 + 0.5 * t if kind == "shifted" else t


def msg_bits(Bm, nbits, columns_last=False, seed=0):
    """int32 [Bm, nbits]: random bits; where there are at least three messages the first is all zeros and the last all ones; where there are at
    least three bits, bit column 0 is all zero and bit column nbits - 1 all one.  columns_last: the constant columns win where the two meet
    (table rows 1 and 2 nbits - 2 are then selected by no message: the table gradient's case), else the constant messages do (the latent's)"""
    g = torch.Generator().manual_seed(2900 + Bm + nbits + seed)
    m = torch.randint(0, 2, (Bm, nbits), generator=g).to(torch.int32)

    def cols():
        if nbits >= 3:
            m[:, 0], m[:, -1] = 0, 1

    def rows():
        if Bm >= 3:
            m[0], m[-1] = 0, 1
    for f in ((rows, cols) if columns_last else (cols, rows)):
        f()
    return m


def msg_rows(msgs):
    return 2 * torch.arange(msgs.shape[1])[None, :] + (msgs != 0).long()


def msg_latent(table, msgs, *, seq32=False):
    """[Bm, hidden]: msg_processor.py:88-98, the sum of the selected rows.  DEFECT seq32: the rows added one by one in fp32"""
    sel = table[msg_rows(msgs)]
    if not seq32:
        return sel.sum(1)
    s = torch.zeros_like(sel[:, 0])
    for k in range(sel.shape[1]):
        s = s + sel[:, k]
    return s


def msg_latent_ref(table, msgs, **defect):
    return both(lambda dt: msg_latent(table.to(dt), msgs, **(defect if dt == F32 else {})))


def msg_latent_mag(table, msgs):
    return table.double().abs()[msg_rows(msgs)].sum(1)


def msg_table_grad(dlat, msgs):
    """[2 nbits, hidden]: the adjoint of msg_latent, row r = the sum of dlat over the messages that select r"""
    Bm, nbits = msgs.shape
    sel = torch.zeros(Bm, 2 * nbits, dtype=dlat.dtype)
    sel.scatter_(1, msg_rows(msgs), 1.0)
    return sel.t() @ dlat


def msg_table_grad_ref(dlat, msgs):
    return both(lambda dt: msg_table_grad(dlat.to(dt), msgs))


# ------------------------------------------------------------------------------------------------------------------------ border-class table
MSG_PRE_CASES = [(Bm, N) for Bm in (1, 3) for N in (1, 5, 64)]


def msg_pre(P, N, *, swap_defect=False):
    """[Bm, 9, N] from P [Bm, 9 N] (tap-major): class cy * 3 + cx = the sum of the taps that fall inside the map for a pixel in the first (0) /
    an interior (1) / the last (2) row resp. column (zero padding 1: tap 0 misses on the first, tap 2 on the last).  DEFECT swap_defect: first and
    last swapped"""
    p = P.view(P.shape[0], 3, 3, N)
    valid = {0: slice(1, 3), 1: slice(0, 3), 2: slice(0, 2)}
    if swap_defect:
        valid = {0: valid[2], 1: valid[1], 2: valid[0]}
    return torch.stack([p[:, valid[cy], valid[cx]].sum((1, 2)) for cy in range(3) for cx in range(3)], 1)


def msg_pre_ref(P, N, **defect):
    return both(lambda dt: msg_pre(P.to(dt), N, **(defect if dt == F32 else {})))


# ------------------------------------------------------------------------------------------------------------------------ reflection adjoints
REFLECT_MAPS = [(2, 2), (2, 5), (3, 3), (7, 4)]
REFLECT_CL = [(1, 4), (6, 8), (130, 132)]


def reflect_fold(dxp):
    """[B, C, H, W]: autograd of ReflectionPad2d(1) for dxp [B, C, H + 2, W + 2]"""
    B, C, H2, W2 = dxp.shape
    x = torch.zeros(B, C, H2 - 2, W2 - 2, dtype=dxp.dtype, requires_grad=True)
    F.pad(x, (1, 1, 1, 1), mode="reflect").backward(dxp)
    return x.grad


def col2im_reflect(dcols, C, H, W):
    """[B, C, H, W]: autograd of (ReflectionPad2d(1) + unfold 3 x 3) for dcols [B, H W, 9, C] (tap-major, channels last: vs_im2col3x3's order)"""
    B = dcols.shape[0]
    x = torch.zeros(B, C, H, W, dtype=dcols.dtype, requires_grad=True)
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), mode="reflect"), 3)                    # [B, C * 9, H W], channel-major
    cols.view(B, C, 9, H * W).permute(0, 3, 2, 1).backward(dcols)
    return x.grad


# ------------------------------------------------------------------------------------------------------------------------ bit-for-bit restatements
def im2col3x3(x, pad_mode, stride=1):
    """[B Ho Wo, 9, C] of x [B, C, H, W] (pad_mode "zeros" | "reflect", padding 1), tap-major with the channels last"""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect") if pad_mode == "reflect" else F.pad(x, (1, 1, 1, 1))
    cols = F.unfold(xp, 3, stride=stride)
    return cols.view(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9, C)


def dilate2(dy, H, W):
    """[B, C, H, W]: dy [B, C, Ho, Wo] on the even pixels, zeros elsewhere"""
    B, C, Ho, Wo = dy.shape
    out = torch.zeros(B, C, H, W, dtype=dy.dtype)
    out[:, :, 0:2 * Ho:2, 0:2 * Wo:2] = dy
    return out
