"""Emulator of the split arithmetic of the matrix-core kernels (csrc/conv_common.h, Arith<2> / Arith<3>) and the hard operands, cases and metric
shared by tests/test_split_contract_cpu.py (the contract itself, no GPU) and tests/test_gpu_split_envelope.py (every kernel family against it).

An fp32 operand reaches the matrix cores as 16-bit planes:
  arithmetic 2 ("2 x f16"): x * mul = h + l,  h = RN_f16(x * mul),  l = RN_f16(x * mul - h) (residual taken in fp32, exact), mul a power of two;
                            three partial products  h_a h_w + h_a l_w + l_a h_w,  accumulator times acc_mul = 1 / (a_mul w_mul)
  arithmetic 3 ("3 x bf16"): three truncated bf16 terms that add up to x exactly, six partial products: the exact product of the fp32 operands
  arithmetic 0 (fp32-input MFMA): the operand unchanged
`ideal` evaluates that sum in float64: S, the value a kernel with an exact accumulator would form, and P = sum |p| over the partial products of
every output element (+ |bias|, + |residual| where the epilogue adds them: they are terms of the same fp32 sum).  A correct kernel differs from S
by the order of its fp32 accumulation and the final rounding only -- a few units of 2^-24 P per element, whatever the rest of the tensor holds.
The comparator of that difference is ATen's float32 product of the SAME split operands on the CPU (one thread), measured in the same unit."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests._envelope import U32, one_thread
from videoseal_amd.engine import split_bf16x3, split_f16x2

TINY = 1e-300
F16_MIN_NORMAL = 2.0 ** -14
# Twice the largest ratio  max r / max(max r_ref, 1)  measured on an MI355X over every case of tests/test_gpu_split_envelope.py
# (profiles/split_fp64_envelope.txt lists them), never more than 8: a family that needs more has a defect.
SPLIT_MARGIN = 6.61          # 2 x 3.306, the largest ratio measured: the 64-column patch kernel (tile 11) with the tanh epilogue in the 2 x f16 arithmetic
OLD_TOL = 2e-5          # the criterion of the older parity tests: max |got - ref| < 2e-5 max |ref| over the whole tensor


# ------------------------------------------------------------------------------------------------------------------------ the splits
def split_f16(x: torch.Tensor, mul: float):
    """arithmetic 2, activation side (conv_common.h::split4h): float16 tensors (h, l)"""
    xs = x.float() * mul                                    # exact: mul is a power of two
    h = xs.to(torch.float16)
    return h, (xs - h.float()).to(torch.float16)            # |xs - h| <= ulp_f16(h) / 2: the fp32 residual is exact


def split_f16_weights(w: torch.Tensor):
    """arithmetic 2, weight side: the planes engine.split_f16x2 packs (what the kernel reads) as float16 (h, l), and w_mul"""
    planes, w_mul = split_f16x2(w)
    return planes[0].view(torch.float16), planes[1].view(torch.float16), w_mul


def split_bf16(x: torch.Tensor):
    """arithmetic 3: the three truncated bf16 terms as float64 tensors"""
    p = split_bf16x3(x)
    return [(p[i].to(torch.int32) << 16).view(torch.float32).double() for i in range(3)]


def flush_denormal(l: torch.Tensor) -> torch.Tensor:
    """DEFECT for the teeth test: a low plane whose f16 denormals are read as zero"""
    return torch.where(l.float().abs() < F16_MIN_NORMAL, torch.zeros_like(l), l)


# ------------------------------------------------------------------------------------------------------------------------ ideal result
def _cols(x, k, stride, pad, reflect):
    """[B, C, H, W] -> patch matrix [B, L, C k k] (K index = c k k + tap, the order of w.reshape(N, -1))"""
    if pad:
        x = F.pad(x, (pad, pad, pad, pad), mode="reflect" if reflect else "constant")
    return F.unfold(x, k, stride=stride).transpose(1, 2)


def _conv32(x, w, stride, pad, reflect):
    if pad:
        x = F.pad(x, (pad, pad, pad, pad), mode="reflect" if reflect else "constant")
    return F.conv2d(x, w, stride=stride)


def ideal(a, w, arith, a_mul=16.0, w_mul=None, *, stride=1, pad=0, reflect=False, extras=False):
    """a [B, C, H, W], w [N, C, k, k] float32 (CPU).  A GEMM is the k = 1 case ([rows, K] -> gemm_as_conv).  Returns a namespace of
    [B, N, Ho, Wo] tensors: S, P (float64, see the module docstring), ref32 (the comparator, float32), true (float64 product of the fp32 operands),
    and with extras=True: bound (a-priori bound of |S - true| from the per-element split errors), S_flush and S_tail (the two defective
    emulations of the teeth test: denormal low terms read as zero; l_a h_w dropped on the last 16 of K in the kernels' (tap, channel) order).
    w_mul is engine.split_f16x2's own (the argument only asserts it)."""
    B, C, H, W = a.shape
    N, k = w.shape[0], w.shape[2]
    kw = dict(k=k, stride=stride, pad=pad, reflect=reflect)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    shape = lambda m: m.transpose(1, 2).reshape(B, N, Ho, Wo)          # noqa: E731  [B, L, N] -> [B, N, Ho, Wo]
    A, Wm = _cols(a.double(), **kw), w.double().reshape(N, -1)
    r = SimpleNamespace(true=shape(A @ Wm.T), w_mul=1.0, acc_mul=1.0)
    if arith != 2:
        r.S, r.P = r.true, shape(A.abs() @ Wm.abs().T)
        r.ref32 = one_thread(lambda: _conv32(a, w, stride, pad, reflect))
        return r
    ha, la = split_f16(a, a_mul)
    hw, lw, r.w_mul = split_f16_weights(w)
    assert w_mul is None or w_mul == r.w_mul
    assert torch.isfinite(ha.float()).all(), "operand beyond the range of the 2 x f16 split at this a_mul"
    acc = r.acc_mul = 1.0 / (a_mul * r.w_mul)
    Ha, La = _cols(ha.double(), **kw), _cols(la.double(), **kw)
    Hw, Lw = hw.double().reshape(N, -1), lw.double().reshape(N, -1)
    r.S = shape(acc * (Ha @ (Hw + Lw).T + La @ Hw.T))
    r.P = shape(acc * (Ha.abs() @ (Hw.abs() + Lw.abs()).T + La.abs() @ Hw.abs().T))
    h32, l32, hw32, lw32 = ha.float(), la.float(), hw.float(), lw.float()
    r.ref32 = one_thread(lambda: (_conv32(h32, hw32, stride, pad, reflect) + _conv32(h32, lw32, stride, pad, reflect)
                                  + _conv32(l32, hw32, stride, pad, reflect)) * torch.tensor(acc, dtype=torch.float32))
    if extras:
        at, wt = a.double() * a_mul, w.double() * r.w_mul
        ea, ew = (at - ha.double() - la.double()).abs(), (wt - hw.double() - lw.double()).abs()
        Ea, Ew, At, Wt = _cols(ea, **kw), ew.reshape(N, -1), _cols(at.abs(), **kw), wt.abs().reshape(N, -1)
        r.bound = shape(acc * (Ea @ Wt.T + At @ Ew.T + Ea @ Ew.T + La.abs() @ Lw.abs().T))
        r.ea, r.ew, r.at, r.wt, r.la, r.lw = ea, ew, at, wt, la, lw
        Laf, Lwf = _cols(flush_denormal(la).double(), **kw), flush_denormal(lw).double().reshape(N, -1)
        r.S_flush = shape(acc * (Ha @ (Hw + Lwf).T + Laf @ Hw.T))
        idx = torch.arange(C * k * k)
        tail = (idx % (k * k)) * C + idx // (k * k) >= C * k * k - 16      # position in the kernels' K order (tap, channel)
        r.S_tail = r.S - shape(acc * (La[:, :, tail] @ Hw[:, tail].T))
    return r


def gemm_as_conv(a2d: torch.Tensor) -> torch.Tensor:
    """[rows, K] -> [1, K, rows, 1]: a GEMM row is a pixel of a 1x1 conv"""
    return a2d.t().reshape(1, a2d.shape[1], a2d.shape[0], 1)


ACTS = {0: lambda v: v, 1: F.relu, 2: F.gelu, 3: torch.tanh}


def epilogue(v, P=None, bias=None, act=0, res=None):
    """act(v + bias) + res in v's dtype, channel dim 1; with P also the unit P + |bias| + |res|"""
    if bias is not None:
        b = bias.to(v.dtype).view(1, -1, 1, 1)
        v = v + b
        P = P + b.abs() if P is not None else None
    v = ACTS[act](v)
    if res is not None:
        v = v + res.to(v.dtype)
        P = P + res.to(v.dtype).abs() if P is not None else None
    return v if P is None else (v, P)


def units(got, S, P):
    """r = |got - S| / max(2^-24 P, tiny) per element (float64)"""
    return (got.double() - S).abs() / (U32 * P).clamp_min(TINY)


def old_criterion_accepts(got, ref) -> bool:
    return bool((got.double() - ref.double()).abs().max() < OLD_TOL * ref.double().abs().max())


# ------------------------------------------------------------------------------------------------------------------------ hard operands
NGROUPS = 6
GROUP_NAMES = ["magnitude 1e-4", "mean 30 / std 0.5", "constant 0.37", "one 4e3 outlier", "eight decades", "exact zeros"]


def _group_values(gid, g, shape):
    z = torch.randn(shape, generator=g)
    if gid == 0:
        return 1e-4 * z
    if gid == 1:
        return 30.0 + 0.5 * z
    if gid == 2:
        return torch.full(shape, 0.37)
    if gid == 3:
        return z                                     # (the outlier is planted by the caller: one element per group)
    if gid == 4:
        return torch.sign(z) * 10.0 ** (8.0 * torch.rand(shape, generator=g) - 6.0)       # 1e-6 ... 1e2
    return torch.zeros(shape)


def group_ids(B, C, H, W):
    """[B, C, H, W] group index: by frame and by band of >= 3 image rows (so that interior 3x3 patches stay inside one group and border ones mix
    two); in odd frames also by channel half, so that every patch there mixes two groups"""
    band = band_height(H)
    b = torch.arange(B).view(B, 1, 1, 1)
    c = torch.arange(C).view(1, C, 1, 1)
    y = torch.arange(H).view(1, 1, H, 1)
    gid = b + y // band + (b % 2) * (c // max(1, (C + 1) // 2))
    return (gid % NGROUPS).expand(B, C, H, W)


def band_height(H):
    return max(3, -(-H // NGROUPS))


def hard_act(B, C, H, W, seed, gelu_like=False):
    """hard activations [B, C, H, W] float32, fixed seed.  gelu_like: the operand of the a_mul = 1 GEMMs -- gelu(randn) (two thirds of it below
    0.25: denormal low terms at a_mul = 1) with the small, constant, wide-range and zero groups kept, by rows"""
    g = torch.Generator().manual_seed(seed)
    gid = group_ids(B, C, H, W)
    x = torch.zeros(B, C, H, W)
    for i in range(NGROUPS):
        x = torch.where(gid == i, _group_values(i, g, (B, C, H, W)), x)
    if gelu_like:
        x = torch.where((gid == 1) | (gid == 3), F.gelu(torch.randn(B, C, H, W, generator=g)), x)
    else:                                            # one 4e3 outlier in every (frame, band) of group 3: |a| a_mul = 64000 < 65504
        spot = ((gid == 3) & (torch.arange(W).view(1, 1, 1, W) == W // 2) & (torch.arange(C).view(1, C, 1, 1) == C // 2)
                & (torch.arange(H).view(1, 1, H, 1) % band_height(H) == 0))
        x = torch.where(spot, torch.full_like(x, 4.0e3), x)
    return x.contiguous()


def hard_rows(rows, K, seed, gelu_like=False):
    """the same for a GEMM operand [rows, K]: groups by blocks of 3 rows, in rotation"""
    return hard_act(1, K, rows, 1, seed, gelu_like)[0, :, :, 0].t().contiguous()


def hard_weights(N, C, k, seed):
    """randn / sqrt(K) with output channel 1 scaled by 1e-5, channel 2 with every other tap zero, channel 3 with a single dominant weight"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, C, k, k, generator=g) / math.sqrt(C * k * k)
    flat = w.view(N, -1)
    if N > 1:
        flat[1] *= 1e-5
    if N > 2:
        flat[2, ::2] = 0.0
    if N > 3:
        flat[3, flat.shape[1] // 3] = 50.0
    return w


def hard_bias(N, seed):
    """channel n: zero (n % 3 == 0), 1e-3 randn (1), randn (2) -- a bias of ordinary size would hide a small row's error behind its own rounding"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(N, generator=g)
    n = torch.arange(N)
    return torch.where(n % 3 == 0, torch.zeros(N), torch.where(n % 3 == 1, 1e-3 * b, b))


def hard_dy(rows, N, seed):
    """gradient rows for the weight-gradient kernels: 1e-12 ... 1e3 by row group (blocks of 5 rows, six decades-and-a-half apart), every
    fourth group zero"""
    g = torch.Generator().manual_seed(seed)
    grp = (torch.arange(rows) // 5) % 4
    mag = torch.tensor([1e-12, 1e-6, 1e3, 0.0])[grp]
    return (torch.randn(rows, N, generator=g) * mag[:, None]).contiguous()


# ------------------------------------------------------------------------------------------------------------------------ the cases
# Per distinct tile code the smallest ragged geometry of CONV_CASES / GEMM_PL_CASES / GEMM_PC_CASES (tests/test_gpu_kernels.py).
CONV_ENV_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad, reflect, act, tile
    (2, 16, 17, 23, 16, 3, 1, 1, 0, 1, 0),
    (3, 32, 20, 20, 64, 3, 2, 1, 0, 0, 0),          # stride 2
    (2, 64, 16, 16, 136, 3, 1, 1, 1, 0, 0),         # reflect
    (2, 96, 9, 9, 200, 3, 1, 1, 0, 1, 1),
    (1, 48, 9, 11, 40, 1, 1, 0, 0, 2, 2),
    (2, 32, 20, 20, 64, 3, 2, 1, 0, 0, 2),          # stride 2
    (2, 24, 12, 12, 20, 3, 1, 1, 1, 3, 3),
    (2, 128, 16, 16, 192, 3, 1, 1, 0, 1, 4),
    (2, 128, 16, 16, 96, 1, 1, 0, 0, 2, 5),
    (1, 1, 32, 32, 16, 3, 1, 1, 0, 1, 10),
    (2, 100, 9, 17, 64, 3, 1, 1, 0, 3, 11),
    (2, 32, 13, 21, 136, 3, 1, 1, 1, 0, 12),
    (2, 96, 8, 8, 200, 1, 1, 0, 0, 2, 13),
    (3, 160, 7, 9, 130, 3, 2, 1, 0, 1, 14),         # stride 2
    (3, 48, 13, 21, 136, 3, 1, 1, 1, 2, 15),
    (3, 48, 13, 21, 200, 3, 1, 1, 1, 2, 0x40),
    (3, 48, 13, 21, 70, 3, 1, 1, 1, 2, 0x43),
    (3, 16, 13, 21, 32, 3, 1, 1, 1, 2, 0x44),
    (3, 80, 21, 37, 50, 3, 1, 1, 1, 2, 0x45),
]
CONV_ENV_PARAMS = [(c, ar) for c in CONV_ENV_CASES for ar in ((2, 3, 0) if c[-1] < 10 else (2, 3))]

# planes 3x3 kernel (conv3x3_pl.hip, tile codes 22 / 23): B, C, H, W, Cout, two-phase, K slices
PLANES_ENV_CASES = [(2, 32, 16, 16, 192, False, 1), (1, 16, 16, 16, 64, False, 1), (3, 64, 16, 48, 200, True, 1),
                    (2, 96, 16, 16, 192, True, 2), (2, 96, 16, 16, 192, True, 3), (1, 384, 16, 32, 384, False, 8)]

# planes GEMM (gemm_pl.hip): B, H, W, K, N, act, affine, res, tile (24 / 25 small, 27 big), K slices, a_mul
GEMM_PL_ENV_CASES = [
    (3, 8, 8, 768, 200, 0, False, True, 24, 1, 16.0),         # ragged M (192 rows) and N
    (3, 8, 8, 768, 200, 0, False, True, 24, 1, 1.0),          # the same at a_mul = 1 on the GELU-like operand
    (3, 8, 8, 768, 200, 1, True, True, 24, 4, 1.0),           # through vs_to_planes_affine, K in 4 slices + epilogue kernel
    (5, 8, 8, 64, 40, 3, False, False, 25, 2, 16.0),          # two K16 steps per slice, tanh
    (2, 16, 24, 16, 130, 2, False, True, 24, 1, 16.0),        # a single K step
    (3, 15, 15, 160, 96, 0, False, True, 25, 1, 1.0),         # 225-row frames
    (3, 15, 15, 160, 520, 0, False, True, 27, 1, 16.0),       # big tile (one wave per SIMD): ragged rows (675) and columns, residual
    (2, 16, 24, 48, 300, 2, False, False, 27, 1, 1.0),        # three K steps (odd count), GELU, a_mul = 1
]

# wave-specialised 1x1 GEMM (gemm1x1_pc.hip): B, H, W, K, N, act, res, tile (CONV_TILE_HI | tl), K slices
GEMM_PC_ENV_CASES = [
    (5, 8, 8, 64, 40, 3, False, 1, 2),              # one K pair per slice, tanh, K-slice epilogue
    (3, 15, 15, 160, 96, 0, True, 1, 1),            # frame boundaries at arbitrary rows
    (2, 16, 24, 32, 130, 2, True, 2, 1),            # single pair, three N tiles of which one ragged
    (3, 8, 8, 768, 200, 1, True, 1, 4),             # K in 4 slices + epilogue kernel
    (3, 8, 8, 768, 200, 0, True, 10, 1),            # tile 26 (2 x f16 only): ragged M and N
    (5, 8, 8, 64, 40, 3, False, 10, 2),
]
GEMM_PC_ENV_PARAMS = [(c, ar) for c in GEMM_PC_ENV_CASES for ar in ((2,) if c[7] == 10 else (2, 3))]

# weight gradients: rows, N, K, ld_n, ld_k (N, K >= 64: the bf16-split matrix-core kernel; thinner: the fp32 FMA kernel; VS_WGRAD=mfma: fp32 MFMA)
WGRAD_GEMM_CASES = [(1000, 20, 36, 20, 36), (7, 5, 70, 8, 72), (2500, 130, 200, 132, 200), (33, 64, 64, 64, 64)]
# B, H, W, ci, co, stride, reflect (co, ld >= 64: matrix cores; co <= 32: register tiles)
WGRAD_CONV_CASES = [(3, 9, 11, 70, 130, 1, 0), (2, 15, 13, 64, 96, 2, 0), (2, 16, 24, 64, 64, 1, 1),
                    (2, 20, 18, 16, 16, 1, 0), (2, 33, 31, 16, 32, 2, 0), (1, 19, 35, 20, 12, 1, 1), (1, 5, 3, 4, 4, 1, 0)]


def shapes_of_the_gpu_file():
    """(tag, build) for every 2 x f16 case above; build() -> (a [B, C, H, W], w, a_mul, conv kwargs): the teeth test runs on exactly the
    operands the GPU file uses"""
    out = []
    for c in CONV_ENV_CASES:
        out.append((f"conv tile {c[-1]:#x} {c[:9]}", lambda c=c: (*conv_operands(c)[:2], 16.0, dict(stride=c[6], pad=c[7], reflect=bool(c[8])))))
    for c in PLANES_ENV_CASES:
        out.append((f"conv3x3_pl {c}", lambda c=c: (*planes_operands(c)[:2], 16.0, dict(stride=1, pad=1, reflect=False))))
    for c in GEMM_PL_ENV_CASES:
        out.append((f"gemm_pl {c}", lambda c=c: (gemm_as_conv(gemm_pl_operands(c)[0]), gemm_pl_operands(c)[1], c[10], {})))
    for c in GEMM_PC_ENV_CASES:
        out.append((f"gemm1x1_pc {c}", lambda c=c: (gemm_as_conv(gemm_pc_operands(c)[0]), gemm_pc_operands(c)[1], 16.0, {})))
    return out


def conv_operands(c):
    B, Cin, H, W, Cout, k = c[:6]
    seed = 1000 + 7 * c[-1] + Cin
    return hard_act(B, Cin, H, W, seed), hard_weights(Cout, Cin, k, seed + 1), hard_bias(Cout, seed + 2)


def planes_operands(c):
    B, C, H, W, Co, two, sk = c
    seed = 2000 + C + sk
    return (hard_act(B, C, H, W, seed), hard_weights(Co, C, 3, seed + 1), hard_bias(Co, seed + 2),
            hard_act(B, C, H, W, seed + 3), hard_weights(Co, C, 1, seed + 4), hard_bias(Co, seed + 5))


def affine_of(x, scale, shift, hw):
    """vs_to_planes_affine's GRN apply, x[r][c] * scale[r / hw][c] + shift[c]: one fused multiply-add per element in fp32 (float64 holds the
    product exactly; the sum is rounded once to 53 bits and then to 24, which differs from the single rounding on a measure-zero set)"""
    rows, K = x.shape
    s = scale.double()[torch.arange(rows) // hw]
    return (x.double() * s + shift.double()).float()


def gemm_pl_operands(c):
    """(a [rows, K] as split by the kernel, w, bias, res, x, scale, shift)"""
    B, H, W, K, Nn, act, affine, res, tile, sk, am = c
    seed = 3000 + K + Nn + int(am)
    rows = B * H * W
    x = hard_rows(rows, K, seed, gelu_like=(am == 1.0))
    g = torch.Generator().manual_seed(seed + 9)
    scale, shift = 1 + 0.5 * torch.randn(B, K, generator=g), 0.1 * torch.randn(K, generator=g)
    a = affine_of(x, scale, shift, H * W) if affine else x
    r = hard_rows(rows, Nn, seed + 3) if res else None
    return a, hard_weights(Nn, K, 1, seed + 1), hard_bias(Nn, seed + 2), r, x, scale, shift


def gemm_pc_operands(c):
    B, H, W, K, Nn, act, res, tl, sk = c
    seed = 4000 + K + Nn + tl
    rows = B * H * W
    return hard_rows(rows, K, seed), hard_weights(Nn, K, 1, seed + 1), hard_bias(Nn, seed + 2), (hard_rows(rows, Nn, seed + 3) if res else None)
