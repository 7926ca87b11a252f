"""Emulation, operands, cases and seeded defects for the two fused kernels whose intermediate tensor never leaves the chip:
vs_cnx_block (csrc/convnext_fused.hip: pwconv1 -> GELU -> GRN apply -> split -> pwconv2) and vs_resblock_thin (csrc/resblock_thin.hip:
conv3x3 -> ReLU -> split -> conv3x3 + 1x1).  Shared by tests/test_fused_contract_cpu.py (the metric bites; no GPU) and
tests/test_gpu_fused_envelope.py (the kernels against it).  The metric is the one of tests/_split_ref.py carried through the on-chip stage.

Both kernels are  first product -> f (on accumulator registers) -> operand split -> last product.  With the emulated planes of _split_ref:
  S1, P1    first product in float64 and the sum of the magnitudes of its terms;           u1 = 2^-24 (P1 + |b_first|)
  v         = f(S1 + b_first) in float64: gelu(.) * scale[frame] + beta with the exact erf GELU (ConvNeXt), relu(.) (ResnetBlock; exactly 0
              outside the image: conv1's zero padding).  First-order propagation of u1:
                  u_v = 1.13 |scale| u1   (max |gelu'| = 1.129)          u_v = u1   (ReLU is 1-Lipschitz: no element needs an exclusion)
              (whole ConvNeXt block: + |gelu| u_scale, the same propagation through  scale = 1 + gamma Gx / (mean_c Gx + 1e-6))
  fmt       the a-priori format term of the second split of v (2 x f16 only; the 3 x bf16 split is exact):
                  2^-22 |v a_mul| / a_mul  (h and l are both rounded to 11 bits)  +  2^-25 / a_mul  (half an f16 denormal step of l)
              a_mul = 1 for the GRN-scaled operand of pwconv2, 16 for t of the ResnetBlock; 0 where v is the padding
  S, P      last product of the emulated split of fp32(v) in float64, then bias and residual (ResnetBlock: relu(. + b1) + 1x1 product + b_res)
  unit      = 2^-24 (P + |bias| + |residual|)  +  sum_k |w[n][k]| (u_v[k] + fmt[k])           per output element
  r         = |got - S| / unit over EVERY element.
The statistics launch of vs_cnx_block is held the same way:  S = sum over 32 pixels of gelu^2,  unit = 2^-24 S + sum (2 |gelu| d + d^2),  d = 1.13 u1:
the propagation of d through the square, written out in full because its first-order part vanishes where gelu is 0 (x1 = -60 next to |x1| = 1e-4
in one group: the exact GELU is 0 there, any fp32 one is within d of it, and d^2 is what the group's sum sees).
The yardstick r_ref is never the code under test: the same chain by ATen in float32 on the CPU (one thread) on the same emulated operands --
ref32 of the first product, float32 GELU / affine / ReLU, split_f16, ref32 of the last product.  A case passes when
max r <= FUSED_MARGIN max(max r_ref, 1);  FUSED_MARGIN is twice the largest ratio measured on an MI355X (profiles/fused_fp64_envelope.txt) and
never above CAP = 8."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests import _split_ref as R

# Twice the largest ratio  max r / max(max r_ref, 1)  measured on an MI355X over every case of tests/test_gpu_fused_envelope.py
# (profiles/fused_fp64_envelope.txt lists them), never more than CAP: a kernel that needs more has a defect.
FUSED_MARGIN = 4.218          # 2 x 2.109, the largest ratio measured: vs_resblock_thin 1 -> 16 -> 16 in the 3 x bf16 arithmetic on B = 2 maps of 9 x 1
GELU_LIP = 1.13
U22, U25 = 2.0 ** -22, 2.0 ** -25
A_MUL, A_MUL_GRN = 16.0, 1.0
F16_OVERFLOW = 65520.0


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ratio_units(got, S, unit):
    """r = |got - S| / max(unit, tiny) per element (float64)"""
    return (got.double() - S).abs() / unit.clamp_min(R.TINY)


def stage(a, w, arith, a_mul=A_MUL, pad=0):
    """_split_ref.ideal for stride-1 zero-padded convs without the patch matrix (the large ResnetBlock maps): a [B, C, H, W], w [N, C, k, k]
    float32 -> S, P (float64), ref32, and for the 2 x f16 arithmetic low = acc_mul l_a h_w and low_flush (the same with f16 denormals of l_a
    read as zero), the planes and acc_mul"""
    c = lambda x, k: F.conv2d(x, k, padding=pad)          # noqa: E731
    r = SimpleNamespace(acc=1.0, w_mul=1.0)
    if arith != 2:
        r.S, r.P = c(a.double(), w.double()), c(a.double().abs(), w.double().abs())
        r.ref32 = R.one_thread(lambda: c(a, w))
        return r
    ha, la = R.split_f16(a, a_mul)
    hw, lw, r.w_mul = R.split_f16_weights(w)
    assert torch.isfinite(ha.float()).all(), "operand beyond the range of the 2 x f16 split at this a_mul"
    acc = r.acc = 1.0 / (a_mul * r.w_mul)
    Ha, La, Hw, Lw = ha.double(), la.double(), hw.double(), lw.double()
    r.low, r.low_flush = acc * c(La, Hw), acc * c(R.flush_denormal(la).double(), Hw)
    r.S = acc * c(Ha, Hw + Lw) + r.low
    r.P = acc * (c(Ha.abs(), Hw.abs() + Lw.abs()) + c(La.abs(), Hw.abs()))
    h32, l32, hw32, lw32 = ha.float(), la.float(), hw.float(), lw.float()
    r.ref32 = R.one_thread(lambda: (c(h32, hw32) + c(h32, lw32) + c(l32, hw32)) * torch.tensor(acc, dtype=torch.float32))
    r.la, r.hw = La, Hw
    return r


def _rows(t):
    """[1, N, rows, 1] -> [rows, N]"""
    return t[0, :, :, 0].t()


def gemm_stage(a2d, w, a_mul):
    r = stage(R.gemm_as_conv(a2d), w, 2, a_mul)
    for k in ("S", "P", "ref32", "low", "low_flush"):
        setattr(r, k, _rows(getattr(r, k)))
    return r


# ------------------------------------------------------------------------------------------------------------------------ vs_cnx_block
# C, HW, B.  The apply launch gives a workgroup 128 consecutive pixels and ONE GRN scale row: frames of 128 k pixels are what it supports.
CNX_SHAPES = [(96, 128, 2), (96, 256, 3), (192, 128, 3), (192, 1024, 1)]
# frames that are no multiple of 128 pixels: two frames per workgroup / a boundary in the middle of one.  vs_cnx_block_supported refuses them
CNX_STRADDLE = [(96, 64, 4), (96, 192, 4), (192, 32, 4), (192, 96, 4)]
FRAME_FACTOR = (1.0, 3.0, 0.25, -2.0)
SCALE_PAD = 8                 # scale_ld = 4C + SCALE_PAD
NSEL = 4                      # one-hot selections of W2 that together show all 4C hidden channels


@functools.lru_cache(maxsize=None)
def cnx_operands(C, HW, B):
    seed, rows, H4 = 8000 + C + HW, B * HW, 4 * C
    k = torch.arange(H4, dtype=torch.float32)
    ramp = 0.25 + 3.75 * k / (H4 - 1)
    g = torch.Generator().manual_seed(seed + 9)
    return SimpleNamespace(
        C=C, HW=HW, B=B, rows=rows, tn=R.hard_rows(rows, C, seed), w1=R.hard_weights(H4, C, 1, seed + 1), b1=R.hard_bias(H4, seed + 2),
        w2=R.hard_weights(C, H4, 1, seed + 3), beta=R.hard_bias(H4, seed + 4), bias2=R.hard_bias(C, seed + 5), res=R.hard_rows(rows, C, seed + 6),
        scale=(torch.tensor([FRAME_FACTOR[b % 4] for b in range(B)])[:, None] * ramp[None]).contiguous(),
        gamma=(0.5 * torch.randn(H4, generator=g)).clamp_min(-0.75))


def cnx_randn_operands(C=96, HW=128, B=2):
    """operands of the older parity tests: randn activations, randn / sqrt(K) weights (the frame-dependent scale kept)"""
    o, g = cnx_operands(C, HW, B), torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return SimpleNamespace(C=C, HW=HW, B=B, rows=o.rows, tn=rn(o.rows, C), w1=rn(4 * C, C, 1, 1) / C ** 0.5, b1=0.3 * rn(4 * C),
                           w2=rn(C, 4 * C, 1, 1) / (4 * C) ** 0.5, beta=0.3 * rn(4 * C), bias2=0.3 * rn(C), res=rn(o.rows, C), scale=o.scale, gamma=o.gamma)


def one_hot_w2(C, sel):
    """row n selects hidden channel k_n = sel C + n with a power of two (exact in f16)"""
    w = torch.zeros(C, 4 * C, 1, 1)
    n = torch.arange(C)
    w[n, sel * C + n, 0, 0] = 2.0 ** ((n % 3) - 1).float()
    return w


def scale_rows_of(scale, HW, rows):
    return scale[torch.arange(rows) // HW]


def neighbour_frame_rows(scale, HW, rows):
    """DEFECT: the last 32 pixels of every 128-pixel group read the scale row of the next frame (the last frame: of the previous one)"""
    p = torch.arange(rows)
    f = p // HW
    B = scale.shape[0]
    other = torch.where(f + 1 < B, f + 1, f - 1).clamp_min(0)
    return scale[torch.where(p % 128 >= 96, other, f)]


def cnx_first(o, drop_tail=False):
    """pwconv1 + GELU and the statistics launch.  DEFECT drop_tail: l_a h_w dropped on the last k-step (16 channels) of pwconv1"""
    r = gemm_stage(o.tn, o.w1, A_MUL)
    S1 = r.S
    if drop_tail:
        S1 = S1 - r.acc * _rows(F.conv2d(r.la[:, -16:], r.hw[:, -16:]))
    f = SimpleNamespace(u1=R.U32 * (r.P + o.b1.double().abs()), w_mul=r.w_mul)
    f.g = gelu64(S1 + o.b1.double())
    f.g32 = R.one_thread(lambda: F.gelu(r.ref32 + o.b1))
    G, H4 = o.rows // 32, 4 * o.C
    f.part = (f.g * f.g).view(G, 32, H4).sum(1)
    d = GELU_LIP * f.u1
    f.part_unit = R.U32 * f.part + (2.0 * f.g.abs() * d + d * d).view(G, 32, H4).sum(1)
    f.part32 = R.one_thread(lambda: (f.g32 * f.g32).view(G, 32, H4).sum(1))
    return f


def cnx_second(o, f, w2, *, rows64=None, rows32=None, u_scale=None, bias2=None, res=None, zero=None, want_ref=True):
    """GRN apply, second split, pwconv2 (+ bias2 + res).  rows64 / rows32: the [rows, 4C] scale of the reference / the yardstick (default: o.scale
    by frame); u_scale: the unit of a scale that was itself computed; zero: (pixel, channel) of a planted overflow, taken out of the emulation"""
    if rows64 is None:
        rows64 = scale_rows_of(o.scale, o.HW, o.rows)
    rows32 = rows64.float() if rows32 is None else rows32
    v = f.g * rows64.double() + o.beta.double()
    u_v = GELU_LIP * rows64.double().abs() * f.u1 + (f.g.abs() * u_scale if u_scale is not None else 0.0)
    fmt = U22 * v.abs() + U25 / A_MUL_GRN
    if zero is not None:
        v[zero] = 0.0
    r = gemm_stage(v.float(), w2, A_MUL_GRN)
    e = SimpleNamespace(low=r.low, low_flush=r.low_flush, w_mul=r.w_mul, v=v)
    b2 = torch.zeros(o.C) if bias2 is None else bias2
    rs = torch.zeros(o.rows, o.C) if res is None else res
    e.S = r.S + b2.double() + rs.double()
    e.unit = R.U32 * (r.P + b2.double().abs() + rs.double().abs()) + (u_v + fmt) @ w2.double().abs()[:, :, 0, 0].t()
    if want_ref:
        v32 = R.one_thread(lambda: f.g32 * rows32 + o.beta)
        if zero is not None:
            v32[zero] = 0.0
        e.ref = R.one_thread(lambda: gemm_stage(v32, w2, A_MUL_GRN).ref32 + b2 + rs)
    return e


def swap_in_k_group(w2):
    """DEFECT: hidden channels 0 and 1 (v = 0, 1 of k(s = 0, half = 0, v)) exchanged in the packed W2"""
    w = w2.clone()
    w[:, [0, 1]] = w2[:, [1, 0]]
    return w


def grn_scale64(part, gamma, B, unit_part=None):
    """scale = 1 + gamma Gx / (mean_c Gx + 1e-6) from [groups][4C] partial sums, in part's dtype; with unit_part the first-order unit of scale"""
    ss = part.view(B, -1, part.shape[1]).sum(1)
    gx = ss.sqrt()
    m = gx.mean(1, keepdim=True) + 1e-6
    scale = 1 + gamma.to(part.dtype) * (gx / m)
    if unit_part is None:
        return scale
    u_ss = unit_part.view(B, -1, part.shape[1]).sum(1)
    u_gx = torch.where(gx > 0, u_ss / (2 * gx).clamp_min(R.TINY), u_ss.sqrt())
    u = gamma.double().abs() * (u_gx / m + gx * u_gx.mean(1, keepdim=True) / (m * m)) + R.U32 * (1 + (gamma.double() * gx / m).abs())
    return scale, u


def cnx_block_operands(C, HW, B):
    """the whole-block operands: the last frame all zeros (B > 1), the one before it of magnitude 1e-3, the others hard"""
    o = cnx_operands(C, HW, B)
    tn = o.tn.clone().view(B, HW, C)
    tn[max(B - 2, 0)] = 1e-3 * torch.randn(HW, C, generator=torch.Generator().manual_seed(5))
    if B > 1:
        tn[B - 1] = 0.0
    q = SimpleNamespace(**vars(o))
    q.tn = tn.view(o.rows, C).contiguous()
    return q


def overflow_plant(o, f):
    """(frame, channel, pixel, scale entry): ONE hidden element pushed beyond the f16 range through its scale entry -- the channel of frame 0
    whose largest |gelu| stands out most from the second largest"""
    g0 = f.g[: o.HW].abs()
    top = g0.topk(2, dim=0).values
    k = int(torch.where(top[0] >= 1.0, top[0] / top[1].clamp_min(R.TINY), torch.zeros_like(top[0])).argmax())
    assert top[0, k] >= 1.0 and top[0, k] > 1.2 * top[1, k]
    s = 1.1 * F16_OVERFLOW / float(top[0, k]) + abs(float(o.beta[k])) / float(top[0, k])
    p = int(g0[:, k].argmax())
    assert abs(float(f.g[p, k]) * s + float(o.beta[k])) >= F16_OVERFLOW and float(top[1, k]) * s + abs(float(o.beta[k])) < 65000.0
    return 0, k, p, s


# ------------------------------------------------------------------------------------------------------------------------ vs_resblock_thin
RB_FORMS = [(16, 2, 1), (16, 2, 4), (16, 2, 12), (16, 2, 16), (16, 3, 1), (16, 3, 4), (16, 3, 12), (16, 3, 16), (32, 2, 32), (32, 2, 20)]   # C, arith, Cin
RB_SMALL = [(2, 1, 1), (2, 1, 17), (2, 9, 1), (2, 8, 16), (2, 7, 15), (2, 17, 33)]          # B, H, W: the tile is 8 x 16
# many small frames of 3 x 5 (ragged) tiles: 360 and 540 tiles, more than one and more than two per CU of an MI355X (256) at a fifth of the pixels of a
# single large map.  16 channels (two workgroups per CU) walk 1 and 2 tiles, 32 channels 2 and 3: runs of 2 cross tile rows (5 tiles) and frames (15)
RB_LARGE = [(24, 17, 65), (36, 17, 65)]
T_LIMIT = 1900.0


@functools.lru_cache(maxsize=None)
def rb_operands(C, Cin, B, H, W):
    """hard operands; w0 scaled by a power of two so that |conv0| <= T_LIMIT (|t| * 16 < 65504 with any bias used here)"""
    seed = 9000 + 31 * C + Cin + H * W
    x = R.hard_act(B, Cin, H, W, seed)
    w0, b0 = R.hard_weights(C, Cin, 3, seed + 1), R.hard_bias(C, seed + 2)
    m = float(F.conv2d(x.double(), w0.double(), padding=2).abs().max())
    if m > T_LIMIT:
        w0 = w0 * 2.0 ** math.floor(math.log2(T_LIMIT / m))
    return SimpleNamespace(C=C, Cin=Cin, B=B, H=H, W=W, x=x, w0=w0, b0=b0, w1=R.hard_weights(C, C, 3, seed + 3), b1=R.hard_bias(C, seed + 4),
                           wr=R.hard_weights(C, Cin, 1, seed + 5), br=R.hard_bias(C, seed + 6))


def rb_randn_operands(C=16, Cin=16, B=2, H=17, W=33):
    g = torch.Generator().manual_seed(31 + Cin)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return SimpleNamespace(C=C, Cin=Cin, B=B, H=H, W=W, x=rn(B, Cin, H, W), w0=rn(C, Cin, 3, 3) / (Cin * 9) ** 0.5, b0=0.3 * rn(C),
                           w1=rn(C, C, 3, 3) / (C * 9) ** 0.5, b1=0.3 * rn(C), wr=rn(C, Cin, 1, 1) / Cin ** 0.5, br=0.3 * rn(C))


def tap_identity(C, tap):
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), tap // 3, tap % 3] = 1.0
    return w


def with_t_observable(o, tap=4):
    """w1 = identity on one tap, b1 = 0, wr = 0, br = 0: out = t (tap 4) or t shifted by one pixel, the image border reading t's padding"""
    q = SimpleNamespace(**vars(o))
    q.w1, q.b1, q.wr, q.br = tap_identity(o.C, tap), torch.zeros(o.C), torch.zeros_like(o.wr), torch.zeros(o.C)
    return q


def with_positive_ring(o):
    """b0 so large that conv0 of zero-padded data is clearly positive on the ring outside the image"""
    q = SimpleNamespace(**vars(o))
    s0 = F.conv2d(o.x.double(), o.w0.double(), padding=2)
    ring = torch.ones_like(s0, dtype=torch.bool)
    ring[:, :, 1:-1, 1:-1] = False
    q.b0 = (s0.abs() * ring).amax(dim=(0, 2, 3)).float() + 1.0
    return q


def _ring_mask(t):
    m = torch.zeros_like(t, dtype=torch.bool)
    m[:, :, 1:-1, 1:-1] = True
    return m


def rb_chain(o, arith, *, padded_conv0=False, halo_shift=False, zero=None, want_ref=True):
    """the whole ResnetBlock.  t lives on the (H + 2) x (W + 2) domain conv1 reads; outside the image it is exactly 0.
    DEFECTS: padded_conv0 = t outside the image taken as conv0 of zero-padded data; halo_shift = the halo ring of every 8 x 16 tile's t read one
    pixel to the right.  zero: (b, c, y, x) of a planted overflow of t, taken out of the emulation"""
    bc = lambda b: b.view(1, -1, 1, 1)          # noqa: E731
    r0 = stage(o.x, o.w0, arith, A_MUL, pad=2)
    inside = _ring_mask(r0.S)
    t = F.relu(r0.S + bc(o.b0.double()))
    u_t = R.U32 * (r0.P + bc(o.b0.double().abs()))
    if not padded_conv0:
        t = t * inside
    u_t = u_t * inside
    fmt = (U22 * t.abs() + U25 / A_MUL) * inside if arith == 2 else torch.zeros_like(t)
    if zero is not None:
        t[zero[0], zero[1], zero[2] + 1, zero[3] + 1] = 0.0
    rr = stage(o.x, o.wr, arith, A_MUL)
    e = SimpleNamespace(t=t[:, :, 1:-1, 1:-1])
    if halo_shift:
        S1, P1 = _conv1_by_tiles(t.float(), o.w1, arith), None
    else:
        r1 = stage(t.float(), o.w1, arith, A_MUL)
        S1, P1 = r1.S, r1.P
    e.S = F.relu(S1 + bc(o.b1.double())) + rr.S + bc(o.br.double())
    if P1 is not None:
        e.unit = (R.U32 * (P1 + bc(o.b1.double().abs()) + rr.P + bc(o.br.double().abs())) + F.conv2d(u_t + fmt, o.w1.double().abs()))
    if want_ref and not halo_shift:
        t32 = R.one_thread(lambda: F.relu(r0.ref32 + bc(o.b0)) * inside)
        if zero is not None:
            t32[zero[0], zero[1], zero[2] + 1, zero[3] + 1] = 0.0
        e.ref = R.one_thread(lambda: F.relu(stage(t32, o.w1, arith, A_MUL).ref32 + bc(o.b1)) + (rr.ref32 + bc(o.br)))
    return e


def _conv1_by_tiles(t_ext, w1, arith, TH=8, TW=16):
    """DEFECT emulation: conv1 tile by tile, the one-pixel halo ring of each tile's 10 x 18 piece of t taken from one pixel to the right"""
    B, C, He, We = t_ext.shape
    H, W = He - 2, We - 2
    shifted = torch.roll(t_ext, -1, dims=3)
    out = torch.zeros(B, w1.shape[0], H, W, dtype=torch.float64)
    for y0 in range(0, H, TH):
        for x0 in range(0, W, TW):
            h, w = min(TH, H - y0), min(TW, W - x0)
            piece = shifted[:, :, y0:y0 + h + 2, x0:x0 + w + 2].clone()
            piece[:, :, 1:-1, 1:-1] = t_ext[:, :, y0 + 1:y0 + h + 1, x0 + 1:x0 + w + 1]
            out[:, :, y0:y0 + h, x0:x0 + w] = stage(piece, w1, arith, A_MUL).S
    return out


def rb_overflow_operands(o):
    """one element of t beyond 65520 / 16: every |x| clamped to 1000, one spike of 4000 under the largest weight of conv0, w0 and b0 rescaled so that
    this t is 4300 and every other one stays below 4094.  Returns (operands, (b, c, y, x) of the element)"""
    q = SimpleNamespace(**vars(o))
    x = o.x.clamp(-1000.0, 1000.0)
    n, ci, ky, kx = [int(i) for i in torch.unravel_index(o.w0.abs().argmax(), o.w0.shape)]
    sgn = 1.0 if float(o.w0[n, ci, ky, kx]) > 0 else -1.0
    ty, tx = min(o.H - 1, o.H // 2), min(o.W - 1, o.W // 2)
    sy, sx = ty + ky - 1, tx + kx - 1
    if not (0 <= sy < o.H and 0 <= sx < o.W):
        return None, None
    x[0, ci, sy, sx] = 4000.0 * sgn
    t = F.relu(F.conv2d(x.double(), o.w0.double(), padding=1) + o.b0.double().view(1, -1, 1, 1))
    top = t.flatten().topk(2).values
    if not (float(t[0, n, ty, tx]) == float(top[0]) and top[0] > 1.2 * top[1]):
        return None, None
    f = 4300.0 / float(top[0])
    q.x, q.w0, q.b0 = x.contiguous(), o.w0 * f, o.b0 * f
    return q, (0, n, ty, tx)
