"""fp64 envelopes of the pixel-wise head (csrc/pixel_head.hip) and of vs_matmul_small (csrc/bwd_ops.hip): float64 references, hard inputs, metrics
and the case lists shared by tests/test_pixel_contract_cpu.py (the references agree with torch modules and the oracle, seeded defects fall outside;
no GPU) and tests/test_gpu_pixel_envelope.py (every kernel against them, between red zones).

The rule and its helpers are tests/_envelope.py's.  Two metrics:
    sums of products (vs_pixel_linear in front of the sigmoid, its dx / dw / db, vs_matmul_small, the raw mode of vs_pixel_upgather and
    vs_pixel_upgather_bwd): S = the float64 result, P = the float64 sum of the magnitudes of its terms, r = |got - S| / (2^-24 P) per element,
    no element left out (`units`, floor 1); an element with P = 0 has no non-zero term and must be exactly 0.  The yardstick is the same
    operation in ATen float32 on one thread.
    normalised or squashed outputs (vs_pixel_upgather with LayerNorm + GELU, vs_pixel_linear with the sigmoid): `group_err` per pixel resp. per
    channel plane against float64, floor 2^-24; the yardstick is F.layer_norm + F.gelu resp. torch.sigmoid in float32.  The constant pixels --
    every pixel of the constant frame -- are a class of their own, as the constant BatchNorm channel of tests/_unet_ref.py.
vs_pixel_vote counts: bit for bit against torch on the same values.
A plain CPU module: torch and the standard library only."""
import functools
import math

import torch
import torch.nn.functional as F

from tests._envelope import U32, check_rows, check_units, group_err, one_thread

# Twice the largest ratio measured on an MI355X over every case of tests/test_gpu_pixel_envelope.py (profiles/pixel_fp64_envelope.txt lists them),
# never more than 8: a kernel that needs more has a defect.
PIXEL_MARGIN = 5.43            # 2 x 2.713, the largest ratio measured: LayerNorm + GELU of vs_pixel_upgather at Co = 20 (two lanes of 12 floats, masked vectors), x2, 2 x 2 latent, hard frame (2.9e-6 against ATen's 1.1e-6)
WIDTH = 78
envelope = functools.partial(check_rows, "PIXEL-ENVELOPE", WIDTH, "aten-fp32", PIXEL_MARGIN)
envelope_units = functools.partial(check_units, "PIXEL-ENVELOPE", WIDTH, PIXEL_MARGIN)
LN_EPS = 1e-6

F64, F32 = torch.float64, torch.float32


def both(fn):
    """(float64 reference, fp32 yardstick) of fn(dtype), ATen on one thread"""
    return one_thread(lambda: (fn(F64), fn(F32)))


F32_MIN_NORMAL = 2.0 ** -126


def units(got, ref, mag, nterms=0):
    """worst |got - ref| in units of 2^-24 * mag (mag = the sum of the magnitudes of the terms of each output); where mag is zero the output has no
    non-zero term and must be exactly zero (inf otherwise; a NaN anywhere gives NaN, which no comparison admits).  nterms: the number of terms of
    an output whose terms may lie below fp32's smallest normal number (gradients behind a saturated sigmoid, y (1 - y) down to 1e-38): below it
    the format itself has no 24 bits, so each term adds 2^-126 to the unit"""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    d = (got - ref).abs()
    unit = U32 * mag.clamp_min(1e-300) + nterms * F32_MIN_NORMAL
    u = torch.where(mag > 0, d / unit, torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return float("nan") if bool(torch.isnan(u).any()) else float(u.max())


# ------------------------------------------------------------------------------------------------------------------------ hard inputs
def hard_rows(rows, C, seed):
    """[rows][C] float32 in the vocabulary of _envelope.hard_matrix(..., "rows") for any size: rows of mean 30 / std 0.5; row 1 constant 30.25;
    row 2 with a single 4e3 outlier channel; row 3 of magnitude 1e-3; row 4 exact zeros (each where the matrix has that row)"""
    g = torch.Generator().manual_seed(seed)
    x = 30.0 + 0.5 * torch.randn(rows, C, generator=g)
    tiny = 1e-3 * torch.randn(C, generator=g)
    if rows > 1:
        x[1] = 30.25
    if rows > 2:
        x[2, C // 2] = 4e3
    if rows > 3:
        x[3] = tiny
    if rows > 4:
        x[4] = 0.0
    return x


def hard_weights(K, C, seed):
    """[K][C] randn / sqrt(C); row 1 scaled by 1e-3, row 3 exact zeros (with hard_bias's zero at 3: an output whose terms are all zero)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(K, C, generator=g) / math.sqrt(C)
    if K > 1:
        w[1] *= 1e-3
    if K > 3:
        w[3] = 0.0
    return w


def hard_bias(K, seed):
    """element k: zero (k % 3 == 0), 1e-3 randn (1), randn (2), as _split_ref.hard_bias"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(K, generator=g)
    k = torch.arange(K)
    return torch.where(k % 3 == 0, torch.zeros(K), torch.where(k % 3 == 1, 1e-3 * b, b))


# ------------------------------------------------------------------------------------------------------------------------ per-pixel linear layer
LIN_B = 2
# (C, K, H, W, sigmoid, ld - C): the smallest shapes that reach every instantiation behind vs_pixel_linear / vs_pixel_linear_bwd (read from the
# dispatch in csrc/pixel_head.hip; nout = K (C / 4 + 1)):
LIN_CASES = [
    (16, 6, 12, 20, False, 0),        # pixel_linear_kernel<4,4>, bwd_x<4>,  wgrad<2> (nout 30), 2 workgroups
    (24, 17, 5, 7, True, 0),          # <8,1> (HW odd), bwd_x<8>, wgrad<2> (nout 119), 1 workgroup with a ragged last tile (70 rows)
    (32, 65, 8, 12, False, 0),        # <8,4>, bwd_x<8>, wgrad<4> (nout 585)
    (32, 129, 8, 12, True, 0),        # <8,4>, bwd_x<8>, wgrad<8> (nout 1161)
    (32, 257, 8, 12, False, 0),       # <8,4>, bwd_x<8>, wgrad<20> (nout 2313)
    (48, 17, 6, 10, True, 0),         # <16,1> (C > 32 although HW % 4 == 0), bwd_x<16>, wgrad<2> (nout 221)
    (64, 33, 5, 7, False, 0),         # <16,1>, bwd_x<16>, wgrad<4> (nout 561)
    (8, 3, 257, 257, False, 0),       # <4,1>, bwd_x<4>, wgrad<2>: 132098 rows, the 512-workgroup cap (LIN_CAP)
    (24, 6, 12, 20, True, 4),         # <6,4>, ld = C + 4 with NaN in the pad lanes of x
]
LIN_CAP = LIN_CASES[7]
DP_KINDS = ("positive", "cancelling")
LIN_TILE_ROWS = 32


def lin_name(case):
    C, K, H, W, sig, pad = case
    return f"C{C}-K{K}-{H}x{W}-{'sig' if sig else 'raw'}" + (f"-ld{C + pad}" if pad else "")


def lin_plan(rows, partial_floats, K, C):
    """(workgroups, rows per workgroup, first workgroup without rows) of the weight-gradient kernel from the size of its workspace, by the rule in
    the header of pixel_linear_wgrad_kernel: part is [workgroups][K][C + 4]; a workgroup takes a fixed range of rows in tiles of 32, at least eight
    tiles per workgroup, at most 512 workgroups"""
    assert partial_floats > 0 and partial_floats % (K * (C + 4)) == 0, (partial_floats, K, C)
    nb = partial_floats // (K * (C + 4))
    assert nb == min(512, -(-rows // (8 * LIN_TILE_ROWS))), (nb, rows)
    rpb = -(-(-(-rows // nb)) // LIN_TILE_ROWS) * LIN_TILE_ROWS
    return nb, rpb, -(-rows // rpb)


def lin_partial_floats(rows, K, C):
    """the rule itself (what vs_pixel_linear_bwd_partial_floats answers), for the CPU contract test"""
    return min(512, -(-rows // (8 * LIN_TILE_ROWS))) * K * (C + 4)


@functools.lru_cache(maxsize=None)
def lin_inputs(case):
    """x [B HW][C] hard rows, w [K][C], bias [K]"""
    C, K, H, W, sig, pad = case
    seed = 3100 + 7 * C + K + H * W
    return hard_rows(LIN_B * H * W, C, seed), hard_weights(K, C, seed + 1), hard_bias(K, seed + 2)


def lin_dpreds(case, kind):
    """[B][K][HW]: `positive` = sigmoid(z) / rows, every term of one sign (what the detection loss gives under an all-zero mask); `cancelling` =
    sigmoid(z) - t for random bits t.  Plane K - 1 of frame 0 and the last pixel of the last frame are exact zeros"""
    C, K, H, W, sig, pad = case
    g = torch.Generator().manual_seed(3200 + 7 * C + K + H * W + DP_KINDS.index(kind))
    s = torch.sigmoid(2.0 * torch.randn(LIN_B, K, H * W, generator=g))
    dp = s / (LIN_B * H * W) if kind == "positive" else s - torch.randint(0, 2, s.shape, generator=g).float()
    dp[0, K - 1] = 0.0
    dp[-1, :, -1] = 0.0
    return dp


def lin_fwd(x, w, b, sig, B):
    """[B][K][HW]: pixel_decoder.py:53, 78-83 (Conv2d 1x1 on NHWC rows, optional sigmoid)"""
    v = (x @ w.t() + b).view(B, -1, w.shape[0]).permute(0, 2, 1)
    return torch.sigmoid(v) if sig else v


def lin_fwd_mag(x, w, b, B):
    return lin_fwd(x.double().abs(), w.double().abs(), b.double().abs(), False, B)


@functools.lru_cache(maxsize=None)
def lin_fwd_ref(case):
    """(float64, fp32 yardstick, P) of the forward; with the sigmoid P is None (group_err)"""
    C, K, H, W, sig, pad = case
    x, w, b = lin_inputs(case)
    r64, r32 = both(lambda dt: lin_fwd(x.to(dt), w.to(dt), b.to(dt), sig, LIN_B))
    return r64, r32, (None if sig else lin_fwd_mag(x, w, b, LIN_B))


def lin_y(case):
    """the sigmoid output the backward is GIVEN (its contract: d logit = dpreds * y (1 - y) from that y): the float64 forward rounded to fp32"""
    return lin_fwd_ref(case)[0].float() if case[4] else None


def lin_dlogit(dp, y, *, no_yprime=False, shift_frame=False):
    """[B HW][K]: dpreds, times y (1 - y) behind a sigmoid output.  DEFECTS for the teeth test: no_yprime = the factor omitted; shift_frame = the
    frame of row r taken as r >> floor(log2(HW)) in place of r / HW (the same thing only where HW is a power of two)"""
    d = dp if (y is None or no_yprime) else dp * y * (1 - y)
    B, K, HW = d.shape
    if shift_frame:
        r = torch.arange(B * HW)
        b = (r >> int(math.floor(math.log2(HW)))).clamp_max(B - 1)
        return d[b, :, r % HW]
    return d.permute(0, 2, 1).reshape(B * HW, K)


def lin_bwd(dp, y, x, w, **defect):
    """(dx [rows][C], dw [K][C], db [K]): autograd of lin_fwd written out.  dw and db are ONE product, d^T [x | 1] (the kernel's extra column),
    also in the yardstick"""
    d = lin_dlogit(dp, y, **defect)
    wb = d.t() @ torch.cat((x, torch.ones(x.shape[0], 1, dtype=x.dtype)), 1)
    return d @ w, wb[:, :-1], wb[:, -1]


def lin_bwd_ref(case, kind, **defect):
    """((dx, dw, db) float64, the same in fp32, their magnitudes P -- for `units` together with lin_bwd_terms); a defect enters the fp32 side only"""
    x, w, b = lin_inputs(case)
    dp, y = lin_dpreds(case, kind), lin_y(case)
    r64, r32 = both(lambda dt: lin_bwd(dp.to(dt), None if y is None else y.to(dt), x.to(dt), w.to(dt), **(defect if dt == F32 else {})))
    d = lin_dlogit(dp.double(), None if y is None else y.double()).abs()
    return r64, r32, (d @ w.double().abs(), d.t() @ x.double().abs(), d.sum(0))


def lin_bwd_terms(case):
    """terms per output of (dx, dw, db), for `units`: behind the sigmoid the gradients reach below fp32's smallest normal number"""
    C, K, H, W, sig, pad = case
    return (K, LIN_B * H * W, LIN_B * H * W) if sig else (0, 0, 0)


def lin_wgrad_emulated(d, x, nb, rpb, *, drop_tile_last_row=False, nan_empty=False):
    """(dw, db) float32 the way the kernel partitions the sum: workgroup i adds rows [i rpb, (i + 1) rpb) in fp32, the workgroups are added in
    ascending order in double.  DEFECTS for the teeth test: drop_tile_last_row = row 31 of every 32-row tile left out; nan_empty = a workgroup
    without rows leaves its partial as the workspace held it (NaN) in place of writing zeros"""
    rows, K = d.shape
    xp = torch.cat((x, torch.ones(rows, 1)), 1)
    total = torch.zeros(K, xp.shape[1], dtype=F64)
    for i in range(nb):
        lo, hi = i * rpb, min((i + 1) * rpb, rows)
        if lo >= hi:
            part = torch.full((K, xp.shape[1]), float("nan") if nan_empty else 0.0)
        else:
            keep = torch.arange(lo, hi)
            if drop_tile_last_row:
                keep = keep[(keep - lo) % LIN_TILE_ROWS != LIN_TILE_ROWS - 1]
            part = d[keep].t() @ xp[keep]
        total += part.double()
    out = total.float()
    return out[:, :-1], out[:, -1]


# ------------------------------------------------------------------------------------------------------------------------ Upsample group
UP_B = 2
UP_COS = (4, 8, 20, 24, 64, 256)         # lanes per pixel x floats per lane (upgather_split): 1x4, 1x8, 2x12 (masked vectors), 2x12, 4x16, 16x16
UP_FS = (2, 4)
UP_LATENTS = ((2, 2), (3, 5), (2, 9))
UP_CASES = [(Co, f, H, W, 0) for Co in UP_COS for f in UP_FS for (H, W) in UP_LATENTS] + [(20, 4, 3, 5, 8)]      # last field: z_ld / out_ld above the minimum
UP_CLASSES = ("hard", "const")           # frame 0 | frame 1


def up_name(case):
    Co, f, H, W, pad = case
    return f"Co{Co}-x{f}-{H}x{W}" + (f"-ld+{pad}" if pad else "")


def up_axis(n, f, dtype=F64):
    """[3][f n][n]: row Y of matrix k holds the bilinear weights (nn.Upsample(scale_factor=f), align_corners=False: source index
    max((d + 0.5) / f - 0.5, 0), upper neighbour clamped) with which tap k of a 3-tap window around Y reads the n source rows behind
    ReflectionPad2d(1): d = reflect(Y + k - 1).  All weights are multiples of 1 / (2 f): exact in any float format"""
    m = torch.zeros(3, f * n, n, dtype=dtype)
    for k in range(3):
        for Y in range(f * n):
            d = Y + k - 1
            d = -d if d < 0 else (2 * f * n - 2 - d if d >= f * n else d)
            s = max((d + 0.5) / f - 0.5, 0.0)
            i0 = min(int(s), n - 1)
            i1 = min(i0 + 1, n - 1)
            m[k, Y, i0] += 1.0 - (s - i0)
            m[k, Y, i1] += s - i0
    return m


def up_gather(z, H, W, Co, f):
    """raw gather [B][fH][fW][Co] of z [B][H][W][9 Co] (columns (tap, channel)):
    conv3x3(pad(up_f(v)))[Y, X, c] = sum_t up_f(z_t)[refl(Y + ky - 1), refl(X + kx - 1), c]"""
    B = z.shape[0]
    return torch.einsum("kYy,lXx,byxklc->bYXc", up_axis(H, f, z.dtype), up_axis(W, f, z.dtype), z.reshape(B, H, W, 3, 3, Co))


def up_gather_adjoint(dg, H, W, Co, f):
    """dz [B][H][W][9 Co]: the transpose of up_gather's own matrix applied to dg [B][fH][fW][Co]"""
    B = dg.shape[0]
    return torch.einsum("kYy,lXx,bYXc->byxklc", up_axis(H, f, dg.dtype), up_axis(W, f, dg.dtype), dg).reshape(B, H, W, 9 * Co)


def up_norm(raw, lw, lb, *, tanh_gelu=False, unbiased=False):
    """GELU(LayerNorm over Co) (common.py:45-52, 147-155: biased variance).  DEFECTS for the teeth test: tanh_gelu = the tanh approximation;
    unbiased = the variance divided by Co - 1"""
    Co = raw.shape[-1]
    if unbiased:
        mean = raw.mean(-1, keepdim=True)
        v = (raw - mean) / torch.sqrt(raw.var(-1, unbiased=True, keepdim=True) + LN_EPS) * lw + lb
    else:
        v = F.layer_norm(raw, (Co,), lw, lb, LN_EPS)
    return F.gelu(v, approximate="tanh" if tanh_gelu else "none")


@functools.lru_cache(maxsize=None)
def up_inputs(case):
    """z [B][H][W][9 Co]: frame 0 = hard pixels (mean 30 / std 0.5, one constant pixel, one with a single 4e3 outlier, one of magnitude 1e-3) with
    channel Co - 1 of every tap exactly zero (an output without a non-zero term); frame 1 = the constant 30.25 (every output pixel of it is a
    constant pixel: variance exactly 0, all sums exact in fp32).  LayerNorm weight and bias.  dg [B][fH][fW][Co]: hard pixels, frame 1 with
    random signs (cancelling sums), channel 0 exactly zero"""
    Co, f, H, W, pad = case
    seed = 3300 + 11 * Co + 5 * f + 31 * H + W
    g = torch.Generator().manual_seed(seed)
    z = torch.empty(UP_B, H, W, 9 * Co)
    z[0] = hard_rows(H * W, 9 * Co, seed + 1).view(H, W, 9 * Co)
    z[0].view(H, W, 9, Co)[..., Co - 1] = 0.0
    z[1] = 30.25
    lw, lb = 1 + 0.3 * torch.randn(Co, generator=g), 0.3 * torch.randn(Co, generator=g)
    dg = hard_rows(UP_B * f * H * f * W, Co, seed + 2).view(UP_B, f * H, f * W, Co)
    dg[1] = dg[1] * (2.0 * torch.randint(0, 2, dg[1].shape, generator=g).float() - 1.0)
    dg[..., 0] = 0.0
    return z, lw, lb, dg


@functools.lru_cache(maxsize=None)
def up_ref(case):
    """raw: (float64, fp32, P); out: (float64, fp32) of LayerNorm + GELU; adj: (float64, fp32, P)"""
    Co, f, H, W, pad = case
    z, lw, lb, dg = up_inputs(case)
    raw = both(lambda dt: up_gather(z.to(dt), H, W, Co, f)) + (up_gather(z.double().abs(), H, W, Co, f),)
    out = both(lambda dt: up_norm(up_gather(z.to(dt), H, W, Co, f), lw.to(dt), lb.to(dt)))
    adj = both(lambda dt: up_gather_adjoint(dg.to(dt), H, W, Co, f)) + (up_gather_adjoint(dg.double().abs(), H, W, Co, f),)
    return dict(raw=raw, out=out, adj=adj)


def up_class_rows(name, got, r64, r32):
    """envelope rows of a [B][fH][fW][Co] result, one per pixel class (frame 0: hard, frame 1: constant), groups = pixels"""
    got, r64, r32 = got.detach().cpu(), r64.detach().cpu(), r32.detach().cpu()
    return [(f"{name}/{cls}", group_err(got[b], r64[b], -1), group_err(r32[b], r64[b], -1)) for b, cls in enumerate(UP_CLASSES)]


# ------------------------------------------------------------------------------------------------------------------------ vs_matmul_small
MM_CASES = [(17, 130, 3), (1, 257, 5), (5, 130, 257), (1, 1, 1)]         # M, N, K
MM_PAD = (4, 3, 5)                                                      # lda - K, ldb - N, ldc - N


@functools.lru_cache(maxsize=None)
def mm_inputs(case):
    """A [M][K] hard rows; B [K][N] randn / sqrt(K) with column 1 exactly zero (an output without a non-zero term) and column 2 scaled by 1e-5"""
    M, N, K = case
    g = torch.Generator().manual_seed(3400 + M + 3 * N + 7 * K)
    Bm = torch.randn(K, N, generator=g) / math.sqrt(K)
    if N > 1:
        Bm[:, 1] = 0.0
    if N > 2:
        Bm[:, 2] *= 1e-5
    return hard_rows(M, K, 3401 + M + 3 * N + 7 * K), Bm


@functools.lru_cache(maxsize=None)
def mm_ref(case):
    A, Bm = mm_inputs(case)
    return both(lambda dt: A.to(dt) @ Bm.to(dt)) + (A.double().abs() @ Bm.double().abs(),)


# ------------------------------------------------------------------------------------------------------------------------ vs_pixel_vote
VOTE_CASES = [(2, 3, 35), (3, 5, 323)]                                  # B, K, HW: odd maps, below and above one pass of 256 threads
VOTE_THRESHOLDS = (0.0, 0.25)


def vote_inputs(B, K, HW, thr):
    """logits [B][K][HW]: randn, and in turn exactly the threshold (no vote: `>`), one ulp below and above it, +0.0 and -0.0; masks [B][HW]: ones,
    and in turn 0.0 and -0.0 (not selected), 0.3, the smallest denormal and its negative (selected)"""
    g = torch.Generator().manual_seed(3500 + B + K + HW)
    t = torch.tensor(thr, dtype=F32)
    inf = torch.tensor(float("inf"))
    special = torch.stack([t, torch.nextafter(t, -inf), torch.nextafter(t, inf), torch.tensor(0.0), torch.tensor(-0.0)])
    x = torch.randn(B * K * HW, generator=g)
    idx = torch.arange(0, x.numel(), 2)
    x[idx] = special[(idx // 2) % len(special)]
    mvals = torch.tensor([0.0, -0.0, 0.3, 2.0 ** -149, -(2.0 ** -149), 1.0, 1.0])
    # 7 mask values against 5 logit values on every other element: every pair meets
    m = mvals[torch.arange(B * HW) % len(mvals)]
    return x.view(B, K, HW), m.view(B, HW)


def vote_ref(logits, masks, thr):
    """(votes [B][K], nsel [B]) int64 by torch on the same values: evals/metrics.py:150-206 (`preds > threshold`, `masks.bool()`)"""
    sel = torch.ones(logits.shape[0], logits.shape[2], dtype=torch.bool) if masks is None else masks != 0
    return ((logits > thr) & sel[:, None, :]).sum(-1), sel.sum(-1)
