"""fp64 envelopes of the FORWARD normalisation, GRN and attention kernels: formulas, hard inputs, cases and the metric shared by
tests/test_fwd_contract_cpu.py (the envelope has teeth; no GPU) and tests/test_gpu_fwd_envelope.py (every kernel against it).

As in the backward envelopes (tests/test_gpu_bwd.py; the rule and its helpers are tests/_envelope.py's): the reference is the formula in float64 on the CPU
from the same fp32 input values, the error is taken PER GROUP -- max |got - ref| over the group / max |ref| over the group, worst group: a row
(pixel) for LayerNorm and RMSNorm, a (frame, channel) element for the GRN scale, a (token, head) slice of hd values for attention -- and the
yardstick is the same formula in float32 on the CPU (one thread), written out the way the modelled project writes it (common.py:147-179,
vit.py:302-360), NOT a fused ATen kernel such as F.layer_norm, whose cascade summation is a stricter algorithm than the one specified.
A kernel may exceed the yardstick by FWD_FP64_MARGIN; no element is excluded from any case."""
import functools
import math

import torch
import torch.nn.functional as F

from tests._envelope import check_rows, cpu_autograd, group_err, hard_matrix

# Twice the largest ratio hip / max(aten-fp32, 2^-24) measured on an MI355X over every case of tests/test_gpu_fwd_envelope.py
# (profiles/fwd_fp64_envelope.txt lists them), never more than 8: a kernel that needs more has a defect.
FWD_FP64_MARGIN = 5.76         # 2 x 2.882, the largest ratio measured: vs_layernorm_act small<16> at rows = 301, C = 50, no activation (one thread adds the row's 50 values in order)
EPS = 1e-6
envelope = functools.partial(check_rows, "FWD-ENVELOPE", 58, "aten-fp32", FWD_FP64_MARGIN)


def ACT(act):
    return {0: lambda v: v, 1: F.relu, 2: F.gelu, 4: F.silu}[act]


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm(x, w, b, act=0, *, one_pass=False, div=None):
    """common.py:147-155 over the last dim, in x's dtype.  DEFECTS for the teeth test: one_pass = variance as E[x^2] - E[x]^2;
    div = the variance's divisor (a kernel that divides by ld instead of C)"""
    C = x.shape[-1]
    u = x.mean(-1, keepdim=True)
    if one_pass:
        s = (x * x).mean(-1, keepdim=True) - u * u
    else:
        s = (x - u).pow(2).mean(-1, keepdim=True)
    if div is not None:
        s = s * (C / div)
    return ACT(act)(w * ((x - u) / torch.sqrt(s + EPS)) + b)


def ln_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)


def ln_ref(x, w, b, act=0, **defect):
    """(float64 reference, float32 yardstick) of layernorm on CPU tensors; with a defect keyword: (reference, defective fp32 emulation)"""
    return cpu_autograd(lambda dt: layernorm(x.to(dt), w.to(dt), b.to(dt), act, **_fp32_only(dt, defect)))


# vs_layernorm_act: (tag, rows, C, ld, forced wave-per-row).  out_ld = ld.  Rows 37 / 301: the last workgroup is ragged in every form
# (256 rows per workgroup thread-per-row, 256 / LPP in the lanes forms, 4 wave-per-row)
LN_LANES = [("lanes<8,4>", 301, 96, 96), ("lanes<16,4>", 37, 192, 192), ("lanes<32,4>", 37, 384, 384), ("lanes<64,4>", 37, 768, 768),
            ("lanes<64,12>", 37, 1100, 1104)]
LN_CASES = ([("small<4>", 301, 14, 16, 0), ("small<8>", 37, 18, 20, 0), ("small<16>", 301, 50, 52, 0)]
            + [(t, r, c, ld, 0) for t, r, c, ld in LN_LANES]
            + [("wave", 37, 130, 160, 0)]
            + [("wave forced, shape of " + t, r, c, ld, 1) for t, r, c, ld in LN_LANES])
LN_ACTS = (0, 2)               # none, GELU
PATCH_CASES = [(2, 5, 7, 96), (1, 5, 7, 724)]          # B, H, W, C of vs_layernorm_patch2x2: an odd map, lanes <8,4> and <64,4>


def ln_inputs(rows, C):
    return (hard_matrix(rows, C, 700 + C, "rows"),) + ln_params(C, 701 + C)


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm behind a producer
def _fp32_only(dt, defect):
    return defect if dt == torch.float32 else {}


def _unit_sum_weights(shape, g, zero=True):
    """weights whose taps sum to about 1 per output channel (1 / K each, times 1 + 0.5 randn: the sum is 1 +- 0.5 / sqrt(K)); zero: output channel
    1 exactly zero.  A map of mean 30 / std 0.5 comes out of the conv as rows that sit near 30 with a spread of about a unit -- the shifted
    rows on which a LayerNorm goes wrong.  (Zero-mean weights would give rows of mean ~0 and std ~30: not hard.)  The zero channel adds one
    entry near 0 to every row, i.e. a spread of 30 / sqrt(Co): over 96 or 128 channels the row stays hard, over the 16 or 32 of the up-conv
    levels it does not (the conv's own fp32 rounding then costs as much as a one-pass variance), which is why those cases run in both variants"""
    K = shape[1] * shape[2] * shape[3]
    w = (1 + 0.5 * torch.randn(shape, generator=g)) / K
    if zero:
        w[1] = 0.0
    return w


def _shifted(shape, g, const_frame):
    """activations of mean 30 / std 0.5, frame `const_frame` the constant 30.25"""
    x = 30.0 + 0.5 * torch.randn(shape, generator=g)
    if const_frame is not None:
        x[const_frame] = 30.25
    return x


DW_CASES = [(96, 16, 16), (130, 17, 50), (24, 9, 13), (128, 16, 16), (126, 16, 16)]
# (C, H, W) by the dispatch of dwconv7_ln_any: H W < 256, or a channel stride that no tile's chunk divides -> the row kernel (96: register-resident
# LayerNorm branch, C % 4 == 0; 130: loop branch; 24: four lanes per pixel); H W >= 256 and ld % 128 == 0 -> the tiled kernel <4, 8, 128, 256>
# (128: register-resident; 126 = ld 128: loop branch).  Both branches, with 4 and 8 lanes per pixel; NOT reached by these maps: the 16- / 32- /
# 64-lane instantiations (768-channel stage, two-row strips) and the tile without room for the affine parameters in LDS (WLDS = false)


def dw_inputs(C, H, W):
    """x [2, C, H, W] of mean 30 / std 0.5 with frame 1 constant, depthwise taps that sum to about 1 per channel (1/49 + noise), channel 1 with
    taps exactly zero, bias and LayerNorm parameters"""
    g = torch.Generator().manual_seed(800 + C + H)
    x = _shifted((2, C, H, W), g, 1)
    wd = 1.0 / 49 + 0.01 * torch.randn(C, 1, 7, 7, generator=g)
    wd[1] = 0.0
    bd = 0.1 * torch.randn(C, generator=g)
    return (x, wd, bd) + ln_params(C, 801 + C)


def dw_ref(x, wd, bd, lw, lb, **defect):
    """[B, H, W, C]: depthwise 7x7 + LayerNorm (convnext.py:43-46); a defect keyword of `layernorm` applies to the fp32 run only"""
    C = x.shape[1]
    return cpu_autograd(lambda dt: layernorm(F.conv2d(x.to(dt), wd.to(dt), bd.to(dt), padding=3, groups=C).permute(0, 2, 3, 1), lw.to(dt), lb.to(dt),
                                             **_fp32_only(dt, defect)))


STEM_CASES = [(4, 96, 20), (2, 96, 20), (4, 128, 20), (2, 128, 20)]      # stride, Co, S


def stem_inputs(stride, Co, S):
    g = torch.Generator().manual_seed(900 + stride + Co)
    x = _shifted((2, 3, S, S + 4), g, 1)
    w = _unit_sum_weights((Co, 3, 4, 4), g)
    b = 0.2 * torch.randn(Co, generator=g)
    return (x, w, b) + ln_params(Co, 901 + Co)


def stem_ref(x, w, b, lw, lb, stride, **defect):
    return cpu_autograd(lambda dt: layernorm(F.conv2d(x.to(dt), w.to(dt), b.to(dt), stride=stride).permute(0, 2, 3, 1), lw.to(dt), lb.to(dt),
                                             **_fp32_only(dt, defect)))


UPCONV_SHAPES = [(2, 24, 8, 7, 9, 16), (1, 48, 16, 9, 17, 32)]          # B, C1, C2, H, W, Co (tests/test_gpu_kernels.py)
UPCONV_CASES = [(s, z) for s in UPCONV_SHAPES for z in (True, False)]    # (shape, one output channel with zero weights?)


def upconv_inputs(B, C1, C2, H, W, Co, zero=True):
    g = torch.Generator().manual_seed(1000 + C1 + Co)
    x, sk = _shifted((B, C1, H, W), g, B - 1 if B > 1 else None), _shifted((B, C2, H, W), g, B - 1 if B > 1 else None)
    w = _unit_sum_weights((Co, C1 + C2, 3, 3), g, zero)
    return (x, sk, w) + ln_params(Co, 1001 + Co)


def upconv_ref(x, sk, w, lw, lb, act, f=2, skip_scale=2 ** -0.5, **defect):
    """[B, fH, fW, Co]: bilinear x f -> ReflectionPad2d(1) -> Conv3x3 (no bias) -> LayerNorm -> act (common.py:45-52); sk = None: no concat"""
    def fn(dt):
        v = x.to(dt) if sk is None else torch.cat((x.to(dt), sk.to(dt) * skip_scale), 1)
        up = F.interpolate(v, scale_factor=f, mode="bilinear", align_corners=False)
        cv = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w.to(dt))
        return layernorm(cv.permute(0, 2, 3, 1), lw.to(dt), lb.to(dt), act, **_fp32_only(dt, defect))
    return cpu_autograd(fn)


PIXEL_CASE = (64, 16, 4, 2, 2)          # C, Co, f, H, W: the smallest stage of tests/test_gpu_pixel_head.py


def pixel_inputs(C, Co, f, H, W, zero=True):
    g = torch.Generator().manual_seed(1100 + C + Co)
    x = _shifted((2, C, H, W), g, 1)
    w = _unit_sum_weights((Co, C, 3, 3), g, zero)
    return (x, w) + ln_params(Co, 1101 + Co)


# ------------------------------------------------------------------------------------------------------------------------ RMSNorm
RMS_CASES = [(37, 20), (301, 132), (37, 320)]          # rows, C: 4 / 16 / 64 lanes per row
RMS_ZERO_ROW, RMS_TINY_ROW = 4, 5


def rms_inputs(rows, C):
    """hard rows + one all-zero row (the max(||x||, 1e-12) clamp: the output equals `add` exactly) + one row of 1e-20 (x^2 underflows)"""
    g = torch.Generator().manual_seed(1200 + C)
    x = hard_matrix(rows, C, 1201 + C, "rows")
    x[RMS_ZERO_ROW] = 0.0
    x[RMS_TINY_ROW] = 1e-20
    return x, torch.rand(C, generator=g) + 0.5, torch.randn(rows, C, generator=g)


def rmsnorm(x, gamma, add, act=4):
    """common.py:172-179 + activation + residual branch"""
    return ACT(act)(F.normalize(x, dim=1) * x.shape[1] ** 0.5 * gamma) + add


def rms_ref(x, gamma, add):
    return cpu_autograd(lambda dt: rmsnorm(x.to(dt), gamma.to(dt), add.to(dt)))


# ------------------------------------------------------------------------------------------------------------------------ GRN
GRN_CASES = [(1, 37, 18, 20), (7, 43, 130, 160), (1, 67, 1100, 1104), (2, 67, 600, 608)]
# B, HW, C, ld: grn_finish_kernel<2,16> twice, <8,4> (C > 1024), <4,8> (512 < C <= 1024); 37 / 43 rows: one ragged 64-row chunk, 67: a full one + 3 rows


def grn_inputs(B, HW, C, seed=1300):
    g = torch.Generator().manual_seed(seed + C)
    # gamma >= -0.75: most channels have Gx / mean = 1, and 1 + gamma there must not cancel to nothing -- an element whose VALUE is 1e-4 of its
    # terms measures the cancellation (in fp32 as in any kernel), not the reduction under test
    gamma = (0.5 * torch.randn(C, generator=g)).clamp_min(-0.75)
    return hard_matrix(B * HW, C, seed + 1 + C, "cols").view(B, HW, C), gamma, 0.3 * torch.randn(C, generator=g)


def grn_scale(h, gamma, *, div=None):
    """[B, C]: 1 + gamma Gx / (mean_c Gx + 1e-6) (common.py:166-168).  DEFECT: div = the divisor of the mean over channels (ld instead of C)"""
    gx = torch.norm(h, p=2, dim=1, keepdim=True)
    m = gx.mean(dim=-1, keepdim=True) if div is None else gx.sum(dim=-1, keepdim=True) / div
    return (1 + gamma * (gx / (m + 1e-6)))[:, 0]


def grn_ref(h, gamma, **defect):
    return cpu_autograd(lambda dt: grn_scale(h.to(dt), gamma.to(dt), **(defect if dt == torch.float32 else {})))


def grn_partials32(h):
    """frame-major fp32 partials [B][HW / 32][C] of vs_grn_scale_from_partials: per 32-row group the sum of squares, rows added in ascending order"""
    B, HW, C = h.shape
    sq = (h * h).view(B, HW // 32, 32, C)
    s = torch.zeros(B, HW // 32, C)
    for r in range(32):
        s = s + sq[:, :, r]
    return s.contiguous()


def grn_straddle_partials32(h):
    """[groups][2][C] of vs_grn_scale_from_straddle_partials: 32-row groups of the B HW rows; slot 0 = the rows in the frame of the group's first
    row, slot 1 = those in the next frame; rows added in ascending order"""
    B, HW, C = h.shape
    rows = B * HW
    flat = h.reshape(rows, C)
    ng = (rows + 31) // 32
    p = torch.zeros(ng, 2, C)
    for r in range(rows):
        gi = r // 32
        slot = 0 if r // HW == (gi * 32) // HW else 1
        p[gi, slot] = p[gi, slot] + flat[r] * flat[r]
    return p.contiguous()


# ------------------------------------------------------------------------------------------------------------------------ attention
# (B, H, W, heads, hd, win), relative-position tables?, kernel the default dispatch takes
ATTN_VALU_CASES = [((3, 8, 8, 2, 16, 4), True), ((1, 8, 12, 3, 32, 0), True), ((3, 8, 8, 2, 16, 4), False)]
ATTN_MFMA_CASES = [((1, 8, 8, 2, 16, 0), True), ((1, 8, 16, 2, 32, 0), True), ((1, 16, 16, 1, 64, 0), True), ((2, 16, 16, 2, 32, 8), True),
                   ((1, 8, 8, 2, 16, 0), False)]
LOGIT_STD = 40.0
UNIFORM_QUERY = 5


def _vkind(head, heads):
    return (head + (1 if heads == 1 else 0)) % 3


def attn_inputs(cfg, rel=True):
    """qkv [B, H, W, 3 D] and the tables (or None, None).  Per group of tokens: q, k = sqrt(40) randn, so the logits have std 40 -- most of them
    within +-40, the row maxima near +100: a peaked, nearly one-hot softmax whose exp overflows without the maximum subtracted; query 5 of
    every group is zero in head 0 (every logit exactly 0: uniform softmax, the result is the mean of V -- a zero query also zeroes its
    relative-position terms, so the uniform row of the cases with tables does not exercise those; the peaked rows do); where there is more than one group, the keys of the
    last head of group 0 are all identical (every query there sees one key vector: uniform up to the position terms); V by head: mean 30 / std 0.5 (kind 0), magnitude 1e-4 (kind 1: the low bf16 planes carry it), randn (kind 2) -- a single
    head takes kind 1"""
    B, H, W, heads, hd, win = cfg
    D = heads * hd
    Th, Tw = (win, win) if win else (H, W)
    g = torch.Generator().manual_seed(1400 + sum(cfg))
    nwy, nwx = H // Th, W // Tw
    Bw, T = B * nwy * nwx, Th * Tw
    x = torch.randn(Bw, T, 3, heads, hd, generator=g)
    x[:, :, :2] *= math.sqrt(LOGIT_STD)
    x[:, UNIFORM_QUERY, 0, 0] = 0.0
    if Bw > 1:
        x[0, :, 1, heads - 1] = x[0, 0, 1, heads - 1].clone()
    for h in range(heads):
        k = _vkind(h, heads)
        if k == 0:
            x[:, :, 2, h] = 30.0 + 0.5 * x[:, :, 2, h]
        elif k == 1:
            x[:, :, 2, h] *= 1e-4
    qkv = x.view(B, nwy, nwx, Th, Tw, 3 * D).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, 3 * D).contiguous()
    if not rel:
        return qkv, None, None
    return qkv, 0.3 * torch.randn(2 * Th - 1, hd, generator=g), 0.3 * torch.randn(2 * Tw - 1, hd, generator=g)


def randn_attn_inputs(cfg):
    """the inputs of tests/test_gpu_kernels.py::test_vit_attention (randn qkv, logits O(1))"""
    B, H, W, heads, hd, win = cfg
    D = heads * hd
    g = torch.Generator().manual_seed(43)
    qkv = torch.randn(B, H, W, 3 * D, generator=g)
    Th, Tw = (win, win) if win else (H, W)
    return qkv, 0.3 * torch.randn(2 * Th - 1, hd, generator=g), 0.3 * torch.randn(2 * Tw - 1, hd, generator=g)


def _bf16_plane(p):
    """the first (truncated) bf16 plane of an fp32 tensor, as conv_common.h::split4 forms it"""
    return (p.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _bf16_two_planes(p):
    """the first two of the three planes: the low plane (bits 2^-17 and below of the value) is flushed"""
    h = _bf16_plane(p)
    return h + _bf16_plane(p - h)


def attention(qkv, rel_h, rel_w, cfg, mode="softmax"):
    """[B, H, W, heads, hd]: vit.py:302-360 (scaled q.k^T + decomposed relative positions, softmax, @ v) incl. the window partition, the
    expression of tests/test_gpu_kernels.py::test_vit_attention, in qkv's dtype.  DEFECTS for the teeth test (mode): "nomax" = softmax
    without the maximum subtracted; "nocorr" = online softmax over the keys whose accumulator misses the rescale by exp(m_old - m_new);
    "plane" = un-normalised probabilities cut to one bf16 plane in front of the product with V, "plane2" = to two (the low plane flushed)"""
    B, H, W, heads, hd, win = cfg
    D = heads * hd
    Th, Tw = (win, win) if win else (H, W)
    x = qkv
    if win:
        x = x.view(B, H // win, win, W // win, win, 3 * D).permute(0, 1, 3, 2, 4, 5).reshape(-1, win, win, 3 * D)
    Bw = x.shape[0]
    q, k, v = x.reshape(Bw, Th * Tw, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, Bw * heads, Th * Tw, hd).unbind(0)
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    if rel_h is not None:
        Rh = rel_h[torch.arange(Th)[:, None] - torch.arange(Th)[None, :] + Th - 1]
        Rw = rel_w[torch.arange(Tw)[:, None] - torch.arange(Tw)[None, :] + Tw - 1]
        rq = q.reshape(Bw * heads, Th, Tw, hd)
        attn = (attn.view(Bw * heads, Th, Tw, Th, Tw) + torch.einsum("bhwc,hkc->bhwk", rq, Rh)[:, :, :, :, None]
                + torch.einsum("bhwc,wkc->bhwk", rq, Rw)[:, :, :, None, :]).view(Bw * heads, Th * Tw, Th * Tw)
    if mode == "softmax":
        o = attn.softmax(-1) @ v
    elif mode == "nomax":
        p = attn.exp()
        o = (p @ v) / p.sum(-1, keepdim=True)
    elif mode in ("plane", "plane2"):
        p = (attn - attn.amax(-1, keepdim=True)).exp()
        o = ((_bf16_plane(p) if mode == "plane" else _bf16_two_planes(p)) @ v) / p.sum(-1, keepdim=True)
    elif mode == "nocorr":
        m = torch.full(attn.shape[:2], -math.inf, dtype=attn.dtype)
        l, acc = torch.zeros_like(m), torch.zeros_like(q)
        for j in range(attn.shape[-1]):
            s = attn[:, :, j]
            mn = torch.maximum(m, s)
            corr, p = (m - mn).exp(), (s - mn).exp()
            l = l * corr + p
            acc = acc + p[:, :, None] * v[:, j:j + 1]          # DEFECT: acc * corr[:, :, None] + ...
            m = mn
        o = acc / l[:, :, None]
    else:
        raise ValueError(mode)
    o = o.view(Bw, heads, Th, Tw, hd).permute(0, 2, 3, 1, 4).reshape(Bw, Th, Tw, D)
    if win:
        o = o.view(B, H // win, W // win, win, win, D).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, D)
    return o.reshape(B, H, W, heads, hd)


def attn_ref(qkv, rel_h, rel_w, cfg, mode="softmax"):
    def fn(dt):
        c = lambda t: None if t is None else t.to(dt)          # noqa: E731
        return attention(c(qkv), c(rel_h), c(rel_w), cfg, mode if dt == torch.float32 else "softmax")
    return cpu_autograd(fn)


def attn_lines(got, r64, r32, heads):
    """envelope lines of one attention case: every (token, head) group, and per head (whose V differ in kind) on its own"""
    rows = [("o/tok-head", group_err(got, r64, -1), group_err(r32, r64, -1))]
    for h in range(heads):
        rows.append((f"o/head{h}", group_err(got[..., h, :], r64[..., h, :], -1), group_err(r32[..., h, :], r64[..., h, :], -1)))
    return rows
