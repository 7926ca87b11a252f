"""The 2 x 2 blocked gather of the Upsample groups (csrc/upconv_gather.h) against the per-pixel form it replaces, bit for bit.

vs_upconv_gather_ln and phase 3 of vs_upconv_fused produce the four output pixels of a low-resolution cell from 49 shared z loads; every pixel
still receives its own 36 terms in the per-pixel order, so the outputs must be IDENTICAL (compared as bit patterns: a flipped sign of zero
counts) to the per-pixel kernels, which the development switch UPCONV_FORM = 1 selects.  The shapes walk every border case (1-wide
maps, first / last row and column in one cell, odd sizes, more than one workgroup) and every channel-group / lanes-per-pixel pair; the smallest
real level (32 x 32 x 64) has an edge cell in every wave.  Correctness against torch and fp64 is the business of test_gpu_kernels.py and
test_gpu_fwd_envelope.py, which run the blocked form by default."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._guards import _guarded, _guards_intact  # noqa: E402
from tests._gpu import Eng, dv, to_nhwc  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd.engine import ConvW, pack_conv  # noqa: E402

DEV = "cuda"
NAN = float("nan")
KEY = "UPCONV_FORM"          # VS_DBG_UPCONV_FORM (csrc/vs_common.h): 1 = per-pixel form, 0 = 2 x 2 blocks

# (B, H, W, Co), wide leading dimensions in every second case
GATHER_SHAPES = [(1, 1, 1, 16), (2, 1, 4, 16), (2, 2, 3, 16), (1, 3, 2, 32), (2, 4, 4, 64), (1, 5, 7, 32), (1, 8, 8, 128), (1, 32, 32, 64)]
GATHER_CASES = [(s, i % 2 == 1) for i, s in enumerate(GATHER_SHAPES)]
ACTS = [N.ACT_RELU, N.ACT_SILU]      # what engine.py / model_api.hip pass (unet.py:61-62)
# (B, H, W, C1, C2, Co)
FUSED_SHAPES = [(1, 1, 1, 16, 16, 16), (2, 3, 5, 16, 16, 16), (1, 8, 8, 32, 32, 16), (1, 9, 17, 32, 32, 16), (1, 8, 8, 64, 64, 32)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gather_inputs(shape, wide):
    """z [B*H*W, z_ld] random normal with exact +0 / -0 entries, one all-zero source pixel and one all-negative one; LayerNorm vectors"""
    B, H, W, Co = shape
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Co)
    z_ld, out_ld = 9 * Co + (8 if wide else 0), Co + (4 if wide else 0)
    z = torch.randn(B * H * W, z_ld, generator=g)
    flat = z.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[: max(4, flat.numel() // 50)]
    flat[idx[0::2]] = 0.0
    flat[idx[1::2]] = -0.0
    z[0, :] = -0.0
    z[-1, :] = -z[-1, :].abs() - 0.5
    lw, lb = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g)
    assert torch.isfinite(z).all()
    return z, lw, lb, z_ld, out_ld


def _gather(L, z, z_ld, shape, lw, lb, act, out, out_ld, form):
    B, H, W, Co = shape
    with N.debug(KEY, form):
        N.check(L.vs_upconv_gather_ln(N.ptr(z), z_ld, B, H, W, Co, N.ptr(lw), N.ptr(lb), 1e-6, act, N.ptr(out), out_ld, N.stream()), "upconv_gather_ln")
        torch.cuda.synchronize()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,wide", GATHER_CASES)
def test_gather_blocked_equals_per_pixel(shape, wide, act):
    L = N.lib()
    B, H, W, Co = shape
    z, lw, lb, z_ld, out_ld = _gather_inputs(shape, wide)
    zd, lwd, lbd = dv(z), dv(lw), dv(lb)
    outs = []
    for form in (0, 1):
        out = torch.full((B * 4 * H * W, out_ld), -3.0, device=DEV)
        _gather(L, zd, z_ld, shape, lwd, lbd, act, out, out_ld, form)
        outs.append(out)
    assert torch.isfinite(outs[1][:, :Co]).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))        # pad lanes (still -3) included
    if out_ld > Co:
        assert bool((outs[0][:, Co:] == -3.0).all())


@pytest.mark.parametrize("shape,wide", GATHER_CASES)
def test_gather_blocked_with_red_zones(shape, wide):
    """NaN bands around z and the LayerNorm vectors, sentinels around out: the four stores per thread stay inside the tensor and no clamped
    source address leaves z (a NaN read into an accumulator would show in the comparison with the unguarded launch)"""
    L = N.lib()
    B, H, W, Co = shape
    z, lw, lb, z_ld, out_ld = _gather_inputs(shape, wide)
    plain = torch.full((B * 4 * H * W, out_ld), -3.0, device=DEV)
    _gather(L, dv(z), z_ld, shape, dv(lw), dv(lb), N.ACT_RELU, plain, out_ld, 0)
    zbuf, zg = _guarded(z.to(DEV), NAN)
    wbuf, wg = _guarded(lw.to(DEV), NAN)
    bbuf, bg = _guarded(lb.to(DEV), NAN)
    obuf, og = _guarded(torch.full((B * 4 * H * W, out_ld), -3.0, device=DEV), -7.0)
    _gather(L, zg, z_ld, shape, wg, bg, N.ACT_RELU, og, out_ld, 0)
    assert _guards_intact(obuf, -7.0)
    assert _guards_intact(zbuf, NAN) and _guards_intact(wbuf, NAN) and _guards_intact(bbuf, NAN)
    assert torch.equal(_bits(og), _bits(plain))


def test_gather_blocked_is_deterministic():
    L = N.lib()
    shape = (2, 4, 4, 64)
    B, H, W, Co = shape
    z, lw, lb, z_ld, out_ld = _gather_inputs(shape, False)
    zd, lwd, lbd = dv(z), dv(lw), dv(lb)
    a = torch.full((B * 4 * H * W, out_ld), -3.0, device=DEV)
    b = torch.full((B * 4 * H * W, out_ld), 5.0, device=DEV)
    _gather(L, zd, z_ld, shape, lwd, lbd, N.ACT_RELU, a, out_ld, 0)
    _gather(L, zd, z_ld, shape, lwd, lbd, N.ACT_RELU, b, out_ld, 0)
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("arith", [2, 3])
@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_fused_blocked_equals_per_pixel(shape, arith):
    B, H, W, C1, C2, Co = shape
    eng = Eng(arith=arith)
    L, st = eng.lib, N.stream()
    assert L.vs_upconv_fused_supported(C1, C2, Co) == 1
    g = torch.Generator().manual_seed(77 + H * W + Co)
    x, sk = torch.randn(B, C1, H, W, generator=g), torch.randn(B, C2, H, W, generator=g)
    x[:, :, 0, 0] = 0.0                                   # a source pixel whose nine products are exact zeros
    w = torch.randn(Co, C1 + C2, 3, 3, generator=g) / math.sqrt(9 * (C1 + C2))
    lw, lb = dv(torch.rand(Co, generator=g) + 0.5), dv(torch.randn(Co, generator=g))
    xa, sa = to_nhwc(x), to_nhwc(sk)
    wz, cpz = pack_conv(w.to(DEV).permute(2, 3, 0, 1).reshape(9 * Co, C1 + C2)[:, :, None, None], C1 + C2)
    cw = ConvW(wz, None, 9 * Co, 1, 1, cpz).with_split(arith)
    outs = []
    for form in (0, 1):
        obuf, og = _guarded(torch.full((B * 4 * H * W, Co), -3.0, device=DEV), -7.0)
        with N.debug(KEY, form):
            N.check(L.vs_upconv_fused(N.ptr(xa.t), C1, xa.ld, N.ptr(sa.t), C2, sa.ld, 2 ** -0.5, N.ptr(cw.split), B, H, W, Co, N.ptr(lw), N.ptr(lb),
                                      1e-6, N.ACT_RELU, N.ptr(og), Co, arith, 16.0, 1.0 / (16.0 * cw.w_mul), st), "upconv_fused")
            torch.cuda.synchronize()
        assert _guards_intact(obuf, -7.0)
        outs.append(og)
    assert torch.isfinite(outs[1]).all() and bool((outs[1] != -3.0).any())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
