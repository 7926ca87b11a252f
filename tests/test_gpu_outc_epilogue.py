"""vs_resblock_thin with the U-Net's last layer in its epilogue (csrc/resblock_thin.hip, descriptor members outc_w / outc_b / out_ch / use_tanh /
delta): `outc` (1x1, 16 -> out_ch <= 4) + tanh on the accumulator registers of the last thin ResnetBlock, whose own 16-channel output is then not
stored.  The contract is bit equality with the two launches it replaces (vs_resblock_thin + vs_outc_tanh): same products, same accumulation order
(channels ascending, fused multiply-add from 0, bias, tanhf).  Ragged tiles on both axes, a single tile, more tiles than workgroups walk at once,
1 - 4 output channels, tanh on / off, both operand splits; red zones around every operand, two runs."""
import ctypes as C
import math

import pytest
import torch

from tests._gpu import DEV, NAN, Eng, conv_weights, dv
from tests._guards import _guarded, _guards_intact
from videoseal_amd import native as N
from videoseal_amd.engine import Act

pytestmark = pytest.mark.gpu

SHAPES = [(2, 24, 40), (1, 8, 16), (3, 37, 29)]          # (B, H, W): 8 x 16 tiles -> ragged on both axes / exactly one tile / ragged + odd


def _block(arith, cin, seed):
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn(16, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    w1 = torch.randn(16, 16, 3, 3, generator=g) / math.sqrt(16 * 9)
    wr = torch.randn(16, cin, 1, 1, generator=g) / math.sqrt(cin)
    b0, b1, br = (torch.randn(16, generator=g) * 0.3 for _ in range(3))
    return dict(c0=conv_weights(w0, b0, cin), c1=conv_weights(w1, b1, 16), res=conv_weights(wr, br, cin), cout=16)


def _run(e, xa, p, ow, ob, out_ch, use_tanh, fused):
    """delta [B][out_ch][H][W] (CPU) from the one-launch form or from vs_resblock_thin + vs_outc_tanh; the output sits between guard bands"""
    L, st = e.lib, N.stream()
    dbuf, delta = _guarded(torch.full((xa.B, out_ch, xa.H, xa.W), 9.0, device=DEV), -7.0)
    if fused:
        assert e.resblock_thin(xa, p, "oe", outc=(ow, ob, out_ch, use_tanh, delta)) is None
    else:
        obuf, o = _guarded(torch.full((xa.B, xa.H, xa.W, 16), 9.0, device=DEV), -7.0)
        e.resblock_thin(xa, p, "oe", out=Act(o, xa.B, xa.H, xa.W, 16, 16))
        N.check(L.vs_outc_tanh(N.ptr(o), xa.H * xa.W, xa.B, 16, 16, N.ptr(ow), N.ptr(ob), out_ch, use_tanh, N.ptr(delta), st), "vs_outc_tanh")
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, -7.0), "damaged band around delta"
    assert fused or _guards_intact(obuf, -7.0), "damaged band around the block's output"
    return delta.cpu().clone()


@pytest.mark.parametrize("use_tanh", [0, 1])
@pytest.mark.parametrize("cfg", [(2, 1, 16), (2, 3, 16), (2, 4, 12), (3, 1, 16), (3, 3, 16)], ids=lambda c: f"arith{c[0]}-out{c[1]}-cin{c[2]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_outc_epilogue_equals_the_two_launches_bit_for_bit(shape, cfg, use_tanh):
    (B, H, W), (arith, out_ch, cin) = shape, cfg
    e = Eng(arith=arith)
    g = torch.Generator().manual_seed(100 * H + W + out_ch)
    xbuf, xv = _guarded(torch.randn(B, H, W, cin, generator=g).to(DEV), NAN)
    xa = Act(xv, B, H, W, cin, cin)
    p = _block(arith, cin, 7 + cin)
    assert e._thin_ok(xa, p, None)
    ow = dv(torch.randn(out_ch, 16, generator=g) * 0.25)
    ob = dv(torch.randn(out_ch, generator=g) * 0.1)
    ref = _run(e, xa, p, ow, ob, out_ch, use_tanh, fused=False)
    got = _run(e, xa, p, ow, ob, out_ch, use_tanh, fused=True)
    again = _run(e, xa, p, ow, ob, out_ch, use_tanh, fused=True)
    assert _guards_intact(xbuf, NAN)
    assert not torch.isnan(ref).any() and float(ref.abs().max()) > 0.1 and (not use_tanh or float(ref.abs().max()) < 1.0)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert torch.equal(again, got)


def test_outc_epilogue_over_a_persistent_walk():
    """more tiles than the persistent grid has workgroups (2 per CU): every workgroup walks several tiles across rows and frames"""
    B, H, W, out_ch = 5, 104, 176, 3                  # 5 x 13 x 11 = 715 tiles
    e = Eng(arith=2)
    g = torch.Generator().manual_seed(5)
    xa = Act(torch.randn(B, H, W, 16, generator=g).to(DEV), B, H, W, 16, 16)
    p = _block(2, 16, 3)
    ow, ob = dv(torch.randn(out_ch, 16, generator=g) * 0.25), dv(torch.randn(out_ch, generator=g) * 0.1)
    assert torch.equal(_run(e, xa, p, ow, ob, out_ch, 1, fused=True), _run(e, xa, p, ow, ob, out_ch, 1, fused=False))


def test_outc_epilogue_refuses_what_it_does_not_implement():
    """32-channel blocks and more than four output channels answer VS_ERR_UNSUPPORTED; half-set members answer VS_ERR_BAD_ARG; nothing is launched"""
    e = Eng(arith=2)
    L = e.lib
    x = torch.zeros(1, 8, 16, 32, device=DEV)
    w = torch.zeros(2 * 32 * 9 * 32, dtype=torch.int16, device=DEV)
    z = torch.zeros(64, device=DEV)
    dbuf, delta = _guarded(torch.full((1, 8, 8, 16), 9.0, device=DEV), -7.0)

    def desc(cout, ld, out_ch, **kw):
        d = N.ResblockThinDesc()
        d.x, d.x_ld, d.B, d.H, d.W, d.Cin = N.ptr(x), ld, 1, 8, 16, ld
        d.w0_split = d.w1_split = d.wr_split = N.ptr(w)
        d.arith, d.Cout, d.a_mul, d.acc_mul0, d.acc_mul1, d.acc_mulr = 2, cout, 16.0, 1.0, 1.0, 1.0
        d.outc_w, d.outc_b, d.out_ch, d.use_tanh, d.delta = N.ptr(z), N.ptr(z), out_ch, 1, N.ptr(delta)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    st = N.stream()
    assert L.vs_resblock_thin(C.byref(desc(32, 32, 1)), st) == -2
    assert L.vs_resblock_thin(C.byref(desc(16, 16, 5)), st) == -2
    assert L.vs_resblock_thin(C.byref(desc(16, 16, 0)), st) == -1
    assert L.vs_resblock_thin(C.byref(desc(16, 16, 1, outc_w=None)), st) == -1
    assert L.vs_resblock_thin(C.byref(desc(16, 16, 1, delta=None)), st) == -1          # no delta, no out
    assert L.vs_resblock_thin(C.byref(desc(16, 16, 1, delta=None, out=N.ptr(delta), out_ld=16)), st) == -1      # outc members without delta
    torch.cuda.synchronize()
    assert float(delta.min()) == 9.0 and _guards_intact(dbuf, -7.0)
