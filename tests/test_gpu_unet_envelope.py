"""fp64 envelopes and bit-for-bit checks of the U-Net glue and head kernels on hard inputs, between red zones (tests/_unet_ref.py: formulas,
inputs, cases, metrics; tests/test_unet_contract_cpu.py: the references agree with independent implementations and seeded defects fall outside).
vs_bn_batch_stats and the pair vs_bn_partial_sums -> vs_bn_finish_sums, vs_scale_shift_act, vs_upcat2x(_bwd), vs_outc_tanh(_bwd), vs_pool_linear,
vs_msg_latent, vs_msg_pre(_rows), vs_msg_table_grad, vs_reflect_fold1 and vs_col2im3x3_reflect against the formula in float64, at most UNET_MARGIN
times what the same formula costs in float32 on the CPU; vs_broadcast_channels, vs_cat2_scale, vs_im2col3x3(_strided), vs_dilate2, vs_pad_embed1 and
vs_relu_bwd bit for bit against their torch restatement.  Every input sits between NaN bands and every output between sentinel bands, every
buffer is exactly as large as the header says, pad lanes [C, ld) of the inputs are zero.  Every figure is printed as a UNET-ENVELOPE line;
profiles/unet_fp64_envelope.txt is such a run on an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _envelope as E  # noqa: E402
from tests import _unet_ref as R  # noqa: E402
from tests._gpu import Alloc  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

NAN = float("nan")


def _alloc():
    return Alloc("nan", {})


def _done(a):
    torch.cuda.synchronize()
    assert not a.intact(), f"damaged band around operand(s) {a.intact()} (in order of allocation)"


# ------------------------------------------------------------------------------------------------------------------------ BatchNorm on batch statistics
@pytest.mark.parametrize("momentum", R.BN_MOMENTA)
@pytest.mark.parametrize("rows,C,ld", R.BN_SHAPES)
def test_bn_batch_stats_fp64_envelope(rows, C, ld, momentum):
    """vs_bn_batch_stats and the pair vs_bn_partial_sums -> vs_bn_finish_sums (bit-equal to it): scale, shift and the in-place update of the running
    statistics per channel; with either running pointer NULL the other one and scale / shift keep their bits.  The constant channel: variance
    exactly 0, scale = gamma / sqrt(eps), a finite shift"""
    L, st = N.lib(), N.stream()
    x, gamma, beta, rm, rv = R.bn_inputs(rows, C)
    r64, r32 = R.bn_ref(x, gamma, beta, rm, rv, momentum)
    a = _alloc()
    xg = a.inp(R.padded(x, ld))
    gd, bd = a.inp(R.padded(gamma, ld)), a.inp(R.padded(beta, ld))
    nd = int(L.vs_bn_partial_doubles(rows, ld))

    def run(pair, with_rm=True, with_rv=True):
        rmd, rvd = a.inp(rm) if with_rm else None, a.inp(rv) if with_rv else None        # C floats each: NaN directly behind the last channel
        part, sc, sh = a.scratch(nd, torch.float64), a.out(C), a.out(C)
        if pair:
            sums = a.out(2 * ld + 1, dtype=torch.float64)
            N.check(L.vs_bn_partial_sums(N.ptr(xg), rows, C, ld, N.ptr(part), N.ptr(sums), st), "vs_bn_partial_sums")
            N.check(L.vs_bn_finish_sums(N.ptr(sums), C, ld, N.ptr(gd), N.ptr(bd), R.BN_EPS, momentum, N.ptr(rmd), N.ptr(rvd), N.ptr(sc), N.ptr(sh), st),
                    "vs_bn_finish_sums")
        else:
            N.check(L.vs_bn_batch_stats(N.ptr(xg), rows, C, ld, N.ptr(gd), N.ptr(bd), R.BN_EPS, momentum, N.ptr(rmd), N.ptr(rvd), N.ptr(part), N.ptr(sc),
                                        N.ptr(sh), st), "vs_bn_batch_stats")
        return sc, sh, rmd, rvd
    one, two = run(False), run(True)
    no_rm, no_rv = run(False, with_rm=False), run(True, with_rv=False)
    _done(a)
    for u, v in zip(one, two):
        assert torch.equal(u, v), "the pair is not bit-identical to vs_bn_batch_stats"
    assert torch.equal(no_rm[0], one[0]) and torch.equal(no_rm[1], one[1]) and torch.equal(no_rm[3], one[3])
    assert torch.equal(no_rv[0], one[0]) and torch.equal(no_rv[1], one[1]) and torch.equal(no_rv[2], one[2])
    assert all(torch.isfinite(t).all() for t in one)
    lines = [row for n, g, w, y in zip(R.BN_NAMES, one, r64, r32) for row in R.class_rows(n, g, w, y, None)]
    R.envelope(f"bn_batch_stats rows={rows} C={C} ld={ld} momentum={momentum}", lines)


# ------------------------------------------------------------------------------------------------------------------------ vs_scale_shift_act
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("rows,C,ld,add_ld,out_ld", R.SSA_SHAPES)
def test_scale_shift_act_fp64_envelope(rows, C, ld, add_ld, out_ld, act, with_add):
    """every activation code, with and without the residual branch, three different strides; scale / shift fold the hard channels' statistics, so
    x * scale (about 60; about 1e4 on the constant channel) and shift cancel to O(1); per channel, one line per channel class against the
    yardstick of that class"""
    L, st = N.lib(), N.stream()
    x, sc, sh, add = R.ssa_inputs(rows, C)
    r64, r32 = R.ssa_ref(x, sc, sh, act, add if with_add else None)
    a = _alloc()
    xg, scd, shd = a.inp(R.padded(x, ld)), a.inp(sc), a.inp(sh)
    ad = a.inp(R.padded(add, add_ld)) if with_add else None
    out = a.out(rows, out_ld)
    N.check(L.vs_scale_shift_act(N.ptr(xg), rows, C, ld, N.ptr(scd), N.ptr(shd), act, N.ptr(ad), add_ld if with_add else 0, N.ptr(out), out_ld, st),
            "vs_scale_shift_act")
    _done(a)
    assert (out[:, C:] == 3).all()                         # the kernel owns columns [0, C) of the output only
    R.envelope(f"scale_shift_act rows={rows} C={C} act={act}{' +add' if with_add else ''}", R.class_rows("y", out[:, :C], r64, r32, 0))


@pytest.mark.parametrize("rows,C,ld", R.CHAIN_SHAPES)
def test_bn_relu_add_chain_fp64_envelope(rows, C, ld):
    """vs_bn_batch_stats -> vs_scale_shift_act(ReLU, + add): the train-mode forward of a ResnetBlock against float64 relu(batch_norm(x)) + add per
    channel class.  Elements whose float64 pre-activation lies within tau of zero (R.relu_gate) may fall on either side of the ReLU and are left out:
    at most 0.1 % of them, and ATen's fp32 run takes every decision of the reference"""
    L, st = N.lib(), N.stream()
    C4 = (C + 3) // 4 * 4
    x, gamma, beta, add = R.chain_inputs(rows, C)
    (r64, pre64), (r32, pre32) = R.both(lambda dt: R.bn_relu_add(x.to(dt), gamma.to(dt), beta.to(dt), add.to(dt)))
    keep = R.relu_gate(x, gamma, beta, pre64)
    assert 1 - float(keep.mean()) <= 1e-3
    assert torch.equal(pre32 > 0, pre64 > 0)
    a = _alloc()
    xg, gd, bd, ad = a.inp(R.padded(x, ld)), a.inp(R.padded(gamma, ld)), a.inp(R.padded(beta, ld)), a.inp(R.padded(add, ld))
    part = a.scratch(int(L.vs_bn_partial_doubles(rows, ld)), torch.float64)
    sc, sh = a.out(C4), a.out(C4)
    sc[C:], sh[C:] = 0, 0                                  # vs_scale_shift_act reads whole float4 groups: the engine keeps the pad lanes zero
    out = a.out(rows, ld)
    N.check(L.vs_bn_batch_stats(N.ptr(xg), rows, C, ld, N.ptr(gd), N.ptr(bd), R.BN_EPS, 0.1, None, None, N.ptr(part), N.ptr(sc), N.ptr(sh), st), "vs_bn_batch_stats")
    N.check(L.vs_scale_shift_act(N.ptr(xg), rows, C4, ld, N.ptr(sc), N.ptr(sh), N.ACT_RELU, N.ptr(ad), ld, N.ptr(out), ld, st), "vs_scale_shift_act")
    _done(a)
    assert (out[:, C:C4] == 0).all()
    R.envelope(f"bn -> scale_shift_act relu+add rows={rows} C={C} ld={ld}", R.class_rows("y", out[:, :C], r64, r32, 0, keep))


# ------------------------------------------------------------------------------------------------------------------------ vs_upcat2x and its adjoint
@pytest.mark.parametrize("kind", R.FRAME_KINDS)
@pytest.mark.parametrize("case", R.UPCAT_CASES, ids=str)
def test_upcat2x_fp64_envelope(case, kind):
    """H = 1 / W = 1 / 2 x 2 / odd maps, every stride larger than its channel count once, both skip scales, every frame kind for x and the skip;
    in units of 2^-24 times the interpolated magnitudes (a constant frame comes back constant to within the envelope, the zeros of an impulse
    frame exactly); the pad lanes of the output are written as zeros"""
    L, st = N.lib(), N.stream()
    B, H, W, C1, C2, ld1, ld2, old, s = case
    x, sk = R.frames(kind, B, C1, H, W), R.frames(kind, B, C2, H, W, seed=1)
    r64, r32 = R.upcat_ref(x, sk, s)
    a = _alloc()
    xg, sg = a.inp(R.nhwc(x, ld1)), a.inp(R.nhwc(sk, ld2))
    out = a.out(B * 4 * H * W, old)
    N.check(L.vs_upcat2x(N.ptr(xg), C1, ld1, N.ptr(sg), C2, ld2, s, B, H, W, N.ptr(out), old, st), "vs_upcat2x")
    _done(a)
    assert (out[:, C1 + C2:] == 0).all()
    got = R.nchw(out[:, :C1 + C2].cpu(), B, 2 * H, 2 * W)
    mag = R.upcat_mag(x, sk, s)
    R.envelope_units(f"upcat2x {kind} B={B} {H}x{W} C={C1}+{C2} ld={ld1},{ld2},{old} s={s:.3f}", R.units(got, r64, mag), R.units(r32, r64, mag))


@pytest.mark.parametrize("kind", R.FRAME_KINDS)
@pytest.mark.parametrize("case", R.UPCAT_CASES, ids=str)
def test_upcat2x_bwd_fp64_envelope(case, kind):
    """the adjoint on the same shapes, the upstream gradient of every frame kind, against float64 autograd of F.interpolate(cat); units of 2^-24
    times the adjoint of the magnitudes (its weights are non-negative)"""
    L, st = N.lib(), N.stream()
    B, H, W, C1, C2, ld1, ld2, hld, s = case
    dhi = R.frames(kind, B, C1 + C2, 2 * H, 2 * W, seed=2)
    r64, r32 = R.upcat_bwd_ref(dhi, C1, s)
    m64 = R.upcat_bwd(dhi.double().abs(), C1, abs(R.f32(s)))
    a = _alloc()
    dg = a.inp(R.nhwc(dhi, hld))
    dx, dsk = a.out(B * H * W, ld1), a.out(B * H * W, ld2)
    N.check(L.vs_upcat2x_bwd(N.ptr(dg), hld, B, H, W, C1, C2, s, N.ptr(dx), ld1, N.ptr(dsk), ld2, st), "vs_upcat2x_bwd")
    _done(a)
    assert (dx[:, C1:] == 3).all() and (dsk[:, C2:] == 3).all()          # only the channels are written
    gx, gs = R.nchw(dx[:, :C1].cpu(), B, H, W), R.nchw(dsk[:, :C2].cpu(), B, H, W)
    R.envelope_units(f"upcat2x_bwd {kind} B={B} {H}x{W} C={C1}+{C2} hi_ld={hld} s={s:.3f}",
                     max(R.units(gx, r64[0], m64[0]), R.units(gs, r64[1], m64[1])), max(R.units(r32[0], r64[0], m64[0]), R.units(r32[1], r64[1], m64[1])))


# ------------------------------------------------------------------------------------------------------------------------ vs_outc_tanh and its adjoint
@pytest.mark.parametrize("use_tanh", [0, 1])
@pytest.mark.parametrize("B,rpf,C,Cout,ld", R.OUTC_CASES)
def test_outc_tanh_fp64_envelope(B, rpf, C, Cout, ld, use_tanh):
    """a channel of mean 30 whose weight the bias cancels, pre-activations over [-12, 12] (tanh saturates); planar output [B][Cout][rows per frame]"""
    L, st = N.lib(), N.stream()
    x, w, bias = R.outc_inputs(B, rpf, C, Cout)
    r64, r32 = R.outc_ref(x, w, bias, use_tanh)
    a = _alloc()
    xg, wd, bd = a.inp(R.padded(x, ld)), a.inp(w), a.inp(bias)
    out = a.out(B, Cout, rpf)
    N.check(L.vs_outc_tanh(N.ptr(xg), rpf, B, C, ld, N.ptr(wd), N.ptr(bd), Cout, use_tanh, N.ptr(out), st), "vs_outc_tanh")
    _done(a)
    got = out.cpu().permute(0, 2, 1).reshape(B * rpf, Cout)
    mag = R.outc_mag(x, w, bias, use_tanh)
    R.envelope_units(f"outc_tanh B={B} rpf={rpf} C={C} Cout={Cout} tanh={use_tanh}", R.units(got, r64, mag), R.units(r32, r64, mag))


@pytest.mark.parametrize("use_tanh", [0, 1])
@pytest.mark.parametrize("B,rpf,C,Cout,ld", R.OUTC_CASES)
def test_outc_tanh_bwd_fp64_envelope(B, rpf, C, Cout, ld, use_tanh):
    """dv = d delta (1 - delta^2) from the given fp32 delta -- on, and within a few ulp of, +-1 -- and dx = W^T dv; where delta = +-1 exactly, dv is an
    exact zero, and so is a row of dx whose delta are all +-1; columns [Cout, 4) of dv and [C, dx_ld) of dx are zeros"""
    L, st = N.lib(), N.stream()
    rows = B * rpf
    g = torch.Generator().manual_seed(rows + C)
    delta, dd, w = R.saturated_delta((B, Cout, rpf), rows + C), torch.randn(B, Cout, rpf, generator=g), torch.randn(Cout, C, generator=g)
    if rpf > 1:
        delta[:, :, 1] = torch.tensor([1.0, -1.0, 1.0, -1.0])[:Cout]      # one pixel whose outputs all sit on the ends: its dx row is exactly zero
    to_rows = lambda t: t.permute(0, 2, 1).reshape(rows, Cout)            # noqa: E731
    dl, ddl = to_rows(delta), to_rows(dd)
    r64, r32 = R.outc_bwd_ref(dl, ddl, w, use_tanh)
    mv, mx = R.outc_bwd_mag(dl, ddl, w, use_tanh)
    a = _alloc()
    deg, ddg, wd = a.inp(delta), a.inp(dd), a.inp(w)
    dx, dv = a.out(rows, ld), a.out(rows, 4)
    N.check(L.vs_outc_tanh_bwd(N.ptr(deg), N.ptr(ddg), rpf, B, C, N.ptr(wd), Cout, use_tanh, N.ptr(dx), ld, N.ptr(dv), st), "vs_outc_tanh_bwd")
    _done(a)
    assert (dv[:, Cout:] == 0).all() and (dx[:, C:] == 0).all()
    gv, gx = dv[:, :Cout].cpu(), dx[:, :C].cpu()
    if use_tanh:
        ends = dl.abs() == 1.0
        assert ends.any() and (gv[ends] == 0).all()
        if rpf > 1:
            assert ends.all(1).any() and (gx[ends.all(1)] == 0).all()
    case = f"outc_tanh_bwd B={B} rpf={rpf} C={C} Cout={Cout} tanh={use_tanh}"
    R.envelope_units(case + " dv", R.units(gv, r64[0], mv), R.units(r32[0], r64[0], mv))
    R.envelope_units(case + " dx", R.units(gx, r64[1], mx), R.units(r32[1], r64[1], mx))


# ------------------------------------------------------------------------------------------------------------------------ vs_pool_linear
@pytest.mark.parametrize("B,HW,C,ld,Nn,onehot", R.POOL_CASES)
def test_pool_linear_fp64_envelope(B, HW, C, ld, Nn, onehot):
    """mean over HW + Linear on the hard channels per frame: the 8 x 8, 31 x 31 and 32 x 32 maps of the heads, one pixel, the branch above 1024
    channels, the scalar pooling path (ld odd); one-hot weights expose the pooled means themselves"""
    L, st = N.lib(), N.stream()
    x, w, bias = R.pool_inputs(B, HW, C, Nn, onehot)
    r64, r32 = R.pool_ref(x, w, bias)
    a = _alloc()
    xg, wd, bd = a.inp(R.padded(x, ld)), a.inp(w), a.inp(bias)
    out = a.out(B, Nn)
    N.check(L.vs_pool_linear(N.ptr(xg), B, HW, C, ld, N.ptr(wd), N.ptr(bd), Nn, N.ptr(out), st), "vs_pool_linear")
    _done(a)
    mag = R.pool_mag(x, w, bias)
    R.envelope_units(f"pool_linear B={B} HW={HW} C={C} ld={ld} N={Nn}{' one-hot' if onehot else ''}", R.units(out, r64, mag), R.units(r32, r64, mag))


# ------------------------------------------------------------------------------------------------------------------------ message kernels
@pytest.mark.parametrize("kind", R.MSG_TABLES)
@pytest.mark.parametrize("Bm,nbits,hidden", R.MSG_CASES)
def test_msg_latent_fp64_envelope(Bm, nbits, hidden, kind):
    """the sum of the selected table rows, a randn table and one of mean 3 / std 0.5 (every term of one sign), messages of all zeros / all ones"""
    L, st = N.lib(), N.stream()
    table, msgs = R.msg_table(kind, nbits, hidden), R.msg_bits(Bm, nbits)
    r64, r32 = R.msg_latent_ref(table, msgs)
    a = _alloc()
    td, md = a.inp(table), a.inp(msgs)
    lat = a.out(Bm, hidden)
    N.check(L.vs_msg_latent(N.ptr(td), N.ptr(md), Bm, nbits, hidden, N.ptr(lat), st), "vs_msg_latent")
    _done(a)
    mag = R.msg_latent_mag(table, msgs)
    R.envelope_units(f"msg_latent {kind} Bm={Bm} nbits={nbits} hidden={hidden}", R.units(lat, r64, mag), R.units(r32, r64, mag))


@pytest.mark.parametrize("Bm,nbits,hidden", R.MSG_GRAD_CASES)
def test_msg_table_grad_fp64_envelope(Bm, nbits, hidden):
    """the adjoint: per table row the sum over the messages that select it; a row no message selects is exactly zero"""
    L, st = N.lib(), N.stream()
    msgs = R.msg_bits(Bm, nbits, columns_last=True)
    dlat = 3.0 + 0.5 * torch.randn(Bm, hidden, generator=torch.Generator().manual_seed(Bm + hidden))
    r64, r32 = R.msg_table_grad_ref(dlat, msgs)
    mag = R.msg_table_grad(dlat.double().abs(), msgs)
    a = _alloc()
    dd, md = a.inp(dlat), a.inp(msgs)
    dt = a.out(2 * nbits, hidden)
    N.check(L.vs_msg_table_grad(N.ptr(dd), N.ptr(md), Bm, nbits, hidden, N.ptr(dt), st), "vs_msg_table_grad")
    _done(a)
    unsel = (mag == 0).all(1)
    assert unsel.any()
    assert (dt.cpu()[unsel] == 0).all()
    R.envelope_units(f"msg_table_grad Bm={Bm} nbits={nbits} hidden={hidden}", R.units(dt, r64, mag), R.units(r32, r64, mag))


@pytest.mark.parametrize("extra", [0, 7])
@pytest.mark.parametrize("Bm,Nn", R.MSG_PRE_CASES)
def test_msg_pre_fp64_envelope(Bm, Nn, extra):
    """vs_msg_pre_rows with P_ld = 9 N and 9 N + 7 (the extra floats NaN): each of the nine border classes against the float64 sum of its valid
    taps; vs_msg_pre gives the bits of vs_msg_pre_rows(P_ld = 9 N)"""
    L, st = N.lib(), N.stream()
    P = 3.0 + 0.5 * torch.randn(Bm, 9 * Nn, generator=torch.Generator().manual_seed(Bm + Nn))
    r64, r32 = R.msg_pre_ref(P, Nn)
    mag = R.msg_pre(P.double().abs(), Nn)
    a = _alloc()
    Pw = torch.full((Bm, 9 * Nn + extra), NAN)
    Pw[:, :9 * Nn] = P
    pd = a.inp(Pw.flatten()[:(Bm - 1) * (9 * Nn + extra) + 9 * Nn])          # the last row ends with its last tap
    tab = a.out(Bm, 9, Nn)
    N.check(L.vs_msg_pre_rows(N.ptr(pd), 9 * Nn + extra, Bm, Nn, N.ptr(tab), st), "vs_msg_pre_rows")
    if not extra:
        tab2 = a.out(Bm, 9, Nn)
        N.check(L.vs_msg_pre(N.ptr(pd), Bm, Nn, N.ptr(tab2), st), "vs_msg_pre")
    _done(a)
    if not extra:
        assert torch.equal(tab, tab2)
    R.envelope_units(f"msg_pre_rows Bm={Bm} N={Nn} P_ld=9N+{extra}", R.units(tab, r64, mag), R.units(r32, r64, mag))


# ------------------------------------------------------------------------------------------------------------------------ reflection adjoints
@pytest.mark.parametrize("C,ld", R.REFLECT_CL)
@pytest.mark.parametrize("H,W", R.REFLECT_MAPS)
def test_reflection_adjoints_fp64_envelope(H, W, C, ld):
    """vs_reflect_fold1 and vs_col2im3x3_reflect against float64 autograd of ReflectionPad2d(1) (+ unfold): on a 2 x 2 map every ring pixel folds
    onto an interior one that is also first and last"""
    L, st = N.lib(), N.stream()
    B = 2
    g = torch.Generator().manual_seed(H * W + C)
    dxp = 3.0 + 0.5 * torch.randn(B, C, H + 2, W + 2, generator=g)
    dcols = 3.0 + 0.5 * torch.randn(B, H * W, 9, C, generator=g)
    f64, f32_ = R.both(lambda dt: R.reflect_fold(dxp.to(dt)))
    c64, c32 = R.both(lambda dt: R.col2im_reflect(dcols.to(dt), C, H, W))
    a = _alloc()
    dg, cg = a.inp(R.nhwc(dxp, ld)), a.inp(R.padded(dcols, ld).reshape(B * H * W, 9 * ld))
    fold, dx = a.out(B * H * W, ld), a.out(B * H * W, ld)
    N.check(L.vs_reflect_fold1(N.ptr(dg), B, H, W, ld, N.ptr(fold), st), "vs_reflect_fold1")
    N.check(L.vs_col2im3x3_reflect(N.ptr(cg), B, H, W, ld, N.ptr(dx), st), "vs_col2im3x3_reflect")
    _done(a)
    assert (fold[:, C:] == 0).all() and (dx[:, C:] == 0).all()
    # every term is positive here: the sum of the magnitudes is the reference itself
    R.envelope_units(f"reflect_fold1 {H}x{W} C={C} ld={ld}", R.units(R.nchw(fold[:, :C].cpu(), B, H, W), f64, f64.abs()), R.units(f32_, f64, f64.abs()))
    R.envelope_units(f"col2im3x3_reflect {H}x{W} C={C} ld={ld}", R.units(R.nchw(dx[:, :C].cpu(), B, H, W), c64, c64.abs()), R.units(c32, c64, c64.abs()))


# ------------------------------------------------------------------------------------------------------------------------ bit-for-bit kernels
@pytest.mark.parametrize("Bm", [1, 3])
@pytest.mark.parametrize("hidden,coff,ld", [(8, 4, 16), (6, 4, 12), (8, 3, 12), (8, 4, 13), (1, 0, 1), (130, 2, 132)])
def test_broadcast_channels_bit_exact(hidden, coff, ld, Bm):
    """the float4 kernel (hidden, coff and ld multiples of 4) and the one-float kernel (any of them not); columns outside [coff, coff + hidden) keep
    their prior contents"""
    L, st = N.lib(), N.stream()
    B, HW = 3, 37
    lat = torch.randn(Bm, hidden, generator=torch.Generator().manual_seed(hidden))
    a = _alloc()
    ld_, dst = a.inp(lat), a.out(B * HW, ld)
    N.check(L.vs_broadcast_channels(N.ptr(ld_), Bm, hidden, N.ptr(dst), B, HW, ld, coff, st), "vs_broadcast_channels")
    _done(a)
    want = torch.full((B, HW, ld), 3.0)
    want[:, :, coff:coff + hidden] = (lat.expand(B, hidden) if Bm == 1 else lat)[:, None, :]
    assert torch.equal(dst.cpu().view(B, HW, ld), want)


@pytest.mark.parametrize("with_x", [True, False])
@pytest.mark.parametrize("rows,C1,C2,ld1,ld2,old", [(1, 4, 4, 4, 4, 8), (37, 8, 4, 12, 8, 16), (301, 24, 132, 24, 136, 160)])
def test_cat2_scale_bit_exact(rows, C1, C2, ld1, ld2, old, with_x):
    """out = [x | skip * s]; with x = NULL the first C1 columns keep their prior contents; columns behind C1 + C2 are not written"""
    L, st = N.lib(), N.stream()
    g = torch.Generator().manual_seed(rows)
    x, sk = torch.randn(rows, C1, generator=g), torch.randn(rows, C2, generator=g)
    s = 2 ** -0.5
    a = _alloc()
    xnan, snan = torch.full((rows, ld1), NAN), torch.full((rows, ld2), NAN)          # NaN in everything that must not be read
    xnan[:, :C1], snan[:, :C2] = x, sk
    xg, sg = a.inp(xnan) if with_x else None, a.inp(snan)
    out = a.out(rows, old)
    N.check(L.vs_cat2_scale(N.ptr(xg), C1, ld1, N.ptr(sg), C2, ld2, s, rows, N.ptr(out), old, st), "vs_cat2_scale")
    _done(a)
    want = torch.full((rows, old), 3.0)
    if with_x:
        want[:, :C1] = x
    want[:, C1:C1 + C2] = sk * torch.tensor(s, dtype=torch.float32)
    assert torch.equal(out.cpu(), want)


def _cols(t, ld):
    """[rows, 9, C] -> [rows, 9 ld] with zero pad lanes"""
    return R.padded(t, ld).reshape(t.shape[0], 9 * ld)


@pytest.mark.parametrize("C,ld", [(3, 4), (6, 12), (130, 132)])
@pytest.mark.parametrize("H,W", [(2, 2), (2, 7), (8, 8)])
def test_im2col3x3_bit_exact(H, W, C, ld):
    """both pad modes against F.pad + unfold"""
    L, st = N.lib(), N.stream()
    B = 2
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * W))
    a = _alloc()
    xg = a.inp(R.nhwc(x, ld))
    outs = {}
    for mode, name in ((N.PAD_ZERO, "zeros"), (N.PAD_REFLECT, "reflect")):
        outs[name] = a.out(B * H * W, 9 * ld)
        N.check(L.vs_im2col3x3(N.ptr(xg), B, H, W, ld, mode, N.ptr(outs[name]), st), "vs_im2col3x3")
    _done(a)
    for name, got in outs.items():
        assert torch.equal(got.cpu(), _cols(R.im2col3x3(x, name), ld)), name


@pytest.mark.parametrize("C,ld", [(3, 4), (6, 12), (130, 132)])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 8), (8, 5), (7, 7)])
def test_stride2_pieces_and_pad_embed_bit_exact(H, W, C, ld):
    """vs_im2col3x3_strided (stride 1 and 2, zero padding) against unfold; vs_dilate2 for the Ho / Wo the stride-2 conv gives; vs_pad_embed1 against
    F.pad; pad lanes of every output zero"""
    L, st = N.lib(), N.stream()
    B = 2
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(H * W + C)
    x, dy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, Ho, Wo, generator=g)
    a = _alloc()
    xg, dg = a.inp(R.nhwc(x, ld)), a.inp(R.nhwc(dy, ld))
    c1, c2, dil, canvas = a.out(B * H * W, 9 * ld), a.out(B * Ho * Wo, 9 * ld), a.out(B * H * W, ld), a.out(B * (H + 2) * (W + 2), ld)
    N.check(L.vs_im2col3x3_strided(N.ptr(xg), B, H, W, ld, 1, N.ptr(c1), st), "vs_im2col3x3_strided")
    N.check(L.vs_im2col3x3_strided(N.ptr(xg), B, H, W, ld, 2, N.ptr(c2), st), "vs_im2col3x3_strided")
    N.check(L.vs_dilate2(N.ptr(dg), B, Ho, Wo, ld, H, W, N.ptr(dil), st), "vs_dilate2")
    N.check(L.vs_pad_embed1(N.ptr(xg), B, H, W, ld, N.ptr(canvas), st), "vs_pad_embed1")
    _done(a)
    assert torch.equal(c1.cpu(), _cols(R.im2col3x3(x, "zeros", 1), ld))
    assert torch.equal(c2.cpu(), _cols(R.im2col3x3(x, "zeros", 2), ld))
    assert torch.equal(dil.cpu(), R.nhwc(R.dilate2(dy, H, W), ld))
    assert torch.equal(canvas.cpu(), R.nhwc(torch.nn.functional.pad(x, (1, 1, 1, 1)), ld))


@pytest.mark.parametrize("rows,C,ld,dy_ld,dz_ld", [(7, 1, 4, 8, 4), (37, 3, 4, 4, 8), (301, 130, 132, 136, 140)])
def test_relu_bwd_bit_exact(rows, C, ld, dy_ld, dz_ld):
    """only z > 0 passes: +0, -0, negative denormals and -2^-30 do not, positive denormals do; pad lanes of z and dy hold NaN (they must not decide
    anything), those of the output are zeros"""
    L, st = N.lib(), N.stream()
    z = R.relu_z(rows, C)
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(rows))
    zn, dn = torch.full((rows, ld), NAN), torch.full((rows, dy_ld), NAN)
    zn[:, :C], dn[:, :C] = z, dy
    a = _alloc()
    zg, dg = a.inp(zn), a.inp(dn)
    dz = a.out(rows, dz_ld)
    N.check(L.vs_relu_bwd(N.ptr(zg), ld, N.ptr(dg), dy_ld, rows, C, N.ptr(dz), dz_ld, st), "vs_relu_bwd")
    _done(a)
    want = torch.zeros(rows, dz_ld)
    want[:, :C] = torch.where(z > 0, dy, torch.zeros_like(dy))
    assert torch.equal(dz.cpu().view(torch.int32), want.view(torch.int32))          # the bits: a blocked element is +0, never -0


def test_upconv_fused_preferred_is_supported_and_sixteen():
    """host query: preferred = supported and Co == 16"""
    L = N.lib()
    for C1, C2, Co in [(16, 16, 16), (48, 16, 32), (32, 32, 16), (16, 16, 64), (24, 8, 16), (256, 16, 16)]:
        assert L.vs_upconv_fused_preferred(C1, C2, Co) == int(L.vs_upconv_fused_supported(C1, C2, Co) == 1 and Co == 16)
