"""The two fused kernels whose intermediate tensor never leaves the chip, per output element against the emulated split arithmetic carried through
the on-chip stage (tests/_fused_ref.py: metric, operands, cases): vs_cnx_block (csrc/convnext_fused.hip) by direct C-ABI calls, vs_resblock_thin
(csrc/resblock_thin.hip) through its descriptor.  The hidden tensor is made observable by a one-hot second product (W2 selecting hidden channels, w1
= identity on one tap), so pwconv1, GELU, the per-frame GRN scale, beta, the k(s, half, v) permutation of the packed W2, the second split, t with its
recomputed halo and t's zero padding are checked element by element.  Every operand sits between NaN bands, every output between sentinel bands
(tests/_guards.py); launches are repeated and the serial and the pipelined ConvNeXt kernels compared bit for bit; an operand pushed beyond the f16
range must come out non-finite.  tests/test_fused_contract_cpu.py shows without a GPU that the metric rejects the seeded defects.

vs_cnx_block's apply launch gives a workgroup 128 consecutive pixels and ONE scale row: frames that are no multiple of 128 pixels are refused
(vs_cnx_block_supported), and the refusal is what is tested for them.  Every FUSED-ENVELOPE line of an MI355X run is in
profiles/fused_fp64_envelope.txt."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _fused_ref as Q  # noqa: E402
from tests import _split_ref as R  # noqa: E402
from tests._envelope import check_units  # noqa: E402
from tests._gpu import DEV, planes_of  # noqa: E402
from tests._guards import _guarded, _guards_intact  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd.engine import pack_cnx_block, pack_conv, rup, split_bf16x3, split_f16x2  # noqa: E402

NAN = float("nan")
SENT = -7.0
NAN16 = 0x7FC0          # a NaN as f16 and as bf16
NANB = 0xFF             # bytes of a NaN in either 16-bit format and in fp32
PAD = 8                 # extra lanes of res_ld / out_ld


_check = functools.partial(check_units, "FUSED-ENVELOPE", 84, Q.FUSED_MARGIN)


def envelope(case, got, S, unit, ref, skip=None):
    """prints the case's figures, then asserts max r <= FUSED_MARGIN max(max r_ref, 1) over every element (skip: the pixels of a planted overflow)"""
    r_all, r_ref_all = Q.ratio_units(got, S, unit), Q.ratio_units(ref, S, unit)
    if skip is not None:
        r_all, r_ref_all = r_all.masked_fill(skip, 0.0), r_ref_all.masked_fill(skip, 0.0)
    r, r_ref = float(r_all.max()), float(r_ref_all.max())
    if torch.isnan(r_all).any():
        r = NAN
    _check(case, r, r_ref)


# ---------------------------------------------------------------------------------------------------------------- vs_cnx_block
@functools.lru_cache(maxsize=None)
def first_of(shape, block=False):
    o = Q.cnx_block_operands(*shape) if block else Q.cnx_operands(*shape)
    return o, Q.cnx_first(o)


class Cnx:
    """one set of guarded device operands of vs_cnx_block; stats() and apply() launch on them and check every band"""

    def __init__(self, o, w2, bias2=None, res=None, alias=False):
        self.o, self.L, self.alias = o, N.lib(), alias
        H4, ld = 4 * o.C, o.C + PAD
        self.ld, self.sld = ld, H4 + Q.SCALE_PAD
        img, self.m1, self.m2 = pack_cnx_block(o.w1[:, :, 0, 0], o.b1, w2[:, :, 0, 0], o.beta, "cpu")
        assert img.numel() == self.L.vs_cnx_block_image_bytes(o.C)
        self.tn_buf, self.tn = _guarded(planes_of(*R.split_f16(o.tn, Q.A_MUL)).to(DEV), NAN16)
        self.img_buf, self.img = _guarded(img.to(DEV), NANB)
        self.s_buf, self.scale = _guarded(torch.full((o.B, self.sld), NAN, device=DEV), NAN)
        self.b2_buf, self.b2 = _guarded((torch.zeros(o.C) if bias2 is None else bias2).to(DEV), NAN)
        rs = torch.full((o.rows, ld), SENT if alias else NAN)
        rs[:, :o.C] = torch.zeros(o.rows, o.C) if res is None else res
        self.res_host = rs
        self.r_buf, self.res = _guarded(rs.to(DEV), SENT if alias else NAN)
        self.g_buf, self.gamma = _guarded(o.gamma.to(DEV), NAN)
        self.am1, self.am2 = 1.0 / (Q.A_MUL * self.m1), 1.0 / (Q.A_MUL_GRN * self.m2)

    def inputs_intact(self):
        return (_guards_intact(self.tn_buf, NAN16) and _guards_intact(self.img_buf, NANB) and _guards_intact(self.s_buf, NAN)
                and _guards_intact(self.b2_buf, NAN) and _guards_intact(self.r_buf, SENT if self.alias else NAN) and _guards_intact(self.g_buf, NAN))

    def stats(self, serial=False, expect_ok=True):
        o = self.o
        self.p_buf, self.part = _guarded(torch.full((o.rows // 32, 4 * o.C), NAN, device=DEV), SENT)
        rc = self.L.vs_cnx_block(N.ptr(self.tn), N.ptr(self.img), o.C, o.rows, o.HW, 1 | (2 if serial else 0), self.am1, self.am2, None, 0, None, None, 0,
                                 None, 0, N.ptr(self.part), N.stream())
        torch.cuda.synchronize()
        assert self.inputs_intact() and _guards_intact(self.p_buf, SENT)
        if expect_ok:
            N.check(rc, "vs_cnx_block(stats)")
        return rc, self.part.cpu()

    def set_scale(self, scale):
        self.scale.fill_(NAN)
        self.scale[:, :scale.shape[1]] = scale.to(DEV)

    def finish_scale(self):
        """vs_grn_scale_from_partials on the partial sums of the last stats(), as engine.py sequences the block"""
        o = self.o
        N.check(self.L.vs_grn_scale_from_partials(N.ptr(self.part), o.B, o.HW, 4 * o.C, N.ptr(self.gamma), N.ptr(self.scale), self.sld, N.stream()),
                "vs_grn_scale_from_partials")
        torch.cuda.synchronize()
        return self.scale[:, :4 * o.C].cpu()

    def apply(self, serial=False, expect_ok=True):
        """-> (rc, out [rows, C]); lanes [C, out_ld) and the bands around out must keep their sentinel"""
        o = self.o
        if self.alias:
            self.res.copy_(self.res_host.to(DEV))
            o_buf, out = self.r_buf, self.res
        else:
            o_buf, out = _guarded(torch.full((o.rows, self.ld), SENT, device=DEV), SENT)
        rc = self.L.vs_cnx_block(N.ptr(self.tn), N.ptr(self.img), o.C, o.rows, o.HW, 2 if serial else 0, self.am1, self.am2, N.ptr(self.scale), self.sld,
                                 N.ptr(self.b2), N.ptr(self.res), self.ld, N.ptr(out), self.ld, None, N.stream())
        torch.cuda.synchronize()
        full = out.cpu()
        assert self.inputs_intact() and _guards_intact(o_buf, SENT)
        assert (full[:, o.C:] == SENT).all()
        if expect_ok:
            N.check(rc, "vs_cnx_block(apply)")
        return rc, full[:, :o.C].clone()


def shape_id(s):
    return f"C{s[0]}-HW{s[1]}-B{s[2]}"


@pytest.mark.parametrize("shape", Q.CNX_SHAPES, ids=shape_id)
def test_cnx_statistics_launch(shape):
    """part32[group][4C] = sum over each 32-pixel group of gelu(pwconv1)^2, per entry; serial == pipelined == a second launch, bit for bit"""
    o, f = first_of(shape)
    run = Cnx(o, o.w2)
    assert run.m1 == f.w_mul
    _, part = run.stats()
    assert torch.equal(part, run.stats()[1]) and torch.equal(part, run.stats(serial=True)[1])
    envelope(f"cnx_block stats {shape_id(shape)}", part, f.part, f.part_unit, f.part32)


@pytest.mark.parametrize("sel", range(Q.NSEL))
@pytest.mark.parametrize("shape", Q.CNX_SHAPES, ids=shape_id)
def test_cnx_hidden_tensor_through_a_one_hot_w2(shape, sel):
    """W2 row n selects hidden channel sel C + n: out[p][n] = (gelu(x1) * scale[frame(p)] + beta)[sel C + n] after the split, times a power of two"""
    o, f = first_of(shape)
    w2 = Q.one_hot_w2(o.C, sel)
    e = Q.cnx_second(o, f, w2)
    run = Cnx(o, w2)
    assert run.m2 == e.w_mul
    run.set_scale(o.scale)
    _, out = run.apply()
    assert torch.equal(out, run.apply(serial=True)[1])
    envelope(f"cnx_block hidden channels {sel * o.C}..{(sel + 1) * o.C - 1} {shape_id(shape)}", out, e.S, e.unit, e.ref)


@pytest.mark.parametrize("alias", [False, True], ids=["res-apart", "res-is-out"])
@pytest.mark.parametrize("shape", Q.CNX_SHAPES, ids=shape_id)
def test_cnx_apply_launch(shape, alias):
    """hard W2, bias2 and residual (in a buffer of its own and in place, as the engine calls it), res_ld = out_ld > C"""
    o, f = first_of(shape)
    e = Q.cnx_second(o, f, o.w2, bias2=o.bias2, res=o.res)
    run = Cnx(o, o.w2, o.bias2, o.res, alias)
    assert run.m1 == f.w_mul and run.m2 == e.w_mul
    run.set_scale(o.scale)
    _, out = run.apply()
    assert torch.equal(out, run.apply()[1]) and torch.equal(out, run.apply(serial=True)[1])
    envelope(f"cnx_block apply {'in place' if alias else 'res apart'} {shape_id(shape)}", out, e.S, e.unit, e.ref)


@pytest.mark.parametrize("shape", Q.CNX_SHAPES, ids=shape_id)
def test_cnx_whole_block(shape):
    """statistics -> vs_grn_scale_from_partials -> apply in place, against the ConvNeXt-V2 block formula in float64 (one frame of magnitude 1e-3, one
    whose tn is all zeros)"""
    o, f = first_of(shape, block=True)
    s64, u_s = Q.grn_scale64(f.part, o.gamma.double(), o.B, f.part_unit)
    s32 = R.one_thread(lambda: Q.grn_scale64(f.part32, o.gamma, o.B))
    fr = torch.arange(o.rows) // o.HW
    e = Q.cnx_second(o, f, o.w2, rows64=s64[fr], rows32=s32[fr], u_scale=u_s[fr], bias2=o.bias2, res=o.res)
    run = Cnx(o, o.w2, o.bias2, o.res, alias=True)
    run.stats()
    scale = run.finish_scale()
    envelope(f"cnx_block block: GRN scale {shape_id(shape)}", scale, s64, u_s, s32)
    _, out = run.apply()
    envelope(f"cnx_block block: out {shape_id(shape)}", out, e.S, e.unit, e.ref)


@pytest.mark.parametrize("shape", [Q.CNX_SHAPES[0], Q.CNX_SHAPES[2]], ids=shape_id)
def test_cnx_overflow_of_the_second_split_is_loud(shape):
    """one hidden element with |h * scale + beta| >= 65520: every output of that pixel is non-finite, every other pixel stays inside the envelope"""
    o, f = first_of(shape)
    fr, k, p, s = Q.overflow_plant(o, f)
    scale = o.scale.clone()
    scale[fr, k] = s
    e = Q.cnx_second(o, f, o.w2, rows64=Q.scale_rows_of(scale, o.HW, o.rows), bias2=o.bias2, res=o.res, zero=(p, k))
    run = Cnx(o, o.w2, o.bias2, o.res)
    run.set_scale(scale)
    _, out = run.apply()
    assert not torch.isfinite(out[p]).any()
    skip = torch.zeros_like(out, dtype=torch.bool)
    skip[p] = True
    assert torch.isfinite(out[~skip]).all()
    envelope(f"cnx_block overflow planted at pixel {p} channel {k} {shape_id(shape)}", out, e.S, e.unit, e.ref, skip)


@pytest.mark.parametrize("shape", Q.CNX_STRADDLE, ids=shape_id)
def test_cnx_block_refuses_frames_that_straddle_a_workgroup(shape):
    """HW % 128 != 0: the waves of one apply workgroup would lie in different frames and share one scale row.  Not supported: an error, nothing
    written.  (The engine's gate calls the same function and takes the per-layer path.)"""
    o = Q.cnx_operands(*shape)
    L = N.lib()
    assert L.vs_cnx_block_supported(o.C, o.rows, o.HW) == 0
    run = Cnx(o, o.w2, o.bias2, o.res)
    run.set_scale(o.scale)
    rc, part = run.stats(expect_ok=False)
    assert rc != 0 and torch.isnan(part).all()
    for serial in (False, True):
        rc, out = run.apply(serial=serial, expect_ok=False)
        assert rc != 0 and (out == SENT).all()
    for s in Q.CNX_SHAPES:
        assert L.vs_cnx_block_supported(s[0], s[1] * s[2], s[1]) == 1


# ---------------------------------------------------------------------------------------------------------------- vs_resblock_thin
def rb_launch(o, arith, pad=0):
    """vs_resblock_thin through its descriptor with x, the three weight planes, the biases and out between bands -> out [B, C, H, W] (CPU)"""
    L = N.lib()
    ld, ldo = rup(o.Cin, 4), o.C + pad
    assert L.vs_resblock_thin_supported(ld, o.C, o.C)
    xn = torch.zeros(o.B, o.H, o.W, ld)
    xn[..., :o.Cin] = o.x.permute(0, 2, 3, 1)
    bufs = [_guarded(xn.to(DEV), NAN)]
    muls = []
    for w, in_ld in ((o.w0, ld), (o.w1, o.C), (o.wr, ld)):
        wt, cp = pack_conv(w, in_ld)
        assert cp == o.C
        pl, m = split_f16x2(wt) if arith == 2 else (split_bf16x3(wt), 1.0)
        muls.append(m)
        bufs.append(_guarded(pl.to(DEV), NAN16))
    for b in (o.b0, o.b1, o.br):
        bufs.append(_guarded(b.to(DEV), NAN))
    o_buf, out = _guarded(torch.full((o.B * o.H * o.W, ldo), SENT, device=DEV), SENT)
    v = [b[1] for b in bufs]
    d = N.ResblockThinDesc()
    d.x, d.x_ld, d.B, d.H, d.W, d.Cin = N.ptr(v[0]), ld, o.B, o.H, o.W, ld
    d.w0_split, d.w1_split, d.wr_split = N.ptr(v[1]), N.ptr(v[2]), N.ptr(v[3])
    d.b0, d.b1, d.br = N.ptr(v[4]), N.ptr(v[5]), N.ptr(v[6])
    d.arith, d.Cout, d.a_mul = arith, o.C, Q.A_MUL
    d.acc_mul0, d.acc_mul1, d.acc_mulr = [1.0 / (Q.A_MUL * m) for m in muls]
    d.out, d.out_ld = N.ptr(out), ldo
    N.check(L.vs_resblock_thin(C.byref(d), N.stream()), "vs_resblock_thin")
    torch.cuda.synchronize()
    for i, (buf, _) in enumerate(bufs):
        assert _guards_intact(buf, NAN16 if 1 <= i <= 3 else NAN)
    assert _guards_intact(o_buf, SENT)
    full = out.cpu()
    assert (full[:, o.C:] == SENT).all()
    return full[:, :o.C].reshape(o.B, o.H, o.W, o.C).permute(0, 3, 1, 2).contiguous()


def rb_id(p):
    (c, ar, cin), (b, h, w) = p
    return f"{cin}-{c}-{c}-{'2xf16' if ar == 2 else '3xbf16'}-B{b}-{h}x{w}"


RB_SMALL_PARAMS = [(f, m) for f in Q.RB_FORMS for m in Q.RB_SMALL]
RB_LARGE_PARAMS = [(f, m) for f in ((16, 2, 16), (16, 3, 4), (32, 2, 32)) for m in Q.RB_LARGE]
RB_OVERFLOW_PARAMS = [(f, m) for f in ((16, 2, 1), (16, 2, 16), (32, 2, 20)) for m in ((2, 7, 15), (2, 17, 33))]


@pytest.mark.parametrize("p", RB_SMALL_PARAMS, ids=rb_id)
def test_resblock_thin_on_chip_t(p):
    """w1 = identity on one tap, b1 = 0, no res_conv: out = t, border pixels and the recomputed halo included (centre tap); with the corner taps the
    image border reads t's padding, which is conv1's zeros and not conv0 of padded data (b0 makes the latter clearly positive): exactly 0"""
    (c, arith, cin), m = p
    o = Q.with_positive_ring(Q.rb_operands(c, cin, *m))
    for tap in (4, 0, 8):
        q = Q.with_t_observable(o, tap)
        e = Q.rb_chain(q, arith)
        got = rb_launch(q, arith)
        if tap == 0:
            assert (got[:, :, 0, :] == 0).all() and (got[:, :, :, 0] == 0).all()
        if tap == 8:
            assert (got[:, :, -1, :] == 0).all() and (got[:, :, :, -1] == 0).all()
        envelope(f"resblock_thin t through tap {tap} {rb_id(p)}", got, e.S, e.unit, e.ref)


def rb_whole(p, pads):
    (c, arith, cin), m = p
    o = Q.rb_operands(c, cin, *m)
    e = Q.rb_chain(o, arith)
    for pad in pads:
        got = rb_launch(o, arith, pad)
        assert torch.equal(got, rb_launch(o, arith, pad))
        envelope(f"resblock_thin block out_ld {c + pad} {rb_id(p)}", got, e.S, e.unit, e.ref)


@pytest.mark.parametrize("p", RB_SMALL_PARAMS, ids=rb_id)
def test_resblock_thin_whole_block(p):
    """relu(conv1(t) + b1) + res_conv(x) + b_res on hard operands with the full propagated unit, out_ld = C and C + 8, two launches bit-identical"""
    rb_whole(p, (0, PAD))


@pytest.mark.parametrize("p", RB_LARGE_PARAMS, ids=rb_id)
def test_resblock_thin_persistent_walk(p):
    """more tiles than persistent workgroups (two per CU for 16 channels, one for 32): a workgroup walks several tiles across tile rows and frame
    boundaries with the next patch in flight"""
    (c, arith, cin), (b, h, w) = p
    tiles, cus = b * -(-h // 8) * -(-w // 16), torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles > cus * (1 if (b, h, w) == Q.RB_LARGE[0] else 2)
    rb_whole(p, (0,))


@pytest.mark.parametrize("p", RB_OVERFLOW_PARAMS, ids=rb_id)
def test_resblock_thin_overflow_of_t_is_loud(p):
    """one element of t beyond 65520 / 16: every output in its 3 x 3 footprint is non-finite, the rest stays inside the envelope"""
    (c, arith, cin), m = p
    q, (b, n, y, x) = Q.rb_overflow_operands(Q.rb_operands(c, cin, *m))
    e = Q.rb_chain(q, arith, zero=(b, n, y, x))
    got = rb_launch(q, arith)
    skip = torch.zeros_like(got, dtype=torch.bool)
    skip[b, :, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    assert not torch.isfinite(got[skip]).any() and torch.isfinite(got[~skip]).all()
    envelope(f"resblock_thin overflow of t[{n}] at ({y}, {x}) {rb_id(p)}", got, e.S, e.unit, e.ref, skip)
