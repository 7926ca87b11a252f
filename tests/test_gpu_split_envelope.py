"""Every matrix-core kernel family against the emulated split arithmetic (tests/_split_ref.py), on hard operands, per output element.

S is the float64 value of the sum the kernel is specified to form -- arithmetic 2: acc_mul (h_a h_w + h_a l_w + l_a h_w) over the emulated f16
planes, arithmetic 3 and fp32: the exact product -- followed by bias, activation and residual in float64; P the sum of the magnitudes of its terms.
A correct kernel differs from S by its fp32 summation order and the final rounding only, so  r = |got - S| / (2^-24 P)  is a small number for
EVERY element, however small next to the rest of the tensor; no element is left out.  The yardstick r_ref is ATen's float32 product of the same
split operands on the CPU (one thread); the assertion is  max r <= SPLIT_MARGIN max(max r_ref, 1)  per case, SPLIT_MARGIN = twice the largest
ratio measured on an MI355X and never more than 8 (profiles/split_fp64_envelope.txt lists every case).  tests/test_split_contract_cpu.py shows
without a GPU that a low plane flushed to zero or a product dropped on the last K chunk exceeds that cap on each of these shapes.

The fused kernels with on-chip intermediates (convnext_fused, resblock_thin) are held to the same metric, carried through the on-chip stage, in
tests/test_gpu_fused_envelope.py.  Not here and not there: upconv_fused -- its z is never observable behind the LayerNorm; it keeps the
arithmetic-3 envelope of tests/test_gpu_fwd_envelope.py and the bit-identity tests of tests/test_gpu_upconv_block.py -- attention
(tests/test_gpu_fwd_envelope.py), and range-guard / overflow behaviour of whole networks (tests/test_gpu_e2e.py, test_guards_cpu.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _split_ref as R  # noqa: E402
from tests._envelope import check_units  # noqa: E402
from tests._gpu import DEV, Eng, conv_weights, dv, from_nhwc, planes_of, rows_of, to_nhwc, wgrad_gemm_launch, wgrad_gemm_operands  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd.engine import A_MUL, Act, ConvW, rup  # noqa: E402


_check = functools.partial(check_units, "SPLIT-ENVELOPE", 66, R.SPLIT_MARGIN)


def envelope(case, got, S, P, ref32):
    """prints the case's figures, then asserts max r <= SPLIT_MARGIN max(max r_ref, 1) and that every element of got is finite"""
    got = got.detach().cpu()
    _check(case, float(R.units(got, S, P).max()), float(R.units(ref32, S, P).max()))
    assert torch.isfinite(got).all(), case


def assert_kernel_reads_the_emulated_weights(cw: ConvW, w: torch.Tensor, arith: int):
    """the packed planes [P][N][taps * CinP] the kernel reads are the emulator's"""
    if arith != 2:
        return
    n, c, k, _ = w.shape
    hw, lw, w_mul = R.split_f16_weights(w)
    assert cw.w_mul == w_mul
    pl = cw.split.cpu().view(2, n, k * k, cw.CinP)
    for i, want in enumerate((hw, lw)):
        assert torch.equal(pl[i][..., :c], want.view(torch.int16).permute(0, 2, 3, 1).reshape(n, k * k, c))
        assert (pl[i][..., c:] == 0).all()


def arith_name(ar):
    return {2: "2xf16", 3: "3xbf16", 0: "fp32"}[ar]


def make_eng(arith):
    return Eng(use_split=(arith != 0), arith=(arith or 3))


# ---------------------------------------------------------------------------------------------------------------- vs_conv_gemm through Eng.conv
@pytest.mark.parametrize("case,arith", R.CONV_ENV_PARAMS, ids=[f"tile{c[-1]:#x}-{i}-{arith_name(a)}" for i, (c, a) in enumerate(R.CONV_ENV_PARAMS)])
def test_conv_gemm_envelope(case, arith):
    B, Cin, H, W, Cout, k, s, p, pm, act, tile = case
    eng = make_eng(arith)
    x, w, b = R.conv_operands(case)
    r = R.ideal(x, w, arith, A_MUL, stride=s, pad=p, reflect=bool(pm))
    S, P = R.epilogue(r.S, r.P, b, act)
    ref = R.one_thread(lambda: R.epilogue(r.ref32, None, b, act))
    xa = to_nhwc(x)
    cw = conv_weights(w, b, xa.ld)
    out = eng.new_act("env.o", B, S.shape[2], S.shape[3], Cout)
    out.t.fill_(float("nan"))
    eng.conv(xa, cw, out, stride=s, pad=p, pad_mode=pm, act=act, tile_hint=tile)
    torch.cuda.synchronize()
    if arith:
        assert_kernel_reads_the_emulated_weights(cw, w, arith)
    full = out.t.view(B, out.H, out.W, out.ld).cpu()
    assert (full[..., Cout:] == 0).all()                     # pad lanes written as zero
    envelope(f"conv_gemm tile {tile:#x} {arith_name(arith)} {case[:9]} act {act}", from_nhwc(out), S, P, ref)


def _two_phase(eng, arith, tile, B, Cm, Cx, H, W, Co, out_ld, coff, use_res, split_k, seed):
    """relu(conv3x3(t) + b1) + conv1x1(x) + b2 (+ res), written at a channel offset of a wider buffer"""
    t, x = R.hard_act(B, Cm, H, W, seed), R.hard_act(B, Cx, H, W, seed + 1)
    w1, w2 = R.hard_weights(Co, Cm, 3, seed + 2), R.hard_weights(Co, Cx, 1, seed + 3)
    b1, b2 = R.hard_bias(Co, seed + 4), R.hard_bias(Co, seed + 5)
    res = R.hard_act(B, Co, H, W, seed + 6) if use_res else None
    r1, r2 = R.ideal(t, w1, arith, A_MUL, pad=1), R.ideal(x, w2, arith, A_MUL)
    S1, P1 = R.epilogue(r1.S, r1.P, b1, 1)
    S, P = R.epilogue(S1 + r2.S, P1 + r2.P, b2, 0, res)
    ref = R.one_thread(lambda: R.epilogue(R.epilogue(r1.ref32, None, b1, 1) + r2.ref32, None, b2, 0, res))
    ta, xa = to_nhwc(t), to_nhwc(x)
    cw1, cw2 = conv_weights(w1, b1, ta.ld), conv_weights(w2, b2, xa.ld)
    ra = to_nhwc(res) if use_res else None
    out = eng.new_act("env.wide", B, H, W, out_ld)
    out.t.fill_(7.0)
    eng.conv(ta, cw1, out, pad=1, act=N.ACT_RELU, in2=xa, w2=cw2, res=ra, out_coff=coff, n_store=Co, tile_hint=tile, split_k=split_k)
    torch.cuda.synchronize()
    if arith:
        assert_kernel_reads_the_emulated_weights(cw1, w1, arith)
        assert_kernel_reads_the_emulated_weights(cw2, w2, arith)
    full = out.t.view(B, H, W, out_ld).cpu()
    assert (full[..., :coff] == 7.0).all() and (full[..., coff + Co:] == 7.0).all()        # neighbours untouched
    return full[..., coff:coff + Co].permute(0, 3, 1, 2), S, P, ref


@pytest.mark.parametrize("arith", [2, 3, 0], ids=arith_name)
def test_conv_two_phase_envelope(arith):
    got, S, P, ref = _two_phase(make_eng(arith), arith, 0, 2, 32, 16, 14, 18, 32, 48, 8, False, None, 5100)
    envelope(f"conv_gemm two-phase tile 0 {arith_name(arith)}", got, S, P, ref)


@pytest.mark.parametrize("arith", [2, 3], ids=arith_name)
def test_conv_residual_at_a_channel_offset_envelope(arith):
    """wave-specialised 3x3 kernel: two K slices + the slice of the 1x1 phase + residual in the shared split-K epilogue, channel offset 4"""
    got, S, P, ref = _two_phase(make_eng(arith), arith, 15, 2, 64, 48, 8, 16, 40, 48, 4, True, 2, 5200)
    envelope(f"conv_gemm res + out_coff tile 0xf K slices 2 {arith_name(arith)}", got, S, P, ref)


# ---------------------------------------------------------------------------------------------------------------- operand planes + conv3x3_pl.hip
PLANES_PARAMS = [(c, t) for c in R.PLANES_ENV_CASES for t in ((6, 7) if c[6] == 1 else (6,))]


@pytest.mark.parametrize("case,tl", PLANES_PARAMS, ids=[f"{i}-tile{16 + t}" for i, (c, t) in enumerate(PLANES_PARAMS)])
def test_conv3x3_planes_envelope(case, tl):
    """vs_to_planes emits exactly the emulated planes (denormal low terms included); the all-DMA 3x3 kernel on them (tile codes 22 / 23, with
    and without K slices) stays inside the envelope, and the planes it emits are the split of its own fp32 output"""
    B, C, H, W, Co, two, sk = case
    eng = Eng(arith=2)
    x, w1, b1, x2, w2, b2 = R.planes_operands(case)
    r1 = R.ideal(x, w1, 2, A_MUL, pad=1)
    S, P = R.epilogue(r1.S, r1.P, b1, 1)
    ref = R.one_thread(lambda: R.epilogue(r1.ref32, None, b1, 1))
    if two:
        r2 = R.ideal(x2, w2, 2, A_MUL)
        S, P = R.epilogue(S + r2.S, P + r2.P, b2, 0)
        ref = R.one_thread(lambda: R.epilogue(ref + r2.ref32, None, b2, 0))
    xa, xa2 = to_nhwc(x), to_nhwc(x2)
    cw1, cw2 = conv_weights(w1, b1, xa.ld), conv_weights(w2, b2, xa2.ld)
    xpl, x2pl = eng.to_planes(xa, "env.xpl"), eng.to_planes(xa2, "env.x2pl")
    torch.cuda.synchronize()
    for pl, src in ((xpl, x), (x2pl, x2)):
        assert torch.equal(pl.cpu(), planes_of(*R.split_f16(rows_of(src), A_MUL)))
    emit = Co % 16 == 0
    opl = eng.buf("env.opl", B * H * W * rup(Co, 16)).view(torch.int16)
    out = eng.new_act("env.plo", B, H, W, Co)
    out.t.fill_(float("nan"))
    kw = dict(in2=xa2, w2=cw2, in2_pl=x2pl) if two else {}
    eng.conv(xa, cw1, out, pad=1, act=N.ACT_RELU, tile_hint=N.CONV_TILE_HI | tl, arith=2, in_pl=xpl, out_pl=(opl if emit else None),
             split_k=(sk if sk > 1 else None), **kw)
    torch.cuda.synchronize()
    assert_kernel_reads_the_emulated_weights(cw1, w1, 2)
    got = from_nhwc(out)
    if emit:
        assert torch.equal(opl[: 2 * B * H * W * Co].cpu(), planes_of(*R.split_f16(rows_of(got), A_MUL)))
    envelope(f"conv3x3_pl tile {16 + tl} {case}", got, S, P, ref)


# ---------------------------------------------------------------------------------------------------------------- gemm_pl.hip
@pytest.mark.parametrize("case", R.GEMM_PL_ENV_CASES, ids=[f"{i}-tile{c[8]}-amul{int(c[10])}" for i, c in enumerate(R.GEMM_PL_ENV_CASES)])
def test_gemm_planes_envelope(case):
    """all-DMA 1x1 GEMM on operand planes: small tiles (24 / 25) and the big one (27), a_mul = 16 and a_mul = 1 on the GELU-like operand (most
    low terms denormal: pwconv2's production setting), with K slices, and once through vs_to_planes_affine"""
    B, H, W, K, Nn, act, affine, use_res, tile, sk, am = case
    eng = Eng(arith=2)
    a, w, b, res, x, scale, shift = R.gemm_pl_operands(case)
    rows, HW = B * H * W, H * W
    r = R.ideal(R.gemm_as_conv(a), w, 2, am)
    res4 = R.gemm_as_conv(res) if use_res else None
    S, P = R.epilogue(r.S, r.P, b, act, res4)
    ref = R.one_thread(lambda: R.epilogue(r.ref32, None, b, act, res4))
    xa = Act(dv(x), B, H, W, K, K)
    cw = conv_weights(w, b, K)
    pl = torch.empty(2 * rows * K, dtype=torch.int16, device=DEV)
    N.check(eng.lib.vs_to_planes_affine(N.ptr(xa.t), rows, K, K, am, N.ptr(dv(scale)) if affine else None, K,
                                        N.ptr(dv(shift)) if affine else None, HW, N.ptr(pl), N.stream()), "vs_to_planes_affine")
    torch.cuda.synchronize()
    want = planes_of(*R.split_f16(a, am))
    if affine:
        # x * scale + shift in fp32: one fused multiply-add (the emulated operand) or a rounded product and a sum -- every element of the planes is
        # the split of one of the two
        s_rows = scale[torch.arange(rows) // HW]
        alt = planes_of(*R.split_f16(x * s_rows + shift, am))
        got_pl = pl.cpu()
        assert ((got_pl == want) | (got_pl == alt)).all()
        print(f"vs_to_planes_affine: {float((got_pl == want).float().mean()):.4f} of the plane values are the split of fma(x, scale, shift)")
    else:
        assert torch.equal(pl.cpu(), want)
    ld = rup(Nn, 4)
    ra = None
    if use_res:
        ra = Act(torch.zeros(rows * ld, device=DEV), B, H, W, Nn, ld)
        ra.t.view(rows, ld)[:, :Nn] = res.to(DEV)
    out = Act(torch.full((rows * ld,), float("nan"), device=DEV), B, H, W, Nn, ld)
    eng.conv(xa, cw, out, act=act, res=ra, tile_hint=N.CONV_TILE_HI | (tile - 16), arith=2, in_pl=pl, split_k=sk, a_mul=am)
    torch.cuda.synchronize()
    assert_kernel_reads_the_emulated_weights(cw, w, 2)
    full = out.t.view(rows, ld).cpu()
    assert (full[:, Nn:] == 0).all()
    envelope(f"gemm_pl {case}", R.gemm_as_conv(full[:, :Nn]), S, P, ref)


# ---------------------------------------------------------------------------------------------------------------- gemm1x1_pc.hip
@pytest.mark.parametrize("case,arith", R.GEMM_PC_ENV_PARAMS, ids=[f"{i}-tile{16 + c[7]}-{arith_name(a)}" for i, (c, a) in enumerate(R.GEMM_PC_ENV_PARAMS)])
def test_gemm1x1_pc_envelope(case, arith):
    """wave-specialised 1x1 GEMM (tile codes 17 / 18 / 26), including its K-slice epilogue"""
    B, H, W, K, Nn, act, use_res, tl, sk = case
    eng = make_eng(arith)
    a, w, b, res = R.gemm_pc_operands(case)
    rows = B * H * W
    r = R.ideal(R.gemm_as_conv(a), w, arith, A_MUL)
    res4 = R.gemm_as_conv(res) if use_res else None
    S, P = R.epilogue(r.S, r.P, b, act, res4)
    ref = R.one_thread(lambda: R.epilogue(r.ref32, None, b, act, res4))
    xa = Act(dv(a), B, H, W, K, K)
    cw = conv_weights(w, b, K)
    ld = rup(Nn, 4)
    ra = None
    if use_res:
        ra = Act(torch.zeros(rows * ld, device=DEV), B, H, W, Nn, ld)
        ra.t.view(rows, ld)[:, :Nn] = res.to(DEV)
    out = Act(torch.full((rows * ld,), float("nan"), device=DEV), B, H, W, Nn, ld)
    eng.conv(xa, cw, out, act=act, res=ra, tile_hint=N.CONV_TILE_HI | tl, split_k=sk)
    torch.cuda.synchronize()
    assert_kernel_reads_the_emulated_weights(cw, w, arith)
    full = out.t.view(rows, ld).cpu()
    assert (full[:, Nn:] == 0).all()
    envelope(f"gemm1x1_pc {arith_name(arith)} {case}", R.gemm_as_conv(full[:, :Nn]), S, P, ref)


# ---------------------------------------------------------------------------------------------------------------- weight gradients
def wgrad_gemm_check(case, variant, dw, dw2):
    dy, x = wgrad_gemm_operands(case)
    S, P = dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs()         # the exact product: no operand is quantised
    ref = R.one_thread(lambda: dy.t() @ x)
    assert torch.equal(dw, dw2)          # deterministic
    envelope(f"gemm_wgrad {variant} rows={case[0]} N={case[1]} K={case[2]}", dw, S, P, ref)


@pytest.mark.parametrize("case", R.WGRAD_GEMM_CASES, ids=[f"rows{c[0]}-N{c[1]}-K{c[2]}" for c in R.WGRAD_GEMM_CASES])
def test_gemm_wgrad_envelope(case):
    """vs_gemm_wgrad as shipped: the 3 x bf16 matrix-core kernel where N, K >= 64, the fp32 FMA kernel on the thin shapes"""
    variant = "bf16x3-mfma" if case[1] >= 64 and case[2] >= 64 else "fp32-fma"
    wgrad_gemm_check(case, variant, *wgrad_gemm_launch(case))


@pytest.mark.parametrize("mode", ["mfma", "fma"])
@pytest.mark.parametrize("case", R.WGRAD_GEMM_CASES, ids=[f"rows{c[0]}-N{c[1]}-K{c[2]}" for c in R.WGRAD_GEMM_CASES])
def test_gemm_wgrad_forced_kernels_envelope(case, mode):
    """the fp32 MFMA kernel (mfma) and the fp32 FMA kernel on the wide shapes (fma): what VS_WGRAD selects, here through its development switch"""
    with N.debug("WGRAD", {"mfma": 1, "fma": 2}[mode]):
        dw, dw2 = wgrad_gemm_launch(case)
    wgrad_gemm_check(case, f"VS_WGRAD={mode}", dw, dw2)


@pytest.mark.parametrize("case", R.WGRAD_CONV_CASES, ids=[f"{i}-ci{c[3]}-co{c[4]}-s{c[5]}-{'reflect' if c[6] else 'zero'}" for i, c in enumerate(R.WGRAD_CONV_CASES)])
def test_conv3x3_wgrad_envelope(case):
    """vs_conv3x3_wgrad: matrix-core kernel on the implicit patch matrix (co, ld >= 64) and the register-tile kernel of the thin levels"""
    B, H, W, ci, co, stride, reflect = case
    L, st = N.lib(), N.stream()
    ld, ldn = rup(ci, 4), rup(co, 4)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = R.hard_act(B, ci, H, W, 7000 + ci + co)
    dy = R.hard_dy(B * Ho * Wo, co, 7001 + ci + co)                                   # [rows][co], rows = (b, y, x)
    cols = R._cols(x.double(), 3, stride, 1, bool(reflect))                           # [B, L, ci * 9]
    dyb = dy.double().view(B, Ho * Wo, co)
    S = torch.einsum("bln,blk->nk", dyb, cols).reshape(co, ci, 3, 3)
    P = torch.einsum("bln,blk->nk", dyb.abs(), cols.abs()).reshape(co, ci, 3, 3)
    ref = R.one_thread(lambda: torch.einsum("bln,blk->nk", dyb.float(), cols.float()).reshape(co, ci, 3, 3))
    xa, dya = torch.zeros(B * H * W, ld, device=DEV), torch.zeros(B * Ho * Wo, ldn, device=DEV)
    xa[:, :ci], dya[:, :co] = rows_of(x).to(DEV), dy.to(DEV)
    assert L.vs_conv3x3_wgrad_supported(co, ld, stride)
    part = torch.empty(int(L.vs_conv3x3_wgrad_partial_floats(co, ld, B, H, W, stride)), device=DEV)
    pm = N.PAD_REFLECT if reflect else N.PAD_ZERO
    outs = []
    for _ in range(2):
        dw = torch.full((co, 9 * ld), 7.0, device=DEV)
        N.check(L.vs_conv3x3_wgrad(N.ptr(dya), ldn, co, N.ptr(xa), ld, B, H, W, stride, pm, N.ptr(part), N.ptr(dw), st), "vs_conv3x3_wgrad")
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])          # deterministic
    assert (outs[0].view(co, 9, ld)[..., ci:] == 0).all()
    got = outs[0].view(co, 3, 3, ld)[..., :ci].permute(0, 3, 1, 2)
    envelope(f"conv3x3_wgrad {'mfma' if co >= 64 and ld >= 64 else 'register-tile'} {case}", got, S, P, ref)
