"""fp64 envelopes of the forward normalisation, GRN and attention kernels on hard inputs (tests/_fwd_ref.py: formulas, inputs, cases, metric;
tests/test_fwd_contract_cpu.py: the metric bites).  Every LayerNorm implementation -- the three forms of vs_layernorm_act, the patch-matrix
store, both branches of ln_rows_from_lds behind the depthwise conv (row and tiled kernel, 4 and 8 lanes per pixel; see R.DW_CASES for what
these maps do not reach), the stem and the up-conv gather, the private copies of upconv_fused.hip and pixel_head.hip --, vs_rmsnorm_act,
the GRN finish kernels and both attention kernels: worst group of
max |got - ref| / max |ref| against the formula in float64, at most FWD_FP64_MARGIN times what the same formula costs in float32 on the CPU.
Every figure is printed as a FWD-ENVELOPE line; profiles/fwd_fp64_envelope.txt is such a run on an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _envelope as E  # noqa: E402
from tests import _fwd_ref as R  # noqa: E402
from tests._gpu import Eng, _padded, attention_launch, dv, from_nhwc, to_nhwc  # noqa: E402
from tests._guards import _guarded, _guards_intact  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import pixel_head as PH  # noqa: E402
from videoseal_amd.engine import ConvW, pack_conv, pack_patch_conv, rup  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _pad1(v, ld):
    return dv(torch.cat([v, torch.zeros(ld - v.numel())]))


def _rows(got, r64, r32, name="y/row"):
    """one envelope line: groups = slices along the last dim (a row / pixel)"""
    return (name, E.group_err(got, r64, -1), E.group_err(r32, r64, -1))


# ------------------------------------------------------------------------------------------------------------------------ vs_layernorm_act
@pytest.mark.parametrize("act", R.LN_ACTS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=[c[0] for c in R.LN_CASES])
def test_layernorm_act_fp64_envelope(case, act):
    """every form of vs_layernorm_act (thread-per-row small<4|8|16>, lanes <8|16|32|64, 4> and <64, 12>, wave-per-row by shape and forced through
    development switch LN_FORM) on rows of mean 30 / std 0.5, a constant row, a row with one 4e3 outlier and a row of magnitude 1e-3; input between NaN
    bands, output between guard bands, pad lanes of the output zero"""
    tag, rows, C, ld, force_wave = case
    L = N.lib()
    x, w, b = R.ln_inputs(rows, C)
    r64, r32 = R.ln_ref(x, w, b, act)
    xbuf, xg = _guarded(_padded(x, ld).to(DEV), NAN)
    obuf, og = _guarded(torch.full((rows, ld), 9.0, device=DEV), -7.0)
    wd, bd = _pad1(w, ld), _pad1(b, ld)
    with N.debug("LN_FORM", force_wave):
        N.check(L.vs_layernorm_act(N.ptr(xg), rows, C, ld, N.ptr(wd), N.ptr(bd), 1e-6, act, N.ptr(og), ld, N.stream()), "vs_layernorm_act")
        torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0) and _guards_intact(xbuf, NAN)
    assert (og[:, C:] == 0).all()
    R.envelope(f"layernorm_act {tag} rows={rows} C={C} ld={ld} act={act}", [_rows(og[:, :C], r64, r32)])


@pytest.mark.parametrize("B,H,W,C", R.PATCH_CASES)
def test_layernorm_patch2x2_fp64_envelope(B, H, W, C):
    """vs_layernorm_patch2x2 on an odd map: the rearranged float64 LayerNorm; the dropped last row / column are absent (the output has no room for
    them: the buffer behind it must be intact)"""
    L = N.lib()
    rows = B * H * W
    x, w, b = R.ln_inputs(rows, C)
    r64, r32 = R.ln_ref(x, w, b)
    Ho, Wo = H // 2, W // 2

    def patches(t):
        return t.view(B, H, W, C)[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * Ho * Wo * 4, C)
    xbuf, xg = _guarded(x.to(DEV), NAN)
    obuf, og = _guarded(torch.full((B * Ho * Wo * 4, C), 9.0, device=DEV), -7.0)
    wd, bd = dv(w), dv(b)
    N.check(L.vs_layernorm_patch2x2(N.ptr(xg), B, H, W, C, C, N.ptr(wd), N.ptr(bd), 1e-6, N.ptr(og), N.stream()), "vs_layernorm_patch2x2")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0) and _guards_intact(xbuf, NAN)
    assert torch.isfinite(og).all() and not (og == 9.0).all(1).any()          # every (pixel, tap) row of the patch matrix was written
    R.envelope(f"layernorm_patch2x2 B={B} {H}x{W} C={C}", [_rows(og, patches(r64), patches(r32))])


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm behind a producer
@pytest.mark.parametrize("C,H,W", R.DW_CASES)
def test_dwconv7_ln_fp64_envelope(C, H, W):
    """vs_dwconv7_ln / vs_dwconv7_ln_planes, row and tiled kernel, register-resident and loop branch of the LayerNorm (see R.DW_CASES).  Reference:
    float64 depthwise conv + LayerNorm; yardstick: fp32 conv + the written-out LayerNorm.  The LayerNorm input is hard: activations of mean 30 /
    std 0.5, taps that sum to about 1 per channel (the conv output keeps the shift), one channel whose taps are exactly zero (its conv output
    is the bias alone) and one constant frame (all interior pixels share one row) -- the per-pixel groups hold shifted, constant-across-pixels
    and near-zero entries.  The planes form: bit-equal to vs_to_planes of the fp32 output"""
    L, st = N.lib(), N.stream()
    x, wd, bd, lw, lb = R.dw_inputs(C, H, W)
    r64, r32 = R.dw_ref(x, wd, bd, lw, lb)
    B = x.shape[0]
    xa = to_nhwc(x)
    ld = xa.ld
    wp = torch.zeros(49, ld)
    wp[:, :C] = wd.reshape(C, 49).t()
    wpd, bdd, lwd, lbd = dv(wp), _pad1(bd, ld), _pad1(lw, ld), _pad1(lb, ld)
    xbuf, xg = _guarded(xa.t, NAN)
    obuf, og = _guarded(torch.full((B * H * W, ld), 9.0, device=DEV), -7.0)
    N.check(L.vs_dwconv7_ln(N.ptr(xg), B, H, W, C, ld, N.ptr(wpd), N.ptr(bdd), N.ptr(lwd), N.ptr(lbd), 1e-6, N.ptr(og), ld, st), "vs_dwconv7_ln")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0) and _guards_intact(xbuf, NAN)
    assert (og[:, C:] == 0).all()
    R.envelope(f"dwconv7_ln C={C} {H}x{W}", [_rows(og[:, :C].view(B, H, W, C), r64, r32)])
    Cp = rup(C, 32)
    pl = torch.full((2 * B * H * W * Cp,), 77, dtype=torch.int16, device=DEV)
    N.check(L.vs_dwconv7_ln_planes(N.ptr(xg), B, H, W, C, ld, N.ptr(wpd), N.ptr(bdd), N.ptr(lwd), N.ptr(lbd), 1e-6, 16.0, Cp, N.ptr(pl), st), "dw planes")
    wide = torch.zeros(B * H * W, Cp, device=DEV)
    wide[:, :C] = og[:, :C]
    want = torch.empty_like(pl)
    N.check(L.vs_to_planes(N.ptr(wide), B * H * W, Cp, Cp, 16.0, N.ptr(want), st), "vs_to_planes")
    torch.cuda.synchronize()
    assert torch.equal(pl, want)


@pytest.mark.parametrize("stride,Co,S", R.STEM_CASES)
def test_stem_conv_ln_fp64_envelope(stride, Co, S):
    """vs_stem_conv_ln: frames of mean 30 / std 0.5 (one constant), 48 taps per channel that sum to about 1 (every pixel's row sits near 30), one
    channel with zero taps; float64 conv + LayerNorm against fp32 conv + the written-out LayerNorm"""
    L = N.lib()
    x, w, b, lw, lb = R.stem_inputs(stride, Co, S)
    r64, r32 = R.stem_ref(x, w, b, lw, lb, stride)
    B = x.shape[0]
    xa = to_nhwc(x, 4)
    wt, cp = pack_patch_conv(w.to(DEV), 4)
    Ho, Wo = r64.shape[1], r64.shape[2]
    obuf, og = _guarded(torch.full((B, Ho, Wo, Co), 9.0, device=DEV), -7.0)
    bd, lwd, lbd = dv(b), dv(lw), dv(lb)
    N.check(L.vs_stem_conv_ln(N.ptr(xa.t), B, S, S + 4, stride, N.ptr(wt), N.ptr(bd), N.ptr(lwd), N.ptr(lbd), 1e-6, Co, N.ptr(og), Co, N.stream()), "stem")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0)
    R.envelope(f"stem_conv_ln stride={stride} Co={Co} S={S}", [_rows(og, r64, r32)])


@pytest.mark.parametrize("shape,zero", R.UPCONV_CASES)
def test_upconv_gather_ln_fp64_envelope(shape, zero):
    """vs_upconv_gather_ln behind the low-resolution GEMM on the exact 3 x bf16 split (that GEMM has its own envelope: only the LayerNorm stage
    is new here), and vs_upconv_fused where supported: maps of mean 30 / std 0.5 (the last frame constant where there are two), weights that
    sum to about 1 per output channel -- every pixel's row sits near 27 with a spread of about one unit --, with and without one output
    channel of zero weights (R._unit_sum_weights); float64 up-sampling + conv + LayerNorm + ReLU against the same in fp32"""
    B, C1, C2, H, W, Co = shape
    eng = Eng(arith=3)
    L, st = eng.lib, N.stream()
    x, sk, w, lw, lb = R.upconv_inputs(*shape, zero)
    r64, r32 = R.upconv_ref(x, sk, w, lw, lb, N.ACT_RELU)
    assert L.vs_upconv_supported(Co) == 1
    xa, sa = to_nhwc(x), to_nhwc(sk)
    lc = eng.new_act("fe.lcat", B, H, W, C1 + C2)
    N.check(L.vs_cat2_scale(N.ptr(xa.t), C1, xa.ld, N.ptr(sa.t), C2, sa.ld, 2 ** -0.5, lc.rows, N.ptr(lc.t), lc.ld, st), "cat2")
    wz, cpz = pack_conv(w.to(DEV).permute(2, 3, 0, 1).reshape(9 * Co, C1 + C2)[:, :, None, None], lc.ld)
    z = eng.new_act("fe.z", B, H, W, 9 * Co)
    eng.conv(lc, ConvW(wz, None, 9 * Co, 1, 1, cpz), z)
    lwd, lbd = dv(lw), dv(lb)
    obuf, og = _guarded(torch.full((B, 2 * H, 2 * W, Co), 9.0, device=DEV), -7.0)
    N.check(L.vs_upconv_gather_ln(N.ptr(z.t), z.ld, B, H, W, Co, N.ptr(lwd), N.ptr(lbd), 1e-6, N.ACT_RELU, N.ptr(og), Co, st), "upconv_gather_ln")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0)
    lines = [_rows(og, r64, r32, "gather/px")]
    if L.vs_upconv_fused_supported(C1, C2, Co):
        obuf2, og2 = _guarded(torch.full((B, 2 * H, 2 * W, Co), 9.0, device=DEV), -7.0)
        cw = ConvW(wz, None, 9 * Co, 1, 1, cpz).with_split(3)
        N.check(L.vs_upconv_fused(N.ptr(xa.t), C1, xa.ld, N.ptr(sa.t), C2, sa.ld, 2 ** -0.5, N.ptr(cw.split), B, H, W, Co, N.ptr(lwd), N.ptr(lbd),
                                  1e-6, N.ACT_RELU, N.ptr(og2), Co, 3, 16.0, 1.0 / (16.0 * cw.w_mul), st), "upconv_fused")
        torch.cuda.synchronize()
        assert _guards_intact(obuf2, -7.0)
        lines.append(_rows(og2, r64, r32, "fused/px"))
    R.envelope(f"upconv {shape}{' zero channel' if zero else ''}", lines)


@pytest.mark.parametrize("zero", [True, False])
def test_pixel_upgather_fp64_envelope(zero):
    """vs_pixel_upgather (the LayerNorm of pixel_head.hip) at the smallest stage of tests/test_gpu_pixel_head.py, hard inputs as above, GELU"""
    C, Co, f, H, W = R.PIXEL_CASE
    eng = Eng(arith=3)
    x, w, lw, lb = R.pixel_inputs(*R.PIXEL_CASE, zero)
    r64, r32 = R.upconv_ref(x, None, w, lw, lb, N.ACT_GELU, f=f)
    assert eng.lib.vs_pixel_upgather_supported(Co, f) == 1
    xa = to_nhwc(x)
    lwd, lbd = dv(lw), dv(lb)
    out = PH.stage_forward(eng, xa, PH.pack_stage(w.to(DEV), xa.ld), lwd, lbd, f, "fe.ps")
    torch.cuda.synchronize()
    R.envelope(f"pixel_upgather C={C} Co={Co} x{f} {H}x{W}{' zero channel' if zero else ''}", [_rows(from_nhwc(out).permute(0, 2, 3, 1), r64, r32)])


# ------------------------------------------------------------------------------------------------------------------------ vs_rmsnorm_act
@pytest.mark.parametrize("rows,C", R.RMS_CASES)
def test_rmsnorm_act_fp64_envelope(rows, C):
    """4 / 16 / 64 lanes per row, SiLU + residual branch; the all-zero row gives `add` exactly (the max(||x||, 1e-12) clamp), a row of 1e-20 stays finite"""
    L = N.lib()
    x, gamma, add = R.rms_inputs(rows, C)
    r64, r32 = R.rms_ref(x, gamma, add)
    xbuf, xg = _guarded(x.to(DEV), NAN)
    obuf, og = _guarded(torch.full((rows, C + 4), 9.0, device=DEV), -7.0)
    gd, ad = dv(gamma), dv(add)
    N.check(L.vs_rmsnorm_act(N.ptr(xg), rows, C, C, N.ptr(gd), N.ACT_SILU, N.ptr(ad), C, N.ptr(og), C + 4, N.stream()), "vs_rmsnorm_act")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0) and _guards_intact(xbuf, NAN)
    assert (og[:, C:] == 0).all()
    assert torch.equal(og[R.RMS_ZERO_ROW, :C].cpu(), add[R.RMS_ZERO_ROW])
    R.envelope(f"rmsnorm_act silu+add rows={rows} C={C}", [_rows(og[:, :C], r64, r32)])


# ------------------------------------------------------------------------------------------------------------------------ GRN
@pytest.mark.parametrize("B,HW,C,ld", R.GRN_CASES)
def test_grn_scale_fp64_envelope(B, HW, C, ld):
    """vs_grn_scale: channels of mean 30 / std 0.5, a constant channel, one whose norm a single 4e3 outlier carries, one of magnitude 1e-3; every
    (frame, channel) element of the scale is its own group; pad lanes of the scale are zero"""
    L = N.lib()
    h, gamma, _ = R.grn_inputs(B, HW, C)
    r64, r32 = R.grn_ref(h, gamma)
    hbuf, hg = _guarded(_padded(h.reshape(-1, C), ld).to(DEV), NAN)
    pbuf, part = _guarded(torch.full((((HW + 63) // 64) * B * C,), NAN, device=DEV), -7.0)
    sbuf, scale = _guarded(torch.full((B, ld), NAN, device=DEV), -7.0)
    gd = dv(gamma)
    N.check(L.vs_grn_scale(N.ptr(hg), B, HW, C, ld, N.ptr(gd), N.ptr(part), N.ptr(scale), N.stream()), "vs_grn_scale")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, -7.0) and _guards_intact(pbuf, -7.0) and _guards_intact(hbuf, NAN)
    assert (scale[:, C:] == 0).all()
    R.envelope(f"grn_scale B={B} HW={HW} C={C} ld={ld}", [("scale/elem", E.group_err(scale[:, :C], r64, None), E.group_err(r32, r64, None))])


def _grn_apply_lines(L, h, scale, sld, beta, r64s, r32s):
    """vs_grn_apply with the scale just computed: h * scale + beta in place, per row, against the float64 formula on the float64 scale"""
    B, HW, C = h.shape
    ld = rup(C, 4)
    hbuf, hg = _guarded(_padded(h.reshape(-1, C), ld).to(DEV), -7.0)
    bd = _pad1(beta, ld)
    N.check(L.vs_grn_apply(N.ptr(hg), B, HW, C, ld, N.ptr(scale), sld, N.ptr(bd), N.stream()), "vs_grn_apply")
    torch.cuda.synchronize()
    assert _guards_intact(hbuf, -7.0) and (hg[:, C:] == 0).all()
    a64 = h.double() * r64s[:, None] + beta.double()
    a32 = h * r32s[:, None] + beta
    return _rows(hg[:, :C].view(B, HW, C), a64, a32, "apply/row")


@pytest.mark.parametrize("B,HW,C", [(3, 96, 200), (2, 64, 600)])
def test_grn_scale_from_partials_fp64_envelope(B, HW, C):
    """vs_grn_scale_from_partials (frame-major partials, grn_finish_kernel<2,16> and <4,8>) fed by fp32 partials formed on the CPU in the
    documented order (per 32-row group, rows ascending) from the hard channels, then vs_grn_apply: against the float64 formula on the same h"""
    L = N.lib()
    h, gamma, beta = R.grn_inputs(B, HW, C, seed=1500)
    r64, r32 = R.grn_ref(h, gamma)
    sld = rup(C, 4) + 4
    pbuf, part = _guarded(R.grn_partials32(h).to(DEV), NAN)
    sbuf, scale = _guarded(torch.full((B, sld), NAN, device=DEV), -7.0)
    gd = dv(gamma)
    N.check(L.vs_grn_scale_from_partials(N.ptr(part), B, HW, C, N.ptr(gd), N.ptr(scale), sld, N.stream()), "vs_grn_scale_from_partials")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, -7.0) and _guards_intact(pbuf, NAN)
    assert (scale[:, C:] == 0).all()
    R.envelope(f"grn_scale_from_partials B={B} HW={HW} C={C}", [
        ("scale/elem", E.group_err(scale[:, :C], r64, None), E.group_err(r32, r64, None)),
        _grn_apply_lines(L, h, scale, sld, beta, r64, r32)])


@pytest.mark.parametrize("B,HW,C", [(3, 225, 200), (2, 961, 200), (5, 63, 40)])
def test_grn_scale_from_straddle_partials_fp64_envelope(B, HW, C):
    """vs_grn_scale_from_straddle_partials: 32-row groups that straddle the frames (225-, 961- and 63-row frames), fp32 partials formed on the CPU
    ([group][slot: the frame of the group's first row | the next][C], rows ascending), then vs_grn_apply"""
    L = N.lib()
    h, gamma, beta = R.grn_inputs(B, HW, C, seed=1600)
    r64, r32 = R.grn_ref(h, gamma)
    sld = rup(C, 4)
    pbuf, part = _guarded(R.grn_straddle_partials32(h).to(DEV), NAN)
    sbuf, scale = _guarded(torch.full((B, sld), NAN, device=DEV), -7.0)
    gd = dv(gamma)
    N.check(L.vs_grn_scale_from_straddle_partials(N.ptr(part), B, HW, C, N.ptr(gd), N.ptr(scale), sld, N.stream()), "straddle finish")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, -7.0) and _guards_intact(pbuf, NAN)
    assert (scale[:, C:] == 0).all()
    R.envelope(f"grn_scale_from_straddle_partials B={B} HW={HW} C={C}", [
        ("scale/elem", E.group_err(scale[:, :C], r64, None), E.group_err(r32, r64, None)),
        _grn_apply_lines(L, h, scale, sld, beta, r64, r32)])


# ------------------------------------------------------------------------------------------------------------------------ vs_vit_attention
def attention_check(case, kernel, got):
    cfg, rel = case
    qkv, rh, rw = R.attn_inputs(cfg, rel)
    r64, r32 = R.attn_ref(qkv, rh, rw, cfg)
    assert torch.isfinite(got).all()
    R.envelope(f"vit_attention {kernel} {cfg}{'' if rel else ' no tables'}", R.attn_lines(got, r64, r32, cfg[3]))


def _attn_id(case):
    return f"{case[0]}{'' if case[1] else '-notables'}"


@pytest.mark.parametrize("case", R.ATTN_VALU_CASES + R.ATTN_MFMA_CASES, ids=_attn_id)
def test_vit_attention_fp64_envelope(case):
    """both attention kernels as the library dispatches them (vector kernel: 16 and 96 tokens per group; matrix cores: 64 / 128 / 256 tokens,
    heads of 16 / 32 / 64) on peaked softmax rows (logits of std 40), a uniform row, V of mean 30 / std 0.5 and of magnitude 1e-4, with and
    without relative-position tables: every (token, head) slice of the output is a group"""
    attention_check(case, "mfma" if case in R.ATTN_MFMA_CASES else "valu", attention_launch(case))


@pytest.mark.parametrize("case", R.ATTN_MFMA_CASES, ids=_attn_id)
def test_vit_attention_vector_kernel_on_the_matrix_core_shapes_fp64_envelope(case):
    """the vector kernel on the matrix-core shapes: what VS_VIT_ATTN=valu selects, here through its development switch"""
    with N.debug("VIT_ATTN", 1):
        got = attention_launch(case)
    attention_check(case, "VS_VIT_ATTN=valu", got)
