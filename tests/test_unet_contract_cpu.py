"""The envelope of tests/test_gpu_unet_envelope.py stands on firm ground and has teeth, and every export of the library is accounted for.
  * The float64 references of tests/_unet_ref.py agree with independent implementations (torch modules, oracle/videoseal_ref.py) on ordinary inputs.
  * The conditions the GPU file puts on its inputs hold for the reference alone: the share left out of the gated ReLU comparison, the saturated
    delta, a message table on which the fp32 yardstick has a real error.
  * Seeded fp32 emulations of defects that the single-shape tests of tests/test_gpu_kernels.py accept fall outside  8 x max(yardstick, floor)
    on the inputs and shapes of the GPU file -- the yardstick's own ratio is 1, so no UNET_MARGIN up to the cap admits them.
  * The export ledger (tests/_ledger.py) lists every function include/videoseal_hip.h declares, and the module it names does name the symbol.
Nothing here needs a GPU."""
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import videoseal_ref as O
from tests import _envelope as E
from tests import _ledger
from tests import _unet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))
    assert err <= tol, err


# ------------------------------------------------------------------------------------------------------------------------ references
def test_bn_fold_is_batchnorm2d_over_two_steps():
    """scale / shift reproduce the module's output and the running statistics follow it over two training steps (momentum 0.1, unbiased variance)"""
    g = torch.Generator().manual_seed(1)
    C = 6
    bn = nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.5 * torch.rand(C, generator=g))
        bn.bias.copy_(0.3 * torch.randn(C, generator=g))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for step in range(2):
        x = torch.randn(3, C, 5, 7, dtype=D, generator=g) * 2 + 1
        y = bn(x)
        rows = x.permute(0, 2, 3, 1).reshape(-1, C)
        sc, sh, rm, rv = R.bn_fold(rows, bn.weight.detach(), bn.bias.detach(), rm, rv, 0.1)
        _close((rows * sc + sh), y.detach().permute(0, 2, 3, 1).reshape(-1, C))
        _close(rm, bn.running_mean)
        _close(rv, bn.running_var)
        add = torch.randn(rows.shape, dtype=D, generator=g)
        _close(R.ssa(rows, sc, sh, 1, add), R.bn_relu_add(rows, bn.weight.detach(), bn.bias.detach(), add)[0])


def test_activations_are_the_torch_modules():
    v = torch.linspace(-6, 6, 101, dtype=D)
    for act, mod in ((1, nn.ReLU()), (2, nn.GELU()), (3, nn.Tanh()), (4, nn.SiLU())):
        assert torch.equal(R.act_fn(act)(v), mod(v))
    assert torch.equal(R.act_fn(0)(v), v)


def test_upcat_is_upsample_of_the_concat_and_the_written_out_bilinear_agrees():
    g = torch.Generator().manual_seed(2)
    for B, H, W, C1, C2 in [(2, 7, 9, 3, 2), (1, 1, 5, 2, 2), (1, 6, 1, 2, 2), (1, 1, 1, 1, 1), (1, 2, 2, 1, 1)]:
        x, sk = torch.randn(B, C1, H, W, dtype=D, generator=g), torch.randn(B, C2, H, W, dtype=D, generator=g)
        want = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)(torch.cat((x, sk * 2 ** -0.5), 1))
        _close(R.upcat(x, sk, 2 ** -0.5), want)
        _close(R.bilinear2x(torch.cat((x, sk * 2 ** -0.5), 1)), want)
        # the adjoint: <up(v), d> = <v, up^T d>
        d = torch.randn(want.shape, dtype=D, generator=g)
        dx, ds = R.upcat_bwd(d, C1, 2 ** -0.5)
        lhs, rhs = float((want * d).sum()), float((x * dx).sum() + (sk * ds).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_msg_latent_is_the_oracle_embedding_sum_and_the_table_gradient_is_its_autograd():
    Bm, nbits, hidden = 3, 15, 24
    table, msgs = R.msg_table("randn", nbits, hidden).double(), R.msg_bits(Bm, nbits)
    want = O.msg_latent({"embedder.unet.msg_processor.msg_embeddings.weight": table}, msgs)
    emb = nn.Embedding(2 * nbits, hidden).double()
    with torch.no_grad():
        emb.weight.copy_(table)
    lat = emb(R.msg_rows(msgs)).sum(-2)
    _close(R.msg_latent(table, msgs), want)
    _close(lat.detach(), want)
    dlat = torch.randn(Bm, hidden, dtype=D, generator=torch.Generator().manual_seed(3))
    lat.backward(dlat)
    _close(R.msg_table_grad(dlat, msgs), emb.weight.grad)


def test_pool_linear_is_adaptive_avgpool_and_linear():
    g = torch.Generator().manual_seed(4)
    B, H, W, C, N = 2, 5, 7, 12, 9
    x = torch.randn(B, C, H, W, dtype=D, generator=g)
    lin = nn.Linear(C, N).double()
    want = lin(nn.AdaptiveAvgPool2d(1)(x).flatten(1))
    _close(R.pool_linear(x.permute(0, 2, 3, 1).reshape(B, H * W, C), lin.weight.detach(), lin.bias.detach()), want.detach())


def test_outc_is_the_1x1_conv_with_tanh_and_its_adjoint_is_autograd():
    g = torch.Generator().manual_seed(5)
    B, H, W, C, Co = 2, 3, 4, 6, 3
    x = torch.randn(B, C, H, W, dtype=D, generator=g, requires_grad=True)
    w, b = torch.randn(Co, C, dtype=D, generator=g) / 2, torch.randn(Co, dtype=D, generator=g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, -1)          # noqa: E731
    for use_tanh in (0, 1):
        v = F.conv2d(x, w[:, :, None, None], b)
        y = torch.tanh(v) if use_tanh else v
        _close(R.outc(rows(x.detach()), w, b, use_tanh), rows(y.detach()))
        dd = torch.randn(y.shape, dtype=D, generator=g)
        x.grad = None
        y.backward(dd)
        dv, dx = R.outc_bwd(rows(y.detach()), rows(dd), w, use_tanh)
        _close(dx, rows(x.grad))


def test_msg_pre_is_the_zero_padded_conv_over_constant_message_channels():
    """conv3x3 (zero padding 1) over channels that are constant over space: every pixel's value is the table entry of its border class"""
    g = torch.Generator().manual_seed(6)
    Bm, Cm, N, H, W = 2, 5, 4, 4, 5
    Wt, lat = torch.randn(N, Cm, 3, 3, dtype=D, generator=g), torch.randn(Bm, Cm, dtype=D, generator=g)
    P = torch.einsum("nckl,bc->bkln", Wt, lat).reshape(Bm, 9 * N)                     # P[bm][tap * N + n]
    tab = R.msg_pre(P, N)
    y = F.conv2d(lat[:, :, None, None].expand(Bm, Cm, H, W), Wt, padding=1)
    cls = lambda i, n: 0 if i == 0 else (2 if i == n - 1 else 1)                        # noqa: E731
    for yy in range(H):
        for xx in range(W):
            _close(tab[:, cls(yy, H) * 3 + cls(xx, W)], y[:, :, yy, xx], 1e-11)


def test_patch_matrices_and_their_adjoints():
    """im2col3x3 (both pad modes, stride 1 / 2) turns F.conv2d into a matrix product; col2im_reflect and reflect_fold are adjoint to it / to the
    padding; dilate2 is the adjoint of taking every second pixel"""
    g = torch.Generator().manual_seed(7)
    B, C, H, W, Co = 2, 3, 5, 4, 2
    x, w = torch.randn(B, C, H, W, dtype=D, generator=g), torch.randn(Co, C, 3, 3, dtype=D, generator=g)
    wk = w.permute(2, 3, 1, 0).reshape(9 * C, Co)                                       # [(tap, c), n]
    for mode, stride in (("zeros", 1), ("zeros", 2), ("reflect", 1)):
        xp = F.pad(x, (1, 1, 1, 1), mode="reflect") if mode == "reflect" else F.pad(x, (1, 1, 1, 1))
        want = F.conv2d(xp, w, stride=stride)
        got = R.im2col3x3(x, mode, stride).reshape(-1, 9 * C) @ wk
        _close(got, want.permute(0, 2, 3, 1).reshape(-1, Co))
    dcols = torch.randn(B, H * W, 9, C, dtype=D, generator=g)
    lhs = float((R.im2col3x3(x, "reflect").view(B, H * W, 9, C) * dcols).sum())
    rhs = float((x * R.col2im_reflect(dcols, C, H, W)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    dxp = torch.randn(B, C, H + 2, W + 2, dtype=D, generator=g)
    lhs, rhs = float((F.pad(x, (1, 1, 1, 1), mode="reflect") * dxp).sum()), float((x * R.reflect_fold(dxp)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    dy = torch.randn(B, C, 3, 2, dtype=D, generator=g)
    assert torch.equal(R.dilate2(dy, H, W)[:, :, ::2, ::2], dy) and int((R.dilate2(dy, H, W) != 0).sum()) == dy.numel()


# ------------------------------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("rows,C,ld", R.CHAIN_SHAPES)
def test_the_relu_gate_leaves_out_at_most_a_thousandth_and_the_yardstick_takes_every_decision(rows, C, ld):
    x, gamma, beta, add = R.chain_inputs(rows, C)
    (_, pre64), (_, pre32) = R.both(lambda dt: R.bn_relu_add(x.to(dt), gamma.to(dt), beta.to(dt), add.to(dt)))
    keep = R.relu_gate(x, gamma, beta, pre64)
    print(f"GATE rows={rows} C={C}: left out {1 - float(keep.mean()):.2e}")
    assert 1 - float(keep.mean()) <= 1e-3
    assert torch.equal(pre32 > 0, pre64 > 0)


def test_saturated_delta_holds_the_ends_and_their_neighbours():
    d = R.saturated_delta((2, 3, 257), 5)
    u = 2.0 ** -24
    for v in (1.0, -1.0, 1.0 - u, -(1.0 - u), 1.0 - 2 * u, 1.0 - 3 * u, 0.0):
        assert (d == v).any(), v
    assert float(d.abs().max()) == 1.0 and ((d.abs() < 0.8) & (d != 0)).any()
    z = R.relu_z(37, 3)
    bits = z.view(torch.int32)
    assert (bits == 0).any() and (bits == -2 ** 31).any()                              # +0 and -0
    assert ((z > 0) & (z < 2.0 ** -126)).any() and ((z < 0) & (z > -2.0 ** -126)).any()  # denormals of both signs


def test_the_shifted_table_gives_the_yardstick_a_real_error():
    """on the randn table ATen's fp32 sum stays below one unit of 2^-24 sum |t| at 1000 bits; on the table of mean 3 / std 0.5 it does not"""
    t, m = R.msg_table("shifted", 1000, 24), R.msg_bits(2, 1000)
    r64, r32 = R.msg_latent_ref(t, m)
    hard = R.units(r32, r64, R.msg_latent_mag(t, m))
    t = R.msg_table("randn", 1000, 24)
    r64, r32 = R.msg_latent_ref(t, m)
    easy = R.units(r32, r64, R.msg_latent_mag(t, m))
    print(f"YARDSTICK msg_latent 1000 bits: randn {easy:.3f} units, shifted {hard:.3f} units")
    assert easy < 1.0 < hard


# ------------------------------------------------------------------------------------------------------------------------ seeded defects
def _teeth(what, bad, yard, floor):
    print(f"TEETH {what}: yardstick {yard:.3e}, defect {bad:.3e}")
    assert E.outside(bad, yard, floor), (what, bad, yard)


def test_a_sequential_fp32_pool_falls_outside_at_961_rows():
    """ChunkySeal's 31 x 31 map, one-hot weights (the output IS the pooled mean): rows added one by one in fp32"""
    case = (2, 961, 96, 96, 5, True)
    assert case in R.POOL_CASES
    x, w, b = R.pool_inputs(2, 961, 96, 5, True)
    r64, r32 = R.pool_ref(x, w, b)
    mag = R.pool_mag(x, w, b)
    _teeth("pool_linear HW=961 sequential fp32", R.units(R.pool_ref(x, w, b, seq32=True)[1], r64, mag), R.units(r32, r64, mag), 1.0)


@pytest.mark.parametrize("Bm,nbits,hidden", [(2, 1000, 300), (2, 1024, 300)])
def test_a_sequential_fp32_latent_falls_outside_on_the_shifted_table(Bm, nbits, hidden):
    """the table rows added one by one in fp32.  (With 24 latent channels instead of 300 the worst of 48 outputs is 13.9 units against a yardstick
    of 2.0: inside 8 x 2.0 by a little, which is why the 1000-bit case is also run 300 wide)"""
    assert (Bm, nbits, hidden) in R.MSG_CASES
    t, m = R.msg_table("shifted", nbits, hidden), R.msg_bits(Bm, nbits)
    r64, r32 = R.msg_latent_ref(t, m)
    mag = R.msg_latent_mag(t, m)
    _teeth(f"msg_latent {nbits} bits sequential fp32", R.units(R.msg_latent_ref(t, m, seq32=True)[1], r64, mag), R.units(r32, r64, mag), 1.0)


@pytest.mark.parametrize("rows,C,ld", [s for s in R.BN_SHAPES if s[0] > 1])
def test_a_biased_running_variance_falls_outside(rows, C, ld):
    x, gamma, beta, rm, rv = R.bn_inputs(rows, C)
    r64, r32 = R.bn_ref(x, gamma, beta, rm, rv, 0.1)
    bad = R.bn_ref(x, gamma, beta, rm, rv, 0.1, biased_running=True)[1]
    _teeth(f"bn running_var biased rows={rows}", E.group_err(bad[3], r64[3], None), E.group_err(r32[3], r64[3], None), E.U32)


def test_a_shift_from_a_mean_summed_in_fp32_falls_outside():
    """`shift` = beta - mean * scale with the mean summed row by row in fp32, at the 2049-row shape: behind the 4e3 outlier (row 1024) every
    further row of that channel is added to a sum of 3.5e4 and loses eight bits, and the 2049 terms of the mean-30 channels lose up to eleven"""
    rows, C, ld = 2049, 6, 8
    assert (rows, C, ld) in R.BN_SHAPES
    x, gamma, beta, rm, rv = R.bn_inputs(rows, C)
    r64, r32 = R.bn_ref(x, gamma, beta, rm, rv, 0.1)
    bad = R.bn_ref(x, gamma, beta, rm, rv, 0.1, seq32_mean=True)[1]
    _teeth("bn shift from a sequential fp32 mean", E.group_err(bad[1], r64[1], None), E.group_err(r32[1], r64[1], None), E.U32)


def _by_class(rows):
    return {name.split("/")[1]: (err, yard) for name, err, yard in rows}


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("rows,C,ld,add_ld,out_ld", R.SSA_SHAPES)
def test_scale_shift_act_defects_fall_outside_in_their_channel_class(rows, C, ld, add_ld, out_ld, with_add):
    """The tanh approximation of GELU (off by up to 5e-4) and a result scaled by 1 + 3e-5 (about 500 ulp), scored like the GPU file scores the
    kernel: per channel class.  Scored against the worst channel of all, both pass: on the constant channel x * scale (about 1e4) cancels against
    shift and ATen's unfused fp32 multiply-add is 1e-4 .. 2e-3 off, which is asserted here as the reason for the classes.  On the channel of
    magnitude 1e-3 nothing cancels, the yardstick is a few units of 2^-24, and every activation is held to that"""
    x, sc, sh, add = R.ssa_inputs(rows, C)
    add = add if with_add else None
    for act in R.ACTS:
        r64, r32 = R.ssa_ref(x, sc, sh, act, add)
        yard = _by_class(R.class_rows("y", r32, r64, r32, 0))
        assert yard["const"][1] > 100 * max(yard["tiny"][1], E.U32) and yard["tiny"][1] < 8 * E.U32, (act, yard)
        gain = _by_class(R.class_rows("y", R.ssa_ref(x, sc, sh, act, add, gain=1 + 3e-5)[1], r64, r32, 0))
        _teeth(f"scale_shift_act x (1 + 3e-5) rows={rows} act={act} add={with_add}, channel of magnitude 1e-3", gain["tiny"][0], gain["tiny"][1], E.U32)
        assert not E.outside(gain["const"][0], gain["const"][1])                   # ... and would hide behind the constant channel's yardstick
        if act == 2:
            tg = _by_class(R.class_rows("y", R.ssa_ref(x, sc, sh, act, add, tanh_gelu=True)[1], r64, r32, 0))
            _teeth(f"scale_shift_act tanh-GELU rows={rows} add={with_add}, channel of magnitude 1e-3", tg["tiny"][0], tg["tiny"][1], E.U32)
            _teeth(f"scale_shift_act tanh-GELU rows={rows} add={with_add}, mean-30 channels", tg["mean30"][0], tg["mean30"][1], E.U32)


@pytest.mark.parametrize("case", R.UPCAT_CASES, ids=str)
def test_an_unclamped_source_index_falls_outside(case):
    B, H, W, C1, C2, _, _, _, s = case
    x, sk = R.frames("noise", B, C1, H, W), R.frames("noise", B, C2, H, W, seed=1)
    r64, r32 = R.upcat_ref(x, sk, s)
    mag = R.upcat_mag(x, sk, s)
    bad = R.upcat_ref(x, sk, s, no_clamp=True)[1]
    if H == 1 and W == 1:                    # a single source pixel: both taps are that pixel, the weights sum to 1 either way
        assert not E.outside(R.units(bad, r64, mag), R.units(r32, r64, mag), 1.0)
        return
    _teeth(f"upcat2x without the clamp {H}x{W}", R.units(bad, r64, mag), R.units(r32, r64, mag), 1.0)


@pytest.mark.parametrize("Bm,N", R.MSG_PRE_CASES)
def test_swapped_border_classes_fall_outside(Bm, N):
    P = 3.0 + 0.5 * torch.randn(Bm, 9 * N, generator=torch.Generator().manual_seed(Bm + N))
    r64, r32 = R.msg_pre_ref(P, N)
    mag = R.msg_pre(P.double().abs(), N)
    _teeth(f"msg_pre first / last swapped Bm={Bm} N={N}", R.units(R.msg_pre_ref(P, N, swap_defect=True)[1], r64, mag), R.units(r32, r64, mag), 1.0)


def test_one_minus_delta_in_place_of_one_minus_delta_squared_falls_outside():
    B, rpf, C, Cout, _ = R.OUTC_CASES[1]
    rows = B * rpf
    g = torch.Generator().manual_seed(rows + C)
    delta, dd, w = R.saturated_delta((rows, Cout), rows + C), torch.randn(rows, Cout, generator=g), torch.randn(Cout, C, generator=g)
    r64, r32 = R.outc_bwd_ref(delta, dd, w, 1)
    mv, mx = R.outc_bwd_mag(delta, dd, w, 1)
    bad = R.outc_bwd_ref(delta, dd, w, 1, linear_defect=True)[1]
    _teeth("outc_tanh_bwd dv with 1 - delta", R.units(bad[0], r64[0], mv), R.units(r32[0], r64[0], mv), 1.0)
    _teeth("outc_tanh_bwd dx with 1 - delta", R.units(bad[1], r64[1], mx), R.units(r32[1], r64[1], mx), 1.0)
    ends = delta.abs() == 1.0
    assert ends.any() and (r64[0][ends] == 0).all() and (r32[0][ends] == 0).all()      # the exact zeros the GPU test asks for


# ------------------------------------------------------------------------------------------------------------------------ the export ledger
def _header_exports():
    text = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.findall(r"(?m)^\s*(?:const\s+)?[A-Za-z_]\w*(?:\s*\*)?\s+\*?(vs_\w+)\s*\(", text)


def test_every_export_is_in_the_ledger():
    exports = _header_exports()
    assert len(exports) > 150 and len(set(exports)) == len(exports)
    names = [e[0] for e in _ledger.LEDGER]
    assert len(set(names)) == len(names), "an export is listed twice"
    assert not sorted(set(exports) - set(names)), f"exports without a ledger entry: {sorted(set(exports) - set(names))}"
    assert not sorted(set(names) - set(exports)), f"ledger entries that the header no longer declares: {sorted(set(names) - set(exports))}"
    sources = {}
    for name, kind, module, *wrapper in _ledger.LEDGER:
        assert kind in _ledger.KINDS, (name, kind)
        assert re.fullmatch(r"test_\w+\.py", module), (name, module)
        if module not in sources:
            sources[module] = open(os.path.join(ROOT, "tests", module)).read()
        word = wrapper[0] if wrapper else name
        assert re.search(r"\b" + re.escape(word) + r"\b", sources[module]), f"tests/{module} does not name {word} (ledger entry of {name})"
        if kind == "envelope":                # the module really applies the rule: it calls a binding of check_rows / check_units
            assert re.search(r"(?<![\w.])(?:[A-Za-z]\w*\.)?(?:check_rows|check_units|(?:[a-z]+_)?envelope(?:_units)?)\(", sources[module]), (name, module)


def test_the_header_parser_sees_a_new_declaration():
    """the ledger test would fail for a new export: the parser finds a declaration in the header's own style"""
    text = "int vs_brand_new(const float* x, int n,\n               void* stream);\nint64_t vs_brand_new_floats(int n);\nconst char* vs_name(void);"
    assert re.findall(r"(?m)^\s*(?:const\s+)?[A-Za-z_]\w*(?:\s*\*)?\s+\*?(vs_\w+)\s*\(", text) == ["vs_brand_new", "vs_brand_new_floats", "vs_name"]
