"""The envelope of tests/test_gpu_fwd_envelope.py has teeth: on the very inputs and shapes the GPU file uses, seeded fp32 emulations (plain torch,
tests/_fwd_ref.py) of the defects that the older parity tests accept fall outside  max(yardstick, 2^-24) x 8 -- the yardstick's own ratio is 1, so no
FWD_FP64_MARGIN up to the cap admits them -- while the yardstick itself is meaningful on every input (a row on which fp32 is meaningless would
make the GPU test vacuous).  The last two tests are the record of the gap: the criteria of tests/test_gpu_kernels.py accept a one-pass variance
and a softmax without the maximum on those tests' own randn inputs (single-plane probabilities they do reject: see there).  Nothing here needs a GPU."""
import pytest
import torch

from tests import _envelope as E
from tests import _fwd_ref as R

# what "meaningful" means for the yardstick: fp32 round-off times the condition of the hard rows -- mean 30 / std 0.5 loses log2(60) = 6 bits in
# x - u: 2^-24 * 60 = 4e-6, a few times that over a row.  Attention with logits of std 40 (|logit| up to ~130, error 2^-24 * sum |q_i k_i|
# ~ 1e-5 absolute in the exponent) on a near tie of the two largest logits between unlike rows of V: 1e-4 of the group's largest value.
LN_YARD, ATTN_YARD = 1e-4, 1e-3


def _ln_case_ids():
    return [f"{t} C={c}" for t, r, c, ld, fw in R.LN_CASES if not fw]


@pytest.mark.parametrize("case", [c for c in R.LN_CASES if not c[4]], ids=_ln_case_ids())
@pytest.mark.parametrize("act", R.LN_ACTS)
def test_layernorm_defects_fall_outside_the_envelope(case, act):
    tag, rows, C, ld, _ = case
    x, w, b = R.ln_inputs(rows, C)
    r64, r32 = R.ln_ref(x, w, b, act)
    yard = E.group_err(r32, r64, 1)
    one = E.group_err(R.ln_ref(x, w, b, act, one_pass=True)[1], r64, 1)
    print(f"TEETH layernorm {tag} C={C} act={act}: yardstick {yard:.3e}, one-pass variance {one:.3e}")
    assert yard < LN_YARD
    assert E.outside(one, yard)
    # ... and on a mean-30 row alone (row 0).  The outlier row (2) is listed, not asserted: its variance is the outlier's own square over C,
    # E[x^2] exceeds E[x]^2 by a factor of about C there and the one-pass form cancels nothing -- that row is hard for the MEAN (a sum of
    # 30s next to 4e3) and for a kernel that loses the small elements, not for this defect
    bad = R.ln_ref(x, w, b, act, one_pass=True)[1]
    for row in (0, 2):
        y1, d1 = E.group_err(r32[row:row + 1], r64[row:row + 1], 1), E.group_err(bad[row:row + 1], r64[row:row + 1], 1)
        print(f"TEETH layernorm {tag} C={C} act={act}: row {row}: yardstick {y1:.3e}, one-pass variance {d1:.3e}")
        assert row == 2 or E.outside(d1, y1), (row, d1, y1)
    if ld > C:
        wrong = E.group_err(R.ln_ref(x, w, b, act, div=ld)[1], r64, 1)
        print(f"TEETH layernorm {tag} C={C} act={act}: variance / ld {wrong:.3e}")
        assert E.outside(wrong, yard)


def _producer_cases():
    """(tag, ref(**defect), hard for the variance?) for every LayerNorm-behind-a-producer case of the GPU file, on its own inputs"""
    out = []
    for c in R.DW_CASES:
        out.append((f"dwconv7_ln {c}", lambda c=c, **d: R.dw_ref(*R.dw_inputs(*c), **d), True))
    for c in R.STEM_CASES:
        out.append((f"stem_conv_ln {c}", lambda c=c, **d: R.stem_ref(*R.stem_inputs(*c), c[0], **d), True))
    for c, zero in R.UPCONV_CASES:
        out.append((f"upconv {c} zero channel={zero}", lambda c=c, zero=zero, **d: R.upconv_ref(*R.upconv_inputs(*c, zero), 1, **d), not zero))
    f = R.PIXEL_CASE[2]
    for zero in (True, False):
        def pixel(zero=zero, **d):
            x, w, lw, lb = R.pixel_inputs(*R.PIXEL_CASE, zero)
            return R.upconv_ref(x, None, w, lw, lb, 2, f=f, **d)
        out.append((f"pixel_upgather {R.PIXEL_CASE} zero channel={zero}", pixel, not zero))
    return out


PRODUCERS = _producer_cases()


@pytest.mark.parametrize("case", PRODUCERS, ids=[c[0] for c in PRODUCERS])
def test_layernorm_behind_a_producer_one_pass_variance_falls_outside_the_envelope(case):
    """the LayerNorm input these kernels see is hard: the fp32 conv output of the GPU file's own inputs, normalised with a one-pass variance,
    leaves the envelope, while the written-out two-pass yardstick stays meaningful.  Not so where one of only 16 or 32 output channels has zero
    weights (the variant the up-conv and pixel-head cases also run): that entry near 0 gives the row a spread of 30 / sqrt(Co), the conv's own
    fp32 rounding then costs as much as the one-pass variance and the figure is listed, not asserted -- the variant without it is the hard one"""
    tag, ref, hard = case
    r64, r32 = ref()
    yard = E.group_err(r32, r64, -1)
    one = E.group_err(ref(one_pass=True)[1], r64, -1)
    print(f"TEETH {tag}: yardstick {yard:.3e}, one-pass variance {one:.3e}")
    assert yard < LN_YARD
    assert E.outside(one, yard) or not hard


@pytest.mark.parametrize("case", R.RMS_CASES)
def test_rmsnorm_yardstick_is_meaningful(case):
    rows, C = case
    x, gamma, add = R.rms_inputs(rows, C)
    r64, r32 = R.rms_ref(x, gamma, add)
    yard = E.group_err(r32, r64, 1)
    print(f"TEETH rmsnorm rows={rows} C={C}: yardstick {yard:.3e}")
    assert yard < 1e-6
    assert torch.equal(r64[R.RMS_ZERO_ROW], add[R.RMS_ZERO_ROW].double()) and torch.equal(r32[R.RMS_ZERO_ROW], add[R.RMS_ZERO_ROW])


@pytest.mark.parametrize("case", R.GRN_CASES)
def test_grn_mean_over_ld_falls_outside_the_envelope(case):
    B, HW, C, ld = case
    h, gamma, beta = R.grn_inputs(B, HW, C)
    r64, r32 = R.grn_ref(h, gamma)
    yard = E.group_err(r32, r64, None)
    wrong = E.group_err(R.grn_ref(h, gamma, div=ld)[1], r64, None)
    print(f"TEETH grn B={B} HW={HW} C={C} ld={ld}: yardstick {yard:.3e}, mean over ld {wrong:.3e}")
    assert ld > C and yard < 1e-5
    assert E.outside(wrong, yard)


ATTN_ALL = R.ATTN_VALU_CASES + R.ATTN_MFMA_CASES


@pytest.mark.parametrize("case", ATTN_ALL, ids=[f"{c}{'' if rel else ' no tables'}" for c, rel in ATTN_ALL])
def test_attention_defects_fall_outside_the_envelope(case):
    cfg, rel = case
    heads = cfg[3]
    qkv, rh, rw = R.attn_inputs(cfg, rel)
    r64, r32 = R.attn_ref(qkv, rh, rw, cfg)
    yard = R.attn_lines(r32, r64, r32, heads)
    assert all(y[1] < ATTN_YARD for y in yard), yard
    for mode in ("nomax", "nocorr", "plane", "plane2"):
        bad = R.attn_ref(qkv, rh, rw, cfg, mode)[1]
        lines = R.attn_lines(bad, r64, r32, heads)
        print(f"TEETH attention {cfg} rel={rel} {mode}: " + ", ".join(f"{n} {d:.3e} (yardstick {y:.3e})" for n, d, y in lines))
        if mode == "plane2":          # listed only: 2^-16 of a probability is at the yardstick's own level on these inputs
            continue
        assert E.outside(lines[0][1], lines[0][2]), (mode, lines[0])
        if mode == "nomax":
            assert not torch.isfinite(bad).all()          # exp overflows on the peaked rows
        if mode == "plane":                               # every head on its own line, whatever its V holds
            assert all(E.outside(d, y) for n, d, y in lines), lines


def test_uniform_query_is_the_mean_of_v():
    cfg = (1, 8, 8, 2, 16, 0)
    qkv, rh, rw = R.attn_inputs(cfg, True)
    r64, _ = R.attn_ref(qkv, rh, rw, cfg)
    v0 = qkv.view(64, 3, 2, 16)[:, 2, 0].double()
    assert (r64.view(64, 2, 16)[R.UNIFORM_QUERY, 0] - v0.mean(0)).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------ the gap
@pytest.mark.parametrize("C_,act", [(16, 1), (96, 0), (362, 2), (768, 2)])
def test_old_layernorm_criterion_accepts_a_one_pass_variance(C_, act):
    """tests/test_gpu_kernels.py::test_layernorm_act: randn * 3 + 1, |got - ref| < 2e-5 over the whole tensor"""
    g = torch.Generator().manual_seed(C_)
    x = (torch.randn(2, C_, 9, 7, generator=g) * 3 + 1).permute(0, 2, 3, 1)
    w, b = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    ref = R.layernorm(x, w, b, act)
    bad = R.layernorm(x, w, b, act, one_pass=True)
    assert (bad - ref).abs().max() < 2e-5


@pytest.mark.parametrize("cfg", [(2, 16, 16, 6, 64, 0), (3, 8, 8, 2, 16, 4), (1, 8, 16, 2, 32, 0)])
def test_old_attention_criterion_accepts_a_softmax_without_the_maximum(cfg):
    """tests/test_gpu_kernels.py::test_vit_attention: randn qkv, |got - ref| < 1e-5 over the whole tensor.  With logits O(1) nothing overflows
    and a softmax without the maximum passes (1e-6 .. 3e-6).  The truncated probability planes do NOT pass it in this emulation, so they are
    no part of the gap: one plane costs 4e-3 .. 7e-3, the flushed low plane 1.3e-5 .. 2e-5 (truncation is one-sided, the errors of a row add
    up); both figures are printed, neither is asserted"""
    qkv, rh, rw = R.randn_attn_inputs(cfg)
    ref = R.attention(qkv, rh, rw, cfg)
    err = {m: float((R.attention(qkv, rh, rw, cfg, m) - ref).abs().max()) for m in ("plane", "plane2", "nomax")}
    print(f"GAP attention {cfg}: " + ", ".join(f"{m} {e:.3e}" for m, e in err.items()))
    assert err["nomax"] < 1e-5
