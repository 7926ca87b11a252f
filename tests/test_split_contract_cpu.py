"""The arithmetic contract of the matrix-core kernels (csrc/conv_common.h, Arith<2> / Arith<3>) on the CPU, and the proof that the metric of
tests/test_gpu_split_envelope.py bites.  tests/_split_ref.py is the emulator; nothing here needs a GPU.

Test 1: the quantisation of the 2 x f16 split is what conv_common.h states -- per operand element, and per output element against an
a-priori bound formed from the emulator's own element errors.  Test 2: two deliberately wrong emulations (denormal low terms read as zero; the
l_a h_w product dropped on the last 16 of K) exceed SPLIT_MARGIN * max(r_ref, 1) on every shape and operand the GPU file uses, while the older
criterion (2e-5 of the tensor's largest value) accepts the first of them: the gap the envelope closes."""
import pytest
import torch

from tests import _split_ref as R

CONTRACT_CASES = [
    # tag, a [B, C, H, W], w, a_mul, conv kwargs
    ("gemm K=20", lambda: R.gemm_as_conv(R.hard_rows(67, 20, 11)), lambda: R.hard_weights(9, 20, 1, 12), 16.0, {}),
    ("gemm K=144", lambda: R.gemm_as_conv(R.hard_rows(131, 144, 13)), lambda: R.hard_weights(37, 144, 1, 14), 16.0, {}),
    ("gemm K=3456", lambda: R.gemm_as_conv(R.hard_rows(70, 3456, 15)), lambda: R.hard_weights(20, 3456, 1, 16), 16.0, {}),
    ("gemm K=144 a_mul=1", lambda: R.gemm_as_conv(R.hard_rows(131, 144, 17, gelu_like=True)), lambda: R.hard_weights(37, 144, 1, 18), 1.0, {}),
    ("conv3x3 zero", lambda: R.hard_act(2, 24, 13, 11, 19), lambda: R.hard_weights(20, 24, 3, 20), 16.0, dict(pad=1)),
    ("conv3x3 reflect", lambda: R.hard_act(2, 16, 9, 14, 21), lambda: R.hard_weights(12, 16, 3, 22), 16.0, dict(pad=1, reflect=True)),
    ("conv3x3 stride 2", lambda: R.hard_act(3, 16, 11, 10, 23), lambda: R.hard_weights(12, 16, 3, 24), 16.0, dict(pad=1, stride=2)),
]


def operand_errors_hold(xs, h, l):
    """|x mul - h - l| <= 2^-23 |x mul| where the low term is a normal f16 (|x mul - h| >= 2^-14), <= 2^-25 (half a denormal quantum) otherwise"""
    err = (xs - h.double() - l.double()).abs()
    normal = (xs - h.double()).abs() >= R.F16_MIN_NORMAL
    return bool((err[normal] <= 2.0 ** -23 * xs.abs()[normal]).all()) and bool((err[~normal] <= 2.0 ** -25).all())


@pytest.mark.parametrize("case", CONTRACT_CASES, ids=[c[0] for c in CONTRACT_CASES])
def test_split_quantisation_is_what_conv_common_says(case):
    tag, fa, fw, a_mul, kw = case
    a, w = fa(), fw()
    r = R.ideal(a, w, 2, a_mul, extras=True, **kw)
    ha, la = R.split_f16(a, a_mul)
    hw, lw, w_mul = R.split_f16_weights(w)
    assert torch.isfinite(ha.float()).all() and torch.isfinite(hw.float()).all()            # the 4e3 outlier is inside |a| < 4094
    assert 2 ** 13 <= (w.double().abs().max() * w_mul) < 2 ** 14
    assert operand_errors_hold(a.double() * a_mul, ha, la)
    assert operand_errors_hold(w.double() * w_mul, hw, lw)
    assert (la.float().abs() < R.F16_MIN_NORMAL).any() and (la != 0).any()                  # the denormal regime is exercised
    # S - true = -acc_mul sum_k (d_a w~ + a~ d_w - d_a d_w + l_a l_w),  d = the element's split error: bounded term by term.  Slack: the float64
    # rounding of the four matrix products themselves, 1e-12 of sum |p|
    slack = 1e-12 * r.P
    assert ((r.S - r.true).abs() <= r.bound + slack).all()
    cost = (r.S - r.true).abs().max() / r.true.abs().max()
    print(f"CONTRACT {tag}: worst |S - true| {float((r.S - r.true).abs().max()):.3e}, over the tensor's max {float(cost):.3e}")
    # arithmetic 3: three truncated bf16 terms that add up exactly -> S is the exact product
    for t in (a, w):
        p = R.split_bf16(t)
        assert torch.equal(p[0] + p[1] + p[2], t.double())
        assert all(torch.equal((q.float().view(torch.int32) & 0xffff), torch.zeros_like(q, dtype=torch.int32)) for q in p)
    r3 = R.ideal(a, w, 3, **kw)
    assert torch.equal(r3.S, r3.true)


TEETH = R.shapes_of_the_gpu_file()


@pytest.mark.parametrize("case", TEETH, ids=[c[0] for c in TEETH])
def test_the_envelope_metric_has_teeth(case):
    tag, build = case
    a, w, a_mul, kw = build()
    r = R.ideal(a, w, 2, a_mul, extras=True, **kw)
    r_ref = float(R.units(r.ref32, r.S, r.P).max())
    cap = R.SPLIT_MARGIN * max(r_ref, 1.0)
    flush, tail = float(R.units(r.S_flush, r.S, r.P).max()), float(R.units(r.S_tail, r.S, r.P).max())
    print(f"TEETH {tag}: ATen-fp32 {r_ref:.1f}, cap {cap:.1f}, flushed denormals {flush:.0f}, dropped tail {tail:.0f}  (units of 2^-24 sum|p|)")
    assert r_ref < 64.0                    # the comparator is itself an fp32 accumulation of the split operands, not something looser
    assert flush > cap and tail > cap
    # the record of the gap: the global-maximum criterion of the older parity tests does not see the flushed low plane
    assert R.old_criterion_accepts(r.S_flush, r.true)
    assert R.old_criterion_accepts(r.S, r.true)


def quantisation_cost_by_group(a_mul):
    """worst |S - true| / sum |a||w| per hard activation group (rows of a GEMM, K = 144, ordinary weights): the documented cost of the split, listed in
    profiles/split_fp64_envelope.txt"""
    rows, K = 36 * R.NGROUPS, 144
    a = R.hard_rows(rows, K, 31, gelu_like=(a_mul == 1.0))
    w = torch.randn(37, K, 1, 1, generator=torch.Generator().manual_seed(32)) / K ** 0.5      # plain weights: the activation side's cost alone
    r = R.ideal(R.gemm_as_conv(a), w, 2, a_mul)
    paw = (R.gemm_as_conv(a).double().abs()[0, :, :, 0].t() @ w.double().abs().view(37, K).t())
    q = ((r.S - r.true).abs()[0, :, :, 0].t() / paw.clamp_min(R.TINY))
    gid = R.group_ids(1, K, rows, 1)[0, 0, :, 0]
    return {R.GROUP_NAMES[i]: float(q[gid == i].max()) for i in range(R.NGROUPS)}


def test_documented_cost_of_the_denormal_regime():
    """on rows of magnitude 1e-4 at a_mul = 16 every low term is an f16 denormal: the split costs up to 2^-25 / (16 |a|) ~ 1e-5 of sum |a||w| there
    -- legitimate and 100 x fp32 round-off, which is why the GPU tests compare with the emulated split and not with the true product -- and
    stays at fp32 round-off on rows whose low terms are normal"""
    c16, c1 = quantisation_cost_by_group(16.0), quantisation_cost_by_group(1.0)
    print("COST a_mul=16", c16)
    print("COST a_mul=1 ", c1)
    # sum e_a |w| / sum |a||w| with e_a <= 2^-25 / 16 and |a| ~ 1e-4 E|randn| = 8e-5: ~ 2e-5
    assert 1e-6 < c16["magnitude 1e-4"] < 1e-4
    # normal low terms: 2^-23 per operand + the dropped l_a l_w <= 2^-22 |a w|
    assert c16["mean 30 / std 0.5"] < 2.0 ** -21 and c16["constant 0.37"] < 2.0 ** -21
    assert c16["exact zeros"] == 0.0 and c1["exact zeros"] == 0.0
    assert c1["magnitude 1e-4"] > c16["magnitude 1e-4"]
