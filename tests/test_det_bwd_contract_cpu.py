"""The envelope of tests/test_gpu_det_bwd_envelope.py has teeth: on the very inputs the GPU file uses, the kernels' formulas in fp32 torch arithmetic
(tests/_det_bwd_ref.py) are finite and inside max(yardstick, 1) x 8 on every line, while each seeded defect falls outside at the cap -- no margin up to
8 admits it -- on the kind it is named for; the zeroed kind-1 head is accepted by the old `2e-4 of the largest value` criterion on at least two cases;
and the hard inputs hold what they promise.  Nothing here needs a GPU."""
import math

import pytest
import torch

from tests import _det_bwd_ref as D
from tests import _envelope as E
from tests import _fwd_ref as R

F32, F64 = torch.float32, torch.float64


def _outside(r, r_ref):
    return E.outside(r, r_ref, 1.0)


def _inside(tag, r, yard):
    for name in yard:
        print(f"MODEL {tag:<60s} {name:<10s} model {r[name]:12.3f}  aten-fp32 {yard[name]:12.3f}")
        assert math.isfinite(yard[name]) and math.isfinite(r[name]), (tag, name)
        assert not _outside(r[name], yard[name]), (tag, name, r[name], yard[name])


# ------------------------------------------------------------------------------------------------------------------------ hard inputs
def test_hard_inputs_hold_what_they_promise():
    for cfg, rel in D.ATTN_CASES:
        B, H, W, heads, hd, win = cfg
        qkv, rh, rw = D.attn_case_inputs(cfg, rel, "hard")
        q, k, v = D.grouped_qkv(qkv, cfg)
        G = q.shape[0]
        assert not q[0::heads, R.UNIFORM_QUERY].any(), "the uniform query of head 0"
        if G > heads:
            assert bool((k[heads - 1] == k[heads - 1][0]).all()), "identical keys in the last head of group 0"
        assert (rh is None) == (not rel) and (rw is None) == (not rel)
        p = D._scores(q.double(), k.double(), None if rh is None else rh.double(), None if rw is None else rw.double(), *((win, win) if win else (H, W)), hd).softmax(-1)
        assert float(p.amax(-1).median()) > 0.9, "peaked rows"
        assert bool(((p[0, R.UNIFORM_QUERY] - 1 / p.shape[-1]).abs() < 1e-12).all())
        for kind in D.DO_KINDS:
            do = D.attn_dout(cfg, kind)
            assert do.shape == (B, H, W, heads, hd) and bool(torch.isfinite(do).all())
        imp = D.attn_dout(cfg, "impulse")
        assert [int((imp[b] != 0).sum()) for b in range(B)] == [1] * B
        hs, nz = D.attn_dout(cfg, "head-scaled"), D.attn_dout(cfg, "noise")
        assert torch.equal(hs[:, :, :, heads - 1], nz[:, :, :, heads - 1] * 1e-4) and torch.equal(hs[:, :, :, :heads - 1], nz[:, :, :, :heads - 1])
    cfg, _ = D.SMALL_CASE
    assert cfg[0] * cfg[3] < 64 and cfg[1] * cfg[2] < 64          # fewer groups than RP_CHUNKS, fewer tokens than the launch width
    # the sweep of the activation derivatives
    z = D.gelu_sweep()
    assert z.shape == (D.GELU_ROWS, D.GELU_C) and D.GELU_C % 4 and D.GELU_LD > (D.GELU_C + 3) // 4 * 4 and D.GELU_ROWS % 3 == 0
    f = z.flatten()
    dense = f[:f.numel() - D.gelu_special_points().numel()]
    assert dense.numel() >= 4096 and dense[0] == -9 and dense[-1] == 9 and float((dense[1:] - dense[:-1]).max()) < 5e-3
    sp = D.gelu_special_points().tolist()
    c32, x32 = float(torch.tensor(D.CLAMP, dtype=F32)), float(torch.tensor(D.CROSSING, dtype=F32))
    for v in (13.5, -13.5, 100.0, -100.0, 4e3, -4e3, D.SUBNORMAL, -D.SUBNORMAL, c32, -c32, x32, float(torch.tensor(1e-8, dtype=F32)), -float(torch.tensor(1e-8, dtype=F32))):
        assert v in sp, v
    assert sum(1 for v in sp if v == 0) == 2 and any(math.copysign(1, v) < 0 for v in sp if v == 0)
    for c in (c32, -c32, x32):
        assert any(v < c and abs(v - c) <= abs(c) * 2.0 ** -22 for v in sp) and any(v > c and abs(v - c) <= abs(c) * 2.0 ** -22 for v in sp), c
    assert float(torch.tensor(D.SUBNORMAL, dtype=F32)) > 0 and float(torch.tensor(D.SUBNORMAL, dtype=F32) * 0.5) == 0
    d = D.act_grad64(torch.tensor([x32 - 1e-3, x32 + 1e-3]), "gelu")
    assert d[0] < 0 < d[1], "the zero crossing of gelu'"
    dy = D.gelu_dy()
    assert float(dy[D.SCALED_ROW].abs().max()) < 1e-3 < float(dy[0].abs().max())
    # the depthwise shapes
    assert D.dw_bands(*D.DW_SHAPES[-1][:2]) == (2, 32) and D.DW_SHAPES[-1][1] % 2 == 1          # RB = 2, the 32nd band holds one row
    assert all(D.dw_bands(B, H)[0] == 1 for B, H, W, C, ld in D.DW_SHAPES[:-1])
    assert D.DW_SHAPES[3][2] == 2 * 7 + 1
    for B, H, W, C, ld in D.DW_SHAPES:
        x, w, bias, add = D.dw_inputs(B, H, W, C)
        assert x.shape == (B, C, H, W) and bool((x[:, 1] == 30.25).all()) and float(x[:, 2].max()) == 4e3 and float(x[:, 3].abs().max()) < 0.01
        assert abs(float(x[:, 0].mean()) - 30) < 1
        assert float(w[D.SMALL_CHANNEL].abs().max()) < 2e-5 and not w[D.SPARSE_CHANNEL].view(-1)[1::2].any() and w[D.SPARSE_CHANNEL].view(-1)[0::2].all()
        assert set(D.dw_dy(B, H, W, C, "checker").unique().tolist()) <= {-1.0, 1.0}


# ------------------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("case", D.ATTN_CASES, ids=D.attn_case_id)
def test_attention_model_is_inside_and_the_fp64_model_is_the_autograd(case):
    """the kernel's formulas in fp32 torch arithmetic on every input and dO kind: finite and inside at the cap; the same formulas in float64 agree with
    the float64 autograd to 1e-6 of a unit's 2^24-fold (the model and the units restate the kernel; the reference does not)"""
    cfg, rel = case
    for ik in D.ATTN_INPUT_KINDS:
        for dk in D.DO_KINDS:
            (qkv, rh, rw), do, ref, units, yard = D.attn_reference(case, ik, dk)
            _inside(f"attn {D.attn_case_id(case)} {ik} dO={dk}", D.attn_r(D.attn_model(qkv, rh, rw, cfg, do), ref, units, cfg[3]), yard)
            m64 = D.attn_r(D.attn_model(qkv, rh, rw, cfg, do, F64), ref, units, cfg[3])
            assert max(m64.values()) < 1e-3, (ik, dk, m64)
            if ik == "randn":
                # O(1) logits: the unit covers the whole of the error.  ATen's fp32 measured 1 - 25 units on these lines and up to 630 with an impulse
                # (55 with this one); beyond twice that the unit is off, not the arithmetic
                assert max(yard.values()) < (1260 if dk == "impulse" else 50), (dk, yard)


# defect -> (input kind, dO kind, the lines that must be outside); `tables`: only the cases with tables show it
ATTN_TEETH = {
    "no-D": ("hard", "noise", ("dq", "dk"), False),
    "dk-no-scale": ("randn", "noise", ("dk",), False),
    "dq-last-key": ("randn", "noise", ("dq",), False),
    "gw-first-row": ("randn", "noise", ("dq", "drw"), True),
    "mirrored-index": ("randn", "noise", ("dq", "drh", "drw"), True),
    "table-groups-of-4": ("randn", "noise", ("drh", "drw"), True),
    "no-max": ("hard", "noise", ("dq", "dk", "dv"), False),
}


@pytest.mark.parametrize("defect", sorted(ATTN_TEETH))
def test_attention_defect_falls_outside(defect):
    ik, dk, lines, tables = ATTN_TEETH[defect]
    seen = 0
    for case in D.ATTN_CASES:
        cfg, rel = case
        if tables and not rel:
            continue
        (qkv, rh, rw), do, ref, units, yard = D.attn_reference(case, ik, dk)
        G = ref["dq"].shape[0]
        if defect == "table-groups-of-4" and G % 4 == 0:
            continue
        r = D.attn_r(D.attn_model(qkv, rh, rw, cfg, do, defect=defect), ref, units, cfg[3])
        for n in lines:
            print(f"TEETH attn {defect:<18s} {D.attn_case_id(case):<24s} {n:<4s} defect {r[n]:12.4g}  aten-fp32 {yard[n]:10.3f}")
            assert _outside(r[n], yard[n]), (defect, case, n, r[n], yard[n])
        seen += 1
    assert seen >= 3


def test_zeroed_kind1_head_is_outside_and_the_old_criterion_accepts_it():
    """dq of every head whose V is 1e-4 set to zero, on the hard inputs with noise upstream: millions of units out on that head's line, while
    max |error| <= 2e-4 max |gradient| over the whole of dqkv (tests/test_gpu_bwd.py) still holds on at least two cases"""
    accepted, seen = 0, 0
    for case in D.ATTN_CASES:
        cfg, rel = case
        heads = cfg[3]
        if heads == 1:
            continue          # a single head takes kind 1: the whole of dq is then zero, which any criterion sees
        (qkv, rh, rw), do, ref, units, yard = D.attn_reference(case, "hard", "noise")
        bad = D.attn_model(qkv, rh, rw, cfg, do, defect="kind1-dq-zero")
        r = D.attn_r(bad, ref, units, heads)
        old = D.old_criterion_accepts(bad, ref)
        h1 = [h for h in range(heads) if R._vkind(h, heads) == 1][0]
        print(f"TEETH attn kind1-dq-zero {D.attn_case_id(case):<24s} dq/head{h1} defect {r[f'dq/head{h1}']:12.4g}  aten-fp32 {yard[f'dq/head{h1}']:10.3f}  "
              f"old criterion {'accepts' if old else 'rejects'}")
        assert _outside(r[f"dq/head{h1}"], yard[f"dq/head{h1}"]) and _outside(r["dq"], yard["dq"]), (case, r, yard)
        accepted += old
        seen += 1
    assert seen >= 5 and accepted >= 2, (seen, accepted)


# ------------------------------------------------------------------------------------------------------------------------ GELU'
def test_gelu_fit_is_inside_and_its_defects_fall_outside():
    z, dy = D.gelu_sweep(), D.gelu_dy()
    rows = D.act_lines("fit", dy * D.gelu_grad_fit(z), z, dy, "gelu")
    for name, r, yard in rows:
        print(f"MODEL gelu' {name:<16s} model {r:12.3f}  aten-fp32 {yard:12.3f}")
        assert math.isfinite(r) and math.isfinite(yard) and not _outside(r, yard), (name, r, yard)
    named = {"no-zphi-beyond-4": "(a)", "clamp-at-4": "(a)", "branches-swapped": "(a)"}
    for defect in D.GELU_DEFECTS:
        for name, r, yard in D.act_lines(defect, dy * D.gelu_grad_fit(z, defect), z, dy, "gelu"):
            print(f"TEETH gelu' {name:<32s} defect {r:12.4g}  aten-fp32 {yard:12.3f}")
            if named[defect] in name:
                assert _outside(r, yard), (name, r, yard)
    # the tail line sees a relative defect the absolute line cannot: Phi off by 1e-3 of itself on z < -3
    bad = D.gelu_grad_fit(z)
    bad = torch.where(z < -3, bad + 1e-3 * D.Phi(z.double()).float(), bad)
    la, lb = D.act_lines("phi-1e-3", dy * bad, z, dy, "gelu")
    print(f"TEETH gelu' phi-1e-3: (a) {la[1]:.3f} vs {la[2]:.3f}   (b) {lb[1]:.4g} vs {lb[2]:.4g}")
    assert not _outside(la[1], la[2]) and lb[1] > 0.5 * 1e-3 * 2 ** 24 * 0.1


@pytest.mark.parametrize("act", ["silu", "tanh", "relu"])
def test_other_derivatives_have_a_finite_yardstick(act):
    z, dy = D.gelu_sweep(), D.gelu_dy()
    (name, r, yard), = D.act_lines(act, D.act_yardstick(z, dy, act), z, dy, act)
    print(f"MODEL {act}' (a) aten-fp32 {yard:.3f}")
    assert math.isfinite(yard) and r == yard
    assert _outside(*D.act_lines(act, 1.001 * D.act_yardstick(z, dy, act), z, dy, act)[0][1:]), "a derivative off by 1e-3"


# ------------------------------------------------------------------------------------------------------------------------ depthwise 7 x 7
@pytest.mark.parametrize("shape", D.DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv7_formulas_are_inside_and_the_defects_fall_outside(shape):
    B, H, W, C, ld = shape
    x, w, bias, add = D.dw_inputs(B, H, W, C)
    f64, f32 = D.dw_refs(lambda dt: D.dw_forward(x, w, bias, dt))
    tag = "x".join(map(str, shape))
    for dk in D.DW_DY_KINDS:
        dy = D.dw_dy(B, H, W, C, dk)
        units = D.dw_units(x, w, bias, add, dy)
        if dk == D.DW_DY_KINDS[0]:
            yf = D.units_err(f32, f64, units["fwd"])
            print(f"MODEL dwconv7 {tag} forward aten-fp32 {yf:.3f}")
            assert math.isfinite(yf)
        g64, g32 = D.dw_refs(lambda dt: D.dw_data_grad(dy, w, add, dt))
        w64, w32 = D.dw_refs(lambda dt: D.dw_weight_grad(x, dy, dt))
        yg, yw = D.units_err(g32, g64, units["flip"]), D.units_err(w32, w64, units["wgrad"])
        mg, mw = D.units_err(D.dw_flip(dy, w, add), g64, units["flip"]), D.units_err(D.dw_wgrad(x, dy), w64, units["wgrad"])
        print(f"MODEL dwconv7 {tag} dy={dk:<8s} flip model {mg:8.3f} aten-fp32 {yg:8.3f}   wgrad model {mw:8.3f} aten-fp32 {yw:8.3f}")
        assert not _outside(mg, yg) and not _outside(mw, yw)
        bg = D.units_err(D.dw_flip(dy, w, add, "centre-row-not-flipped"), g64, units["flip"])
        print(f"TEETH dwconv7 {tag} dy={dk:<8s} centre-row-not-flipped {bg:12.4g}")
        if W > 1 and dk == "noise":          # (W = 1: the centre row's only tap inside the image is the centre tap itself)
            assert _outside(bg, yg), (dk, bg, yg)
        if W > 7:
            bw = D.units_err(D.dw_wgrad(x, dy, "window-slot"), w64, units["wgrad"])
            print(f"TEETH dwconv7 {tag} dy={dk:<8s} window-slot {bw:12.4g}")
            assert _outside(bw, yw), (dk, bw, yw)
        if D.dw_bands(B, H)[0] > 1:
            bw = D.units_err(D.dw_wgrad(x, dy, "band-last-row"), w64, units["wgrad"])
            print(f"TEETH dwconv7 {tag} dy={dk:<8s} band-last-row {bw:12.4g}")
            assert _outside(bw, yw), (dk, bw, yw)
