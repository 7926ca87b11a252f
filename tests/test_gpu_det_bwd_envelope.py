"""fp64 envelopes of the detector's backward kernels that decide the extractor's gradients: vs_vit_attention_bwd (kernel Q, kernel K, the two
relative-position table kernels; csrc/bwd_vit.hip), the GELU derivative vs_gelu_grad (csrc/vs_common.h) through vs_gelu_bwd, vs_pool_gelu_bwd and vs_act_bwd
(with the other derivatives of vs_act_bwd), and vs_dwconv7 / vs_dwconv7_wgrad (csrc/bwd_ops.hip).  tests/_det_bwd_ref.py holds the formulas, hard inputs,
cases and units; tests/test_det_bwd_contract_cpu.py shows that the metric bites.  Every kernel is called through the C ABI: inputs sit between NaN bands,
outputs are pre-filled with a sentinel between -7.0 bands, every workspace has exactly the size its contract function returns, NaN-filled, between bands: the
bands must be intact and no sentinel may be left.  Every figure is printed as a DET-BWD-ENVELOPE line; profiles/det_bwd_fp64_envelope.txt is such a run on
an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _det_bwd_ref as D  # noqa: E402
from tests import _envelope as E  # noqa: E402
from tests._guards import _guarded, _guards_intact, scratch  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = 2.0 ** 120              # pre-fill of every output: no kernel under test produces it
F32 = torch.float32


def _in(t):
    return _guarded(t.to(DEV).contiguous(), NAN)


def _out(*shape):
    return _guarded(torch.full(shape, SENT, dtype=F32, device=DEV), -7.0)


def _ws(nelem):
    """a workspace of exactly the contract's size, NaN-filled, between bands"""
    return scratch(int(nelem), F32, NAN, DEV)


def _done(outs, ins=(), wss=()):
    """after the launch: every band intact, every output element written; returns the outputs on the CPU"""
    torch.cuda.synchronize()
    for buf, view in ins:
        assert _guards_intact(buf, NAN), "a band around an input changed"
    for buf, view in wss:
        assert _guards_intact(buf, -7.0), "a kernel wrote outside its workspace"
    res = []
    for buf, view in outs:
        assert _guards_intact(buf, -7.0), "a kernel wrote outside its output"
        v = view.cpu()
        assert not (v == SENT).any(), "an output element was not written"
        res.append(v)
    return res


def _same(got, want, what):
    if not torch.equal(got, want):
        ne = (got != want).flatten()
        first = int(ne.nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at flat index {first}: "
                             f"got {float(got.flatten()[first])!r} want {float(want.flatten()[first])!r}")


# ------------------------------------------------------------------------------------------------------------------------ vs_vit_attention_bwd
def _attention_bwd(cfg, qi, oi, rhi, rwi, do, table_grads):
    """one call: (dqkv, drh, drw) on the CPU (drh = drw = None without table gradients)"""
    L = N.lib()
    B, H, W, heads, hd, win = cfg
    di = _in(do.reshape(B, H, W, heads * hd))
    dqkv, ws = _out(B, H, W, 3 * heads * hd), _ws(L.vs_vit_attention_bwd_scratch_floats(B, H, W, heads, win))
    drh, drw = (_out(*rhi[1].shape), _out(*rwi[1].shape)) if table_grads else (None, None)
    N.check(L.vs_vit_attention_bwd(N.ptr(qi[1]), N.ptr(oi[1]), N.ptr(di[1]), B, H, W, heads, hd, win, N.ptr(rhi[1]) if rhi else None,
                                   N.ptr(rwi[1]) if rwi else None, N.ptr(dqkv[1]), N.ptr(ws[1]), N.ptr(drh[1]) if drh else None,
                                   N.ptr(drw[1]) if drw else None, N.stream()), "vs_vit_attention_bwd")
    res = _done([dqkv] + ([drh, drw] if table_grads else []), [qi, oi, di] + ([rhi, rwi] if rhi else []), [ws])
    return res if table_grads else res + [None, None]


@pytest.mark.parametrize("case", D.ATTN_CASES, ids=D.attn_case_id)
def test_vit_attention_bwd_fp64_envelope(case):
    """dq, dk, dv and the two table gradients on peaked rows (logit std 40), the uniform query, identical keys and the three V kinds, and on randn logits;
    dO noise, ones, an impulse and noise with one head scaled by 1e-4; in units of 2^-24 of the terms' magnitudes (D.attn_units), per quantity and per
    head for dq and dk.  `out` is the HIP forward's own output, as the engine passes it.  With tables: the call with table gradients twice (bit-identical)
    and the data-only pass (drel_h = drel_w = NULL), whose dqkv equals the first bit for bit; without: rel_h = rel_w = NULL"""
    L = N.lib()
    cfg, rel = case
    B, H, W, heads, hd, win = cfg
    for ik in D.ATTN_INPUT_KINDS:
        (qkv, rh, rw), _, _, _, _ = D.attn_reference(case, ik, D.DO_KINDS[0])
        qi = _in(qkv)
        rhi, rwi = (_in(rh), _in(rw)) if rel else (None, None)
        fwd = _out(B, H, W, heads * hd)
        N.check(L.vs_vit_attention(N.ptr(qi[1]), B, H, W, heads, hd, win, N.ptr(rhi[1]) if rel else None, N.ptr(rwi[1]) if rel else None, N.ptr(fwd[1]),
                                   N.stream()), "vs_vit_attention")
        oi = _in(_done([fwd], [qi])[0])
        for dk in D.DO_KINDS:
            _, do, ref, units, yard = D.attn_reference(case, ik, dk)
            dqkv, drh, drw = _attention_bwd(cfg, qi, oi, rhi, rwi, do, rel)
            again = _attention_bwd(cfg, qi, oi, rhi, rwi, do, rel)
            _same(again[0], dqkv, f"{ik} dO={dk}: dqkv of a second run")
            if rel:
                _same(again[1], drh, f"{ik} dO={dk}: drel_h of a second run")
                _same(again[2], drw, f"{ik} dO={dk}: drel_w of a second run")
                _same(_attention_bwd(cfg, qi, oi, rhi, rwi, do, False)[0], dqkv, f"{ik} dO={dk}: dqkv of the data-only pass")
            r = D.attn_r(D.as_quantities(dqkv, drh, drw, cfg), ref, units, heads)
            assert set(r) == set(yard)
            D.units_envelope(D.DET_BWD_MARGIN, f"vit_attention_bwd {D.attn_case_id(case)} {ik} dO={dk}", [(n, r[n], yard[n]) for n in yard])


# ------------------------------------------------------------------------------------------------------------------------ GELU' and the other derivatives
ACT_CODE = {"relu": N.ACT_RELU, "gelu": N.ACT_GELU, "tanh": N.ACT_TANH, "silu": N.ACT_SILU}


def _sweep():
    z, ld = D.gelu_sweep(), D.GELU_LD
    return z, _in(D.padded(z, ld, NAN)), ld          # (the pad columns are never read)


def test_gelu_bwd_fp64_envelope():
    """vs_gelu_bwd over [-9, 9] and the special points: (a) absolute in units of 2^-24 |dy|, (b) relative to Phi + |z| phi on the negative tail"""
    z, zi, ld = _sweep()
    dy = D.gelu_dy()
    di, dz = _in(D.padded(dy, ld, NAN)), _out(D.GELU_ROWS, ld)
    N.check(N.lib().vs_gelu_bwd(N.ptr(zi[1]), ld, N.ptr(di[1]), ld, D.GELU_ROWS, D.GELU_C, N.ptr(dz[1]), ld, N.stream()), "vs_gelu_bwd")
    got = _done([dz], [zi, di])[0]
    assert not got[:, D.GELU_C:].any(), "pad columns of dz"
    D.units_envelope(D.GELU_GRAD_MARGIN, "gelu_bwd", D.act_lines("dz", got[:, :D.GELU_C], z, dy, "gelu"))


@pytest.mark.parametrize("HW", [1, 3])
def test_pool_gelu_bwd_fp64_envelope(HW):
    """dz = dpooled / HW gelu'(z): HW = 1 is the derivative alone, HW = 3 adds the division and the frame index of every row"""
    z, zi, ld = _sweep()
    B = D.GELU_ROWS // HW
    dp = D.gelu_dy(B)
    di, dz = _in(D.padded(dp, ld, NAN)), _out(D.GELU_ROWS, ld)
    N.check(N.lib().vs_pool_gelu_bwd(N.ptr(zi[1]), ld, N.ptr(di[1]), ld, B, HW, D.GELU_C, N.ptr(dz[1]), ld, N.stream()), "vs_pool_gelu_bwd")
    got = _done([dz], [zi, di])[0]
    assert not got[:, D.GELU_C:].any(), "pad columns of dz"

    def yardstick():
        zz = z.clone().requires_grad_(True)
        torch.nn.functional.gelu(zz).view(B, HW, -1).mean(1).backward(dp)
        return zz.grad
    dy = (dp.double() / HW).repeat_interleave(HW, 0)          # what multiplies gelu'(z), in float64: the unit and the reference
    # the yardstick is ATen's autograd through the mean
    D.units_envelope(D.GELU_GRAD_MARGIN, f"pool_gelu_bwd HW={HW}", D.act_lines("dz", got[:, :D.GELU_C], z, dy, "gelu", E.one_thread(yardstick)))


@pytest.mark.parametrize("act", ["gelu", "silu", "tanh", "relu"])
def test_act_bwd_fp64_envelope(act):
    """every mode of vs_act_bwd on the same sweep: float64 derivative, ATen's fp32 autograd as the yardstick; ReLU is exact"""
    z, zi, ld = _sweep()
    dy = D.gelu_dy()
    di, dz = _in(D.padded(dy, ld, NAN)), _out(D.GELU_ROWS, ld)
    N.check(N.lib().vs_act_bwd(N.ptr(zi[1]), ld, N.ptr(di[1]), ld, D.GELU_ROWS, D.GELU_C, ACT_CODE[act], N.ptr(dz[1]), ld, N.stream()), "vs_act_bwd")
    got = _done([dz], [zi, di])[0]
    assert not got[:, D.GELU_C:].any(), "pad columns of dz"
    if act == "relu":
        _same(got[:, :D.GELU_C], dy * (z > 0), "relu'")
    D.units_envelope(D.GELU_GRAD_MARGIN, f"act_bwd {act}", D.act_lines("dz", got[:, :D.GELU_C], z, dy, act))


# ------------------------------------------------------------------------------------------------------------------------ vs_dwconv7 / vs_dwconv7_wgrad
@pytest.mark.parametrize("shape", D.DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv7_forward_flip_and_wgrad_fp64_envelope(shape):
    """forward with bias on channels of mean 30, a constant one, one with a 4e3 outlier and one of 1e-3; the flipped pass with `add` and the weight gradient on
    noise, ones and a checkerboard upstream; per element in units of 2^-24 of sum |w||x| + |bias| + |add| (per (tap, channel): sum |dy||x|).  `partial` is
    exactly vs_dwconv7_wgrad_partial_floats; two runs of the weight gradient are bit-identical"""
    L = N.lib()
    B, H, W, C, ld = shape
    x, w, bias, add = D.dw_inputs(B, H, W, C)
    xi, wi, bi, ai = _in(D.nhwc(x, ld)), _in(D.taps_first(w, ld)), _in(D.padded(bias[None], ld)[0]), _in(D.nhwc(add, ld))
    out = _out(B, H, W, ld)
    N.check(L.vs_dwconv7(N.ptr(xi[1]), B, H, W, C, ld, N.ptr(wi[1]), N.ptr(bi[1]), 0, None, 0, N.ptr(out[1]), ld, N.stream()), "vs_dwconv7")
    got = _done([out], [xi, wi, bi])[0]
    assert not got[..., C:].any(), "pad columns of the forward"
    f64, f32 = D.dw_refs(lambda dt: D.dw_forward(x, w, bias, dt))
    lines = []
    for dk in D.DW_DY_KINDS:
        dy = D.dw_dy(B, H, W, C, dk)
        units = D.dw_units(x, w, bias, add, dy)
        if not lines:
            lines.append(("forward", D.units_err(got[..., :C].permute(0, 3, 1, 2), f64, units["fwd"]), D.units_err(f32, f64, units["fwd"])))
        di, dx = _in(D.nhwc(dy, ld)), _out(B, H, W, ld)
        N.check(L.vs_dwconv7(N.ptr(di[1]), B, H, W, C, ld, N.ptr(wi[1]), None, 1, N.ptr(ai[1]), ld, N.ptr(dx[1]), ld, N.stream()), "vs_dwconv7")
        gx = _done([dx], [di, wi, ai])[0]
        g64, g32 = D.dw_refs(lambda dt: D.dw_data_grad(dy, w, add, dt))
        lines.append((f"dy={dk} flip+add", D.units_err(gx[..., :C].permute(0, 3, 1, 2), g64, units["flip"]), D.units_err(g32, g64, units["flip"])))
        runs = []
        for _ in range(2):
            ws, dw = _ws(L.vs_dwconv7_wgrad_partial_floats(B, H, ld)), _out(49, ld)
            N.check(L.vs_dwconv7_wgrad(N.ptr(xi[1]), ld, N.ptr(di[1]), ld, B, H, W, C, N.ptr(ws[1]), N.ptr(dw[1]), N.stream()), "vs_dwconv7_wgrad")
            runs.append(_done([dw], [xi, di], [ws])[0])
        _same(runs[1], runs[0], f"dy={dk}: the weight gradient of a second run")
        w64, w32 = D.dw_refs(lambda dt: D.dw_weight_grad(x, dy, dt))
        gw = runs[0][:, :C].t().reshape(C, 1, 7, 7)
        lines.append((f"dy={dk} wgrad", D.units_err(gw, w64, units["wgrad"]), D.units_err(w32, w64, units["wgrad"])))
    D.units_envelope(D.DET_BWD_MARGIN, f"dwconv7 {'x'.join(map(str, shape))}", lines)
