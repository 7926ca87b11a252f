"""fp64 envelopes of the detector's BACKWARD kernels that the earlier families left under a `fraction of the largest value` criterion: formulas, hard
inputs, cases, units and seeded defects shared by tests/test_det_bwd_contract_cpu.py (the envelope has teeth; no GPU) and
tests/test_gpu_det_bwd_envelope.py (every kernel against it).  Three parts:
    attention   vs_vit_attention_bwd (csrc/bwd_vit.hip): reference = float64 autograd of tests/_fwd_ref.py::attention, yardstick = its float32 autograd on
                one thread.  On peaked rows dq and dk are cancelled sums (ATen's own fp32 error per (token, head) row is 7e1 .. 4e9 relative to the row), so
                the error is measured in A-PRIORI UNITS: 2^-24 of the sum of the magnitudes of the terms, evaluated in float64 with the float64 softmax P
                (`attn_units`).  The unit leaves out the conditioning of P on the rounding of the logits; the yardstick carries that term.
    GELU'       vs_gelu_grad (csrc/vs_common.h) through vs_gelu_bwd, vs_pool_gelu_bwd and vs_act_bwd: reference = float64 Phi(z) + z phi(z), yardstick = ATen's
                fp32 F.gelu autograd; two lines per kernel, both per element: (a) absolute on the derivative's scale of 1, (b) relative to Phi + |z| phi on
                z in [-5.6, -1], the tail the erfc form exists to keep.
    dwconv7     vs_dwconv7 (forward, flipped backward-data pass with `add`) and vs_dwconv7_wgrad (csrc/bwd_ops.hip): reference = float64 F.conv2d and its
                autograd, yardstick = the same in fp32 on one thread; unit per element = 2^-24 of sum |w||x| + |bias| + |add| (per (tap, channel): sum |dy||x|).
Every line is r = max |got - ref64| / (2^-24 unit) of the kernel and of the yardstick, held by tests/_envelope.py::check_units: hip <= MARGIN max(yardstick, 1).
The torch emulations of the kernels' formulas (`attn_model`, `gelu_grad_fit`, `dw_flip`, `dw_wgrad`) exist for the CPU contract test and its seeded defects only."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import _envelope as E
from tests import _fwd_ref as R

F32, F64 = torch.float32, torch.float64
U = E.U32
FLOOR = 2.0 ** -102            # added to every unit: 2^-24 unit is then at least the smallest normal fp32 (2^-126), results that fp32 flushes are held absolutely
TAG, WIDTH = "DET-BWD-ENVELOPE", 78

# Twice the largest ratio hip / max(aten-fp32, 1) measured on an MI355X over every line of tests/test_gpu_det_bwd_envelope.py
# (profiles/det_bwd_fp64_envelope.txt lists them), never more than 8: a kernel that needs more has a defect.
DET_BWD_MARGIN = 8.0           # the cap: 2 x 4.467 = 8.93, the largest ratio measured: dv of vs_vit_attention_bwd on 2x4x4x1x16x0, hard rows, dO = ones (43.8 units, ATen 9.8)
GELU_GRAD_MARGIN = 2.386       # 2 x 1.193, the largest ratio measured: line (a) of vs_act_bwd in its tanh mode (1.82 units, ATen 1.52); GELU' itself: 0.873 (vs_pool_gelu_bwd, HW = 3)


def units_envelope(margin, case, rows):
    """rows: (name, r of the kernel, r of the yardstick).  E.check_units on every row -- every figure is printed before anything is raised"""
    bad = []
    for name, r, r_ref in rows:
        try:
            E.check_units(TAG, WIDTH, margin, f"{case} {name}", r, r_ref)
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


def units_err(got, ref, unit, keep=None):
    """max |got - ref| / (2^-24 (unit + FLOOR)) in float64; NaN / inf anywhere in `got` -> inf"""
    got, ref, unit = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, unit))
    assert got.shape == ref.shape == unit.shape, (got.shape, ref.shape, unit.shape)
    r = (got - ref).abs() / (U * (unit + FLOOR))
    if keep is not None:
        r = r[keep]
    if not bool(torch.isfinite(r).all()):
        return math.inf
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------ attention backward
SMALL_CASE = ((2, 4, 4, 1, 16, 0), True)          # 2 groups < RP_CHUNKS = 64 (most chunks of the table kernel are empty), T = 16 << the 64-thread launch width
ATTN_CASES = R.ATTN_VALU_CASES + R.ATTN_MFMA_CASES + [SMALL_CASE]
ATTN_INPUT_KINDS = ("hard", "randn")
DO_KINDS = ("noise", "ones", "impulse", "head-scaled")
ATTN_QUANTITIES = ("dq", "dk", "dv", "drh", "drw")


def attn_case_id(case):
    cfg, rel = case
    return "x".join(map(str, cfg)) + ("" if rel else "-notables")


def attn_case_inputs(cfg, rel, kind):
    """hard: _fwd_ref.attn_inputs (logit std 40: peaked rows, the uniform query, identical keys, the three V kinds); randn: the O(1) logits of the old test"""
    if kind == "hard":
        return R.attn_inputs(cfg, rel)
    qkv, rh, rw = R.randn_attn_inputs(cfg)
    return (qkv, rh, rw) if rel else (qkv, None, None)


def attn_dout(cfg, kind):
    """dO [B, H, W, heads, hd].  noise; ones; impulse: one channel of one token per frame (the head changes with the frame), zero elsewhere;
    head-scaled: noise whose last head is scaled by 1e-4"""
    B, H, W, heads, hd, win = cfg
    g = torch.Generator().manual_seed(7)
    do = torch.randn(B, H, W, heads, hd, generator=g)
    if kind == "noise":
        return do
    if kind == "ones":
        return torch.ones_like(do)
    if kind == "impulse":
        do.zero_()
        for b in range(B):
            do[b, 1, 2, b % heads, 3] = 1.0
        return do
    if kind == "head-scaled":
        do[:, :, :, heads - 1] *= 1e-4
        return do
    raise ValueError(kind)


def _part(t, cfg, C):
    B, H, W, heads, hd, win = cfg
    if win:
        t = t.view(B, H // win, win, W // win, win, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, win, win, C)
    return t


def grouped_qkv(x, cfg):
    """[B, H, W, 3 D] (qkv or its gradient) -> (q, k, v), each [groups, T, hd]; group = (frame, window, head), the head fastest"""
    B, H, W, heads, hd, win = cfg
    D = heads * hd
    Th, Tw = (win, win) if win else (H, W)
    x = _part(x.reshape(B, H, W, 3 * D), cfg, 3 * D)
    Bw = x.shape[0]
    return x.reshape(Bw, Th * Tw, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, Bw * heads, Th * Tw, hd).unbind(0)


def grouped_o(x, cfg):
    """[B, H, W, heads, hd] (out or its gradient) -> [groups, T, hd]"""
    B, H, W, heads, hd, win = cfg
    D = heads * hd
    Th, Tw = (win, win) if win else (H, W)
    x = _part(x.reshape(B, H, W, D), cfg, D)
    Bw = x.shape[0]
    return x.reshape(Bw, Th * Tw, heads, hd).permute(0, 2, 1, 3).reshape(Bw * heads, Th * Tw, hd)


def as_quantities(dqkv, drh, drw, cfg):
    """{dq, dk, dv (grouped), drh, drw} of a gradient in qkv's layout and the two table gradients (or None)"""
    dq, dk, dv = grouped_qkv(dqkv, cfg)
    res = dict(dq=dq, dk=dk, dv=dv)
    if drh is not None:
        res.update(drh=drh, drw=drw)
    return res


def attn_autograd(qkv, rh, rw, cfg, do, dt):
    """autograd of _fwd_ref.attention in `dt`: as_quantities of (d qkv, d rel_h, d rel_w)"""
    def run():
        c = lambda t: None if t is None else t.to(dt).clone().requires_grad_(True)          # noqa: E731
        q, a, b = c(qkv), c(rh), c(rw)
        R.attention(q, a, b, cfg).backward(do.to(dt))
        return as_quantities(q.grad, None if a is None else a.grad, None if b is None else b.grad, cfg)
    return run() if dt == F64 else E.one_thread(run)


def _rel_index(Th, Tw):
    ih = torch.arange(Th)[:, None] - torch.arange(Th)[None, :] + Th - 1          # [query row yi][key row yj] -> table row yi - yj + Th - 1
    iw = torch.arange(Tw)[:, None] - torch.arange(Tw)[None, :] + Tw - 1
    return ih, iw


def _scores(q, k, rh, rw, Th, Tw, hd):
    G, T = q.shape[:2]
    s = (q * hd ** -0.5) @ k.transpose(-2, -1)
    if rh is not None:
        ih, iw = _rel_index(Th, Tw)
        rq = q.reshape(G, Th, Tw, hd)
        s = (s.view(G, Th, Tw, Th, Tw) + torch.einsum("bhwc,hkc->bhwk", rq, rh[ih])[:, :, :, :, None]
             + torch.einsum("bhwc,wkc->bhwk", rq, rw[iw])[:, :, :, None, :]).view(G, T, T)
    return s


def attn_units(qkv, rh, rw, cfg, do):
    """the a-priori units in float64, P the float64 softmax (+ FLOOR is added by units_err):
        u[i][j] = P[i][j] (sum_c |dO_ic||v_jc| + sum_c |dO_ic||O_ic|)               the magnitude of the terms of dS[i][j]
        dq_i    = scale sum_j u[i][j] |k_j| + sum_yj uh[i][yj] |Rh[..]| + sum_xj uw[i][xj] |Rw[..]|      (uh, uw: row / column sums of u, as gh, gw are of dS)
        dk_j    = scale sum_i u[i][j] |q_i|,    dv_j = sum_i P[i][j] |dO_i|
        dRh[r]  = sum over groups, i, yj with yi - yj + Th - 1 = r of uh[i][yj] |q_i|,   dRw likewise"""
    B, H, W, heads, hd, win = cfg
    Th, Tw = (win, win) if win else (H, W)
    T = Th * Tw
    c = lambda t: None if t is None else t.double()          # noqa: E731
    q, k, v = grouped_qkv(qkv.double(), cfg)
    g = grouped_o(do.double(), cfg)
    G = q.shape[0]
    sc = hd ** -0.5
    p = _scores(q, k, c(rh), c(rw), Th, Tw, hd).softmax(-1)
    o = p @ v
    u = p * (g.abs() @ v.abs().transpose(-2, -1) + (g.abs() * o.abs()).sum(-1, keepdim=True))
    units = dict(dq=sc * (u @ k.abs()), dk=sc * (u.transpose(-2, -1) @ q.abs()), dv=p.transpose(-2, -1) @ g.abs())
    if rh is not None:
        ih, iw = _rel_index(Th, Tw)
        u5 = u.view(G, Th, Tw, Th, Tw)
        uh, uw = u5.sum(4), u5.sum(3)
        rq = q.reshape(G, Th, Tw, hd).abs()
        units["dq"] = units["dq"] + (torch.einsum("bhwk,hkc->bhwc", uh, rh.double().abs()[ih])
                                     + torch.einsum("bhwk,wkc->bhwc", uw, rw.double().abs()[iw])).reshape(G, T, hd)
        urh, urw = torch.zeros(2 * Th - 1, hd, dtype=F64), torch.zeros(2 * Tw - 1, hd, dtype=F64)
        urh.index_add_(0, ih.reshape(-1), torch.einsum("bhwk,bhwc->hkc", uh, rq).reshape(-1, hd))
        urw.index_add_(0, iw.reshape(-1), torch.einsum("bhwk,bhwc->wkc", uw, rq).reshape(-1, hd))
        units.update(drh=urh, drw=urw)
    return units


ATTN_DEFECTS = ("no-D", "dk-no-scale", "dq-last-key", "gw-first-row", "mirrored-index", "table-groups-of-4", "no-max", "kind1-dq-zero")


def attn_model(qkv, rh, rw, cfg, do, dt=F32, defect=None):
    """the kernel's formulas (csrc/bwd_vit.hip's header comment) in torch arithmetic of `dt`: P recomputed from qkv, D_i = sum_j P[i][j] (dO_i . v_j)
    from that P, dS = P (dO V^T - D).  DEFECTS for the teeth test:
        no-D              dS without the D term                              dk-no-scale        dk = dS^T q (not scale dS^T q)
        dq-last-key       the last key of the group left out of dq           gw-first-row       gw taken from the first key row only (not summed over yj)
        mirrored-index    table row k - yi + Th - 1 where the tables are applied to dq and where their gradients are gathered
        table-groups-of-4 the table gradients drop the groups past the last multiple of four
        no-max            softmax without the maximum subtracted            kind1-dq-zero      dq of every head whose V has kind 1 (1e-4) is zero"""
    assert defect is None or defect in ATTN_DEFECTS, defect
    B, H, W, heads, hd, win = cfg
    Th, Tw = (win, win) if win else (H, W)
    T = Th * Tw
    c = lambda t: None if t is None else t.to(dt)          # noqa: E731
    rh, rw = c(rh), c(rw)
    q, k, v = grouped_qkv(qkv.to(dt), cfg)
    g = grouped_o(do.to(dt), cfg)
    G = q.shape[0]
    sc = hd ** -0.5
    s = _scores(q, k, rh, rw, Th, Tw, hd)
    e = s.exp() if defect == "no-max" else (s - s.amax(-1, keepdim=True)).exp()
    p = e / e.sum(-1, keepdim=True)
    dp = g @ v.transpose(-2, -1)
    Dq = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - (0 if defect == "no-D" else Dq))
    dsq = ds
    if defect == "dq-last-key":
        dsq = ds.clone()
        dsq[:, :, T - 1] = 0
    res = dict(dq=sc * (dsq @ k), dk=(1.0 if defect == "dk-no-scale" else sc) * (ds.transpose(-2, -1) @ q), dv=p.transpose(-2, -1) @ g)
    if rh is not None:
        ih, iw = _rel_index(Th, Tw)
        if defect == "mirrored-index":
            ih, iw = ih.t(), iw.t()
        ds5 = dsq.view(G, Th, Tw, Th, Tw)
        gh = ds5.sum(4)
        gw = ds5[:, :, :, 0, :] if defect == "gw-first-row" else ds5.sum(3)
        rq = q.reshape(G, Th, Tw, hd)
        res["dq"] = res["dq"] + (torch.einsum("bhwk,hkc->bhwc", gh, rh[ih]) + torch.einsum("bhwk,wkc->bhwc", gw, rw[iw])).reshape(G, T, hd)
        ds5 = ds.view(G, Th, Tw, Th, Tw)          # (the table gradients see every key)
        gh, gw = ds5.sum(4), ds5[:, :, :, 0, :] if defect == "gw-first-row" else ds5.sum(3)
        n = G // 4 * 4 if defect == "table-groups-of-4" else G
        drh, drw = torch.zeros(2 * Th - 1, hd, dtype=dt), torch.zeros(2 * Tw - 1, hd, dtype=dt)
        drh.index_add_(0, ih.reshape(-1), torch.einsum("bhwk,bhwc->hkc", gh[:n], rq[:n]).reshape(-1, hd))
        drw.index_add_(0, iw.reshape(-1), torch.einsum("bhwk,bhwc->wkc", gw[:n], rq[:n]).reshape(-1, hd))
        res.update(drh=drh, drw=drw)
    if defect == "kind1-dq-zero":
        res["dq"] = res["dq"].clone()
        res["dq"][kind1_groups(cfg, G)] = 0
    return res


def kind1_groups(cfg, G):
    heads = cfg[3]
    return [gi for gi in range(G) if R._vkind(gi % heads, heads) == 1]


@functools.lru_cache(maxsize=None)
def attn_reference(case, in_kind, do_kind):
    """(inputs (qkv, rh, rw), dO, float64 reference, units, yardstick's r per line) of one (case, input kind, dO kind): computed once, never modified"""
    cfg, rel = case
    qkv, rh, rw = attn_case_inputs(cfg, rel, in_kind)
    do = attn_dout(cfg, do_kind)
    ref, units = attn_autograd(qkv, rh, rw, cfg, do, F64), attn_units(qkv, rh, rw, cfg, do)
    yard = attn_r(attn_autograd(qkv, rh, rw, cfg, do, F32), ref, units, cfg[3])
    return (qkv, rh, rw), do, ref, units, yard


def attn_r(got, ref, units, heads):
    """{line: r}: the maximum per quantity, and per head for dq and dk (the V kinds differ by head)"""
    r = {n: units_err(got[n], ref[n], units[n]) for n in ATTN_QUANTITIES if n in ref}
    if heads > 1:
        for n in ("dq", "dk"):
            for h in range(heads):
                r[f"{n}/head{h}"] = units_err(got[n][h::heads], ref[n][h::heads], units[n][h::heads])
    return r


def old_criterion_accepts(got, ref):
    """the bound of tests/test_gpu_bwd.py::test_vit_attention_bwd on the whole of dqkv: max |got - ref| <= 2e-4 max |ref|"""
    cat = lambda d: torch.cat([d[n].double().reshape(-1) for n in ("dq", "dk", "dv")])          # noqa: E731
    return bool((cat(got) - cat(ref)).abs().max() <= 2e-4 * cat(ref).abs().max())


# ------------------------------------------------------------------------------------------------------------------------ GELU' and the other derivatives
GELU_ROWS, GELU_C, GELU_LD = 84, 50, 56          # 4200 values: C % 4 != 0, ld > 4 ceil(C / 4); 84 rows = 28 frames of HW = 3
CLAMP = 5.65685424949238                          # vs_erfc_sqrt2's clamp (sqrt 32)
CROSSING = -0.7518                                # gelu' changes sign next to it
SUBNORMAL = 2.0 ** -149
TAIL = (-5.6, -1.0)                               # line (b); beyond the clamp the kernel's Phi is stuck at 7.9e-9, which is within (a)
SCALED_ROW = 1


def _neighbours(v):
    t = torch.tensor([v], dtype=F32)
    return [t, torch.nextafter(t, torch.tensor([-math.inf])), torch.nextafter(t, torch.tensor([math.inf]))]


def gelu_special_points():
    pts = [torch.tensor([0.0, -0.0, SUBNORMAL, -SUBNORMAL, 1e-8, -1e-8, 13.5, -13.5, 100.0, -100.0, 4e3, -4e3], dtype=F32)]
    pts += _neighbours(CLAMP) + _neighbours(-CLAMP) + _neighbours(CROSSING)
    return torch.cat(pts)


def gelu_sweep():
    """z [GELU_ROWS][GELU_C]: [-9, 9] densely (4179 points, step 4.3e-3), then +-0.0, +- the smallest subnormal, +-1e-8, +-13.5, +-100, +-4e3 and the
    floats on either side of +-5.65685424949238 and of -0.7518"""
    sp = gelu_special_points()
    n = GELU_ROWS * GELU_C - sp.numel()
    assert n >= 4096
    return torch.cat([torch.linspace(-9, 9, n, dtype=F64).to(F32), sp]).view(GELU_ROWS, GELU_C)


def gelu_dy(rows=GELU_ROWS):
    """noise [rows][GELU_C], row SCALED_ROW scaled by 1e-4"""
    dy = torch.randn(rows, GELU_C, generator=torch.Generator().manual_seed(2100 + rows))
    dy[SCALED_ROW] *= 1e-4
    return dy


def Phi(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2))


def phi(z):
    return torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def act_grad64(z, act):
    """the derivative of the activation in float64 from the fp32 values z; act: "gelu", "silu", "tanh", "relu" """
    z = z.double()
    if act == "gelu":
        return Phi(z) + z * phi(z)
    if act == "silu":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if act == "tanh":
        return 1 - torch.tanh(z) ** 2
    if act == "relu":
        return (z > 0).double()
    raise ValueError(act)


ACT_FN = {"gelu": F.gelu, "silu": F.silu, "tanh": torch.tanh, "relu": F.relu}


def act_yardstick(z, dy, act):
    """ATen's fp32 autograd of the activation: dy act'(z)"""
    def run():
        zz = z.clone().requires_grad_(True)
        ACT_FN[act](zz).backward(dy)
        return zz.grad
    return E.one_thread(run)


def act_lines(name, got, z, dy, act, yard=None):
    """[(line, r of `got`, r of ATen's fp32 autograd)]: (a) |got - ref| / (2^-24 |dy|) over every element; for GELU also (b) on z in TAIL
    |got - ref| / (2^-24 |dy| (Phi + |z| phi)).  dy: the upstream value of every element ([rows][C], what multiplies act'(z)); yard: ATen's fp32
    result where it is not simply act_yardstick(z, dy, act)"""
    d = act_grad64(z, act)
    ref = dy.double() * d
    yard = act_yardstick(z, dy, act) if yard is None else yard
    rows = [(f"{name} (a)", units_err(got, ref, dy.double().abs()), units_err(yard, ref, dy.double().abs()))]
    if act == "gelu":
        zd = z.double()
        keep = (zd >= TAIL[0]) & (zd <= TAIL[1])
        unit = dy.double().abs() * (Phi(zd) + zd.abs() * phi(zd))
        rows.append((f"{name} (b) tail", units_err(got, ref, unit, keep), units_err(yard, ref, unit, keep)))
    return rows


_ERFC_COEFFS = (5.128553084e-07, -9.560153558e-06, 7.497344632e-05, -2.843466646e-04, 1.498938855e-05, 6.931120995e-03, -5.243476480e-02, -4.592214525e-01,
                -1.151104212e+00)
GELU_DEFECTS = ("no-zphi-beyond-4", "clamp-at-4", "branches-swapped")


def gelu_grad_fit(z, defect=None):
    """vs_gelu_grad in fp32 torch arithmetic (no fused multiply-add, torch's exp in place of the hardware's): the CPU stand-in of the kernel.  DEFECTS:
    no-zphi-beyond-4 = the z phi(z) term dropped for |z| > 4; clamp-at-4 = the clamp of the fit's argument moved from 5.657 to 4;
    branches-swapped = Phi = 1 - erfc / 2 taken for negative z and erfc / 2 for the others"""
    assert defect is None or defect in GELU_DEFECTS, defect
    z = z.to(F32)
    u = z.abs().clamp(max=4.0 if defect == "clamp-at-4" else CLAMP)
    q = torch.full_like(u, _ERFC_COEFFS[0])
    for co in _ERFC_COEFFS[1:]:
        q = q * u + co
    e = torch.exp2(q * u)
    pos = (z < 0) if defect == "branches-swapped" else (z >= 0)
    P = torch.where(pos, 1 - 0.5 * e, 0.5 * e)
    zp = z * (0.3989422804014327 * torch.exp(-0.5 * z * z))
    if defect == "no-zphi-beyond-4":
        zp = torch.where(z.abs() > 4, torch.zeros_like(zp), zp)
    return P + zp


def padded(t, ld, fill=0.0):
    """[rows][C] -> [rows][ld], the pad columns `fill`"""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ------------------------------------------------------------------------------------------------------------------------ depthwise 7 x 7
# (B, H, W, C, ld).  1x1: every tap but the centre is padding; 3x2: W < 3, the window's pre-load stops early; 9x11x6 in ld 8: pad lanes, W = 7 + 4;
# 7x15: W = 2 * 7 + 1 crosses the unrolled walk twice and ends one pixel past it; 33x63x8: B H = 2079 > 2048 -> RB = 2, nband = 32, a one-row last band
DW_SHAPES = [(1, 1, 1, 4, 4), (1, 3, 2, 4, 4), (2, 9, 11, 6, 8), (1, 7, 15, 24, 24), (33, 63, 8, 4, 4)]
DW_DY_KINDS = ("noise", "ones", "checker")
SMALL_CHANNEL, SPARSE_CHANNEL = 0, 3          # weights: channel 0 scaled by 1e-5, channel 3 with every other tap zero


def dw_bands(B, H):
    """(RB, nband) of vs_dwconv7_wgrad: rows per chunk = ceil(B H / 2048)"""
    RB = -(-B * H // 2048)
    return RB, -(-H // RB)


def dw_inputs(B, H, W, C):
    """x [B, C, H, W]: per channel (hard_matrix "cols") mean 30 / std 0.5, channel 1 constant, channel 2 with a 4e3 outlier, channel 3 of magnitude 1e-3;
    w [C, 1, 7, 7] = 0.2 randn with channel 0 scaled by 1e-5 and every other tap of channel 3 zero; bias [C]; add [B, C, H, W] noise"""
    g = torch.Generator().manual_seed(2200 + 7 * B + H + W + C)
    x = E.hard_matrix(B * H * W, C, 2201 + H + W, "cols").view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    w = 0.2 * torch.randn(C, 1, 7, 7, generator=g)
    w[SMALL_CHANNEL] *= 1e-5
    w[SPARSE_CHANNEL].view(-1)[1::2] = 0.0
    return x, w, 0.1 * torch.randn(C, generator=g), torch.randn(B, C, H, W, generator=g)


def dw_dy(B, H, W, C, kind):
    if kind == "noise":
        return torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(2300 + H + W))
    if kind == "ones":
        return torch.ones(B, C, H, W)
    if kind == "checker":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        return (1.0 - 2.0 * ((yy + xx) % 2)).expand(B, C, H, W).contiguous()
    raise ValueError(kind)


def dw_forward(x, w, bias, dt):
    C = x.shape[1]
    return F.conv2d(x.to(dt), w.to(dt), None if bias is None else bias.to(dt), padding=3, groups=C)


def dw_data_grad(dy, w, add, dt):
    """the flipped pass: autograd of the conv w.r.t. its input, + add"""
    x0 = torch.zeros_like(dy, dtype=dt).requires_grad_(True)
    return torch.autograd.grad(dw_forward(x0, w, None, dt), x0, dy.to(dt))[0] + add.to(dt)


def dw_weight_grad(x, dy, dt):
    C = x.shape[1]
    w0 = torch.zeros(C, 1, 7, 7, dtype=dt).requires_grad_(True)
    return torch.autograd.grad(dw_forward(x, w0, None, dt), w0, dy.to(dt))[0]


def dw_refs(fn):
    """(float64 reference, fp32 yardstick on one thread) of fn(dtype)"""
    return fn(F64), E.one_thread(lambda: fn(F32))


def dw_units(x, w, bias, add, dy):
    """float64 units: forward sum |w||x| + |bias|; flipped pass sum |w||dy| + |add|; weight gradient per (tap, channel) sum |dy||x|"""
    ax, aw, ad = x.double().abs(), w.double().abs(), dy.double().abs()
    return dict(fwd=dw_forward(ax, aw, bias.abs(), F64), flip=dw_data_grad(ad, aw, add.abs(), F64), wgrad=dw_weight_grad(ax, ad, F64))


DW_DEFECTS = ("centre-row-not-flipped", "band-last-row", "window-slot")


def dw_flip(dy, w, add, defect=None):
    """the flipped pass as the kernel states it, in fp32: a correlation with the taps 48 - t, + add.  DEFECT centre-row-not-flipped: tap row ky = 3 keeps
    its own order"""
    assert defect in (None, "centre-row-not-flipped"), defect
    wf = w.flip(2, 3).clone()
    if defect:
        wf[:, :, 3] = w[:, :, 3]
    return F.conv2d(dy, wf, None, padding=3, groups=dy.shape[1]) + add


def dw_wgrad(x, dy, defect=None):
    """dw[c][ky][kx] = sum_{b,y,x} dy[b,c,y,x] x[b,c,y+ky-3,x+kx-3] in fp32, tap by tap.  DEFECTS: band-last-row = the last row of every band of RB > 1
    image rows (dw_bands) is left out; window-slot = from the second group of seven pixels on (x >= 7) the window is read one slot further"""
    assert defect in (None, "band-last-row", "window-slot"), defect
    B, C, H, W = x.shape
    if defect == "band-last-row":
        RB, _ = dw_bands(B, H)
        if RB > 1:
            dy = dy.clone()
            dy[:, :, RB - 1::RB] = 0
    xp = F.pad(x, (3, 4, 3, 3))
    dw = torch.zeros(C, 1, 7, 7)
    shift = (torch.arange(W) >= 7) if defect == "window-slot" else None
    for ky in range(7):
        for kx in range(7):
            t = xp[:, :, ky:ky + H, kx:kx + W]
            if shift is not None:
                t = torch.where(shift, xp[:, :, ky:ky + H, kx + 1:kx + 1 + W], t)
            dw[:, 0, ky, kx] = (dy * t).sum((0, 2, 3))
    return dw


def nhwc(x, ld):
    """[B, C, H, W] -> the rows [B, H, W, ld] a kernel reads, pad columns zero"""
    Bn, C, H, W = x.shape
    t = torch.zeros(Bn, H, W, ld, dtype=x.dtype)
    t[..., :C] = x.permute(0, 2, 3, 1)
    return t


def taps_first(w, ld):
    """[C, 1, 7, 7] -> [49][ld], pad lanes zero"""
    C = w.shape[0]
    t = torch.zeros(49, ld, dtype=w.dtype)
    t[:, :C] = w.reshape(C, 49).t()
    return t
