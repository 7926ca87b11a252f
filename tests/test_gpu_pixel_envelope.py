"""The pixel-wise head (csrc/pixel_head.hip: vs_pixel_upgather, vs_pixel_upgather_bwd, vs_pixel_linear, vs_pixel_linear_bwd, vs_pixel_vote) and
vs_matmul_small through the C entry points, on the hard inputs and cases of tests/_pixel_ref.py, against float64 -- the fp64-envelope rule of
tests/_envelope.py with PIXEL_MARGIN (profiles/pixel_fp64_envelope.txt is a recording of the lines printed here).

Every operand sits between guard bands (tests/_guards.py): NaN around what a kernel reads, a sentinel around what it writes and around the
partial-sum workspace.  The cases reach every template instantiation behind the entry points (the list in _pixel_ref.LIN_CASES / UP_COS names
them), the 512-workgroup cap of the weight gradient with its empty workgroups, frames whose size is odd, and row strides above the minimum with
NaN in the pad lanes.  tests/test_pixel_contract_cpu.py shows without a GPU that the references are the torch modules' and that seeded defects
fall outside the rule at its cap on these very cases."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _pixel_ref as R  # noqa: E402
from tests._guards import _guarded, _guards_intact, scratch, scratch_sentinel  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = -7.0
ERR_BAD_ARG = -1            # VS_ERR_BAD_ARG (include/videoseal_hip.h)


class Bands:
    """operands between guard bands; `intact()` after the launches"""

    def __init__(self):
        self.bufs = []

    def inp(self, t, ld=None):
        """device copy of a CPU tensor between NaN bands; ld: rows [..., C] widened to [..., ld] with NaN pad lanes"""
        if ld is not None and ld != t.shape[-1]:
            wide = torch.full(t.shape[:-1] + (ld,), NAN, dtype=t.dtype)
            wide[..., : t.shape[-1]] = t
            t = wide
        buf, v = _guarded(t.to(DEV), NAN)
        self.bufs.append((buf, NAN))
        return v

    def out(self, *shape, dtype=torch.float32):
        buf, v = _guarded(torch.full(shape, SENT, device=DEV, dtype=dtype), SENT)
        self.bufs.append((buf, SENT))
        return v

    def scratch(self, nelem, fill):
        buf, v = scratch(nelem, torch.float32, fill, DEV)
        self.bufs.append((buf, scratch_sentinel(torch.float32)))
        return v

    def intact(self):
        torch.cuda.synchronize()
        return all(_guards_intact(b, f) for b, f in self.bufs)


def _untouched(t):
    return bool((t == SENT).all())


# ------------------------------------------------------------------------------------------------------------------------ vs_pixel_linear
def _linear_forward(case, G):
    C, K, H, W, sig, pad = case
    x, w, b = R.lin_inputs(case)
    xd, wd, bd = G.inp(x, C + pad), G.inp(w), G.inp(b)
    out = G.out(R.LIN_B, K, H * W)
    N.check(N.lib().vs_pixel_linear(N.ptr(xd), C + pad, R.LIN_B, H * W, C, N.ptr(wd), N.ptr(bd), K, int(sig), N.ptr(out), N.stream()), "vs_pixel_linear")
    return xd, wd, out


@pytest.mark.parametrize("case", R.LIN_CASES, ids=R.lin_name)
def test_pixel_linear_fp64_envelope(case):
    """vs_pixel_linear: logits in units of 2^-24 P per element (an element whose terms are all zero exactly 0); behind the sigmoid per channel plane"""
    C, K, H, W, sig, pad = case
    G = Bands()
    _, _, out = _linear_forward(case, G)
    assert G.intact()
    r64, r32, P = R.lin_fwd_ref(case)
    got = out.cpu()
    assert torch.isfinite(got).all()
    if sig:
        R.envelope(f"pixel_linear {R.lin_name(case)}", [("y/plane", R.group_err(got, r64, -1), R.group_err(r32, r64, -1))])
    else:
        R.envelope_units(f"pixel_linear {R.lin_name(case)}", R.units(got, r64, P), R.units(r32, r64, P))


def _linear_backward(case, kind, G, fills=(NAN,), want_dx=True, want_dw=True):
    """vs_pixel_linear_bwd once per entry of `fills`, every launch over the SAME partial workspace refilled with that value (what a previous user
    of the memory may have left) -> a list of (dx, dw, db) device views (the sentinel where not asked for)"""
    C, K, H, W, sig, pad = case
    L = N.lib()
    rows = R.LIN_B * H * W
    x, w, b = R.lin_inputs(case)
    y = R.lin_y(case)
    xd, wd, dpd = G.inp(x, C + pad), G.inp(w), G.inp(R.lin_dpreds(case, kind))
    yd = None if y is None else G.inp(y)
    part = G.scratch(int(L.vs_pixel_linear_bwd_partial_floats(rows, K, C)), NAN)
    runs = []
    for fill in fills:
        part.fill_(fill)
        dx, dw, db = G.out(rows, C + pad), G.out(K, C), G.out(K)
        N.check(L.vs_pixel_linear_bwd(N.ptr(dpd), N.ptr(yd), N.ptr(xd) if want_dw else None, C + pad, R.LIN_B, H * W, C, N.ptr(wd), K,
                                      N.ptr(dx) if want_dx else None, C + pad, N.ptr(dw) if want_dw else None, N.ptr(db) if want_dw else None,
                                      N.ptr(part) if want_dw else None, N.stream()), "vs_pixel_linear_bwd")
        runs.append((dx, dw, db))
    return runs


@pytest.mark.parametrize("kind", R.DP_KINDS)
@pytest.mark.parametrize("case", R.LIN_CASES, ids=R.lin_name)
def test_pixel_linear_bwd_fp64_envelope(case, kind):
    """vs_pixel_linear_bwd: dx, dw and db in units of 2^-24 P per element, for gradients of one sign and for cancelling ones; twice over the same
    partial workspace, filled with NaN and then with 0: bit-identical (a workgroup without rows writes zero partials); pad lanes of dx untouched"""
    C, K, H, W, sig, pad = case
    G = Bands()
    first, second = _linear_backward(case, kind, G, (NAN, 0.0))
    assert G.intact()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "the result depends on what the partial workspace held"
    dx, dw, db = (t.cpu() for t in first)
    assert _untouched(dx[:, C:])
    (x64, w64, b64), (x32, w32, b32), (Px, Pw, Pb) = R.lin_bwd_ref(case, kind)
    nx, nw, nb = R.lin_bwd_terms(case)
    figures = [("dx", dx[:, :C], x64, x32, Px, nx), ("dw", dw, w64, w32, Pw, nw), ("db", db, b64, b32, Pb, nb)]
    bad = []
    for name, got, r64, r32, P, n in figures:              # every figure is printed before anything is asserted
        try:
            R.envelope_units(f"pixel_linear_bwd {R.lin_name(case)} {kind} {name}", R.units(got, r64, P, n), R.units(r32, r64, P, n))
        except AssertionError as e:
            bad.append(e)
    assert not bad, bad


def test_pixel_linear_bwd_plan_at_the_workgroup_cap():
    """the case that stands for the 512-workgroup cap really is at it: 132098 rows, 288 rows per workgroup, workgroups 459..511 without rows --
    derived from vs_pixel_linear_bwd_partial_floats and the rule in the kernel's header, so that a changed rule fails here instead of silently
    missing the edge"""
    C, K, H, W, sig, pad = R.LIN_CAP
    rows = R.LIN_B * H * W
    assert rows == 132098 and (H * W) % 2 == 1
    floats = int(N.lib().vs_pixel_linear_bwd_partial_floats(rows, K, C))
    assert floats == R.lin_partial_floats(rows, K, C)
    assert R.lin_plan(rows, floats, K, C) == (512, 288, 459)
    for case in R.LIN_CASES:                                # and no other case is: their workgroups all have rows
        c, k, h, w = case[:4]
        r = R.LIN_B * h * w
        nb, rpb, first_empty = R.lin_plan(r, int(N.lib().vs_pixel_linear_bwd_partial_floats(r, k, c)), k, c)
        assert (first_empty < nb) == (case == R.LIN_CAP), (case, nb, rpb, first_empty)


@pytest.mark.parametrize("case", [R.LIN_CASES[1], R.LIN_CASES[8]], ids=R.lin_name)
def test_pixel_linear_bwd_dx_only_and_dw_only(case):
    """dx alone (no x, no workspace) and dw / db alone give the bits of the full call and leave what they were not asked for untouched"""
    G = Bands()
    (full,) = _linear_backward(case, "cancelling", G)
    (only_x,) = _linear_backward(case, "cancelling", G, want_dw=False)
    (only_w,) = _linear_backward(case, "cancelling", G, want_dx=False)
    assert G.intact()
    assert torch.equal(only_x[0], full[0]) and _untouched(only_x[1]) and _untouched(only_x[2])
    assert _untouched(only_w[0]) and torch.equal(only_w[1], full[1]) and torch.equal(only_w[2], full[2])


def test_pixel_linear_refusals_launch_nothing():
    """C % 4 != 0, C > 64, a weight gradient with K (C / 4 + 1) > 5120 outputs: unsupported; x, w or out 4 bytes off a 16-byte boundary: a bad
    argument.  After each refusal every output still holds its sentinel"""
    L, st = N.lib(), N.stream()
    G = Bands()
    HW, K = 16, 4
    # sized for the largest shape asked for below, so that a launch that should have been refused would still stay inside its operands
    big, dp = G.inp(torch.zeros(2 * HW * 72 + 8)), G.inp(torch.zeros(2 * 320 * HW))
    wbig = G.inp(torch.zeros(320 * 72 + 8))
    out, dx, dw, db = G.out(2, 320, HW + 1), G.out(2 * HW, 72), G.out(320, 72), G.out(320)
    part = G.scratch(int(L.vs_pixel_linear_bwd_partial_floats(2 * HW, 320, 64)), NAN)
    p = N.ptr

    def refused(code, want, what):
        """the call answered `want` and launched nothing: after it every output still holds its sentinel and the workspace its NaN"""
        assert code == want, (what, code)
        assert G.intact() and all(_untouched(t) for t in (out, dx, dw, db)) and bool(torch.isnan(part).all()), what

    for C, ld in ((6, 8), (68, 68), (72, 72)):
        refused(L.vs_pixel_linear(p(big), ld, 2, HW, C, p(wbig), None, K, 0, p(out), st), N.ERR_UNSUPPORTED, ("forward", C))
        refused(L.vs_pixel_linear_bwd(p(dp), None, p(big), ld, 2, HW, C, p(wbig), K, p(dx), ld, p(dw), p(db), p(part), st), N.ERR_UNSUPPORTED,
                ("backward", C))
    # K = 320, C = 64: 5440 outputs for at most 256 threads x 20
    refused(L.vs_pixel_linear_bwd(p(dp), None, p(big), 64, 2, HW, 64, p(wbig), 320, p(dx), 64, p(dw), p(db), p(part), st), N.ERR_UNSUPPORTED, "nout")
    # one float into a larger allocation: 4 bytes off
    x1, w1, o1, dx1, p1 = big[1:], wbig[1:], out.view(-1)[1:], dx.view(-1)[1:], part[1:]
    assert p(x1) % 16 == 4 and p(w1) % 16 == 4 and p(o1) % 16 == 4 and p(big) % 16 == 0 and p(wbig) % 16 == 0 and p(out) % 16 == 0
    C = 8
    for i, (xa, wa, oa) in enumerate(((x1, wbig, out), (big, w1, out), (big, wbig, o1))):
        refused(L.vs_pixel_linear(p(xa), C, 2, HW, C, p(wa), None, K, 0, p(oa), st), ERR_BAD_ARG, ("forward off by 4 bytes", i))
    for i, (xa, wa, dxa, pa) in enumerate(((x1, wbig, dx, part), (big, w1, dx, part), (big, wbig, dx1, part), (big, wbig, dx, p1))):
        refused(L.vs_pixel_linear_bwd(p(dp), None, p(xa), C, 2, HW, C, p(wa), K, p(dxa), C, p(dw), p(db), p(pa), st), ERR_BAD_ARG,
                ("backward off by 4 bytes", i))


# ------------------------------------------------------------------------------------------------------------------------ vs_pixel_upgather
def _upgather(case, G, z, lw, lb, act):
    Co, f, H, W, pad = case
    zd = G.inp(z, 9 * Co + pad)
    lwd, lbd = (None, None) if lw is None else (G.inp(lw), G.inp(lb))
    out = G.out(R.UP_B, f * H, f * W, Co + pad)
    N.check(N.lib().vs_pixel_upgather(N.ptr(zd), 9 * Co + pad, R.UP_B, H, W, Co, f, N.ptr(lwd), N.ptr(lbd), R.LN_EPS, act, N.ptr(out), Co + pad,
                                      N.stream()), "vs_pixel_upgather")
    return out


@pytest.mark.parametrize("case", R.UP_CASES, ids=R.up_name)
def test_pixel_upgather_fp64_envelope(case):
    """vs_pixel_upgather: the raw mode in units of 2^-24 P per element (the zero channel exactly 0); LayerNorm + GELU per pixel, the hard frame and
    the constant frame (variance exactly 0) each against its own yardstick; pad lanes of the output untouched"""
    Co, f, H, W, pad = case
    assert N.lib().vs_pixel_upgather_supported(Co, f) == 1
    z, lw, lb, _ = R.up_inputs(case)
    G = Bands()
    raw = _upgather(case, G, z, None, None, 0)
    out = _upgather(case, G, z, lw, lb, N.ACT_GELU)
    assert G.intact()
    raw, out = raw.cpu(), out.cpu()
    assert _untouched(raw[..., Co:]) and _untouched(out[..., Co:])
    assert torch.isfinite(raw[..., :Co]).all() and torch.isfinite(out[..., :Co]).all()
    ref = R.up_ref(case)
    r64, r32, P = ref["raw"]
    o64, o32 = ref["out"]
    bad = []
    try:
        R.envelope_units(f"pixel_upgather raw {R.up_name(case)}", R.units(raw[..., :Co], r64, P), R.units(r32, r64, P))
    except AssertionError as e:
        bad.append(e)
    try:
        R.envelope(f"pixel_upgather ln+gelu {R.up_name(case)}", R.up_class_rows("px", out[..., :Co], o64, o32))
    except AssertionError as e:
        bad.append(e)
    assert not bad, bad


@pytest.mark.parametrize("case", R.UP_CASES, ids=R.up_name)
def test_pixel_upgather_bwd_fp64_envelope(case):
    """vs_pixel_upgather_bwd against the float64 adjoint built from the forward's own float64 matrix, in units of 2^-24 P per element; columns of
    dz beyond 9 Co untouched"""
    Co, f, H, W, pad = case
    _, _, _, dg = R.up_inputs(case)
    G = Bands()
    dgd = G.inp(dg, Co + pad)
    dz = G.out(R.UP_B, H, W, 9 * Co + pad)
    N.check(N.lib().vs_pixel_upgather_bwd(N.ptr(dgd), Co + pad, R.UP_B, H, W, Co, f, N.ptr(dz), 9 * Co + pad, N.stream()), "vs_pixel_upgather_bwd")
    assert G.intact()
    dz = dz.cpu()
    assert _untouched(dz[..., 9 * Co:])
    a64, a32, P = R.up_ref(case)["adj"]
    R.envelope_units(f"pixel_upgather_bwd {R.up_name(case)}", R.units(dz[..., : 9 * Co], a64, P), R.units(a32, a64, P))


# ------------------------------------------------------------------------------------------------------------------------ vs_matmul_small
@pytest.mark.parametrize("case", R.MM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_matmul_small_fp64_envelope(case):
    """vs_matmul_small with lda, ldb and ldc above the minimum: NaN in the gaps of A and B, the sentinel still in the gaps of C"""
    M, Nn, K = case
    pa, pb, pc = R.MM_PAD
    A, Bm = R.mm_inputs(case)
    G = Bands()
    Ad, Bd = G.inp(A, K + pa), G.inp(Bm, Nn + pb)
    Cd = G.out(M, Nn + pc)
    N.check(N.lib().vs_matmul_small(N.ptr(Ad), K + pa, N.ptr(Bd), Nn + pb, M, Nn, K, N.ptr(Cd), Nn + pc, N.stream()), "vs_matmul_small")
    assert G.intact()
    got = Cd.cpu()
    assert _untouched(got[:, Nn:])
    r64, r32, P = R.mm_ref(case)
    R.envelope_units(f"matmul_small M={M} N={Nn} K={K}", R.units(got[:, :Nn], r64, P), R.units(r32, r64, P))


# ------------------------------------------------------------------------------------------------------------------------ vs_pixel_vote
@pytest.mark.parametrize("thr", R.VOTE_THRESHOLDS)
@pytest.mark.parametrize("shape", R.VOTE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_pixel_vote_counts_bit_for_bit(shape, thr):
    """vs_pixel_vote: whole-number counts equal to torch's on the same values -- logits exactly at the threshold (no vote), one ulp either side,
    +-0.0; masks 0.0 and -0.0 (not selected), a fraction and a denormal (selected) -- with and without a mask, frames a wider stride apart"""
    B, K, HW = shape
    logits, masks = R.vote_inputs(B, K, HW, thr)
    stride = K * HW + 5
    for m in (masks, None):
        G = Bands()
        ld = G.inp(logits.reshape(B, K * HW), stride)
        md = None if m is None else G.inp(m)
        votes, nsel = G.out(B, K, dtype=torch.int32), G.out(B, dtype=torch.int32)
        N.check(N.lib().vs_pixel_vote(N.ptr(ld), stride, N.ptr(md), B, K, HW, thr, N.ptr(votes), N.ptr(nsel), N.stream()), "vs_pixel_vote")
        assert G.intact()
        want_v, want_n = R.vote_ref(logits, m, thr)
        print(f"PIXEL-VOTE {shape} thr {thr} mask {m is not None}: votes {votes.cpu().flatten().tolist()} nsel {nsel.cpu().tolist()}")
        assert torch.equal(votes.cpu().long(), want_v) and torch.equal(nsel.cpu().long(), want_n)
