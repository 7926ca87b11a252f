"""The pixel-wise extractor head on the HIP path (csrc/pixel_head.hip, videoseal_amd/pixel_head.py, the 4-D dispatch of metrics.bit_accuracy /
bit_accuracy_1msg) against the float64 run of the unmodified reference (tests/golden/pixel_head_ops.npz, tests/golden/make_golden_pixel_head.py).

Tolerance.  The yardstick is the reference, not the code under test: per tensor the fixture holds what the reference's OWN fp32 run loses
against its float64 run (`e`, largest absolute difference).  The HIP result, compared with the same float64 values, gets 4 x that figure -- a
different but equally valid fp32 evaluation (low-resolution products, other summation orders) -- with an absolute floor of 1e-6 where `e` is
below it.  The gather's adjoint is also checked without any reference by <A x, y> = <x, A^T y> in double on the host, to 1e-5 relative.

The stage tests run the per-tap GEMM (vs_conv_gemm, not part of this head) on the engine's exact 3 x bf16 split and on the fp32-input MFMA path:
both multiply fp32 operands exactly, so the error measured is the new kernels'.  The model-level tests run the default arithmetic.

With VS_PIXEL_HEAD_PARITY_OUT=<file> the measured errors of every case are written there (profiles/pixel_head_parity.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _pixel_head_util as U
from tests._util import load_golden
from tests._gpu import Eng, from_nhwc, to_nhwc
from tests._guards import _guarded, _guards_intact
from videoseal_amd import metrics as M
from videoseal_amd import native as N
from videoseal_amd import pixel_head as PH
from videoseal_amd.engine import Act

pytestmark = pytest.mark.gpu

G = load_golden("pixel_head_ops")
E = G["meta"]["e"]
MEASURED = {}


def _record(key, err, bound):
    MEASURED[key] = dict(err=float(err), e_ref=float(E.get(key.split("@")[0], float("nan"))), bound=float(bound))
    path = os.environ.get("VS_PIXEL_HEAD_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _check_inputs(key, *tensors):
    want = np.array(G["meta"]["sums"][key])
    got = U.checksum(*tensors)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9), f"{key}: the seeded inputs differ from the ones the fixture was made with"


def _against(key, t, note=""):
    """largest |t - float64 reference| over the stored (sub-)sample, asserted against max(4 e_ref, 1e-6)"""
    want, stats = G[key], G[key + ".stats"]
    flat = t.detach().double().cpu().flatten()
    assert flat.numel() == int(stats[2]), f"{key}: {flat.numel()} elements, fixture has {int(stats[2])}"
    err = float((flat[::int(stats[3])] - torch.from_numpy(want)).abs().max())
    bound = max(4 * E[key], 1e-6)
    print(f"{key}{note}: max |hip - float64| = {err:.3e} (reference fp32: {E[key]:.3e}, bound {bound:.3e})")
    _record(key + note, err, bound)
    assert torch.isfinite(flat).all() and err <= bound, f"{key}{note}: {err:.3e} > {bound:.3e}"
    return err


@pytest.fixture(scope="module", params=["bf16x3", "f32"])
def eng(request):
    return Eng(use_split=(request.param != "f32"), arith=3)


def _nchw(a: Act):
    return from_nhwc(a)


STAGE_CASES = [(C, Co, f, H, W) for (C, Co, f) in U.STAGES for (H, W) in U.LATENTS]


@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda c: U.stage_name(*c))
def test_upsample_stage_forward(eng, case):
    """z = v W on the low-resolution rows (vs_conv_gemm), then vs_pixel_upgather: fused LayerNorm + GELU, and the raw mode of the training forward"""
    C, Co, f, H, W = case
    key = U.stage_name(*case)
    x, w, lw, lb, dout = U.stage_tensors(*case)
    _check_inputs(key, x, w, lw, lb, dout)
    assert eng.lib.vs_pixel_upgather_supported(Co, f) == 1
    xa = to_nhwc(x)
    wz = PH.pack_stage(w.cuda(), xa.ld)
    lwd, lbd = lw.cuda(), lb.cuda()
    note = "@" + ("split" if eng.use_split else "f32")
    out = PH.stage_forward(eng, xa, wz, lwd, lbd, f, "t.ps")
    _against(key + ".out", _nchw(out), note)
    out2, raw, ln = PH.stage_forward(eng, xa, wz, lwd, lbd, f, "t.ps2", keep_raw=True)
    _against(key + ".raw", _nchw(raw), note + ".raw_mode")
    _against(key + ".out", _nchw(out2), note + ".raw_mode")


@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda c: U.stage_name(*c))
def test_gather_adjoint_inner_product(case):
    """<A z, y> = <z, A^T y> for the raw gather A and vs_pixel_upgather_bwd, sums in double on the host, 1e-5 relative to the inner product itself.
    z is seeded; y = seeded noise + 2 A z, so that the inner product is a sum of mostly positive terms: with two independent random vectors it is
    the small remainder of a cancellation and its fp32 rounding noise can exceed 1e-5 of it by chance (seen at 96 -> 24 channels, x2, in a host
    build of the same kernels), which would say nothing about the adjoint."""
    C, Co, f, H, W = case
    g = torch.Generator().manual_seed(1000 + Co + 7 * f + 31 * H + W)
    z = torch.randn(U.B, H, W, 9 * Co, generator=g).cuda()
    noise = torch.randn(U.B, f * H, f * W, Co, generator=g).cuda()
    Az, Aty = torch.empty_like(noise), torch.empty_like(z)
    L = N.lib()
    N.check(L.vs_pixel_upgather(N.ptr(z), 9 * Co, U.B, H, W, Co, f, None, None, 1e-6, 0, N.ptr(Az), Co, N.stream()), "vs_pixel_upgather")
    y = (noise + 2.0 * Az).contiguous()
    N.check(L.vs_pixel_upgather_bwd(N.ptr(y), Co, U.B, H, W, Co, f, N.ptr(Aty), 9 * Co, N.stream()), "vs_pixel_upgather_bwd")
    lhs = float((Az.double().cpu() * y.double().cpu()).sum())
    rhs = float((z.double().cpu() * Aty.double().cpu()).sum())
    rel = abs(lhs - rhs) / min(abs(lhs), abs(rhs))
    print(f"{U.stage_name(*case)}: <Az, y> = {lhs:.9e}, <z, A^T y> = {rhs:.9e}, relative difference {rel:.2e}")
    assert lhs > 0 and rel <= 1e-5


def test_upsample_stage_gradients(eng):
    """input and parameter gradients of one stage (GELU, LayerNorm, the gather's adjoint, dz -> dv GEMM, vs_gemm_wgrad) against float64 autograd"""
    case = U.BWD_STAGE
    C, Co, f, H, W = case
    key = U.stage_name(*case)
    x, w, lw, lb, dout = U.stage_tensors(*case)
    xa = to_nhwc(x)
    wd, lwd, lbd = w.cuda(), lw.cuda(), lb.cuda()
    out, raw, ln = PH.stage_forward(eng, xa, PH.pack_stage(wd, xa.ld), lwd, lbd, f, "t.pg", keep_raw=True)
    dx, Gd = PH.stage_backward(eng, xa, wd, lwd, raw, ln, to_nhwc(dout), f, "t.pgb")
    note = "@" + ("split" if eng.use_split else "f32")
    _against(key + ".dx", _nchw(dx), note)
    _against(key + ".dw", Gd["conv"], note)
    _against(key + ".dlw", Gd["lnw"], note)
    _against(key + ".dlb", Gd["lnb"], note)


@pytest.mark.parametrize("case", U.LINEAR, ids=lambda c: U.linear_name(*c))
def test_pixel_linear_forward_and_backward(case):
    K, sig, hw = case
    key = U.linear_name(*case)
    x, w, b, dp = U.linear_tensors(K, hw)
    _check_inputs(key, x, w, b, dp)
    xa = to_nhwc(x)
    wd, bd = w.cuda(), b.cuda()
    out = PH.linear_forward(xa, wd, bd, sig)
    assert out.shape == (U.B, K, hw[0], hw[1]) and out.is_contiguous()
    _against(key + ".out", out)
    dx, dw, db = PH.linear_backward(xa, wd, dp.cuda(), out if sig else None)
    _against(key + ".dx", _nchw(dx))
    _against(key + ".dw", dw)
    _against(key + ".db", db)


def test_pixel_linear_refuses_what_it_does_not_cover():
    L = N.lib()
    x, o, w = torch.zeros(64 * 72, device="cuda"), torch.zeros(4 * 64, device="cuda"), torch.zeros(4 * 72, device="cuda")
    assert L.vs_pixel_linear(N.ptr(x), 72, 1, 64, 68, N.ptr(w), None, 4, 0, N.ptr(o), N.stream()) == N.ERR_UNSUPPORTED      # C > 64
    assert L.vs_pixel_upgather_supported(24, 3) == 0 and L.vs_pixel_upgather_supported(22, 2) == 0 and L.vs_pixel_upgather_supported(260, 2) == 0
    assert all(L.vs_pixel_upgather_supported(c, f) == 1 for c in (4, 16, 20, 24, 32, 48, 64, 96, 192, 256) for f in (2, 4))
    assert L.vs_pixel_upgather(N.ptr(x), 72, 1, 2, 2, 6, 2, None, None, 1e-6, 0, N.ptr(o), 8, N.stream()) == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("hw", U.LATENTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_head_chain(eng, hw):
    """[4, 4, 2] chain + per-pixel linear layer (widths 32 / 8 / 4, 17 logits) through pixel_head.head_forward against the reference's PixelDecoder"""
    H, W = hw
    sd = U.head_tensors(U.CHAIN["embed_dim"], U.CHAIN["stages"], U.CHAIN["nbits"])
    x = U.chain_input(H, W)
    _check_inputs(f"chain_{H}x{W}", x, *sd.values())
    xa = to_nhwc(x)
    P = PH.pack_head(lambda k: sd[k].cuda(), "pixel_decoder", U.CHAIN["embed_dim"], U.CHAIN["stages"], xa.ld, True, False)
    preds = PH.head_forward(eng, xa, P, "t.chain")
    assert preds.shape == (U.B, U.CHAIN["nbits"] + 1, 32 * H, 32 * W)
    _against(f"chain_{H}x{W}.out", preds, "@" + ("split" if eng.use_split else "f32"))


LOSS_CASES = [(sk, kind) for sk in U.LOSS_SHAPES for kind in U.LOSS_MASKS if kind != "none"]


def _run_loss(sk, kind):
    preds, masks, msgs = U.loss_tensors(sk, kind)
    _check_inputs(f"loss_{sk}_{kind}", preds, masks, msgs.float())
    w_det, w_dec = G["meta"]["loss_w"]
    return PH.pixel_bce(preds.cuda(), masks.cuda(), msgs.to(torch.int32).cuda(), temperature=U.LOSS_T[kind], w_det=w_det, w_dec=w_dec)


@pytest.mark.parametrize("sk,kind", LOSS_CASES)
def test_detection_and_masked_decoding_loss(sk, kind):
    key = f"loss_{sk}_{kind}"
    loss, dpreds = _run_loss(sk, kind)
    want = G[key + ".loss"]
    err = float(np.abs(loss.double().cpu().numpy() - want).max())
    bound = max(4 * E[key + ".loss"], 1e-6)
    print(f"{key}.loss: {loss.tolist()} vs {want.tolist()}: err {err:.3e} (reference fp32 {E[key + '.loss']:.3e}, bound {bound:.3e})")
    _record(key + ".loss", err, bound)
    assert err <= bound
    _against(key + ".dpreds", dpreds)


@pytest.mark.parametrize("sk", list(U.LOSS_SHAPES))
def test_decoding_loss_over_nothing_is_nan(sk):
    key = f"loss_{sk}_none"
    loss, dpreds = _run_loss(sk, "none")
    want = G[key + ".loss"]
    assert np.isnan(want[1]) and torch.isnan(loss[1]), (want, loss)
    assert abs(float(loss[0]) - want[0]) <= max(4 * E[key + ".loss"], 1e-6)
    assert float(dpreds[:, 1:].abs().max()) == 0.0          # the decoding term reaches no logit; the plane is written, not left as it was
    _against(key + ".dpreds", dpreds)


def test_loss_refuses_a_mask_of_another_size():
    preds, masks, msgs = U.loss_tensors("e", "ones")
    with pytest.raises(ValueError):
        PH.pixel_bce(preds.cuda(), masks[..., :-1].contiguous().cuda(), msgs.to(torch.int32).cuda())


def _all_entry_points(guard):
    """every new entry point once, on tensors made by `guard(t, fill)` -> (buffer, view); returns (outputs, buffers with their fills)"""
    L, st = N.lib(), N.stream()
    bufs, outs = [], []

    def inp(t):
        b, v = guard(t.cuda().contiguous(), float("nan"))
        bufs.append((b, float("nan")))
        return v

    def outp(*shape, dtype=torch.float32):
        b, v = guard(torch.zeros(*shape, device="cuda", dtype=dtype), -7.0 if dtype.is_floating_point else -7)
        bufs.append((b, -7.0 if dtype.is_floating_point else -7))
        outs.append(v)
        return v
    g = torch.Generator().manual_seed(9)
    Bn, H, W, Co, f = 2, 3, 5, 24, 4
    z = inp(torch.randn(Bn, H, W, 9 * Co, generator=g))
    lw, lb = inp(torch.rand(Co, generator=g) + 0.5), inp(torch.randn(Co, generator=g))
    o = outp(Bn, f * H, f * W, Co)
    N.check(L.vs_pixel_upgather(N.ptr(z), 9 * Co, Bn, H, W, Co, f, N.ptr(lw), N.ptr(lb), 1e-6, N.ACT_GELU, N.ptr(o), Co, st), "vs_pixel_upgather")
    o = outp(Bn, f * H, f * W, Co)
    N.check(L.vs_pixel_upgather(N.ptr(z), 9 * Co, Bn, H, W, Co, f, None, None, 1e-6, 0, N.ptr(o), Co, st), "vs_pixel_upgather")
    for ff in (2, 4):
        dg = inp(torch.randn(Bn, ff * H, ff * W, Co, generator=g))
        dz = outp(Bn, H, W, 9 * Co)
        N.check(L.vs_pixel_upgather_bwd(N.ptr(dg), Co, Bn, H, W, Co, ff, N.ptr(dz), 9 * Co, st), "vs_pixel_upgather_bwd")
    for (hh, ww, K, C) in ((12, 20, 17, 24), (5, 7, 6, 24), (9, 31, 17, 32)):
        HW = hh * ww
        x = inp(torch.randn(Bn * HW, C, generator=g))
        w, b = inp(torch.randn(K, C, generator=g)), inp(torch.randn(K, generator=g))
        y = outp(Bn, K, hh, ww)
        N.check(L.vs_pixel_linear(N.ptr(x), C, Bn, HW, C, N.ptr(w), N.ptr(b), K, 1, N.ptr(y), st), "vs_pixel_linear")
        dp = inp(torch.randn(Bn, K, hh, ww, generator=g))
        dx, dw, db = outp(Bn * HW, C), outp(K, C), outp(K)
        part = outp(int(L.vs_pixel_linear_bwd_partial_floats(Bn * HW, K, C)))
        N.check(L.vs_pixel_linear_bwd(N.ptr(dp), N.ptr(y), N.ptr(x), C, Bn, HW, C, N.ptr(w), K, N.ptr(dx), C, N.ptr(dw), N.ptr(db), N.ptr(part), st),
                "vs_pixel_linear_bwd")
        m = inp((torch.rand(Bn, 1, hh, ww, generator=g) > 0.4).float())
        msgs = torch.randint(0, 2, (Bn, K - 1), generator=g).to(torch.int32).cuda()
        dpr, loss = outp(Bn, K, hh, ww), outp(2)
        pd = outp(int(L.vs_pixel_bce_partial_doubles(Bn, K, HW)), dtype=torch.float64)
        N.check(L.vs_pixel_bce(N.ptr(dp), N.ptr(m), N.ptr(msgs), Bn, Bn, K, HW, 1.5, 1.0, 0.5, N.ptr(dpr), N.ptr(pd), N.ptr(loss), st), "vs_pixel_bce")
        votes, nsel = outp(Bn, K, dtype=torch.int32), outp(Bn, dtype=torch.int32)
        N.check(L.vs_pixel_vote(N.ptr(dp), K * HW, N.ptr(m), Bn, K, HW, 0.1, N.ptr(votes), N.ptr(nsel), st), "vs_pixel_vote")
    torch.cuda.synchronize()
    return outs, bufs


def test_red_zones_and_two_runs_bit_identical():
    """every new entry point between poisoned guard areas (NaN around what it reads, a sentinel around what it writes), twice"""
    runs = []
    for _ in range(2):
        outs, bufs = _all_entry_points(_guarded)
        assert all(_guards_intact(b, fill) for b, fill in bufs)
        runs.append([o.clone() for o in outs])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num())
                                                for a, b in zip(*runs))
    assert all(torch.isfinite(o.double()).all() for o in runs[0])


def test_metrics_take_the_vote_kernel():
    """bit_accuracy / bit_accuracy_1msg on device 4-D logits equal the torch path on the same values and the reference's recorded results
    (the logits keep a distance of more than 1e-3 from both thresholds, so `>` is the same decision in any arithmetic)"""
    Bn, K, H, W = 3, 7, 10, 12
    logits = U.vote_logits(Bn, K, H, W, seed=21)
    gg = torch.Generator().manual_seed(22)
    bits = torch.randint(0, 2, (Bn, K), generator=gg)
    mask = torch.zeros(Bn, 1, H, W)
    mask[:, :, 2:7, 3:11] = 1.0
    _check_inputs("vote", logits, bits.float(), mask)
    # "the torch path on the same values" runs on the same device (float64 copies of the logits: exactly the same values, and float64 never takes
    # the kernel), so the comparison is exact; the host's `mean` may round the last bit of k/7 differently from the device's, hence 1e-7 against
    # the values recorded from the reference on a CPU
    for thr in (0.0, 0.25):
        assert float((logits - thr).abs().min()) > 1e-3
        for m, tag in ((None, ""), (mask, "_masked")):
            md = None if m is None else m.cuda()
            M.LAST_VOTE_BACKEND = None
            a = M.bit_accuracy(logits.cuda(), bits.cuda(), md, thr)
            assert M.LAST_VOTE_BACKEND == "hip"
            want = M.bit_accuracy(logits.cuda().double(), bits.cuda(), md, thr)
            assert M.LAST_VOTE_BACKEND == "torch"
            assert a.dtype == want.dtype and torch.equal(a, want)
            assert np.abs(a.cpu().double().numpy() - G[f"vote_acc{tag}_thr{thr}"]).max() <= 1e-7
            b = M.bit_accuracy_1msg(logits.cuda(), bits.cuda(), md, thr)
            assert M.LAST_VOTE_BACKEND == "hip"
            want = M.bit_accuracy_1msg(logits.cuda().double(), bits.cuda(), md, thr)
            assert M.LAST_VOTE_BACKEND == "torch"
            # exact: the hits are whole numbers counted by torch on the same values, and the result is their ratio rounded once (a float32 `mean` may
            # round sum x (1 / n) or sum / n, one ulp apart, which is why the comparison goes through the counts)
            sel_ = torch.ones(Bn, 1, H, W, dtype=torch.bool) if m is None else m.bool()
            hit_ = (((logits > thr) == (bits > 0.5)[:, :, None, None]) & sel_).sum(dim=(1, 2, 3))
            exact = (hit_.double() / (sel_.sum(dim=(1, 2, 3)) * K).double()).float()
            assert b.dtype == want.dtype and b.device == want.device and torch.equal(b.cpu(), exact)
            assert float((b - want).abs().max()) <= 2.0 ** -24          # and the torch path's own float32 mean is that ratio within its last bit
            assert np.abs(b.cpu().double().numpy() - G[f"vote_1msg{tag}_thr{thr}"]).max() <= 1e-7
            votes, nsel = PH.pixel_vote(logits.cuda(), md, thr)
            sel = torch.ones(Bn, 1, H, W, dtype=torch.bool) if m is None else m.bool()
            assert torch.equal(votes.cpu().long(), ((logits > thr) & sel).sum(dim=(2, 3))) and torch.equal(nsel.cpu().long(), sel.sum(dim=(1, 2, 3)))
    # a channel slice of wider predictions is read in place (`preds[:, 1:]`, what train.py passes)
    wide = torch.cat([torch.randn(Bn, 1, H, W), logits], dim=1).cuda()
    assert torch.equal(M.bit_accuracy(wide[:, 1:], bits.cuda(), mask.cuda()), M.bit_accuracy(logits.cuda().double(), bits.cuda(), mask.cuda()))
    # frames that select different numbers of pixels: the reference's view() regroups values across frames -- only the torch code does that
    uneven = mask.clone()
    uneven[0, :, 2:4] = 0.0
    uneven[1, :, 0:2, 3:11] = 1.0
    assert int(uneven[0].sum()) != int(uneven[1].sum()) and int(uneven.sum()) % Bn == 0
    M.LAST_VOTE_BACKEND = None
    got = M.bit_accuracy(logits.cuda(), bits.cuda(), uneven.cuda())
    assert M.LAST_VOTE_BACKEND == "torch" and torch.equal(got, M.bit_accuracy(logits.cuda().double(), bits.cuda(), uneven.cuda()))
