"""SSIM / MS-SSIM / JND on the HIP path (csrc/ssim.hip, autograd.SsimStatsFn / JndLossFn / percep_loss, metrics.ssim / msssim) against the
float64 run of the unmodified reference (tests/golden/ssim_loss.npz, tests/golden/make_golden_ssim.py).

Tolerance.  The yardstick is the reference, not the code under test: per case and quantity the fixture holds what the reference's OWN fp32 run
loses against its float64 run (`e_*`).  The HIP result, compared with the same float64 values, gets 4 x that figure -- a different but equally
valid fp32 evaluation (tiles, ring order, per-tile partial sums) --, with two floors so that a lucky small e_ref does not make the bound
meaningless: 2e-7 absolute on a loss value or a statistic, 2e-5 relative-to-max on a gradient element (2e-5 of the norm on the L2 error).
The `jnd` term is bounded by the heat-map's error the project already holds (|dh| < 2e-6, tests/test_gpu_kernels.py::test_jnd_heatmap_nchw):
every element of N g within 2 * 2e-6 + 1e-6, the loss within 2 * mean||d| - h| * 2e-6 + 2e-7.  `mse` / `yuv` terms get the bounds of
tests/test_gpu_train.py::test_perceptual_and_decoding_loss_nodes (2e-6 relative on the loss, 1e-5 of max|g| per element).  A combined string
gets the weighted sum of its terms' bounds.  Derived bounds for the summaries of a gradient with element bound E, L2 bound L and n elements:
|norm - norm64| <= L (triangle inequality); sum and the +-1 projection: 4 x max(the reference's own error of that quantity, L) -- an error
vector of L2 norm L projected on a sign vector has standard deviation L.

With VS_SSIM_PARITY_OUT=<file> the measured errors of every case are written there (profiles/ssim_parity.json is such a run)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.weights import make_state_dict, tiny_spec
from tests._util import load_golden, projection_vector
from tests._cases import check_inputs, make_inputs
from tests._guards import _guarded, _guards_intact
from videoseal_amd import autograd as AG
from videoseal_amd import metrics as M
from videoseal_amd import native as N

pytestmark = pytest.mark.gpu

G = load_golden("ssim_loss")
CASES = G["meta"]["cases"]
PAIRS = [(c, s) for c, info in CASES.items() for s in info["strings"]]
MEASURED = {}


def _record(key, **kw):
    MEASURED.setdefault(key, {}).update({k: float(v) for k, v in kw.items()})
    path = os.environ.get("VS_SSIM_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _inputs(cname):
    x, y = make_inputs(CASES[cname])
    check_inputs(G, cname, x, y)
    return x, y


@pytest.mark.parametrize("cname", list(CASES))
def test_statistics_kernel_matches_the_reference_at_every_level(cname):
    info = CASES[cname]
    x, y = _inputs(cname)
    s, c, _ = AG.ssim_pyramid(x.cuda(), y.cuda(), info["levels"])
    got = torch.stack([s, c], dim=1).cpu().numpy()                  # [L, 2, F, C]
    err = np.abs(got - G[f"{cname}.stats"]).max()
    tol = max(4 * info["e_stats"], 2e-7)
    print(f"{cname}: max |stat - float64| = {err:.3e} (reference fp32: {info['e_stats']:.3e}, bound {tol:.3e})")
    _record(f"{cname}.stats", err=err, e_ref=info["e_stats"], bound=tol)
    assert err <= tol


def _term_bounds(cname, name, n):
    """(V, E, L): bounds on the loss, on a gradient element and on the L2 norm of the gradient error of ONE term"""
    info = CASES[cname]
    t = info["terms"][name]
    if name in ("mse", "yuv"):
        E = 1e-5 * t["gmax"]
        return 2e-6 * abs(t["loss"]) + 1e-12, E, E * math.sqrt(n)
    if name == "jnd":
        E = (2 * 2e-6 + 1e-6) / n
        return 2 * info["jnd_mean_abs"] * 2e-6 + 2e-7, E, E * math.sqrt(n)
    r = info["strings"][name]
    return max(4 * r["e_loss"], 2e-7), max(4 * r["e_grad_max"], 2e-5) * t["gmax"], max(4 * r["e_grad_l2"], 2e-5) * t["gnorm"]


def _bounds(cname, string, n):
    weights, names = AG.parse_percep_loss(string)
    if weights is None:
        return _term_bounds(cname, names[0], n)
    per = [_term_bounds(cname, nm, n) for nm in names]
    return tuple(sum(w * b[k] for w, b in zip(weights, per)) for k in range(3))


def _hip_loss_and_grad(x, y, string):
    yg = y.cuda().requires_grad_(True)
    loss = AG.percep_loss(x.cuda(), yg, string).mean()
    loss.backward()
    return loss.detach(), yg.grad


@pytest.mark.parametrize("cname,string", PAIRS)
def test_loss_and_gradient_match_the_reference(cname, string):
    info, ref = CASES[cname], CASES[cname]["strings"][string]
    x, y = _inputs(cname)
    loss, grad = _hip_loss_and_grad(x, y, string)
    g = grad.double().cpu()
    n = g.numel()
    V, E, L = _bounds(cname, string, n)
    key = f"{cname}.{string}"
    want = G[key + ".grad_summary"]                                   # norm, sum, projection, max|g| of the float64 gradient
    flat = g.flatten()
    e_loss = abs(float(loss) - ref["loss"])
    e_sub = float((g[..., ::info["sub"], ::info["sub"]] - torch.from_numpy(G[key + ".grad_sub"]).double()).abs().max())
    e_norm = abs(float(flat.norm()) - want[0])
    e_sum = abs(float(flat.sum()) - want[1])
    e_proj = abs(float((flat * projection_vector(key, n)).sum()) - want[2])
    sub_store = float(np.abs(G[key + ".grad_sub"]).max()) * 2.0 ** -24           # the fixture keeps the sub-sample in float32
    print(f"{key}: loss err {e_loss:.3e} (ref fp32 {ref['e_loss']:.3e}, bound {V:.3e}); element err / max|g| {e_sub / want[3]:.3e} "
          f"(ref {ref['e_grad_max']:.3e}, bound {E / want[3]:.3e}); norm err {e_norm:.3e} (bound {L:.3e}); sum err {e_sum:.3e} "
          f"(ref {ref['e_sum']:.3e}); proj err {e_proj:.3e} (ref {ref['e_proj']:.3e})")
    _record(key, e_loss=e_loss, e_loss_ref=ref["e_loss"], loss_bound=V, e_grad_max_rel=e_sub / want[3], e_grad_max_rel_ref=ref["e_grad_max"],
            grad_bound_rel=E / want[3], e_norm=e_norm, norm_bound=L, e_sum=e_sum, e_sum_ref=ref["e_sum"], e_proj=e_proj, e_proj_ref=ref["e_proj"])
    assert torch.isfinite(grad).all()
    assert e_loss <= V
    assert e_sub <= E + sub_store
    assert e_norm <= L
    assert e_sum <= 4 * max(ref["e_sum"], L)
    assert e_proj <= 4 * max(ref["e_proj"], L)


@pytest.mark.parametrize("cname,string", [("c40x37", "ssim"), ("c200x176", "ssim"), ("c200x176", "msssim")])
def test_full_gradient_against_float64_autograd_through_the_torch_restatement(cname, string):
    ref = CASES[cname]["strings"][string]
    x, y = _inputs(cname)
    y64 = y.double().requires_grad_(True)
    l64 = -(M.ssim if string == "ssim" else M.msssim)(x.double(), y64).mean()
    l64.backward()
    loss, grad = _hip_loss_and_grad(x, y, string)
    gmax = float(y64.grad.abs().max())
    d = grad.double().cpu() - y64.grad
    e_max, e_l2 = float(d.abs().max()) / gmax, float(d.norm() / y64.grad.norm())
    print(f"{cname}.{string}: max element err / max|g| = {e_max:.3e} (ref fp32 {ref['e_grad_max']:.3e}); L2 err / norm = {e_l2:.3e} "
          f"(ref {ref['e_grad_l2']:.3e})")
    _record(f"{cname}.{string}.full", e_grad_max_rel=e_max, e_grad_max_rel_ref=ref["e_grad_max"], e_grad_l2_rel=e_l2, e_grad_l2_rel_ref=ref["e_grad_l2"])
    assert abs(float(loss) - float(l64)) <= max(4 * ref["e_loss"], 2e-7)
    assert e_max <= max(4 * ref["e_grad_max"], 2e-5)
    assert e_l2 <= max(4 * ref["e_grad_l2"], 2e-5)


@pytest.mark.parametrize("H,W", [(37, 41), (40, 36), (177, 164), (64, 33)])
def test_pooling_and_its_adjoint(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x, y = torch.rand(2, 3, H, W, generator=g), torch.rand(2, 3, H, W, generator=g)
    pad = [H % 2, W % 2]
    xo, yo = AG.avgpool2_pad(x.cuda(), y.cuda())
    ulp = 2.0 ** -23                                                   # 1 ulp of the largest input (< 1)
    for got, src in ((xo, x), (yo, y)):
        want = F.avg_pool2d(src, 2, padding=pad)
        assert got.shape == want.shape and (got.cpu() - want).abs().max() <= ulp
    # the adjoint lives in vs_ssim_grad's store: with zero coefficients the output is the pooled-level gradient through the 2 x 2 mean alone
    xr = x.clone().requires_grad_(True)
    gc = torch.rand(F.avg_pool2d(x, 2, padding=pad).shape, generator=g)
    F.avg_pool2d(xr, 2, padding=pad).backward(gc)
    z = torch.zeros(6, device="cuda")
    got = AG.ssim_grad(x.cuda(), y.cuda(), z, z, gc.cuda().contiguous())
    assert (got.cpu() - xr.grad).abs().max() <= ulp


def test_red_zones():
    """odd W, H no multiple of any tile: x, y between NaN guards, the gradient (and the statistics) between sentinels"""
    Fr, Cc, H, W = 2, 3, 139, 131
    g = torch.Generator().manual_seed(5)
    x = torch.rand(Fr, Cc, H, W, generator=g).cuda()
    y = (x + 0.03 * torch.randn(Fr, Cc, H, W, generator=g).cuda()).clamp(0, 1)
    gs = torch.rand(Fr * Cc, generator=g).cuda() - 0.5
    gc = torch.rand(Fr * Cc, generator=g).cuda() - 0.5
    gco = torch.rand(Fr, Cc, (H + 1) // 2, (W + 1) // 2, generator=g).cuda()
    s0, c0, _ = AG.ssim_pyramid(x, y, 1)
    d0 = AG.ssim_grad(x, y, gs, gc, gco)
    p0 = AG.avgpool2_pad(x, y)
    nan = float("nan")
    (bx, vx), (by, vy), (bgs, vgs), (bgc, vgc), (bgo, vgo) = (_guarded(t, nan) for t in (x, y, gs, gc, gco))
    L = N.lib()
    P = Fr * Cc
    bo, vo = _guarded(torch.zeros(2, P, device="cuda", dtype=torch.float64), -7.0)
    part = torch.empty(int(L.vs_ssim_partial_doubles(P, H, W)), device="cuda", dtype=torch.float64)
    N.check(L.vs_ssim_stats(N.ptr(vx), N.ptr(vy), P, H, W, 1.0, AG._win11(), N.ptr(part), N.ptr(vo), N.stream()), "vs_ssim_stats")
    bd, vd = _guarded(torch.zeros_like(x), -7.0)
    N.check(L.vs_ssim_grad(N.ptr(vx), N.ptr(vy), N.ptr(vgs), N.ptr(vgc), N.ptr(vgo), P, H, W, 1.0, AG._win11(), N.ptr(vd), N.stream()), "vs_ssim_grad")
    bpx, vpx = _guarded(torch.zeros_like(p0[0]), -7.0)
    bpy, vpy = _guarded(torch.zeros_like(p0[1]), -7.0)
    N.check(L.vs_avgpool2_pad(N.ptr(vx), N.ptr(vy), P, H, W, N.ptr(vpx), N.ptr(vpy), N.stream()), "vs_avgpool2_pad")
    torch.cuda.synchronize()
    assert torch.equal(vo[0].view(Fr, Cc), s0[0]) and torch.equal(vo[1].view(Fr, Cc), c0[0])
    assert torch.equal(vd, d0) and torch.equal(vpx, p0[0]) and torch.equal(vpy, p0[1])
    assert all(_guards_intact(b, nan) for b in (bx, by, bgs, bgc, bgo))
    assert all(_guards_intact(b, -7.0) for b in (bo, bd, bpx, bpy))


def test_two_launches_are_bit_identical():
    x, y = _inputs("c177x163")
    runs = []
    for _ in range(2):
        s, c, _ = AG.ssim_pyramid(x.cuda(), y.cuda(), 5)
        out = [s.clone(), c.clone()]
        for string in ("ssim", "msssim", "jnd"):
            out += list(_hip_loss_and_grad(x, y, string))
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_metrics_take_the_hip_path():
    cname = "c200x176"
    info = CASES[cname]
    x, y = _inputs(cname)
    tol = max(4 * info["e_stats"], 2e-7)
    M.LAST_SSIM_BACKEND = None
    s = M.ssim(x.cuda(), y.cuda())
    assert M.LAST_SSIM_BACKEND == "hip" and s.shape == (info["F"],) and s.dtype == torch.float32
    assert np.abs(s.cpu().double().numpy() - M.ssim(x.double(), y.double()).numpy()).max() <= tol + 2.0 ** -24
    assert M.LAST_SSIM_BACKEND == "torch"
    m = M.msssim(x.cuda(), y.cuda())
    assert M.LAST_SSIM_BACKEND == "hip" and m.shape == (info["F"],)
    assert np.abs(m.cpu().double().numpy() - M.msssim(x.double(), y.double()).numpy()).max() <= tol + 2.0 ** -24
    with pytest.raises(AssertionError, match="larger than 160"):
        M.msssim(x[..., :160, :].cuda(), y[..., :160, :].cuda())
    with pytest.raises(ValueError):
        M.ssim(x[..., :10, :].contiguous().cuda(), y[..., :10, :].contiguous().cuda())
    lib = N.lib()
    assert lib.vs_ssim_stats(None, None, 6, 40, 40, 1.0, None, None, None, None) == -1
    assert lib.vs_ssim_partial_doubles(6, 10, 40) == 0


@pytest.mark.parametrize("string", ["ssim", "msssim", "mse+0.1_ssim"])
def test_generator_step_with_the_new_terms(string):
    from tests._model import make_model
    from oracle.inputs import synthetic_frames, synthetic_msgs
    from videoseal_amd import augmentation as A
    from videoseal_amd.training import GeneratorStep
    spec = tiny_spec()
    model = make_model(spec, make_state_dict(spec, seed=3))
    model.augmenter = A.Augmenter(masks={"kind": "none"}, augs={"identity": 1}, augs_params={}, num_augs=1)
    model.train()
    imgs = synthetic_frames(16, 256, 256, seed=71).cuda()
    msgs = synthetic_msgs(16, spec.nbits, seed=71)
    masks = torch.ones(16, 1, 256, 256, device="cuda")
    step = GeneratorStep(model, percep_loss=string, percep_weight=1.0, decode_weight=1.0, balanced=True)
    torch.manual_seed(1)
    _, log, outputs = step.step(imgs, masks, msgs)
    node = AG.percep_loss(imgs, outputs["imgs_w"].detach(), string).mean()
    assert torch.equal(log["loss_percep"].reshape(()), node.detach().reshape(()))
    sc = float(log["scale_percep"])
    assert math.isfinite(sc) and sc > 0
    emb = [(k, p) for k, p in model.named_parameters() if k.startswith("embedder.") and p.requires_grad]
    assert emb and all(p.grad is not None and torch.isfinite(p.grad).all() for _, p in emb), [k for k, p in emb if p.grad is None]
    assert float(model.embedder.get_last_layer().grad.abs().max()) > 0
