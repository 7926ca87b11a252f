"""End-to-end parity of the HIP path, through the public Videoseal API, against
 (a) the golden vectors produced by the unmodified reference (tests/golden/*.npz) and
 (b) the CPU oracle on fresh seeded inputs,
with the tolerances of BASELINE.json: PSNR / logits within 1e-3, thresholded bit decisions identical."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import videoseal_ref as R  # noqa: E402
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from oracle.weights import legacy_tiny_spec, make_state_dict, spec_from_card, tiny_spec  # noqa: E402
from tests._cases import CARDS, FULL, TINY, TINYC  # noqa: E402
from tests._model import TOL_IMG, TOL_LOGIT, _run_case, cfg_of, make_model  # noqa: E402
from tests._util import DECISION_MARGIN, assert_decisions, check_sub, load_golden, psnr_np  # noqa: E402

import videoseal_amd  # noqa: E402


@pytest.fixture(scope="module")
def tiny():
    s = tiny_spec()
    sd = make_state_dict(s, seed=3)
    return s, sd, make_model(s, sd)


@pytest.fixture(scope="module")
def vs10():
    s = spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml"))
    sd = make_state_dict(s, seed=0)
    return s, sd, make_model(s, sd)


@pytest.mark.parametrize("name", TINY)
def test_tiny_matches_reference_golden(tiny, name):
    _run_case(*tiny, name)


@pytest.fixture(scope="module")
def tinyc():
    s = tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16)
    sd = make_state_dict(s, seed=4)
    return s, sd, make_model(s, sd)


@pytest.mark.parametrize("name", TINYC)
def test_tiny_chunky_matches_reference_golden(tinyc, name):
    """ChunkySeal-shaped architecture: RGB embedder, stride-2 stem, channel counts not multiple of 4, odd feature maps."""
    _run_case(*tinyc, name)


@pytest.fixture(scope="module")
def tinyv():
    s = legacy_tiny_spec()
    sd = make_state_dict(s, seed=6)
    return s, sd, make_model(s, sd)


@pytest.mark.parametrize("name", ["tinyv_img", "tinyv_img_resize", "tinyv_vid"])
def test_tiny_legacy_matches_reference_golden(tinyv, name):
    """videoseal_0.0 family: ChanRMSNorm/SiLU RGB U-Net, ViT extractor (windowed + global attention with decomposed
    relative positions), no JND -- HIP path vs fixtures of the unmodified reference"""
    _run_case(*tinyv, name)


@pytest.mark.parametrize("name", ["vs00_img256", "vs00_vid"])
def test_vs00_matches_reference_golden(name):
    """the released legacy card itself (96 bits, 12-block ViT-S/16 extractor) through videoseal_amd.build"""
    s = spec_from_card(os.path.join(CARDS, "videoseal_0.0.yaml"))
    sd = make_state_dict(s, seed=5)
    m = videoseal_amd.build("videoseal_0.0")
    assert m.attenuation is None and m.embedder.cfg.extractor == "sam"
    msg = m.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    _run_case(s, sd, m.eval().to("cuda"), name)


@pytest.mark.parametrize("name", FULL)
def test_vs10_matches_reference_golden(vs10, name):
    _run_case(*vs10, name)


def test_configs1_stated_size_matches_the_reference_golden(vs10):
    """BASELINE configs[1] AT ITS STATED SIZE -- the workload bench.py's `value` is measured on: 32 frames of 768 x 768, image mode (one
    message per frame, every frame through the U-Net, full-resolution JND), embed + detect, against the unmodified reference's run of
    exactly that (tests/golden/make_golden_cfg1.py): watermarked pixels, PSNR (whole batch and per frame), logits on watermarked and on
    clean frames, every thresholded decision."""
    spec, sd, model = vs10
    _run_case(spec, sd, model, "vs10_img_768x32")
    g = load_golden("vs10_img_768x32")
    meta = g["meta"]
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"])
    msgs = synthetic_msgs(meta["n"], spec.nbits, seed=meta["seed"])
    w = model.embed(imgs.cuda(), msgs, is_video=False)["imgs_w"]
    d = 255.0 * (w.double() - imgs.cuda().double())
    psnr_frame = (20 * torch.log10(torch.tensor(255.0, dtype=torch.float64)) - 10 * torch.log10((d ** 2).mean(dim=(1, 2, 3)).cpu()))
    assert (psnr_frame - torch.from_numpy(g["psnr_frame"])).abs().max().item() < 1e-3
    preds = model.detect(w, is_video=False)["preds"].cpu()
    acc = float(((preds[:, 1:] > 0) == (msgs > 0.5)).float().mean())
    assert acc == meta["bit_acc"], "bit accuracy against the embedded messages differs from the reference's"


@pytest.mark.parametrize("mode,name", [("bf16x3", "vs10_img256"), ("bf16x3", "vs10_vid"), ("f32", "vs10_img256"), ("f16x2", "vs10_img_odd")])
def test_vs10_every_arithmetic_matches_reference_golden(monkeypatch, mode, name):
    """the three arithmetic back-ends of the dense layers (VIDEOSEAL_CONV: 2 x f16 split = default, exact 3 x bf16 split, f32 MFMA)
    against the same goldens of the unmodified reference, same tolerances, bit decisions identical on identical inputs."""
    monkeypatch.setenv("VIDEOSEAL_CONV", mode)
    s = spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml"))
    sd = make_state_dict(s, seed=0)
    m = make_model(s, sd)
    eng = m._engine()
    assert (eng.use_split, eng.arith if eng.use_split else 0) == {"bf16x3": (True, 3), "f16x2": (True, 2), "f32": (False, 0)}[mode]
    _run_case(s, sd, m, name)


def test_f16_range_overflow_is_handled_by_default_and_loud_when_forced(monkeypatch):
    """2 x f16 arithmetic: an activation beyond the f16 range of the operand split becomes inf / NaN (never a silently wrong finite number).
    Default (VIDEOSEAL_CONV unset = auto): the always-on guard sees it on the first pass with these weights, switches the network to the exact
    3 x bf16 split and repeats the pass -- the caller gets correct frames.  Forced f16x2: NaN frames, or an exception with VIDEOSEAL_CHECK_FINITE=1."""
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    big = {k: (v * 3e4 if k.endswith("inc.double_conv.0.weight") else v) for k, v in sd.items()}      # first conv: activations ~1e4..1e5
    imgs = synthetic_frames(2, 64, 64, seed=8).cuda()
    msgs = synthetic_msgs(2, spec.nbits, seed=8)
    monkeypatch.delenv("VIDEOSEAL_CONV", raising=False)
    monkeypatch.delenv("VIDEOSEAL_CHECK_FINITE", raising=False)
    m = make_model(spec, big)
    with pytest.warns(UserWarning, match="3 x bf16"):
        out = m.embed(imgs, msgs, is_video=False)["imgs_w"]
    ref = R.embed_image(big, spec, imgs.cpu(), msgs)["imgs_w"]
    assert torch.isfinite(out).all() and (out.cpu() - ref).abs().max() < TOL_IMG
    assert m._engine().arith_net == {"E": 3, "X": 2}
    out2 = m.embed(imgs, msgs, is_video=False)["imgs_w"]                     # stays on the safe arithmetic, no second warning / sync
    assert torch.equal(out, out2)
    monkeypatch.setenv("VIDEOSEAL_CHECK_FINITE", "1")
    monkeypatch.setenv("VIDEOSEAL_CONV", "f16x2")
    m = make_model(spec, big)
    with pytest.raises(videoseal_amd.native.NativeError, match="bf16x3"):
        m.embed(imgs, msgs, is_video=False)
    monkeypatch.setenv("VIDEOSEAL_CHECK_FINITE", "0")          # forced fast arithmetic without the check: the NaN reaches the caller
    m0 = make_model(spec, big)
    assert not torch.isfinite(m0.embed(imgs, msgs, is_video=False)["imgs_w"]).all()
    monkeypatch.setenv("VIDEOSEAL_CONV", "bf16x3")
    m3 = make_model(spec, big)
    assert torch.isfinite(m3.embed(imgs, msgs, is_video=False)["imgs_w"]).all()


def test_grn_outlier_channels_match_the_oracle_by_default(monkeypatch):
    """GRN gamma x 1e3 (the kind of outlier channel a trained ChunkySeal-size extractor can carry): the pwconv2 operand h * (1 + gamma Nx)
    leaves the f16 range; with the default arithmetic selection the logits still match the oracle"""
    monkeypatch.delenv("VIDEOSEAL_CONV", raising=False)
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    big = {k: (v * 1e3 if k.endswith("grn.gamma") else v) for k, v in sd.items()}
    imgs = synthetic_frames(3, 64, 64, seed=9)
    ref = R.detect(big, spec, imgs)["preds"]
    assert ref.abs().max() < 1e6
    m = make_model(spec, big)
    preds = m.detect(imgs.cuda(), is_video=False)["preds"].cpu()
    assert torch.isfinite(preds).all()
    assert (preds - ref).abs().max() <= 2e-3 * max(1.0, float(ref.abs().max()))


def test_one_outlier_block_keeps_the_rest_of_the_extractor_on_the_fast_split(monkeypatch):
    """the arithmetic is chosen per LAYER: GRN gamma x 1e3 in ONE block -> the calibration pass (engine._calibrate_extractor, vs_absmax of every
    block GEMM's operand on the exact split) pins that block's pwconv2 to 3 x bf16 and leaves every other layer on the 2 x f16 split; logits
    match the oracle; VIDEOSEAL_LAYER_ARITH=0 keeps the whole-network switch"""
    monkeypatch.delenv("VIDEOSEAL_CONV", raising=False)
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    key = "detector.convnext.stages.1.0.grn.gamma"
    big = {k: (v * 1e5 if k == key else v) for k, v in sd.items()}           # (x 1e3 in this one block stays inside the f16 range: no switch at all)
    imgs = synthetic_frames(3, 64, 64, seed=9)
    ref = R.detect(big, spec, imgs)["preds"]
    m = make_model(spec, big)
    with pytest.warns(UserWarning, match="keep the exact 3 x bf16 split"):
        preds = m.detect(imgs.cuda(), is_video=False)["preds"].cpu()
    eng = m._engine()
    assert eng.arith_net["X"] == 2 and eng.verified["X"] and set(eng.layer_arith) == {(1, 0, "pw2")}
    assert eng.calib_absmax[(1, 0, "pw2")] > 65504 and len(eng.calib_absmax) == 2 * sum(spec.depths)
    assert torch.isfinite(preds).all()
    assert (preds - ref).abs().max() <= 2e-3 * max(1.0, float(ref.abs().max()))
    again = m.detect(imgs.cuda(), is_video=False)["preds"].cpu()           # steady state: same configuration, same values
    assert torch.equal(again, preds)
    m.load_state_dict(sd)                                                   # new weights: back to the fast split everywhere
    ok = m.detect(imgs.cuda(), is_video=False)["preds"].cpu()
    assert not m._engine().layer_arith and m._engine().arith_net["X"] == 2
    assert (ok - R.detect(sd, spec, imgs)["preds"]).abs().max() <= 1e-3
    monkeypatch.setenv("VIDEOSEAL_LAYER_ARITH", "0")
    m2 = make_model(spec, big)
    p2 = m2.detect(imgs.cuda(), is_video=False)["preds"].cpu()
    assert m2._engine().arith_net["X"] == 3 and not m2._engine().layer_arith
    assert (p2 - ref).abs().max() <= 2e-3 * max(1.0, float(ref.abs().max()))


def test_data_dependent_overflow_is_reported_by_the_next_call(monkeypatch):
    """weights verified on ordinary frames, then an input that drives the stem out of the f16 range: the pass itself cannot be repeated without
    a synchronisation per call, so its logits are non-finite -- but the next API call says so and the model has moved to 3 x bf16"""
    monkeypatch.delenv("VIDEOSEAL_CONV", raising=False)
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    m = make_model(spec, sd)
    imgs = synthetic_frames(2, 64, 64, seed=10).cuda()
    ok = m.detector(imgs)                                      # verifies the extractor's weights (synchronous check, passes)
    assert torch.isfinite(ok).all() and m._engine().verified["X"]
    bad = m.detector(imgs * 3e4)
    torch.cuda.synchronize()
    assert not torch.isfinite(bad).all()
    with pytest.raises(videoseal_amd.native.NativeError, match="earlier call"):
        m.detector(imgs)
    again = m.detector(imgs * 3e4)                             # the range-free arithmetic handles it
    assert torch.isfinite(again).all() and m._engine().arith_net["X"] == 3
    ref = R.extractor_forward(sd, spec, imgs.cpu() * 3e4)
    assert (again.cpu() - ref).abs().max() <= 2e-3 * max(1.0, float(ref.abs().max()))


def test_bottleneck_planes_chain_is_bit_identical(vs10):
    """26 frames at the processing size give the all-DMA planes kernel a workgroup per CU, so the engine runs the bottleneck chain on
    pre-split operand planes (engine.bottleneck_planes); same products, same K order, same scaling as the per-conv path: bit-identical."""
    spec, sd, model = vs10
    imgs = synthetic_frames(26, 256, 256, seed=41).cuda()
    msgs = synthetic_msgs(26, spec.nbits, seed=41)
    eng = model._engine()
    if eng.arith != 2:
        pytest.skip("2 x f16 arithmetic only")
    used = []
    orig = eng.bottleneck_planes
    eng.bottleneck_planes = lambda *a, **k: (used.append(1), orig(*a, **k))[1]
    try:
        a = model.embed(imgs, msgs, is_video=False)["imgs_w"].clone()
        assert used, "the planes chain did not run"
        eng.planes_chain = False
        b = model.embed(imgs, msgs, is_video=False)["imgs_w"].clone()
    finally:
        eng.planes_chain = True
        eng.bottleneck_planes = orig
    assert torch.equal(a, b)
    ref = R.embed_image(sd, spec, imgs[:2].cpu(), msgs[:2])["imgs_w"]
    assert (a[:2].cpu() - ref).abs().max() < TOL_IMG


@pytest.mark.parametrize("nkey", [4, 8, 3])
def test_bottleneck_planes_chain_with_k_slices_for_few_key_frames(vs10, nkey):
    """4 - 8 key frames (a 16- / 32-frame video call) give the planes kernel 32 - 64 output tiles: the chain then runs with K slices (raw partial
    sums per slice, summed in slice order by the split-K epilogue, which also writes the next conv's operand planes) -- deterministic, and equal to
    the per-conv path up to the summation order"""
    spec, sd, model = vs10
    imgs = synthetic_frames(nkey, 256, 256, seed=43).cuda()
    msgs = synthetic_msgs(nkey, spec.nbits, seed=43)
    eng = model._engine()
    if eng.arith_net["E"] != 2 or not eng.planes_splitk:
        pytest.skip("2 x f16 arithmetic only")
    used = []
    orig = eng.bottleneck_planes
    eng.bottleneck_planes = lambda *a, **k: (used.append(eng._planes_split(a[0])), orig(*a, **k))[1]
    try:
        a = model.embed(imgs, msgs, is_video=False)["imgs_w"].clone()
        a2 = model.embed(imgs, msgs, is_video=False)["imgs_w"].clone()
        assert used and used[0] > 1, "the planes chain did not run with K slices"
        eng.planes_chain = False
        b = model.embed(imgs, msgs, is_video=False)["imgs_w"].clone()
    finally:
        eng.planes_chain = True
        eng.bottleneck_planes = orig
    assert torch.equal(a, a2)
    assert (a - b).abs().max() < 2e-6
    ref = R.embed_image(sd, spec, imgs.cpu(), msgs)["imgs_w"]
    assert (a.cpu() - ref).abs().max() < TOL_IMG


def test_submodules_match_golden(vs10):
    """model.embedder(y, msgs) / model.detector(x) / model.attenuation.heatmaps(x) (SURVEY 8(b) method surface)."""
    spec, sd, model = vs10
    g = load_golden("vs10_img256")
    meta = g["meta"]
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"])
    msgs = synthetic_msgs(meta["n"], spec.nbits, seed=meta["seed"])
    y = R.rgb2y(sd, imgs)
    check_sub(g, "delta", model.embedder(y.cuda(), msgs), 2e-5)
    check_sub(g, "hmaps", model.attenuation.heatmaps(imgs.cuda()), 2e-6)
    logits = model.detector(imgs.cuda()).cpu()
    assert (logits - torch.from_numpy(g["preds_clean"])).abs().max() < 1e-4


def test_cpu_inputs_round_trip(tiny):
    """frames handed over on the CPU come back on the CPU with identical values (wam.py:165,186 device contract)."""
    spec, sd, model = tiny
    imgs = synthetic_frames(4, 64, 64, seed=21)
    msgs = synthetic_msgs(1, spec.nbits, seed=21)
    model.chunk_size, model.step_size, model.video_mode = 4, 2, "repeat"
    a = model.embed(imgs, msgs, is_video=True)
    b = model.embed(imgs.cuda(), msgs, is_video=True)
    assert a["imgs_w"].device.type == "cpu" and torch.equal(a["imgs_w"], b["imgs_w"].cpu())
    assert a["msgs"].shape == (4, spec.nbits)


def test_cpu_callers_get_the_device_results_through_pinned_host_memory(tiny):
    """every no-grad entry point with the frames on the CPU: results on the CPU, bit-equal to the device-resident call, delivered
    through torch's pinned allocator (asynchronous copies + one synchronise; videoseal_amd/model.py::_result_buffer) -- also when the
    clip goes through in several chunks, for uint8 clips, and for a second call that reuses the cached host blocks."""
    spec, sd, model = tiny
    imgs = synthetic_frames(6, 64, 80, seed=22)
    dev = imgs.cuda()
    msgs = synthetic_msgs(6, spec.nbits, seed=22)
    model.chunk_size, model.step_size, model.video_mode = 4, 2, "repeat"          # 6 frames = two chunks

    def same(a, b, keys):
        for k in keys:
            assert a[k].device.type == "cpu" and a[k].is_pinned(), k
            assert torch.equal(a[k], b[k].cpu()), k

    for _ in range(2):
        same(model.embed(imgs, msgs, is_video=False), model.embed(dev, msgs, is_video=False), ("imgs_w", "preds_w"))
        same(model.embed(imgs, msgs[:1], is_video=True, lowres_attenuation=True),
             model.embed(dev, msgs[:1], is_video=True, lowres_attenuation=True), ("imgs_w",))
        pa, pb = model.detect(imgs, is_video=True)["preds"], model.detect(dev, is_video=True)["preds"]
        assert pa.device.type == "cpu" and torch.equal(pa, pb.cpu())
    with torch.no_grad():
        masks = torch.ones(6, 1, 64, 80)
        fa, fb = model(imgs, masks, msgs, is_video=False), model(dev, masks.cuda(), msgs, is_video=False)
        for k in ("imgs_w", "preds_w"):                    # (the augmenter draws from the global RNG: compare what does not depend on it)
            assert fa[k].device.type == "cpu" and torch.equal(fa[k], fb[k].cpu()), k
        assert fa["imgs_w"].is_pinned()
    u8 = (imgs * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    ua, ub = model.embed_u8(u8, msgs[:1]), model.embed_u8(u8.cuda(), msgs[:1])
    assert ua["imgs_w"].dtype == torch.uint8 and ua["imgs_w"].is_pinned() and torch.equal(ua["imgs_w"], ub["imgs_w"].cpu())


def test_pageable_results_on_request(tiny, monkeypatch):
    import videoseal_amd.model as M
    spec, sd, model = tiny
    monkeypatch.setattr(M, "_PINNED_RESULTS", False)
    imgs = synthetic_frames(2, 64, 64, seed=23)
    msgs = synthetic_msgs(2, spec.nbits, seed=23)
    a, b = model.embed(imgs, msgs, is_video=False), model.embed(imgs.cuda(), msgs, is_video=False)
    assert not a["imgs_w"].is_pinned() and torch.equal(a["imgs_w"], b["imgs_w"].cpu()) and torch.equal(a["preds_w"], b["preds_w"].cpu())


def test_errors_are_loud(tiny):
    spec, sd, model = tiny
    imgs = synthetic_frames(2, 64, 64, seed=1).cuda()
    with pytest.raises(AssertionError, match="Message should be unique"):
        model.embed(imgs, synthetic_msgs(2, spec.nbits), is_video=True)
    with pytest.raises(NotImplementedError):
        model.detect(imgs, interpolation={"mode": "bicubic", "align_corners": False})
    with pytest.raises(NotImplementedError, match="mixed"):         # OpenCV mask embedder: loud, not silently the full mask
        from videoseal_amd.augmentation import Augmenter
        Augmenter(masks={"kind": None}, augs={"identity": 1}, augs_params={}).train()(imgs, imgs, None)


def test_embed_in_train_mode_uses_batch_statistics():
    """README.md:61-71 never calls .eval(): load() returns a train-mode module whose BatchNorm runs on batch statistics and updates
    its running statistics (SURVEY 8(b) 'Train/eval flag').  Same here (fresh module: the call mutates the buffers)."""
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    model = make_model(spec, sd).train()
    imgs = synthetic_frames(3, 64, 64, seed=1)
    msgs = synthetic_msgs(3, spec.nbits, seed=1)
    out = model.embed(imgs.cuda(), msgs, is_video=False)["imgs_w"].cpu()
    P = (spec.img_size, spec.img_size)
    bn = {}
    with torch.no_grad():
        y = R.rgb2y(sd, imgs)
        delta = R.embedder_forward(sd, spec, y, msgs, bn)
        ref = torch.clamp(spec.scaling_i * imgs + spec.scaling_w * R.jnd_heatmaps(sd, spec, imgs) * delta, 0, 1)
    assert P == tuple(imgs.shape[-2:]) and (out - ref).abs().max() < 1e-4
    new = model.state_dict()
    for k, v in bn.items():
        assert (new[k].cpu().float() - v.float()).abs().max() < 2e-5 * max(1.0, float(v.float().abs().max())), k
    assert (out - R.embed_image(sd, spec, imgs, msgs)["imgs_w"]).abs().max() > 1e-5        # not the eval-mode result


def test_full_size_properties():
    """BASELINE config 2 shape (768x768, batch 8 here): size-independent properties instead of an oracle run.
    * zero watermark strength is the identity; the residual scales linearly with scaling_w
    * video mode with step_size=1 equals image mode with a repeated message
    * detection is per-frame: any permutation of the frames permutes the logits."""
    model = videoseal_amd.build("videoseal_1.0", seed=5).eval().to("cuda")
    imgs = synthetic_frames(8, 768, 768, seed=9).cuda()
    msgs = synthetic_msgs(1, 256, seed=9)
    model.blender.scaling_w = 0.0
    assert torch.equal(model.embed(imgs, msgs, is_video=True)["imgs_w"], imgs)
    model.clamp = False
    model.blender.scaling_w = 0.2
    w1 = model.embed(imgs, msgs, is_video=True)["imgs_w"] - imgs
    model.blender.scaling_w = 0.4
    w2 = model.embed(imgs, msgs, is_video=True)["imgs_w"] - imgs
    assert (w2 - 2 * w1).abs().max() < 1e-6
    model.clamp = True
    model.blender.scaling_w = 0.2
    model.step_size = 1
    v = model.embed(imgs, msgs, is_video=True)["imgs_w"]
    i = model.embed(imgs, msgs.repeat(8, 1), is_video=False)["imgs_w"]
    assert torch.equal(v, i)
    p = model.detect(v, is_video=True)["preds"]
    perm = torch.tensor([3, 1, 7, 0, 2, 6, 5, 4])
    assert (model.detect(v[perm.cuda()], is_video=True)["preds"] - p[perm.cuda()]).abs().max() < 1e-5


def test_edge_shapes(tiny):
    """ragged / degenerate inputs: empty clip, a single frame, frame count not a multiple of step or chunk, frames smaller
    than a JND tile, non-square frames, channel-last strided views; every case against the oracle."""
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 3, 2, "repeat"
    msgs = synthetic_msgs(1, spec.nbits, seed=9)
    empty = torch.zeros(0, 3, 48, 40, device="cuda")
    assert model.embed(empty, msgs, is_video=True)["imgs_w"].shape == (0, 3, 48, 40)
    assert model.detect(empty, is_video=True)["preds"].shape == (0, spec.nbits + 1)
    for n, h, w in [(1, 64, 64), (7, 48, 40), (5, 9, 300), (2, 5, 7), (4, 130, 33)]:
        imgs = synthetic_frames(n, h, w, seed=n + h)
        out = model.embed(imgs.cuda(), msgs, is_video=True, lowres_attenuation=(n % 2 == 0))
        ref = R.embed_video(sd, spec, imgs, msgs, chunk_size=3, step_size=2, lowres_attenuation=(n % 2 == 0))
        assert (out["imgs_w"].cpu() - ref["imgs_w"]).abs().max() < TOL_IMG, (n, h, w)
        p = model.detect(out["imgs_w"], is_video=True)["preds"].cpu()
        assert (p - R.detect(sd, spec, ref["imgs_w"])["preds"]).abs().max() < TOL_LOGIT
    # non-contiguous input (HWC video decoded by a caller and permuted): values must not depend on the memory layout
    hwc = synthetic_frames(4, 64, 80, seed=3).permute(0, 2, 3, 1).contiguous().cuda()
    a = model.embed(hwc.permute(0, 3, 1, 2), msgs, is_video=True)["imgs_w"]
    b = model.embed(hwc.permute(0, 3, 1, 2).contiguous(), msgs, is_video=True)["imgs_w"]
    assert torch.equal(a, b)
    # float / bool messages are accepted like int64 ones (msg_processor.py:92)
    c = model.embed(hwc.permute(0, 3, 1, 2), msgs.float(), is_video=True)["imgs_w"]
    assert torch.equal(a, c)


def test_hipgraph_replay_matches_eager(tiny):
    """VIDEOSEAL_GRAPHS path: the captured launch sequence replays bit-identically, for changing inputs and messages."""
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 8, 2, "repeat"
    outs = {}
    for use in (False, True):
        model.use_graphs = use
        res = []
        for seed in (1, 2, 3):
            imgs = synthetic_frames(16, 96, 80, seed=seed).cuda()
            msgs = synthetic_msgs(1, spec.nbits, seed=seed)
            w = model.embed(imgs, msgs, is_video=True, lowres_attenuation=True)["imgs_w"]
            res.append((w, model.detect(w, is_video=True)["preds"]))
        outs[use] = res
    model.use_graphs = False
    assert len(model._graphs) == 2          # one embed graph + one detect graph, reused for the 3 clips
    for (w0, p0), (w1, p1) in zip(outs[False], outs[True]):
        assert torch.equal(w0, w1) and torch.equal(p0, p1)


@pytest.mark.parametrize("lowres", [True, False])
def test_uint8_rgb24_clip_path(tiny, lowres):
    """inference_streaming.py:23-32,119-125: uint8 RGB24 clip in, uint8 RGB24 out, conversions fused into the HIP kernels.
    Checked against the CPU oracle fed with clip/255 and against our own fp32 entry points (exactly equal before the final
    truncation, so the uint8 results may differ from the ORACLE's by one level where x*255 lands within ~1e-5 of an integer)."""
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 2, 2, "repeat"
    g = torch.Generator().manual_seed(11)
    clip = (synthetic_frames(6, 72, 88, seed=5, kind="smooth") * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # [F,H,W,3]
    msgs = synthetic_msgs(1, spec.nbits, seed=5)
    out = model.embed_u8(clip.cuda(), msgs, lowres_attenuation=lowres)
    assert out["imgs_w"].dtype == torch.uint8 and out["imgs_w"].shape == clip.shape
    x01 = clip.float().permute(0, 3, 1, 2) / 255.0
    # (1) same engine, fp32 entry point: identical arithmetic up to the last conversion -> exactly equal
    w32 = model.embed(x01.cuda(), msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
    assert torch.equal((w32 * 255.0).byte().permute(0, 2, 3, 1), out["imgs_w"])
    # (2) CPU oracle
    ref = R.embed_video(sd, spec, x01, msgs, chunk_size=2, step_size=2, lowres_attenuation=lowres)["imgs_w"]
    ref_u8 = (ref * 255.0).byte().permute(0, 2, 3, 1)
    diff = (ref_u8.int() - out["imgs_w"].cpu().int()).abs()
    assert diff.max().item() <= 1 and (diff != 0).float().mean().item() < 2e-3
    # detect on the uint8 clip == detect on clip/255
    p8 = model.detect_u8(out["imgs_w"])["preds"]
    # (the division runs on the CPU as in inference_streaming.py:120 -- ATen's GPU `tensor / scalar` multiplies by 1/255 instead)
    p32 = model.detect((out["imgs_w"].cpu().float().permute(0, 3, 1, 2) / 255.0).cuda(), is_video=True)["preds"]
    assert torch.equal(p8, p32)
    pref = R.detect(sd, spec, ref_u8.float().permute(0, 3, 1, 2) / 255.0)["preds"]
    sel = (diff.flatten(1).max(1).values == 0)           # frames whose pixels all agree with the oracle: logits must too
    if sel.any():
        assert (p8.cpu()[sel] - pref[sel]).abs().max().item() < TOL_LOGIT
    with pytest.raises(ValueError):
        model.embed_u8(clip.cuda().float(), msgs)
    with pytest.raises(ValueError):
        model.detect_u8(clip.cuda()[..., :2])


def test_wide_chunky_detector_vs_oracle():
    """ChunkySeal's extractor shape at a size the CPU oracle handles: channel counts >= 128 that are not multiples of 32 (activation
    strides padded to whole 32-channel K pairs), stride-2 stem -> 31 x 31 / 15 x 15 feature maps (frames do not align with the GEMM's
    64-row halves -> GRN applied by vs_grn_apply), wave-specialised 1x1 GEMM + K split on the padded layers."""
    s = tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[130, 148, 260, 300], depths=[1, 1, 2, 1], stem_stride=2, hidden=32, nbits=16)
    sd = make_state_dict(s, seed=6)
    model = make_model(s, sd)
    imgs = synthetic_frames(5, 80, 72, seed=12)
    ref = R.detect(sd, s, imgs)["preds"]
    got = model.detect(imgs.cuda(), is_video=True)["preds"].cpu()
    assert (got - ref).abs().max().item() < TOL_LOGIT * max(1.0, ref.abs().max().item())
    assert_decisions(got, ref, what="wide chunky detector vs oracle")


def test_config2_batch_partition_invariance():
    """BASELINE config 2 at its full size (32 x 768 x 768): frames are independent, so the whole batch in one call must equal four
    calls of 8 frames up to fp32 summation order (different batch sizes select different tiles / K splits), in image and video mode."""
    model = videoseal_amd.build("videoseal_1.0", seed=7).eval().to("cuda")
    imgs = synthetic_frames(32, 768, 768, seed=21).cuda()
    msgs = synthetic_msgs(32, 256, seed=21)
    model.chunk_size = 32
    full = model.embed(imgs, msgs, is_video=False)["imgs_w"]
    parts = torch.cat([model.embed(imgs[a:a + 8], msgs[a:a + 8], is_video=False)["imgs_w"] for a in range(0, 32, 8)])
    assert (full - parts).abs().max().item() < 2e-6
    pf = model.detect(full, is_video=True)["preds"]
    pp = torch.cat([model.detect(full[a:a + 8], is_video=True)["preds"] for a in range(0, 32, 8)])
    assert (pf - pp).abs().max().item() < 2e-5
    assert_decisions(pp, pf, what="32 frames vs 4 x 8 frames")
    vfull = model.embed(imgs, msgs[:1], is_video=True)["imgs_w"]           # key frames 0,4,..,28 in one chunk
    model.chunk_size = 2                                                     # 8 frames per chunk
    vparts = model.embed(imgs, msgs[:1], is_video=True)["imgs_w"]
    assert (vfull - vparts).abs().max().item() < 2e-6


@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_model_level_c_api(which, tiny, tinyc):
    """include/videoseal_hip.h vs_model_create / vs_model_embed / vs_model_detect (host code in C++: weight folding + packing +
    launch sequences) against the CPU oracle and against the Python host path on the same inputs."""
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny if which == "tiny" else tinyc
    cm = CModel(cfg_of(spec), sd)
    imgs = synthetic_frames(6, 96, 80, seed=33)
    msgs = synthetic_msgs(1, spec.nbits, seed=33)
    for lowres in (False, True):
        ref = R.embed_video(sd, spec, imgs, msgs, chunk_size=3, step_size=2, lowres_attenuation=lowres)["imgs_w"]
        got = cm.embed(imgs.cuda(), msgs, step=2, video_mode=0, lowres_attenuation=lowres)
        assert (got.cpu() - ref).abs().max().item() < TOL_IMG
        model.chunk_size, model.step_size, model.video_mode = 3, 2, "repeat"
        py = model.embed(imgs.cuda(), msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
        assert (got - py).abs().max().item() < 1e-6            # same kernels; tile choices may differ (tuned vs static)
    ref = R.embed_video(sd, spec, imgs, msgs, chunk_size=3, step_size=2)["imgs_w"]
    lg = cm.detect(ref.cuda()).cpu()
    pref = R.detect(sd, spec, ref)["preds"]
    assert (lg - pref).abs().max().item() < TOL_LOGIT
    assert_decisions(lg, pref, what="model-level C-ABI detect vs oracle")
    # uint8 RGB24 clip in / out == the Python host's embed_u8 / detect_u8
    clip = (imgs * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    model.chunk_size, model.step_size = 3, 2
    u_py = model.embed_u8(clip, msgs, lowres_attenuation=True)["imgs_w"]
    u_c = cm.embed(clip, msgs, step=2, lowres_attenuation=True)
    assert u_c.dtype == torch.uint8 and (u_c.int() - u_py.int()).abs().max().item() <= 1 and (u_c != u_py).float().mean().item() < 1e-3
    assert (cm.detect(u_py) - model.detect_u8(u_py)["preds"]).abs().max().item() < 1e-4
    # image mode: one message per frame, preds_w returned
    m6 = synthetic_msgs(6, spec.nbits, seed=34)
    out, pw = cm.embed(imgs.cuda(), m6, step=1, want_preds_w=True)
    r = R.embed_image(sd, spec, imgs, m6)
    assert (out.cpu() - r["imgs_w"]).abs().max().item() < TOL_IMG and (pw.cpu() - r["preds_w"]).abs().max().item() < TOL_IMG


def test_model_level_c_api_vs10(vs10):
    """the released VideoSeal 1.0 architecture through the model-level C-ABI vs the Python host path (same kernels)."""
    from videoseal_amd.capi import CModel
    spec, sd, model = vs10
    cm = CModel(cfg_of(spec), sd)
    imgs = synthetic_frames(4, 320, 288, seed=41).cuda()
    msgs = synthetic_msgs(1, spec.nbits, seed=41)
    model.chunk_size, model.step_size, model.video_mode = 8, 2, "repeat"
    py = model.embed(imgs, msgs, is_video=True, lowres_attenuation=True)["imgs_w"]
    got = cm.embed(imgs, msgs, step=2, lowres_attenuation=True)
    assert (got - py).abs().max().item() < 1e-6
    assert (cm.detect(got) - model.detect(py, is_video=True)["preds"]).abs().max().item() < 1e-4


@pytest.mark.parametrize("which", ["tiny", "tinyc", "vs10"])
def test_model_level_c_api_equals_the_engine_bit_for_bit_without_the_tuner(which, monkeypatch):
    """With the tuner off both hosts take every K-slice / tile / GRN-fold decision of a dense layer from vs_conv_plan and
    vs_cnx_stage_plan (csrc/conv_plan.hip): embed and detect are torch.equal (measured equal on these cases before the rules moved into the
    library as well).  vs10 at 4 frames, step 2, is the case in which both K-slice rules fire (stage-3 GEMMs, bottleneck convs of two key
    frames).  It runs with VIDEOSEAL_PLANES_SPLITK=0: the K-sliced form of the bottleneck's planes chain (< 200 tiles, engine._planes_split)
    exists in the Python engine only -- the C host keeps the wave-specialised 3x3 kernel there, measured 6e-8 apart --, and with it off both
    hosts run these convs by the rule under test."""
    from videoseal_amd.capi import CModel
    monkeypatch.setenv("VIDEOSEAL_AUTOTUNE", "0")
    monkeypatch.setenv("VIDEOSEAL_PLANES_SPLITK", "0")
    spec, seed, (n, h, w), chunk = {"tiny": (tiny_spec(), 3, (6, 96, 80), 3),
                                    "tinyc": (tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16), 4, (6, 96, 80), 3),
                                    "vs10": (spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml")), 0, (4, 320, 288), 8)}[which]
    sd = make_state_dict(spec, seed=seed)
    model, cm = make_model(spec, sd), CModel(cfg_of(spec), sd)
    imgs = synthetic_frames(n, h, w, seed=41).cuda()
    msgs = synthetic_msgs(1, spec.nbits, seed=41)
    model.chunk_size, model.step_size, model.video_mode = chunk, 2, "repeat"
    for lowres in (False, True):
        py = model.embed(imgs, msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
        assert torch.equal(cm.embed(imgs, msgs, step=2, video_mode=0, lowres_attenuation=lowres), py), (which, lowres)
    assert torch.equal(cm.detect(py), model.detect(py, is_video=True)["preds"])
    m_img = synthetic_msgs(n, spec.nbits, seed=34)
    assert torch.equal(cm.embed(imgs, m_img, step=1), model.embed(imgs, m_img, is_video=False)["imgs_w"])


def test_streaming_overlap_equals_sequential(tiny):
    """videoseal_amd/streaming.py: detect(chunk i) overlapped with embed(chunk i+1) on two HIP streams returns exactly what the
    sequential 16-frame calls return (fp32 and uint8 clips), chunk after chunk."""
    from videoseal_amd.streaming import embed_detect_chunks
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 4, 4, "repeat"
    frames = synthetic_frames(40, 96, 80, seed=51).cuda()
    msgs = synthetic_msgs(1, spec.nbits, seed=51)
    seq_w, ovl_w = [], []
    a = embed_detect_chunks(model, frames, msgs, chunk=16, overlap=False, sink=lambda i, w: seq_w.append(w.clone()))
    for _ in range(3):          # repeated: a stream race would not be deterministic
        ovl_w.clear()
        b = embed_detect_chunks(model, frames, msgs, chunk=16, overlap=True, sink=lambda i, w: ovl_w.append(w.clone()))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert all(torch.equal(x, y) for x, y in zip(seq_w, ovl_w))
    clip = (frames * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(embed_detect_chunks(model, clip, msgs, overlap=False), embed_detect_chunks(model, clip, msgs, overlap=True))
    ref = R.detect(sd, spec, R.embed_video(sd, spec, frames[:16].cpu(), msgs, chunk_size=4, step_size=4, lowres_attenuation=True)["imgs_w"])["preds"]
    assert (a[:16].cpu() - ref).abs().max().item() < TOL_LOGIT


@pytest.mark.parametrize("mode", ["repeat", "alternate", "interpolate"])
def test_streaming_key_frame_groups_equal_the_per_chunk_calls(tiny, mode):
    """streaming.embed_detect_chunks with the key frames of several chunks in ONE U-Net pass (group > 1) against the literal per-chunk calls
    (group = 1 = inference_streaming.py:83-164), every video mode (videoseal.py:303-344: 'interpolate' treats the last key frame of each CHUNK
    specially, so the watermark must still be expanded chunk by chunk), ragged last chunk, fp32 and uint8 clips.  Not bit-equal by
    construction: whether a dense layer splits K is a function of the batch shape -> fp32 summation order."""
    from videoseal_amd.streaming import default_group, embed_detect_chunks
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 4, 4, mode
    try:
        frames = synthetic_frames(44, 96, 80, seed=52).cuda()
        msgs = synthetic_msgs(1, spec.nbits, seed=52)
        assert default_group(16, 4) == 8 and default_group(16, 5) == 1 and default_group(8, 4) == 16
        one_w, grp_w = [], []
        a = embed_detect_chunks(model, frames, msgs, chunk=16, overlap=False, group=1, sink=lambda i, w: one_w.append((i, w.clone())))
        b = embed_detect_chunks(model, frames, msgs, chunk=16, overlap=True, group=2, sink=lambda i, w: grp_w.append((i, w.clone())))
        torch.cuda.synchronize()
        assert [i for i, _ in one_w] == [i for i, _ in grp_w] == [0, 16, 32]
        assert [w.shape[0] for _, w in grp_w] == [16, 16, 12]
        for (_, x), (_, y) in zip(one_w, grp_w):
            assert (x - y).abs().max().item() < 1e-5
        assert (a - b).abs().max().item() < 1e-3
        # decisions of the grouped path = decisions of the per-chunk calls (per frame and aggregated)
        assert_decisions(b, a, what=f"grouped vs per-chunk streaming ({mode})", min_sure=0.99)
        ma, mb = a[:, 1:].mean(dim=0), b[:, 1:].mean(dim=0)
        assert torch.equal((ma > 0)[ma.abs() > 1e-5], (mb > 0)[ma.abs() > 1e-5])
        # the per-chunk expansion matters: one tail launch over the whole group differs in 'interpolate' mode (frames 13-15 of a chunk)
        if mode == "interpolate":
            model.chunk_size = 8                       # embed() itself with 32-frame chunks: a different (legal) chunking of the clip
            whole = model.embed(frames[:32], msgs, is_video=True, lowres_attenuation=True)["imgs_w"]
            assert (whole[13:16] - one_w[0][1][13:16]).abs().max().item() > 1e-6
            assert (whole[:13] - one_w[0][1][:13]).abs().max().item() < 1e-5
        clip = (frames * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        model.chunk_size = 4
        u1, u2 = [], []
        c = embed_detect_chunks(model, clip, msgs, chunk=16, overlap=False, group=1, sink=lambda i, w: u1.append(w.clone()))
        d = embed_detect_chunks(model, clip, msgs, chunk=16, overlap=True, sink=lambda i, w: u2.append(w.clone()))
        torch.cuda.synchronize()
        for x, y in zip(u1, u2):             # uint8 frames: a 1e-7 difference may cross a rounding boundary of (x * 255).byte() in rare pixels
            assert (x.int() - y.int()).abs().max().item() <= 1
            assert (x != y).float().mean().item() < 1e-4
        assert (c - d).abs().max().item() < 5e-3
        assert torch.equal((c > 0)[c.abs() > 1e-2], (d > 0)[c.abs() > 1e-2])
        mc, md = c[:, 1:].mean(dim=0), d[:, 1:].mean(dim=0)
        assert torch.equal((mc > 0)[mc.abs() > 1e-3], (md > 0)[mc.abs() > 1e-3])
        with pytest.raises(ValueError):
            embed_detect_chunks(model, frames, msgs, chunk=10, group=2)
    finally:
        model.video_mode = "repeat"


def test_configs3_stated_size_streaming_equals_the_reference_run_of_inference_streaming(vs10):
    """BASELINE configs[3] at its STATED size and in the form bench.py's stream leg times: VideoSeal 1.0, a 128-frame 768 x 768 clip = 8
    chunks of 16, streaming.embed_detect_chunks with its defaults (key frames of 8 chunks in one U-Net pass, extractor on 128 frames per
    pass, detect overlapped on a second stream) against tests/golden/vs10_stream_768.npz -- the unmodified reference called chunk by chunk
    through inference_streaming.py's own embed_video_clip / detect_video_clip (make_golden_stream.py).  fp32 clip: watermarked frames, PSNR,
    per-frame logits, and the aggregated decision (`soft_msgs.mean(0) > 0`, inference_streaming.py:162-163) IDENTICAL; uint8 RGB24 clip (the
    script's data format): bytes within one grey level in < 1e-4 of the pixels, soft bits, identical decision; and the literal per-chunk
    calls (group = 1) of the same clip."""
    from videoseal_amd.streaming import default_group, embed_detect_chunks
    spec, sd, model = vs10
    g = load_golden("vs10_stream_768")
    meta = g["meta"]
    assert (meta["n"], meta["h"], meta["chunk"]) == (128, 768, 16)
    model.chunk_size, model.step_size, model.video_mode = meta["model_chunk_size"], meta["step"], "repeat"
    frames = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"])
    msgs = synthetic_msgs(1, spec.nbits, seed=meta["seed"])
    assert torch.equal(msgs, torch.from_numpy(g["msgs"]))
    fr = frames.cuda()
    assert default_group(16, model.step_size, fr[0].numel() * 4) == 8
    gold, agg_gold = torch.from_numpy(g["preds"]), torch.from_numpy(g["agg_f32"])
    sure = agg_gold.abs() > 1e-5                  # (a mean logit closer to zero than the fp32 noise of a 128-frame mean has no defined sign)
    for group in (None, 1):                       # the grouped default (what the bench leg runs) and the script's literal per-chunk calls
        got_w = []
        preds = embed_detect_chunks(model, fr, msgs, chunk=16, lowres_attenuation=True, group=group, sink=lambda i, w: got_w.append(w.clone())).cpu()
        torch.cuda.synchronize()
        w = torch.cat(got_w)
        del got_w
        check_sub(g, "imgs_w", w, TOL_IMG, f"stream group={group} ")
        assert abs(psnr_np(w.cpu(), frames) - meta["psnr"]) < 1e-3
        del w
        assert preds.shape == gold.shape and (preds - gold).abs().max().item() < TOL_LOGIT
        assert_decisions(preds, gold, what=f"stream 128 x 768^2 group={group}")
        agg = preds[:, 1:].mean(dim=0)
        assert (agg - agg_gold).abs().max().item() < 1e-4
        assert torch.equal((agg > 0)[sure], (agg_gold > 0)[sure])
        assert sure.all() and float(((agg > 0) == (msgs[0] > 0.5)).float().mean()) == meta["bit_acc_f32"]      # (min |mean logit| of the fixture: 2.4e-3)
    # uint8 RGB24 in and out, as the script moves frames
    clip = (frames * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    del fr
    got_b = []
    soft = embed_detect_chunks(model, clip, msgs, chunk=16, lowres_attenuation=True, sink=lambda i, w: got_b.append(w.clone()))[:, 1:].cpu()
    torch.cuda.synchronize()
    wb = torch.cat(got_b).cpu()
    stride = int(g["w_u8.stats"][2])
    assert wb.numel() == int(g["w_u8.stats"][1])
    diff = (wb.flatten()[::stride].int() - torch.from_numpy(g["w_u8.sub"]).int()).abs()
    assert diff.max().item() <= 1 and (diff != 0).float().mean().item() < 1e-4
    assert abs(float(wb.double().sum()) - g["w_u8.stats"][0]) < 1e-6 * wb.numel()
    soft_gold, agg_u8 = torch.from_numpy(g["soft_u8"]), torch.from_numpy(g["agg_u8"])
    assert (soft - soft_gold).abs().max().item() < 5 * TOL_LOGIT          # a byte that rounds the other way moves a logit by ~1e-4
    sure8 = agg_u8.abs() > 1e-4
    assert torch.equal((soft.mean(dim=0) > 0)[sure8], (agg_u8 > 0)[sure8]) and sure8.float().mean() > 0.98


def test_a_one_group_shard_overlaps_detect_inside_the_group(vs10, monkeypatch):
    """configs[3] on 8 GPUs gives every rank 128 frames = ONE default group (8 chunks' key frames per U-Net pass): there is no "next embed" to
    run the extractor under, so the overlap can be cut inside the group -- with det_batch = 32 the extractor starts on the first 32 watermarked
    frames while the tail of the others is still being issued (streaming.py, `embed_group(on_tail=...)`; the DEFAULT since the same round is one
    extractor pass over the whole 128-frame group, which measured 14 % faster than four passes of 32 -- this test pins the finer cut).  (i) frames and logits BIT-EQUAL to the whole-group
    hand-over (same U-Net batch, same extractor batches), for 'repeat' (one tail launch per 32 frames) and 'interpolate' (per chunk);
    (ii) wall time of the 128-frame shard printed next to the whole-group hand-over and embed-only + detect-only (sanity bounds only)."""
    import time
    from videoseal_amd.streaming import embed_detect_chunks
    spec, sd, model = vs10
    frames = synthetic_frames(128, 768, 768, seed=83).cuda()
    msgs = synthetic_msgs(1, spec.nbits, seed=83)
    model.chunk_size, model.step_size = 32, 4
    try:
        for mode in ("repeat", "interpolate"):
            model.video_mode = mode
            res = {}
            for fine in ("1", "0"):
                monkeypatch.setenv("VIDEOSEAL_STREAM_FINE", fine)
                got = []
                p = embed_detect_chunks(model, frames, msgs, chunk=16, lowres_attenuation=True, det_batch=32, sink=lambda i, w: got.append((i, w.clone())))
                torch.cuda.synchronize()
                assert [i for i, _ in got] == list(range(0, 128, 16))
                res[fine] = (p.clone(), torch.cat([w for _, w in got]))
            assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1]), mode
        model.video_mode = "repeat"

        def wall(fn, n=5):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n
        t = {}
        for fine in ("1", "0"):
            monkeypatch.setenv("VIDEOSEAL_STREAM_FINE", fine)
            t[fine] = wall(lambda: embed_detect_chunks(model, frames, msgs, chunk=16, lowres_attenuation=True, det_batch=32))
        w = model.embed_group(frames, msgs, 16, lowres_attenuation=True)
        t_emb = wall(lambda: model.embed_group(frames, msgs, 16, lowres_attenuation=True))
        t_det = wall(lambda: model.detect(w, is_video=True))
        print(f"128-frame shard: fine {t['1'] * 1e3:.2f} ms, whole-group {t['0'] * 1e3:.2f} ms, embed-only {t_emb * 1e3:.2f} + detect-only {t_det * 1e3:.2f} ms")
        # (wall-clock sanity bounds only -- the measured ratios are 0.99 and 1.01 (profiles/r06b), but a timing assertion must not be what stops a
        # `pytest -x` run on a box with a noisy neighbour, or in the --no-caching-allocator mode where every tensor is a hipMalloc)
        assert t["1"] <= 1.5 * t["0"]
        assert t["1"] <= 1.5 * (t_emb + t_det)
    finally:
        model.video_mode = "repeat"


def test_chunkyseal_released_size_detector_vs_oracle():
    """BASELINE config 5 architecture at its released size (ConvNeXt dims 362/724/1448/2896, depths 3/3/27/3, 774 M extractor
    parameters, 1024 bits, stride-2 stem -> 127/63/31/15 feature maps): HIP detect vs the CPU oracle on two frames."""
    spec = spec_from_card(os.path.join(CARDS, "chunkyseal.yaml"))
    sd = make_state_dict(spec, seed=2)
    model = make_model(spec, sd)
    imgs = synthetic_frames(2, 512, 480, seed=7)
    ref = R.detect(sd, spec, imgs)["preds"]
    got = model.detect(imgs.cuda(), is_video=True)["preds"].cpu()
    assert (got - ref).abs().max().item() < 1e-4
    assert_decisions(got, ref, what="ChunkySeal released size vs oracle")
    # ... and against the UNMODIFIED reference at configs[4]'s frame size: `build_extractor` of the released card + `Wam.detect` on 2 frames
    # of 1024 x 1024 (tests/golden/make_golden_cfg1.py --chunky; the 4:1 antialiased resize of wam.py:221-225 included)
    g = load_golden("chunky_detect_1024x2")
    meta = g["meta"]
    assert meta["sd_seed"] == 2 and (meta["h"], meta["w"]) == (1024, 1024)
    big = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"]).cuda()
    gold = torch.from_numpy(g["preds"])
    for is_video in (False, True):
        p = model.detect(big, is_video=is_video)["preds"].cpu()
        assert p.shape == gold.shape == (2, 1025)
        assert (p - gold).abs().max().item() < 1e-4, float((p - gold).abs().max())
        assert_decisions(p, gold, what="ChunkySeal released size, 1024 x 1024, vs the reference golden")
    del model
    torch.cuda.empty_cache()


def test_vs10_768_vs_oracle(vs10):
    """BASELINE config 2 frame size (768 x 768) directly against the CPU oracle: image mode (full-res JND) and video mode (key frames
    every 2, low-res JND), watermarked frames, PSNR and logits."""
    spec, sd, model = vs10
    imgs = synthetic_frames(4, 768, 768, seed=61)
    m4, m1 = synthetic_msgs(4, spec.nbits, seed=61), synthetic_msgs(1, spec.nbits, seed=62)
    model.chunk_size, model.step_size, model.video_mode = 8, 2, "repeat"
    for got, ref in ((model.embed(imgs.cuda(), m4, is_video=False)["imgs_w"].cpu(), R.embed_image(sd, spec, imgs, m4)["imgs_w"]),
                     (model.embed(imgs.cuda(), m1, is_video=True, lowres_attenuation=True)["imgs_w"].cpu(),
                      R.embed_video(sd, spec, imgs, m1, chunk_size=8, step_size=2, lowres_attenuation=True)["imgs_w"])):
        assert (got - ref).abs().max().item() < TOL_IMG
        assert abs(R.psnr(got, imgs).mean().item() - R.psnr(ref, imgs).mean().item()) < 1e-3
        p, pr = model.detect(got.cuda(), is_video=True)["preds"].cpu(), R.detect(sd, spec, ref)["preds"]
        assert (p - pr).abs().max().item() < TOL_LOGIT
        assert_decisions(p, pr, what="768 x 768 vs oracle")


def test_fused_convnext_blocks_match_the_unfused_path_and_the_oracle(vs10):
    """stage 0 / 1 blocks of the extractor with h kept on chip (csrc/convnext_fused.hip: transposed pwconv1 whose accumulator layout is pwconv2's
    A operand, GRN by a statistics pass) against the per-layer GEMM path and the CPU oracle"""
    spec, sd, model = vs10
    imgs = synthetic_frames(3, 256, 256, seed=77)
    eng = model._engine()
    if eng.arith_net["X"] != 2 or not eng.fused_blocks:
        pytest.skip("2 x f16 arithmetic with fused blocks only")
    calls = []
    orig = eng.lib.vs_cnx_block

    class Spy:
        def __call__(self, *a):
            calls.append(a[5])
            return orig(*a)
    try:
        eng.lib.vs_cnx_block = Spy()
        p1 = model.detect(imgs.cuda(), is_video=False)["preds"].cpu()
    finally:
        eng.lib.vs_cnx_block = orig
    assert calls.count(1) == 6 and calls.count(0) == 6, "six blocks (stages 0 and 1), one statistics and one apply launch each"
    eng.fused_blocks = False
    try:
        p0 = model.detect(imgs.cuda(), is_video=False)["preds"].cpu()
    finally:
        eng.fused_blocks = True
    ref = R.detect(sd, spec, imgs)["preds"]
    assert (p1 - p0).abs().max() < 2e-5, float((p1 - p0).abs().max())
    assert (p1 - ref).abs().max() < 1e-4 and (p0 - ref).abs().max() < 1e-4


def test_pipelined_convnext_block_kernel_equals_the_serial_one_bit_for_bit(vs10):
    """csrc/convnext_fused.hip: cnx_pipe_kernel (pwconv1 of block hb + 1 issued under the GELU / GRN arithmetic of block hb, separate rings for
    W1 and W2) multiplies the same products in the same order as cnx_block_kernel (stats bit 1 selects it): identical logits (both channel counts, 32- and 64-pixel tiles per wave)"""
    spec, sd, model = vs10
    imgs = synthetic_frames(4, 256, 256, seed=78).cuda()
    eng = model._engine()
    if eng.arith_net["X"] != 2 or not eng.fused_blocks:
        pytest.skip("2 x f16 arithmetic with fused blocks only")
    orig = eng.lib.vs_cnx_block
    p_pipe = model.detect(imgs, is_video=False)["preds"].clone()

    class Serial:
        def __call__(self, *a):
            a = list(a)
            a[5] = int(a[5]) | 2
            return orig(*a)
    try:
        eng.lib.vs_cnx_block = Serial()
        p_serial = model.detect(imgs, is_video=False)["preds"].clone()
    finally:
        eng.lib.vs_cnx_block = orig
    assert torch.equal(p_pipe, p_serial), float((p_pipe - p_serial).abs().max())


def test_convnext_blocks_whose_frames_straddle_an_apply_workgroup_take_the_per_layer_path(vs10):
    """96 x 96 frames: stage 0 has 576 pixels per frame, no multiple of the 128 pixels an apply workgroup of csrc/convnext_fused.hip shares one GRN
    scale row for (2304 rows and HW % 64 == 0: the older gate accepted it and part of the waves read the neighbouring frame's scale).
    vs_cnx_block_supported refuses it, the engine's gate calls that function: no fused launch, and the logits are the unfused path's bits"""
    spec, sd, model = vs10
    imgs = synthetic_frames(4, 96, 96, seed=79).cuda()
    eng = model._engine()
    if eng.arith_net["X"] != 2 or not eng.fused_blocks:
        pytest.skip("2 x f16 arithmetic with fused blocks only")
    assert eng.lib.vs_cnx_block_supported(96, 4 * 576, 576) == 0 and eng.lib.vs_cnx_block_supported(96, 4 * 4096, 4096) == 1
    calls = []
    orig = eng.lib.vs_cnx_block

    class Spy:
        def __call__(self, *a):
            calls.append(a[5])
            return orig(*a)
    try:
        eng.lib.vs_cnx_block = Spy()
        p1 = model.detector(imgs).clone()
    finally:
        eng.lib.vs_cnx_block = orig
    assert not calls
    eng.fused_blocks = False
    try:
        p0 = model.detector(imgs).clone()
    finally:
        eng.fused_blocks = True
    assert torch.isfinite(p1).all() and torch.equal(p1, p0)
    with torch.no_grad():
        ref = R.extractor_forward(sd, spec, imgs.cpu())
    assert (p1.cpu() - ref).abs().max() < 1e-4
