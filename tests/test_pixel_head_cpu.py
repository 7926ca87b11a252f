"""Host side of the pixel-wise extractor head, without a GPU: the fixture's self-checks, the builder cases (names and shapes of every
`pixel_decoder.*` entry against what the reference's own `build_extractor` made, recorded in tests/golden/pixel_head_ops.npz; the refusals)
and the torch side of the bit metrics on 4-D predictions against the reference's evals/metrics.py values."""
import copy

import numpy as np
import pytest
import torch

from tests import _pixel_head_util as U
from tests._util import load_golden
from videoseal_amd import metrics as M
from videoseal_amd.builders import build_extractor, load_config
from videoseal_amd.layout import cfg_from_card, head_widths

G = load_golden("pixel_head_ops")
META = G["meta"]


def test_fixture_is_consistent_with_the_seeded_inputs():
    sums = META["sums"]
    for case in [(C, Co, f, H, W) for (C, Co, f) in U.STAGES for (H, W) in U.LATENTS]:
        assert np.allclose(U.checksum(*U.stage_tensors(*case)), sums[U.stage_name(*case)], rtol=1e-9, atol=1e-9)
    for (K, sig, hw) in U.LINEAR:
        assert np.allclose(U.checksum(*U.linear_tensors(K, hw)), sums[U.linear_name(K, sig, hw)], rtol=1e-9, atol=1e-9)
    for sk in U.LOSS_SHAPES:
        for kind in U.LOSS_MASKS:
            p, m, b = U.loss_tensors(sk, kind)
            assert np.allclose(U.checksum(p, m, b.float()), sums[f"loss_{sk}_{kind}"], rtol=1e-9, atol=1e-9)
            assert int((m != 0).sum()) % p.shape[0] == 0
            if kind == "none":
                assert not m.any() and np.isnan(G[f"loss_{sk}_none.loss"][1])
            if kind == "one_frame":
                assert not m[0].any() and m[1].any()
            if kind == "frac":
                assert ((m > 0) & (m < 1)).any() and (m == 0).any()


def test_fixture_arrays_and_yardsticks():
    e = META["e"]
    keys = [k for k in G if k.endswith(".stats")]
    assert len(keys) == 56          # 16 stage outputs + raw, 4 gradients, 6 x 4 linear, 2 chains, 10 loss gradients
    for k in keys:
        name, st = k[:-len(".stats")], G[k]
        n, stride = int(st[2]), int(st[3])
        assert G[name].dtype == np.float64 and G[name].size == (n + stride - 1) // stride and stride % 2 == 1
        assert name in e and 0 <= e[name] < 1e-3, (name, e.get(name))
        if stride == 1:
            assert abs(G[name].sum() - st[0]) <= 1e-9 * max(1.0, abs(st[0]))
    # every stage and latent of the operator test, the one stage with gradients, every linear case
    for (C, Co, f) in U.STAGES:
        for (H, W) in U.LATENTS:
            assert G[U.stage_name(C, Co, f, H, W) + ".out.stats"][2] == U.B * Co * f * H * f * W
    assert all(U.stage_name(*U.BWD_STAGE) + s in G for s in (".dx", ".dw", ".dlw", ".dlb"))


@pytest.mark.parametrize("name", ["convnext_tiny_pw", "convnext_base_pw", "sam_small_pw"])
def test_builder_makes_the_reference_names_and_shapes(name):
    cfg = load_config("extractor")[name]
    ext = build_extractor(name, cfg, 256, 96)
    got = {k: list(v.shape) for k, v in ext.state_dict().items() if k.startswith("pixel_decoder.")}
    assert got == META["heads"][name]
    c = ext.cfg
    assert c.head_pixelwise and not c.head_sigmoid and c.head_stages == list(cfg["pixel_decoder"]["upscale_stages"])
    widths = {"convnext_tiny_pw": [192, 48, 24], "convnext_base_pw": [256, 64, 32], "sam_small_pw": [96, 48, 24]}[name]
    assert head_widths(c) == widths
    assert got["pixel_decoder.linear.weight"] == [97, widths[-1], 1, 1]


def test_builder_accepts_chains_without_the_pixelwise_layer_and_sigmoid():
    base = {"encoder": {"depths": [1, 1, 1, 1], "dims": [8, 16, 32, 64]}, "pixel_decoder": {"upscale_stages": [4, 2, 1], "pixelwise": False,
                                                                                          "sigmoid_output": True}}
    ext = build_extractor("convnext_tiny", copy.deepcopy(base), 64, 16)
    sd = ext.state_dict()
    assert sd["pixel_decoder.output_upscaling.0.upsample_block.2.weight"].shape == (16, 64, 3, 3)
    assert sd["pixel_decoder.output_upscaling.1.upsample_block.2.weight"].shape == (8, 16, 3, 3)
    assert sd["pixel_decoder.output_upscaling.2.upsample_block.2.weight"].shape == (8, 8, 3, 3)
    assert sd["pixel_decoder.output_upscaling.2.upsample_block.3.bias"].shape == (8,)
    assert sd["pixel_decoder.linear.weight"].shape == (17, 8) and ext.cfg.head_sigmoid and not ext.cfg.head_pixelwise
    # the per-frame head of the released cards is what it was: any width, [1] / False
    plain = build_extractor("convnext_tiny", {"encoder": {"depths": [1, 1, 1, 1], "dims": [8, 16, 24, 30]}, "pixel_decoder": {}}, 64, 16)
    assert plain.cfg.head_stages == [1] and plain.pixel_decoder.linear.weight.shape == (17, 30)


@pytest.mark.parametrize("pd,why", [
    ({"upscale_stages": [4, 4, 2], "pixelwise": True, "upscale_type": "nearest"}, "nearest"),
    ({"upscale_stages": [4, 4, 2], "pixelwise": True, "upscale_type": "conv"}, "conv"),
    ({"upscale_stages": [4, 4, 2], "pixelwise": True, "upscale_type": "pixelshuffle"}, "pixelshuffle"),
    ({"upscale_stages": [8, 2], "pixelwise": True}, "factor 8"),
    ({"upscale_stages": [3], "pixelwise": True}, "factor 3"),
    ({"upscale_stages": [4, 4, 4], "pixelwise": True}, "multiple of 4"),          # 128 -> 32 / 8 / 2
    ({"upscale_stages": [1], "pixelwise": True, "embed": 30}, "multiple of 4"),
    ({"upscale_stages": [1], "pixelwise": True}, "at most 64"),                  # the per-pixel linear kernel on 128 channels
    ({"upscale_stages": [1], "sigmoid_output": True}, "at most 64"),            # pooled, then the linear kernel with its sigmoid on 128 channels
])
def test_builder_refusals_give_the_reason(pd, why):
    pd = dict(pd)
    last = pd.pop("embed", 128)
    with pytest.raises(NotImplementedError, match=why):
        build_extractor("convnext_tiny", {"encoder": {"depths": [1, 1, 1, 1], "dims": [8, 16, 24, last]}, "pixel_decoder": pd}, 64, 16)
    sam = {"encoder": {"img_size": 64, "embed_dim": 32, "out_chans": last, "depth": 1, "num_heads": 2, "patch_size": 16, "global_attn_indexes": [0],
                       "window_size": 0, "mlp_ratio": 2, "qkv_bias": True, "use_rel_pos": False}, "pixel_decoder": dict(pd, embed_dim=last)}
    with pytest.raises(NotImplementedError, match=why):
        build_extractor("sam_tiny", sam, 64, 16)


def test_card_with_a_pixelwise_head():
    from videoseal_amd.layout import load_card
    import glob
    import os
    cards = sorted(glob.glob(os.path.join(os.path.dirname(M.__file__), "cards", "*.yaml")))
    card = next(c for c in map(load_card, cards) if str(c["extractor"]["model"]).startswith("convnext") and cfg_from_card(c).dims[-1] == 768)
    card = copy.deepcopy(card)
    card["extractor"]["params"]["pixel_decoder"].update(upscale_stages=[4, 4, 2], pixelwise=True)
    c = cfg_from_card(card)
    assert c.head_stages == [4, 4, 2] and c.head_pixelwise and head_widths(c)[-1] == c.dims[-1] // 32
    card["extractor"]["params"]["pixel_decoder"]["upscale_type"] = "pixelshuffle"
    with pytest.raises(NotImplementedError, match="pixelshuffle"):
        cfg_from_card(card)


def test_torch_side_of_the_bit_metrics_on_4d_predictions():
    Bn, K, H, W = 3, 7, 10, 12
    logits = U.vote_logits(Bn, K, H, W, seed=21)
    bits = torch.randint(0, 2, (Bn, K), generator=torch.Generator().manual_seed(22))
    mask = torch.zeros(Bn, 1, H, W)
    mask[:, :, 2:7, 3:11] = 1.0
    assert np.allclose(U.checksum(logits, bits.float(), mask), META["sums"]["vote"], rtol=1e-9, atol=1e-9)
    for thr in (0.0, 0.25):
        assert float((logits - thr).abs().min()) > 1e-3
        for m, tag in ((None, ""), (mask, "_masked")):
            M.LAST_VOTE_BACKEND = None
            assert np.array_equal(M.bit_accuracy(logits, bits, m, thr).double().numpy(), G[f"vote_acc{tag}_thr{thr}"])
            assert M.LAST_VOTE_BACKEND == "torch"
            assert np.array_equal(M.bit_accuracy_1msg(logits, bits, m, thr).double().numpy(), G[f"vote_1msg{tag}_thr{thr}"])
    flat = torch.randn(4, 16)
    M.LAST_VOTE_BACKEND = None
    M.bit_accuracy(flat, flat > 0)
    assert M.LAST_VOTE_BACKEND is None          # rows of logits never were a vote
