#!/usr/bin/env python
"""Golden values for the pixel-wise extractor head (csrc/pixel_head.hip, videoseal_amd/pixel_head.py) from the UNMODIFIED reference, run on
the CPU next to a reference checkout with the stub-import recipe of make_golden.py / make_golden_bwd.py:

    python tests/golden/make_golden_pixel_head.py

Writes tests/golden/pixel_head_ops.npz and tests/golden/pixel_head_model.npz (whole tiny models: see model_cases).  Inputs come from seeds (tests/_pixel_head_util.py, shared with the tests); the fixture stores a
checksum of them, not the tensors.  Every case is run in float64 and in fp32: the fixture keeps the float64 result and, in meta["e"], what the
reference's own fp32 run loses against it (largest absolute difference per tensor) -- the yardstick of tests/test_gpu_pixel_head.py.

  st<C>_<Co>_x<f>_<H>x<W>.out   the reference's `Upsample('bilinear', C, Co, f, nn.GELU)` (modules/common.py:45-52) on a B x C x H x W latent
  ... .raw                      the Conv3x3 output in front of its LayerNorm (what the raw mode of the gather kernel stores)
  ... .dx / .dw / .dlw / .dlb   d <out, dout> / d input, conv weight, LayerNorm weight and bias (one stage: _pixel_head_util.BWD_STAGE)
  lin<K>_<sig|raw>_<H>x<W>.out  `PixelDecoder.linear` (Conv2d 1x1) and the optional sigmoid of PixelDecoder.forward, with .dx / .dw / .db
  chain_<H>x<W>.out             a whole `PixelDecoder(embed_dim=128, upscale_stages=[4, 4, 2], pixelwise=True, nbits=16)` with a strict load
  loss_<shape>_<mask>           `VideosealLoss(optimizer_idx=0)` with detect and decode weights on pixel-wise logits: [detect, decode] of its
                                log and d(total) / d preds; the decode logits are divided by the case's temperature first (train.py:628)
  vote_*                        evals/metrics.py `bit_accuracy` / `bit_accuracy_1msg` on 4-D logits with and without a mask
  meta["heads"]                 names and shapes of every `pixel_decoder.*` entry of convnext_tiny_pw, convnext_base_pw and sam_small_pw as the
                                reference's `build_extractor` makes them from its configs/extractor.yaml
Tensors beyond 4 096 elements are stored as a strided sub-sample of the flattened tensor (an odd stride that keeps at most 4 096 values) plus sum
and sum of squares."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import yaml
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                   # noqa: E402
import make_golden_bwd as MB                               # noqa: E402
import make_golden_fwd as MF                               # noqa: E402

from tests import _pixel_head_util as U                    # noqa: E402

FULL_LIMIT = 4096


def store(d, e, key, t64, t32):
    t64 = t64.detach().double()
    e[key] = float((t32.detach().double() - t64).abs().max())
    flat = t64.flatten()
    stride = 1 if flat.numel() <= FULL_LIMIT else (flat.numel() // FULL_LIMIT + 1) | 1       # odd: never in step with an even row length
    d[key] = flat[::stride].numpy()
    d[key + ".stats"] = np.array([float(flat.sum()), float((flat ** 2).sum()), flat.numel(), stride], dtype=np.float64)


def load_metrics():
    if "pytorch_msssim" not in sys.modules and importlib.util.find_spec("pytorch_msssim") is None:
        sys.modules["pytorch_msssim"] = types.ModuleType("pytorch_msssim")
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(MG.REF, "videoseal", "evals", "metrics.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return M


def main():
    torch.set_num_threads(8)
    _, build_extractor, *_ = MG.import_reference()
    MF.patch_torchvision()
    MB.extra_stubs()
    from videoseal.losses.videosealloss import VideosealLoss
    from videoseal.modules.common import Upsample
    from videoseal.modules.pixel_decoder import PixelDecoder
    d, e, sums = {}, {}, {}

    # ---- one Upsample group
    for (C, Co, f) in U.STAGES:
        for (H, W) in U.LATENTS:
            key = U.stage_name(C, Co, f, H, W)
            x, w, lw, lb, dout = U.stage_tensors(C, Co, f, H, W)
            sums[key] = U.checksum(x, w, lw, lb, dout).tolist()
            res = {}
            for dt in (torch.float64, torch.float32):
                m = Upsample("bilinear", C, Co, f, nn.GELU).to(dt)
                m.load_state_dict({"upsample_block.2.weight": w.to(dt), "upsample_block.3.weight": lw.to(dt), "upsample_block.3.bias": lb.to(dt)}, strict=True)
                xi = x.to(dt).requires_grad_(True)
                raw = m.upsample_block[2](m.upsample_block[1](m.upsample_block[0](xi)))
                out = m(xi)
                (out * dout.to(dt)).sum().backward()
                res[dt] = dict(out=out, raw=raw, dx=xi.grad, dw=m.upsample_block[2].weight.grad, dlw=m.upsample_block[3].weight.grad,
                               dlb=m.upsample_block[3].bias.grad)
            names = ("out", "raw") + (("dx", "dw", "dlw", "dlb") if (C, Co, f, H, W) == U.BWD_STAGE else ())
            for n in names:
                store(d, e, f"{key}.{n}", res[torch.float64][n], res[torch.float32][n])

    # ---- the per-pixel linear layer
    for (K, sig, hw) in U.LINEAR:
        key = U.linear_name(K, sig, hw)
        x, w, b, dp = U.linear_tensors(K, hw)
        sums[key] = U.checksum(x, w, b, dp).tolist()
        res = {}
        for dt in (torch.float64, torch.float32):
            pd = PixelDecoder(embed_dim=U.LINEAR_C, nbits=K - 1, upscale_stages=[], sigmoid_output=sig, pixelwise=True).to(dt)
            pd.load_state_dict({"linear.weight": w.to(dt), "linear.bias": b.to(dt)}, strict=True)
            xi = x.to(dt).requires_grad_(True)
            out = pd(xi)
            (out * dp.to(dt)).sum().backward()
            res[dt] = dict(out=out, dx=xi.grad, dw=pd.linear.weight.grad, db=pd.linear.bias.grad)
        for n in ("out", "dx", "dw", "db"):
            store(d, e, f"{key}.{n}", res[torch.float64][n], res[torch.float32][n])

    # ---- a whole head
    sd = {k[len("pixel_decoder."):]: v for k, v in U.head_tensors(U.CHAIN["embed_dim"], U.CHAIN["stages"], U.CHAIN["nbits"]).items()}
    for (H, W) in U.LATENTS:
        x = U.chain_input(H, W)
        sums[f"chain_{H}x{W}"] = U.checksum(x, *sd.values()).tolist()
        res = {}
        for dt in (torch.float64, torch.float32):
            pd = PixelDecoder(embed_dim=U.CHAIN["embed_dim"], nbits=U.CHAIN["nbits"], upscale_stages=list(U.CHAIN["stages"]), pixelwise=True).to(dt)
            pd.load_state_dict({k: v.to(dt) for k, v in sd.items()}, strict=True)
            with torch.no_grad():
                res[dt] = pd(x.to(dt))
        store(d, e, f"chain_{H}x{W}.out", res[torch.float64], res[torch.float32])

    # ---- the losses on pixel-wise logits
    w_det, w_dec = U.LOSS_W
    for sk in U.LOSS_SHAPES:
        for kind in U.LOSS_MASKS:
            key = f"loss_{sk}_{kind}"
            preds, masks, msgs = U.loss_tensors(sk, kind)
            sums[key] = U.checksum(preds, masks, msgs.float()).tolist()
            T = U.LOSS_T[kind]
            res = {}
            for dt in (torch.float64, torch.float32):
                crit = VideosealLoss(balanced=False, percep_weight=0.0, disc_weight=0.0, detect_weight=w_det, decode_weight=w_dec, percep_loss="mse").to(dt)
                p = preds.to(dt).requires_grad_(True)
                scaled = torch.cat([p[:, :1], p[:, 1:] / T], dim=1)
                imgs = torch.zeros(preds.shape[0], 3, 8, 8, dtype=dt)
                total, logs = crit(imgs, imgs, masks.to(dt), msgs, scaled, 0, 0, last_layer=None)
                total.backward()
                det, dec = float(logs["loss_detect"]), float(logs["loss_decode"])
                if kind == "none":
                    assert np.isnan(dec) and np.isfinite(det), (det, dec)
                res[dt] = dict(loss=torch.tensor([det, dec], dtype=torch.float64), dpreds=p.grad)
            store(d, e, key + ".dpreds", res[torch.float64]["dpreds"], res[torch.float32]["dpreds"])
            l64, l32 = res[torch.float64]["loss"], res[torch.float32]["loss"]
            d[key + ".loss"] = l64.numpy()
            e[key + ".loss"] = float(np.nanmax(np.abs((l32 - l64).numpy())))
            if kind == "none":              # nothing selected: the decoding term reaches no logit
                assert float(res[torch.float64]["dpreds"][:, 1:].abs().max()) == 0.0

    # ---- the metrics on 4-D logits
    M = load_metrics()
    Bn, K, H, W = 3, 7, 10, 12
    logits = U.vote_logits(Bn, K, H, W, seed=21)
    g = torch.Generator().manual_seed(22)
    bits = torch.randint(0, 2, (Bn, K), generator=g)
    mask = torch.zeros(Bn, 1, H, W)
    mask[:, :, 2:7, 3:11] = 1.0
    sums["vote"] = U.checksum(logits, bits.float(), mask).tolist()
    for thr in (0.0, 0.25):
        d[f"vote_acc_thr{thr}"] = M.bit_accuracy(logits, bits, None, thr).double().numpy()
        d[f"vote_acc_masked_thr{thr}"] = M.bit_accuracy(logits, bits, mask, thr).double().numpy()
        d[f"vote_1msg_thr{thr}"] = M.bit_accuracy_1msg(logits, bits, None, thr).double().numpy()
        d[f"vote_1msg_masked_thr{thr}"] = M.bit_accuracy_1msg(logits, bits, mask, thr).double().numpy()

    # ---- names and shapes of the pixel-wise heads the reference builds from its own configuration file
    heads = {}
    cfgs = yaml.safe_load(open(os.path.join(MG.REF, "configs", "extractor.yaml")))
    for name in ("convnext_tiny_pw", "convnext_base_pw", "sam_small_pw"):
        ext = build_extractor(name, MG.toD(cfgs[name]), 256, 96)
        heads[name] = {k: list(v.shape) for k, v in ext.state_dict().items() if k.startswith("pixel_decoder.")}
    d["meta"] = json.dumps(dict(e=e, sums=sums, heads=heads, loss_w=list(U.LOSS_W)))
    out = os.path.join(HERE, "pixel_head_ops.npz")
    np.savez_compressed(out, **d)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(d) - 1} arrays")
    model_cases(e)
    for k in sorted(e):
        print(f"  {k:40s} e_ref {e[k]:.3e}")


def train_cases(d):
    """the tiny ConvNeXt `_pw` model in train mode, float64, a rectangle mask handed through the mask embedder, no augmentation:
    'gen': train.py:626-643 with VideosealLoss(percep 'mse', detect 1, decode 1, balanced): the log and every detector gradient;
    'det': the detector alone on the frames, detection + masked decoding loss with fixed weights 1 / 1 (what DetectorStep computes).
    Per gradient tensor: its largest magnitude and a strided sub-sample (_pixel_head_util.grad_sub)."""
    from videoseal.augmentation.augmenter import Augmenter
    from videoseal.losses.videosealloss import VideosealLoss
    spec = U.model_specs()["cnx"]
    card = MG.card_for_spec(spec)
    card["extractor"]["params"]["pixel_decoder"].update(pixelwise=True, upscale_stages=list(U.MODEL_STAGES["cnx"]))
    imgs, masks, msgs = U.train_inputs(spec.nbits)
    meta = {}
    for case in ("gen", "det"):
        model = MG.build_reference(spec, card)
        model.load_state_dict(U.model_state_dict(spec, "cnx"), strict=True)
        model = model.double().train()
        model.augmenter = Augmenter(masks={"kind": "none"}, augs={"identity": 1}, augs_params={}, num_augs=1)
        model.augmenter.mask_embedder = lambda imgs_w, masks=None, **kw: masks          # the caller's masks are the mask targets
        torch.manual_seed(7)
        if case == "gen":
            crit = VideosealLoss(disc_weight=0.0, balanced=True, percep_weight=1.0, detect_weight=1.0, decode_weight=1.0, percep_loss="mse").double()
            out = model(imgs.double(), masks.double(), msgs, is_video=False)
            loss, logs = crit(imgs.double(), out["imgs_w"], out["masks"], out["msgs"], out["preds"], 0, 0, last_layer=model.embedder.get_last_layer())
            assert [k for k in logs if k.startswith("loss_")] == ["loss_percep", "loss_detect", "loss_decode"]
        else:
            crit = VideosealLoss(disc_weight=0.0, balanced=False, percep_weight=0.0, detect_weight=1.0, decode_weight=1.0, percep_loss="mse").double()
            preds = model.detector(imgs.double())
            loss, logs = crit(imgs.double(), imgs.double(), masks.double(), msgs, preds, 0, 0, last_layer=None)
        assert tuple((out["preds"] if case == "gen" else preds).shape[-2:]) == tuple(masks.shape[-2:])
        loss.backward()
        names = [k for k, p in model.named_parameters() if k.startswith("detector.") and p.grad is not None]
        gd = dict(model.named_parameters())
        d[f"train.{case}.names"] = np.array(names)
        d[f"train.{case}.gmax"] = np.array([float(gd[k].grad.abs().max()) for k in names])
        for i, k in enumerate(names):
            d[f"train.{case}.g{i}"] = U.grad_sub(gd[k].grad).numpy()
        meta[case] = dict(loss=float(loss), log={k: float(v) for k, v in logs.items()},
                          no_grad=[k for k, p in model.named_parameters() if k.startswith("detector.") and p.grad is None])
        print(f"train.{case}: loss {float(loss):.6f} log { {k: round(float(v), 6) for k, v in logs.items()} } {len(names)} detector gradients")
    return meta


def model_cases(e_all):
    """tests/golden/pixel_head_model.npz: `detect` (image and video form) and `extract_message` (every aggregation) of whole tiny models whose
    extractor ends in a pixel-wise head, float64 with the fp32 run's own error; the share of reference logits inside the decision margin of
    tests/_util.assert_decisions is checked here, so that the test's `min_sure` cannot fail for the seed's sake."""
    from oracle.inputs import synthetic_frames
    from tests._util import DECISION_MARGIN
    d, e, sums = {}, {}, {}
    n, h, w, seed = U.MODEL_FRAMES
    imgs = synthetic_frames(n, h, w, seed=seed)
    for tag, spec in U.model_specs().items():
        card = MG.card_for_spec(spec)
        card["extractor"]["params"]["pixel_decoder"].update(pixelwise=True, upscale_stages=list(U.MODEL_STAGES[tag]))
        sd = U.model_state_dict(spec, tag)
        sums[tag] = U.checksum(imgs, *[sd[k] for k in sorted(sd) if k.startswith("detector.pixel_decoder.")]).tolist()
        res = {}
        for dt in (torch.float64, torch.float32):
            model = MG.build_reference(spec, card)
            model.load_state_dict(sd, strict=True)
            model = model.to(dt).eval()
            with torch.no_grad():
                res[dt] = {f"{tag}.preds_{'vid' if v else 'img'}": model.detect(imgs.to(dt), is_video=v)["preds"] for v in (True, False)}
                if dt == torch.float64:
                    for a in U.AGGREGATIONS:
                        d[f"{tag}.msg_{a}"] = model.extract_message(imgs.to(dt), aggregation=a).numpy()
        for k in res[torch.float64]:
            store(d, e, k, res[torch.float64][k], res[torch.float32][k])
            p = res[torch.float64][k]
            inside = float((p.abs() <= DECISION_MARGIN).double().mean())
            assert inside <= 0.0005, f"{k}: {inside:.2%} of the reference logits lie inside the decision margin -- choose another seed"
            d[k + ".shape"] = np.array(p.shape)
    # a chain that pools: [4, 2, 1], `pixelwise: False`, sigmoid_output -- stages, a factor-1 stage, the mean over the pixels, Linear, sigmoid
    from videoseal.modules.pixel_decoder import PixelDecoder
    psd = {k[len("pixel_decoder."):]: v for k, v in U.head_tensors(64, U.POOLED_CHAIN, 16, seed=17).items()}
    psd["linear.weight"] = psd["linear.weight"].reshape(17, -1)
    x = U.chain_input(3, 5)[:, :64].contiguous()
    sums["pooled_chain"] = U.checksum(x, *psd.values()).tolist()
    res = {}
    for dt in (torch.float64, torch.float32):
        pd = PixelDecoder(embed_dim=64, nbits=16, upscale_stages=list(U.POOLED_CHAIN), pixelwise=False, sigmoid_output=True).to(dt)
        pd.load_state_dict({k: v.to(dt) for k, v in psd.items()}, strict=True)
        with torch.no_grad():
            res[dt] = pd(x.to(dt))
    store(d, e, "pooled_chain.out", res[torch.float64], res[torch.float32])
    train = train_cases(d)
    d["meta"] = json.dumps(dict(e=e, sums=sums, train=train))
    out = os.path.join(HERE, "pixel_head_model.npz")
    np.savez_compressed(out, **d)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(d) - 1} arrays")
    e_all.update(e)


if __name__ == "__main__":
    main()
