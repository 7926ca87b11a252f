#!/usr/bin/env python
"""The pixel-wise extractor head (csrc/pixel_head.hip, videoseal_amd/pixel_head.py) at the working size of `convnext_tiny_pw` and
`convnext_base_pw`: 32 frames of 256^2 (an 8 x 8 latent), 96 bits, head [4, 4, 2].  One process, warmed up, device events, >= 0.3 s of timed
work per figure, every figure twice (`runs`; the smaller one is reported).

  per stage and for the linear layer: ms on the HIP path and for the same layer as plain torch modules on the same device tensors
  linear layer: bytes written / time as a fraction of 8 TB/s
  whole `detect` of the model with the pixel-wise head and with the per-frame head on the same backbone (what the head adds to the backbone)
  backward kernels of the head at 16 x 256^2 (stage backward, linear backward, the two losses, the pixel vote)
  training at 16 x 256^2: DetectorStep (detection + masked decoding loss) and GeneratorStep(detect 1, decode 1, 'mse') on the `_pw` model,
  and the same steps on the per-frame head of the same backbone

One JSON line per figure; --out FILE also writes the list.     usage: tools/bench_pixel_head.py [--out FILE] [--quick]     (GPU box)"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from videoseal_amd import native as N
from videoseal_amd import pixel_head as PH
from videoseal_amd.engine import Act
from videoseal_amd.layout import ModelCfg
from videoseal_amd.model import build_model

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
MIN_S = 0.03 if QUICK else 0.3
CARDS = {"convnext_tiny_pw": dict(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768]), "convnext_base_pw": dict(depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024])}
STAGES, NBITS, S = [4, 4, 2], 96, 256


def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    n = max(3, int(MIN_S * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def twice(fn):
    r = [timed(fn), timed(fn)]
    return min(r), r


def torch_stage(x, w, lw, lb, f):
    y = F.conv2d(F.pad(F.interpolate(x, scale_factor=f, mode="bilinear", align_corners=False), (1, 1, 1, 1), mode="reflect"), w)
    u = y.mean(1, keepdim=True)
    s = (y - u).pow(2).mean(1, keepdim=True)
    return F.gelu(lw[:, None, None] * ((y - u) / torch.sqrt(s + 1e-6)) + lb[:, None, None])


def nhwc(x):
    B, C, H, W = x.shape
    return Act(x.permute(0, 2, 3, 1).contiguous().view(-1), B, H, W, C, C)


def main():
    out = []

    def emit(**r):
        print(json.dumps(r), flush=True)
        out.append(r)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    for card, arch in CARDS.items():
        cfg = ModelCfg(nbits=NBITS, hidden=2 * NBITS, img_size=S, head_stages=STAGES, head_pixelwise=True, **arch)
        model = build_model(cfg).eval().to(dev)
        plain = build_model(ModelCfg(nbits=NBITS, hidden=2 * NBITS, img_size=S, **arch)).eval().to(dev)
        eng = model._engine()
        for B, backward in ((32, False), (16, True)):
            c, hw = arch["dims"][-1], S // 32
            x = torch.randn(B, c, hw, hw, device=dev, generator=g)
            with torch.no_grad():
                for i, f in enumerate(STAGES):
                    co = c // f
                    w = torch.randn(co, c, 3, 3, device=dev, generator=g) / math.sqrt(9 * c)
                    lw, lb = torch.rand(co, device=dev, generator=g) + 0.5, torch.randn(co, device=dev, generator=g)
                    xa = nhwc(x)
                    wz = PH.pack_stage(w, xa.ld)
                    if not backward:
                        h, hr = twice(lambda: PH.stage_forward(eng, xa, wz, lw, lb, f, f"b.s{i}"))
                        t, tr = twice(lambda: torch_stage(x, w, lw, lb, f))
                        emit(card=card, what=f"stage {i}: {c} -> {co} x{f} at {hw * f}^2", frames=B, hip_ms=h, hip_runs_ms=hr, torch_ms=t, torch_runs_ms=tr,
                             torch_over_hip=t / h, direct_conv_gmac=B * (hw * f) ** 2 * 9 * c * co / 1e9)
                    else:
                        o, raw, ln = PH.stage_forward(eng, xa, wz, lw, lb, f, f"b.t{i}", keep_raw=True)
                        do = Act(torch.randn(o.rows * o.ld, device=dev, generator=g), o.B, o.H, o.W, o.C, o.ld)
                        h, hr = twice(lambda: PH.stage_backward(eng, xa, w, lw, raw, ln, do, f, f"b.u{i}"))
                        emit(card=card, what=f"stage {i} backward (dx, dW, LayerNorm grads): {c} -> {co} x{f} at {hw * f}^2", frames=B, hip_ms=h, hip_runs_ms=hr)
                    x = torch_stage(x, w, lw, lb, f)
                    c, hw = co, hw * f
                K = NBITS + 1
                w, b = torch.randn(K, c, device=dev, generator=g) / math.sqrt(c), torch.randn(K, device=dev, generator=g)
                xa = nhwc(x)
                preds = torch.empty(B, K, hw, hw, device=dev)
                nbytes = preds.numel() * 4
                if not backward:
                    h, hr = twice(lambda: PH.linear_forward(xa, w, b, False, preds))
                    t, tr = twice(lambda: F.conv2d(x, w[:, :, None, None], b))
                    emit(card=card, what=f"linear {c} -> {K} at {hw}^2 (NCHW logits)", frames=B, hip_ms=h, hip_runs_ms=hr, torch_ms=t, torch_runs_ms=tr,
                         torch_over_hip=t / h, bytes_written=nbytes, hip_fraction_of_8TBs_write=nbytes / (h * 1e-3) / PEAK)
                else:
                    PH.linear_forward(xa, w, b, False, preds)
                    dp = torch.randn(preds.shape, device=dev, generator=g)
                    h, hr = twice(lambda: PH.linear_backward(xa, w, dp))
                    emit(card=card, what=f"linear backward (dx, dW, db) {c} -> {K} at {hw}^2", frames=B, hip_ms=h, hip_runs_ms=hr)
                    masks = (torch.rand(B, 1, hw, hw, device=dev, generator=g) > 0.5).float()
                    msgs = torch.randint(0, 2, (B, NBITS), device=dev, generator=g).to(torch.int32)
                    h, hr = twice(lambda: PH.pixel_bce(preds, masks, msgs))
                    emit(card=card, what="detection + masked decoding loss with dpreds", frames=B, hip_ms=h, hip_runs_ms=hr,
                         fraction_of_8TBs=2 * nbytes / (h * 1e-3) / PEAK)
                    h, hr = twice(lambda: PH.pixel_vote(preds[:, 1:], masks, 0.0))
                    emit(card=card, what="pixel vote (bit_accuracy)", frames=B, hip_ms=h, hip_runs_ms=hr, fraction_of_8TBs=nbytes / (h * 1e-3) / PEAK)
        imgs = torch.rand(32, 3, S, S, device=dev, generator=g)
        with torch.no_grad():
            h, hr = twice(lambda: model.detect(imgs, is_video=False))
            p, pr = twice(lambda: plain.detect(imgs, is_video=False))
        emit(card=card, what="detect, 32 x 256^2: pixel-wise head vs the per-frame head on the same backbone", pixelwise_ms=h, pixelwise_runs_ms=hr,
             per_frame_ms=p, per_frame_runs_ms=pr, head_adds_ms=h - p)
        from videoseal_amd.training import DetectorStep, GeneratorStep
        fr = torch.rand(16, 3, S, S, device=dev, generator=g)
        masks = torch.zeros(16, 1, S, S, device=dev)
        masks[:, :, 32:200, 40:220] = 1.0
        msgs = torch.randint(0, 2, (16, NBITS), device=dev, generator=g)
        for m_, name in ((model, "pixel-wise head"), (plain, "per-frame head")):
            m_.train()
            pw = m_ is model
            ds = DetectorStep(m_)
            kw = dict(masks=masks, detect_weight=1.0, decode_weight=1.0) if pw else {}
            h, hr = twice(lambda: ds.step(fr, msgs, accumulate=False, **kw))
            emit(card=card, what=f"DetectorStep, 16 x 256^2, {name}", hip_ms=h, hip_runs_ms=hr)
            gs = GeneratorStep(m_, percep_loss="mse", decode_weight=1.0, detect_weight=1.0 if pw else 0.0)

            def gen_step():
                m_.zero_grad(set_to_none=True)
                gs.step(fr, masks, msgs)
            h, hr = twice(gen_step)
            emit(card=card, what=f"GeneratorStep, 16 x 256^2, {name}", hip_ms=h, hip_runs_ms=hr)
            m_.zero_grad(set_to_none=True)
        del model, plain, ds, gs
        torch.cuda.empty_cache()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
