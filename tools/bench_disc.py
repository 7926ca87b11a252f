#!/usr/bin/env python
"""The PatchGAN discriminator on the HIP path (csrc/disc.hip, videoseal_amd/discriminator.py) at 16 x 256^2, n_layers = 2, input_nc = 1 -- the
recipe of the reference's train.py header -- in ONE process, with the protocol of tools/bench_ssim.py: warmed up, device events around batches of
calls, >= 0.5 s of timed work per figure, everything twice so that the run-to-run spread stands next to each figure.  Seeded inputs, no
reference checkout.

  (a) discriminator forward                         (b) forward + backward of the generator term -mean(D(x)), weights frozen
  (c) the hinge update (DiscriminatorStep.step on 16 real + 16 watermarked frames), with the share of each kernel group
  (d) GeneratorStep.step (VideoSeal 1.0) with disc_weight = 0.1 against the same object with disc_weight = 0 (the step as it was)
  (e) for orientation only: an eager torch.nn stack of the same layers on the same device tensors, (a) - (c)

usage: tools/bench_disc.py [--out FILE] [--quick]       (GPU box)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import bench
from tools.bench_ssim import spread, timed
from videoseal_amd import native as N
from videoseal_amd.discriminator import NLayerDiscriminator, generator_disc_loss
from videoseal_amd.training import DiscriminatorStep, GeneratorStep

QUICK = "--quick" in sys.argv
MIN_S = 0.05 if QUICK else 0.5
B, S = 16, 256


def twice(fn):
    for _ in range(2):
        fn()
    return [timed(fn, MIN_S) for _ in range(2)]


def eager_stack(d):
    """the same layers as torch modules sharing the parameters (input_nc = 1: Y = M[0] . rgb first)"""
    def fwd(x):
        if d.input_nc == 1:
            x = torch.einsum("bchw,c->bhw", x, d.rgb2yuv.M[0])[:, None]
        return d.main(x)
    return fwd


def kernel_shares(d, step, real, fake):
    """share of (c) per kernel group: device events around each launch wrapper of one hinge update (serialised, so the sum exceeds the step a little)"""
    spans = {}

    def wrap(obj, name, label):
        fn = getattr(obj, name)

        def timed_fn(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            spans.setdefault(label(*a, **k) if callable(label) else label, []).append((e0, e1))
            return r
        setattr(obj, name, timed_fn)
        return fn
    eng = d.engine()
    saved = [(eng, "conv", wrap(eng, "conv", lambda x, w, out, **k: f"vs_conv_gemm {'bwd-data' if k.get('pad') == 2 else 'fwd'} {x.C}->{w.N}")),
             (d, "_wgrad", wrap(d, "_wgrad", lambda eng_, p, l, n, x, s, ci: f"vs_conv4x4_wgrad {ci}->{n}")),
             (d, "_colsum", wrap(d, "_colsum", "bias column sums"))]
    L = eng.lib
    for name in ("vs_groupnorm_lrelu", "vs_groupnorm_lrelu_bwd", "vs_disc_input", "vs_conv4x4_n1", "vs_conv4x4_n1_bwd", "vs_disc_loss", "vs_dilate2"):
        saved.append((L, name, wrap(L, name, name)))
    for _ in range(3):
        spans.clear()
        d.zero_grad(set_to_none=True)
        step.step(real, fake)
    torch.cuda.synchronize()
    for obj, name, fn in saved:
        setattr(obj, name, fn)
    ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in spans.items()}
    tot = sum(ms.values())
    return {k: dict(ms=round(v, 4), share=round(v / tot, 4)) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])}


def main():
    dev = torch.device("cuda", 0)
    out = []
    real = bench.synthetic_batch(B, S, dev, seed=3)
    fake = (real + 0.02 * torch.randn(real.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(4))).clamp(0, 1)
    torch.manual_seed(11)
    d = NLayerDiscriminator(input_nc=1, ndf=32, n_layers=2).to(dev)
    eager = eager_stack(d)
    step = DiscriminatorStep(d)

    def fwd():
        with torch.no_grad():
            return d(real)

    def gen_term():
        for p in d.parameters():
            p.requires_grad_(False)
        x = fake.detach().requires_grad_(True)
        generator_disc_loss(d(x)).backward()
        for p in d.parameters():
            p.requires_grad_(True)

    def hinge():
        d.zero_grad(set_to_none=True)
        step.step(real, fake)

    def e_fwd():
        with torch.no_grad():
            return eager(real)

    def e_gen():
        for p in d.parameters():
            p.requires_grad_(False)
        x = fake.detach().requires_grad_(True)
        (-eager(x).mean()).backward()
        for p in d.parameters():
            p.requires_grad_(True)

    def e_hinge():
        d.zero_grad(set_to_none=True)
        lr, lf = eager(real), eager(fake)
        (0.5 * (F.relu(1 - lr).mean() + F.relu(1 + lf).mean())).backward()

    for what, hip_fn, torch_fn in (("(a) forward", fwd, e_fwd), ("(b) generator term, forward + backward, weights frozen", gen_term, e_gen),
                                   ("(c) hinge update", hinge, e_hinge)):
        h = twice(hip_fn)
        try:
            t = twice(torch_fn)
        except Exception as e:                                        # recorded, not hidden
            t = f"{type(e).__name__}: {e}"[:300]
        r = dict(what=what, frames=B, size=S, n_layers=2, input_nc=1, hip_ms=min(h), hip_runs_ms=h, hip_spread=spread(h))
        if isinstance(t, str):
            r["eager_error"] = t
        else:
            r.update(eager_ms=min(t), eager_runs_ms=t, eager_spread=spread(t), eager_over_hip=min(t) / min(h))
        print(json.dumps(r), flush=True)
        out.append(r)
    r = dict(what="(c) per kernel group", groups=kernel_shares(d, step, real, fake))
    print(json.dumps(r), flush=True)
    out.append(r)
    # (d) what the term costs a training step
    import videoseal_amd
    model = videoseal_amd.build("videoseal_1.0", seed=0).to(dev).train()
    masks = torch.ones(B, 1, S, S, device=dev)
    msgs = torch.randint(0, 2, (B, model.embedder.cfg.nbits), generator=torch.Generator().manual_seed(5))
    gs = GeneratorStep(model, percep_loss="yuv", percep_weight=0.1, decode_weight=1.0, balanced=False, disc_weight=0.1, disc_num_layers=2,
                       disc_in_channels=1, discriminator=d)
    steps = {"disc_weight_0": [], "disc_weight_0.1": []}

    def one():
        model.zero_grad(set_to_none=True)
        gs.step(real, masks, msgs)
    for _ in range(2):                                               # the two settings alternate
        for key, wgt in (("disc_weight_0", 0.0), ("disc_weight_0.1", 0.1)):
            gs.disc_weight = wgt
            for _ in range(3):
                one()
            torch.cuda.synchronize()
            k = 3 if QUICK else 12
            t0 = time.perf_counter()
            for _ in range(k):
                one()
            torch.cuda.synchronize()
            steps[key].append((time.perf_counter() - t0) / k * 1e3)
    a, b = min(steps["disc_weight_0"]), min(steps["disc_weight_0.1"])
    r = dict(what="(d) GeneratorStep videoseal_1.0 16x256^2, wall ms per step (two alternating runs)", **steps, added_ms=b - a, added_fraction=(b - a) / a)
    print(json.dumps(r), flush=True)
    out.append(r)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
