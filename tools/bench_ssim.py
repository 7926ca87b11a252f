#!/usr/bin/env python
"""SSIM / MS-SSIM on the HIP path (csrc/ssim.hip) against the torch path it replaces on device tensors (`metrics._ssim_cs` through ten
grouped F.conv2d per scale, and torch.autograd through it for the loss), in ONE process: warmed up, device events, the two sides
alternating, >= 0.5 s of timed work per figure, the whole measurement twice so that the run-to-run spread is printed next to the ratio.

  32 x 3 x 768^2   metric, forward only (what evals/full.py feeds)        16 x 3 x 768^2, 16 x 3 x 256^2   loss, forward + backward
  GeneratorStep (VideoSeal 1.0, 16 x 256^2) with percep_loss = yuv / ssim / msssim: what the term costs a training step

One JSON line per shape: ms per call, algorithmic bytes (8 B per pixel-channel forward, 20 B forward + backward; five pyramid levels add
1/3), bytes / time as a fraction of 8 TB/s, kernel launches per call (counted from the call sequence), the same for the torch side (its
launches are not counted), `spread` = |run 1 - run 2| / mean per side.  If the torch side cannot run, its error text is the result.
usage: tools/bench_ssim.py [--out FILE] [--quick]       (GPU box)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from videoseal_amd import autograd as AG
from videoseal_amd import metrics as M

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
MIN_S = 0.05 if QUICK else 0.5


def torch_ssim(x, y):
    s, _ = M._ssim_cs(x, y, 1.0, M._gauss_window(11, 1.5, x))
    return s.mean(1)


def torch_msssim(x, y):
    win = M._gauss_window(11, 1.5, x)
    fs = []
    for lv in range(5):
        s, cs = M._ssim_cs(x, y, 1.0, win)
        if lv < 4:
            fs.append(torch.relu(cs))
            pad = [d % 2 for d in x.shape[2:]]
            x, y = torch.nn.functional.avg_pool2d(x, 2, padding=pad), torch.nn.functional.avg_pool2d(y, 2, padding=pad)
    fs.append(torch.relu(s))
    w = torch.tensor(M._MS_WEIGHTS, device=x.device, dtype=x.dtype).view(-1, 1, 1)
    return torch.prod(torch.stack(fs, 0) ** w, 0).mean(1)


def timed(fn, min_s):
    """ms per call over >= min_s of device time (events around a batch of calls sized from a first probe)"""
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    n = max(3, int(min_s * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def ab(hip_fn, torch_fn):
    """two alternating rounds -> ([hip ms run 1, run 2], [torch ms ...] or the error text)"""
    for _ in range(2):
        hip_fn()
    err = None
    try:
        for _ in range(2):
            torch_fn()
        torch.cuda.synchronize()
    except Exception as e:                                           # e.g. grouped convolutions without MIOpen kernels: recorded, not hidden
        err = f"{type(e).__name__}: {e}"[:300]
    h, t = [], []
    for _ in range(2):
        h.append(timed(hip_fn, MIN_S))
        if err is None:
            t.append(timed(torch_fn, MIN_S))
    return h, (t if err is None else err)


def spread(v):
    return abs(v[0] - v[1]) / (0.5 * (v[0] + v[1]))


def report(name, shape, levels, backward, h, t, launches):
    n = shape[0] * shape[1] * shape[2] * shape[3]
    nbytes = n * (20 if backward else 8) * (4 / 3 if levels > 1 else 1)
    r = dict(what=name, shape=list(shape), levels=levels, backward=backward, algorithmic_bytes=int(nbytes), hip_ms=min(h), hip_runs_ms=h,
             hip_spread=spread(h), hip_fraction_of_8TBs=nbytes / (min(h) * 1e-3) / PEAK, hip_launches=launches)
    if isinstance(t, str):
        r["torch_error"] = t
    else:
        r.update(torch_ms=min(t), torch_runs_ms=t, torch_spread=spread(t), torch_fraction_of_8TBs=nbytes / (min(t) * 1e-3) / PEAK,
                 torch_over_hip=min(t) / min(h), hip_not_slower=bool(min(h) <= min(t) * (1 + max(spread(h), spread(t)))))
    print(json.dumps(r), flush=True)
    return r


def main():
    dev = torch.device("cuda", 0)
    out = []
    # launches per call: per level vs_ssim_stats = 2 (+ 1 pooling between levels); backward: 1 vs_ssim_grad per level
    for B, S, backward in ((32, 768, False), (16, 768, True), (16, 256, True)):
        x = bench.synthetic_batch(B, S, dev, seed=3)
        y = (x + 0.02 * torch.randn(x.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(4))).clamp(0, 1)
        for levels, hip_metric, torch_metric, loss in ((1, M.ssim, torch_ssim, AG.ssim_loss), (5, M.msssim, torch_msssim, AG.msssim_loss)):
            if not backward:
                with torch.no_grad():
                    h, t = ab(lambda: hip_metric(x, y), lambda: torch_metric(x, y))
                    assert M.LAST_SSIM_BACKEND == "hip"
                launches = 2 * levels + (levels - 1)
            else:
                yg = y.clone().requires_grad_(True)

                def hip_fb():
                    yg.grad = None
                    loss(x, yg).backward()

                def torch_fb():
                    yg.grad = None
                    (-torch_metric(x, yg).mean()).backward()
                h, t = ab(hip_fb, torch_fb)
                launches = 2 * levels + (levels - 1) + levels
            out.append(report("ssim" if levels == 1 else "msssim", (B, 3, S, S), levels, backward, h, t, launches))
    # what the term costs a training step
    import videoseal_amd
    from videoseal_amd.training import GeneratorStep
    model = videoseal_amd.build("videoseal_1.0", seed=0).to(dev).train()
    frames = bench.synthetic_batch(16, 256, dev, seed=7)
    masks = torch.ones(16, 1, 256, 256, device=dev)
    msgs = torch.randint(0, 2, (16, model.embedder.cfg.nbits), generator=torch.Generator().manual_seed(5))
    steps = {}
    for kind in ("yuv", "ssim", "msssim"):
        gs = GeneratorStep(model, percep_loss=kind, percep_weight=0.1, decode_weight=1.0, balanced=False)

        def one():
            model.zero_grad(set_to_none=True)
            gs.step(frames, masks, msgs)
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        runs = []
        for _ in range(2):
            t0 = time.perf_counter()
            k = 3 if QUICK else 12
            for _ in range(k):
                one()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / k * 1e3)
        steps[kind] = runs
    r = dict(what="GeneratorStep videoseal_1.0 16x256^2, wall ms per step (two runs)", **{k: v for k, v in steps.items()},
             ssim_minus_yuv_ms=min(steps["ssim"]) - min(steps["yuv"]), msssim_minus_yuv_ms=min(steps["msssim"]) - min(steps["yuv"]))
    print(json.dumps(r), flush=True)
    out.append(r)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
