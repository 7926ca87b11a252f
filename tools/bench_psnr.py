#!/usr/bin/env python
"""Embedding to a target PSNR (Videoseal.embed_psnr) against the fixed-strength embed and against the route a caller had before, in ONE
process: seeded inputs, warmed up, device events, the legs alternating, every timed step under its own time limit (the protocol of
tools/bench_rgbpack.py).

Scenario: VideoSeal 1.0, 32 x 768^2 frames resident in HBM, target 42 dB; image mode (a message per frame) and video mode (key frames every
4, 32 frames per chunk).  Legs per mode:
  (a) embed_psnr                                  fp32 (full-resolution JND) and uint8 (low-resolution JND, embed_u8's default);
  (b) embed / embed_u8 on the same frames;
  (c) fp32 only, through torch: embed at scaling_w = 1 with the clamp off, the perturbation (preds_w in image mode, imgs_w - imgs in video
      mode) reduced per frame in torch, imgs + s * d rebuilt and clamped.
Two conditions, both relative and read from the run itself:
  1. median(a) is below median(c) by more than the spread (max - min) of (c);
  2. (a) - (b) is recorded beside the per-launch times of the energy pass, the tail and the scaled tail and their fraction of 8 TB/s over
     algorithmic bytes -- the expectation is about one more read of the frames where the heat-map is computed at full resolution.
Nothing is tuned to the comparison: a condition that does not hold is reported with its numbers.
usage: tools/bench_psnr.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/psnr_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (a whole embed of the clip) may not take longer
TARGET = 42.0


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


class StepTimeout(RuntimeError):
    pass


def limited(fn, what):
    """run fn(), then wait for the device by polling an event against a deadline: a hanging kernel ends the run with StepTimeout"""
    t0 = time.monotonic()
    out = fn()
    done = torch.cuda.Event()
    done.record()
    while not done.query():
        if time.monotonic() - t0 > STEP_LIMIT_S:
            raise StepTimeout(f"{what}: no result after {STEP_LIMIT_S} s")
        time.sleep(2e-4)
    return out


def timed_ms(fn, what):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        e0.record()
        fn()
        e1.record()
    limited(run, what)
    return e0.elapsed_time(e1)


def shell_records(model, fn):
    """{kernel name: us, launches, algorithmic bytes, fraction of 8 TB/s} of the shell kernels of one untimed pass of fn()"""
    eng = model._engine()
    eng.shell_timers = []
    try:
        limited(fn, "shell timing pass")
        rec = {}
        for name, a, b, nbytes in eng.shell_timers:
            us, nb, each = rec.get(name, (0.0, 0, []))
            t = a.elapsed_time(b) * 1e3
            rec[name] = (us + t, nb + nbytes, each + [round(t, 1)])
    finally:
        eng.shell_timers = None
    return {k: {"us": round(us, 1), "launches_us": each, "bytes": nb, "frac_of_8TBs": round(nb / (us * 1e-6) / PEAK, 4)}
            for k, (us, nb, each) in rec.items()}


def torch_route(model, x, msgs, is_video):
    """what a caller did before: strength 1, clamp off, the perturbation reduced and the frame rebuilt in torch"""
    sw, clamp = model.blender.scaling_w, model.clamp
    model.blender.scaling_w, model.clamp = 1.0, False
    try:
        r = model.embed(x, msgs, is_video=is_video)
    finally:
        model.blender.scaling_w, model.clamp = sw, clamp
    d = r["imgs_w"] - x if is_video else r["preds_w"]
    e = d.square().sum(dim=(1, 2, 3), dtype=torch.float64) * (3.0 / d.shape[1])
    s = (10.0 ** (-TARGET / 20.0) * torch.sqrt(3.0 * x.shape[-2] * x.shape[-1] / e)).float()
    return torch.clamp(x + s[:, None, None, None] * d, 0.0, 1.0)


def main():
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "psnr_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    Fn, H, W = (8, 256, 256) if QUICK else (32, 768, 768)
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.step_size, model.video_mode = 4, "repeat"
    x = synthetic_frames(Fn, H, W, seed=123).to(dev)
    x8 = (x * 255.0).round().byte().permute(0, 2, 3, 1).contiguous()
    nbits = model.embedder.cfg.nbits
    msgs = {True: synthetic_msgs(1, nbits, seed=123), False: synthetic_msgs(Fn, nbits, seed=123)}
    chunk = {True: 8, False: 32}                             # 32 frames per chunk either way

    def leg(fn, is_video):
        def run():
            model.chunk_size = chunk[is_video]
            return fn()
        return run

    routes = {}
    for is_video, tag in ((False, "image"), (True, "video")):
        m = msgs[is_video]
        routes[f"{tag}.a_embed_psnr"] = leg(lambda m=m, v=is_video: model.embed_psnr(x, TARGET, m, is_video=v)["imgs_w"], is_video)
        routes[f"{tag}.b_embed"] = leg(lambda m=m, v=is_video: model.embed(x, m, is_video=v)["imgs_w"], is_video)
        routes[f"{tag}.c_torch"] = leg(lambda m=m, v=is_video: torch_route(model, x, m, v), is_video)
    routes["video.a_embed_psnr_u8"] = leg(lambda: model.embed_psnr(x8, TARGET, msgs[True], lowres_attenuation=True)["imgs_w"], True)
    routes["video.b_embed_u8"] = leg(lambda: model.embed_u8(x8, msgs[True])["imgs_w"], True)
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    # the two routes to a target agree up to the rounding of the torch route's fp32 reduction input
    agree = {tag: float((routes[f"{tag}.a_embed_psnr"]() - routes[f"{tag}.c_torch"]()).abs().max()) for tag in ("image", "video")}
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every leg alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    shell = {name: shell_records(model, routes[name]) for name in routes if ".c_" not in name}

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}
    look = {}
    for tag in ("image", "video"):
        a, b, c = res[f"{tag}.a_embed_psnr"], res[f"{tag}.b_embed"], res[f"{tag}.c_torch"]
        look[f"{tag}.below_the_torch_route"] = {"condition": "median(a) < median(c) - spread(c)", "c_minus_a_ms": round(c["median_ms"] - a["median_ms"], 3),
                                                "spread_c_ms": c["spread_ms"], "holds": bool(a["median_ms"] < c["median_ms"] - c["spread_ms"])}
        look[f"{tag}.cost_over_embed"] = {"a_minus_b_ms": round(a["median_ms"] - b["median_ms"], 3), "spread_b_ms": b["spread_ms"],
                                          "frames_bytes": x.numel() * 4,
                                          "one_read_of_the_frames_at_8TBs_ms": round(x.numel() * 4 / PEAK * 1e3, 3),
                                          "launches": {"embed_psnr": {k: v for k, v in shell[f"{tag}.a_embed_psnr"].items() if "tail" in k},
                                                       "embed": {k: v for k, v in shell[f"{tag}.b_embed"].items() if "tail" in k}}}
    a8, b8 = res["video.a_embed_psnr_u8"], res["video.b_embed_u8"]
    look["video.u8.cost_over_embed_u8"] = {"a_minus_b_ms": round(a8["median_ms"] - b8["median_ms"], 3), "spread_b_ms": b8["spread_ms"],
                                           "launches": {"embed_psnr": {k: v for k, v in shell["video.a_embed_psnr_u8"].items() if "tail" in k},
                                                        "embed_u8": {k: v for k, v in shell["video.b_embed_u8"].items() if "tail" in k}}}
    doc = {
        "tool": "tools/bench_psnr.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"frames": Fn, "H": H, "W": W, "model": "videoseal_1.0", "target_psnr": TARGET, "video_mode": "repeat", "step_size": 4,
                     "frames_per_chunk": 32, "resident": "HBM", "repeats": repeats, "quick": QUICK,
                     "fp32": "full-resolution JND", "uint8": "low-resolution JND"},
        "legs_ms_per_step": res,
        "what_to_look_for": look,
        "all_conditions_hold": all(v["holds"] for v in look.values() if "holds" in v),
        "max_abs_difference_embed_psnr_vs_torch_route": agree,
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
