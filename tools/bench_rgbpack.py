#!/usr/bin/env python
"""Packed RGB clips on the HIP path (Videoseal.embed_rgb / detect_rgb) against the routes a caller had before, in ONE process: seeded inputs,
warmed up, device events, the routes alternating, every timed step under its own time limit (the protocol of tools/bench_yuv.py).

Scenario: VideoSeal 1.0, 32 x 768^2 frames resident in HBM, video mode, key frames every 4.  Per step (embed + detect of the clip):
  (a) embed_rgb + detect_rgb for rgb24, bgra, rgba64, x2rgb10;
  (b) embed_u8 + detect_u8 on the rgb24 frames;
  (c) the bgra frames through torch: channel select to RGB24, embed_u8 + detect_u8, re-pack with the alpha.
Two conditions, both relative and read from the run itself:
  1. median(a, rgb24) is not above median(b) by more than the spread (max - min) of (b);
  2. median(a, bgra) is below median(c) by more than the spread of (c).
The shell kernels' time and fraction of 8 TB/s over their algorithmic bytes (the frame's pixels each way + the low-resolution tensors) stand
beside those of resize_pre_kernel<u8> / embed_tail_kernel<u8> from the same run.  Nothing is tuned to the comparison: a condition that does
not hold is reported with its numbers and the kernel that loses.
usage: tools/bench_rgbpack.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/rgbpack_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs
from videoseal_amd import rgbpack

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (a whole embed + detect of the clip) may not take longer
FMTS = ("rgb24", "bgra", "rgba64", "x2rgb10")


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


def main():
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "rgbpack_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    Fn, H, W = (8, 256, 256) if QUICK else (32, 768, 768)
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.chunk_size, model.step_size, model.video_mode = 8, 4, "repeat"          # 32 frames per chunk, key frames every 4
    x = synthetic_frames(Fn, H, W, seed=123)
    msgs = synthetic_msgs(1, model.embedder.cfg.nbits, seed=123)
    g = torch.Generator().manual_seed(7)
    clips = {}
    for fmt in FMTS:
        c = rgbpack.from_rgb(x, fmt)
        if fmt == "bgra":                                   # a capture surface's alpha is not constant
            c[..., 3] = torch.randint(0, 256, c.shape[:3], dtype=torch.uint8, generator=g)
        clips[fmt] = c.to(dev)

    def route_a(fmt):
        def run():
            w = model.embed_rgb(clips[fmt], fmt, msgs, lowres_attenuation=True)["imgs_w"]
            return w, model.detect_rgb(w, fmt)["preds"]
        return run

    def route_b():
        w = model.embed_u8(clips["rgb24"], msgs, lowres_attenuation=True)["imgs_w"]
        return w, model.detect_u8(w)["preds"]

    def route_c():
        src = clips["bgra"]
        rgb = src[..., [2, 1, 0]].contiguous()                                    # channel select to RGB24
        w = model.embed_u8(rgb, msgs, lowres_attenuation=True)["imgs_w"]
        p = model.detect_u8(w)["preds"]
        return torch.cat([w[..., [2, 1, 0]], src[..., 3:4]], dim=-1), p            # re-pack with the alpha

    routes = {"b_u8_rgb24": route_b, "c_bgra_via_torch": route_c}
    for fmt in FMTS:
        routes[f"a_{fmt}"] = route_a(fmt)
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    same_as_u8 = bool(torch.equal(route_a("rgb24")()[0], route_b()[0]))
    wa, wc = route_a("bgra")()[0], route_c()[0]
    same_alpha = bool(torch.equal(wa[..., 3], wc[..., 3]))
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every route alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    shell = {}
    for name in ["b_u8_rgb24"] + [f"a_{f}" for f in FMTS]:
        shell.update({k: v for k, v in shell_records(model, routes[name]).items() if k not in shell})

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}
    a24, ab, b, c = res["a_rgb24"], res["a_bgra"], res["b_u8_rgb24"], res["c_bgra_via_torch"]
    u8 = {k.split("<")[0].replace("_kernel", ""): v for k, v in shell.items() if k.endswith("<u8>")}
    own = {k.split("<")[0].replace("_rgb_kernel", ""): v for k, v in shell.items() if k.endswith("<rgb24>")}
    look = {
        "rgb24_vs_u8": {"condition": "median(a, rgb24) <= median(b) + spread(b)", "a_minus_b_ms": round(a24["median_ms"] - b["median_ms"], 3),
                        "spread_b_ms": b["spread_ms"], "holds": bool(a24["median_ms"] <= b["median_ms"] + b["spread_ms"]),
                        "shell_kernels_us_rgb24_minus_u8": {k: round(own[k]["us"] - u8[k]["us"], 1) for k in own if k in u8}},
        "bgra_vs_torch": {"condition": "median(a, bgra) < median(c) - spread(c)", "c_minus_a_ms": round(c["median_ms"] - ab["median_ms"], 3),
                          "spread_c_ms": c["spread_ms"], "holds": bool(ab["median_ms"] < c["median_ms"] - c["spread_ms"])},
    }
    doc = {
        "tool": "tools/bench_rgbpack.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"frames": Fn, "H": H, "W": W, "model": "videoseal_1.0", "video_mode": "repeat", "step_size": 4, "chunk_size": 8,
                     "lowres_attenuation": True, "resident": "HBM", "repeats": repeats, "quick": QUICK},
        "routes_ms_per_step": res,
        "what_to_look_for": look,
        "all_conditions_hold": all(v["holds"] for v in look.values()),
        "embed_rgb_rgb24_equals_embed_u8": same_as_u8, "bgra_alpha_equals_the_torch_route": same_alpha,
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
