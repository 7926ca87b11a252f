#!/usr/bin/env python
"""Half-precision clips on the HIP path (Videoseal.embed_half / detect_half) against the route a caller had before, in ONE process: seeded
inputs, warmed up, device events, the routes alternating, every timed step under its own time limit (the protocol of tools/bench_rgbpack.py).

Scenario: VideoSeal 1.0, 32 x 768^2 frames resident in HBM, embed + detect per step, video mode (key frames every 4) and image mode.
  (a) embed_half + detect_half on bf16 signed planar, fp16 unit planar, bf16 signed channels-last, fp16 unit nhwc-4;
  (b) the same tensors through torch: halfpix.to_rgb -> embed + detect -> halfpix.from_rgb(like=clip);
  (c) embed + detect on the fp32 frames alone, for orientation.
Condition, relative and read from the run itself: median(a) is below median(b) by more than the spread (max - min) of (b), for every case.
Also reported: (a) - (c), and the new shell kernels' time per launch (device events around each launch, the engine's shell timers) with
their fraction of 8 TB/s over algorithmic bytes (the frame's samples each way + the low-resolution tensors).  Nothing is tuned to the
comparison: a condition that does not hold is reported with its numbers.
usage: tools/bench_half.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/half_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs
from videoseal_amd import halfpix

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (a whole embed + detect of the clip) may not take longer
CASES = {                   # name: dtype, value_range, layout, memory form
    "bf16_signed_planar": (torch.bfloat16, "signed", "nchw", "planar"),
    "fp16_unit_planar": (torch.float16, "unit", "nchw", "planar"),
    "bf16_signed_channels_last": (torch.bfloat16, "signed", "nchw", "cl"),
    "fp16_unit_nhwc4": (torch.float16, "unit", "nhwc", "nhwc4"),
}


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
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "half_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    Fn, H, W = (8, 256, 256) if QUICK else (32, 768, 768)
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.chunk_size, model.step_size, model.video_mode = 8, 4, "repeat"          # 32 frames per chunk, key frames every 4
    x = synthetic_frames(Fn, H, W, seed=123)
    nbits = model.embedder.cfg.nbits
    msgs = {True: synthetic_msgs(1, nbits, seed=123), False: synthetic_msgs(Fn, nbits, seed=123)}
    g = torch.Generator().manual_seed(7)
    clips = {}
    for name, (dt, rng, layout, form) in CASES.items():
        c = halfpix.from_rgb(x, layout=layout, value_range=rng, dtype=dt)
        if form == "nhwc4":
            c = torch.cat([c, torch.rand(Fn, H, W, 1, generator=g).to(dt)], dim=-1).contiguous()
        elif form == "cl":
            c = c.contiguous(memory_format=torch.channels_last)
        clips[name] = c.to(dev)
    x32 = x.to(dev)

    def route_a(name, video):
        _, rng, layout, _ = CASES[name]

        def run():
            w = model.embed_half(clips[name], msgs[video], is_video=video, value_range=rng, layout=layout, lowres_attenuation=True)["imgs_w"]
            return w, model.detect_half(w, is_video=video, value_range=rng, layout=layout)["preds"]
        return run

    def route_b(name, video):
        _, rng, layout, _ = CASES[name]

        def run():
            src = clips[name]
            f = halfpix.to_rgb(src, layout, rng)
            w = model.embed(f, msgs[video], is_video=video, lowres_attenuation=True)["imgs_w"]
            p = model.detect(w, is_video=video)["preds"]
            return halfpix.from_rgb(w, like=src, layout=layout, value_range=rng), p
        return run

    def route_c(video):
        def run():
            w = model.embed(x32, msgs[video], is_video=video, lowres_attenuation=True)["imgs_w"]
            return w, model.detect(w, is_video=video)["preds"]
        return run

    routes, same = {}, {}
    for video in (True, False):
        tag = "video" if video else "image"
        routes[f"c_fp32_{tag}"] = route_c(video)
        for name in CASES:
            routes[f"a_{name}_{tag}"] = route_a(name, video)
            routes[f"b_{name}_{tag}"] = route_b(name, video)
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    for video in (True, False):
        tag = "video" if video else "image"
        for name in CASES:
            wa, wb = routes[f"a_{name}_{tag}"]()[0], routes[f"b_{name}_{tag}"]()[0]
            same[f"{name}_{tag}"] = bool(torch.equal(wa.contiguous().view(torch.int16), wb.contiguous().view(torch.int16)))
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every route alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    shell = {}
    for name in CASES:
        shell.update({k: v for k, v in shell_records(model, routes[f"a_{name}_video"]).items() if k not in shell})

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}
    look = {}
    for video in (True, False):
        tag = "video" if video else "image"
        c = res[f"c_fp32_{tag}"]
        for name in CASES:
            a, b = res[f"a_{name}_{tag}"], res[f"b_{name}_{tag}"]
            look[f"{name}_{tag}"] = {"condition": "median(a) < median(b) - spread(b)", "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 3),
                                     "spread_b_ms": b["spread_ms"], "holds": bool(a["median_ms"] < b["median_ms"] - b["spread_ms"]),
                                     "a_minus_c_ms": round(a["median_ms"] - c["median_ms"], 3)}
    doc = {
        "tool": "tools/bench_half.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"frames": Fn, "H": H, "W": W, "model": "videoseal_1.0", "video_mode": "repeat", "step_size": 4, "chunk_size": 8,
                     "lowres_attenuation": True, "resident": "HBM", "repeats": repeats, "quick": QUICK},
        "routes_ms_per_step": res,
        "what_to_look_for": look,
        "all_conditions_hold": all(v["holds"] for v in look.values()),
        "embed_half_equals_the_torch_route": same,
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
