#!/usr/bin/env python
"""4:2:2 and 4:4:4 clips on the HIP path (Videoseal.embed_yuv / detect_yuv) against the route a caller had before and against the 4:2:0 format
of the same depth and layout, in ONE process: seeded inputs, warmed up, device events, the routes alternating, every timed step under its own
time limit (the protocol of tools/bench_yuv420.py).

Scenario: VideoSeal 1.0, 32 x 768^2 frames resident in HBM, video mode, key frames every 4.  Per step (embed + detect of the clip), for each of
yuv422p, yuv422p10, nv16, p210, yuv444p, yuv444p10:
  (a) embed_yuv + detect_yuv on the surfaces;
  (b) the same surfaces through torch: yuv.to_rgb -> embed + detect (fp32) -> yuv.from_rgb;
  (c) embed_yuv420 + detect_yuv420 on the 4:2:0 format of the same depth and layout (i420, yuv420p10, nv12, p010) of the same frames.
The condition: for every format median(a) is below median(b) by more than the spread (max - min) of (b).  (a) - (c) is stated next to the
surface bytes the format moves relative to 4:2:0 (4:2:2: 4/3, 4:4:4: 2) and to what its two shell kernels take beyond the 4:2:0 ones, with
the shell kernels' time and fraction of 8 TB/s over their algorithmic bytes (the frame's samples each way + the low-resolution tensors).
usage: tools/bench_yuv.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/yuv_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs
from videoseal_amd import yuv

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (a whole embed + detect of the clip) may not take longer
TWIN_420 = {"yuv422p": "i420", "yuv422p10": "yuv420p10", "nv16": "nv12", "p210": "p010", "yuv444p": "i420", "yuv444p10": "yuv420p10"}
FMTS = tuple(TWIN_420)
BYTES_OVER_420 = {422: round(4 / 3, 4), 444: 2.0}


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
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "yuv_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    Fn, H, W = (8, 256, 256) if QUICK else (32, 768, 768)
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.chunk_size, model.step_size, model.video_mode = 8, 4, "repeat"          # 32 frames per chunk, key frames every 4
    x = synthetic_frames(Fn, H, W, seed=123)
    msgs = synthetic_msgs(1, model.embedder.cfg.nbits, seed=123)
    clips = {fmt: tuple(p.to(dev) for p in yuv.from_rgb(x, fmt)) for fmt in FMTS + tuple(sorted(set(TWIN_420.values())))}      # the decoder's surfaces

    def route_a(fmt):
        def run():
            w = model.embed_yuv(clips[fmt], fmt, msgs, lowres_attenuation=True)["planes_w"]
            return w, model.detect_yuv(w, fmt)["preds"]
        return run

    def route_b(fmt):
        def run():
            w = model.embed(yuv.to_rgb(clips[fmt], fmt), msgs, is_video=True, lowres_attenuation=True)["imgs_w"]
            p = model.detect(w, is_video=True)["preds"]
            return yuv.from_rgb(w, fmt), p
        return run

    def route_c(fmt):
        def run():
            w = model.embed_yuv420(clips[fmt], fmt, msgs, lowres_attenuation=True)["planes_w"]
            return w, model.detect_yuv420(w, fmt)["preds"]
        return run

    routes = {f"c_{f}": route_c(f) for f in sorted(set(TWIN_420.values()))}
    for fmt in FMTS:
        routes[f"a_{fmt}"] = route_a(fmt)
        routes[f"b_{fmt}_via_torch"] = route_b(fmt)
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every route alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    shell = {}
    for name in [k for k in routes if k[:2] in ("a_", "c_")]:
        shell.update({k: v for k, v in shell_records(model, routes[name]).items() if k not in shell})

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}
    look = {}
    for fmt in FMTS:
        a, b, c = res[f"a_{fmt}"], res[f"b_{fmt}_via_torch"], res[f"c_{TWIN_420[fmt]}"]
        own = {k.split("<")[0]: v["us"] for k, v in shell.items() if f"<{fmt}>" in k}
        twin = {k.split("<")[0]: v["us"] for k, v in shell.items() if f"<{TWIN_420[fmt]}>" in k}
        look[fmt] = {
            "condition": "median(a) < median(b) - spread(b)",
            "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 3), "spread_b_ms": b["spread_ms"],
            "holds": bool(a["median_ms"] < b["median_ms"] - b["spread_ms"]),
            "twin_420": TWIN_420[fmt], "a_minus_c_ms": round(a["median_ms"] - c["median_ms"], 3), "spread_c_ms": c["spread_ms"],
            "a_minus_c_exceeds_spread_c": bool(a["median_ms"] - c["median_ms"] > c["spread_ms"]),
            "surface_bytes_over_420": BYTES_OVER_420[yuv.fmt_info(fmt)[3]],
            "shell_kernels_minus_twin_us": {k: round(own[k] - twin[k], 1) for k in own if k in twin},
        }
    doc = {
        "tool": "tools/bench_yuv.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"frames": Fn, "H": H, "W": W, "model": "videoseal_1.0", "video_mode": "repeat", "step_size": 4, "chunk_size": 8,
                     "lowres_attenuation": True, "resident": "HBM", "repeats": repeats, "quick": QUICK},
        "routes_ms_per_step": res,
        "what_to_look_for": look,
        "all_conditions_hold": all(v["holds"] for v in look.values()),
        "a_over_b": {fmt: round(res[f"a_{fmt}"]["median_ms"] / res[f"b_{fmt}_via_torch"]["median_ms"], 4) for fmt in FMTS},
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
