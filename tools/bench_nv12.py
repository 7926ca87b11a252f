#!/usr/bin/env python
"""NV12 clips on the HIP path (Videoseal.embed_nv12 / detect_nv12) against the routes a caller has today, in ONE process: seeded inputs,
warmed up, device events, the three routes alternating, every timed step under its own time limit.

Scenario: VideoSeal 1.0, 32 x 768^2 frames resident in HBM, video mode, key frames every 4.  Per step (embed + detect of the clip):
  (a) embed_nv12 + detect_nv12 on the NV12 surfaces;
  (b) today's route for the same surfaces: torch nv12_to_rgb -> RGB24 -> embed_u8 + detect_u8 -> torch rgb_to_nv12;
  (c) embed_u8 + detect_u8 alone on RGB24 frames.
The condition: (a) is not slower than (c) by more than the spread of (c) over its own repeats in this process; the json states the spread,
and where the condition fails, the shell kernel that costs the difference.  The two NV12 shell kernels are listed with their time and the
fraction of 8 TB/s over their algorithmic bytes (1.5 B per pixel each way + the low-resolution tensors) beside resize_pre_kernel<u8> and
embed_tail_kernel<u8> from the same process.
usage: tools/bench_nv12.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/nv12_bench.json)
       tools/bench_nv12.py --sweep [--out FILE]                       (strip heights of the NV12 resize; default profiles/nv12_resize_strip_sweep.json)"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs
from videoseal_amd import nv12

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (a whole embed + detect of the clip) may not take longer


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


class StepTimeout(RuntimeError):
    pass


def limited(fn, what):
    """run fn(), then wait for the device by polling an event against a deadline: a blocking synchronize would keep the interpreter from ever
    noticing that a kernel hangs; here the run ends with StepTimeout after STEP_LIMIT_S"""
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


def sweep(out_path):
    """us per launch of vs_resize_pre_nv12 at 768^2 -> 256^2 for the tile form and the row-streaming form at every strip height, for the launch
    shapes of the scenario (8-frame detect chunks, 16 frames, the 32-frame embed launch with key frames): what the strip rule in yuv420.hip follows"""
    from videoseal_amd import native as N
    lib = N.lib()
    _, inv = nv12.color_affine()
    dec = (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)])
    ym = (C.c_float * 3)(0.299, 0.587, 0.114)
    g = torch.Generator().manual_seed(7)
    res = {}
    for B, want_key in ((8, False), (16, False), (32, True)):
        clip = torch.randint(0, 256, (B, 1152, 768), generator=g, dtype=torch.uint8).cuda()
        rgb = torch.empty(B, 256, 256, 4, device="cuda")
        key = torch.empty((B + 3) // 4, 256, 256, 4, device="cuda") if want_key else None

        def run():
            N.check(lib.vs_resize_pre_nv12(clip.data_ptr(), B, 768, 768, 768, 1152 * 768, dec, 256, 256, 1, rgb.data_ptr(), 2.0, -1.0,
                                           N.ptr(key), 4, ym, None), "vs_resize_pre_nv12")
        for form, strip in [("tile", 0), ("stream", 0)] + [("stream", s) for s in (8, 12, 16, 24, 32, 48, 64)]:
            with N.debug("RESIZE_FORM", 1 if form == "tile" else 0), N.debug("RESIZE_STRIP", strip):
                limited(lambda: [run() for _ in range(5)], "sweep warm-up")
                ms = timed_ms(lambda: [run() for _ in range(50)], "sweep")
            name = form if form == "tile" else ("stream, default strip" if strip == 0 else f"stream, strip {strip}")
            res.setdefault(f"{B} frames" + (" + key frames" if want_key else ""), {})[name] = round(ms / 50 * 1e3, 1)
    doc = {"tool": "tools/bench_nv12.py --sweep", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
           "what": "us per launch of vs_resize_pre_nv12, 768x768 -> 256x256, antialias, 50 launches per figure", "us_per_launch": res}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def shell_records(model, fn):
    """{kernel name: (us, algorithmic bytes)} of the shell kernels of one untimed pass of fn()"""
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
    if "--sweep" in sys.argv:
        return sweep(_arg("--out", os.path.join(ROOT, "profiles", "nv12_resize_strip_sweep.json")))
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "nv12_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    Fn, H, W = (8, 256, 256) if QUICK else (32, 768, 768)
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.chunk_size, model.step_size, model.video_mode = 8, 4, "repeat"          # 32 frames per chunk, key frames every 4
    x = synthetic_frames(Fn, H, W, seed=123)
    msgs = synthetic_msgs(1, model.embedder.cfg.nbits, seed=123)
    clip = nv12.rgb_to_nv12(x).to(dev)                                            # the decoder's surfaces
    rgb24 = (nv12.nv12_to_rgb(clip.cpu()) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)

    def route_a():
        w = model.embed_nv12(clip, msgs, lowres_attenuation=True)["imgs_w"]
        return w, model.detect_nv12(w)["preds"]

    def route_b():
        u8 = (nv12.nv12_to_rgb(clip) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        w = model.embed_u8(u8, msgs, lowres_attenuation=True)["imgs_w"]
        p = model.detect_u8(w)["preds"]
        return nv12.rgb_to_nv12(w.permute(0, 3, 1, 2).float() / 255.0), p

    def route_c():
        w = model.embed_u8(rgb24, msgs, lowres_attenuation=True)["imgs_w"]
        return w, model.detect_u8(w)["preds"]

    routes = {"a_nv12": route_a, "b_nv12_via_rgb24": route_b, "c_rgb24": route_c}
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every route alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    # the two halves of (a) and (c) on their own: which of them carries a difference
    w_a, w_c = route_a()[0], route_c()[0]
    halves = {"a_embed": lambda: model.embed_nv12(clip, msgs, lowres_attenuation=True), "a_detect": lambda: model.detect_nv12(w_a),
              "c_embed": lambda: model.embed_u8(rgb24, msgs, lowres_attenuation=True), "c_detect": lambda: model.detect_u8(w_c)}
    hms = {k: [] for k in halves}
    for _ in range(repeats):
        for name, fn in halves.items():
            hms[name].append(timed_ms(fn, name))
    shell = {}
    shell.update(shell_records(model, route_a))
    shell.update({k: v for k, v in shell_records(model, route_c).items() if k not in shell})

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}
    a, c = res["a_nv12"], res["c_rgb24"]
    gap = a["median_ms"] - c["median_ms"]
    holds = gap <= c["spread_ms"]
    pairs = [("resize_pre_yuv_kernel<nv12>", "resize_pre_kernel<u8>"), ("embed_tail_yuv_kernel<nv12>", "embed_tail_kernel<u8>")]
    kernel_gaps = {n: round(shell[n]["us"] - shell[u]["us"], 1) for n, u in pairs if n in shell and u in shell}
    doc = {
        "tool": "tools/bench_nv12.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"frames": Fn, "H": H, "W": W, "model": "videoseal_1.0", "video_mode": "repeat", "step_size": 4, "chunk_size": 8,
                     "lowres_attenuation": True, "resident": "HBM", "repeats": repeats, "quick": QUICK},
        "routes_ms_per_step": res,
        "condition": {"text": "median(a) - median(c) <= spread of (c) over its own repeats (max - min)", "a_minus_c_ms": round(gap, 3),
                      "spread_c_ms": c["spread_ms"], "holds": bool(holds),
                      "kernel_us_nv12_minus_u8": kernel_gaps,
                      "costliest_kernel": (max(kernel_gaps, key=kernel_gaps.get) if kernel_gaps and not holds else None)},
        "halves_median_ms": {k: round(sorted(v)[len(v) // 2], 3) for k, v in hms.items()},
        "a_over_b": round(a["median_ms"] / res["b_nv12_via_rgb24"]["median_ms"], 4),
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
