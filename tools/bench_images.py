#!/usr/bin/env python
"""Lists of images of different sizes on the HIP path (Videoseal.embed_images / detect_images) against the route a caller had before, in ONE
process: seeded inputs, warmed up, device events, the routes alternating, every timed step under its own time limit (the protocol of
tools/bench_yuv.py).

Scenario: VideoSeal 1.0 at its released processing size, 32 device-resident fp32 images whose sides come from a seeded list spanning 256 to
1024 pixels (non-square, sides that are no multiple of 4 included), image mode.  Per step (embed + detect of all 32):
  (a) embed_images + detect_images on the list;
  (b) the per-image loop: embed + detect (is_video=False) at batch 1 on the same tensors;
  (c) embed + detect on 32 x 768^2 in image mode -- orientation only: what an equal-size batch costs on this box.
The condition: median(a) is below median(b) by more than the spread (max - min) of (b).  Also written down: kernel launches per step of (a) and
(b) (shell launches from the plan / the loop; all launches from the profiler where it is available) and the two image-list kernels' time beside
the sum of the per-image launches they replace.
usage: tools/bench_images.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/images_bench.json)"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs
from videoseal_amd import native as N

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (embed + detect of the whole list) may not take longer
SIZE_SEED = 2024


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
            us, nb, cnt = rec.get(name, (0.0, 0, 0))
            rec[name] = (us + a.elapsed_time(b) * 1e3, nb + nbytes, cnt + 1)
    finally:
        eng.shell_timers = None
    return {k: {"us": round(us, 1), "calls": cnt, "bytes": nb, "frac_of_8TBs": round(nb / (us * 1e-6) / PEAK, 4)} for k, (us, nb, cnt) in rec.items()}


def kernel_launches(fn):
    """device kernels of one pass of fn(), counted by the profiler (None where it is not available)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            limited(fn, "launch count pass")
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()
                and not e.name.lower().startswith(("memcpy", "memset")))
        return n or None
    except Exception:          # noqa: BLE001 -- a count, not a result
        return None


def main():
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "images_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    n = 8 if QUICK else 32
    rng = random.Random(SIZE_SEED)
    sizes = [(rng.randint(256, 1024), rng.randint(256, 1024)) for _ in range(n)]
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.chunk_size = 32
    S = int(model.img_size)
    imgs = [synthetic_frames(1, h, w, seed=300 + i)[0].to(dev).contiguous() for i, (h, w) in enumerate(sizes)]
    msgs = synthetic_msgs(n, model.embedder.cfg.nbits, seed=123)
    side_c = 256 if QUICK else 768
    batch_c = synthetic_frames(n, side_c, side_c, seed=123).to(dev)

    def route_a():
        w = model.embed_images(imgs, msgs)["imgs_w"]
        return w, model.detect_images(w)["preds"]

    def route_b():
        w = [model.embed(t[None], msgs[i:i + 1], is_video=False)["imgs_w"] for i, t in enumerate(imgs)]
        return w, [model.detect(t, is_video=False)["preds"] for t in w]

    def route_c():
        w = model.embed(batch_c, msgs, is_video=False)["imgs_w"]
        return w, model.detect(w, is_video=False)["preds"]

    routes = {"a_images": route_a, "b_per_image_loop": route_b, "c_equal_size_batch": route_c}
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification, graph capture per shape
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every route alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    graphs, model.use_graphs = model.use_graphs, False      # (a replayed hipGraph has no per-call events: the shell timing pass runs eagerly)
    try:
        shell = {name: shell_records(model, fn) for name, fn in routes.items() if name[0] in "ab"}
    finally:
        model.use_graphs = graphs
    launches = {name: kernel_launches(fn) for name, fn in routes.items() if name[0] in "ab"}

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}
    a, b = res["a_images"], res["b_per_image_loop"]
    plans = {"embed resize": N.images_plan(sizes, N.IMAGES_RESIZE, False, S, S, True), "embed tail": N.images_plan(sizes, N.IMAGES_TAIL, False, S, S, True),
             "detect resize": N.images_plan(sizes, N.IMAGES_RESIZE, False, S, S, True)}
    sa, sb = shell["a_images"], shell["b_per_image_loop"]
    doc = {
        "tool": "tools/bench_images.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"images": n, "sizes_hw": sizes, "size_seed": SIZE_SEED, "model": "videoseal_1.0", "processing_size": S, "dtype": "float32",
                     "lowres_attenuation": False, "resident": "HBM", "repeats": repeats, "quick": QUICK, "c_batch": [n, side_c, side_c]},
        "routes_ms_per_step": res,
        "what_to_look_for": {
            "condition": "median(a) < median(b) - spread(b)", "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 3), "spread_b_ms": b["spread_ms"],
            "holds": bool(a["median_ms"] < b["median_ms"] - b["spread_ms"]), "a_over_b": round(a["median_ms"] / b["median_ms"], 4),
        },
        "launches_per_step": {
            "a_shell": {k: len(v) for k, v in plans.items()}, "a_shell_forms": {k: [g[0] for g in v] for k, v in plans.items()},
            "b_shell": {"embed resize": n, "embed tail": n, "detect resize": n},
            "a_all_kernels": launches["a_images"], "b_all_kernels": launches["b_per_image_loop"],
        },
        "shell_kernels_us": {
            "resize": {"a_images_kernels": sa.get("resize_pre_images_kernel", {}).get("us"), "b_sum_of_per_image_launches": sb.get("resize_pre_kernel", {}).get("us")},
            "tail": {"a_images_kernels": sa.get("embed_tail_images_kernel", {}).get("us"), "b_sum_of_per_image_launches": sb.get("embed_tail_kernel", {}).get("us")},
            "note": "resize: embed + detect of the step; times are event pairs around each call, launch overhead of back-to-back calls included",
        },
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
