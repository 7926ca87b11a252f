#!/usr/bin/env python
"""Lists of clips on the HIP path (Videoseal.embed_clips / detect_clips) against the route a caller had before, in ONE process: seeded inputs,
warmed up, device events, the routes alternating, every timed step under its own time limit (the protocol of tools/bench_images.py).

Scenario: VideoSeal 1.0 at its released processing size, eight device-resident fp32 clips of 16 frames whose sides come from a seeded list
between 360 and 768 pixels (non-square, no multiples of 4 asked), a message per clip, video mode, step_size 4.  Per step (embed + detect):
  (a) embed_clips + detect_clips on the list;
  (b) the per-clip loop: embed + detect (is_video=True) on the same tensors;
  (c) embed_group + detect on 128 frames of 768^2 -- orientation only: what one long clip of the same frame count costs.
The condition: median(b) - median(a) exceeds the spread (max - min) of (b).  Also written down: kernel launches per step of (a) and (b), the two
clip-list kernels' time beside the sum of the per-clip launches they replace, and the register / scratch figures of the clip-list kernels beside
those of the image-list kernels (`--resources-only` compiles csrc/shell.hip and csrc/aggregate.hip for the device with resource remarks and
writes profiles/clips_kernel_resources.json; needs hipcc, no GPU -- the timed run copies that file into its result when it is there).
usage: tools/bench_clips.py [--out FILE] [--quick] [--repeats N] | --resources-only      (default --out profiles/clips_bench.json)"""
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESOURCES = os.path.join(ROOT, "profiles", "clips_kernel_resources.json")

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (embed + detect of the whole list) may not take longer
SIZE_SEED = 2025


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_resources():
    """{kernel: VGPRs, SGPRs, scratch bytes per lane, waves per SIMD, LDS bytes} of the image-list, clip-list and aggregation kernels (gfx950)"""
    csrc = os.path.join(ROOT, "videoseal_amd", "csrc")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ("shell", "aggregate"):
            r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                                "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, unit + ".hip"),
                                "-o", os.path.join(tmp, unit + ".o")], capture_output=True, text=True, check=True)
            for blk in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
                name = blk.split()[0]
                m = re.search(r"(resize_pre|embed_tail)_(images|clips)(_stream)?_kernelI([^E]*)E|(aggregate_clips)_kernel", name)
                if not m:
                    continue
                short = m.group(5) or f"{m.group(1)}_{m.group(2)}{m.group(3) or ''}<{m.group(4)}>"
                f = lambda pat: int(re.search(pat + r": (\d+)", blk).group(1))      # noqa: E731
                out[short] = {"vgprs": f("VGPRs"), "sgprs": f("SGPRs"), "scratch_bytes_per_lane": f(r"ScratchSize \[bytes/lane\]"),
                              "waves_per_simd": f(r"Occupancy \[waves/SIMD\]"), "lds_bytes": f(r"LDS Size \[bytes/block\]")}
    return dict(sorted(out.items()))


if "--resources-only" in sys.argv:
    doc = {"tool": "tools/bench_clips.py --resources-only", "arch": "gfx950",
           "template_arguments": "Itanium spelling: f = float, h = unsigned char, Lb0 / Lb1 = false / true, Li64 / Li128 = 64 / 128", "kernels": kernel_resources()}
    with open(RESOURCES, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))
    sys.exit(0)

import torch  # noqa: E402

import videoseal_amd  # noqa: E402
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from videoseal_amd import clips as CL  # noqa: E402
from videoseal_amd import native as N  # noqa: E402


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
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "clips_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    n, frames = (4, 8) if QUICK else (8, 16)
    rng = random.Random(SIZE_SEED)
    sizes = []
    while len(sizes) < n:
        h, w = rng.randint(360, 768), rng.randint(360, 768)
        if h != w:
            sizes.append((h, w))
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.step_size = 4
    S, step, ck = int(model.img_size), int(model.step_size), int(model.chunk_size)
    clips = [synthetic_frames(frames, h, w, seed=500 + i).to(dev).contiguous() for i, (h, w) in enumerate(sizes)]
    msgs = synthetic_msgs(n, model.embedder.cfg.nbits, seed=321)
    side_c = 256 if QUICK else 768
    long_c = synthetic_frames(n * frames, side_c, side_c, seed=321).to(dev)

    def route_a():
        w = model.embed_clips(clips, msgs)["imgs_w"]
        return w, model.detect_clips(w)["preds"]

    def route_b():
        w = [model.embed(t, msgs[i:i + 1], is_video=True)["imgs_w"] for i, t in enumerate(clips)]
        return w, [model.detect(t, is_video=True)["preds"] for t in w]

    def route_c():
        w = model.embed_group(long_c, msgs[:1], frames)
        return w, model.detect(w, is_video=True)["preds"]

    routes = {"a_clips": route_a, "b_per_clip_loop": route_b, "c_one_long_clip": route_c}
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
    a, b = res["a_clips"], res["b_per_clip_loop"]
    lengths = [frames] * n
    epasses, dpasses = CL.embed_passes(lengths, step, ck), CL.detect_passes(lengths)

    def groups(passes, kind):
        return sum(len(N.clips_plan([(s[2],) + sizes[s[0]] for s in slots], kind, False, S, S, True)) for slots in passes)
    eslots = [p[0] for p in epasses]
    sa, sb = shell["a_clips"], shell["b_per_clip_loop"]
    doc = {
        "tool": "tools/bench_clips.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"clips": n, "frames_per_clip": frames, "sizes_hw": sizes, "size_seed": SIZE_SEED, "model": "videoseal_1.0", "processing_size": S,
                     "dtype": "float32", "step_size": step, "chunk_size": ck, "video_mode": model.video_mode, "lowres_attenuation": False,
                     "resident": "HBM", "repeats": repeats, "quick": QUICK, "c_clip": [n * frames, side_c, side_c]},
        "routes_ms_per_step": res,
        "what_to_look_for": {
            "condition": "median(b) - median(a) > spread(b)", "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 3), "spread_b_ms": b["spread_ms"],
            "holds": bool(b["median_ms"] - a["median_ms"] > b["spread_ms"]), "a_over_b": round(a["median_ms"] / b["median_ms"], 4),
        },
        "passes_per_step": {"a_embed": len(epasses), "a_embed_key_frames": [len(p[1]) for p in epasses], "a_detect": len(dpasses),
                            "b_embed": sum(len(CL.spans([f], step, ck)) for f in lengths), "b_detect": sum(-(-f // ck) for f in lengths)},
        "launches_per_step": {
            "a_shell": {"embed resize": groups(eslots, N.IMAGES_RESIZE), "embed tail": groups(eslots, N.IMAGES_TAIL), "detect resize": groups(dpasses, N.IMAGES_RESIZE)},
            "b_shell": {k: v.get("calls") for k, v in sb.items()},
            "a_all_kernels": launches["a_clips"], "b_all_kernels": launches["b_per_clip_loop"],
        },
        "shell_kernels_us": {
            "resize": {"a_clips_kernels": sa.get("resize_pre_clips_kernel", {}).get("us"), "b_sum_of_per_clip_launches": sb.get("resize_pre_kernel", {}).get("us")},
            "tail": {"a_clips_kernels": sa.get("embed_tail_clips_kernel", {}).get("us"), "b_sum_of_per_clip_launches": sb.get("embed_tail_kernel", {}).get("us")},
            "note": "resize: embed + detect of the step; times are event pairs around each call, launch overhead of back-to-back calls included",
        },
        "shell_kernels": shell,
        "kernel_resources": json.load(open(RESOURCES))["kernels"] if os.path.exists(RESOURCES) else None,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
