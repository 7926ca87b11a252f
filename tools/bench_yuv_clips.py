#!/usr/bin/env python
"""Lists of YUV clips (Videoseal.embed_clips_yuv / detect_clips_yuv) against the routes a caller had before, in ONE process: seeded inputs,
warmed up, device events, the routes alternating, every timed step under its own time limit (the protocol of tools/bench_clips.py).

Scenario: VideoSeal 1.0, eight clips of 16 frames with seeded EVEN sides between 360 and 768, resident in HBM as decoder surfaces, step_size 4,
the default low-resolution heat-map.  Per step (embed + detect of all clips), for nv12 and for p010:
  (a) embed_clips_yuv + detect_clips_yuv on the list;
  (b) the per-clip loop embed_yuv + detect_yuv on the same planes;
  (c) embed_clips + detect_clips on the same frames as RGB24 -- for orientation only (another surface: 3 bytes per pixel, 8 bits).
The condition: median(b) - median(a) exceeds the spread (max - min) of (b), per format.  Also written down: (a) / (b), network passes and
kernel launches per step, the list resize and list tail beside the sum of the per-clip launches they replace (event pairs around each call;
the list tail runs the 16-row tile kernel where the per-clip call streams rows), and the register / LDS / scratch figures of the list kernels
(--resources-only, needs no GPU: profiles/yuv_clips_kernel_resources.json).
Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o yc -- python tools/bench_yuv_clips.py --trace-pass
    python tools/bench_yuv_clips.py --merge-stats DIR/.../yc_kernel_stats.csv      (adds "kernels_per_step" to the result file; needs no GPU)
usage: tools/bench_yuv_clips.py [--out FILE] [--quick] [--repeats N] | --resources-only | --trace-pass | --merge-stats CSV
(default --out profiles/yuv_clips_bench.json)"""
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
RESOURCES = os.path.join(ROOT, "profiles", "yuv_clips_kernel_resources.json")
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step (embed + detect of the whole list) may not take longer
SIZE_SEED = 2026
FMTS = ("nv12", "p010")


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_resources():
    """{kernel: VGPRs, SGPRs, scratch bytes per lane, waves per SIMD, static LDS bytes} of the 40 list instantiations (gfx950)"""
    csrc = os.path.join(ROOT, "videoseal_amd", "csrc")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                            "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "yuv_clips.hip"),
                            "-o", os.path.join(tmp, "yuv_clips.o")], capture_output=True, text=True, check=True)
    names = {(0, 8, 0, 1, 1): "nv12", (1, 8, 0, 1, 1): "i420", (0, 10, 1, 1, 1): "p010", (1, 10, 0, 1, 1): "yuv420p10", (0, 8, 0, 1, 0): "nv16",
             (1, 8, 0, 1, 0): "yuv422p", (0, 10, 1, 1, 0): "p210", (1, 10, 0, 1, 0): "yuv422p10", (1, 8, 0, 0, 0): "yuv444p", (1, 10, 0, 0, 0): "yuv444p10"}
    for blk in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        m = re.search(r"(resize_pre_yuv_stream|resize_pre_yuv|embed_tail_yuv)_kernelINS_4SurfILb(\d)ELi(\d+)ELb(\d)ELi(\d)ELi(\d)E.*?E(Li(\d+)E)?NS_1[12]YuvClips", name)
        if not m:
            continue
        fmt = names[tuple(int(m.group(i)) for i in (2, 3, 4, 5, 6))]
        f = lambda pat: int(re.search(pat + r": (\d+)", blk).group(1))      # noqa: E731
        out[f"{m.group(1)}_clips{'_' + m.group(8) if m.group(8) else ''}<{fmt}>"] = {
            "vgprs": f("VGPRs"), "sgprs": f("SGPRs"), "scratch_bytes_per_lane": f(r"ScratchSize \[bytes/lane\]"),
            "waves_per_simd": f(r"Occupancy \[waves/SIMD\]"), "static_lds_bytes": f(r"LDS Size \[bytes/block\]")}
    return dict(sorted(out.items()))


if "--resources-only" in sys.argv:
    k = kernel_resources()
    doc = {"tool": "tools/bench_yuv_clips.py --resources-only", "arch": "gfx950", "instantiations": len(k),
           "max_scratch_bytes_per_lane": max(v["scratch_bytes_per_lane"] for v in k.values()), "kernels": k}
    with open(RESOURCES, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))
    sys.exit(0)

TRACE_STEPS = 5             # passes of every route in --trace-pass (the first two are its warm-up; the shell kernels cost the same in all)


def merge_stats(path, out_path):
    """kernel_stats CSV of rocprofv3 (Name, Calls, TotalDurationNs, ...) -> per step, the list resize and list tail beside the sum of the
    per-clip launches they replace, per format"""
    import csv
    names = {("false", "8", "false", "1", "1"): "nv12", ("false", "10", "true", "1", "1"): "p010"}
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            m = re.search(r"(resize_pre_yuv_stream|resize_pre_yuv|embed_tail_yuv_stream|embed_tail_yuv)_kernel<.*?Surf<(\w+), (\d+), (\w+), (\d), (\d)", name)
            if not m or m.groups()[1:] not in names:
                continue
            key = (names[m.groups()[1:]], "resize" if m.group(1).startswith("resize") else "tail", "list" if "YuvClips" in name else "per_clip")
            c0, t0 = rows.get(key, (0, 0.0))
            rows[key] = (c0 + int(r["Calls"]), t0 + float(r.get("TotalDurationNs") or 0.0))
    per = {}
    for (fmt, what, form), (calls, tot) in sorted(rows.items()):
        per.setdefault(fmt, {}).setdefault(what, {})[form] = {"launches_per_step": calls / TRACE_STEPS, "us_per_step": round(tot / TRACE_STEPS / 1e3, 1)}
    doc = json.load(open(out_path))
    doc["kernels_per_step"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (--trace-pass); resize: embed + detect of the step; "
                                         "per_clip: the sum over the launches of the per-clip loop (tail: its row-streaming form)", "formats": per}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["kernels_per_step"]))


if "--merge-stats" in sys.argv:
    merge_stats(_arg("--merge-stats", ""), _arg("--out", os.path.join(ROOT, "profiles", "yuv_clips_bench.json")))
    sys.exit(0)

import torch  # noqa: E402

import videoseal_amd  # noqa: E402
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from videoseal_amd import clips as CL  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import yuv  # noqa: E402


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
    """{kernel name: us, calls} of the shell kernels of one untimed pass of fn()"""
    eng = model._engine()
    eng.shell_timers = []
    try:
        limited(fn, "shell timing pass")
        rec = {}
        for name, a, b, _ in eng.shell_timers:
            us, cnt = rec.get(name, (0.0, 0))
            rec[name] = (us + a.elapsed_time(b) * 1e3, cnt + 1)
    finally:
        eng.shell_timers = None
    return {k: {"us": round(us, 1), "calls": cnt} for k, (us, cnt) in rec.items()}


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
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "yuv_clips_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    n, frames = (4, 8) if QUICK else (8, 16)
    rng = random.Random(SIZE_SEED)
    sizes = []
    while len(sizes) < n:
        h, w = 2 * rng.randint(180, 384), 2 * rng.randint(180, 384)
        if h != w:
            sizes.append((h, w))
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.step_size = 4
    S, step, ck = int(model.img_size), int(model.step_size), int(model.chunk_size)
    rgb = [synthetic_frames(frames, h, w, seed=500 + i) for i, (h, w) in enumerate(sizes)]
    msgs = synthetic_msgs(n, model.embedder.cfg.nbits, seed=321)
    planes = {fmt: [tuple(p.to(dev) for p in yuv.from_rgb(x, fmt)) for x in rgb] for fmt in FMTS}          # the decoder's surfaces
    rgb24 = [(x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev) for x in rgb]

    def route_a(fmt):
        def run():
            w = model.embed_clips_yuv(planes[fmt], fmt, msgs)["planes_w"]
            return w, model.detect_clips_yuv(w, fmt)["preds"]
        return run

    def route_b(fmt):
        def run():
            w = [model.embed_yuv(p, fmt, msgs[i:i + 1])["planes_w"] for i, p in enumerate(planes[fmt])]
            return w, [model.detect_yuv(p, fmt)["preds"] for p in w]
        return run

    def route_c():
        w = model.embed_clips(rgb24, msgs, lowres_attenuation=True)["imgs_w"]
        return w, model.detect_clips(w)["preds"]

    routes = {"c_rgb24_clips": route_c}
    for fmt in FMTS:
        routes[f"a_{fmt}_clips"] = route_a(fmt)
        routes[f"b_{fmt}_per_clip_loop"] = route_b(fmt)
    if "--trace-pass" in sys.argv:                      # under rocprofv3: TRACE_STEPS passes of (a) and (b), nothing timed here
        for name, fn in routes.items():
            if name[0] in "ab":
                for i in range(TRACE_STEPS):
                    limited(fn, f"trace pass {name} {i}")
        torch.cuda.synchronize()
        return
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
    lengths = [frames] * n
    epasses, dpasses = CL.embed_passes(lengths, step, ck), CL.detect_passes(lengths)

    def groups(fmt, passes, kind):
        return sum(len(N.yuv_clips_plan([(s[2],) + sizes[s[0]] for s in slots], fmt, kind, S, S, True)) for slots in passes)
    eslots = [p[0] for p in epasses]
    look, per_fmt = {}, {}
    for fmt in FMTS:
        a, b = res[f"a_{fmt}_clips"], res[f"b_{fmt}_per_clip_loop"]
        sa, sb = shell[f"a_{fmt}_clips"], shell[f"b_{fmt}_per_clip_loop"]
        look[fmt] = {"condition": "median(b) - median(a) > spread(b)", "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 3),
                     "spread_b_ms": b["spread_ms"], "holds": bool(b["median_ms"] - a["median_ms"] > b["spread_ms"]),
                     "a_over_b": round(a["median_ms"] / b["median_ms"], 4)}
        per_fmt[fmt] = {
            "launches_per_step": {
                "a_shell": {"embed resize": groups(fmt, eslots, N.IMAGES_RESIZE), "embed tail": groups(fmt, eslots, N.IMAGES_TAIL),
                            "detect resize": groups(fmt, dpasses, N.IMAGES_RESIZE)},
                "b_shell": {k: v["calls"] for k, v in sb.items()},
                "a_all_kernels": launches[f"a_{fmt}_clips"], "b_all_kernels": launches[f"b_{fmt}_per_clip_loop"]},
            "shell_kernels_us": {
                "resize": {"a_list_kernels": sa.get(f"resize_pre_yuv_clips_kernel<{fmt}>", {}).get("us"),
                           "b_sum_of_per_clip_launches": sb.get(f"resize_pre_yuv_kernel<{fmt}>", {}).get("us")},
                "tail": {"a_list_kernels": sa.get(f"embed_tail_yuv_clips_kernel<{fmt}>", {}).get("us"),
                         "b_sum_of_per_clip_launches": sb.get(f"embed_tail_yuv_kernel<{fmt}>", {}).get("us")},
                "note": "resize: embed + detect of the step; event pairs around each call, launch overhead of back-to-back calls included; the list "
                        "tail is the 16-row tile kernel, the per-clip tail streams rows"},
        }
    doc = {
        "tool": "tools/bench_yuv_clips.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"clips": n, "frames_per_clip": frames, "sizes_hw": sizes, "size_seed": SIZE_SEED, "model": "videoseal_1.0", "processing_size": S,
                     "formats": FMTS, "step_size": step, "chunk_size": ck, "video_mode": model.video_mode, "lowres_attenuation": True,
                     "resident": "HBM", "repeats": repeats, "quick": QUICK},
        "routes_ms_per_step": res,
        "what_to_look_for": look,
        "all_conditions_hold": all(v["holds"] for v in look.values()),
        "passes_per_step": {"a_embed": len(epasses), "a_embed_key_frames": [len(p[1]) for p in epasses], "a_detect": len(dpasses),
                            "b_embed": sum(len(CL.spans([f], step, ck)) for f in lengths), "b_detect": sum(-(-f // ck) for f in lengths)},
        "per_format": per_fmt,
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
