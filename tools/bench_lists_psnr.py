#!/usr/bin/env python
"""Target PSNR on lists (Videoseal.embed_images_psnr / embed_clips_psnr) against the fixed-strength list calls and against the route a caller had
before -- a loop of embed_psnr per item -- in ONE process: seeded inputs, warmed up, device events, the legs alternating, every timed step
under its own time limit (the protocol and the inputs of tools/bench_images.py and tools/bench_clips.py: 32 fp32 images with seeded sides of
256 - 1024, eight 16-frame clips of 360 - 768, all resident in HBM; VideoSeal 1.0, target 42 dB).

Legs, images / clips:
  (a) embed_images_psnr                                   / embed_clips_psnr(per="clip")
  (b) embed_images                                        / embed_clips                              (the fixed strength: what the target costs)
  (c) per-image loop of embed_psnr(img[None], is_video=False) / per-clip loop of embed_psnr(per="clip")  (the baseline)
The condition: median(c) - median(a) exceeds the spread (max - min) of (c).  (a) - (b) is written down, not judged.

Per-launch kernel times come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -o lists -- python tools/bench_lists_psnr.py --trace-pass
    python tools/bench_lists_psnr.py --merge-stats DIR/.../lists_kernel_stats.csv      (no GPU: adds "kernels_per_launch" to the result file)
usage: tools/bench_lists_psnr.py [--out FILE] [--quick] [--repeats N] | --trace-pass | --merge-stats CSV   (default --out profiles/lists_psnr_bench.json)"""
import csv
import importlib.util
import json
import os
import random
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
QUICK = "--quick" in sys.argv
TARGET_DB = 42.0
OUT_DEFAULT = os.path.join(ROOT, "profiles", "lists_psnr_bench.json")


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scenario():
    """the sizes of tools/bench_images.py and tools/bench_clips.py (their seeds, their rules)"""
    BI, BC = _tool("bench_images"), _tool("bench_clips")
    n_img = 8 if QUICK else 32
    rng = random.Random(BI.SIZE_SEED)
    img_sizes = [(rng.randint(256, 1024), rng.randint(256, 1024)) for _ in range(n_img)]
    n_clip, frames = (4, 8) if QUICK else (8, 16)
    rng = random.Random(BC.SIZE_SEED)
    clip_sizes = []
    while len(clip_sizes) < n_clip:
        h, w = rng.randint(360, 768), rng.randint(360, 768)
        if h != w:
            clip_sizes.append((h, w))
    return BI, img_sizes, clip_sizes, frames


def algorithmic_bytes(img_sizes, clip_sizes, frames, cd):
    """HBM bytes a launch group cannot avoid, fp32, full-resolution heat-map: the energy pass reads every frame once, the tails read and write it
    (the list calls of the model also store preds_w for images); the processing-size operands are cache hits"""
    ipx = sum(h * w for h, w in img_sizes)
    cpx = frames * sum(h * w for h, w in clip_sizes)
    return {"images": {"energy": 12 * ipx, "tail": 24 * ipx + 4 * cd * ipx}, "clips": {"energy": 12 * cpx, "tail": 24 * cpx}}


def merge_stats(path, out_path):
    """kernel_stats CSV of rocprofv3 (Name, Calls, TotalDurationNs, AverageNs, ...) -> per-launch times of the list kernels in the result file"""
    doc = json.load(open(out_path))
    sc = doc["scenario"]
    nbytes = algorithmic_bytes(sc["image_sizes_hw"], sc["clip_sizes_hw"], sc["frames_per_clip"], sc["Cd"])
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            m = re.search(r"embed_tail_(images|clips)_kernel<.*?(\d)>", name)
            if m:
                key = f"embed_tail_{m.group(1)}_kernel<{('blend', 'scaled', 'energy')[int(m.group(2))]}>"
            elif "tail_list_energy_finish_kernel" in name:
                key = "tail_list_energy_finish_kernel"
            elif "psnr_scale_groups_kernel" in name or "psnr_scale_items_kernel" in name:
                key = "psnr_scale_groups_kernel" if "groups" in name else "psnr_scale_items_kernel"
            else:
                continue
            calls, avg = int(r["Calls"]), float(r.get("AverageNs") or r.get("Average") or 0.0)
            c0, t0 = rows.get(key, (0, 0.0))
            rows[key] = (c0 + calls, t0 + calls * avg)
    per = {}
    for key, (calls, tot) in sorted(rows.items()):
        us = tot / calls / 1e3
        per[key] = {"launches": calls, "avg_us": round(us, 2)}
        m = re.match(r"embed_tail_(images|clips)_kernel<(\w+)>", key)
        if m:       # one launch group covers the whole list in this scenario (32 images; eight clips in one pass)
            b = nbytes[m.group(1)]["energy" if m.group(2) == "energy" else "tail"]
            per[key].update({"algorithmic_bytes": b, "frac_of_8TBs": round(b / (us * 1e-6) / PEAK, 4)})
    doc["kernels_per_launch"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (--trace-pass)", "kernels": per}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["kernels_per_launch"]))


def main():
    out_path = _arg("--out", OUT_DEFAULT)
    if "--merge-stats" in sys.argv:
        return merge_stats(_arg("--merge-stats", ""), out_path)
    import torch

    import videoseal_amd
    from oracle.inputs import synthetic_frames, synthetic_msgs
    BI, img_sizes, clip_sizes, frames = scenario()
    repeats = _arg("--repeats", 3 if QUICK else 7)
    dev = torch.device("cuda:0")
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    imgs = [synthetic_frames(1, h, w, seed=300 + i)[0].to(dev).contiguous() for i, (h, w) in enumerate(img_sizes)]
    clips = [synthetic_frames(frames, h, w, seed=500 + i).to(dev).contiguous() for i, (h, w) in enumerate(clip_sizes)]
    mi = synthetic_msgs(len(imgs), model.embedder.cfg.nbits, seed=123)
    mc = synthetic_msgs(len(clips), model.embedder.cfg.nbits, seed=321)
    ck_clips = int(model.chunk_size)

    def images(fn):
        def run():
            model.chunk_size, model.step_size = 32, 1
            return fn()
        return run

    def video(fn):
        def run():
            model.chunk_size, model.step_size = ck_clips, 4
            return fn()
        return run

    legs = {
        "images_a_embed_images_psnr": images(lambda: model.embed_images_psnr(imgs, TARGET_DB, mi)["imgs_w"]),
        "images_b_embed_images": images(lambda: model.embed_images(imgs, mi)["imgs_w"]),
        "images_c_embed_psnr_loop": images(lambda: [model.embed_psnr(t[None], TARGET_DB, mi[i:i + 1], is_video=False)["imgs_w"] for i, t in enumerate(imgs)]),
        "clips_a_embed_clips_psnr": video(lambda: model.embed_clips_psnr(clips, TARGET_DB, mc, per="clip")["imgs_w"]),
        "clips_b_embed_clips": video(lambda: model.embed_clips(clips, mc)["imgs_w"]),
        "clips_c_embed_psnr_loop": video(lambda: [model.embed_psnr(t, TARGET_DB, mc[i:i + 1], per="clip")["imgs_w"] for i, t in enumerate(clips)]),
    }
    step0 = int(model.step_size)
    try:
        for name, fn in legs.items():                       # warm-up: workspaces, tile tuning, arithmetic verification
            for _ in range(3):
                BI.limited(fn, f"warm-up {name}")
        if "--trace-pass" in sys.argv:                      # under the profiler: the list legs only, three times each
            for name in ("images_a_embed_images_psnr", "images_b_embed_images", "clips_a_embed_clips_psnr", "clips_b_embed_clips"):
                for _ in range(3):
                    BI.limited(legs[name], name)
            torch.cuda.synchronize()
            print(json.dumps({"trace_pass": "done"}))
            return
        ms = {k: [] for k in legs}
        for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every leg alike
            for name, fn in legs.items():
                ms[name].append(BI.timed_ms(fn, name))
        shell = {name: BI.shell_records(model, fn) for name, fn in legs.items() if "_c_" not in name}
    finally:
        model.chunk_size, model.step_size = ck_clips, step0

    def summary(v):
        s = sorted(v)
        return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
                "all_ms": [round(t, 3) for t in v]}
    res = {k: summary(v) for k, v in ms.items()}

    def verdict(kind):
        a, b, c = (res[k] for k in legs if k.startswith(kind))
        return {"condition": "median(c) - median(a) > spread(c)", "c_minus_a_ms": round(c["median_ms"] - a["median_ms"], 3), "spread_c_ms": c["spread_ms"],
                "holds": bool(c["median_ms"] - a["median_ms"] > c["spread_ms"]), "a_over_c": round(a["median_ms"] / c["median_ms"], 4),
                "a_minus_b_ms": round(a["median_ms"] - b["median_ms"], 3), "a_over_b": round(a["median_ms"] / b["median_ms"], 4)}
    doc = {
        "tool": "tools/bench_lists_psnr.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"images": len(imgs), "image_sizes_hw": img_sizes, "clips": len(clips), "frames_per_clip": frames, "clip_sizes_hw": clip_sizes,
                     "model": "videoseal_1.0", "processing_size": int(model.img_size), "Cd": int(model.embedder.cfg.out_ch), "dtype": "float32",
                     "target_psnr_db": TARGET_DB, "lowres_attenuation": False, "resident": "HBM", "repeats": repeats, "quick": QUICK,
                     "images_chunk_size": 32, "clips_step_size": 4, "clips_chunk_size": ck_clips},
        "legs_ms_per_step": res,
        "what_to_look_for": {"images": verdict("images"), "clips": verdict("clips")},
        "shell_kernels": shell,
        "shell_kernels_note": "event pairs around each engine call, launch overhead included; *_energy_kernel covers the energy pass and its finish launch",
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
