#!/usr/bin/env python
"""Region-wise watermarks (Videoseal.embed_regions / decode_regions) against the routes a caller had before, in ONE process: seeded inputs,
warmed up, device events, the legs alternating, every timed step under its own time limit (the protocol of tools/bench_psnr.py).

Embed: VideoSeal 1.0, 32 x 768^2 fp32 frames resident in HBM, video mode, key frames every 4, 32 frames per chunk, R = 4 regions; two label
maps: quadrants (a region edge on few tiles) and 64-pixel vertical stripes (every tile of the tail holds all four labels).
  (a) embed_regions
  (b) four `embed` calls on the same frames composed with torch.where over full-resolution frames
  (c) one plain `embed`
Decode: the architecture of `convnext_tiny_pw` (96 bits, head [4, 4, 2], 256^2 maps), 32 frames of 256^2, R = 4 quadrants.
  (a) decode_regions
  (b) `detect`, then four pixel_vote calls with the masks of the regions on the same maps
  and the vote alone on resident maps: one vs_pixel_vote_regions launch against four vs_pixel_vote launches.
Conditions, relative and read from the run itself: median(a) is below median(b) by more than the spread (max - min) of (b).  Reported beside
them: (a) - (c), the tail launches of (a) and (c) with their fraction of 8 TB/s over algorithmic bytes (the label map is one more byte
per pixel read), the vote launch as a fraction of 8 TB/s over one read of the maps.  Nothing is tuned to the comparison: a condition that
does not hold is reported with its numbers.
usage: tools/bench_regions.py [--out FILE] [--quick] [--repeats N]       (GPU box; default --out profiles/regions_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import videoseal_amd
from oracle.inputs import synthetic_frames, synthetic_msgs
from videoseal_amd import regions as RG
from videoseal_amd.layout import ModelCfg
from videoseal_amd.model import build_model
from videoseal_amd.pixel_head import pixel_vote

PEAK = 8.0e12
QUICK = "--quick" in sys.argv
STEP_LIMIT_S = 120          # one timed step may not take longer
R = 4


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


def label_maps(Fn, H, W, dev):
    quad = torch.zeros(Fn, H, W, dtype=torch.uint8)
    quad[:, : H // 2, : W // 2], quad[:, : H // 2, W // 2:], quad[:, H // 2:, : W // 2], quad[:, H // 2:, W // 2:] = 1, 2, 3, 4
    stripes = ((torch.arange(W) // 64) % R + 1).to(torch.uint8)[None, None, :].expand(Fn, H, W).contiguous()
    return {"quadrants": quad.to(dev), "stripes64": stripes.to(dev)}


def summary(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "spread_ms": round(s[-1] - s[0], 3),
            "all_ms": [round(t, 3) for t in v]}


def below(a, b):
    return {"condition": "median(a) < median(b) - spread(b)", "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 3), "spread_b_ms": b["spread_ms"],
            "holds": bool(a["median_ms"] < b["median_ms"] - b["spread_ms"])}


def run_legs(routes, repeats):
    for name, fn in routes.items():                     # warm-up: workspaces, tile tuning, arithmetic verification
        for _ in range(3):
            limited(fn, f"warm-up {name}")
    ms = {k: [] for k in routes}
    for _ in range(repeats):                            # alternating, so that clock and temperature drift hit every leg alike
        for name, fn in routes.items():
            ms[name].append(timed_ms(fn, name))
    return {k: summary(v) for k, v in ms.items()}


def main():
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "regions_bench.json"))
    repeats = _arg("--repeats", 3 if QUICK else 7)
    Fn, H, W = (8, 256, 256) if QUICK else (32, 768, 768)
    dev = torch.device("cuda:0")
    look, shell = {}, {}

    # ---- embed
    model = videoseal_amd.build("videoseal_1.0", seed=0).eval().to(dev)
    model.step_size, model.video_mode, model.chunk_size = 4, "repeat", 8          # 32 frames per chunk: 8 key frames x 4 regions in one U-Net pass
    x = synthetic_frames(Fn, H, W, seed=123).to(dev)
    nbits = model.embedder.cfg.nbits
    msgs = synthetic_msgs(R, nbits, seed=123)
    labels = label_maps(Fn, H, W, dev)

    def four_embeds(lab):
        out = x
        sel = lab[:, None]
        for r in range(R):
            out = torch.where(sel == r + 1, model.embed(x, msgs[r:r + 1], is_video=True)["imgs_w"], out)
        return out
    routes = {"embed.c_plain_embed": lambda: model.embed(x, msgs[:1], is_video=True)["imgs_w"]}
    for tag, lab in labels.items():
        routes[f"embed.{tag}.a_embed_regions"] = lambda lab=lab: model.embed_regions(x, lab, msgs, is_video=True)["imgs_w"]
        routes[f"embed.{tag}.b_four_embeds_where"] = lambda lab=lab: four_embeds(lab)
    res = run_legs(routes, repeats)
    agree = {tag: float((routes[f"embed.{tag}.a_embed_regions"]() - routes[f"embed.{tag}.b_four_embeds_where"]()).abs().max()) for tag in labels}
    shell = {name: shell_records(model, fn) for name, fn in routes.items() if ".b_" not in name}
    c = res["embed.c_plain_embed"]
    for tag in labels:
        a, b = res[f"embed.{tag}.a_embed_regions"], res[f"embed.{tag}.b_four_embeds_where"]
        look[f"embed.{tag}.below_four_embeds"] = below(a, b)
        look[f"embed.{tag}.cost_over_one_embed"] = {
            "a_minus_c_ms": round(a["median_ms"] - c["median_ms"], 3), "spread_c_ms": c["spread_ms"],
            "label_bytes": int(labels[tag].numel()), "labels_at_8TBs_ms": round(labels[tag].numel() / PEAK * 1e3, 4),
            "tail_launches": {"embed_regions": {k: v for k, v in shell[f"embed.{tag}.a_embed_regions"].items() if "tail" in k},
                              "embed": {k: v for k, v in shell["embed.c_plain_embed"].items() if "tail" in k}}}
    del model, routes
    torch.cuda.empty_cache()

    # ---- decode
    S, NB = (64, 16) if QUICK else (256, 96)
    arch = dict(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768])                   # convnext_tiny_pw
    det = build_model(ModelCfg(nbits=NB, hidden=2 * NB, img_size=S, head_stages=[4, 4, 2], head_pixelwise=True, **arch)).eval().to(dev)
    det.chunk_size = 8
    Fd = 8 if QUICK else 32
    y = synthetic_frames(Fd, S, S, seed=124).to(dev)
    lab = label_maps(Fd, S, S, dev)["quadrants"]
    masks = [(lab == r + 1)[:, None].float() for r in range(R)]
    eng = det._engine()

    def detect_and_four_votes():
        p = det.detect(y, is_video=True)["preds"]
        return [pixel_vote(p[:, 1:], m, 0.0) for m in masks]
    preds = det.detect(y, is_video=True)["preds"]
    routes = {"decode.a_decode_regions": lambda: det.decode_regions(y, lab, R=R),
              "decode.b_detect_and_four_votes": detect_and_four_votes,
              "vote.a_one_regions_launch": lambda: eng.pixel_vote_regions(preds[:, 1:], lab, R, 0.0),
              "vote.b_four_pixel_votes": lambda: [pixel_vote(preds[:, 1:], m, 0.0) for m in masks]}
    dres = run_legs(routes, repeats)
    res.update(dres)
    va, vb = eng.pixel_vote_regions(preds[:, 1:], lab, R, 0.0), [pixel_vote(preds[:, 1:], m, 0.0) for m in masks]
    votes_agree = all(torch.equal(va[0][:, r], vb[r][0]) and torch.equal(va[1][:, r], vb[r][1]) for r in range(R))
    look["decode.below_detect_and_four_votes"] = below(dres["decode.a_decode_regions"], dres["decode.b_detect_and_four_votes"])
    look["vote.below_four_pixel_votes"] = below(dres["vote.a_one_regions_launch"], dres["vote.b_four_pixel_votes"])
    nbytes = preds[:, 1:].numel() * 4
    look["vote.fraction_of_8TBs_over_one_read_of_preds"] = {
        "bytes": nbytes, "median_ms": dres["vote.a_one_regions_launch"]["median_ms"],
        "frac_of_8TBs": round(nbytes / (dres["vote.a_one_regions_launch"]["median_ms"] * 1e-3) / PEAK, 4),
        "note": "vs_pixel_vote_regions + its finish launch, as timed by device events around the call"}

    doc = {
        "tool": "tools/bench_regions.py", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "device": torch.cuda.get_device_name(0),
        "scenario": {"embed": {"frames": Fn, "H": H, "W": W, "model": "videoseal_1.0", "video_mode": "repeat", "step_size": 4, "frames_per_chunk": 32,
                               "regions": R, "label_maps": list(labels), "dtype": "fp32, full-resolution JND"},
                     "decode": {"frames": Fd, "S": S, "nbits": NB, "arch": "convnext_tiny_pw", "regions": R, "label_map": "quadrants"},
                     "resident": "HBM", "repeats": repeats, "quick": QUICK},
        "legs_ms_per_step": res,
        "what_to_look_for": look,
        "all_conditions_hold": all(v["holds"] for v in look.values() if "holds" in v),
        "max_abs_difference_embed_regions_vs_four_embeds": agree,
        "votes_equal_four_pixel_votes": bool(votes_agree),
        "shell_kernels": shell,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
