"""Golden case lists and the CPU checks shared by the oracle tests and the GPU tests (a plain helper module, no pytest in it)."""
import os

import numpy as np
import torch

from oracle import videoseal_ref as R
from oracle.inputs import synthetic_frames, synthetic_msgs
from tests._util import GOLDEN, check_sub, load_golden, psnr_np

CARDS = os.path.join(os.path.dirname(GOLDEN), "..", "videoseal_amd", "cards")

TINY = ["tiny_img", "tiny_img_resize", "tiny_vid_repeat", "tiny_vid_alternate", "tiny_vid_interpolate"]
TINYC = ["tinyc_img", "tinyc_vid"]
FULL = ["vs10_img256", "vs10_img_odd", "vs10_img_lowres", "vs10_vid", "vs10_vid_lowres", "vs10_img_uniform"]

FWD_TINY = ["tiny_fwd_img_train", "tiny_fwd_img_evalbn", "tiny_fwd_img_si", "tiny_fwd_vid_train", "tiny_fwd_vid_lowres", "tiny_fwd_vid_alt"]
FWD_FULL = ["vs10_fwd_img_train"]
PIXELSEAL = ["pixelseal_img", "pixelseal_vid"]


def _run(spec, sd, meta):
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"], kind=meta["kind"])
    msgs = synthetic_msgs(1 if meta["is_video"] else meta["n"], spec.nbits, seed=meta["seed"])
    if meta["is_video"]:
        out = R.embed_video(sd, spec, imgs, msgs, lowres_attenuation=meta["lowres"], chunk_size=meta["chunk"],
                            step_size=meta["step"], video_mode=meta["video_mode"])
    else:
        out = R.embed_image(sd, spec, imgs, msgs, lowres_attenuation=meta["lowres"])
    return imgs, msgs, out


def _check_case(spec, sd, name):
    g = load_golden(name)
    meta = g["meta"]
    with torch.no_grad():
        imgs, msgs, out = _run(spec, sd, meta)
        assert (msgs.numpy() == g["msgs"]).all(), f"{name}: the seeded messages differ from the fixture's"
        check_sub(g, "imgs_w", out["imgs_w"], 2e-6, name + " ")
        if "preds_w.sub" in g:
            check_sub(g, "preds_w", out["preds_w"], 2e-6, name + " ")
        preds = R.detect(sd, spec, out["imgs_w"])["preds"]
        assert (preds - torch.from_numpy(g["preds"])).abs().max() < 2e-5, (name, "preds")
        assert ((preds > 0).numpy() == (g["preds"] > 0)).all(), "bit decisions differ from the reference"
        clean = R.detect(sd, spec, imgs)["preds"]
        assert (clean - torch.from_numpy(g["preds_clean"])).abs().max() < 2e-5, (name, "preds_clean")
        assert abs(psnr_np(out["imgs_w"], imgs) - meta["psnr"]) < 1e-3, (name, "psnr", meta["psnr"])
        if meta["is_video"]:
            mh = R.extract_message(sd, spec, out["imgs_w"])
            assert (mh.numpy() == g["msg_hat"]).all(), f"{name}: extract_message differs from the reference"
        if "delta.sub" in g:
            y = R.rgb2y(sd, imgs) if spec.yuv else imgs
            check_sub(g, "delta", R.embedder_forward(sd, spec, y, msgs), 2e-6, name + " ")
            if "hmaps.sub" in g:
                check_sub(g, "hmaps", R.jnd_heatmaps(sd, spec, imgs), 1e-6, name + " ")


def bn_vectors(sd, bn):
    merged = dict(sd)
    merged.update(bn or {})
    rm = torch.cat([v.flatten() for k, v in merged.items() if k.endswith("running_mean")])
    rv = torch.cat([v.flatten() for k, v in merged.items() if k.endswith("running_var")])
    nbt = torch.stack([v for k, v in merged.items() if k.endswith("num_batches_tracked")])
    return rm, rv, nbt


def make_inputs(info):
    x = synthetic_frames(info["F"], info["H"], info["W"], seed=info["seed"])
    y = (x + info["amp"] * torch.randn(x.shape, generator=torch.Generator().manual_seed(info["seed"]))).clamp(0, 1)
    return x, y


def check_inputs(g, cname, x, y):
    """a generator mismatch must read as such, not as a kernel error"""
    got = np.array([float(x.double().sum()), float(y.double().sum()), float((x.double() * y.double()).sum())])
    assert np.allclose(got, g[f"{cname}.checksum"], rtol=1e-12, atol=0), f"{cname}: the seeded inputs differ from the fixture's ({got} vs {g[cname + '.checksum']})"
