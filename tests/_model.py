"""What the model-level GPU tests share: building a model from an oracle spec, the end-to-end tolerances, the golden-case run and the
train-mode set-ups (a plain helper module, no pytest in it).  Importing it does not touch the device."""
import torch

from oracle import videoseal_ref as R
from oracle.inputs import synthetic_frames, synthetic_msgs
from tests._util import assert_decisions, check_sub, load_golden, psnr_np
from videoseal_amd import augmentation as G
from videoseal_amd.layout import ModelCfg
from videoseal_amd.model import build_model

TOL_IMG = 1e-4      # |imgs_w - reference| (values in [0,1]); BASELINE asks 1e-3 on PSNR
TOL_LOGIT = 1e-3


def cfg_of(spec) -> ModelCfg:
    return ModelCfg(nbits=spec.nbits, hidden=spec.hidden, img_size=spec.img_size, scaling_w=spec.scaling_w, scaling_i=spec.scaling_i,
                    chunk_size=spec.chunk_size, step_size=spec.step_size, yuv=spec.yuv, in_ch=spec.in_ch, out_ch=spec.out_ch, z=spec.z,
                    mults=list(spec.mults), num_blocks=spec.num_blocks, last_tanh=spec.last_tanh, depths=list(spec.depths),
                    dims=list(spec.dims), stem_stride=spec.stem_stride, jnd_in=spec.jnd_in, jnd_out=spec.jnd_out,
                    unet_act=spec.unet_act, unet_norm=spec.unet_norm, extractor=spec.extractor, vit_dim=spec.vit_dim,
                    vit_depth=spec.vit_depth, vit_heads=spec.vit_heads, vit_patch=spec.vit_patch, vit_window=spec.vit_window,
                    vit_global=list(spec.vit_global), vit_out=spec.vit_out, vit_mlp_ratio=spec.vit_mlp_ratio, vit_rel_pos=spec.vit_rel_pos)


def make_model(spec, sd):
    m = build_model(cfg_of(spec))
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys, (missing.missing_keys, missing.unexpected_keys)
    return m.eval().to("cuda")


def _run_case(spec, sd, model, name):
    g = load_golden(name)
    meta = g["meta"]
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"], kind=meta["kind"])
    msgs = synthetic_msgs(1 if meta["is_video"] else meta["n"], spec.nbits, seed=meta["seed"])
    model.chunk_size, model.step_size, model.video_mode = meta["chunk"], meta["step"], meta["video_mode"]
    out = model.embed(imgs.cuda(), msgs, is_video=meta["is_video"], lowres_attenuation=meta["lowres"])
    imgs_w = out["imgs_w"]
    assert imgs_w.is_cuda and imgs_w.shape == imgs.shape, (name, imgs_w.device, imgs_w.shape)
    check_sub(g, "imgs_w", imgs_w, TOL_IMG, name + " ")
    if "preds_w.sub" in g:
        check_sub(g, "preds_w", out["preds_w"], TOL_IMG, name + " ")
    assert abs(psnr_np(imgs_w.cpu(), imgs) - meta["psnr"]) < 1e-3, "PSNR differs from the reference by more than 1e-3 dB"
    preds = model.detect(imgs_w, is_video=meta["is_video"])["preds"].cpu()
    gold = torch.from_numpy(g["preds"])
    # logits of OUR watermarked frames vs logits of the reference's watermarked frames
    assert (preds - gold).abs().max() < TOL_LOGIT, (name, "preds", float((preds - gold).abs().max()))
    assert_decisions(preds, gold, what=name + " preds", min_sure=0.99)        # largest measured logit error of any case: 3.5e-6
    # detector alone on identical inputs: decisions must be bit-exact
    clean = model.detect(imgs.cuda(), is_video=meta["is_video"])["preds"].cpu()
    gclean = torch.from_numpy(g["preds_clean"])
    assert (clean - gclean).abs().max() < 1e-4, (name, "preds_clean", float((clean - gclean).abs().max()))
    assert ((clean > 0) == (gclean > 0)).all(), "bit decisions differ from the reference on identical frames"
    if meta["is_video"]:
        # extract_message (antialias=False resize + frame mean): the oracle on OUR frames is the checker
        na = {"mode": "bilinear", "align_corners": False, "antialias": False}
        agg = model.detect(imgs_w, is_video=True, interpolation=na)["preds"][:, 1:].mean(dim=0).cpu()
        ref_agg = R.detect(sd, spec, imgs_w.cpu(), na)["preds"][:, 1:].mean(dim=0)
        assert (agg - ref_agg).abs().max() < 1e-4, (name, "aggregated logits", float((agg - ref_agg).abs().max()))
        # extract_message on OUR watermarked frames against the decision the REFERENCE took on its own (the golden's `msg_hat`), wherever
        # the mean logit is further from 0 than 10 x the measured logit error; no flip allowance
        mh = model.extract_message(imgs_w).cpu()
        gold_mh = torch.from_numpy(g["msg_hat"]).bool()
        sure = ref_agg.abs() > 1e-5
        assert mh.shape == gold_mh.shape and int((~sure).sum()) <= 1, (name, mh.shape, gold_mh.shape, int((~sure).sum()))
        assert torch.equal(mh.bool()[:, sure], gold_mh[:, sure]), "extract_message differs from the reference's own decision"
        assert torch.equal(mh.bool()[:, sure], (ref_agg > 0)[None][:, sure]), "extract_message differs from the oracle's decision on the same frames"


def hip_forward(model, spec, meta):
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"], kind=meta["kind"])
    msgs = synthetic_msgs(1 if meta["is_video"] else meta["n"], spec.nbits, seed=meta["seed"])
    masks = torch.ones(meta["n"], 1, meta["h"], meta["w"])
    model.augmenter = G.Augmenter(masks={"kind": "none"}, augs=meta["augs"], augs_params=meta["augs_params"], num_augs=meta["num_augs"])
    model.train()
    if not meta["bn_train"]:
        model.embedder.eval()
        model.detector.eval()
    model.step_size, model.video_mode, model.lowres_attenuation = meta["step"], meta["video_mode"], meta["lowres"]
    model.blender.scaling_i = meta["scaling_i"]
    torch.manual_seed(meta["torch_seed"])
    return model(imgs.cuda(), masks.cuda(), msgs, is_video=meta["is_video"]), imgs, msgs


def _setup(spec, sd, meta):
    model = make_model(spec, sd)
    model.augmenter = G.Augmenter(masks={"kind": "none"}, augs=meta["augs"], augs_params=meta["augs_params"], num_augs=meta["num_augs"])
    model.train()
    if meta["is_video"]:
        model.step_size = meta["step"]
    imgs = synthetic_frames(meta["n"], meta["h"], meta["w"], seed=meta["seed"], kind=meta["kind"])
    msgs = synthetic_msgs(1 if meta["is_video"] else meta["n"], spec.nbits, seed=meta["seed"])
    masks = torch.ones(meta["n"], 1, meta["h"], meta["w"])
    return model, imgs, msgs, masks
