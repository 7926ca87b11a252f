#!/usr/bin/env python
"""Golden vectors of the PatchGAN discriminator and of the two training steps that use it, produced by the UNMODIFIED reference modules on the CPU
(needs a reference checkout next to the repository, as tests/golden/make_golden_bwd.py; same import recipe and stubs):

    python tests/golden/make_golden_disc.py            # -> disc_ops.npz, disc_step.npz

disc_ops.npz -- `NLayerDiscriminator` (modules/discriminator.py:89-148) in float64 on the seeded inputs of tests/_disc_util.py, three
configurations: every layer's output (the convolution outputs and the activations), the logits, d imgs of the generator term -mean(logits) with
every parameter frozen, and the gradient of every parameter for the hinge step (hinge_d_loss on real / fake frames) and for a seeded d logits.
Every tensor is stored as a sub-sample with an odd stride plus [norm, sum, Rademacher projection, numel, stride, max], and with `e`: what the
reference's own float32 run loses against float64 in the same five measures (tests/_disc_util.errors).
Two conditions are asserted and recorded:
  LeakyReLU kink: input seeds are tried in order and the first is kept for which no LeakyReLU input of the float64 run has |z| < 1e-6 (an element
    within rounding of zero takes slope 0.2 or 1 depending on rounding, in the reference's float32 run as well);
  hinge kink: with weights_init the logits stay inside (-1, 1) and both ReLUs of the hinge loss are always active; the hinge cases scale the last
    convolution by 8 and give it a seeded bias: at least 10 % of the real logits exceed 1, at least 10 % of the fake ones are below -1, none lies
    within 1e-4 of +-1.

disc_step.npz -- the reference's own `VideosealLoss(disc_weight=1.0, disc_num_layers=2, disc_in_channels=1, percep_loss="mse", decode_weight=1.0,
detect_weight=0.0)` on the tiny model of make_golden_bwd.py in float64 (and float32 for `e`): optimizer_idx 0 and 1, balanced and not, global_step
below and at disc_start, image mode 2 x 64^2 and video mode 4 x 64^2 with step 2: the log, the gradient summaries of all embedder, detector and
discriminator parameters, and the parameters left without a gradient."""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                   # noqa: E402
import make_golden_fwd as MF                               # noqa: E402
import make_golden_bwd as MB                               # noqa: E402

from tests import _disc_util as U                          # noqa: E402

KINK = 1e-6


def run_disc(Disc, case, sd, imgs_list, dtype):
    """reference forward of each frame batch: (module, [leaf frames], [logits], per batch {conv / act outputs}, smallest |LeakyReLU input|)"""
    nl, nc = case[0], case[1]
    m = Disc(input_nc=nc, ndf=U.NDF, n_layers=nl)
    m.load_state_dict(sd, strict=True)
    m = m.to(dtype)
    rec, zmin = {}, [float("inf")]
    hooks = []
    for i, mod in enumerate(m.main):
        if isinstance(mod, torch.nn.LeakyReLU):
            hooks.append(mod.register_forward_pre_hook(lambda _m, a: zmin.__setitem__(0, min(zmin[0], float(a[0].detach().abs().min())))))
            hooks.append(mod.register_forward_hook(lambda _m, a, o, i=i: rec.__setitem__(f"act{i}", o.detach().clone())))
        elif isinstance(mod, torch.nn.Conv2d):
            hooks.append(mod.register_forward_hook(lambda _m, a, o, i=i: rec.__setitem__(f"conv{i}", o.detach().clone())))
    leaves, logits, recs = [], [], []
    for x in imgs_list:
        x = x.detach().to(dtype).clone().requires_grad_(True)
        rec.clear()
        logits.append(m(x))
        leaves.append(x)
        recs.append(dict(rec))
    for h in hooks:
        h.remove()
    return m, leaves, logits, recs, zmin[0]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def ops_case(Disc, hinge_d_loss, case, out):
    name = U.case_name(case)
    sd = U.state_dict(case[0], case[1])
    for seed in range(200):
        real, fake = U.frames(case, seed, 0), U.frames(case, seed, 1)
        *_, zmin = run_disc(Disc, case, sd, [real, fake], torch.float64)
        if zmin >= KINK:
            break
    else:
        raise SystemExit(f"{name}: no seed below 200 keeps every LeakyReLU input {KINK} away from zero")
    for hseed in range(200):         # the first bias seed that meets the hinge conditions
        sdh = U.state_dict(case[0], case[1], hinge=True, hinge_seed=hseed)
        _, _, (lr, lf), _, _ = run_disc(Disc, case, sdh, [real, fake], torch.float64)
        lr, lf = lr.detach(), lf.detach()
        gap = min(float((lr - 1).abs().min()), float((lf + 1).abs().min()), float((lr + 1).abs().min()), float((lf - 1).abs().min()))
        if float((lr > 1).double().mean()) >= 0.1 and float((lf < -1).double().mean()) >= 0.1 and gap >= 1e-4:
            break
    else:
        raise SystemExit(f"{name}: no bias seed below 200 meets the hinge conditions")
    dl = U.dlogits(case)
    store = {}

    def put(key, t64, t32):
        sub, stats = U.summary(key, t64)
        store[key] = (sub, stats, U.errors(key, t32, sub, stats))

    runs = {}
    for dt in (torch.float64, torch.float32):
        r = {}
        # forward records + generator term with every parameter frozen + the seeded d logits
        m, (x,), (lg,), (rec,), _ = run_disc(Disc, case, sd, [real], dt)
        for k, v in rec.items():
            r["fwd." + k] = nhwc(v)
        r["logits"] = lg.detach()
        r["gen.loss"] = (-lg.mean()).detach()
        frozen = run_disc(Disc, case, sd, [], dt)[0]
        for p in frozen.parameters():
            p.requires_grad_(False)
        xg = real.detach().to(dt).clone().requires_grad_(True)
        (-frozen(xg).mean()).backward()
        r["gen.dimgs"] = xg.grad
        r["gen.no_grad"] = [k for k, p in frozen.named_parameters() if p.grad is None]
        m3, (x3,), (lg3,), _, _ = run_disc(Disc, case, sd, [real], dt)
        lg3.backward(dl.to(dt))
        r["rand.dimgs"] = x3.grad
        for k, p in m3.named_parameters():
            r["rand.grad." + k] = p.grad
        # hinge step on the scaled last layer
        mh, _, (lr, lf), _, _ = run_disc(Disc, case, sdh, [real, fake], dt)
        d_loss = hinge_d_loss(lr, lf)
        d_loss.backward()
        r["hinge.loss"], r["hinge.logits_real"], r["hinge.logits_fake"] = d_loss.detach(), lr.detach(), lf.detach()
        r["hinge.mean_real"], r["hinge.mean_fake"] = lr.detach().mean(), lf.detach().mean()
        for k, p in mh.named_parameters():
            r["hinge.grad." + k] = p.grad
        runs[dt] = r
    r64, r32 = runs[torch.float64], runs[torch.float32]
    assert r64["gen.no_grad"] == [k for k in sd if k != "rgb2yuv.M"], r64["gen.no_grad"]
    lr, lf = r64["hinge.logits_real"], r64["hinge.logits_fake"]
    share_r, share_f = float((lr > 1).double().mean()), float((lf < -1).double().mean())
    gap = min(float((lr - 1).abs().min()), float((lf + 1).abs().min()), float((lr + 1).abs().min()), float((lf - 1).abs().min()))
    assert share_r >= 0.1 and share_f >= 0.1 and gap >= 1e-4, (name, share_r, share_f, gap)
    for k in r64:
        if k != "gen.no_grad":
            put(k, r64[k], r32[k])
    for k, (sub, stats, e) in store.items():
        out[f"{name}/{k}.sub"], out[f"{name}/{k}.stats"], out[f"{name}/{k}.e"] = sub, stats, e
    out[f"{name}/checksum"] = U.checksum(real, fake, dl, *[v for v in sd.values()], *[v for v in sdh.values()])
    ref = Disc(input_nc=case[1], ndf=U.NDF, n_layers=case[0])
    meta = dict(case=list(case), seed=seed, hinge_seed=hseed, min_abs_lrelu_input=zmin, kink_threshold=KINK, hinge_share_real_above_1=share_r, hinge_share_fake_below_m1=share_f,
                hinge_gap=gap, logits_range=[float(r64["logits"].min()), float(r64["logits"].max())], keys=sorted(store),
                no_grad_gen=r64["gen.no_grad"], state_dict=[[k, list(v.shape), str(v.dtype)] for k, v in ref.state_dict().items()])
    worst = max((float(e[0] / s[5]), k) for k, (_, s, e) in store.items() if s[5] > 0)
    print(f"{name}: seed {seed} hinge seed {hseed} min|z| {zmin:.2e} hinge shares {share_r:.2f}/{share_f:.2f} gap {gap:.1e} d_loss {float(r64['hinge.loss']):.4f} "
          f"worst e/max|g| {worst[0]:.2e} ({worst[1]})")
    return meta


# ------------------------------------------------------------------------------------------------------------------ the two training steps
STEP_LOSS = dict(disc_weight=1.0, disc_num_layers=2, disc_in_channels=1, percep_loss="mse", decode_weight=1.0, detect_weight=0.0, percep_weight=1.0)
DISC_START = 5
STEP_CASES = [dict(name=f"{mode}_{'bal' if bal else 'fix'}_{'before' if gs < DISC_START else 'at'}_opt{oi}", mode=mode, balanced=bal, global_step=gs,
                   optimizer_idx=oi)
              for mode in ("img", "vid") for bal in (True, False) for gs in (DISC_START - 1, DISC_START) for oi in (0, 1)]


def step_case(model_fn, Augmenter, VideosealLoss, spec, c, out):
    from oracle.inputs import synthetic_frames, synthetic_msgs
    vid = c["mode"] == "vid"
    n, h, w, seed = (4, 64, 64, 61) if vid else (2, 64, 64, 62)
    res = {}
    for dt in (torch.float64, torch.float32):
        model = model_fn()
        model.augmenter = Augmenter(masks={"kind": "none"}, augs={"identity": 1}, augs_params={}, num_augs=1)
        model.train()
        if vid:
            model.step_size = 2
        crit = VideosealLoss(balanced=c["balanced"], disc_start=DISC_START, **STEP_LOSS)
        crit.discriminator.load_state_dict(U.state_dict(2, 1), strict=True)
        model, crit = model.to(dt), crit.to(torch.device("cpu")).to(dt)
        imgs = synthetic_frames(n, h, w, seed=seed).to(dt)
        msgs = synthetic_msgs(1 if vid else n, spec.nbits, seed=seed)
        masks = torch.ones(n, 1, h, w, dtype=dt)
        torch.manual_seed(1000 + seed)
        o = model(imgs, masks, msgs, is_video=vid)
        loss, logs = crit(imgs, o["imgs_w"], o["masks"], o["msgs"], o["preds"], c["optimizer_idx"], c["global_step"],
                          last_layer=model.embedder.get_last_layer())
        loss.backward()
        named = [(k, p) for k, p in model.named_parameters() if p.requires_grad] + [("disc." + k, p) for k, p in crit.discriminator.named_parameters()]
        res[dt] = dict(log={k: float(v) for k, v in logs.items()}, loss=float(loss), grads={k: p.grad.detach() for k, p in named if p.grad is not None},
                       missing=[k for k, p in named if p.grad is None])
    r64, r32 = res[torch.float64], res[torch.float32]
    assert r64["missing"] == r32["missing"]
    names = sorted(r64["grads"])
    rows, es = [], []
    for k in names:
        sub, stats = U.summary(k, r64["grads"][k])
        rows.append(stats)
        es.append(U.errors(k, r32["grads"][k], sub, stats))
    nm = c["name"]
    out[f"{nm}/grad_names"] = np.array(names)
    out[f"{nm}/grad_stats"] = np.array(rows).reshape(len(names), 6)
    out[f"{nm}/grad_e"] = np.array(es).reshape(len(names), 5)
    print(f"{nm}: loss {r64['loss']:.6f} log { {k: round(v, 6) for k, v in r64['log'].items()} } grads {len(names)} missing {len(r64['missing'])}")
    return dict(c, n=n, h=h, w=w, seed=seed, torch_seed=1000 + seed, step=2 if vid else 1, disc_start=DISC_START, loss_kw=STEP_LOSS, log=r64["log"],
                log_e={k: abs(r32["log"][k] - v) for k, v in r64["log"].items()}, loss=r64["loss"], loss_e=abs(r32["loss"] - r64["loss"]),
                no_grad_params=r64["missing"])


def main():
    torch.set_num_threads(8)
    MG.import_reference()
    MF.patch_torchvision()
    MB.extra_stubs()
    from videoseal.augmentation.augmenter import Augmenter
    from videoseal.losses.videosealloss import VideosealLoss, hinge_d_loss
    from videoseal.modules.discriminator import NLayerDiscriminator
    from oracle.weights import make_state_dict, tiny_spec
    which = sys.argv[1:] or ["ops", "step"]
    if "ops" in which:
        out, metas = {}, {}
        for case in U.CASES:
            metas[U.case_name(case)] = ops_case(NLayerDiscriminator, hinge_d_loss, case, out)
        out["meta"] = json.dumps(dict(cases=metas, ndf=U.NDF, hinge_gain=U.HINGE_GAIN, sub=U.SUB))
        np.savez_compressed(os.path.join(HERE, "disc_ops.npz"), **out)
    if "step" in which:
        ts = tiny_spec()

        def tiny_model():
            m = MG.build_reference(ts, MG.card_for_spec(ts))
            m.load_state_dict(make_state_dict(ts, seed=3), strict=True)
            return m
        out, metas = {}, {}
        for c in STEP_CASES:
            metas[c["name"]] = step_case(tiny_model, Augmenter, VideosealLoss, ts, c, out)
        out["meta"] = json.dumps(dict(cases=metas))
        np.savez_compressed(os.path.join(HERE, "disc_step.npz"), **out)


if __name__ == "__main__":
    main()
