#!/usr/bin/env python
"""Golden values for the SSIM / MS-SSIM / JND perceptual terms and the SSIM / MS-SSIM metrics, from the UNMODIFIED reference
(losses/ssim.py loaded by file path -- it imports torch only; `PerceptualLoss` / `JNDLoss` through the stub-import recipe of
make_golden_bwd.py).  Run on the CPU next to a reference checkout:

    python tests/golden/make_golden_ssim.py

Inputs come from seeds (x = oracle.inputs.synthetic_frames, y = clamp(x + amp * randn(seeded), 0, 1)); the fixture stores no frames,
only a float64 checksum of x and y, so that a generator mismatch on another machine reads as such and not as a kernel error.

Per case: the per-plane SSIM and cs means at every pyramid level (float64 run of losses/ssim.py's `_ssim` + its pooling), and per
perceptual-loss string the loss and, of d loss / d imgs_w, norm, sum, a seeded projection and a strided sub-sample (every 7th row and
column -- every 14th at 768 x 768 --, stored in float32) -- all from the float64 run; and what the SAME reference code loses in fp32 against its float64 run
(`e_*`): the yardstick of tests/test_gpu_ssim.py.  The float64 run of a combined string is the weighted sum of its terms' float64
runs (the reference's YUV matrix is fp32-only: its term is evaluated with that matrix cast to float64); the fp32 run is the
reference's own `PerceptualLoss(string)`.  MS-SSIM cases must keep every factor away from 0 (relu(f)^w has no derivative there)."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                   # noqa: E402
import make_golden_bwd as MB                               # noqa: E402
import make_golden_fwd as MF                               # noqa: E402

from oracle.inputs import synthetic_frames                  # noqa: E402
from oracle.loss import _YUV                                # noqa: E402
from tests._util import projection_vector                   # noqa: E402
from videoseal_amd import autograd as AG                    # noqa: E402

# F, H, W, amp, seed
CASES = {"c200x176": (2, 200, 176, 0.02, 61), "c256x256": (2, 256, 256, 0.01, 62), "c177x163": (2, 177, 163, 0.05, 63),
         "c768x768": (1, 768, 768, 0.01, 64), "c40x37": (2, 40, 37, 0.02, 65)}
STRINGS = ("ssim", "msssim", "jnd", "mse+0.1_ssim", "yuv+0.5_msssim+0.1_jnd")
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SUB = 7                  # every 7th row and column of the gradient is stored ...
SUB_LARGE = 14           # ... every 14th at 768 x 768, which keeps the fixture under 1 MB


def make_inputs(F, H, W, amp, seed):
    x = synthetic_frames(F, H, W, seed=seed)
    y = (x + amp * torch.randn(x.shape, generator=torch.Generator().manual_seed(seed))).clamp(0, 1)
    return x, y


def checksum(x, y):
    return np.array([float(x.double().sum()), float(y.double().sum()), float((x.double() * y.double()).sum())])


def grad_summary(name, g, sub=SUB):
    g = g.detach().double()
    flat = g.flatten()
    return np.array([float(flat.norm()), float(flat.sum()), float((flat * projection_vector(name, flat.numel())).sum()), float(flat.abs().max())]), \
        g[..., ::sub, ::sub].contiguous()


def main():
    torch.set_num_threads(8)
    MG.import_reference()
    MF.patch_torchvision()
    MB.extra_stubs()
    spec = importlib.util.spec_from_file_location("ref_ssim", os.path.join(MG.REF, "videoseal", "losses", "ssim.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    from videoseal.losses.perceptual import PerceptualLoss

    def stats(x, y):
        """per-plane (ssim, cs) at every level the sides allow, as ms_ssim walks them"""
        win = S._fspecial_gauss_1d(11, 1.5).repeat([x.shape[1], 1, 1, 1])
        out = []
        for _ in range(5):
            if min(x.shape[-2:]) < 11:
                break
            s, c = S._ssim(x, y, data_range=1.0, win=win, size_average=False)
            out.append(torch.stack([s, c]))
            pad = [d % 2 for d in x.shape[2:]]
            x, y = torch.nn.functional.avg_pool2d(x, 2, padding=pad), torch.nn.functional.avg_pool2d(y, 2, padding=pad)
        return torch.stack(out)                                      # [L, 2, F, C]

    def term(name, x, y):
        """one term of the grammar in the dtype of x (float64 run)"""
        if name == "yuv":
            m = torch.tensor(_YUV, dtype=torch.float32).to(x.dtype)
            f = lambda t: torch.matmul(t.permute(0, 2, 3, 1), m.T)
            return torch.nn.functional.mse_loss(f(x), f(y))
        mod = PerceptualLoss(name)
        for v in mod.losses.values():
            v.to(x.dtype)
        return mod(x, y)

    def run64(string, x, y):
        weights, names = AG.parse_percep_loss(string)      # the repository's parser; the fp32 run below goes through the reference's own
        if weights is None:
            return term(names[0], x, y)
        return sum(w * term(n, x, y).mean() for w, n in zip(weights, names))

    d, meta = {}, {"cases": {}, "strings": list(STRINGS)}
    for cname, (F, H, W, amp, seed) in CASES.items():
        x, y = make_inputs(F, H, W, amp, seed)
        d[f"{cname}.checksum"] = checksum(x, y)
        st64, st32 = stats(x.double(), y.double()), stats(x, y)
        d[f"{cname}.stats"] = st64.numpy()
        e_stats = float((st32.double() - st64).abs().max())
        big = min(H, W) > 160
        sub = SUB_LARGE if H * W > 256 * 256 else SUB
        info = dict(sub=sub, F=F, H=H, W=W, amp=amp, seed=seed, levels=int(st64.shape[0]), e_stats=e_stats, strings={})
        if big:
            f = torch.cat([st64[:4, 1], st64[4:5, 0]])
            info["min_factor"] = float(f.min())
            assert info["min_factor"] > 0.25, (cname, info["min_factor"])
        d[f"{cname}.ssim_img"] = st64[0, 0].mean(1).numpy()
        if big:
            w = torch.tensor(MS_WEIGHTS, dtype=torch.float64).view(-1, 1, 1)
            d[f"{cname}.msssim_img"] = torch.prod(torch.relu(torch.cat([st64[:4, 1], st64[4:5, 0]])) ** w, dim=0).mean(1).numpy()
        # per-term float64 facts the bounds of combined strings need
        h64 = PerceptualLoss("jnd").losses["jnd"].double().jnd.heatmaps(x.double())
        info["jnd_mean_abs"] = float(((y.double() - x.double()).abs() - h64).abs().mean())
        for name in ("mse", "yuv", "ssim", "jnd") + (("msssim",) if big else ()):
            yy = y.double().requires_grad_(True)
            lt = term(name, x.double(), yy).mean()
            lt.backward()
            info.setdefault("terms", {})[name] = dict(loss=float(lt), gmax=float(yy.grad.abs().max()), gnorm=float(yy.grad.norm()))
        for string in STRINGS:
            if "msssim" in string and not big:
                continue
            y64 = y.double().requires_grad_(True)
            l64 = run64(string, x.double(), y64).mean()
            l64.backward()
            y32 = y.clone().requires_grad_(True)
            l32 = PerceptualLoss(string)(x, y32).mean()
            l32.backward()
            key = f"{cname}.{string}"
            s64, sub64 = grad_summary(key, y64.grad, sub)
            s32, _ = grad_summary(key, y32.grad)
            assert abs(float(l32) - float(l64)) < 1e-6, (cname, string, float(l32), float(l64))      # same grammar, same terms
            dg = y32.grad.double() - y64.grad
            d[key + ".grad_summary"] = s64
            d[key + ".grad_sub"] = sub64.float().numpy()
            info["strings"][string] = dict(loss=float(l64), loss32=float(l32), e_loss=abs(float(l32) - float(l64)),
                                           e_grad_max=float(dg.abs().max()) / s64[3], e_grad_l2=float(dg.norm()) / s64[0],
                                           e_norm=abs(s32[0] - s64[0]), e_sum=abs(s32[1] - s64[1]), e_proj=abs(s32[2] - s64[2]))
            print(cname, string, info["strings"][string])
        meta["cases"][cname] = info
        print(cname, {k: v for k, v in info.items() if k != "strings"})
    d["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "ssim_loss.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
