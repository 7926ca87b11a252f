"""Seeded inputs of the discriminator fixtures, shared by tests/golden/make_golden_disc.py (which runs the reference on them) and by the tests
(which rebuild them and check the fixture's checksums first, so that a generator mismatch on another machine reads as such and not as a kernel
error).  Everything comes from torch's CPU generator."""
import math

import numpy as np
import torch

# (n_layers, input_nc, B, H, W): 38 x 50 gives odd maps (19 x 25) to the second stride-2 convolution; no row count is a multiple of a tile
CASES = ((2, 1, 2, 40, 56), (2, 3, 3, 38, 50), (3, 3, 2, 40, 56))
NDF = 32
SUB = 1024                      # values kept per stored tensor
HINGE_GAIN = 8.0                # the hinge cases scale the last convolution by this and give it a seeded bias: logits on both sides of +-1


def case_name(case) -> str:
    nl, nc, B, H, W = case
    return f"n{nl}_c{nc}_b{B}_{H}x{W}"


def _gen(*key):
    return torch.Generator().manual_seed(2_000_003 * len(key) + sum((i + 1) * 104729 * int(k) for i, k in enumerate(key)))


def layer_plan(n_layers: int, input_nc: int):
    """[(index in `main`, kind, shape...)] of the parameters, in the reference's order: conv (co, ci, stride), GroupNorm (c)"""
    plan, idx, mult = [("conv", 0, NDF, input_nc, 2)], 2, 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        plan += [("conv", idx, NDF * mult, NDF * prev, 2), ("gn", idx + 1, NDF * mult)]
        idx += 3
    prev, mult = mult, min(2 ** n_layers, 8)
    plan += [("conv", idx, NDF * mult, NDF * prev, 1), ("gn", idx + 1, NDF * mult), ("conv", idx + 3, 1, NDF * mult, 1)]
    return plan


def state_dict(n_layers: int, input_nc: int, hinge: bool = False, hinge_seed: int = 0):
    """seeded parameters with the reference's names: conv weights N(0, 0.02) (weights_init), conv biases U(+-1 / sqrt(fan_in)) (torch's default),
    GroupNorm weight 1 + 0.2 N and bias 0.2 N (at their defaults 1 / 0 the affine part would not be tested).  hinge: the last convolution times
    HINGE_GAIN with the bias 4 N of `hinge_seed` (the fixture records the first seed that puts logits on both sides of +-1)"""
    g = _gen(n_layers, input_nc, 17)
    sd = {"rgb2yuv.M": torch.tensor([[0.299, 0.587, 0.114], [-0.14713, -0.28886, 0.436], [0.615, -0.51499, -0.10001]], dtype=torch.float32)}
    plan = layer_plan(n_layers, input_nc)
    for p in plan:
        if p[0] == "conv":
            _, i, co, ci, _ = p
            sd[f"main.{i}.weight"] = 0.02 * torch.randn(co, ci, 4, 4, generator=g)
            sd[f"main.{i}.bias"] = (2 * torch.rand(co, generator=g) - 1) / math.sqrt(16 * ci)
        else:
            _, i, c = p
            sd[f"main.{i}.weight"] = 1 + 0.2 * torch.randn(c, generator=g)
            sd[f"main.{i}.bias"] = 0.2 * torch.randn(c, generator=g)
    if hinge:
        last = plan[-1][1]
        sd[f"main.{last}.weight"] = HINGE_GAIN * sd[f"main.{last}.weight"]
        sd[f"main.{last}.bias"] = 4.0 * torch.randn(1, generator=_gen(n_layers, input_nc, 23, hinge_seed))
    return sd


def frames(case, seed: int, which: int = 0):
    """[B, 3, H, W] in [0, 1]: smooth structure plus noise; which = 0 the real frames, 1 the 'watermarked' ones of the hinge step"""
    nl, nc, B, H, W = case
    g = _gen(nl, nc, B, H, W, seed, which)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    ph = 6.0 * torch.rand(B, 3, 1, 1, generator=g)
    base = 0.5 + 0.25 * torch.sin(5.0 * yy[None, None] + ph) * torch.cos(4.0 * xx[None, None] - ph)
    return (base + 0.2 * (torch.rand(B, 3, H, W, generator=g) - 0.5)).clamp(0, 1).float()


def logit_hw(case):
    nl, _, _, H, W = case
    for _ in range(nl):
        H, W = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    return H - 2, W - 2


def dlogits(case):
    nl, nc, B, H, W = case
    h, w = logit_hw(case)
    return torch.randn(B, 1, h, w, generator=_gen(nl, nc, B, H, W, 5)) / (B * h * w)


def checksum(*tensors):
    return np.array([float(t.double().sum()) for t in tensors] + [float(sum((t.double() ** 2).sum() for t in tensors))])


def projection(name: str, numel: int):
    g = torch.Generator().manual_seed(sum(name.encode()) * 7919 + numel)
    return (torch.randint(0, 2, (numel,), generator=g, dtype=torch.int64) * 2 - 1).double()


def stride_of(numel: int) -> int:
    return max(1, numel // SUB) | 1


def summary(name: str, t: torch.Tensor):
    """(sub-sample with an odd stride, [L2 norm, sum, Rademacher projection, numel, stride, max |t|]) in float64"""
    f = t.detach().double().flatten().cpu()
    s = stride_of(f.numel())
    return f[::s].numpy().copy(), np.array([float(f.norm()), float(f.sum()), float((f * projection(name, f.numel())).sum()), f.numel(), s,
                                            float(f.abs().max()) if f.numel() else 0.0])


def errors(name: str, t: torch.Tensor, sub64: np.ndarray, stats64: np.ndarray):
    """what `t` loses against the float64 record: [max |element| on the sub-sample, L2 on the sub-sample, |norm|, |sum|, |projection|]"""
    sub, stats = summary(name, t)
    d = sub - sub64
    return np.array([float(np.abs(d).max()) if d.size else 0.0, float(np.sqrt((d ** 2).sum())), abs(stats[0] - stats64[0]), abs(stats[1] - stats64[1]),
                     abs(stats[2] - stats64[2])])

