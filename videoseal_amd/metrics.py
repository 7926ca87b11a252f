"""Evaluation metrics of the path (videoseal/evals/metrics.py), plain torch on the caller's device.

`psnr` / `bit_accuracy` are the two parity metrics (evals/metrics.py:22-36, 150-178).  The others are what train.py:65,649,667-670,814
and evals/full.py:46 import next to them -- mask metrics (`accuracy`, `iou`), message statistics (`pvalue`, `capacity`,
`bit_accuracy_1msg`) and the structural-similarity scores.  The reference takes `ssim` / `msssim` from the third-party package
`pytorch_msssim` (evals/metrics.py:20, 38-54; absent from this image and not vendored in the checkout): restated here from its
published algorithm (Wang et al. 2004 / 2003: 11-tap Gaussian window, sigma 1.5, K = (0.01, 0.03), 'valid' filtering, five scales
with weights 0.0448 / 0.2856 / 0.3001 / 0.2363 / 0.1333).  The reference checkout vendors that algorithm in losses/ssim.py: this
restatement is pinned against the unmodified file (tests/golden/make_golden_ssim.py, tests/test_oracle_ssim.py: equal in float64) and
against an independent float64 scipy evaluation in tests/test_host.py.  Device fp32 inputs run on the HIP statistics kernel
(csrc/ssim.hip: one streaming pass per scale instead of ten grouped convolutions); `LAST_SSIM_BACKEND` says which path a call took.
`bit_accuracy` / `bit_accuracy_1msg` send device fp32 pixel-wise (4-D) predictions through the pixel-vote kernel (csrc/pixel_head.hip);
`LAST_VOTE_BACKEND` says which path such a call took.
"""
import math

import torch
import torch.nn.functional as F


def psnr(x: torch.Tensor, y: torch.Tensor, is_video: bool = False) -> torch.Tensor:
    """20 log10(255) - 10 log10(mean((255 (x - y))^2)), per image or over the whole clip (is_video)."""
    delta = (255 * (x - y)).reshape(-1, x.shape[-3], x.shape[-2], x.shape[-1])
    dims = (0, 1, 2, 3) if is_video else (1, 2, 3)
    return 20 * math.log10(255.0) - 10 * torch.log10(torch.mean(delta ** 2, dim=dims))


LAST_VOTE_BACKEND = None      # "hip" or "torch": which path the last bit_accuracy / bit_accuracy_1msg call on 4-D predictions took


def _vote_on_hip(preds: torch.Tensor, mask) -> bool:
    """device fp32 4-D predictions go through the pixel-vote kernel (csrc/pixel_head.hip: one read of the logits); everything else keeps the torch code"""
    return (preds.dim() == 4 and preds.is_cuda and preds.dtype == torch.float32 and preds.numel() > 0 and preds.shape[-2] * preds.shape[-1] < 2 ** 24
            and (mask is None or (torch.is_tensor(mask) and mask.is_cuda and mask.dim() == 4 and mask.shape[1] == 1
                                  and mask.shape[0] in (1, preds.shape[0]) and mask.shape[-2:] == preds.shape[-2:])))


def _hip_votes(preds, mask, threshold):
    """(votes [B, K], nsel [B]) as int64, or None when the frames select different numbers of pixels: the reference's
    `masked_select(...).view(bsz, nbits, -1)` then regroups the selected values across frames, which only the torch code reproduces"""
    from .pixel_head import pixel_vote
    with torch.no_grad():
        votes, nsel = pixel_vote(preds, mask, threshold)
    if mask is not None and not bool((nsel == nsel[0]).all()):
        return None
    return votes.long(), nsel.long()


def bit_accuracy(preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor = None, threshold: float = 0.0) -> torch.Tensor:
    """fraction of bits where (pred > threshold) == (target > 0.5); pixel-wise predictions are majority-voted first."""
    global LAST_VOTE_BACKEND
    if _vote_on_hip(preds, mask):
        vn = _hip_votes(preds, mask, threshold)
        if vn is not None:
            LAST_VOTE_BACKEND = "hip"
            votes, nsel = vn
            voted = (votes.double() / nsel.double()[:, None]) > 0.5          # the mean of the 0 / 1 decisions in double, as `.mean(dtype=float)`
            return (voted == (targets > 0.5)).float().mean(dim=-1)
    if preds.dim() == 4:
        LAST_VOTE_BACKEND = "torch"
    preds = preds > threshold
    if preds.dim() == 4:
        bsz, nbits, h, w = preds.size()
        if mask is not None:
            mask = mask.expand_as(preds).bool()
            preds = preds.masked_select(mask).view(bsz, nbits, -1).mean(dim=-1, dtype=float)
        else:
            preds = preds.mean(dim=(-2, -1), dtype=float)
        preds = preds > 0.5
    targets = targets > 0.5
    return (preds == targets).float().mean(dim=-1)


def bit_accuracy_1msg(preds: torch.Tensor, targets: torch.Tensor, masks: torch.Tensor = None, threshold: float = 0.0) -> torch.Tensor:
    """evals/metrics.py:180-206: per-pixel bit accuracy averaged over the (unmasked) pixels of each image; preds B x K x H x W.
    Return value as the reference's: with `masks` a HOST tensor (the reference builds it from `.item()` values, so this form synchronises on
    either path), without masks a tensor on the predictions' device."""
    global LAST_VOTE_BACKEND
    if _vote_on_hip(preds, masks):
        from .pixel_head import pixel_vote
        LAST_VOTE_BACKEND = "hip"
        with torch.no_grad():
            votes, nsel = pixel_vote(preds, masks, threshold)
        votes, nsel = votes.long(), nsel.long()[:, None]
        hits = torch.where(targets.to(votes.device) > 0.5, votes, nsel - votes).sum(dim=1)        # whole numbers below 2^24 x K: exact
        acc = (hits.double() / (nsel[:, 0] * preds.shape[1]).double()).float()      # the exact ratio of two whole numbers, rounded once
        return acc if masks is None else acc.cpu()                                                 # (the masked form returns a host tensor)
    LAST_VOTE_BACKEND = "torch"
    hit = ((preds > threshold) == (targets > 0.5)[:, :, None, None]).float()
    if masks is None:
        return hit.mean(dim=(1, 2, 3))
    sel = masks.expand_as(hit).bool()
    return torch.tensor([hit[i].masked_select(sel[i]).mean().item() for i in range(len(sel))])


def accuracy(preds: torch.Tensor, targets: torch.Tensor, threshold: float = 0.0) -> torch.Tensor:
    """evals/metrics.py:87-102: per-image fraction of mask pixels where (pred > threshold) == (target > 0.5); B x 1 x H x W."""
    return ((preds > threshold) == (targets > 0.5)).float().mean(dim=(1, 2, 3))


def iou(preds: torch.Tensor, targets: torch.Tensor, threshold: float = 0.0, label: int = 1) -> torch.Tensor:
    """evals/metrics.py:66-85: intersection over union of the `label` class per image.  An empty union scores 0: the reference's chained
    assignment `union[union == 0] = intersection[union == 0] = 1` patches `union` first, so its second mask is already empty and the
    intersection stays 0 (pinned against the unmodified function in tests/test_host.py)."""
    p, t = preds > threshold, targets > 0.5
    if label == 0:
        p, t = ~p, ~t
    inter = (p & t).float().sum((1, 2, 3))
    union = (p | t).float().sum((1, 2, 3))
    union[union == 0.0] = 1
    return inter / union


def linf(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """evals/metrics.py:56-64: max |x - y| in 8-bit grey levels."""
    return (x - y).abs().max() * (255.0 / data_range)


def pvalue(preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor = None, threshold: float = 0.0) -> torch.Tensor:
    """evals/metrics.py:104-121: one-sided binomial test of the number of matching bits against chance."""
    from scipy import stats
    nbits = targets.shape[-1]
    accs = bit_accuracy(preds, targets, mask, threshold)
    return torch.tensor([stats.binomtest(int(a * nbits), nbits, 0.5, alternative="greater").pvalue for a in accs])


def plogp(p: torch.Tensor) -> torch.Tensor:
    """p log2 p with 0 log 0 = 0 (evals/metrics.py:123-131)."""
    out = p * torch.log2(p)
    out[p == 0] = 0
    return out


def capacity(preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor = None, threshold: float = 0.0) -> torch.Tensor:
    """evals/metrics.py:133-148: nbits x (1 - H2(bit accuracy)), the capacity of nbits binary symmetric channels."""
    acc = bit_accuracy(preds, targets, mask, threshold)
    return targets.shape[-1] * (1 - (-plogp(acc) - plogp(1 - acc)))       # (the reference's operation order: equal to the last bit)


# ---- structural similarity (pytorch_msssim 1.0's algorithm; see the module docstring) ----

_MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _gauss_window(size: int, sigma: float, like: torch.Tensor) -> torch.Tensor:
    c = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).to(device=like.device, dtype=like.dtype)


def _blur_valid(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """separable 'valid' Gaussian filter per channel (a side shorter than the window is left unfiltered along that axis)"""
    ch = x.shape[1]
    w = win.view(1, 1, -1).repeat(ch, 1, 1)
    if x.shape[2] >= win.numel():
        x = F.conv2d(x, w.unsqueeze(-1), groups=ch)
    if x.shape[3] >= win.numel():
        x = F.conv2d(x, w.unsqueeze(-2), groups=ch)
    return x


def _ssim_cs(x, y, data_range, win, k1=0.01, k2=0.03):
    """(ssim, cs) per image and channel: means of the SSIM map and of its contrast-structure factor"""
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mu1, mu2 = _blur_valid(x, win), _blur_valid(y, win)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _blur_valid(x * x, win) - mu1_sq
    s2 = _blur_valid(y * y, win) - mu2_sq
    s12 = _blur_valid(x * y, win) - mu12
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim_map = ((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


LAST_SSIM_BACKEND = None      # "hip" or "torch": which path the last ssim / msssim call took


def _on_hip_path(x: torch.Tensor, y: torch.Tensor) -> bool:
    """device fp32 4-D inputs that nobody differentiates go to the HIP statistics kernel (csrc/ssim.hip); everything else -- CPU tensors,
    float64, inputs that require a gradient -- keeps the torch code below"""
    return (x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32 and x.dim() == 4 and x.shape == y.shape
            and not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)))


def _hip_factors(x, y, levels, data_range):
    from . import autograd as AG
    from .native import f32c
    with torch.no_grad():
        s, c, _ = AG.ssim_pyramid(f32c(x), f32c(y), levels, data_range)      # (a side shorter than 11: ValueError)
    return s, c


def ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """evals/metrics.py:38-45 (`pytorch_msssim.ssim(..., size_average=False)`): one score per image, B x C x H x W in [0, data_range].
    On the HIP path a side shorter than 11 raises ValueError (the reference skips the filter along that axis with a warning: not built)."""
    global LAST_SSIM_BACKEND
    if _on_hip_path(x, y):
        LAST_SSIM_BACKEND = "hip"
        s, _ = _hip_factors(x, y, 1, data_range)
        return s[0].mean(1).float()
    LAST_SSIM_BACKEND = "torch"
    s, _ = _ssim_cs(x, y, data_range, _gauss_window(11, 1.5, x))
    return s.mean(1)


def msssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """evals/metrics.py:47-54 (`pytorch_msssim.ms_ssim(..., size_average=False)`): five dyadic scales, sides must exceed 160."""
    global LAST_SSIM_BACKEND
    if min(x.shape[-2:]) <= (11 - 1) * 2 ** 4:
        raise AssertionError("Image size should be larger than 160 due to the 4 downsamplings in ms-ssim")
    if _on_hip_path(x, y):
        LAST_SSIM_BACKEND = "hip"
        s, c = _hip_factors(x, y, len(_MS_WEIGHTS), data_range)
        f = torch.relu(torch.cat([c[:-1], s[-1:]], dim=0))
        from .autograd import _ms_weights
        return torch.prod(f ** _ms_weights(x.device), dim=0).mean(1).float()
    LAST_SSIM_BACKEND = "torch"
    win = _gauss_window(11, 1.5, x)
    factors = []
    for level in range(len(_MS_WEIGHTS)):
        s, cs = _ssim_cs(x, y, data_range, win)
        if level < len(_MS_WEIGHTS) - 1:
            factors.append(torch.relu(cs))
            pad = [d % 2 for d in x.shape[2:]]
            x, y = F.avg_pool2d(x, kernel_size=2, padding=pad), F.avg_pool2d(y, kernel_size=2, padding=pad)
    factors.append(torch.relu(s))
    w = torch.tensor(_MS_WEIGHTS, device=x.device, dtype=x.dtype).view(-1, 1, 1)
    return torch.prod(torch.stack(factors, dim=0) ** w, dim=0).mean(1)
