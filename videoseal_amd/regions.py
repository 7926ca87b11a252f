"""Region-wise watermarks: the torch definition of what `Videoseal.embed_regions` / `decode_regions` / `detect_regions` compute on the HIP
path (csrc/shell.hip mode TAIL_REGIONS, csrc/regions.hip; include/videoseal_regions.h), and their argument checks.

A label map is uint8 [F, H, W]: 0 is background, r in 1 .. R selects message r - 1, a value above R counts as background.  Regions are
disjoint by construction; fractional masks are not covered.

  embed   : a pixel of label r > 0 is the pixel of `embed(imgs, msgs[r - 1])`; a pixel of label 0 is the pixel of `imgs`, bit for bit.
            For binary masks that is the reference's blend (augmenter.py: imgs_w * m + imgs * (1 - m)) applied once per region.
  decode  : evals/metrics.py:208-256 (`bit_accuracy_inference`) per region, the region's pixels taken from the label map sampled at the
            centres of the map's pixels (`label_index`).
  detect  : `detect_images` on the bounding box of every region.
Everything here is plain torch and runs on the CPU; nothing in this module launches a kernel.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

REGIONS_MAX = 8          # VS_REGIONS_MAX: with chunk_size key frames per pass the U-Net sees keys * R frames, and its passes are sized for 32
UNET_FRAMES = 32

DECODE_METHODS = ("hard", "semihard")


# ---------------------------------------------------------------------------------------------------------------- argument checks
def check_labels(labels, F: int, H: int, W: int) -> None:
    if not torch.is_tensor(labels):
        raise TypeError(f"labels must be a uint8 tensor [F, H, W], got {type(labels).__name__}")
    if labels.dtype != torch.uint8:
        raise TypeError(f"labels must be uint8 (0 = background, r = region r), got {labels.dtype}: fractional masks are not covered")
    if labels.dim() != 3 or tuple(labels.shape) != (F, H, W):
        raise ValueError(f"labels of shape {tuple(labels.shape)} do not match {F} frames of {H} x {W}")


def check_regions(R: int) -> int:
    if isinstance(R, bool) or not isinstance(R, int):
        raise TypeError(f"the number of regions must be an int, got {type(R).__name__}")
    if R < 1 or R > REGIONS_MAX:
        raise ValueError(f"{R} regions: between 1 and {REGIONS_MAX} (the U-Net sees key frames x regions frames per pass)")
    return R


def check_frames(imgs, what: str) -> Tuple[int, int, int, bool]:
    """(F, H, W, uint8?) of fp32 [F, 3, H, W] or uint8 RGB24 [F, H, W, 3] frames; everything else is refused with the reason"""
    if isinstance(imgs, (list, tuple)):
        raise NotImplementedError(f"{what} takes one clip: lists of images or clips (embed_images / embed_clips) carry no label maps")
    if not torch.is_tensor(imgs):
        raise NotImplementedError(f"{what} takes fp32 [F, 3, H, W] or uint8 RGB24 [F, H, W, 3] frames: YUV and packed-RGB clips carry no label maps")
    if imgs.requires_grad:
        raise NotImplementedError(f"{what} is an inference call: autograd does not pass through it (the training path blends with masks, forward())")
    if imgs.dim() != 4:
        raise ValueError(f"{what} wants 4-D frames, got {tuple(imgs.shape)}")
    if imgs.dtype == torch.uint8:
        if imgs.shape[-1] != 3:
            raise ValueError(f"{what}: uint8 frames must be RGB24 [F, H, W, 3]")
        return imgs.shape[0], imgs.shape[1], imgs.shape[2], True
    if imgs.shape[1] != 3:
        raise ValueError(f"{what}: float frames must be [F, 3, H, W]")
    return imgs.shape[0], imgs.shape[2], imgs.shape[3], False


def check_msgs(msgs, F: int, is_video: bool) -> int:
    """-> R.  [R, k] for both modes, [F, R, k] in image mode only (video mode keeps 'message unique per region')"""
    if not torch.is_tensor(msgs) or msgs.dim() not in (2, 3):
        raise ValueError("msgs must be [R, k] (one message per region) or, in image mode, [F, R, k]")
    if msgs.requires_grad:
        raise NotImplementedError("embed_regions is an inference call: autograd does not pass through it")
    if msgs.dim() == 3:
        if is_video:
            raise ValueError("video mode keeps one message per region: msgs must be [R, k]")
        if msgs.shape[0] != F:
            raise ValueError(f"msgs has {msgs.shape[0]} rows of regions for {F} images")
    return check_regions(int(msgs.shape[-2]))


def check_decode(method: str, per: str) -> None:
    if method == "soft":
        raise NotImplementedError("method='soft' weighs pixels by a fractional mask; a label map has no fractional weights")
    if method not in DECODE_METHODS:
        raise ValueError(f"unknown method {method!r}: one of {DECODE_METHODS}")
    if per not in ("frame", "clip"):
        raise ValueError(f"per must be 'frame' or 'clip', got {per!r}")


# ---------------------------------------------------------------------------------------------------------------- label maps
def labels_from_masks(masks: torch.Tensor) -> torch.Tensor:
    """masks [F, R, H, W] (any dtype; non-zero selects) -> uint8 labels [F, H, W]: where masks overlap the highest r wins"""
    if not torch.is_tensor(masks) or masks.dim() != 4:
        raise ValueError("masks must be [F, R, H, W]")
    R = check_regions(int(masks.shape[1]))
    labels = torch.zeros((masks.shape[0],) + tuple(masks.shape[2:]), dtype=torch.uint8, device=masks.device)
    for r in range(R):
        labels = torch.where(masks[:, r] != 0, torch.full_like(labels, r + 1), labels)
    return labels


def clean_labels(labels: torch.Tensor, R: int) -> torch.Tensor:
    """a value above R counts as background"""
    return torch.where(labels > R, torch.zeros_like(labels), labels)


def label_index(n_map: int, n_frame: int) -> torch.Tensor:
    """row (or column) of the label map that map row (column) i looks at: ((2 i + 1) n_frame) // (2 n_map), the pixel under the centre of
    map pixel i, in integer arithmetic; the identity when the sizes agree"""
    i = torch.arange(n_map, dtype=torch.int64)
    return ((2 * i + 1) * n_frame) // (2 * n_map)


def labels_at_map(labels: torch.Tensor, S_h: int, S_w: int) -> torch.Tensor:
    """labels [F, H, W] -> [F, S_h, S_w] by `label_index` (what vs_pixel_vote_regions reads without storing it)"""
    iy = label_index(S_h, labels.shape[1]).to(labels.device)
    ix = label_index(S_w, labels.shape[2]).to(labels.device)
    return labels[:, iy][:, :, ix]


# ---------------------------------------------------------------------------------------------------------------- embed
def compose(imgs: torch.Tensor, per_region: Sequence[torch.Tensor], labels: torch.Tensor, background: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the region-wise result from the R whole-frame results: pixel p of frame f is per_region[labels[f, p] - 1][f, :, p], or `imgs` (or
    `background`) where the label is 0 or above R.  fp32 [F, C, H, W] or uint8 [F, H, W, 3] frames."""
    R = len(per_region)
    out = imgs if background is None else background
    lab = clean_labels(labels, R)
    sel = lab[:, :, :, None] if imgs.dtype == torch.uint8 else lab[:, None]
    for r, w in enumerate(per_region):
        out = torch.where(sel == r + 1, w, out)
    return out


def blend_reference(imgs: torch.Tensor, per_region: Sequence[torch.Tensor], labels: torch.Tensor) -> torch.Tensor:
    """the reference's own blend (augmenter.py: imgs_w * m + imgs * (1 - m)) applied once per region with the binary mask of that region"""
    x = imgs
    for r, w in enumerate(per_region):
        m = (labels == r + 1)[:, None].to(imgs.dtype)
        x = w * m + x * (1 - m)
    return x


def embed_regions(embed: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], imgs: torch.Tensor, labels: torch.Tensor,
                  msgs: torch.Tensor) -> torch.Tensor:
    """the definition: `embed(imgs, msgs_r) -> imgs_w` once per region (msgs [R, k]: msgs_r = msgs[r:r + 1]; [F, R, k]: msgs[:, r]),
    composed by the label map"""
    F_, H, W, _ = check_frames(imgs, "embed_regions")
    check_labels(labels, F_, H, W)
    R = check_regions(int(msgs.shape[-2]))
    per_region = [embed(imgs, msgs[r:r + 1] if msgs.dim() == 2 else msgs[:, r]) for r in range(R)]
    return compose(imgs, per_region, labels)


# ---------------------------------------------------------------------------------------------------------------- decode
def vote_regions(preds: torch.Tensor, labels: torch.Tensor, R: int, threshold: float = 0.0):
    """preds [B, K, S_h, S_w] fp32, labels [B, H, W] -> (votes int64 [B, R, K], nsel int64 [B, R], sums float64 [B, R, K]): per region the
    pixels above the threshold, the pixels, and the float64 sum of the logits"""
    lab = clean_labels(labels_at_map(labels, preds.shape[-2], preds.shape[-1]), R)
    votes, nsel, sums = [], [], []
    for r in range(1, R + 1):
        sel = (lab == r)[:, None]
        votes.append(((preds > threshold) & sel).sum((-2, -1)))
        nsel.append(sel.sum((-3, -2, -1)))
        sums.append(torch.where(sel, preds.double(), torch.zeros((), dtype=torch.float64, device=preds.device)).sum((-2, -1)))
    return torch.stack(votes, 1), torch.stack(nsel, 1), torch.stack(sums, 1)


def decide(votes: torch.Tensor, nsel: torch.Tensor, sums: torch.Tensor, method: str = "hard", per: str = "frame") -> dict:
    """evals/metrics.py:208-256 on the counts: hard: score = votes / count, semihard: score = sums / count (the mean logit), float64;
    the bit is `score > 0.5` in BOTH (the reference compares the mean logit with 0.5 too, line 252).  An empty region has a NaN score,
    False bits and count 0.  per='clip' adds votes, sums and counts over the frames first and answers [1, R, k]."""
    check_decode(method, per)
    if per == "clip":
        votes, nsel, sums = votes.sum(0, keepdim=True), nsel.sum(0, keepdim=True), sums.sum(0, keepdim=True)
    num = votes.double() if method == "hard" else sums.double()
    score = num / nsel.double()[..., None]           # 0 / 0 = NaN, as the reference's mean over nothing
    return {"msgs": score > 0.5, "score": score, "count": nsel.to(torch.int32)}


def decode_regions(preds: torch.Tensor, labels: torch.Tensor, R: int, method: str = "hard", threshold: float = 0.0, per: str = "frame") -> dict:
    """the definition on the detector's maps preds [F, 1 + k, S_h, S_w]: channels 1.. are the message"""
    check_decode(method, per)
    return decide(*vote_regions(preds[:, 1:].float(), labels, check_regions(R), threshold), method, per)


# ---------------------------------------------------------------------------------------------------------------- boxes
def label_boxes(labels: torch.Tensor, R: int) -> torch.Tensor:
    """int32 [F, R, 4] = (y0, x0, y1, x1) with exclusive ends; (0, 0, 0, 0) for a label without a pixel"""
    F_, H, W = labels.shape
    boxes = torch.zeros(F_, check_regions(R), 4, dtype=torch.int32)
    for f in range(F_):
        for r in range(1, R + 1):
            ys, xs = torch.nonzero(labels[f] == r, as_tuple=True)
            if ys.numel():
                boxes[f, r - 1] = torch.tensor([int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1], dtype=torch.int32)
    return boxes
