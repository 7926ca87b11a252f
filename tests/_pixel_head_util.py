"""Seeded inputs of the pixel-wise head's fixtures, shared by tests/golden/make_golden_pixel_head.py (which runs the reference on them)
and by the tests (which rebuild them and check the fixture's checksums first, so that a generator mismatch on another machine reads as
such and not as a kernel error).  Everything comes from torch's CPU generator."""
import math

import numpy as np
import torch

LATENTS = ((2, 2), (3, 5))                     # odd, non-square; every pixel is near a clamped or reflected edge
STAGES = ((64, 16, 4), (96, 24, 4), (48, 24, 2), (256, 64, 4))      # C -> Co at factor f: one lane per pixel, 12-float groups, many lanes
B = 2
BWD_STAGE = (96, 24, 4, 3, 5)                  # the stage whose gradients are stored (C, Co, f, H, W)
LINEAR = tuple((k, s, hw) for k in (6, 17) for s in (False, True) for hw in ((12, 20),)) + ((6, False, (5, 7)), (17, True, (5, 7)))
LINEAR_C = 24
CHAIN = dict(embed_dim=128, stages=(4, 4, 2), nbits=16)             # a whole head: widths 32 / 8 / 4, 17 logits per pixel
LOSS_SHAPES = {"e": (2, 6, 12, 20), "o": (2, 6, 5, 7)}              # HW a multiple of 4 (16-byte path) and odd (one pixel per lane)
LOSS_MASKS = ("ones", "rect", "frac", "one_frame", "none")
LOSS_T = {"ones": 1.0, "rect": 2.0, "frac": 1.0, "one_frame": 1.0, "none": 1.0}
LOSS_W = (1.0, 0.5)                            # detect_weight, decode_weight of the gradient


def stage_name(C, Co, f, H, W):
    return f"st{C}_{Co}_x{f}_{H}x{W}"


def linear_name(K, sig, hw):
    return f"lin{K}_{'sig' if sig else 'raw'}_{hw[0]}x{hw[1]}"


def _gen(*key):
    return torch.Generator().manual_seed(1_000_003 * len(key) + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def stage_tensors(C, Co, f, H, W):
    """x [B, C, H, W], conv weight [Co, C, 3, 3], LayerNorm weight / bias [Co], dout [B, Co, fH, fW]"""
    g = _gen(C, Co, f, H, W)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(9 * C)
    lw, lb = torch.rand(Co, generator=g) + 0.5, 0.5 * torch.randn(Co, generator=g)
    dout = torch.randn(B, Co, f * H, f * W, generator=g)
    return x, w, lw, lb, dout


def linear_tensors(K, hw):
    """x [B, C, H, W], weight [K, C, 1, 1], bias [K], dpreds [B, K, H, W]"""
    g = _gen(K, hw[0], hw[1], 5)
    x = torch.randn(B, LINEAR_C, hw[0], hw[1], generator=g)
    w = torch.randn(K, LINEAR_C, 1, 1, generator=g) / math.sqrt(LINEAR_C)
    b = 0.3 * torch.randn(K, generator=g)
    dp = torch.randn(B, K, hw[0], hw[1], generator=g)
    return x, w, b, dp


def head_tensors(embed_dim, stages, nbits, seed=11):
    """the `pixel_decoder.*` entries of a pixel-wise head with the reference's names and shapes (what oracle.weights has no layout for)"""
    g = torch.Generator().manual_seed(seed * 104729 + embed_dim + nbits)
    sd, c = {}, embed_dim
    for i, f in enumerate(stages):
        co = c // f
        p = f"pixel_decoder.output_upscaling.{i}.upsample_block."
        sd[p + "2.weight"] = torch.randn(co, c, 3, 3, generator=g) / math.sqrt(9 * c)
        sd[p + "3.weight"] = torch.rand(co, generator=g) + 0.5
        sd[p + "3.bias"] = 0.5 * torch.randn(co, generator=g)
        c = co
    sd["pixel_decoder.linear.weight"] = torch.randn(nbits + 1, c, 1, 1, generator=g) / math.sqrt(c)
    sd["pixel_decoder.linear.bias"] = 0.3 * torch.randn(nbits + 1, generator=g)
    return sd


def chain_input(H, W):
    return torch.randn(B, CHAIN["embed_dim"], H, W, generator=_gen(H, W, 77))


def loss_tensors(shape_key, kind):
    """preds [B, K, H, W], masks [B, 1, H, W] float, msgs [B, K - 1] (0 / 1)"""
    Bn, K, H, W = LOSS_SHAPES[shape_key]
    g = _gen(H, W, LOSS_MASKS.index(kind), 3)
    preds = 2.0 * torch.randn(Bn, K, H, W, generator=g)
    msgs = torch.randint(0, 2, (Bn, K - 1), generator=g)
    m = torch.zeros(Bn, 1, H, W)
    if kind == "ones":
        m[:] = 1.0
    elif kind == "rect":
        m[:, :, 1:H - 1, 2:W - 2] = 1.0
    elif kind == "frac":                         # fractional values select (`masks.bool()`), exact zeros do not
        r = torch.rand(Bn, 1, H, W, generator=g)
        m = torch.where(r < 0.3, torch.zeros(()), r)
        if int((m != 0).sum()) % Bn:             # the reference's `.view(bsz, nbits, -1)` needs a selected count divisible by the batch size
            m.view(-1)[int((m.view(-1) != 0).nonzero()[0])] = 0.0
    elif kind == "one_frame":                    # frame 0 fully unselected beside a selected one (an even count, for the same reason)
        m[1, :, 1:H - 1, 1:W - 1 - ((H - 2) * (W - 2)) % 2] = 1.0
    return preds, m, msgs


def checksum(*tensors):
    return np.array([float(t.double().sum()) for t in tensors] + [float(sum((t.double() ** 2).sum() for t in tensors))])


def vote_logits(Bn, K, H, W, seed, margin=1e-3):
    """logits whose distance from the threshold 0 exceeds `margin`, so that `> threshold` is the same decision in any arithmetic"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Bn, K, H, W, generator=g)
    return torch.where(x.abs() < 2 * margin, torch.full_like(x, 4 * margin), x)


# ---- model level: tiny extractors that end in a pixel-wise head
MODEL_STAGES = {"cnx": (4, 4, 2), "vit": (4, 2, 2)}
MODEL_FRAMES = (3, 80, 72, 51)                 # frames, height, width, seed of oracle.inputs.synthetic_frames
AGGREGATIONS = (None, "avg", "squared_avg", "l1norm_avg", "l2norm_avg")
TRAIN_FRAMES = (2, 64, 64, 52)                 # the training cases: frames at the processing size, so the maps have the size of the masks
POOLED_CHAIN = (4, 2, 1)                       # on 64 channels: widths 16 / 8 / 8, then the mean over the pixels, Linear and sigmoid
TRAIN_SUB = 512                                # values kept per gradient tensor


def model_specs():
    """tag -> spec.  'cnx': the tiny ConvNeXt-V2 spec with dims [16, 32, 64, 128] (stem stride 4: a 2 x 2 latent at the 64^2 processing size) and
    the head [4, 4, 2] (widths 32 / 8 / 4), so `preds` is [F, 17, 64, 64] as for the real `_pw` cards; on the spec's own 64 channels [4, 4, 2] would
    give widths 16 / 4 / 2, which the 4-channel rule of the head refuses.  'vit': the tiny ViT spec with vit_out = 64 and the head [4, 2, 2]."""
    from oracle.weights import legacy_tiny_spec, tiny_spec
    return {"cnx": tiny_spec(dims=[16, 32, 64, 128]), "vit": legacy_tiny_spec(vit_out=64, dims=[0, 0, 0, 64])}


def model_state_dict(spec, tag, seed=3):
    """oracle.weights.make_state_dict for everything it has a layout for; the head's tensors from head_tensors"""
    from oracle.weights import make_state_dict
    sd = {k: v for k, v in make_state_dict(spec, seed=seed).items() if not k.startswith("detector.pixel_decoder.")}
    e = spec.vit_out if spec.extractor == "sam" else spec.dims[-1]
    sd.update({"detector." + k: v for k, v in head_tensors(e, MODEL_STAGES[tag], spec.nbits, seed=13).items()})
    return sd


def train_inputs(nbits):
    """frames, a rectangle mask [F, 1, S, S] and one message per frame"""
    from oracle.inputs import synthetic_frames, synthetic_msgs
    n, h, w, seed = TRAIN_FRAMES
    masks = torch.zeros(n, 1, h, w)
    masks[:, :, 10:50, 8:40] = 1.0
    return synthetic_frames(n, h, w, seed=seed), masks, synthetic_msgs(n, nbits, seed=seed)


def grad_sub(g):
    flat = g.detach().double().flatten()
    return flat[::max(1, flat.numel() // TRAIN_SUB) | 1]
