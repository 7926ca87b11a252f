"""Host side of the pixel-wise extractor head (csrc/pixel_head.hip; modules/pixel_decoder.py:43-83 with up-scaling stages of 2 / 4 and
`pixelwise: True`): launch wrappers of one Upsample group, of the per-pixel linear layer, of the losses on [B, 1+nbits, H, W] logits and
of the pixel vote, forward and backward.  `eng` is a HipEngine (its `conv`, `new_act` / `buf` and library handle); activations are the
engine's NHWC `Act`s, logits are plain NCHW tensors.  Nothing here falls back to torch: an unsupported width raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import native as N
from .engine import Act, ConvW, pack_conv, pack_conv_bwd, rup

FACTORS = (1, 2, 4)
BWD_ARITH = 3          # backward GEMMs on the exact 3 x bf16 split, as training.py


def check_stage(c_in: int, f: int) -> int:
    """width after one stage; the rule itself (factors 1 / 2 / 4, widths that are multiples of 4, at most 256 behind a factor 2 / 4) lives in
    layout.stage_width, which `head_cfg` applies when a model is configured"""
    from .layout import stage_width
    return stage_width(c_in, f)


def pack_stage(w: torch.Tensor, in_ld: int) -> ConvW:
    """Conv3x3 weight [Co, C, 3, 3] -> the 1 x 1 GEMM of the nine per-tap products on the low-resolution map: rows ordered (tap, channel)"""
    co, c = w.shape[0], w.shape[1]
    wz, cpz = pack_conv(w.float().permute(2, 3, 0, 1).reshape(9 * co, c)[:, :, None, None], in_ld)
    return ConvW(wz, None, 9 * co, 1, 1, cpz)


def stage_forward(eng, x: Act, wz: ConvW, lnw: torch.Tensor, lnb: torch.Tensor, f: int, tag: str, *, keep_raw: bool = False,
                  act: int = N.ACT_GELU, arith: Optional[int] = None):
    """one Upsample group at factor 2 / 4.  Returns the output Act [B, fH, fW, Co]; with keep_raw also the raw gather (pre-LayerNorm) and the
    LayerNorm output (pre-activation) that the backward needs: (out, raw, ln)."""
    L, st = eng.lib, N.stream()
    co = wz.N // 9
    if not L.vs_pixel_upgather_supported(co, f):
        raise N.NativeError(f"pixel decoder stage {x.C} -> {co} at factor {f} is not supported by vs_pixel_upgather")
    z = eng.new_act(tag + ".z", x.B, x.H, x.W, 9 * co)
    eng.conv(x, wz, z, **({} if arith is None else dict(arith=arith)))
    out = eng.new_act(tag + ".o", x.B, f * x.H, f * x.W, co)
    if not keep_raw:
        N.check(L.vs_pixel_upgather(N.ptr(z.t), z.ld, x.B, x.H, x.W, co, f, N.ptr(lnw), N.ptr(lnb), 1e-6, act, N.ptr(out.t), out.ld, st),
                "vs_pixel_upgather")
        return out
    raw = eng.new_act(tag + ".g", x.B, f * x.H, f * x.W, co)
    N.check(L.vs_pixel_upgather(N.ptr(z.t), z.ld, x.B, x.H, x.W, co, f, None, None, 1e-6, N.ACT_NONE, N.ptr(raw.t), raw.ld, st), "vs_pixel_upgather")
    ln = eng.new_act(tag + ".n", x.B, f * x.H, f * x.W, co)
    N.check(L.vs_layernorm_act(N.ptr(raw.t), raw.rows, co, raw.ld, N.ptr(lnw), N.ptr(lnb), 1e-6, N.ACT_NONE, N.ptr(ln.t), ln.ld, st), "vs_layernorm_act")
    N.check(L.vs_layernorm_act(N.ptr(raw.t), raw.rows, co, raw.ld, N.ptr(lnw), N.ptr(lnb), 1e-6, act, N.ptr(out.t), out.ld, st), "vs_layernorm_act")
    return out, raw, ln


def stage_backward(eng, x: Act, w: torch.Tensor, lnw: torch.Tensor, raw: Act, ln: Act, dout: Act, f: int, tag: str, *, want_params: bool = True,
                   want_input: bool = True) -> Tuple[Optional[Act], Dict[str, torch.Tensor]]:
    """backward of stage_forward(keep_raw=True) with GELU: dout [B, fH, fW, Co] -> (dx or None, {"conv": [Co, C, 3, 3], "lnw": [Co], "lnb": [Co]})"""
    L, st = eng.lib, N.stream()
    co, c = w.shape[0], w.shape[1]
    dn = eng.new_act(tag + ".dn", raw.B, raw.H, raw.W, co)
    N.check(L.vs_gelu_bwd(N.ptr(ln.t), ln.ld, N.ptr(dout.t), dout.ld, ln.rows, co, N.ptr(dn.t), dn.ld, st), "vs_gelu_bwd")
    dg = eng.new_act(tag + ".dg", raw.B, raw.H, raw.W, co)
    stats = eng.buf(tag + ".ln.stats", 2 * raw.rows)
    part = eng.buf(tag + ".ln.part", int(L.vs_colreduce_partial_floats(1, raw.rows, raw.ld)))
    dlw = torch.empty(co, device=eng.dev, dtype=torch.float32)
    dlb = torch.empty(co, device=eng.dev, dtype=torch.float32)
    N.check(L.vs_layernorm_bwd(N.ptr(raw.t), raw.ld, N.ptr(dn.t), dn.ld, N.ptr(lnw), raw.rows, co, 1e-6, N.ptr(dg.t), dg.ld, N.ptr(stats), N.ptr(part),
                               N.ptr(dlw), N.ptr(dlb), st), "vs_layernorm_bwd")
    dz = eng.new_act(tag + ".dz", x.B, x.H, x.W, 9 * co)
    N.check(L.vs_pixel_upgather_bwd(N.ptr(dg.t), dg.ld, x.B, x.H, x.W, co, f, N.ptr(dz.t), dz.ld, st), "vs_pixel_upgather_bwd")
    G = {"lnw": dlw, "lnb": dlb}
    if want_params:
        wpart = eng.buf(tag + ".wg.part", int(L.vs_gemm_wgrad_partial_floats(dz.rows, 9 * co, c)))
        dwz = torch.empty(9 * co, c, device=eng.dev, dtype=torch.float32)
        N.check(L.vs_gemm_wgrad(N.ptr(dz.t), dz.ld, 9 * co, N.ptr(x.t), x.ld, c, dz.rows, N.ptr(wpart), N.ptr(dwz), st), "vs_gemm_wgrad")
        G["conv"] = dwz.view(3, 3, co, c).permute(2, 3, 0, 1).contiguous()
    dx = None
    if want_input:
        w2d = w.float().permute(2, 3, 0, 1).reshape(9 * co, c).contiguous()
        p, cp = pack_conv_bwd(w2d[:, :, None, None], dz.ld)                   # dX = dZ Wz: [C][9 Co]
        dx = eng.new_act(tag + ".dx", x.B, x.H, x.W, c, x.ld)
        if x.ld != rup(c, 4):
            dx.t.zero_()
        eng.conv(dz, ConvW(p, None, c, 1, 1, cp), dx, arith=BWD_ARITH)
    return dx, G


def linear_forward(x: Act, w: torch.Tensor, b: Optional[torch.Tensor], sigmoid: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """per-pixel linear layer: NHWC x, w [K, C] (or [K, C, 1, 1]), b [K] -> NCHW [B, K, H, W] (sigmoid applied when asked)"""
    K = w.shape[0]
    w = N.f32c(w.reshape(K, -1))
    if out is None:
        out = torch.empty(x.B, K, x.H, x.W, device=x.t.device, dtype=torch.float32)
    N.check(N.lib().vs_pixel_linear(N.ptr(x.t), x.ld, x.B, x.H * x.W, x.C, N.ptr(w), N.ptr(b), K, 1 if sigmoid else 0, N.ptr(out), N.stream()),
            "vs_pixel_linear")
    return out


def linear_backward(x: Act, w: torch.Tensor, dpreds: torch.Tensor, y: Optional[torch.Tensor] = None, *, want_params: bool = True,
                    want_input: bool = True):
    """backward of linear_forward: dpreds [B, K, H, W] (y: the sigmoid output when the layer applied one) -> (dx Act or None, dw [K, C], db [K])"""
    L = N.lib()
    K = w.shape[0]
    w = N.f32c(w.reshape(K, -1))
    dpreds = N.f32c(dpreds)
    dev = x.t.device
    dx = Act(torch.zeros(x.rows * x.ld, device=dev), x.B, x.H, x.W, x.C, x.ld) if want_input else None
    dw = db = part = None
    if want_params:
        dw, db = torch.empty(K, x.C, device=dev), torch.empty(K, device=dev)
        part = torch.empty(int(L.vs_pixel_linear_bwd_partial_floats(x.rows, K, x.C)), device=dev)
    N.check(L.vs_pixel_linear_bwd(N.ptr(dpreds), N.ptr(y), N.ptr(x.t), x.ld, x.B, x.H * x.W, x.C, N.ptr(w), K, N.ptr(dx.t) if dx else None,
                                  dx.ld if dx else 0, N.ptr(dw), N.ptr(db), N.ptr(part), N.stream()), "vs_pixel_linear_bwd")
    return dx, dw, db


def pixel_bce(preds: torch.Tensor, masks: torch.Tensor, msgs_i32: torch.Tensor, *, temperature: float = 1.0, w_det: float = 1.0,
              w_dec: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """videosealloss.py:138-167 on pixel-wise logits: (loss, dpreds) with loss[0] = detection, loss[1] = masked decoding (NaN with nothing selected) and
    dpreds = w_det d loss[0] + w_dec d loss[1].  preds [B, 1+nbits, H, W], masks [B, 1, H, W] (float; non-zero selects), msgs [1 | B, nbits] int32."""
    B, K, H, W = preds.shape
    if tuple(masks.shape[-2:]) != (H, W) or masks.numel() != B * H * W:
        raise ValueError(f"mask of shape {tuple(masks.shape)} does not match the predictions {tuple(preds.shape)}")
    L = N.lib()
    preds, masks = N.f32c(preds), N.f32c(masks)
    if preds.data_ptr() % 16:               # a view that starts inside another tensor: the kernel reads 16-byte pieces
        preds = preds.clone()
    msgs_i32 = msgs_i32.to(torch.int32).contiguous()
    dpreds = torch.empty_like(preds)
    loss = torch.empty(2, device=preds.device, dtype=torch.float32)
    part = torch.empty(int(L.vs_pixel_bce_partial_doubles(B, K, H * W)), device=preds.device, dtype=torch.float64)
    N.check(L.vs_pixel_bce(N.ptr(preds), N.ptr(masks), N.ptr(msgs_i32), msgs_i32.shape[0], B, K, H * W, float(temperature), float(w_det), float(w_dec),
                           N.ptr(dpreds), N.ptr(part), N.ptr(loss), N.stream()), "vs_pixel_bce")
    return loss, dpreds


def pixel_vote(preds: torch.Tensor, masks: Optional[torch.Tensor], threshold: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(votes [B, K] int32, nsel [B] int32): selected pixels above the threshold per frame and channel, selected pixels per frame.  preds may be a
    channel slice of a wider contiguous tensor (`preds[:, 1:]`): it is read in place."""
    B, K, H, W = preds.shape
    HW = H * W
    s = preds.stride()
    if preds.dtype != torch.float32 or (s[1], s[2], s[3]) != (HW, W, 1) or (B > 1 and s[0] < K * HW):
        preds = N.f32c(preds).contiguous()
        s = preds.stride()
    bs = s[0] if B > 1 else K * HW
    m = None
    if masks is not None:
        if tuple(masks.shape[-2:]) != (H, W):
            raise ValueError(f"mask of shape {tuple(masks.shape)} does not match the predictions {tuple(preds.shape)}")
        m = N.f32c(masks.expand(B, 1, H, W)).contiguous()
    votes = torch.empty(B, K, device=preds.device, dtype=torch.int32)
    nsel = torch.empty(B, device=preds.device, dtype=torch.int32)
    N.check(N.lib().vs_pixel_vote(N.ptr(preds), bs, N.ptr(m), B, K, HW, float(threshold), N.ptr(votes), N.ptr(nsel), N.stream()), "vs_pixel_vote")
    return votes, nsel


# ---- a whole head: the chain of Upsample groups, then the per-pixel linear layer (or the pooled one of the per-frame extractors)
def pack_head(g, prefix: str, embed_dim: int, stages, in_ld: int, pixelwise: bool, sigmoid: bool) -> dict:
    """`g(name)` -> parameter; the packed operands of head_forward.  Factor-1 stages keep the 3 x 3 conv (reflect padding) of the per-frame head."""
    P = dict(stages=[], pixelwise=bool(pixelwise), sigmoid=bool(sigmoid))
    c, ld = int(embed_dim), in_ld
    for i, f in enumerate(stages):
        co = check_stage(c, int(f))
        p = f"{prefix}.output_upscaling.{i}.upsample_block."
        w = g(p + "2.weight").float()
        st = dict(f=int(f), co=co, lnw=g(p + "3.weight").float().contiguous(), lnb=g(p + "3.bias").float().contiguous())
        if f == 1:
            wc, cp = pack_conv(w, ld)
            st["conv"] = ConvW(wc, None, co, 3, 3, cp)
        else:
            st["gemm"] = pack_stage(w, ld)
        P["stages"].append(st)
        c, ld = co, rup(co, 4)
    K = g(prefix + ".linear.weight").shape[0]
    P["lin_w"] = g(prefix + ".linear.weight").float().reshape(K, c).contiguous()
    P["lin_b"] = g(prefix + ".linear.bias").float().contiguous()
    return P


def head_forward(eng, cur: Act, P: dict, tag: str = "phead") -> torch.Tensor:
    """pixel_decoder.py:61-83 for a chain of stages: [B, 1+nbits, fH, fW] logits when pixel-wise, [B, 1+nbits] after the mean over the pixels otherwise"""
    for i, s in enumerate(P["stages"]):
        if s["f"] == 1:
            hc = eng.new_act(f"{tag}.{i}.c", cur.B, cur.H, cur.W, s["co"])
            eng.conv(cur, s["conv"], hc, pad=1, pad_mode=N.PAD_REFLECT)
            nxt = eng.new_act(f"{tag}.{i}.o", cur.B, cur.H, cur.W, s["co"])
            eng.layernorm(hc, s["lnw"], s["lnb"], nxt, act=N.ACT_GELU)
            cur = nxt
        else:
            cur = stage_forward(eng, cur, s["gemm"], s["lnw"], s["lnb"], s["f"], f"{tag}.{i}")
    K = P["lin_w"].shape[0]
    if P["pixelwise"]:
        # a fresh tensor, not an engine buffer: the caller owns the result and needs no copy of it (0.8 GB at 32 x 97 x 256^2)
        out = torch.empty(cur.B, K, cur.H, cur.W, device=cur.t.device, dtype=torch.float32)
        return linear_forward(cur, P["lin_w"], P["lin_b"], P["sigmoid"], out)
    out = eng.buf(f"{tag}.logits", cur.B * K).view(cur.B, K)
    if not P["sigmoid"]:
        N.check(eng.lib.vs_pool_linear(N.ptr(cur.t), cur.B, cur.H * cur.W, cur.C, cur.ld, N.ptr(P["lin_w"]), N.ptr(P["lin_b"]), K, N.ptr(out), N.stream()),
                "vs_pool_linear")
        return out
    # sigmoid_output on a pooled head: the mean over the pixels, then the linear kernel with its sigmoid on B "pixels"
    pooled = eng.buf(f"{tag}.pooled", cur.B * cur.ld)
    N.check(eng.lib.vs_colmean(N.ptr(cur.t), cur.B, cur.H * cur.W, cur.ld, N.ptr(pooled), N.stream()), "vs_colmean")
    return linear_forward(Act(pooled, cur.B, 1, 1, cur.C, cur.ld), P["lin_w"], P["lin_b"], True, out)
