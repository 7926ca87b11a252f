"""PatchGAN discriminator of the adversarial term on the HIP path (modules/discriminator.py:89-148; csrc/disc.hip).

`NLayerDiscriminator` has the reference's constructor arguments, parameter names and shapes (`main.0.weight`, ..., the buffer `rgb2yuv.M`): a
reference state dict loads with `strict=True`, and `from_module` copies a reference instance.  Its `nn.Sequential` only holds the parameters;
`forward` is one `autograd.Function` whose forward and backward are kernel launches:

  frames -> NHWC rows (RGB, or Y for `input_nc == 1`)                                   vs_disc_input / vs_disc_input_bwd
  4 x 4 convolutions, their backward-data products on flipped weights (padding 2; the
  stride-2 layers through a zero-dilated gradient)                                      vs_conv_gemm (+ vs_dilate2)
  GroupNorm(4, C) + LeakyReLU(0.2) (layer 1: LeakyReLU alone), forward and backward     vs_groupnorm_lrelu / vs_groupnorm_lrelu_bwd
  weight gradients straight from the NHWC activations, bias gradients as column sums    vs_conv4x4_wgrad, vs_bn_partial_sums
  the one-channel last layer                                                            vs_conv4x4_n1 / _bwd / _bias_grad
  -mean(fake) and the hinge loss with their gradients (videosealloss.py:16-23, 133-134)  vs_disc_loss

Built: `input_nc` 1 or 3, `ndf` a multiple of 16, `n_layers` 2 or 3, GroupNorm, the hinge loss, `cond = None`.  `use_actnorm=True`, the "vanilla"
loss, a `cond` tensor and `UNetDiscriminatorSN` raise NotImplementedError.  No CPU / ATen fallback: without the library or a GPU `forward` raises.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import native as N
from .engine import Act, ConvW, HipEngine, pack_conv, pack_conv_bwd, rup

SLOPE = 0.2
GN_EPS = 1e-5


def adopt_weight(weight: float, global_step: int, threshold: int = 0, value: float = 0.0) -> float:
    """videosealloss.py:25-31"""
    return value if global_step < threshold else weight


def weights_init(m: nn.Module) -> None:
    """videosealloss.py:33-39: convolution weights N(0, 0.02); BatchNorm does not occur in this network, everything else keeps torch's default"""
    if m.__class__.__name__.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)


class _Engine(HipEngine):
    """the kernel wrappers and the workspace of HipEngine without a model (`conv`, `buf`, `new_act`)"""

    def __init__(self, device: torch.device, gemm: str):
        self.dev = device
        self.lib = N.lib()
        self._ws, self._ws_used = {}, {}
        self.kernel_timers, self.time_all_convs = None, False
        self.gemm = gemm
        self.use_split = gemm != "f32"            # "f32": v_mfma_f32_32x32x2_f32; "bf16x3": 3 x bf16 operand split; "f16x2": 2 x f16 split
        self.arith = 2 if gemm == "f16x2" else 3
        # the 2 x f16 split has the range of f16 (|a| * 2^4 in [2^-14, 65504)): right for images and normalised activations, not for
        # gradients, whose size nothing bounds from below.  Its backward-data products run on the fp32 MFMA path.
        self.bwd_hint = N.CONV_FORCE_F32 if gemm == "f16x2" else 0
        self.autotune = False                     # static, shape-only tile rules: nothing is timed
        self._tile_cache = {}
        self.layer_arith = {}


class UNetDiscriminatorSN(nn.Module):
    def __init__(self, *a, **k):
        raise NotImplementedError("UNetDiscriminatorSN (spectral-norm U-Net discriminator, modules/discriminator.py:151-210) is not built on the HIP "
                                  "path: train.py never constructs it; only NLayerDiscriminator is")


def check_disc_loss(disc_loss: str) -> None:
    if disc_loss == "vanilla":
        raise NotImplementedError("disc_loss='vanilla' (BCE-with-logits on the patch logits) is not built on the HIP path: train.py never passes "
                                  "it; only the hinge loss is")
    if disc_loss != "hinge":
        raise ValueError(f"disc_loss={disc_loss!r}: expected 'hinge'")


class NLayerDiscriminator(nn.Module):
    # arithmetic of the vs_conv_gemm launches.  "f16x2" (the default, as in the embedder and the extractor): forward products on the 2 x f16
    # round-to-nearest split, K walked 16 at a time -- every layer output from the second convolution on has 0.5 - 0.75 x the L2 error of the fp32 MFMA
    # chain (profiles/disc_parity.json) -- and backward-data products on the fp32 MFMA path, because the split has the range of f16 and
    # nothing bounds a gradient from below.  "f32": everything on v_mfma_f32_32x32x2_f32 (an fp32 fma chain).  "bf16x3": the 3 x bf16 split;
    # it truncates, so every product comes out ~4e-8 short, which does not average out in the sums over a map.
    gemm = "f16x2"

    def __init__(self, input_nc: int = 3, ndf: int = 32, n_layers: int = 3, use_actnorm: bool = False):
        super().__init__()
        if use_actnorm:
            raise NotImplementedError("use_actnorm=True (ActNorm with data-dependent initialisation, modules/discriminator.py:17-86) is not built "
                                      "on the HIP path: train.py never passes it; only GroupNorm(4, C) is")
        if input_nc not in (1, 3):
            raise NotImplementedError(f"input_nc={input_nc}: the HIP path reads RGB frames (3) or their Y channel (1)")
        if n_layers < 1 or ndf % 16 or ndf > 128:
            raise NotImplementedError(f"ndf={ndf}, n_layers={n_layers}: vs_groupnorm_lrelu needs widths that are multiples of 16 up to 1024")
        from .model import RGB2YUV
        self.input_nc, self.n_layers = input_nc, n_layers
        self.rgb2yuv = RGB2YUV()
        seq: List[nn.Module] = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(SLOPE, True)]
        self._plan: List[Tuple[int, Optional[int], int]] = [(0, None, 2)]          # (conv index, GroupNorm index, stride) of the dense layers
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            self._plan.append((len(seq), len(seq) + 1, 2))
            seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2, 1), nn.GroupNorm(4, ndf * mult), nn.LeakyReLU(SLOPE, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        self._plan.append((len(seq), len(seq) + 1, 1))
        seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 1, 1), nn.GroupNorm(4, ndf * mult), nn.LeakyReLU(SLOPE, True)]
        self._last = len(seq)
        seq += [nn.Conv2d(ndf * mult, 1, 4, 1, 1)]
        self.main = nn.Sequential(*seq)
        self.apply(weights_init)
        self._eng: Optional[_Engine] = None
        self._packed: Dict[tuple, tuple] = {}

    def __getstate__(self):
        """copies (copy.deepcopy, pickling) take the parameters; the engine and the packed operands are per instance and rebuilt on first use"""
        state = self.__dict__.copy()
        state["_eng"], state["_packed"] = None, {}
        return state

    @classmethod
    def from_module(cls, ref: nn.Module) -> "NLayerDiscriminator":
        """a native copy of a reference `NLayerDiscriminator` (same configuration, parameters, device)"""
        convs = [m for m in ref.main if isinstance(m, nn.Conv2d)]
        if any(m.__class__.__name__ == "ActNorm" for m in ref.main):
            raise NotImplementedError("use_actnorm=True is not built on the HIP path")
        d = cls(input_nc=int(ref.input_nc), ndf=convs[0].out_channels, n_layers=len(convs) - 2)
        d.load_state_dict(ref.state_dict(), strict=True)
        return d.to(next(ref.parameters()).device)

    # ------------------------------------------------------------------ plumbing
    def engine(self) -> _Engine:
        dev = self.main[0].weight.device
        if dev.type != "cuda":
            raise N.NativeError("NLayerDiscriminator runs on the HIP path only: move it to a cuda device (there is no CPU / ATen fallback)")
        if self._eng is None or self._eng.dev != dev or self._eng.gemm != self.gemm:
            self._eng = _Engine(dev, self.gemm)
        return self._eng

    def _pack(self, idx: int, in_ld: int, bwd: bool) -> ConvW:
        """packed operand of conv `idx` (forward, or flipped / transposed for the backward-data product), re-made when the parameter changed"""
        m = self.main[idx]
        key, stamp = (idx, in_ld, bwd), (m.weight._version, m.weight.data_ptr(), None if m.bias is None else m.bias._version)
        hit = self._packed.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        w = m.weight.detach()
        if bwd:
            p, cp = pack_conv_bwd(w, in_ld)
            cw = ConvW(p, None, w.shape[1], 4, 4, cp)
        else:
            p, cp = pack_conv(w, in_ld)
            cw = ConvW(p, N.f32c(m.bias.detach()), w.shape[0], 4, 4, cp)
        self._packed[key] = (stamp, cw)
        return cw

    def _last_w(self, ld: int) -> torch.Tensor:
        """weights of the last layer [1, C, 4, 4] -> [16 * ld] in (tap, channel) order"""
        p, cp = pack_conv(self.main[self._last].weight.detach(), ld)
        if cp != ld:
            raise N.NativeError(f"last layer: row stride {ld} of the activations is not the packed channel count {cp}")
        return p

    def forward(self, imgs: torch.Tensor, cond: Optional[torch.Tensor] = None) -> torch.Tensor:
        if cond is not None:
            raise NotImplementedError("a `cond` tensor (videosealloss.py:199-203: channels concatenated to the frames) is not built on the HIP path: "
                                      "train.py never passes one")
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"NLayerDiscriminator: frames [B, 3, H, W] expected, got {tuple(imgs.shape)}")
        return _DiscFn.apply(self, imgs, *self.parameters())

    # ------------------------------------------------------------------ launches
    def _forward(self, imgs: torch.Tensor, keep_acts: bool):
        eng, L, st = self.engine(), N.lib(), N.stream()
        dev = eng.dev
        B, _, H, W = imgs.shape
        if min(H, W) < 2 ** self.n_layers * 3:
            raise ValueError(f"frames of {H} x {W} are too small for {self.n_layers} stride-2 layers and two 4 x 4 convolutions")
        x = N.f32c(imgs)
        m0 = self.rgb2yuv.M[0].float().contiguous() if self.input_nc == 1 else None
        cur = Act(torch.empty(B * H * W * 4, device=dev), B, H, W, self.input_nc, 4)
        N.check(L.vs_disc_input(N.ptr(x), B, H, W, N.ptr(m0), N.ptr(cur.t), st), "vs_disc_input")
        S = dict(m0=m0, layers=[], in_hw=(H, W))
        for li, (ci, gi, stride) in enumerate(self._plan):
            conv = self.main[ci]
            co = conv.out_channels
            Ho, Wo = (cur.H - 2) // stride + 1, (cur.W - 2) // stride + 1
            z = Act(torch.empty(B * Ho * Wo * co, device=dev), B, Ho, Wo, co, co)          # pre-norm value: kept for the backward
            eng.conv(cur, self._pack(ci, cur.ld, False), z, stride=stride, pad=1)
            a = Act(torch.empty(z.rows * co, device=dev) if keep_acts else eng.buf(f"disc.a{li}", z.rows * co), B, Ho, Wo, co, co)
            mean = rstd = None
            if gi is None:
                N.check(L.vs_groupnorm_lrelu(N.ptr(z.t), z.ld, B, Ho * Wo, co, 0, None, None, GN_EPS, SLOPE, None, None, None, N.ptr(a.t), a.ld, st),
                        "vs_groupnorm_lrelu")
            else:
                gn = self.main[gi]
                mean, rstd = torch.empty(B * 4, device=dev, dtype=torch.float64), torch.empty(B * 4, device=dev, dtype=torch.float64)
                part = eng.buf("disc.gn.part", 2 * int(L.vs_groupnorm_partial_doubles(B, Ho * Wo, co))).view(torch.float64)
                N.check(L.vs_groupnorm_lrelu(N.ptr(z.t), z.ld, B, Ho * Wo, co, 4, N.ptr(N.f32c(gn.weight.detach())), N.ptr(N.f32c(gn.bias.detach())),
                                             float(gn.eps), SLOPE, N.ptr(part), N.ptr(mean), N.ptr(rstd), N.ptr(a.t), a.ld, st), "vs_groupnorm_lrelu")
            S["layers"].append(dict(x=cur if keep_acts else None, z=z, mean=mean, rstd=rstd))
            cur = a
        wl = self._last_w(cur.ld)
        logits = torch.empty(B, 1, cur.H - 1, cur.W - 1, device=dev, dtype=torch.float32)
        N.check(L.vs_conv4x4_n1(N.ptr(cur.t), cur.ld, B, cur.H, cur.W, N.ptr(wl), N.ptr(N.f32c(self.main[self._last].bias.detach())), N.ptr(logits), st),
                "vs_conv4x4_n1")
        S["last_x"], S["last_geom"] = (cur if keep_acts else None), (B, cur.H, cur.W, cur.ld)
        return logits, S

    def _wgrad(self, eng, dy_ptr: int, dy_ld: int, n: int, x: Act, stride: int, ci: int) -> torch.Tensor:
        L = eng.lib
        part = eng.buf("disc.wg.part", int(L.vs_conv4x4_wgrad_partial_floats(n, x.ld, x.B, x.H, x.W, stride)))
        dw = torch.empty(n, 16 * x.ld, device=eng.dev, dtype=torch.float32)
        N.check(L.vs_conv4x4_wgrad(dy_ptr, dy_ld, n, N.ptr(x.t), x.ld, x.B, x.H, x.W, stride, N.ptr(part), N.ptr(dw), N.stream()), "vs_conv4x4_wgrad")
        return dw.view(n, 4, 4, x.ld)[..., :ci].permute(0, 3, 1, 2).contiguous()

    def _colsum(self, eng, x: Act, n: int) -> torch.Tensor:
        """bias gradient: the fp64 column sums of the BatchNorm kernels"""
        L = eng.lib
        part = eng.buf("disc.cs.part", 2 * int(L.vs_bn_partial_doubles(x.rows, x.ld)))
        sums = eng.buf("disc.cs.sums", 2 * (2 * x.ld + 2)).view(torch.float64)[: 2 * x.ld + 1]
        N.check(L.vs_bn_partial_sums(N.ptr(x.t), x.rows, x.C, x.ld, N.ptr(part), N.ptr(sums), N.stream()), "vs_bn_partial_sums")
        return sums[:n].float()

    @staticmethod
    def _bwd_data(eng, dz: Act, wt: ConvW, stride: int, iH: int, iW: int, ic: int, tag: str) -> Act:
        """backward-data of a 4 x 4 convolution with padding 1: the forward kernel on the flipped, transposed weights with padding 2; a stride-2
        layer first spreads dz over an (iH - 1) x (iW - 1) map with zeros between (the zero-dilated gradient)"""
        src = dz
        if stride == 2:
            src = eng.new_act(tag + ".dil", dz.B, iH - 1, iW - 1, dz.C, dz.ld)
            N.check(eng.lib.vs_dilate2(N.ptr(dz.t), dz.B, dz.H, dz.W, dz.ld, iH - 1, iW - 1, N.ptr(src.t), N.stream()), "vs_dilate2")
        da = eng.new_act(tag + ".da", dz.B, iH, iW, ic, rup(ic, 4))
        eng.conv(src, wt, da, pad=2, tile_hint=eng.bwd_hint)
        return da

    def _backward(self, S, dlogits: torch.Tensor, want_params: bool, want_input: bool):
        """-> ({parameter name: gradient}, d imgs or None)"""
        eng, L, st = self.engine(), N.lib(), N.stream()
        dev = eng.dev
        G: Dict[str, torch.Tensor] = {}
        B, H, W, ld = S["last_geom"]
        dl = N.f32c(dlogits)
        if want_params:
            if S["last_x"] is None:
                raise N.NativeError("this forward ran with every parameter frozen: its activations were not kept for the weight gradients")
            cl = self.main[self._last].in_channels
            G[f"main.{self._last}.weight"] = self._wgrad(eng, N.ptr(dl), 1, 1, S["last_x"], 1, cl)
            db = torch.empty(1, device=dev)
            N.check(L.vs_conv4x4_n1_bias_grad(N.ptr(dl), dl.numel(), N.ptr(db), st), "vs_conv4x4_n1_bias_grad")
            G[f"main.{self._last}.bias"] = db
        da = eng.new_act("disc.da.last", B, H, W, ld, ld)
        N.check(L.vs_conv4x4_n1_bwd(N.ptr(dl), B, H, W, ld, N.ptr(self._last_w(ld)), N.ptr(da.t), st), "vs_conv4x4_n1_bwd")
        for li in range(len(self._plan) - 1, -1, -1):
            ci, gi, stride = self._plan[li]
            rec = S["layers"][li]
            z = rec["z"]
            co = z.C
            dz = eng.new_act(f"disc.dz{li}", z.B, z.H, z.W, co, co)
            if gi is None:
                N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(da.t), da.ld, N.ptr(z.t), z.ld, z.B, z.H * z.W, co, 0, None, None, None, None, SLOPE, None,
                                                 N.ptr(dz.t), dz.ld, None, None, st), "vs_groupnorm_lrelu_bwd")
            else:
                gn = self.main[gi]
                dg, dbeta = torch.empty(co, device=dev), torch.empty(co, device=dev)
                part = eng.buf("disc.gn.part", 2 * int(L.vs_groupnorm_partial_doubles(z.B, z.H * z.W, co))).view(torch.float64)
                N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(da.t), da.ld, N.ptr(z.t), z.ld, z.B, z.H * z.W, co, 4, N.ptr(N.f32c(gn.weight.detach())),
                                                 N.ptr(N.f32c(gn.bias.detach())), N.ptr(rec["mean"]), N.ptr(rec["rstd"]), SLOPE, N.ptr(part), N.ptr(dz.t),
                                                 dz.ld, N.ptr(dg), N.ptr(dbeta), st), "vs_groupnorm_lrelu_bwd")
                G[f"main.{gi}.weight"], G[f"main.{gi}.bias"] = dg, dbeta
            x = rec["x"]
            if want_params:
                G[f"main.{ci}.weight"] = self._wgrad(eng, N.ptr(dz.t), dz.ld, co, x, stride, self.main[ci].in_channels)
                G[f"main.{ci}.bias"] = self._colsum(eng, dz, co)
            if li == 0 and not want_input:
                return G, None
            xin = S["layers"][li - 1]["z"] if li > 0 else None            # geometry of this layer's input
            iB, iH, iW, ic = (xin.B, xin.H, xin.W, xin.C) if li > 0 else (z.B, S["in_hw"][0], S["in_hw"][1], self.input_nc)
            da = self._bwd_data(eng, dz, self._pack(ci, dz.ld, True), stride, iH, iW, ic, f"disc.{li}")
        dimgs = torch.empty(z.B, 3, S["in_hw"][0], S["in_hw"][1], device=dev, dtype=torch.float32)
        N.check(L.vs_disc_input_bwd(N.ptr(da.t), z.B, S["in_hw"][0], S["in_hw"][1], N.ptr(S["m0"]), N.ptr(dimgs), st), "vs_disc_input_bwd")
        return G, dimgs


class _DiscFn(torch.autograd.Function):
    """frames [B, 3, H, W] + the discriminator's parameters -> logits [B, 1, h, w]"""

    @staticmethod
    def forward(ctx, disc, imgs, *params):
        ctx.disc = disc
        ctx.keep = any(ctx.needs_input_grad[2:])           # frozen parameters: no weight gradient will be asked for, the activations are not kept
        with torch.cuda.device(disc.engine().dev):
            logits, ctx.S = disc._forward(imgs.detach(), ctx.keep)
        ctx.names = [k for k, _ in disc.named_parameters()]
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        disc = ctx.disc
        need = ctx.needs_input_grad
        want_params, want_input = any(need[2:]), need[1]
        with torch.cuda.device(disc.engine().dev):
            G, dimgs = disc._backward(ctx.S, dlogits, want_params, want_input)
        grads = []
        for n, nd, p in zip(ctx.names, need[2:], disc.parameters()):
            g = G.get(n) if nd else None
            if nd and g is None:
                raise N.NativeError(f"no gradient produced for {n}")
            grads.append(g.reshape(p.shape) if g is not None else None)
        return (None, dimgs) + tuple(grads)


# ----------------------------------------------------------------------------------------------------------------- loss nodes
def disc_loss_raw(logits_real: Optional[torch.Tensor], logits_fake: torch.Tensor, hinge: bool, gscale: float = 1.0):
    """vs_disc_loss: (out [4] = (loss, mean real, mean fake, 0), d logits_real or None, d logits_fake); the gradients are multiplied with gscale"""
    f = N.f32c(logits_fake)
    r = N.f32c(logits_real) if logits_real is not None else None
    out = torch.empty(4, device=f.device, dtype=torch.float32)
    df = torch.empty_like(f)
    dr = torch.empty_like(r) if r is not None else None
    N.check(N.lib().vs_disc_loss(N.ptr(r), r.numel() if r is not None else 0, N.ptr(f), f.numel(), 1 if hinge else 0, float(gscale), N.ptr(dr), N.ptr(df),
                                 N.ptr(out), N.stream()), "vs_disc_loss")
    return out, dr, df


class GeneratorDiscLossFn(torch.autograd.Function):
    """videosealloss.py:133-134: -mean(logits_fake)"""

    @staticmethod
    def forward(ctx, logits):
        out, _, d = disc_loss_raw(None, logits, hinge=False)
        ctx.save_for_backward(d)
        return out[0]

    @staticmethod
    def backward(ctx, up):
        (d,) = ctx.saved_tensors
        return d * up


def generator_disc_loss(logits_fake: torch.Tensor) -> torch.Tensor:
    return GeneratorDiscLossFn.apply(logits_fake)
