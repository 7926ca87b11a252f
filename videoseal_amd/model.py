"""The ``Videoseal`` nn.Module surface on top of the HIP engine.

Drop-in boundary: same constructor products, attributes, method signatures, state_dict
keys and error behaviour as the reference's ``videoseal.models.Videoseal`` (models/videoseal.py:15-428,
models/wam.py:18-234) for the inference path ``embed / detect / extract_message`` plus the forward-only
``forward``; all arithmetic runs in hand-written gfx950 kernels (engine.py -> native.py -> csrc/).

Deliberate differences, each loud rather than silent:
  * no CPU / ATen execution path: the model must live on a ROCm device (``.to('cuda')``);
  * ``forward`` is differentiable (videoseal_amd/autograd.py): with autograd enabled and trainable parameters it returns tensors
    whose graph nodes run the HIP backward kernels, so train.py's `loss.backward()` / `torch.autograd.grad(loss, last_layer)` / DDP hooks
    work unchanged; under ``torch.no_grad()`` (or with everything frozen) it is the values-only launch sequence;
  * frames handed over on the CPU are copied to the model's device, processed there end to end and the
    results are copied back to ``imgs.device`` (the reference keeps the full-resolution shell on the CPU); for a CPU caller the
    no-grad entry points return tensors from torch's caching pinned allocator (``_result_buffer``).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import native as N
from . import switches as SW
from .engine import Act, HipEngine
from .layout import ModelCfg, build_tree, detector_entries, embedder_entries

_DEFAULT_INTERP = {"mode": "bilinear", "align_corners": False, "antialias": True}


_PINNED_RESULTS = SW.flag("VIDEOSEAL_PINNED_RESULTS", True)


def _result_buffer(shape, dtype, device) -> torch.Tensor:
    """Where a result goes when the caller's frames are not on the model's device.  For a CPU caller (the calling convention of
    videoseal.py:286-297 / inference_av.py: the clip stays on the CPU) the tensor comes from torch's caching PINNED allocator: the copy
    back runs at link speed instead of through a freshly mapped pageable tensor (32 x 768^2 fp32 frames: 4 ms instead of ~40 ms,
    tools/bench_pcie.py).  It is an ordinary CPU tensor for the caller; VIDEOSEAL_PINNED_RESULTS=0 returns pageable memory."""
    device = torch.device(device)
    if device.type == "cpu" and _PINNED_RESULTS:
        try:
            return torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
        except RuntimeError:          # the host refuses to lock that much memory: pageable result, same values
            pass
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def _raw_frames(x) -> bool:
    """frames that travel in their own format: uint8 tensors (RGB24), YUV clips (yuv.Clip, NV12 clips among them) and packed RGB clips
    (rgbpack.Clip); everything else is fp32 NCHW"""
    return not torch.is_tensor(x) or x.dtype == torch.uint8


def _refuse_half(x, what: str, why: str) -> None:
    """float16 / bfloat16 frames have a fused route of their own (embed_half / detect_half, halfpix.py) and no other: `what` would turn them
    into fp32 frames silently and answer in fp32"""
    ts = x if isinstance(x, (list, tuple)) else [x]
    if any(torch.is_tensor(t) and t.dtype in (torch.float16, torch.bfloat16) for t in ts):
        raise NotImplementedError(f"{what} does not take half-precision clips: {why} (embed_half / detect_half take one float16 / bfloat16 clip)")


def _empty_like(x):
    return torch.empty_like(x) if torch.is_tensor(x) else x.empty_like()


def _to_caller(t, device):
    """device tensor -> the caller's device (no-grad result paths)"""
    if not torch.is_tensor(t) or t.device == torch.device(device):
        return t
    if torch.device(device).type != "cpu" or not t.is_cuda:
        return t.to(device)
    out = _result_buffer(t.shape, t.dtype, device)
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return out


def _antialias_flag(interpolation: Optional[dict]) -> bool:
    it = dict(_DEFAULT_INTERP if interpolation is None else interpolation)
    if it.get("mode", "bilinear") != "bilinear" or it.get("align_corners", False):
        raise NotImplementedError(f"interpolation {it}: the HIP path implements mode='bilinear', align_corners=False "
                                  f"(antialias True/False)")
    return bool(it.get("antialias", False))


def psnr_strength(energy: float, n: int, target_psnr: float, max_scaling_w: Optional[float] = None) -> float:
    """The strength that puts a perturbation of energy `energy` (the sum of its squares over `n` elements, data range 1, at strength 1) at
    `target_psnr` dB: 10^(-T / 20) * sqrt(n / energy) in float64, 0 for a zero perturbation, at most `max_scaling_w`.  The host statement
    of what vs_psnr_scale evaluates on the device (there rounded once to fp32)."""
    import math
    if energy == 0.0:
        return 0.0
    s = 10.0 ** (-float(target_psnr) / 20.0) * math.sqrt(float(n) / float(energy))
    return min(s, float(max_scaling_w)) if max_scaling_w is not None else s


def check_psnr_args(target_psnr, per: str, max_scaling_w) -> None:
    """the argument checks of Videoseal.embed_psnr that need neither frames nor a device"""
    import math

    def number(v, what):        # Python and numpy scalars, 0-dim tensors; a bool or a string is not a number of dB
        if isinstance(v, (bool, str, bytes)):
            raise ValueError(f"{what} must be a number (got {v!r})")
        try:
            return float(v)
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"{what} must be a number (got {v!r}: {e})") from None

    t = number(target_psnr, "target_psnr")
    if not math.isfinite(t) or t <= 0:
        raise ValueError(f"target_psnr must be finite and positive, in dB (got {target_psnr!r})")
    if per not in ("frame", "clip"):
        raise ValueError(f'per must be "frame" or "clip" (got {per!r})')
    if max_scaling_w is not None:
        c = number(max_scaling_w, "max_scaling_w")
        if not math.isfinite(c) or c <= 0:
            raise ValueError(f"max_scaling_w must be finite and positive, or None (got {max_scaling_w!r})")


class _EngineOwner:
    """Lazily (re)builds the packed-weight engine when parameters, device or mode change."""

    def _engine_for(self, root: "Wam") -> HipEngine:
        return root._engine()


class Embedder(nn.Module):
    """``model.embedder(imgs01, msgs) -> delta`` (models/embedder.py:130-165).  Holds ``unet`` / ``msg_processor``
    parameter trees; ``yuv`` tells Wam to feed the Y channel (embedder.py:281)."""

    def __init__(self, cfg: ModelCfg, seed: int = 0):
        super().__init__()
        tree = build_tree(embedder_entries(cfg), seed)
        self.unet = tree.unet
        self.msg_processor = tree.msg_processor
        self.cfg = cfg
        self.yuv = cfg.yuv
        self._root = None      # set by Wam (plain attribute holder, avoids a module cycle)

    def get_random_msg(self, bsz: int = 1, nb_repetitions: int = 1) -> torch.Tensor:
        k = self.cfg.nbits                                   # msg_processor.py:45-59
        if nb_repetitions != 1:
            assert k % nb_repetitions == 0, f"nbits must be divisible by nb_repetitions, got {k} and {nb_repetitions}"
            aux = torch.randint(0, 2, (bsz, k // nb_repetitions))
            return aux.unsqueeze(1).repeat(1, nb_repetitions, 1).view(bsz, k)
        return torch.randint(0, 2, (bsz, k))

    def get_last_layer(self) -> torch.Tensor:
        return self.unet.outc.weight                         # embedder.py:147-149

    def forward(self, imgs: torch.Tensor, msgs: torch.Tensor) -> torch.Tensor:
        root = self._root[0]
        eng = root._engine()
        with torch.cuda.device(eng.dev):
            x = N.f32c(imgs.to(eng.dev))
            B, Cc, H, W = x.shape
            if Cc != self.cfg.in_ch:
                raise ValueError(f"embedder expects {self.cfg.in_ch} input channel(s), got {Cc}")
            ident = (1.0, 0.0, 0.0)
            import ctypes as C
            key = eng.new_act("emb.in", B, H, W, Cc, 4)
            ymat = (C.c_float * 3)(*ident) if Cc == 1 else None
            N.check(eng.lib.vs_resize_pre(N.ptr(x), B, Cc, H, W, H, W, 0, None, 1.0, 0.0, N.ptr(key.t), 1, ymat, N.stream()), "vs_resize_pre")
            delta = eng.embedder_forward(key, _msgs_i32(msgs, eng.dev), bn_train=self.training)
            return delta.clone().to(imgs.device)


class Extractor(nn.Module):
    """``model.detector(imgs01) -> logits [b, 1+nbits]`` (models/extractor.py:140-167)."""

    def __init__(self, cfg: ModelCfg, seed: int = 0):
        super().__init__()
        tree = build_tree(detector_entries(cfg), seed + 1)
        if cfg.extractor == "sam":            # SegmentationExtractor (extractor.py:40-75): image_encoder + pixel_decoder
            self.image_encoder = tree.image_encoder
        else:
            self.convnext = tree.convnext
        self.pixel_decoder = tree.pixel_decoder
        self.cfg = cfg
        self._root = None

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        root = self._root[0]
        eng = root._engine()
        with torch.cuda.device(eng.dev):
            x = N.f32c(imgs.to(eng.dev))
            rgb, _ = eng.resize_pre(x, (x.shape[-2], x.shape[-1]), False, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
            p = eng.extractor_forward(rgb)
            return (p if eng.preds_owned else p.clone()).to(imgs.device)


class Blender(nn.Module):
    """models/blender.py:12-68: only the additive mode is used by the released cards."""
    AVAILABLE_BLENDING_METHODS = ["additive"]

    def __init__(self, scaling_i: float, scaling_w: float, method: str = "additive"):
        super().__init__()
        if method != "additive":
            raise NotImplementedError(f"blending method '{method}': only 'additive' is implemented in the HIP path")
        self.method, self.scaling_i, self.scaling_w = method, scaling_i, scaling_w


class RGB2YUV(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("M", torch.tensor([[0.299, 0.587, 0.114], [-0.14713, -0.28886, 0.436], [0.615, -0.51499, -0.10001]],
                                               dtype=torch.float32))


class _Kernel2d(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.weight = nn.Parameter(k, requires_grad=False)


class JND(nn.Module):
    """modules/jnd.py:11-114 parameter holder (frozen 3x3 Sobel / 5x5 luminance taps live in the state_dict);
    ``heatmaps`` runs the HIP kernel."""

    def __init__(self, in_channels: int = 1, out_channels: int = 3):
        super().__init__()
        if (in_channels, out_channels) != (1, 1):
            raise NotImplementedError("JND: only in_channels=1, out_channels=1 (jnd_1_1, used by every released card)")
        self.in_channels, self.out_channels = in_channels, out_channels
        kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]])
        ky = torch.tensor([[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]])
        kl = torch.tensor([[1., 1., 1., 1., 1.], [1., 2., 2., 2., 1.], [1., 2., 0., 2., 1.], [1., 2., 2., 2., 1.], [1., 1., 1., 1., 1.]])
        self.conv_x = _Kernel2d(kx[None, None].repeat(in_channels, 1, 1, 1))
        self.conv_y = _Kernel2d(ky[None, None].repeat(in_channels, 1, 1, 1))
        self.conv_lum = _Kernel2d(kl[None, None].repeat(in_channels, 1, 1, 1))
        self._root = None

    def heatmaps(self, imgs: torch.Tensor, clc: float = 0.3) -> torch.Tensor:
        if clc != 0.3:
            raise NotImplementedError("clc != 0.3")
        eng = self._root[0]._engine()
        with torch.cuda.device(eng.dev):
            return eng.jnd_full(N.f32c(imgs.to(eng.dev))).to(imgs.device)


def get_dummy_augmenter() -> nn.Module:
    """augmentation/augmenter.py:48-57 ``get_dummy_augmenter()``: an Augmenter whose only op is Identity.  The reference builds it
    with masks={'kind': None}, i.e. its OpenCV-drawn MixedMaskEmbedder; here the mask embedder is the full mask of the training
    config (configs/all_augs.yaml:2-3 `kind: none`) -- assign ``augmenter.mask_embedder`` to plug any other callable."""
    from .augmentation import Augmenter
    return Augmenter(augs={"identity": 1}, augs_params={}, masks={"kind": "none"})


def _msgs_i32(msgs: torch.Tensor, dev) -> torch.Tensor:
    m = msgs.to(dev)
    if m.is_floating_point():
        m = m.long()            # msg_processor.py:92 `(indices + msg).long()` truncation
    return m.to(torch.int32).contiguous()


_EXTRACTOR_FIELDS = ("depths", "dims", "stem_stride", "extractor", "vit_dim", "vit_depth", "vit_heads", "vit_patch", "vit_window", "vit_global",
                     "vit_out", "vit_mlp_ratio", "vit_rel_pos", "head_stages", "head_pixelwise", "head_sigmoid")


def merge_cfg(embedder: "Embedder", detector: "Extractor", **own) -> ModelCfg:
    """One ModelCfg for the engine out of the halves `build_embedder` / `build_extractor` produced (videoseal_amd/builders.py, train.py:262-281)
    + the numbers the Wam / Videoseal constructor was given.  Models built from a card already share one cfg."""
    import dataclasses
    e, d = embedder.cfg, detector.cfg
    if e is d:
        return e
    if e.nbits != d.nbits:
        raise ValueError(f"embedder carries {e.nbits} bits, extractor {d.nbits}")
    return dataclasses.replace(e, **{f: getattr(d, f) for f in _EXTRACTOR_FIELDS}, **own)


class Wam(nn.Module):
    """Image path (models/wam.py:18-234)."""

    def __init__(self, embedder: Embedder, detector: Extractor, augmenter: nn.Module, attenuation: Optional[JND] = None,
                 scaling_w: float = 1.0, scaling_i: float = 1.0, clamp: bool = True, img_size: int = 256,
                 blending_method: str = "additive") -> None:
        super().__init__()
        if embedder.cfg is not detector.cfg:      # halves from build_embedder / build_extractor (train.py:262-305)
            jnd = (attenuation.in_channels, attenuation.out_channels) if attenuation is not None else (0, 0)
            embedder.cfg = detector.cfg = merge_cfg(embedder, detector, img_size=int(img_size), scaling_w=float(scaling_w), scaling_i=float(scaling_i),
                                                    blending_method=str(blending_method), jnd_in=jnd[0], jnd_out=jnd[1])
        self.embedder, self.detector, self.augmenter = embedder, detector, augmenter
        self.img_size = img_size
        self.rgb2yuv = RGB2YUV()
        self.blender = Blender(scaling_i, scaling_w, blending_method)
        self.attenuation = attenuation
        self.clamp = clamp
        self._eng: Optional[HipEngine] = None
        self._wkeys: Dict[str, tuple] = {}
        self._wgroups: Optional[Dict[str, list]] = None
        self._msg_cache: Optional[tuple] = None
        self._bn_sync = None          # set by videoseal_amd.dist.convert_sync_batchnorm: the BatchNorm exchange of distributed training
        self._emb_bwd = self._det_bwd = None      # training.EmbedderBackward / DetectorStep of the differentiable forward (built on first use)
        self._train_gen: Dict[str, int] = {}      # generation of the operands the HIP backward reads from the engine's workspace
        self._warned_no_backward = False
        # hipGraph replay of the per-chunk launch sequences (fixed chunk shapes, e.g. streaming callers): the ~300 kernel
        # launches of an embed / detect chunk are captured once per (shape, flags) and replayed with one launch
        self.use_graphs = SW.flag("VIDEOSEAL_GRAPHS", False)
        self._graphs: Dict[tuple, dict] = {}
        holder = [self]
        embedder._root = detector._root = holder
        if attenuation is not None:
            attenuation._root = holder

    def __setattr__(self, name, value):
        if name == "attenuation" and isinstance(value, JND):       # evals swap the attenuation module (evals/full.py:317-336)
            value._root = [self]
        if name in ("attenuation", "embedder", "detector", "rgb2yuv") and "_wgroups" in self.__dict__:
            self.__dict__["_wgroups"] = None
        super().__setattr__(name, value)

    # ---- plumbing
    @property
    def device(self):
        return next(self.parameters()).device

    def get_random_msg(self, bsz: int = 1, nb_repetitions=1) -> torch.Tensor:
        return self.embedder.get_random_msg(bsz, nb_repetitions)

    def _apply(self, fn, *a, **k):                 # .to() / .cuda() / .float(): tensors are replaced -> regroup
        self._wgroups = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._wgroups = None
        return super().load_state_dict(*a, **k)

    def _weight_groups(self) -> Dict[str, list]:
        """the tensors each packed weight group is built from (cached: walking the module tree costs 0.6 ms per call)"""
        if self._wgroups is None:
            emb_p = list(self.embedder.parameters())
            emb_b = list(self.embedder.buffers())
            det = list(self.detector.parameters()) + list(self.detector.buffers())
            misc = list(self.rgb2yuv.buffers()) + (list(self.attenuation.parameters()) if self.attenuation is not None else [])
            self._wgroups = {"Et": emb_p, "E": emb_p + emb_b, "X": det, "misc": misc}
        return self._wgroups

    def _engine(self) -> HipEngine:
        dev = self.device
        if dev.type != "cuda":
            raise N.NativeError("Videoseal (MI355X build) has no CPU execution path: move the model to a ROCm device "
                                "with .to('cuda') before embed()/detect().")
        if self._eng is None or self._eng.dev != dev:
            self._eng = HipEngine(self.embedder.cfg, self.state_dict, dev)
            self._wkeys = {}
            self._graphs.clear()
            self._emb_bwd = self._det_bwd = None
            self._train_gen = {}
        # packed weights go stale when any source tensor is replaced (data_ptr) or written in place (_version): every tensor of
        # the group is part of the key
        stale = []
        for name, ts in self._weight_groups().items():
            key = tuple((t.data_ptr(), t._version) for t in ts)
            if self._wkeys.get(name) != key:
                if name in self._wkeys:
                    stale.append(name)
                self._wkeys[name] = key
        if stale:
            self._eng.invalidate(*stale)
            self._graphs.clear()
        if self._bn_sync is None and self.embedder.training and SW.choice("VIDEOSEAL_SYNC_BN", "auto") == "auto":
            # train.py:438-440 converts every BatchNorm to SyncBatchNorm when it runs distributed; nn.SyncBatchNorm.convert_sync_batchnorm finds
            # no nn.BatchNorm2d children here (the U-Net is one HIP launch sequence), so the same switch is made when a process group with
            # more than one rank exists at the first train-mode forward (VIDEOSEAL_SYNC_BN=0 keeps per-rank statistics)
            import torch.distributed as td
            if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                from .dist import bn_all_reduce
                self._bn_sync = bn_all_reduce()
        self._eng.bn_sync = self._bn_sync
        self._eng.poll_nonfinite()
        return self._eng

    def repack(self) -> None:
        """Force re-packing of the weights (after edits that bypass tensor versioning, e.g. writes through raw pointers)."""
        self._wgroups = None
        if self._eng is not None:
            self._eng.invalidate()
        self._graphs.clear()

    def _msgs_dev(self, msgs: torch.Tensor, dev) -> torch.Tensor:
        """int32 device copy of the message; a CPU message that has not changed since the last call is not copied again
        (streaming callers pass the same [1, k] tensor for every chunk: one pageable H2D sync per call otherwise)."""
        if msgs.device == dev:
            return _msgs_i32(msgs, dev)
        c = self._msg_cache
        if c is not None and c[0] is msgs and c[1] == msgs._version and c[2].device == dev:
            return c[2]
        mi = _msgs_i32(msgs, dev)
        self._msg_cache = (msgs, msgs._version, mi)
        return mi

    def _graphed(self, key: tuple, ins: Dict[str, torch.Tensor], run, rekey=None):
        """Replay `run(static_inputs) -> dict of output tensors` from a hipGraph captured once per key.
        The first call runs eagerly twice (workspace allocation + tile autotune), then captures.  `rekey()` recomputes the key after the
        eager passes: the first of them verifies new weights and may switch the network (or single layers) to 3 x bf16; the graph records
        the kernels of the arithmetic in force at capture, so it is filed under the key a later call will compute (a stale key would
        capture a second graph on the next call)."""
        ent = self._graphs.get(key)
        if ent is None:
            static_in = {k: v.clone() for k, v in ins.items()}
            run(static_in)
            run(static_in)
            torch.cuda.synchronize()
            if rekey is not None:
                key = rekey()
                ent = self._graphs.get(key)
        if ent is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = run(static_in)
            ent = {"g": g, "in": static_in, "out": outs}
            self._graphs[key] = ent
        for k, v in ins.items():
            ent["in"][k].copy_(v)
        ent["g"].replay()
        return ent["out"]

    @property
    def pixelwise(self) -> bool:
        """the detector predicts [F, 1+nbits, S, S] maps (pixel_decoder.pixelwise) instead of one row of logits per frame"""
        return bool(getattr(self.detector.cfg, "head_pixelwise", False))

    def _empty_preds_shape(self) -> tuple:
        """shape of `preds` for a clip without frames: the maps of a pixel-wise head are the latent grid times the product of its factors"""
        c = self.detector.cfg
        k = self.embedder.cfg.nbits + 1
        if not self.pixelwise:
            return (0, k)
        S = int(self.img_size)
        side = S // c.vit_patch if c.extractor == "sam" else ((S - 4) // c.stem_stride + 1) // 8
        for f in c.head_stages:
            side *= int(f)
        return (0, k, side, side)

    def _per_frame_rows_only(self, what: str) -> None:
        if self.pixelwise:
            raise NotImplementedError(f"{what} passes [F, 1+nbits] rows of logits: a pixel-wise detector predicts [F, 1+nbits, S, S] maps "
                                      f"(use detect / extract_message)")

    def _detect_frames(self, eng: HipEngine, fr: torch.Tensor, S, antialias: bool) -> torch.Tensor:
        def run(si):
            rgb, _ = eng.resize_pre(si["fr"], S, antialias, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
            return {"preds": eng.extractor_forward(rgb)}
        if self.use_graphs and not torch.cuda.is_current_stream_capturing():
            def key():           # the arithmetic is part of the key: network-wide split AND the layers the calibration pinned to the exact split
                return ("det", fr.dtype, tuple(fr.shape), getattr(fr, "graph_key", None), tuple(S), antialias, id(eng), eng.arith_net["X"], tuple(sorted(eng.layer_arith.items())))
            out = self._graphed(key(), {"fr": fr}, run, rekey=key)["preds"].clone()
            eng.note_guard()           # the captured vs_check_finite has run: deliver its flag like an eager steady-state pass does
            return out
        p = run({"fr": fr})["preds"]
        return p if eng.preds_owned else p.clone()      # (the maps of a pixel-wise head are already the caller's: no second 0.8 GB pass)

    # ---- core of embed: one chunk of frames on the device
    def _embed_frames(self, eng: HipEngine, fr: torch.Tensor, msgs_i32: torch.Tensor, out: torch.Tensor, *, step: int,
                      video_mode: int, antialias: bool, lowres: bool, preds_w: Optional[torch.Tensor] = None,
                      fwd_order: bool = False, tail_span: int = 0) -> None:
        bn_train = self.embedder.training
        if self.use_graphs and not bn_train and not torch.cuda.is_current_stream_capturing():
            key = ("emb", fr.dtype, tuple(fr.shape), getattr(fr, "graph_key", None), tuple(msgs_i32.shape), step, video_mode, antialias, lowres, preds_w is not None, self.img_size,
                   self.clamp, float(self.blender.scaling_i), float(self.blender.scaling_w), self.attenuation is not None, fwd_order, tail_span, id(eng), eng.arith_net["E"])
            ent = self._graphs.get(key)
            if ent is None:
                sin = {"fr": fr.clone(), "msgs": msgs_i32.clone()}
                sout = _empty_like(sin["fr"])
                spw = torch.empty_like(preds_w) if preds_w is not None else None
                for _ in range(2):
                    self._embed_frames_eager(eng, sin["fr"], sin["msgs"], sout, step=step, video_mode=video_mode, antialias=antialias,
                                             lowres=lowres, preds_w=spw, fwd_order=fwd_order, tail_span=tail_span)
                torch.cuda.synchronize()
                if eng.arith_net["E"] != key[-1]:      # the verification pass switched the embedder to 3 x bf16: capture under the new key
                    return self._embed_frames(eng, fr, msgs_i32, out, step=step, video_mode=video_mode, antialias=antialias, lowres=lowres,
                                              preds_w=preds_w, fwd_order=fwd_order, tail_span=tail_span)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._embed_frames_eager(eng, sin["fr"], sin["msgs"], sout, step=step, video_mode=video_mode, antialias=antialias,
                                             lowres=lowres, preds_w=spw, fwd_order=fwd_order, tail_span=tail_span)
                ent = {"g": g, "in": sin, "out": sout, "pw": spw}
                self._graphs[key] = ent
            ent["in"]["fr"].copy_(fr)
            ent["in"]["msgs"].copy_(msgs_i32)
            ent["g"].replay()
            eng.note_guard()
            out.copy_(ent["out"])
            if preds_w is not None:
                preds_w.copy_(ent["pw"])
            return
        self._embed_frames_eager(eng, fr, msgs_i32, out, step=step, video_mode=video_mode, antialias=antialias, lowres=lowres,
                                 preds_w=preds_w, fwd_order=fwd_order, tail_span=tail_span)

    def _embed_front(self, eng: HipEngine, fr: torch.Tensor, msgs_i32: torch.Tensor, *, step: int, antialias: bool, lowres: bool):
        """everything before the tail: resize -> key frames -> U-Net -> (delta [keys,Cd,S,S], low-resolution heat-map or None), both in the
        engine's workspace (overwritten by the next call)"""
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        rgb, key = eng.resize_pre(fr, S, antialias, want_rgb=(att and lowres), want_key=True, key_step=step)
        delta = eng.embedder_forward(key, msgs_i32, bn_train=self.embedder.training)
        return delta, (eng.jnd_lowres(rgb) if (att and lowres) else None)

    def _embed_frames_eager(self, eng: HipEngine, fr: torch.Tensor, msgs_i32: torch.Tensor, out: torch.Tensor, *, step: int,
                            video_mode: int, antialias: bool, lowres: bool, preds_w: Optional[torch.Tensor] = None,
                            fwd_order: bool = False, tail_span: int = 0, on_tail=None, tail_batch: int = 0) -> None:
        """tail_span > 0 (a multiple of `step`): `fr` is a GROUP of consecutive caller chunks of tail_span frames each.  The key frames of the
        whole group go through the U-Net as one batch (the matrix kernels want >= 32 key frames to fill 256 CUs), the watermark is then
        expanded chunk by chunk exactly as the per-chunk calls would do it (videoseal.py:303-344: the last key frame of a chunk has no
        successor in 'interpolate' mode), so the group equals the sequence of per-chunk calls up to the summation order of the dense layers."""
        att = self.attenuation is not None
        delta, hmap = self._embed_front(eng, fr, msgs_i32, step=step, antialias=antialias, lowres=lowres)
        S = (self.img_size, self.img_size)
        kw = dict(step=step, video_mode=video_mode, attenuate=(2 if (att and fwd_order and not lowres) else int(att)), clamp=self.clamp,
                  antialias=antialias, scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w)
        F_ = fr.shape[0]
        # on_tail(a, b) (streaming.py): called on this stream's timeline every time another `tail_batch` watermarked frames [a, b) have been
        # issued, so that the consumer (the extractor on a second stream) starts on the first frames of a group while the rest is still being
        # blended.  The tail is a per-frame operation given (delta, hmap): cutting it at chunk boundaries does not change a value
        cut = tail_batch if (on_tail is not None and tail_batch > 0) else 0
        if tail_span > 0 and tail_span % step:
            raise ValueError("tail_span must be a multiple of the key-frame step")
        if cut and cut % max(tail_span, step):
            raise ValueError(f"tail_batch ({tail_batch}) must be a multiple of the chunk ({tail_span}) and of the key-frame step ({step})")
        per_chunk = not (tail_span <= 0 or tail_span >= F_ or video_mode == N.VIDEO_MODES["repeat"])
        # 'repeat' looks at one key frame per output frame: one launch over the group is the per-chunk launches
        span = tail_span if per_chunk else (cut if cut else F_)
        hw = S[0] * S[1]
        done = 0
        for a in range(0, F_, span):
            b = min(F_, a + span)
            if a == 0 and b == F_:
                eng.embed_tail(fr, out, delta, hmap_low=hmap, preds_w=preds_w, **kw)
            else:
                eng.embed_tail(fr[a:b], out[a:b], delta[a // step:(b + step - 1) // step], hmap_low=(hmap[a * hw:b * hw] if hmap is not None else None),
                               preds_w=(preds_w[a:b] if preds_w is not None else None), **kw)
            if cut and (b - done >= cut or b == F_):
                on_tail(done, b)
                done = b
        if on_tail is not None and not cut:
            on_tail(0, F_)

    def _run_chunks(self, eng: HipEngine, imgs: torch.Tensor, span: int, fn, *, want_out: bool = True, extra=None):
        """Drive `fn(chunk_on_device, out_chunk_on_device, a, b)` over [a, b) frame ranges of `span` frames.  Frames that are not
        on the model's device move one chunk at a time (videoseal.py:286-297 keeps the full clip where the caller put it);
        the result comes back on imgs.device."""
        on_dev = imgs.device == eng.dev
        if on_dev:
            src = imgs if _raw_frames(imgs) else N.f32c(imgs)
            out = _empty_like(src) if want_out else None
        else:
            src = imgs
            if not want_out:
                out = None
            elif torch.is_tensor(imgs):
                out = _result_buffer(imgs.shape, imgs.dtype if imgs.dtype == torch.uint8 else torch.float32, imgs.device)
            else:
                out = imgs.empty_like()
        for attempt in range(2):
            for a in range(0, imgs.shape[0], span):
                b = min(imgs.shape[0], a + span)
                if on_dev:
                    fn(src[a:b], out[a:b] if want_out else None, a, b)
                else:
                    ch = src[a:b].to(eng.dev)
                    ch = ch.contiguous() if _raw_frames(ch) else N.f32c(ch)
                    oc = _empty_like(ch) if want_out else None
                    fn(ch, oc, a, b)
                    if want_out:
                        out[a:b].copy_(oc, non_blocking=True)
            if on_dev:
                break
            # the copies into (pinned) host memory are asynchronous: the results are valid from here on.  This entry point synchronises
            # anyway, so the range guard of every pass of the call is read here: a data-dependent overflow repeats the call on the exact
            # split instead of handing non-finite frames to the caller
            torch.cuda.current_stream(eng.dev).synchronize()
            if attempt or not eng.guard_tripped_after_sync():
                break
            if extra is not None:
                extra()               # (the caller's per-call accumulators, e.g. the list of logits, start over)
        return out

    @torch.no_grad()
    def embed(self, imgs: torch.Tensor, msgs: torch.Tensor = None, interpolation: dict = None,
              lowres_attenuation: bool = False) -> dict:
        """wam.py:134-204."""
        if msgs is None:
            msgs = self.get_random_msg(imgs.shape[0])
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        B = imgs.shape[0]
        cd = self.embedder.cfg.out_ch
        if B == 0:
            return {"msgs": msgs, "preds_w": imgs.new_zeros((0, cd) + tuple(imgs.shape[-2:])), "imgs_w": imgs.clone()}
        if msgs.shape[0] != B:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {B} images")
        with torch.cuda.device(eng.dev):
            mi = self._msgs_dev(msgs, eng.dev)
            on_dev = imgs.device == eng.dev
            preds_w = _result_buffer((B, cd, imgs.shape[-2], imgs.shape[-1]), torch.float32, imgs.device)

            def one(fr, oc, a, b):
                pw = preds_w[a:b] if on_dev else torch.empty(b - a, cd, fr.shape[-2], fr.shape[-1], device=eng.dev, dtype=torch.float32)
                self._embed_frames(eng, fr, mi[a:b], oc, step=1, video_mode=0, antialias=aa, lowres=lowres_attenuation, preds_w=pw)
                if not on_dev:
                    preds_w[a:b].copy_(pw, non_blocking=True)       # _run_chunks synchronises before it returns
            out = self._run_chunks(eng, imgs, max(1, int(getattr(self, "chunk_size", 32))), one)
        return {"msgs": msgs, "preds_w": preds_w, "imgs_w": out}

    @torch.no_grad()
    def detect(self, imgs: torch.Tensor, interpolation: dict = None) -> dict:
        """wam.py:206-234."""
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        if imgs.shape[0] == 0:
            return {"preds": imgs.new_zeros(self._empty_preds_shape())}
        with torch.cuda.device(eng.dev):
            x = N.f32c(imgs.to(eng.dev))
            return {"preds": self._detect_frames(eng, x, (self.img_size, self.img_size), aa).to(imgs.device)}

    # ---- lists of images of different sizes: one network pass per chunk of the list, the two full-resolution passes on the list itself
    @staticmethod
    def _image_list(imgs, what: str):
        """-> (the images as [3, H, W] float or [H, W, 3] uint8 views, uint8?)"""
        imgs = list(imgs)
        if not all(torch.is_tensor(t) for t in imgs):
            raise TypeError(f"{what} wants a sequence of tensors")
        if len({t.dtype for t in imgs}) > 1:
            raise ValueError(f"{what}: the images of one call are all fp32 [3, H, W] or all uint8 [H, W, 3], got {sorted({str(t.dtype) for t in imgs})}")
        u8 = bool(imgs) and imgs[0].dtype == torch.uint8
        if imgs and not (u8 or imgs[0].is_floating_point()):
            raise ValueError(f"{what}: images are fp32 [3, H, W] or uint8 [H, W, 3], got {imgs[0].dtype}")
        views = []
        for t in imgs:
            v = t[0] if (not u8 and t.dim() == 4 and t.shape[0] == 1) else t
            if v.dim() != 3 or v.shape[-1 if u8 else 0] != 3 or 0 in v.shape:
                raise ValueError(f"{what}: " + ("uint8 images are RGB24 [H, W, 3]" if u8 else "fp32 images are [3, H, W] or [1, 3, H, W]") +
                                 f", got {tuple(t.shape)}")
            views.append(v)
        return views, u8

    def _image_chunks(self, eng: HipEngine, views, u8: bool, fn, restart=None) -> None:
        """Drive `fn(chunk_on_device, a, b)` over the list in chunks of chunk_size images.  Images that are not on the model's device move one
        chunk at a time; such a call synchronises before it returns, so the range guard of its passes is read here and a data-dependent
        overflow repeats the call on the exact split (as _run_chunks does for a clip)."""
        ck = max(1, int(getattr(self, "chunk_size", 32)))
        on_dev = all(v.device == eng.dev for v in views)
        for attempt in range(2):
            for a in range(0, len(views), ck):
                b = min(len(views), a + ck)
                ch = [v if v.device == eng.dev else v.to(eng.dev) for v in views[a:b]]
                fn([t.contiguous() if u8 else N.f32c(t) for t in ch], a, b)
            if on_dev:
                break
            torch.cuda.current_stream(eng.dev).synchronize()
            if attempt or not eng.guard_tripped_after_sync():
                break
            if restart is not None:
                restart()

    @torch.no_grad()
    def embed_images(self, imgs, msgs: torch.Tensor = None, interpolation: dict = None, lowres_attenuation: bool = False) -> dict:
        """`embed(img[None], msg[None], is_video=False)` (wam.py:134-204) for every image of a list whose images differ in size, with the
        network running once per chunk_size images instead of once per image.  imgs: n tensors, all fp32 [3, H_i, W_i] (or [1, 3, H_i, W_i])
        or all uint8 RGB24 [H_i, W_i, 3] (needs clamp=True); msgs [n, k] or None (random).  -> {'imgs_w': list, 'preds_w': list of fp32
        [Cd, H_i, W_i], 'msgs'}: every result has the shape of its input on its input's device; for device-resident images they are views
        of one allocation per call.  Per chunk: one resize launch group over the chunk (vs_resize_pre_images), one embedder pass, one
        low-resolution heat-map when asked, one tail over the chunk (vs_embed_tail_images) -- the pieces of `embed`, so image i equals
        what the per-image pieces give up to the batch size of the network pass.  Always eager (no hipGraph route)."""
        imgs = list(imgs)
        _refuse_half(imgs, "embed_images", "lists of images are fp32 or uint8")
        views, u8 = self._image_list(imgs, "embed_images")
        n = len(views)
        if u8 and not self.clamp:
            raise NotImplementedError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg(n)
        elif msgs.shape[0] != n:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {n} images")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        cd = self.embedder.cfg.out_ch
        if n == 0:
            return {"msgs": msgs, "preds_w": [], "imgs_w": []}
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        lowres = bool(lowres_attenuation)
        odt = torch.uint8 if u8 else torch.float32
        hw = [(v.shape[0], v.shape[1]) if u8 else (v.shape[1], v.shape[2]) for v in views]
        lead = [(1,) if (not u8 and t.dim() == 4) else () for t in imgs]
        on_dev = all(v.device == eng.dev for v in views)
        outs, pws = [None] * n, [None] * n

        def carve(a, b):
            """results of images [a, b) as views of one device allocation each"""
            o = torch.empty(sum(3 * h * w for h, w in hw[a:b]), dtype=odt, device=eng.dev)
            p = torch.empty(sum(cd * h * w for h, w in hw[a:b]), dtype=torch.float32, device=eng.dev)
            oo, pp, io, ip = [], [], 0, 0
            for h, w in hw[a:b]:
                oo.append(o[io:io + 3 * h * w].view((h, w, 3) if u8 else (3, h, w)))
                pp.append(p[ip:ip + cd * h * w].view(cd, h, w))
                io, ip = io + 3 * h * w, ip + cd * h * w
            return oo, pp

        with torch.cuda.device(eng.dev):
            mi = self._msgs_dev(msgs, eng.dev)
            if on_dev:
                outs, pws = carve(0, n)

            def one(ch, a, b):
                oo, pp = (outs[a:b], pws[a:b]) if on_dev else carve(a, b)
                rgb, key = eng.resize_pre_images(ch, S, aa, want_rgb=(att and lowres), want_key=True)
                delta = eng.embedder_forward(key, mi[a:b], bn_train=self.embedder.training)
                hmap = eng.jnd_lowres(rgb) if (att and lowres) else None
                eng.embed_tail_images(ch, oo, delta, hmap_low=hmap, attenuate=int(att), clamp=self.clamp, antialias=aa,
                                      scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w, preds_w=pp)
                if not on_dev:        # back to where each image came from (_image_chunks synchronises before it returns)
                    for i in range(a, b):
                        if outs[i] is None:
                            outs[i] = _result_buffer(oo[i - a].shape, odt, views[i].device)
                            pws[i] = _result_buffer(pp[i - a].shape, torch.float32, views[i].device)
                        outs[i].copy_(oo[i - a], non_blocking=True)
                        pws[i].copy_(pp[i - a], non_blocking=True)
            self._image_chunks(eng, views, u8, one)
        return {"msgs": msgs, "preds_w": [p.view(ld + tuple(p.shape)) for p, ld in zip(pws, lead)],
                "imgs_w": [o.view(ld + tuple(o.shape)) for o, ld in zip(outs, lead)]}

    @torch.no_grad()
    def embed_images_psnr(self, imgs, target_psnr: float, msgs: torch.Tensor = None, max_scaling_w: Optional[float] = None,
                          interpolation: dict = None, lowres_attenuation: bool = False) -> dict:
        """`embed_images` with `blender.scaling_w` replaced, image by image, by the strength that puts that image at `target_psnr` dB against
        its original: with d the perturbation of image i at scaling_w = 1 (its `preds_w`), E_i = (3 / Cd) * sum d^2 in float64 and
            s_i = 10^(-target_psnr / 20) * sqrt(3 H_i W_i / E_i),   0 where E_i == 0,   at most max_scaling_w when one is given
        (the formula of `embed_psnr`).  Image i is then image i of `embed_images` at blender.scaling_w = s_i, bit for bit.
        Returns what `embed_images` returns plus 'scaling_w' (fp32 [n], the strengths applied) and 'energy' (float64 [n]), both on the first
        image's device.  Per chunk: the resize, the embedder pass and the heat-map of `embed_images`, then an energy pass over the chunk
        (vs_embed_tail_images_energy: the tail's own d, reduced per image, no image stored), the strengths (vs_psnr_scale_items) and the tail
        with a strength per image (vs_embed_tail_images_scaled), following each other on the stream without a host synchronisation.  The
        clamp and uint8 quantisation are not corrected for, as in `embed_psnr`.  Always eager."""
        check_psnr_args(target_psnr, "frame", max_scaling_w)
        imgs = list(imgs)
        _refuse_half(imgs, "embed_images_psnr", "lists of images are fp32 or uint8")
        views, u8 = self._image_list(imgs, "embed_images_psnr")
        n = len(views)
        if u8 and not self.clamp:
            raise ValueError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg(n)
        elif msgs.shape[0] != n:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {n} images")
        aa = _antialias_flag(interpolation)
        eng = self._engine()
        cd = self.embedder.cfg.out_ch
        if n == 0:
            return {"msgs": msgs, "preds_w": [], "imgs_w": [], "scaling_w": torch.zeros(0, dtype=torch.float32),
                    "energy": torch.zeros(0, dtype=torch.float64)}
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        lowres = bool(lowres_attenuation)
        odt = torch.uint8 if u8 else torch.float32
        hw = [(v.shape[0], v.shape[1]) if u8 else (v.shape[1], v.shape[2]) for v in views]
        lead = [(1,) if (not u8 and t.dim() == 4) else () for t in imgs]
        on_dev = all(v.device == eng.dev for v in views)
        cap = float(max_scaling_w) if max_scaling_w is not None else None
        outs, pws = [None] * n, [None] * n

        def carve(a, b):
            """results of images [a, b) as views of one device allocation each"""
            o = torch.empty(sum(3 * h * w for h, w in hw[a:b]), dtype=odt, device=eng.dev)
            p = torch.empty(sum(cd * h * w for h, w in hw[a:b]), dtype=torch.float32, device=eng.dev)
            oo, pp, io, ip = [], [], 0, 0
            for h, w in hw[a:b]:
                oo.append(o[io:io + 3 * h * w].view((h, w, 3) if u8 else (3, h, w)))
                pp.append(p[ip:ip + cd * h * w].view(cd, h, w))
                io, ip = io + 3 * h * w, ip + cd * h * w
            return oo, pp

        with torch.cuda.device(eng.dev):
            mi = self._msgs_dev(msgs, eng.dev)
            energy = torch.empty(n, device=eng.dev, dtype=torch.float64)
            scale = torch.empty(n, device=eng.dev, dtype=torch.float32)
            elems = torch.tensor([3.0 * h * w for h, w in hw], dtype=torch.float64).to(eng.dev)
            if on_dev:
                outs, pws = carve(0, n)

            def one(ch, a, b):
                oo, pp = (outs[a:b], pws[a:b]) if on_dev else carve(a, b)
                rgb, key = eng.resize_pre_images(ch, S, aa, want_rgb=(att and lowres), want_key=True)
                delta = eng.embedder_forward(key, mi[a:b], bn_train=self.embedder.training)
                hmap = eng.jnd_lowres(rgb) if (att and lowres) else None
                eng.tail_energy_images(ch, delta, hmap_low=hmap, attenuate=int(att), antialias=aa, energy=energy[a:b])
                eng.psnr_scale_items(energy[a:b], elems[a:b], target_psnr, max_scale=cap, scale=scale[a:b])
                eng.embed_tail_images(ch, oo, delta, hmap_low=hmap, attenuate=int(att), clamp=self.clamp, antialias=aa,
                                      scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w, preds_w=pp, frame_scale=scale[a:b])
                if not on_dev:        # back to where each image came from (_image_chunks synchronises before it returns)
                    for i in range(a, b):
                        if outs[i] is None:
                            outs[i] = _result_buffer(oo[i - a].shape, odt, views[i].device)
                            pws[i] = _result_buffer(pp[i - a].shape, torch.float32, views[i].device)
                        outs[i].copy_(oo[i - a], non_blocking=True)
                        pws[i].copy_(pp[i - a], non_blocking=True)
            self._image_chunks(eng, views, u8, one)
        return {"msgs": msgs, "preds_w": [p.view(ld + tuple(p.shape)) for p, ld in zip(pws, lead)],
                "imgs_w": [o.view(ld + tuple(o.shape)) for o, ld in zip(outs, lead)],
                "scaling_w": scale.to(views[0].device), "energy": energy.to(views[0].device)}

    @torch.no_grad()
    def detect_images(self, imgs, interpolation: dict = None) -> dict:
        """`detect` (wam.py:206-234) on a list of images of different sizes (see embed_images): one resize launch group and one extractor pass
        per chunk_size images -> {'preds'}: what detect returns for n stacked frames of the processing size, on the first image's device."""
        views, u8 = self._image_list(imgs, "detect_images")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        if not views:
            return {"preds": torch.zeros(self._empty_preds_shape())}
        S = (self.img_size, self.img_size)
        preds = []

        def one(ch, a, b):
            rgb, _ = eng.resize_pre_images(ch, S, aa, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
            p = eng.extractor_forward(rgb)
            preds.append(p if eng.preds_owned else p.clone())
        with torch.cuda.device(eng.dev):
            self._image_chunks(eng, views, u8, one, restart=preds.clear)
            return {"preds": torch.cat(preds, dim=0).to(views[0].device)}

    def _augment_detect(self, eng: HipEngine, imgs_w: torch.Tensor, imgs: torch.Tensor, masks, is_video: bool, aa: bool):
        """wam.py:115-125 / videoseal.py:231-243: augment -> resize to the processing size -> detector (device tensors)."""
        from . import augmentation as A
        imgs_aug, masks, selected = self.augmenter(imgs_w, imgs, masks.to(eng.dev) if torch.is_tensor(masks) else masks,
                                                   is_video=is_video, do_resize=False)
        S = (self.img_size, self.img_size)
        if tuple(imgs_aug.shape[-2:]) != S:
            imgs_aug = A.resize(imgs_aug, S, aa)
        rgb, _ = eng.resize_pre(N.f32c(imgs_aug), S, False, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
        return imgs_aug, masks, selected, eng.extractor_forward(rgb).clone()

    def _trainable(self) -> Tuple[bool, bool]:
        """(embedder, detector) have parameters that want gradients in the current autograd mode"""
        if not torch.is_grad_enabled():
            return False, False
        emb = any(p.requires_grad for p in self.embedder.parameters())
        det = any(p.requires_grad for p in self.detector.parameters())
        return emb, det

    def _forward_graph(self, x: torch.Tensor, masks, mi: torch.Tensor, *, step: int, video_mode: int, aa: bool, lowres: bool, is_video: bool,
                       emb_train: bool):
        """the differentiable forward (wam.py:86-125 / videoseal.py:181-243): EmbedTrainFn -> augmenter nodes -> ResizeFn -> DetectTrainFn"""
        from . import augmentation as A
        from . import autograd as AG
        eng = self._engine()
        if emb_train:
            named = [(k, p) for k, p in AG._named_unique(self.embedder, "embedder.")]
            opts = dict(step=step, video_mode=video_mode, antialias=aa, lowres=lowres)
            imgs_w, preds_w = AG.EmbedTrainFn.apply(self, x, mi, opts, [k for k, _ in named], *[p for _, p in named])
        else:
            with torch.no_grad():
                imgs_w = torch.empty_like(x)
                preds_w = torch.empty(x.shape[0], self.embedder.cfg.out_ch, x.shape[-2], x.shape[-1], device=eng.dev, dtype=torch.float32)
                self._embed_frames(eng, x, mi, imgs_w, step=step, video_mode=video_mode, antialias=aa, lowres=lowres, preds_w=preds_w, fwd_order=True)
        imgs_aug, masks, selected = self.augmenter(imgs_w, x, masks.to(eng.dev) if torch.is_tensor(masks) else masks, is_video=is_video,
                                                   do_resize=False)
        S = (self.img_size, self.img_size)
        if tuple(imgs_aug.shape[-2:]) != S:
            imgs_aug = A.resize(imgs_aug, S, aa)
        named = AG._named_unique(self.detector, "detector.")
        if imgs_aug.requires_grad or any(p.requires_grad for _, p in named):
            preds = AG.DetectTrainFn.apply(self, imgs_aug, [k for k, _ in named], *[p for _, p in named])
        else:
            with torch.no_grad():
                rgb, _ = eng.resize_pre(N.f32c(imgs_aug), S, False, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
                preds = eng.extractor_forward(rgb).clone()
        return imgs_w, preds_w, imgs_aug, masks, selected, preds

    def forward(self, imgs: torch.Tensor, masks: torch.Tensor, msgs: torch.Tensor = None, interpolation: dict = None) -> dict:
        """wam.py:68-132: embed (blend, then full-resolution attenuation(imgs, imgs_w), clamp) -> augmenter -> resize to img_size ->
        detector.  `preds_w` is the UN-attenuated resized delta and `imgs_aug` the resized augmented batch, like the reference.
        BatchNorm follows ``self.embedder.training``.  With autograd enabled and trainable parameters the outputs carry a graph whose
        backward runs on the HIP kernels (autograd.py); otherwise values only."""
        emb_t, det_t = self._trainable()
        if not (emb_t or det_t):
            with torch.no_grad():
                return self._forward_values(imgs, masks, msgs, interpolation)
        if msgs is None:
            msgs = self.get_random_msg(imgs.shape[0]).to(imgs.device)
        eng = self._engine()
        aa = _antialias_flag(_DEFAULT_INTERP if interpolation is None else interpolation)
        back = imgs.device
        with torch.cuda.device(eng.dev):
            x = N.f32c(imgs.detach().to(eng.dev))
            imgs_w, preds_w, imgs_aug, masks, selected, preds = self._forward_graph(
                x, masks, self._msgs_dev(msgs, eng.dev), step=1, video_mode=0, aa=aa, lowres=False, is_video=False, emb_train=emb_t)
        to = (lambda t: t.to(back) if torch.is_tensor(t) else t)     # noqa: E731
        return {"msgs": msgs, "masks": to(masks), "preds_w": to(preds_w), "imgs_w": to(imgs_w), "imgs_aug": to(imgs_aug),
                "preds": to(preds), "selected_aug": selected}

    def _forward_values(self, imgs: torch.Tensor, masks: torch.Tensor, msgs: torch.Tensor = None, interpolation: dict = None) -> dict:
        if msgs is None:
            msgs = self.get_random_msg(imgs.shape[0]).to(imgs.device)
        eng = self._engine()
        aa = _antialias_flag(_DEFAULT_INTERP if interpolation is None else interpolation)
        back = imgs.device
        with torch.cuda.device(eng.dev):
            x = N.f32c(imgs.to(eng.dev))
            B = x.shape[0]
            out = torch.empty_like(x)
            preds_w = torch.empty(B, self.embedder.cfg.out_ch, x.shape[-2], x.shape[-1], device=eng.dev, dtype=torch.float32)
            self._embed_frames(eng, x, self._msgs_dev(msgs, eng.dev), out, step=1, video_mode=0, antialias=aa, lowres=False,
                               preds_w=preds_w, fwd_order=True)
            imgs_aug, masks, selected, preds = self._augment_detect(eng, out, x, masks, False, aa)
        to = (lambda t: _to_caller(t, back))     # noqa: E731
        return {"msgs": msgs, "masks": to(masks), "preds_w": to(preds_w), "imgs_w": to(out), "imgs_aug": to(imgs_aug),
                "preds": to(preds), "selected_aug": selected}


class Videoseal(Wam):
    """Video path (models/videoseal.py:15-428): key-frame stepping, chunking, frame aggregation."""

    def __init__(self, embedder, detector, augmenter, attenuation=None, scaling_w: float = 1.0, scaling_i: float = 1.0,
                 img_size: int = 256, clamp: bool = True, chunk_size: int = 8, step_size: int = 4,
                 blending_method: str = "additive", video_mode: str = "repeat", lowres_attenuation: bool = False) -> None:
        super().__init__(embedder, detector, augmenter, attenuation, scaling_w, scaling_i, clamp, img_size, blending_method)
        self.chunk_size, self.step_size = chunk_size, step_size
        if self.embedder.cfg.chunk_size != int(chunk_size) or self.embedder.cfg.step_size != int(step_size):
            import dataclasses            # (a fresh object: a card's cfg may be shared between models)
            self.embedder.cfg = self.detector.cfg = dataclasses.replace(self.embedder.cfg, chunk_size=int(chunk_size), step_size=int(step_size))
        self.video_mode = video_mode
        self.lowres_attenuation = lowres_attenuation

    def _embed_clip(self, imgs: torch.Tensor, msgs: torch.Tensor, interpolation, lowres_attenuation: bool) -> torch.Tensor:
        if self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        step, ck = int(self.step_size), int(self.chunk_size)
        with torch.cuda.device(eng.dev):
            mi = self._msgs_dev(msgs, eng.dev)
            vm = N.VIDEO_MODES[self.video_mode]
            return self._run_chunks(eng, imgs, ck * step,       # frames per chunk (videoseal.py:292-297)
                                    lambda fr, oc, a, b: self._embed_frames(eng, fr, mi, oc, step=step, video_mode=vm, antialias=aa,
                                                                            lowres=lowres_attenuation))

    @torch.no_grad()
    def embed_group(self, frames: torch.Tensor, msgs: torch.Tensor, chunk: int, interpolation: dict = None,
                    lowres_attenuation: bool = False, on_tail=None, tail_batch: int = 0) -> torch.Tensor:
        """`frames` (device-resident fp32 [F,3,H,W] or uint8 RGB24 [F,H,W,3]) = consecutive caller chunks of `chunk` frames (the last one may be
        short), `chunk` a multiple of step_size.  Returns what `torch.cat([embed(c, msgs, is_video=True)['imgs_w'] for c in chunks])` returns
        (embed_u8 for uint8), with the key frames of ALL chunks going through the U-Net as one batch: 16-frame streaming calls
        (inference_streaming.py:83-107) carry 4 key frames each, which leaves the matrix kernels at a third of the rate they reach with 32.
        The per-chunk semantics of videoseal.py:303-344 are kept by expanding the watermark chunk by chunk (`_embed_frames_eager`); values
        differ from the per-chunk calls only by the summation order of the dense layers (a K split is a function of the batch shape)."""
        if self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        assert msgs.shape[0] == 1, "Message should be unique"
        eng = self._engine()
        step = int(self.step_size)
        if chunk % step:
            raise ValueError(f"chunk ({chunk}) must be a multiple of step_size ({step}): the key frames of the group are every step-th frame")
        if chunk > int(self.chunk_size) * step:
            # embed() itself walks a call in chunk_size * step_size frames (videoseal.py:291-297) and the watermark expansion restarts there;
            # a caller chunk that spans several of them is not one expansion span
            raise ValueError(f"chunk ({chunk}) exceeds chunk_size * step_size = {int(self.chunk_size) * step}: embed() would split such a call "
                             f"internally; raise model.chunk_size or pass smaller chunks")
        if frames.device != eng.dev:
            raise ValueError("embed_group wants device-resident frames")
        u8 = frames.dtype == torch.uint8
        if u8 and not self.clamp:
            raise NotImplementedError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        aa = _antialias_flag(interpolation)
        with torch.cuda.device(eng.dev):
            src = frames.contiguous() if u8 else N.f32c(frames)
            out = torch.empty_like(src)
            if on_tail is not None and not self.use_graphs:
                # (streaming.py) `on_tail(first, imgs_w[first:last])` as soon as another `tail_batch` watermarked frames are issued
                self._embed_frames_eager(eng, src, self._msgs_dev(msgs, eng.dev), out, step=step, video_mode=N.VIDEO_MODES[self.video_mode],
                                         antialias=aa, lowres=lowres_attenuation, tail_span=int(chunk), tail_batch=int(tail_batch),
                                         on_tail=lambda a, b: on_tail(a, out[a:b]))
                return out
            self._embed_frames(eng, src, self._msgs_dev(msgs, eng.dev), out, step=step, video_mode=N.VIDEO_MODES[self.video_mode], antialias=aa,
                               lowres=lowres_attenuation, tail_span=int(chunk))
            if on_tail is not None:
                on_tail(0, out)
        return out

    @torch.no_grad()
    def embed(self, imgs: torch.Tensor, msgs: torch.Tensor = None, is_video: bool = True, interpolation: dict = None,
              lowres_attenuation: bool = False) -> dict:
        """videoseal.py:258-350."""
        if not is_video:
            return super().embed(imgs, msgs, interpolation, lowres_attenuation)
        if msgs is None:
            msgs = self.get_random_msg()
        else:
            assert msgs.shape[0] == 1, "Message should be unique"
        out = self._embed_clip(imgs, msgs, interpolation, lowres_attenuation)
        return {"imgs_w": out, "msgs": msgs[0:1].repeat(len(imgs), 1)}

    def _detect_clip(self, imgs: torch.Tensor, interpolation) -> torch.Tensor:
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        S = (self.img_size, self.img_size)
        preds = []
        with torch.cuda.device(eng.dev):
            self._run_chunks(eng, imgs, max(1, int(self.chunk_size)),
                             lambda fr, oc, a, b: preds.append(self._detect_frames(eng, fr, S, aa)), want_out=False, extra=preds.clear)
            return torch.cat(preds, dim=0).to(imgs.device)

    @torch.no_grad()
    def detect(self, imgs: torch.Tensor, is_video: bool = True, interpolation: dict = None) -> dict:
        """videoseal.py:352-388."""
        if not is_video:
            return super().detect(imgs) if interpolation is None else super().detect(imgs, interpolation)
        if imgs.shape[0] == 0:
            self._engine()
            return {"preds": imgs.new_zeros(self._empty_preds_shape())}
        return {"preds": self._detect_clip(imgs, interpolation)}

    # ---- uint8 RGB24 clips, the data format on either side of the path in inference_streaming.py
    @torch.no_grad()
    def embed_u8(self, clip: torch.Tensor, msgs: torch.Tensor = None, interpolation: dict = None,
                 lowres_attenuation: bool = True) -> dict:
        """inference_streaming.py:23-32 (`embed_video_clip`) in one pass: clip uint8 [F,H,W,3] (RGB24, as read from the ffmpeg
        pipe) -> {'imgs_w': uint8 [F,H,W,3], 'msgs'}.  Equals (embed(clip.float().permute(0,3,1,2)/255, is_video=True,
        lowres_attenuation=...)['imgs_w'] * 255).byte().permute(0,2,3,1) with the conversions fused into the resize and tail
        kernels (3 B/pixel instead of 12 B/pixel through HBM, no fp32 copy of the clip)."""
        if clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[-1] != 3:
            raise ValueError("embed_u8 wants a uint8 RGB24 clip [F, H, W, 3]")
        if not self.clamp:
            raise NotImplementedError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg()
        else:
            assert msgs.shape[0] == 1, "Message should be unique"
        out = self._embed_clip(clip.contiguous(), msgs, interpolation, lowres_attenuation)
        return {"imgs_w": out, "msgs": msgs[0:1].repeat(len(clip), 1)}

    # ---- region-wise watermarks: a label map ties message r - 1 to the pixels of label r (videoseal_amd/regions.py holds the definition)
    def _embed_regions_eager(self, eng: HipEngine, fr: torch.Tensor, lab: torch.Tensor, msgs_i32: torch.Tensor, out: torch.Tensor, R: int, *,
                             step: int, video_mode: int, antialias: bool, lowres: bool, preds_w: Optional[torch.Tensor]) -> None:
        """one chunk on the device: the resize runs once per frame, the key frames go through the U-Net R times in ONE batch (frame k * R + r
        = key frame k with message r; msgs_i32 [keys * R, k] in that order), the tail picks the plane set of every pixel's label"""
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        rgb, key = eng.resize_pre(fr, S, antialias, want_rgb=(att and lowres), want_key=True, key_step=step)
        delta = eng.embedder_forward(eng.repeat_keys(key, R), msgs_i32, bn_train=False)
        hmap = eng.jnd_lowres(rgb) if (att and lowres) else None
        eng.embed_tail_regions(fr, out, delta, lab, R, step=step, video_mode=video_mode, hmap_low=hmap, attenuate=int(att), clamp=self.clamp,
                               antialias=antialias, scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w, preds_w=preds_w)

    def _embed_regions_frames(self, eng: HipEngine, fr, lab, msgs_i32, out, R: int, *, step, video_mode, antialias, lowres, preds_w) -> None:
        kw = dict(step=step, video_mode=video_mode, antialias=antialias, lowres=lowres)
        if self.use_graphs and not torch.cuda.is_current_stream_capturing():
            def run(si):
                o = _empty_like(si["fr"])
                pw = torch.empty_like(preds_w) if preds_w is not None else None
                self._embed_regions_eager(eng, si["fr"], si["lab"], si["msgs"], o, R, preds_w=pw, **kw)
                return {"out": o, "pw": pw}

            def key():           # R is part of the key: the U-Net batch is keys * R frames
                return ("embr", R, fr.dtype, tuple(fr.shape), tuple(msgs_i32.shape), step, video_mode, antialias, lowres, preds_w is not None,
                        self.img_size, self.clamp, float(self.blender.scaling_i), float(self.blender.scaling_w), self.attenuation is not None,
                        id(eng), eng.arith_net["E"])
            res = self._graphed(key(), {"fr": fr, "lab": lab, "msgs": msgs_i32}, run, rekey=key)
            eng.note_guard()
            out.copy_(res["out"])
            if preds_w is not None:
                preds_w.copy_(res["pw"])
            return
        self._embed_regions_eager(eng, fr, lab, msgs_i32, out, R, preds_w=preds_w, **kw)

    @torch.no_grad()
    def embed_regions(self, imgs: torch.Tensor, labels: torch.Tensor, msgs: torch.Tensor, is_video: bool = True, interpolation: dict = None,
                      lowres_attenuation: bool = False) -> dict:
        """A message per region of the frame.  imgs fp32 [F,3,H,W] or uint8 RGB24 [F,H,W,3]; labels uint8 [F,H,W] (0 = background, r in 1..R =
        message r - 1, above R = background); msgs [R,k], or [F,R,k] with is_video=False (video mode keeps one message per region).
        A pixel of label r is the pixel of `embed(imgs, msgs[r - 1])`, a pixel of label 0 is the pixel of imgs bit for bit (regions.embed_regions).
        -> {'imgs_w', 'msgs' [F,R,k]} and, with is_video=False, 'preds_w' fp32 [F,Cd,H,W] (0 on background), as `embed` returns them.
        The key frames of a chunk pass the U-Net once per region in one batch: chunks hold min(chunk_size, 32 // R) key frames.  Frames that
        are not on the model's device move chunk by chunk, and their labels with them.  The embedder runs in eval mode.  The strength is
        blender.scaling_w for every region: `embed_psnr` takes no label map (its strength comes from the energy of ONE watermark over the frame)."""
        from . import regions as RG
        _refuse_half(imgs, "embed_regions", "half clips carry no label maps")
        F_, H, W, u8 = RG.check_frames(imgs, "embed_regions")
        RG.check_labels(labels, F_, H, W)
        R = RG.check_msgs(msgs, F_, is_video)
        if u8 and not self.clamp:
            raise NotImplementedError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if is_video and self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        cd = self.embedder.cfg.out_ch
        msgs_out = msgs if msgs.dim() == 3 else msgs[None].repeat(F_, 1, 1)
        if F_ == 0:
            res = {"imgs_w": imgs.clone(), "msgs": msgs_out}
            if not is_video:
                res["preds_w"] = torch.zeros((0, cd, H, W), dtype=torch.float32, device=imgs.device)
            return res
        step = int(self.step_size) if is_video else 1
        ck = max(1, min(int(getattr(self, "chunk_size", 32)), RG.UNET_FRAMES // R))
        vm = N.VIDEO_MODES[self.video_mode] if is_video else 0
        with torch.cuda.device(eng.dev):
            mi = _msgs_i32(msgs.reshape(-1, msgs.shape[-1]), eng.dev)         # [R, k] or [F * R, k], rows in (frame, region) order
            on_dev = imgs.device == eng.dev
            preds_w = None if is_video else _result_buffer((F_, cd, H, W), torch.float32, imgs.device)

            def one(fr, oc, a, b):
                lab = labels[a:b].to(eng.dev).contiguous()
                keys = (b - a + step - 1) // step
                m = mi.repeat(keys, 1) if msgs.dim() == 2 else mi[a * R:b * R]
                pw = None
                if preds_w is not None:
                    pw = preds_w[a:b] if on_dev else torch.empty(b - a, cd, H, W, device=eng.dev, dtype=torch.float32)
                self._embed_regions_frames(eng, fr, lab, m, oc, R, step=step, video_mode=vm, antialias=aa, lowres=lowres_attenuation, preds_w=pw)
                if pw is not None and not on_dev:
                    preds_w[a:b].copy_(pw, non_blocking=True)       # _run_chunks synchronises before it returns
            out = self._run_chunks(eng, imgs.contiguous() if u8 else imgs, ck * step, one)
        res = {"imgs_w": out, "msgs": msgs_out}
        if preds_w is not None:
            res["preds_w"] = preds_w
        return res

    @torch.no_grad()
    def decode_regions(self, imgs: torch.Tensor, labels: torch.Tensor, method: str = "hard", threshold: float = 0.0, per: str = "frame",
                       is_video: bool = True, interpolation: dict = None, R: Optional[int] = None) -> dict:
        """The message of every region, for pixel-wise detectors: `detect`'s pass chunk by chunk, then ONE pass of the vote kernel over channels
        1.. of the chunk's maps for all regions (the maps never leave the device and are not kept).  labels uint8 [F,H,W] at frame resolution:
        a map pixel looks at the label under its centre (regions.label_index).  R: the number of regions; None reads labels.max() (one host
        synchronisation).  -> {'msgs' bool [F,R,k], 'score' float64 [F,R,k], 'count' int32 [F,R]} on imgs.device, following
        evals/metrics.py:208-256: 'hard': score = votes above `threshold` / pixels; 'semihard': score = mean logit; the bit is score > 0.5 in
        BOTH -- the reference compares the mean logit with 0.5 as well (line 252), and that is kept.  'soft' raises: a label map has no
        fractional weights.  An empty region has a NaN score, False bits and count 0.  per='clip' adds votes, sums and counts over the
        frames first and answers [1,R,k]."""
        from . import regions as RG
        RG.check_decode(method, per)
        F_, H, W, _ = RG.check_frames(imgs, "decode_regions")
        RG.check_labels(labels, F_, H, W)
        if not self.pixelwise:
            raise NotImplementedError("decode_regions votes over [F, 1+nbits, S, S] maps: this detector predicts one row of logits per frame "
                                      "(use detect_regions: the detector on the bounding box of every region)")
        if R is None:
            R = max(1, min(RG.REGIONS_MAX, int(labels.max()))) if F_ else 1
        R = RG.check_regions(R)
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        S = (self.img_size, self.img_size)
        k = self.embedder.cfg.nbits
        if F_ == 0:
            return RG.decide(torch.zeros(0, R, k, dtype=torch.int64), torch.zeros(0, R, dtype=torch.int64), torch.zeros(0, R, k, dtype=torch.float64),
                             method, per)
        parts = []

        def one(fr, oc, a, b):
            p = self._detect_frames(eng, fr, S, aa)
            parts.append(eng.pixel_vote_regions(p[:, 1:], labels[a:b].to(eng.dev).contiguous(), R, threshold))
        with torch.cuda.device(eng.dev):
            self._run_chunks(eng, imgs, max(1, int(self.chunk_size)) if is_video else F_, one, want_out=False, extra=parts.clear)
            votes, nsel, sums = (torch.cat([p[i] for p in parts], 0) for i in range(3))
            res = RG.decide(votes, nsel, sums, method, per)
        return {n: t.to(imgs.device) for n, t in res.items()}

    @torch.no_grad()
    def detect_regions(self, imgs: torch.Tensor, labels: torch.Tensor, R: int, interpolation: dict = None) -> dict:
        """The logits of every region, for per-frame detectors.  By definition `detect_images` on the crops imgs[f, :, y0:y1, x0:x1] of the
        bounding boxes of the present regions, in (f, r) order: NOTHING is masked inside a box, a region that is not a rectangle shares its
        crop with whatever else lies in its box.  The boxes come from one launch on the label map and one copy to the host.
        -> {'preds' fp32 [F,R,1+k] with NaN rows for absent regions, 'boxes' int32 [F,R,4] = (y0, x0, y1, x1), exclusive ends}."""
        from . import regions as RG
        F_, H, W, u8 = RG.check_frames(imgs, "detect_regions")
        RG.check_labels(labels, F_, H, W)
        R = RG.check_regions(R)
        if self.pixelwise:
            raise NotImplementedError("detect_regions runs a per-frame detector on the box of every region: this detector predicts [F, 1+nbits, S, S] "
                                      "maps (use decode_regions: the vote of every region's pixels)")
        eng = self._engine()
        k1 = self.embedder.cfg.nbits + 1
        preds = torch.full((F_, R, k1), float("nan"), dtype=torch.float32, device=imgs.device)
        if F_ == 0:
            return {"preds": preds, "boxes": torch.zeros(0, R, 4, dtype=torch.int32, device=imgs.device)}
        with torch.cuda.device(eng.dev):
            boxes = eng.label_boxes(labels.to(eng.dev).contiguous(), R).cpu()
        where, crops = [], []
        for f, r, (y0, x0, y1, x1) in ((f, r, boxes[f, r].tolist()) for f in range(F_) for r in range(R)):
            if y1 > y0:
                where.append((f, r))
                crops.append(imgs[f, y0:y1, x0:x1, :] if u8 else imgs[f, :, y0:y1, x0:x1])
        if crops:
            rows = self.detect_images(crops, interpolation)["preds"].to(imgs.device)
            idx = torch.tensor(where, dtype=torch.int64, device=imgs.device)
            preds[idx[:, 0], idx[:, 1]] = rows
        return {"preds": preds, "boxes": boxes.to(imgs.device)}

    # ---- embedding to a target PSNR: the watermark's strength per frame, chosen on the device
    @torch.no_grad()
    def embed_psnr(self, imgs: torch.Tensor, target_psnr: float, msgs: torch.Tensor = None, is_video: bool = True, per: str = "frame",
                   max_scaling_w: Optional[float] = None, interpolation: dict = None, lowres_attenuation: bool = False) -> dict:
        """`embed` / `embed_u8` with `blender.scaling_w` replaced by the strength that puts each frame at `target_psnr` dB against `imgs`.
        imgs: fp32 [F,3,H,W] (as `embed`; is_video=False: one message per frame) or uint8 RGB24 [F,H,W,3] (as `embed_u8`).  With d the
        perturbation of frame f at scaling_w = 1 (`preds_w` of `embed`), E_f = (3 / Cd) * sum d^2 in float64 and
            s_f = 10^(-target_psnr / 20) * sqrt(3 H W / E_f),   0 where E_f == 0,   at most max_scaling_w when one is given;
        per="clip": one s for all frames from sum_f E_f over 3 F H W elements (`metrics.psnr(..., is_video=True)`).  Frame f is then
        `embed` of its chunk at blender.scaling_w = s_f, bit for bit.
        Returns {'imgs_w': dtype, shape and device of imgs, 'msgs', 'scaling_w': fp32 [F] the strengths applied, 'energy': float64 [F]}.
        Before the clamp and at scaling_i = 1 the PSNR of imgs_w equals target_psnr (up to the fp32 rounding of s and of the blend) unless the
        ceiling binds.  The clamp only moves pixels towards imgs, so the clamped fp32 result is at or above the target; a uint8 result also
        carries its quantisation noise.  Neither is corrected for.
        An energy pass (the tail's own d, reduced per frame, no frame stored), the strengths and the tail follow each other on the stream
        without a host synchronisation; the call runs eagerly even where VIDEOSEAL_GRAPHS is set.  per="frame" walks the clip in the chunks
        of `embed` (host-resident frames move one chunk at a time); per="clip" keeps the watermark and the low-resolution heat-map of all
        chunks on the device between its two sweeps and needs frames resident on the model's device.
        Lists of images and of clips have their own calls, `embed_images_psnr` and `embed_clips_psnr`.  The YUV and packed-RGB surface routes
        keep the fixed strength: they are not covered."""
        check_psnr_args(target_psnr, per, max_scaling_w)
        _refuse_half(imgs, "embed_psnr", "the half surface route keeps the fixed strength")
        if not torch.is_tensor(imgs) or imgs.dim() != 4:
            raise ValueError("embed_psnr wants fp32 frames [F, 3, H, W] or a uint8 RGB24 clip [F, H, W, 3]")
        u8 = imgs.dtype == torch.uint8
        if (u8 and imgs.shape[-1] != 3) or (not u8 and (imgs.dtype != torch.float32 or imgs.shape[1] != 3)):
            raise ValueError("embed_psnr wants fp32 frames [F, 3, H, W] or a uint8 RGB24 clip [F, H, W, 3]")
        if u8 and not self.clamp:
            raise ValueError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if is_video and self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        F_ = imgs.shape[0]
        if msgs is None:
            msgs = self.get_random_msg() if is_video else self.get_random_msg(F_)
        elif msgs.shape[0] != (1 if is_video else F_):
            raise ValueError("one message for a clip (is_video=True), one per frame otherwise")
        msgs_out = msgs[0:1].repeat(F_, 1) if is_video else msgs
        if F_ == 0:
            return {"imgs_w": imgs.clone(), "msgs": msgs_out, "scaling_w": imgs.new_zeros(0, dtype=torch.float32),
                    "energy": imgs.new_zeros(0, dtype=torch.float64)}
        if u8:
            imgs = imgs.contiguous()          # (as embed_u8: the kernels read packed RGB24; a permuted or strided view of a clip is packed first)
        eng = self._engine()
        if per == "clip" and imgs.device != eng.dev:
            raise ValueError('per="clip" keeps the watermark of the whole clip on the device: it wants frames resident on the model\'s device')
        aa = _antialias_flag(interpolation)
        step = int(self.step_size) if is_video else 1
        span = int(self.chunk_size) * step if is_video else max(1, int(getattr(self, "chunk_size", 32)))
        vm = N.VIDEO_MODES[self.video_mode] if is_video else 0
        H, W = (imgs.shape[1], imgs.shape[2]) if u8 else (imgs.shape[2], imgs.shape[3])
        cap = float(max_scaling_w) if max_scaling_w is not None else None
        with torch.cuda.device(eng.dev):
            mi = self._msgs_dev(msgs, eng.dev)
            energy = torch.empty(F_, device=eng.dev, dtype=torch.float64)
            scale = torch.empty(F_, device=eng.dev, dtype=torch.float32)
            ekw = dict(step=step, video_mode=vm, attenuate=int(self.attenuation is not None), antialias=aa)
            tkw = dict(clamp=self.clamp, scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w, **ekw)

            def front(fr, a, b):
                return self._embed_front(eng, fr, mi if is_video else mi[a:b], step=step, antialias=aa, lowres=lowres_attenuation)

            if per == "frame":
                def one(fr, oc, a, b):
                    delta, hmap = front(fr, a, b)
                    eng.tail_energy(fr, delta, hmap_low=hmap, energy=energy[a:b], **ekw)
                    eng.psnr_scale(energy[a:b], H, W, target_psnr, max_scale=cap, scale=scale[a:b])
                    eng.embed_tail(fr, oc, delta, hmap_low=hmap, frame_scale=scale[a:b], **tkw)
                out = self._run_chunks(eng, imgs, span, one)
            else:
                src = imgs if u8 else N.f32c(imgs)
                out = torch.empty_like(src)
                kept = []
                for a in range(0, F_, span):
                    b = min(F_, a + span)
                    delta, hmap = front(src[a:b], a, b)
                    delta, hmap = delta.clone(), (hmap.clone() if hmap is not None else None)
                    eng.tail_energy(src[a:b], delta, hmap_low=hmap, energy=energy[a:b], **ekw)
                    kept.append((a, b, delta, hmap))
                eng.psnr_scale(energy, H, W, target_psnr, per_clip=True, max_scale=cap, scale=scale)
                for a, b, delta, hmap in kept:
                    eng.embed_tail(src[a:b], out[a:b], delta, hmap_low=hmap, frame_scale=scale[a:b], **tkw)
        return {"imgs_w": out, "msgs": msgs_out, "scaling_w": scale.to(imgs.device), "energy": energy.to(imgs.device)}

    @torch.no_grad()
    def detect_u8(self, clip: torch.Tensor, interpolation: dict = None) -> dict:
        """inference_streaming.py:119-125 (`detect_video_clip`): uint8 [F,H,W,3] -> {'preds': [F, 1+nbits]}."""
        if clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[-1] != 3:
            raise ValueError("detect_u8 wants a uint8 RGB24 clip [F, H, W, 3]")
        self._per_frame_rows_only("detect_u8")
        if clip.shape[0] == 0:
            self._engine()
            return {"preds": torch.zeros((0, self.embedder.cfg.nbits + 1), device=clip.device)}
        return {"preds": self._detect_clip(clip.contiguous(), interpolation)}

    # ---- lists of clips of different sizes and lengths, a message per clip: the key frames of many short clips share a U-Net pass (clips.py)
    @staticmethod
    def _clip_list(clips, what: str):
        """-> (the clips as given, uint8?) after the checks: all fp32 [F, 3, H, W] or all uint8 RGB24 [F, H, W, 3]; F may be 0"""
        clips = list(clips)
        if not all(torch.is_tensor(t) for t in clips):
            raise TypeError(f"{what} wants a sequence of tensors")
        if len({t.dtype for t in clips}) > 1:
            raise ValueError(f"{what}: the clips of one call are all fp32 [F, 3, H, W] or all uint8 [F, H, W, 3], got {sorted({str(t.dtype) for t in clips})}")
        u8 = bool(clips) and clips[0].dtype == torch.uint8
        if clips and not (u8 or clips[0].is_floating_point()):
            raise ValueError(f"{what}: clips are fp32 [F, 3, H, W] or uint8 [F, H, W, 3], got {clips[0].dtype}")
        for t in clips:
            if t.dim() != 4 or t.shape[-1 if u8 else 1] != 3 or 0 in t.shape[1:]:
                raise ValueError(f"{what}: " + ("uint8 clips are RGB24 [F, H, W, 3]" if u8 else "fp32 clips are [F, 3, H, W]") + f", got {tuple(t.shape)}")
        return clips, u8

    def _clip_passes(self, eng: HipEngine, clips, u8: bool, passes, fn, restart=None) -> None:
        """Drive `fn(slots, extra, frames)` over `passes` = [(slots, extra)] of clips.py: frames[s] is slot s of the pass on the device, contiguous.  Device-resident clips
        are sliced in place; others move pass by pass, and such a call synchronises before it returns, so the range guard of its passes is read
        here and a data-dependent overflow repeats the call on the exact split (as _image_chunks does for a list of images)."""
        on_dev = all(t.device == eng.dev for t in clips if t.shape[0])
        res = [(t.contiguous() if u8 else N.f32c(t)) if (t.device == eng.dev and t.shape[0]) else t for t in clips]
        for attempt in range(2):
            for slots, extra in passes:
                frames = []
                for s in slots:
                    ch = res[s[0]][s[1]:s[1] + s[2]]
                    if ch.device != eng.dev:
                        ch = ch.to(eng.dev)
                        ch = ch.contiguous() if u8 else N.f32c(ch)
                    frames.append(ch)
                fn(slots, extra, frames)
            if on_dev:
                break
            torch.cuda.current_stream(eng.dev).synchronize()
            if attempt or not eng.guard_tripped_after_sync():
                break
            if restart is not None:
                restart()

    @torch.no_grad()
    def embed_clips(self, clips, msgs: torch.Tensor = None, interpolation: dict = None, lowres_attenuation: bool = False) -> dict:
        """`embed(clip_i, msgs[i:i+1], is_video=True)` (`embed_u8` for uint8) for every clip of a list whose clips differ in size and length, with
        the key frames of many clips going through the U-Net as one batch (up to streaming.KEY_BATCH per pass) instead of chunk_size per clip.
        clips: n tensors, all fp32 [F_i, 3, H_i, W_i] or all uint8 RGB24 [F_i, H_i, W_i, 3] (needs clamp=True), F_i >= 0; msgs [n, k] (row i for
        clip i) or None (random).  -> {'imgs_w': list, 'msgs'}: result i has the shape, dtype and device of clip i; for device-resident clips
        the results are views of one allocation per call.  Per pass (clips.py): one resize launch group (vs_resize_pre_clips), one embedder pass
        with one message row per key frame, one low-resolution heat-map when asked, one tail launch group (vs_embed_tail_clips).  The watermark
        expansion restarts at every span as in the per-clip call, so clip i equals that call up to the summation order of the dense layers (a K
        split is a function of the batch shape, see embed_group).  Always eager (no hipGraph route)."""
        from . import clips as CL
        if self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        clips = list(clips)
        _refuse_half(clips, "embed_clips", "lists of clips are fp32 or uint8")
        clips, u8 = self._clip_list(clips, "embed_clips")
        n = len(clips)
        if u8 and not self.clamp:
            raise NotImplementedError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg(n)
        elif msgs.shape[0] != n:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {n} clips")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        if n == 0:
            return {"msgs": msgs, "imgs_w": []}
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        lowres = bool(lowres_attenuation)
        step, vm = int(self.step_size), N.VIDEO_MODES[self.video_mode]
        odt = torch.uint8 if u8 else torch.float32
        passes = CL.embed_passes([t.shape[0] for t in clips], step, max(1, int(self.chunk_size)))
        on_dev = all(t.device == eng.dev for t in clips if t.shape[0])
        with torch.cuda.device(eng.dev):
            if on_dev:          # one allocation, clip after clip
                flat = torch.empty(sum(t.numel() for t in clips), dtype=odt, device=eng.dev)
                outs, pos = [], 0
                for t in clips:
                    outs.append(flat[pos:pos + t.numel()].view(t.shape))
                    pos += t.numel()
            else:
                outs = [_result_buffer(t.shape, odt, t.device) if t.shape[0] else torch.empty(t.shape, dtype=odt, device=t.device) for t in clips]
            if passes:
                mi = self._msgs_dev(msgs, eng.dev)

            def one(slots, rows, frames):
                dst = [outs[c][a:a + f] if on_dev else torch.empty_like(fr) for (c, a, f, _, _), fr in zip(slots, frames)]
                desc = [(fr, ff, fk) for (_, _, _, ff, fk), fr in zip(slots, frames)]
                rgb, key = eng.resize_pre_clips(desc, S, aa, want_rgb=(att and lowres), want_key=True, key_step=step)
                delta = eng.embedder_forward(key, mi.index_select(0, torch.tensor(rows, device=eng.dev)), bn_train=self.embedder.training)
                hmap = eng.jnd_lowres(rgb) if (att and lowres) else None
                eng.embed_tail_clips(desc, dst, delta, step=step, video_mode=vm, hmap_low=hmap, attenuate=int(att), clamp=self.clamp, antialias=aa,
                                     scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w)
                if not on_dev:        # back to where each clip came from (_clip_passes synchronises before it returns)
                    for (c, a, f, _, _), o in zip(slots, dst):
                        outs[c][a:a + f].copy_(o, non_blocking=True)
            self._clip_passes(eng, clips, u8, passes, one)
        return {"msgs": msgs, "imgs_w": outs}

    @torch.no_grad()
    def embed_clips_psnr(self, clips, target_psnr: float, msgs: torch.Tensor = None, per: str = "frame", max_scaling_w: Optional[float] = None,
                         interpolation: dict = None, lowres_attenuation: bool = False) -> dict:
        """`embed_clips` with `blender.scaling_w` replaced by the strength that puts every frame (per="frame") or every clip (per="clip") at
        `target_psnr` dB against its original, by the formula of `embed_psnr`: s = 10^(-target_psnr / 20) * sqrt(n / E) with E the float64
        energy of the perturbation at strength 1 over n = 3 H_i W_i elements of a frame, or over the 3 F_i H_i W_i elements of clip i with E
        summed over all its frames -- as a whole, also where chunk_size cut the clip into several spans and passes.  0 where E == 0, at most
        max_scaling_w when one is given.  Every frame is then that frame of `embed_clips` at blender.scaling_w = its strength, bit for bit.
        Returns what `embed_clips` returns plus 'scaling_w' (list of fp32 [F_i], the strengths applied) and 'energy' (list of float64 [F_i]),
        each on its clip's device.
        per="frame": every pass of `embed_clips` is followed, on the stream, by its energy pass (vs_embed_tail_clips_energy), its strengths
        (vs_psnr_scale_items) and the tail with a strength per frame (vs_embed_tail_clips_scaled); host-resident clips move pass by pass.
        per="clip" makes two sweeps: the first runs the network passes and the energy passes and keeps the watermark and the low-resolution
        heat-map of every pass on the device, one vs_psnr_scale_items call with the clip boundaries sits between them, the second runs the
        tails.  It needs clips resident on the model's device.  No host synchronisation in either; always eager."""
        from . import clips as CL
        check_psnr_args(target_psnr, per, max_scaling_w)
        if self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        clips = list(clips)
        _refuse_half(clips, "embed_clips_psnr", "lists of clips are fp32 or uint8")
        clips, u8 = self._clip_list(clips, "embed_clips_psnr")
        n = len(clips)
        if u8 and not self.clamp:
            raise ValueError("uint8 output needs clamp=True ((x * 255).byte() is undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg(n)
        elif msgs.shape[0] != n:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {n} clips")
        aa = _antialias_flag(interpolation)
        eng = self._engine()
        if n == 0:
            return {"msgs": msgs, "imgs_w": [], "scaling_w": [], "energy": []}
        on_dev = all(t.device == eng.dev for t in clips if t.shape[0])
        if per == "clip" and not on_dev:
            raise ValueError('per="clip" keeps the watermark of every pass on the device: it wants clips resident on the model\'s device')
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        lowres = bool(lowres_attenuation)
        step, vm = int(self.step_size), N.VIDEO_MODES[self.video_mode]
        odt = torch.uint8 if u8 else torch.float32
        lengths = [t.shape[0] for t in clips]
        passes = CL.embed_passes(lengths, step, max(1, int(self.chunk_size)))
        first = CL.first_rows(lengths)          # the frames of the list, clip after clip: the passes walk them in this order
        total = first[-1]
        cap = float(max_scaling_w) if max_scaling_w is not None else None
        with torch.cuda.device(eng.dev):
            if on_dev:          # one allocation, clip after clip
                flat = torch.empty(sum(t.numel() for t in clips), dtype=odt, device=eng.dev)
                outs, pos = [], 0
                for t in clips:
                    outs.append(flat[pos:pos + t.numel()].view(t.shape))
                    pos += t.numel()
            else:
                outs = [_result_buffer(t.shape, odt, t.device) if t.shape[0] else torch.empty(t.shape, dtype=odt, device=t.device) for t in clips]
            energy = torch.empty(total, device=eng.dev, dtype=torch.float64)
            scale = torch.empty(total, device=eng.dev, dtype=torch.float32)
            if passes:
                mi = self._msgs_dev(msgs, eng.dev)
                hw = [(t.shape[1], t.shape[2]) if u8 else (t.shape[2], t.shape[3]) for t in clips]
                elems = torch.tensor([3.0 * h * w for (h, w), f in zip(hw, lengths) for _ in range(f)], dtype=torch.float64).to(eng.dev)
            ekw = dict(step=step, video_mode=vm, attenuate=int(att), antialias=aa)
            tkw = dict(clamp=self.clamp, scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w, **ekw)
            kept = []

            def one(slots, rows, frames):
                # the pass owns a contiguous run of the list's frames: slot s sits at first_frame inside it
                p0 = first[slots[0][0]] + slots[0][1]
                p1 = first[slots[-1][0]] + slots[-1][1] + slots[-1][2]
                desc = [(fr, ff, fk) for (_, _, _, ff, fk), fr in zip(slots, frames)]
                rgb, key = eng.resize_pre_clips(desc, S, aa, want_rgb=(att and lowres), want_key=True, key_step=step)
                delta = eng.embedder_forward(key, mi.index_select(0, torch.tensor(rows, device=eng.dev)), bn_train=self.embedder.training)
                hmap = eng.jnd_lowres(rgb) if (att and lowres) else None
                if per == "clip":         # the workspaces of the next pass would overwrite them
                    delta, hmap = delta.clone(), (hmap.clone() if hmap is not None else None)
                eng.tail_energy_clips(desc, delta, hmap_low=hmap, energy=energy[p0:p1], **ekw)
                if per == "clip":
                    kept.append((slots, desc, delta, hmap, p0, p1))
                    return
                eng.psnr_scale_items(energy[p0:p1], elems[p0:p1], target_psnr, max_scale=cap, scale=scale[p0:p1])
                dst = [outs[c][a:a + f] if on_dev else torch.empty_like(fr) for (c, a, f, _, _), fr in zip(slots, frames)]
                eng.embed_tail_clips(desc, dst, delta, hmap_low=hmap, frame_scale=scale[p0:p1], **tkw)
                if not on_dev:        # back to where each clip came from (_clip_passes synchronises before it returns)
                    for (c, a, f, _, _), o in zip(slots, dst):
                        outs[c][a:a + f].copy_(o, non_blocking=True)
            self._clip_passes(eng, clips, u8, passes, one)
            if per == "clip" and kept:
                eng.psnr_scale_items(energy, elems, target_psnr, first_item=torch.tensor(first, dtype=torch.int32).to(eng.dev), max_scale=cap,
                                     scale=scale)
                for slots, desc, delta, hmap, p0, p1 in kept:
                    dst = [outs[c][a:a + f] for (c, a, f, _, _) in slots]
                    eng.embed_tail_clips(desc, dst, delta, hmap_low=hmap, frame_scale=scale[p0:p1], **tkw)
        return {"msgs": msgs, "imgs_w": outs,
                "scaling_w": [scale[first[i]:first[i + 1]].to(clips[i].device) for i in range(n)],
                "energy": [energy[first[i]:first[i + 1]].to(clips[i].device) for i in range(n)]}

    def _detect_clip_rows(self, eng: HipEngine, clips, u8: bool, aa: bool) -> Optional[torch.Tensor]:
        """the detector's output for every frame of the flattened list, on the device (None for a list without frames): one resize launch group
        and one extractor pass per streaming.DET_BATCH frames, whichever clips they belong to"""
        from . import clips as CL
        S = (self.img_size, self.img_size)
        preds = []

        def one(slots, _, frames):
            rgb, _ = eng.resize_pre_clips([(fr, ff, 0) for (_, _, _, ff), fr in zip(slots, frames)], S, aa, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
            p = eng.extractor_forward(rgb)
            preds.append(p if eng.preds_owned else p.clone())
        self._clip_passes(eng, clips, u8, [(s, None) for s in CL.detect_passes([t.shape[0] for t in clips])], one, restart=preds.clear)
        return torch.cat(preds, dim=0) if preds else None

    @torch.no_grad()
    def detect_clips(self, clips, interpolation: dict = None) -> dict:
        """`detect(clip_i, is_video=True)` for every clip of a list (see embed_clips) -> {'preds': list of [F_i, 1+nbits]}, entry i on clip i's
        device; the extractor runs on up to streaming.DET_BATCH frames of the flattened list at a time."""
        from . import clips as CL
        clips, u8 = self._clip_list(clips, "detect_clips")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        with torch.cuda.device(eng.dev):
            rows = self._detect_clip_rows(eng, clips, u8, aa)
            first = CL.first_rows([t.shape[0] for t in clips])
            return {"preds": [rows[first[i]:first[i + 1]].to(t.device) if t.shape[0] else torch.zeros(self._empty_preds_shape(), device=t.device)
                              for i, t in enumerate(clips)]}

    @torch.no_grad()
    def extract_messages(self, clips, aggregation: str = "avg",
                         interpolation: dict = {"mode": "bilinear", "align_corners": False, "antialias": False}) -> torch.Tensor:
        """`extract_message(clip_i, aggregation, interpolation)` for every clip of a list -> bool [n, nbits], row i for clip i (on the first
        clip's device): detect_clips' passes, then the frame aggregation of all clips in one launch (vs_aggregate_clips); a clip without
        frames aggregates to zeros, i.e. to all-False."""
        from . import clips as CL
        self._per_frame_rows_only("extract_messages")
        if aggregation not in N.AGGREGATIONS:
            raise ValueError(f"unknown aggregation {aggregation}")
        clips, u8 = self._clip_list(clips, "extract_messages")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        n, k = len(clips), self.embedder.cfg.nbits
        if n == 0:
            return torch.zeros((0, k), dtype=torch.bool)
        with torch.cuda.device(eng.dev):
            rows = self._detect_clip_rows(eng, clips, u8, aa)
            if rows is None:
                return torch.zeros((n, k), dtype=torch.bool, device=clips[0].device)
            first = torch.tensor(CL.first_rows([t.shape[0] for t in clips]), dtype=torch.int32, device=eng.dev)
            return (eng.aggregate_clips(rows.contiguous(), first, aggregation) > 0).to(clips[0].device)

    # ---- YUV clips (videoseal_amd/yuv.py): one body for the three pairs of methods below
    def _yuv_clip(self, planes, fmt: str, what: str, matrix: str, full_range: bool, module):
        """the validated planes as a yuv.Clip; `module` (yuv or its restriction yuv420) has the formats and matrices `what` accepts"""
        from .yuv import Clip
        module.check_clip(planes, fmt, what)
        if matrix not in module.MATRICES:
            raise ValueError(f"{what}: matrix must be one of {sorted(module.MATRICES)}, got {matrix!r}")
        return Clip(planes, fmt, (matrix, bool(full_range)))

    def _embed_yuv(self, clip, what: str, msgs, interpolation, lowres_attenuation):
        """(the watermarked clip -- packed: `buf` [F, samples per frame] and the plane views of it --, msgs per frame)"""
        if not self.clamp:
            raise NotImplementedError(f"{what} needs clamp=True (codes are undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg()
        else:
            assert msgs.shape[0] == 1, "Message should be unique"
        if clip.shape[0] == 0 or clip.numel() == 0:
            out = clip.clone()
        else:
            out = self._embed_clip(clip, msgs, interpolation, lowres_attenuation)
        return out, msgs[0:1].repeat(len(clip), 1)

    def _detect_yuv(self, clip, what: str, interpolation) -> dict:
        self._per_frame_rows_only(what)
        if clip.shape[0] == 0:
            return {"preds": torch.zeros((0, self.embedder.cfg.nbits + 1), device=clip.device)}
        return {"preds": self._detect_clip(clip, interpolation)}

    # ---- uint8 NV12 clips (videoseal_amd/nv12.py): what a hardware decoder hands over, 1.5 bytes per pixel each way
    def _nv12_clip(self, clip: torch.Tensor, what: str, matrix: str, full_range: bool):
        """the clip as a yuv.Clip of format "nv12": its two planes are strided views of the caller's buffer"""
        from . import nv12
        from .yuv import Clip
        y, uv = nv12.planes(clip, what)
        if matrix not in nv12.MATRICES:
            raise ValueError(f"{what}: matrix must be one of {sorted(nv12.MATRICES)}, got {matrix!r}")
        F_, R, W = clip.shape
        if clip.stride(1) < W or (F_ > 1 and clip.stride(0) < clip.stride(1) * (R - 1) + W):
            raise ValueError(f"{what}: rows and frames must not overlap")
        self._engine()
        return Clip((y, uv), "nv12", (matrix, bool(full_range)))

    @torch.no_grad()
    def embed_nv12(self, clip: torch.Tensor, msgs: torch.Tensor = None, interpolation: dict = None, lowres_attenuation: bool = True,
                   matrix: str = "bt709", full_range: bool = False) -> dict:
        """clip uint8 [F, 3H/2, W] (NV12: H luma rows, then H/2 rows of interleaved CbCr per 2 x 2 block; H, W even; last stride 1, any row
        pitch >= W and frame stride -- a pitched decoder surface is a strided view, not a copy) -> {'imgs_w': contiguous uint8
        [F, 3H/2, W], 'msgs'}.  Means: NV12 -> RGB fp32 (nv12.nv12_to_rgb: the block's chroma for its four pixels, clamp to [0, 1]) ->
        embed(..., is_video=True) -> RGB -> NV12 (nv12.rgb_to_nv12: mean of the block's four chroma values, codes =
        floor(clamp(v, 0, 255) + 0.5)), with both conversions fused into the resize and tail kernels: no RGB or fp32 frame is written.
        `matrix` is "bt601" or "bt709", `full_range` selects 0..255 codes instead of 16..235 / 16..240.  Needs clamp=True."""
        planes = self._nv12_clip(clip, "embed_nv12", matrix, full_range)
        out, msgs = self._embed_yuv(planes, "embed_nv12", msgs, interpolation, lowres_attenuation)      # a packed buffer [F, 3HW/2]: Y, then UV
        if clip.numel() == 0:
            return {"imgs_w": clip.clone().contiguous(), "msgs": msgs}
        return {"imgs_w": out.buf.view(clip.shape), "msgs": msgs}

    @torch.no_grad()
    def detect_nv12(self, clip: torch.Tensor, interpolation: dict = None, matrix: str = "bt709", full_range: bool = False) -> dict:
        """clip uint8 [F, 3H/2, W] (see embed_nv12) -> {'preds': [F, 1+nbits]}: detect(nv12.nv12_to_rgb(clip), is_video=True) with the
        conversion fused into the resize kernel."""
        return self._detect_yuv(self._nv12_clip(clip, "detect_nv12", matrix, full_range), "detect_nv12", interpolation)

    # ---- 4:2:0 clips as planes (videoseal_amd/yuv420.py): nv12, i420, p010, yuv420p10, every plane at its own pitch
    @torch.no_grad()
    def embed_yuv420(self, planes, fmt: str, msgs: torch.Tensor = None, interpolation: dict = None, lowres_attenuation: bool = True,
                     matrix: str = "bt709", full_range: bool = False) -> dict:
        """planes: the plane tensors of a 4:2:0 clip of format `fmt` ("nv12", "i420", "p010", "yuv420p10": yuv.py; H, W even, last stride 1,
        any row pitch and frame stride per plane) -> {'planes_w': plane views, 'imgs_w': the packed contiguous buffer [F, 3HW/2] they view,
        'msgs'}.  Means: yuv420.to_rgb -> embed(..., is_video=True) -> yuv420.from_rgb with both conversions fused into the resize and tail
        kernels: no RGB or fp32 frame is written, and a 10-bit clip keeps its 10 bits.  `matrix` is "bt601", "bt709" or "bt2020",
        `full_range` selects full-range codes.  Needs clamp=True."""
        from . import yuv420
        clip = self._yuv_clip(planes, fmt, "embed_yuv420", matrix, full_range, yuv420)
        out, msgs = self._embed_yuv(clip, "embed_yuv420", msgs, interpolation, lowres_attenuation)
        return {"planes_w": out.planes, "imgs_w": out.buf, "msgs": msgs}

    @torch.no_grad()
    def detect_yuv420(self, planes, fmt: str, interpolation: dict = None, matrix: str = "bt709", full_range: bool = False) -> dict:
        """planes, fmt as in embed_yuv420 -> {'preds': [F, 1+nbits]}: detect(yuv420.to_rgb(planes, fmt), is_video=True) with the conversion
        fused into the resize kernel."""
        from . import yuv420
        return self._detect_yuv(self._yuv_clip(planes, fmt, "detect_yuv420", matrix, full_range, yuv420), "detect_yuv420", interpolation)

    # ---- clips of any of the ten YUV formats (videoseal_amd/yuv.py): the 4:2:0 ones and yuv422p, yuv422p10, nv16, p210, yuv444p, yuv444p10
    @torch.no_grad()
    def embed_yuv(self, planes, fmt: str, msgs: torch.Tensor = None, interpolation: dict = None, lowres_attenuation: bool = True,
                  matrix: str = "bt709", full_range: bool = False) -> dict:
        """planes: the plane tensors of a clip of format `fmt` (yuv.py: the four 4:2:0 formats of embed_yuv420, "yuv422p", "yuv422p10", "nv16",
        "p210" -- W even -- and "yuv444p", "yuv444p10" -- any size; last stride 1, any row pitch and frame stride per plane) -> {'planes_w':
        plane views, 'imgs_w': the packed contiguous buffer they view (2HW samples per frame for 4:2:2, 3HW for 4:4:4), 'msgs'}.  Means:
        yuv.to_rgb -> embed(..., is_video=True) -> yuv.from_rgb with both conversions and the chroma resampling fused into the resize and tail
        kernels: no RGB or fp32 frame is written, and a 10-bit clip keeps its 10 bits.  A 4:2:0 `fmt` gives embed_yuv420's words.  `matrix` is
        "bt601", "bt709" or "bt2020", `full_range` selects full-range codes.  Needs clamp=True."""
        from . import yuv
        clip = self._yuv_clip(planes, fmt, "embed_yuv", matrix, full_range, yuv)
        out, msgs = self._embed_yuv(clip, "embed_yuv", msgs, interpolation, lowres_attenuation)
        return {"planes_w": out.planes, "imgs_w": out.buf, "msgs": msgs}

    @torch.no_grad()
    def detect_yuv(self, planes, fmt: str, interpolation: dict = None, matrix: str = "bt709", full_range: bool = False) -> dict:
        """planes, fmt as in embed_yuv -> {'preds': [F, 1+nbits]}: detect(yuv.to_rgb(planes, fmt), is_video=True) with the conversion fused
        into the resize kernel.  A 4:2:0 `fmt` gives detect_yuv420's logits."""
        from . import yuv
        return self._detect_yuv(self._yuv_clip(planes, fmt, "detect_yuv", matrix, full_range, yuv), "detect_yuv", interpolation)

    # ---- lists of YUV clips: the clip lists above on decoder surfaces (vs_resize_pre_yuv_clips / vs_embed_tail_yuv_clips)
    def _yuv_clip_list(self, clips, fmt: str, what: str, matrix: str, full_range: bool):
        """the clips as yuv.Clip objects after the checks: plane tuples of ONE format, each a valid clip of it (F may be 0)"""
        from . import yuv
        clips = list(clips)
        if any(torch.is_tensor(c) for c in clips):
            raise TypeError(f"{what} wants a sequence of plane tuples of format {fmt!r}; fp32 and uint8 RGB24 tensors go to {what[:-len('_yuv')]}")
        yuv.fmt_info(fmt)
        if matrix not in yuv.MATRICES:
            raise ValueError(f"{what}: matrix must be one of {sorted(yuv.MATRICES)}, got {matrix!r}")
        out = []
        for i, planes in enumerate(clips):
            if isinstance(planes, yuv.Clip):
                if planes.fmt != fmt:
                    raise ValueError(f"{what}: the clips of one call share a format, clip {i} is {planes.fmt}, not {fmt}")
                planes = planes.planes
            yuv.check_clip(planes, fmt, f"{what}: clip {i}")
            out.append(yuv.Clip(planes, fmt, (matrix, bool(full_range))))
        return out

    def _yuv_clip_passes(self, eng: HipEngine, clips, passes, fn, restart=None) -> None:
        """_clip_passes for yuv.Clip objects: device-resident planes are sliced in place at their own pitches, others move pass by pass"""
        on_dev = all(c.device == eng.dev for c in clips if c.shape[0])
        for attempt in range(2):
            for slots, extra in passes:
                frames = []
                for s in slots:
                    ch = clips[s[0]][s[1]:s[1] + s[2]]
                    frames.append(ch if ch.device == eng.dev else ch.to(eng.dev))
                fn(slots, extra, frames)
            if on_dev:
                break
            torch.cuda.current_stream(eng.dev).synchronize()
            if attempt or not eng.guard_tripped_after_sync():
                break
            if restart is not None:
                restart()

    @torch.no_grad()
    def embed_clips_yuv(self, clips, fmt: str, msgs: torch.Tensor = None, interpolation: dict = None, lowres_attenuation: bool = True,
                        matrix: str = "bt709", full_range: bool = False) -> dict:
        """`embed_yuv(clip_i, fmt, msgs[i:i+1])` for every clip of a list whose clips differ in size and length, with the key frames of many
        clips going through the U-Net as one batch, as embed_clips does for fp32 and RGB24 clips.  clips: n plane tuples as embed_yuv takes
        them, all of format `fmt` and one colour choice (planes at any pitch and frame stride: views of decoder surfaces are fine), F_i >= 0;
        msgs [n, k] or None (random).  -> {'planes_w': [plane tuple per clip], 'imgs_w': [the packed buffer [F_i, samples per frame] each
        tuple views], 'msgs'}; for device-resident clips the buffers are views of one allocation per call, clip after clip.  Per pass
        (clips.embed_passes): one resize launch set (vs_resize_pre_yuv_clips), one embedder pass with a message row per key frame, one
        low-resolution heat-map when asked, one tail launch set (vs_embed_tail_yuv_clips, always the 16-row tile kernel).  No RGB or fp32 frame
        is written and a 10-bit clip keeps its 10 bits.  Needs clamp=True.  Always eager (no hipGraph route)."""
        from . import clips as CL
        from . import yuv
        if self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        clips = self._yuv_clip_list(clips, fmt, "embed_clips_yuv", matrix, full_range)
        n = len(clips)
        if not self.clamp:
            raise NotImplementedError("embed_clips_yuv needs clamp=True (codes are undefined outside [0, 1])")
        if msgs is None:
            msgs = self.get_random_msg(n)
        elif msgs.shape[0] != n:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {n} clips")
        if n == 0:
            return {"msgs": msgs, "planes_w": [], "imgs_w": []}
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        S = (self.img_size, self.img_size)
        att = self.attenuation is not None
        lowres = bool(lowres_attenuation)
        step, vm = int(self.step_size), N.VIDEO_MODES[self.video_mode]
        passes = CL.embed_passes([c.shape[0] for c in clips], step, max(1, int(self.chunk_size)))
        on_dev = all(c.device == eng.dev for c in clips if c.shape[0])
        with torch.cuda.device(eng.dev):
            if on_dev:          # one allocation, clip after clip
                sizes = [c.shape[0] * yuv.frame_samples(fmt, c.shape[1], c.shape[2]) for c in clips]
                flat = torch.empty(sum(sizes), dtype=yuv.fmt_dtype(fmt), device=eng.dev)
                outs, pos = [], 0
                for c, sz in zip(clips, sizes):
                    buf = flat[pos:pos + sz].view(c.shape[0], -1) if c.shape[0] else flat[pos:pos].view(0, yuv.frame_samples(fmt, c.shape[1], c.shape[2]))
                    outs.append(yuv.Clip(yuv.planes_of(buf, fmt, c.shape[1], c.shape[2]), fmt, c.color, buf))
                    pos += sz
            else:
                outs = [c.empty_like() for c in clips]
            if passes:
                mi = self._msgs_dev(msgs, eng.dev)

            def one(slots, rows, frames):
                dst = [outs[c][a:a + f] if on_dev else fr.empty_like() for (c, a, f, _, _), fr in zip(slots, frames)]
                desc = [(fr, ff, fk) for (_, _, _, ff, fk), fr in zip(slots, frames)]
                rgb, key = eng.resize_pre_clips(desc, S, aa, want_rgb=(att and lowres), want_key=True, key_step=step)
                delta = eng.embedder_forward(key, mi.index_select(0, torch.tensor(rows, device=eng.dev)), bn_train=self.embedder.training)
                hmap = eng.jnd_lowres(rgb) if (att and lowres) else None
                eng.embed_tail_clips(desc, dst, delta, step=step, video_mode=vm, hmap_low=hmap, attenuate=int(att), clamp=self.clamp, antialias=aa,
                                     scaling_i=self.blender.scaling_i, scaling_w=self.blender.scaling_w)
                if not on_dev:        # back to where each clip came from (_yuv_clip_passes synchronises before it returns)
                    for (c, a, f, _, _), o in zip(slots, dst):
                        outs[c][a:a + f].copy_(o, non_blocking=True)
            self._yuv_clip_passes(eng, clips, passes, one)
        return {"msgs": msgs, "planes_w": [o.planes for o in outs], "imgs_w": [o.buf for o in outs]}

    def _detect_yuv_clip_rows(self, eng: HipEngine, clips, aa: bool) -> Optional[torch.Tensor]:
        """_detect_clip_rows for yuv.Clip objects"""
        from . import clips as CL
        S = (self.img_size, self.img_size)
        preds = []

        def one(slots, _, frames):
            rgb, _ = eng.resize_pre_clips([(fr, ff, 0) for (_, _, _, ff), fr in zip(slots, frames)], S, aa, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
            p = eng.extractor_forward(rgb)
            preds.append(p if eng.preds_owned else p.clone())
        self._yuv_clip_passes(eng, clips, [(s, None) for s in CL.detect_passes([c.shape[0] for c in clips])], one, restart=preds.clear)
        return torch.cat(preds, dim=0) if preds else None

    @torch.no_grad()
    def detect_clips_yuv(self, clips, fmt: str, interpolation: dict = None, matrix: str = "bt709", full_range: bool = False) -> dict:
        """`detect_yuv(clip_i, fmt)` for every clip of a list (see embed_clips_yuv) -> {'preds': list of [F_i, 1+nbits]}, entry i on clip i's
        device; the extractor runs on up to streaming.DET_BATCH frames of the flattened list at a time (clips.detect_passes)."""
        from . import clips as CL
        clips = self._yuv_clip_list(clips, fmt, "detect_clips_yuv", matrix, full_range)
        if not clips:
            return {"preds": []}
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        with torch.cuda.device(eng.dev):
            rows = self._detect_yuv_clip_rows(eng, clips, aa)
            first = CL.first_rows([c.shape[0] for c in clips])
            return {"preds": [rows[first[i]:first[i + 1]].to(c.device) if c.shape[0] else torch.zeros(self._empty_preds_shape(), device=c.device)
                              for i, c in enumerate(clips)]}

    @torch.no_grad()
    def extract_messages_yuv(self, clips, fmt: str, aggregation: str = "avg",
                             interpolation: dict = {"mode": "bilinear", "align_corners": False, "antialias": False},
                             matrix: str = "bt709", full_range: bool = False) -> torch.Tensor:
        """`extract_message(yuv.to_rgb(clip_i, fmt), aggregation, interpolation)` for every clip of a list -> bool [n, nbits], row i for clip i
        (on the first clip's device): detect_clips_yuv's passes, then the frame aggregation of all clips in one launch (vs_aggregate_clips); a
        clip without frames aggregates to zeros, i.e. to all-False."""
        from . import clips as CL
        self._per_frame_rows_only("extract_messages_yuv")
        if aggregation not in N.AGGREGATIONS:
            raise ValueError(f"unknown aggregation {aggregation}")
        clips = self._yuv_clip_list(clips, fmt, "extract_messages_yuv", matrix, full_range)
        n, k = len(clips), self.embedder.cfg.nbits
        if n == 0:
            return torch.zeros((0, k), dtype=torch.bool)
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        with torch.cuda.device(eng.dev):
            rows = self._detect_yuv_clip_rows(eng, clips, aa)
            if rows is None:
                return torch.zeros((n, k), dtype=torch.bool, device=clips[0].device)
            first = torch.tensor(CL.first_rows([c.shape[0] for c in clips]), dtype=torch.int32, device=eng.dev)
            return (eng.aggregate_clips(rows.contiguous(), first, aggregation) > 0).to(clips[0].device)

    # ---- packed RGB clips (videoseal_amd/rgbpack.py): what capture, compositors and image decoders hold, alpha / X carried through
    @torch.no_grad()
    def embed_rgb(self, clip: torch.Tensor, fmt: str, msgs: torch.Tensor = None, interpolation: dict = None,
                  lowres_attenuation: bool = True) -> dict:
        """clip: a packed RGB clip of format `fmt` (rgbpack.py: "rgb24", "bgr24", "rgba", "bgra", "argb", "abgr" uint8 [F, H, W, 3 | 4];
        "rgb48", "bgr48", "rgba64", "bgra64" uint16 [F, H, W, 3 | 4]; "x2rgb10", "x2bgr10" int32 [F, H, W]; compact pixels, any row pitch and
        frame stride) -> {'imgs_w': a contiguous clip of the same dtype and shape, 'msgs'}.  Means: rgbpack.to_rgb -> embed(..., is_video=True)
        -> rgbpack.from_rgb(like=clip) with both conversions fused into the resize and tail kernels: no fp32 frame is written, a 16-bit clip
        keeps its 16 bits, and alpha / X of the result are the clip's, bit for bit."""
        from . import rgbpack
        rgbpack.check_clip(clip, fmt, "embed_rgb")
        out, msgs = self._embed_yuv(rgbpack.Clip(clip, fmt), "embed_rgb", msgs, interpolation, lowres_attenuation)
        res = out.tensor
        return {"imgs_w": res.view(clip.dtype) if res.dtype != clip.dtype else res, "msgs": msgs}

    @torch.no_grad()
    def detect_rgb(self, clip: torch.Tensor, fmt: str, interpolation: dict = None) -> dict:
        """clip, fmt as in embed_rgb -> {'preds': [F, 1+nbits]}: detect(rgbpack.to_rgb(clip, fmt), is_video=True) with the conversion fused
        into the resize kernel."""
        from . import rgbpack
        rgbpack.check_clip(clip, fmt, "detect_rgb")
        return self._detect_yuv(rgbpack.Clip(clip, fmt), "detect_rgb", interpolation)

    # ---- half-precision clips (videoseal_amd/halfpix.py): what an image or video generator's decoder hands over
    def _half_clip(self, imgs, what: str, value_range: str, layout: str):
        from . import halfpix
        if isinstance(imgs, (list, tuple)):
            raise NotImplementedError(f"{what} takes one clip: lists of images or clips (embed_images / embed_clips) are fp32 or uint8")
        if torch.is_tensor(imgs) and imgs.dtype not in halfpix.DTYPES:
            raise ValueError(f"{what} wants a float16 or bfloat16 clip, got {imgs.dtype}: fp32 frames go to embed / detect, integer ones to "
                             f"embed_rgb / detect_rgb")
        halfpix.check_clip(imgs, layout, value_range, what)
        return halfpix.Clip(imgs, layout, value_range)

    @torch.no_grad()
    def embed_half(self, imgs: torch.Tensor, msgs: torch.Tensor = None, is_video: bool = True, value_range: str = "unit", layout: str = "nchw",
                   interpolation: dict = None, lowres_attenuation: bool = True) -> dict:
        """imgs: a float16 or bfloat16 clip (halfpix.py): layout "nchw" [F, 3, H, W], planar or channels-last memory, or "nhwc" [F, H, W, 3 | 4]
        (the fourth component is alpha); value_range "unit" (values in [0, 1]) or "signed" ([-1, 1], as a VAE decoder leaves them); any row
        pitch and frame stride -> {'imgs_w': a compact clip of the same dtype, shape and memory form, 'msgs'}.  Means: halfpix.from_rgb(embed(
        halfpix.to_rgb(imgs), msgs, is_video=..., lowres_attenuation=...)['imgs_w'], like=imgs), bit for bit, with both conversions fused into
        the resize and tail kernels: no fp32 frame is written; alpha of the result is the clip's, bit for bit.  is_video=False is image mode:
        a message row per frame (msgs [F, k], or random), the embedder on every frame, no 'preds_w'.  Needs clamp=True."""
        clip = self._half_clip(imgs, "embed_half", value_range, layout)
        if is_video:
            out, msgs = self._embed_yuv(clip, "embed_half", msgs, interpolation, lowres_attenuation)
            return {"imgs_w": out.tensor, "msgs": msgs}
        if not self.clamp:
            raise NotImplementedError("embed_half needs clamp=True (words are undefined outside the value range)")
        F_ = clip.shape[0]
        if msgs is None:
            msgs = self.get_random_msg(F_)
        elif msgs.shape[0] != F_:
            raise ValueError(f"msgs has {msgs.shape[0]} rows for {F_} images")
        if F_ == 0 or clip.numel() == 0:
            return {"imgs_w": clip.clone().tensor, "msgs": msgs}
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        with torch.cuda.device(eng.dev):
            mi = self._msgs_dev(msgs, eng.dev)
            out = self._run_chunks(eng, clip, max(1, int(getattr(self, "chunk_size", 32))),
                                   lambda fr, oc, a, b: self._embed_frames(eng, fr, mi[a:b], oc, step=1, video_mode=0, antialias=aa,
                                                                           lowres=lowres_attenuation))
        return {"imgs_w": out.tensor, "msgs": msgs}

    @torch.no_grad()
    def detect_half(self, imgs: torch.Tensor, is_video: bool = True, value_range: str = "unit", layout: str = "nchw",
                    interpolation: dict = None) -> dict:
        """imgs, value_range, layout as in embed_half -> {'preds': [F, 1+nbits]}: detect(halfpix.to_rgb(imgs), is_video=...)['preds'] with the
        conversion fused into the resize kernel.  As for fp32 frames, is_video=True walks the clip in chunks of chunk_size frames and
        is_video=False sends all frames through the extractor in one pass."""
        clip = self._half_clip(imgs, "detect_half", value_range, layout)
        if is_video or clip.shape[0] == 0:
            return self._detect_yuv(clip, "detect_half", interpolation)
        self._per_frame_rows_only("detect_half")
        eng = self._engine()
        aa = _antialias_flag(interpolation)
        with torch.cuda.device(eng.dev):
            fr = clip if clip.device == eng.dev else clip.to(eng.dev)
            return {"preds": self._detect_frames(eng, fr, (self.img_size, self.img_size), aa).to(clip.device)}

    def extract_message(self, imgs: torch.Tensor, aggregation: str = "avg",
                        interpolation: dict = {"mode": "bilinear", "align_corners": False, "antialias": False}) -> torch.Tensor:
        """videoseal.py:390-428."""
        preds = self.detect(imgs, is_video=True, interpolation=interpolation)["preds"]
        bit_preds = preds[:, 1:]
        decoded = aggregate_bits(bit_preds, aggregation)
        return (decoded > 0).squeeze().unsqueeze(0)

    def forward(self, imgs: torch.Tensor, masks: torch.Tensor, msgs: torch.Tensor = None, is_video: bool = True):
        """videoseal.py:120-161 (differentiable, see Wam.forward)."""
        assert not (is_video and len(imgs.shape) not in [4, 5]), \
            "If is_video is True, input shape should be [b, frames, c, h, w] or [frames, c, h, w]"
        assert not (not is_video and len(imgs.shape) != 4), "If is_video is False, input shape should be [b, c, h, w]"
        if not is_video:
            return super().forward(imgs, masks, msgs)
        if imgs.dim() == 5:
            return [self.video_forward(imgs[i], masks[i] if masks is not None else None, msgs[i] if msgs is not None else None)
                    for i in range(imgs.shape[0])]
        return self.video_forward(imgs, masks, msgs)

    def video_forward(self, imgs, masks, msgs=None, interpolation: dict = None) -> dict:
        """videoseal.py:163-256: the whole clip as one chunk, key frames every step_size, video_mode expansion, attenuation at low
        resolution (self.lowres_attenuation) or as attenuation(imgs, imgs_w) at full resolution, clamp, augment, resize, detect."""
        if msgs is None:
            msgs = self.get_random_msg()
        else:
            assert msgs.shape[0] == 1, "Message should be unique"
        msgs = msgs.to(imgs.device)
        if self.video_mode not in N.VIDEO_MODES:
            raise ValueError(f"unknown video_mode {self.video_mode}")
        eng = self._engine()
        aa = _antialias_flag(_DEFAULT_INTERP if interpolation is None else interpolation)
        back = imgs.device
        emb_t, det_t = self._trainable()
        with torch.cuda.device(eng.dev), torch.set_grad_enabled(emb_t or det_t):
            x = N.f32c(imgs.detach().to(eng.dev))
            if emb_t or det_t:
                out, _, imgs_aug, masks, selected, preds = self._forward_graph(
                    x, masks, self._msgs_dev(msgs, eng.dev), step=int(self.step_size), video_mode=N.VIDEO_MODES[self.video_mode], aa=aa,
                    lowres=bool(self.lowres_attenuation), is_video=True, emb_train=emb_t)
            else:
                out = torch.empty_like(x)
                self._embed_frames(eng, x, self._msgs_dev(msgs, eng.dev), out, step=int(self.step_size),
                                   video_mode=N.VIDEO_MODES[self.video_mode], antialias=aa, lowres=bool(self.lowres_attenuation), fwd_order=True)
                imgs_aug, masks, selected, preds = self._augment_detect(eng, out, x, masks, True, aa)
        to = (lambda t: (t.to(back) if torch.is_tensor(t) else t) if (emb_t or det_t) else _to_caller(t, back))     # noqa: E731
        return {"msgs": msgs.expand(imgs.shape[0], -1), "masks": to(masks), "imgs_w": to(out), "imgs_aug": to(imgs_aug), "preds": to(preds),
                "selected_aug": selected}


def aggregate_bits(bit_preds: torch.Tensor, aggregation: Optional[str]) -> torch.Tensor:
    """Frame aggregation of videoseal.py:411-426 (tiny [F,k] reduction, plain torch on the caller's device)."""
    if aggregation is None:
        return bit_preds
    if aggregation == "avg":
        return bit_preds.mean(dim=0)
    if aggregation == "squared_avg":
        return (bit_preds * bit_preds.abs()).mean(dim=0)
    if aggregation == "l1norm_avg":
        return (bit_preds * torch.norm(bit_preds, p=1, dim=1).unsqueeze(1)).mean(dim=0)
    if aggregation == "l2norm_avg":
        return (bit_preds * torch.norm(bit_preds, p=2, dim=1).unsqueeze(1)).mean(dim=0)
    raise ValueError(f"unknown aggregation {aggregation}")


def build_model(cfg: ModelCfg, seed: int = 0) -> Videoseal:
    """cfg.py:120-144: embedder + extractor + identity augmenter + JND -> Videoseal (train mode, CPU, like the reference)."""
    return Videoseal(Embedder(cfg, seed), Extractor(cfg, seed), get_dummy_augmenter(),
                     attenuation=(JND(in_channels=cfg.jnd_in, out_channels=cfg.jnd_out) if cfg.jnd_in > 0 else None), scaling_w=cfg.scaling_w,
                     scaling_i=cfg.scaling_i, img_size=cfg.img_size, chunk_size=cfg.chunk_size, step_size=cfg.step_size,
                     blending_method=cfg.blending_method)
