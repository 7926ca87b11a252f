"""Environment switches of the Python side: one registry, and the only file of the package that touches os.environ.

Every reader refuses a name that is not registered here, and reads the environment at the moment it is called -- nothing is cached, so a
variable set before an engine / model is constructed (tests, bench.py) is seen by it.  The switches of the library itself (kernel forms,
strip heights) are the table in csrc/vs_common.h; INTEGRATION.md lists both.
"""
from __future__ import annotations

import os
from typing import Mapping, Optional, Sequence

REGISTRY = {
    # ---- arithmetic (engine construction)
    "VIDEOSEAL_CONV": "arithmetic of the dense layers: auto (default: 2 x f16 split with an always-on range guard that switches a network "
                      "whose activations leave the f16 range to 3 x bf16 and repeats the pass), f16x2 (no guard: NaN frames on overflow), "
                      "bf16x3 (exact split), f32 (v_mfma_f32_32x32x2_f32); the library reads f16x2 / bf16x3 as its own default too",
    "VIDEOSEAL_LAYER_ARITH": "0: the range guard switches the whole network; default: only the extractor layers whose operand leaves the f16 "
                             "range (one calibration pass, vs_absmax, 4 x margin) stay on 3 x bf16",
    "VIDEOSEAL_CHECK_FINITE": "1: synchronise after every network pass and raise if the output is not finite",
    # ---- launch sequences of the engine (engine construction; A/B handles, every form computes the same network)
    "VIDEOSEAL_UPCONV": "Upsample groups: lowres (default: low-resolution 9-tap GEMM + gather, fused into one kernel on the thin levels), "
                        "unfused (GEMM and gather as two launches everywhere), direct (the literal bilinear x2 -> reflect-pad conv3x3 -> LayerNorm)",
    "VIDEOSEAL_MSG_TABLE": "0: first bottleneck block without the message-channel table",
    "VIDEOSEAL_PLANES": "0: neither the bottleneck chain nor the ConvNeXt 1x1 GEMMs on pre-split operand planes",
    "VIDEOSEAL_MSG0_PLANES": "0: the chain's first block off the operand planes",
    "VIDEOSEAL_GEMM_BIG": "1: planes GEMMs of >= 3 rounds on 256 x 256 tiles, one wave per SIMD",
    "VIDEOSEAL_STEM_FUSED": "1: stem conv + LayerNorm in one vector-ALU kernel (measured neutral: opt-in; the library's model-level host reads it too)",
    "VIDEOSEAL_DOWN_PATCH": "0: down-samplers without the LayerNorm -> patch matrix -> dense GEMM route",
    "VIDEOSEAL_GRN_STRADDLE": "0: no GRN statistics from the planes GEMM's epilogue for HW % 32 != 0",
    "VIDEOSEAL_GRN_FOLD": "0: GRN finish as its own launch instead of inside the wave-specialised pwconv2 GEMM",
    "VIDEOSEAL_PW2_NARROW": "0: stage-2 pwconv2 in the K-slice form instead of 128 x 96 tiles (tile 26)",
    "VIDEOSEAL_PW2_SMALL_PC": "0: stage-3 pwconv2 on planes instead of the wave-specialised GEMM",
    "VIDEOSEAL_CNX_FUSED": "0: stage 0 / 1 ConvNeXt blocks unfused (default: h kept on chip, convnext_fused.hip)",
    "VIDEOSEAL_THIN_FUSED": "0: 16-channel ResnetBlocks as separate launches (default: one launch, resblock_thin.hip)",
    "VIDEOSEAL_MSG_VECTORS": "0: the message channels as a broadcast tensor ([latent | message] map, K = 384 res_conv, K = 768 first Upsample GEMM) "
                             "instead of per-frame bias vectors (the model-level C host has no such switch)",
    "VIDEOSEAL_OUTC_FUSED": "0: outc + tanh as its own launch behind the last thin ResnetBlock (default: in that block's epilogue, same bits)",
    "VIDEOSEAL_PLANES_SPLITK": "0: planes chain without K slices for 4 - 8 key frames",
    "VIDEOSEAL_PLANES_SK": "experiments: another K-slice count of the planes conv for launches below 200 tiles (read per call)",
    # ---- tile selection (engine construction)
    "VIDEOSEAL_AUTOTUNE": "0: static tile heuristic; default: per-shape timing of the candidate tiles (all bit-identical: only speed changes)",
    "VIDEOSEAL_TUNED_TILES": "0: ignore the packaged tile choices for the benchmark shapes (tools/tune_tiles.py)",
    "VIDEOSEAL_TILE_CACHE": "path of an on-disk copy of the tile choices: a profiled run then has no tuning launches",
    # ---- model / training / streaming / augmentation
    "VIDEOSEAL_GRAPHS": "1: replay the network passes as captured graphs (model construction)",
    "VIDEOSEAL_PINNED_RESULTS": "0: detect() results through pageable instead of pinned host memory (import)",
    "VIDEOSEAL_SYNC_BN": "anything but auto: per-rank BatchNorm statistics although a process group with several ranks exists (per call)",
    "VIDEOSEAL_DIRECT_WGRAD": "0: 3x3 weight gradients through the explicit patch matrix (import)",
    "VIDEOSEAL_STREAM_FINE": "0: streaming hands whole groups from embed to detect instead of overlapping inside a group (per call)",
    "VIDEOSEAL_AUG_FUSE": "0: Sequential runs consecutive Crop / Resize / colour ops one by one instead of in fused passes (import)",
    "VIDEOSEAL_CODEC": "H264 augmentation: proxy (default: on-GPU transform-coding proxy) or pyav (the reference's CPU round trip; construction)",
    "VIDEOSEAL_LIB": "path of another build of the same ABI (same-box A/B of two source trees; import)",
}


def _text(name: str, env: Optional[Mapping[str, str]]) -> Optional[str]:
    if name not in REGISTRY:
        raise KeyError(f"{name} is not a registered switch (videoseal_amd/switches.py)")
    return (os.environ if env is None else env).get(name)


def flag(name: str, default: bool, env: Optional[Mapping[str, str]] = None, off: str = "0") -> bool:
    """default True: on unless the variable says `off`; default False: on only if it says 1"""
    v = _text(name, env)
    return v != off if default else v == "1"


def choice(name: str, default: str, allowed: Optional[Sequence[str]] = None, env: Optional[Mapping[str, str]] = None) -> str:
    v = _text(name, env)
    v = default if v is None else v
    if allowed is not None and v not in allowed:
        raise ValueError(f"{name}={v!r}: expected " + " or ".join(repr(a) for a in allowed))
    return v


def integer(name: str, default: int, env: Optional[Mapping[str, str]] = None) -> int:
    v = _text(name, env)
    return default if v is None else int(v)


def path(name: str, env: Optional[Mapping[str, str]] = None) -> Optional[str]:
    return _text(name, env) or None
