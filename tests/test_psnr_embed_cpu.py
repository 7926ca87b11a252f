"""Embedding to a target PSNR on the CPU: the new entry points are listed, declared and built and refuse bad arguments on the host before any
launch; the strength formula against a hand-computed case; the argument checks of Videoseal.embed_psnr, which run before the model asks for a
device.  The library loads without a GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from oracle.weights import tiny_spec
from tests._model import cfg_of
from videoseal_amd import native as N
from videoseal_amd.model import build_model, check_psnr_args, psnr_strength

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_SYMBOLS = ("vs_embed_tail_energy", "vs_psnr_scale", "vs_embed_tail_scaled", "vs_model_embed_psnr")
I64_SYMBOLS = ("vs_tail_energy_partial_doubles", "vs_model_embed_psnr_workspace_bytes")


def test_the_symbols_are_listed_declared_and_built():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    lib = N.lib()
    for sym in INT_SYMBOLS:
        assert sym in N.EXPORTS and re.search(r"\bint " + sym + r"\(", header) and hasattr(lib, sym), sym
    for sym in I64_SYMBOLS:
        assert sym in N.EXPORTS and re.search(r"\bint64_t " + sym + r"\(", header) and hasattr(lib, sym), sym
    # vs_tail_desc_t stays what it was: the ctypes mirror is checked against the library when it loads
    assert lib.vs_sizeof_tail_desc() == C.sizeof(N.TailDesc) == 112


def test_bad_arguments_are_refused_on_the_host():
    lib = N.lib()
    d = N.TailDesc()
    one = C.c_void_p(256)                                          # a non-null address nothing ever follows: every call below stops before a launch
    assert lib.vs_embed_tail_energy(None, one, one, None) == -1
    assert lib.vs_embed_tail_energy(C.byref(d), None, one, None) == -1
    assert lib.vs_embed_tail_energy(C.byref(d), one, None, None) == -1
    assert lib.vs_embed_tail_energy(C.byref(d), one, one, None) == -1          # an empty descriptor: F = 0, no frames
    assert lib.vs_embed_tail_scaled(None, one, None) == -1
    assert lib.vs_embed_tail_scaled(C.byref(d), None, None) == -1
    assert lib.vs_embed_tail_scaled(C.byref(d), one, None) == -1
    assert lib.vs_psnr_scale(None, 1, 8, 8, 0, 42.0, 0.0, one, None) == -1
    assert lib.vs_psnr_scale(one, 1, 8, 8, 0, 42.0, 0.0, None, None) == -1
    assert lib.vs_psnr_scale(one, 0, 8, 8, 0, 42.0, 0.0, one, None) == -1
    assert lib.vs_psnr_scale(one, -3, 8, 8, 0, 42.0, 0.0, one, None) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.vs_psnr_scale(one, 1, 8, 8, 0, bad, 0.0, one, None) == -1
    assert lib.vs_tail_energy_partial_doubles(0, 8, 8) == -1 and lib.vs_tail_energy_partial_doubles(1, 0, 8) == -1
    # room for every form: 256-column tiles, strips of at least four rows
    assert lib.vs_tail_energy_partial_doubles(5, 37, 53) == 5 * 1 * 10
    assert lib.vs_tail_energy_partial_doubles(2, 40, 600) == 2 * 3 * 10
    assert lib.vs_model_embed_psnr_workspace_bytes(None, 1, 8, 8, 1) == -1


def test_strength_formula_by_hand():
    # a perturbation of 0.01 on each of n elements has rms 0.01 = -40 dB: at 40 dB the strength is 1, at 60 dB 0.1, at 20 dB 10
    n = 3 * 4 * 5
    e = n * 0.01 ** 2
    assert math.isclose(psnr_strength(e, n, 40.0), 1.0, rel_tol=1e-12)
    assert math.isclose(psnr_strength(e, n, 60.0), 0.1, rel_tol=1e-12)
    assert math.isclose(psnr_strength(e, n, 20.0), 10.0, rel_tol=1e-12)
    # E = 3, n = 12, T = 20 log10(2) dB: 0.5 * sqrt(4) = 1
    assert math.isclose(psnr_strength(3.0, 12, 20 * math.log10(2.0)), 1.0, rel_tol=1e-12)
    assert psnr_strength(0.0, n, 42.0) == 0.0
    assert psnr_strength(e, n, 20.0, max_scaling_w=2.5) == 2.5 and math.isclose(psnr_strength(e, n, 60.0, max_scaling_w=2.5), 0.1, rel_tol=1e-12)
    # the definition: scaling the perturbation by the strength gives the target PSNR
    x = torch.linspace(-0.03, 0.05, n, dtype=torch.float64)
    s = psnr_strength(float((x * x).sum()), n, 37.5)
    assert math.isclose(-10 * math.log10(float(((s * x) ** 2).mean())), 37.5, rel_tol=1e-12)


def test_argument_checks():
    for bad in (float("nan"), float("inf"), 0, -42.0, "42", None, True):
        with pytest.raises(ValueError, match="target_psnr"):
            check_psnr_args(bad, "frame", None)
    with pytest.raises(ValueError, match="per must be"):
        check_psnr_args(42.0, "chunk", None)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2", [2.0], True, torch.ones(2)):
        with pytest.raises(ValueError, match="max_scaling_w"):
            check_psnr_args(42.0, "clip", bad)
    for bad in ("42", None, True, [42.0], torch.ones(2)):                  # the message names the cause, not a range
        with pytest.raises(ValueError, match="target_psnr must be a number"):
            check_psnr_args(bad, "frame", None)
    check_psnr_args(42, "frame", None)
    check_psnr_args(36.5, "clip", 2.0)
    # numpy scalars and 0-dim tensors are numbers
    import numpy as np
    check_psnr_args(np.float32(42.0), "frame", np.float64(2.0))
    check_psnr_args(torch.tensor(42.0), "clip", torch.tensor(2.5, dtype=torch.float64))
    check_psnr_args(np.int64(40), "frame", None)
    with pytest.raises(ValueError, match="finite and positive"):
        check_psnr_args(np.float32("nan"), "frame", None)


def test_embed_psnr_refuses_before_it_needs_a_device():
    model = build_model(cfg_of(tiny_spec())).eval()
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(ValueError, match="target_psnr"):
        model.embed_psnr(x, float("nan"))
    with pytest.raises(ValueError, match="target_psnr"):
        model.embed_psnr(x, -3.0)
    with pytest.raises(ValueError, match="per must be"):
        model.embed_psnr(x, 42.0, per="chunk")
    with pytest.raises(ValueError, match="max_scaling_w"):
        model.embed_psnr(x, 42.0, max_scaling_w=-1.0)
    with pytest.raises(ValueError, match="fp32 frames"):
        model.embed_psnr(x.double(), 42.0)
    with pytest.raises(ValueError, match="fp32 frames"):
        model.embed_psnr(torch.zeros(2, 16, 16, 4, dtype=torch.uint8), 42.0)
    with pytest.raises(ValueError, match="one message"):
        model.embed_psnr(x, 42.0, msgs=torch.zeros(2, model.embedder.cfg.nbits))
    model.clamp = False
    with pytest.raises(ValueError, match="clamp"):
        model.embed_psnr(torch.zeros(2, 16, 16, 3, dtype=torch.uint8), 42.0)
    # the signatures of embed and embed_u8 stay what they were
    import inspect
    assert list(inspect.signature(model.embed).parameters) == ["imgs", "msgs", "is_video", "interpolation", "lowres_attenuation"]
    assert list(inspect.signature(model.embed_u8).parameters) == ["clip", "msgs", "interpolation", "lowres_attenuation"]
    assert list(inspect.signature(model.embed_psnr).parameters) == ["imgs", "target_psnr", "msgs", "is_video", "per", "max_scaling_w", "interpolation",
                                                                    "lowres_attenuation"]
