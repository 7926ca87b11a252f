"""SSIM / MS-SSIM: the torch restatement of videoseal_amd/metrics.py against the unmodified losses/ssim.py of the reference
(tests/golden/make_golden_ssim.py -> tests/golden/ssim_loss.npz), and the perceptual-loss grammar of losses/perceptual.py:84-113.  No GPU."""
import numpy as np
import pytest
import torch

from tests._cases import check_inputs, make_inputs
from tests._util import load_golden
from videoseal_amd import autograd as AG
from videoseal_amd import metrics as M


@pytest.fixture(scope="module")
def golden():
    return load_golden("ssim_loss")


def test_metrics_equal_the_reference_in_float64(golden):
    for cname, info in golden["meta"]["cases"].items():
        x, y = make_inputs(info)
        check_inputs(golden, cname, x, y)
        got = M.ssim(x.double(), y.double()).numpy()
        assert M.LAST_SSIM_BACKEND == "torch"
        assert np.abs(got - golden[f"{cname}.ssim_img"]).max() <= 1e-12
        if min(info["H"], info["W"]) > 160:
            assert np.abs(M.msssim(x.double(), y.double()).numpy() - golden[f"{cname}.msssim_img"]).max() <= 1e-12
        # the per-plane statistics the HIP kernel is compared with are those of metrics._ssim_cs
        s, c = M._ssim_cs(x.double(), y.double(), 1.0, M._gauss_window(11, 1.5, x.double()))
        assert np.abs(torch.stack([s, c]).numpy() - golden[f"{cname}.stats"][0]).max() <= 1e-12


GRAMMAR = [
    ("mse", (None, ["mse"])), ("ssim", (None, ["ssim"])), ("msssim", (None, ["msssim"])), ("jnd", (None, ["jnd"])), ("none", (None, ["none"])),
    ("jnd2", (None, ["jnd2"])),                                      # constructs in the reference, fails in its forward
    ("mse+ssim", ([1.0, 1.0], ["mse", "ssim"])), ("mse+0.1_ssim", ([1.0, 0.1], ["mse", "ssim"])),
    ("yuv+0.5_msssim+0.1_jnd", ([1.0, 0.5, 0.1], ["yuv", "msssim", "jnd"])), ("2_mse+mse", ([2.0, 1.0], ["mse", "mse"])),
    ("0.5_ssim", ValueError),                                         # no weight syntax on a single term
    ("psnr", ValueError), ("mse+psnr", ValueError), ("mse+x_ssim", ValueError), ("mse+0.1_0.2_ssim", ValueError), ("", ValueError),
    ("mse+x_lpips", ValueError),                                      # the weight is rejected there before anything is evaluated
    ("mse+watson_vgg", ValueError),                                  # 'watson_vgg' splits at its own underscore there too
    ("lpips", NotImplementedError), ("dists", NotImplementedError), ("watson_vgg", NotImplementedError), ("watson_dft", NotImplementedError),
    ("focal", NotImplementedError), ("mse+0.1_lpips", NotImplementedError), ("mse+focal", NotImplementedError),
]


@pytest.mark.parametrize("string,want", GRAMMAR)
def test_percep_loss_grammar(string, want):
    if isinstance(want, type):
        with pytest.raises(want):
            AG.parse_percep_loss(string)
    else:
        assert AG.parse_percep_loss(string) == want


def test_messages_say_why_a_term_is_missing():
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="weight file"):
        AG.percep_loss(x, x, "lpips")
    with pytest.raises(NotImplementedError, match="FFT"):
        AG.percep_loss(x, x, "focal")
    with pytest.raises(ValueError, match="not supported"):
        AG.percep_loss(x, x, "jnd2")
    with pytest.raises(ValueError):
        AG.percep_loss(x, x, "0.5_ssim")
    from videoseal_amd.training import GeneratorStep
    for ok in ("ssim", "msssim", "mse+0.1_ssim", "yuv+0.5_msssim+0.1_jnd"):
        GeneratorStep(None, percep_loss=ok)
    with pytest.raises(NotImplementedError, match="weight file"):
        GeneratorStep(None, percep_loss="mse+0.1_lpips")
