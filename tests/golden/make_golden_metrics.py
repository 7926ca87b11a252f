"""Fixture for tests/test_host.py::test_mask_and_message_metrics_equal_the_reference_functions: the seeded inputs and what the UNMODIFIED
evals/metrics.py of a reference checkout returns for them (accuracy, iou, linf, psnr, bit_accuracy(+_1msg, masked), pvalue, capacity),
stored as tests/golden/reference_metrics.npz.

    VIDEOSEAL_REFERENCE_ROOT=/path/to/facebookresearch-videoseal python tests/golden/make_golden_metrics.py

The checkout's file is executed on its own; its `pytorch_msssim` import gets an empty stand-in module when the package is absent (none of
the functions recorded here touches it)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def metric_inputs():
    """the seeded inputs, incl. an empty mask / empty union (row 3), a perfect logit row (p log p at 0) and a mask shared by all rows"""
    g = torch.Generator().manual_seed(5)
    x = {}
    x["preds"] = torch.randn(5, 1, 12, 9, generator=g)
    x["targets"] = (torch.rand(5, 1, 12, 9, generator=g) > 0.6).float()
    x["targets"][3] = 0
    x["preds"][3] = -1.0
    x["a"], x["b"] = torch.rand(2, 3, 20, 20, generator=g), torch.rand(2, 3, 20, 20, generator=g)
    x["bits"] = torch.randint(0, 2, (4, 32), generator=g)
    x["logits"] = (x["bits"].float() * 2 - 1) * torch.rand(4, 32, generator=g) + 0.4 * torch.randn(4, 32, generator=g)
    x["logits"][1] = x["bits"][1].float() * 2 - 1
    x["pix"] = torch.randn(3, 8, 6, 6, generator=g)
    x["tb"] = torch.randint(0, 2, (3, 8), generator=g)
    x["mask"] = (torch.rand(3, 1, 6, 6, generator=g) > 0.5).float()
    x["mask"][:] = x["mask"][0]                  # (masked_select + view needs equal counts, as in the reference)
    return x


def metric_outputs(M, x):
    """{name: tensor} of the metrics module `M` on the inputs `x`"""
    out = {}
    for thr in (0.0, 0.3):
        out[f"accuracy_thr{thr}"] = M.accuracy(x["preds"], x["targets"], thr)
        for label in (0, 1):
            out[f"iou_thr{thr}_label{label}"] = M.iou(x["preds"].clone(), x["targets"], thr, label)
    out["linf"] = M.linf(x["a"], x["b"])
    out["psnr"] = M.psnr(x["a"], x["b"])
    out["psnr_is_video"] = M.psnr(x["a"], x["b"], True)
    out["bit_accuracy"] = M.bit_accuracy(x["logits"], x["bits"])
    out["pvalue"] = M.pvalue(x["logits"], x["bits"])
    out["capacity"] = M.capacity(x["logits"], x["bits"])
    out["bit_accuracy_masked"] = M.bit_accuracy(x["pix"], x["tb"], x["mask"])
    out["bit_accuracy_1msg"] = M.bit_accuracy_1msg(x["pix"], x["tb"])
    out["bit_accuracy_1msg_masked"] = M.bit_accuracy_1msg(x["pix"], x["tb"], x["mask"])
    return out


def main():
    path = os.path.join(os.environ["VIDEOSEAL_REFERENCE_ROOT"], "videoseal", "evals", "metrics.py")
    if "pytorch_msssim" not in sys.modules and importlib.util.find_spec("pytorch_msssim") is None:
        sys.modules["pytorch_msssim"] = types.ModuleType("pytorch_msssim")
    spec = importlib.util.spec_from_file_location("_reference_metrics", path)
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    x = metric_inputs()
    out = metric_outputs(R, x)
    np.savez(os.path.join(HERE, "reference_metrics.npz"), **{"in_" + k: v.numpy() for k, v in x.items()},
             **{"out_" + k: torch.as_tensor(v).numpy() for k, v in out.items()})
    print({k: (tuple(torch.as_tensor(v).shape), str(torch.as_tensor(v).dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
