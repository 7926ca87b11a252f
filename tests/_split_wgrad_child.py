"""Child process of tests/test_gpu_split_envelope.py: runs vs_gemm_wgrad on the hard operands of every WGRAD_GEMM_CASES entry under the VS_WGRAD
setting of its environment (the library reads it once per process) and saves [(dw, dw of a second launch), ...] to the path given."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import _split_ref as R  # noqa: E402
from tests._gpu import wgrad_gemm_launch  # noqa: E402

if __name__ == "__main__":
    torch.save([wgrad_gemm_launch(c) for c in R.WGRAD_GEMM_CASES], sys.argv[1])
