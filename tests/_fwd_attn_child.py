"""Child process of tests/test_gpu_fwd_envelope.py: runs vs_vit_attention on the hard qkv of every ATTN_MFMA_CASES entry under the VS_VIT_ATTN
setting of its environment (the library reads it once per process) and saves the outputs, in that order, to the path given."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import _fwd_ref as R  # noqa: E402
from tests._gpu import attention_launch  # noqa: E402

if __name__ == "__main__":
    torch.save([attention_launch(c) for c in R.ATTN_MFMA_CASES], sys.argv[1])
