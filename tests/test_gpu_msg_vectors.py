"""The U-Net with the message channels as per-frame vectors (engine.py::resblock_msg0_vec, model_api.hip: res_conv of the first bottleneck block
and the first Upsample GEMM take their message part as one bias vector per frame; no broadcast, no 384-wide planes, K = 128 / 512 instead of
384 / 768) against the tensor path the switch VIDEOSEAL_MSG_VECTORS=0 keeps.

VideoSeal 1.0 architecture, seeded weights, 256 x 256 key frames: 16 frames with 16 distinct messages and with one shared message (the smallest
batch that passes _msg0_ok; its planes convs take two K slices: 128 tiles, so bias2 travels through the K-slice epilogue), and a 4-frame call,
which fails _msg0_ok (32 tiles of 8 x 16 pixels) and must keep the tensor path whatever the switch says.  Both paths are measured
against a float64 evaluation of the reference U-Net (oracle/videoseal_ref.py on float64 tensors).  The bound: both paths add the same products,
the vector path sums the 256 message terms of an output separately and adds them as a bias -- another association of the same fp32 sum, with
the same worst-case bound, so its error may not exceed the tensor path's by more than the factor two that separates two orders of one sum
(MARGIN, with the 2^-24 floor of tests/_envelope.py).  Every figure is printed before anything is asserted (profiles/msg_vectors_envelope.txt).

The model-level C host has no switch of its own (the library's key table is closed: its last key is pinned by tests/test_switches_cpu.py): it
takes the vector path wherever the engine does by default and must agree with the engine's vector path like every other case of
tests/test_gpu_e2e.py (1e-6: same kernels, tuned against static tiles) -- at 32 frames on the planes chain, at 16 on the per-conv route (its planes
chain has no K-sliced form) -- and differ from the engine's tensor path, which shows that it left it."""
import ctypes as C
import os

import pytest
import torch

from oracle import videoseal_ref as R
from oracle.inputs import synthetic_frames, synthetic_msgs
from oracle.weights import make_state_dict, spec_from_card
from tests._envelope import check_rows, frame_err
from tests._model import cfg_of, make_model
from videoseal_amd import native as N

pytestmark = pytest.mark.gpu

CARDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videoseal_amd", "cards")
MARGIN = 2.0


@pytest.fixture(scope="module")
def vs10():
    spec = spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml"))
    sd = make_state_dict(spec, seed=0)
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    return spec, sd, sd64, make_model(spec, sd)


def _y01(spec, n, seed):
    imgs = synthetic_frames(n, spec.img_size, spec.img_size, seed=seed)
    return (0.299 * imgs[:, 0:1] + 0.587 * imgs[:, 1:2] + 0.114 * imgs[:, 2:3]).contiguous()


def _engine_delta(model, spec, y01, msgs, vectors):
    from videoseal_amd.model import _msgs_i32
    eng = model._engine()
    n, S = y01.shape[0], spec.img_size
    xd = y01.cuda()
    key = eng.new_act("t.msgv.in", n, S, S, spec.in_ch, 4)
    ymat = (C.c_float * 3)(1.0, 0.0, 0.0)
    N.check(eng.lib.vs_resize_pre(N.ptr(xd), n, 1, S, S, S, S, 0, None, 1.0, 0.0, N.ptr(key.t), 1, ymat, N.stream()), "vs_resize_pre")
    eng.msg_vectors = vectors
    try:
        delta = eng.embedder_forward(key, _msgs_i32(msgs, eng.dev)).clone()
        torch.cuda.synchronize()
    finally:
        eng.msg_vectors = True
    return delta.cpu()


@pytest.mark.parametrize("n,bm", [(16, 16), (16, 1), (4, 4)], ids=["16-frames-16-msgs", "16-frames-1-msg", "4-frames-fall-back"])
def test_vector_path_stays_inside_the_tensor_paths_envelope(vs10, n, bm):
    spec, sd, sd64, model = vs10
    assert spec.in_ch == 1 and spec.yuv
    y01 = _y01(spec, n, seed=70 + n + bm)
    msgs = synthetic_msgs(bm, spec.nbits, seed=70 + n + bm)
    eng = model._engine()
    E_ok = lambda: eng._msg_vectors_ok(n, spec.img_size // 8, spec.img_size // 8, eng.E, False)
    # eval mode: frames are independent, so the float64 reference is evaluated on four of them (it is what the test's time goes to)
    pick = list(range(0, n, max(1, n // 4)))[:4]
    ref = R.embedder_forward(sd64, spec, y01[pick].double(), (msgs.expand(n, -1) if bm == 1 else msgs)[pick])
    tensor = _engine_delta(model, spec, y01, msgs, vectors=False)
    vector = _engine_delta(model, spec, y01, msgs, vectors=True)
    assert E_ok() == (n >= 16), "which shapes take the vector path changed: the cases of this test must follow"
    if n >= 16:
        assert "msgv" in eng.E and not torch.equal(tensor, vector)
    else:
        assert torch.equal(tensor, vector)          # fall-back: the tensor path, unchanged
    again = _engine_delta(model, spec, y01, msgs, vectors=True)
    assert torch.equal(again, vector)
    e_t, e_v = frame_err(tensor[pick], ref), frame_err(vector[pick], ref)
    print(f"MSG-VECTORS {n} frames {bm} msgs: vector vs tensor path max |diff| {float((vector - tensor).abs().max()):.3e}")
    check_rows("MSG-VECTORS", 24, "tensor-path", MARGIN, f"{n} frames {bm} msgs", [("delta", e_v, e_t)])


@pytest.mark.parametrize("n", [32, 16], ids=["32-frames-planes", "16-frames-per-conv"])
def test_model_level_c_host_takes_the_vector_path(vs10, n):
    from videoseal_amd.capi import CModel
    spec, sd, sd64, model = vs10
    cm = CModel(cfg_of(spec), sd)
    S = spec.img_size
    imgs = synthetic_frames(n, S, S, seed=91).cuda()
    msgs = synthetic_msgs(n, spec.nbits, seed=91)
    eng = model._engine()
    py = {}
    for vectors in (True, False):
        eng.msg_vectors = vectors
        try:
            py[vectors] = model.embed(imgs, msgs, is_video=False)["imgs_w"].clone()
        finally:
            eng.msg_vectors = True
    got = cm.embed(imgs, msgs, step=1)
    torch.cuda.synchronize()
    d_v, d_t = float((got - py[True]).abs().max()), float((got - py[False]).abs().max())
    print(f"MSG-VECTORS C host, {n} frames: max |diff| against the engine's vector path {d_v:.3e}, against its tensor path {d_t:.3e}")
    assert d_v < 1e-6
    if n == 32:                     # (same route and tiles on both hosts: the C host is bit-equal to the vector path, hence not to the tensor path)
        assert d_v == 0.0 and d_t > 0.0, "the C host did not leave the tensor path"
    # one message for every frame: frame stride 0
    m1 = synthetic_msgs(1, spec.nbits, seed=92)
    model.chunk_size, model.step_size, model.video_mode = n, 1, "repeat"
    p1 = model.embed(imgs, m1, is_video=True)["imgs_w"]
    assert float((cm.embed(imgs, m1, step=1) - p1).abs().max()) < 1e-6
