"""vs_conv_desc_t::bias_fs / bias2_fs: one bias vector per frame -- what spatially constant input channels contribute to a pointwise
conv -- in the kernels that implement it, through vs_conv_gemm: the planes 3x3 kernel's own epilogue (bias2 behind the activation, in front of
the 1x1 second phase) and its K-sliced form (splitk_epilogue), the wave-specialised 3x3 kernel likewise, the generic GEMM kernel on every tile, the wave-specialised 1x1 GEMM with and
without K slices.  Expected values: a float64 host convolution; the bound is the 2e-5 of the output range every conv test of the split
arithmetic uses (tests/test_gpu_kernels.py).  Stride 0 is the shared vector bit for bit; kernels without the per-frame form refuse it."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests._gpu import DEV, Eng, conv_weights, dv, from_nhwc, rel_err, to_nhwc
from tests._guards import _guarded, _guards_intact
from videoseal_amd import native as N
from videoseal_amd.engine import Act

pytestmark = pytest.mark.gpu
HI = N.CONV_TILE_HI


def _guarded_out(eng, B, H, W, Co):
    buf, v = _guarded(torch.full((B, H, W, Co), 9.0, device=DEV), -7.0)
    return buf, Act(v, B, H, W, Co, Co)


def _frames(vec, pad, seed):
    """[F][n] vectors inside a row stride of n + pad floats, the gaps poisoned with NaN -> (device tensor [F][n + pad], stride)"""
    t = torch.full((vec.shape[0], vec.shape[1] + pad), float("nan"))
    t[:, : vec.shape[1]] = vec
    return dv(t), vec.shape[1] + pad


# ---------------------------------------------------------------------------------------------------------------- planes 3x3 + phase 2, bias2 per frame
@pytest.fixture(scope="module")
def planes_case():
    B, H, W, Cin, Co, Cin2 = 3, 16, 16, 32, 192, 16
    g = torch.Generator().manual_seed(11)
    x, x2 = torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cin2, H, W, generator=g)
    w1 = torch.randn(Co, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    w2 = torch.randn(Co, Cin2, 1, 1, generator=g) / math.sqrt(Cin2)
    b1, b2 = torch.randn(Co, generator=g) * 0.3, torch.randn(B, Co, generator=g)
    ref = (F.relu(F.conv2d(x.double(), w1.double(), b1.double(), padding=1)) + F.conv2d(x2.double(), w2.double()) + b2.double()[:, :, None, None])
    return dict(shape=(B, H, W, Cin, Co, Cin2), x=x, x2=x2, w1=w1, w2=w2, b1=b1, b2=b2, ref=ref)


def _planes_run(c, sk, bias2_frames=None, shared=None, planes=True):
    """planes: the all-DMA kernel on operand planes (tile 22), else the wave-specialised 3x3 kernel (tile 16) on the fp32 activations"""
    B, H, W, Cin, Co, Cin2 = c["shape"]
    eng = Eng(arith=2)
    xa, xa2 = to_nhwc(c["x"]), to_nhwc(c["x2"])
    cw1, cw2 = conv_weights(c["w1"], c["b1"], xa.ld), conv_weights(c["w2"], shared, xa2.ld)
    obuf, out = _guarded_out(eng, B, H, W, Co)
    kw = dict(tile_hint=HI | 6, arith=2, in_pl=eng.to_planes(xa, "fb.xpl"), in2_pl=eng.to_planes(xa2, "fb.x2pl")) if planes else dict(tile_hint=HI | 0)
    eng.conv(xa, cw1, out, pad=1, act=N.ACT_RELU, in2=xa2, w2=cw2, split_k=(sk if sk > 1 else None), bias2_frames=bias2_frames, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0), "damaged band around the output"
    return from_nhwc(out).clone()


@pytest.mark.parametrize("sk", [1, 2])
@pytest.mark.parametrize("planes", [True, False], ids=["planes-tile22", "wave-specialised-tile16"])
def test_conv3x3_with_second_phase_takes_bias2_per_frame(planes_case, planes, sk):
    c = planes_case
    got = _planes_run(c, sk, bias2_frames=_frames(c["b2"], 12, 1), planes=planes)
    e = rel_err(got.double(), c["ref"])
    print(f"FRAME-BIAS 3x3 + phase 2, {'planes' if planes else 'wave-specialised'} kernel, split_k {sk}: {e:.3e}")
    assert e < 2e-5
    # stride 0 = the shared vector, bit for bit
    v0 = c["b2"][0].contiguous()
    assert torch.equal(_planes_run(c, sk, bias2_frames=(dv(v0), 0), planes=planes), _planes_run(c, sk, shared=v0, planes=planes))


def test_both_3x3_kernels_give_the_same_bits_with_bias2_per_frame(planes_case):
    """what keeps the planes chain bit-identical to the per-conv path (tests/test_gpu_e2e.py) with the message part as a per-frame bias2"""
    f = _frames(planes_case["b2"], 4, 1)
    assert torch.equal(_planes_run(planes_case, 1, bias2_frames=f, planes=True), _planes_run(planes_case, 1, bias2_frames=f, planes=False))


# ---------------------------------------------------------------------------------------------------------------- 1x1 GEMM, bias per frame
def _gemm_case(B, H, W, K, Co, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, H, W, generator=g)
    w = torch.randn(Co, K, 1, 1, generator=g) / math.sqrt(K)
    b = torch.randn(B, Co, generator=g)
    ref = F.conv2d(x.double(), w.double()) + b.double()[:, :, None, None]
    return x, w, b, ref


def _gemm_run(x, w, tile, sk=None, bias_frames=None, shared=None, act=N.ACT_NONE):
    B, K, H, W = x.shape
    eng = Eng(arith=2)
    xa = to_nhwc(x)
    cw = conv_weights(w, shared, xa.ld)
    obuf, out = _guarded_out(eng, B, H, W, w.shape[0])
    eng.conv(xa, cw, out, tile_hint=tile, split_k=sk, bias_frames=bias_frames, act=act)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0), "damaged band around the output"
    return from_nhwc(out).clone()


# frames of 16 rows (a 32-row accumulator block straddles frames): the generic kernel's tiles and the K-sliced wave-specialised GEMM;
# frames of 128 rows: the wave-specialised GEMM's own epilogue (one vector per 128-row tile)
GEMM_CASES = [((3, 4, 4, 32, 64), t, None) for t in (0, 1, 2, 3, 4, 5, 13, 14)] + [((3, 4, 4, 64, 64), HI | 1, 2)] + \
             [((3, 8, 16, 64, 192), t, None) for t in (0, 1, HI | 1, HI | 2)] + [((3, 8, 16, 64, 192), HI | 2, 2)]


@pytest.mark.parametrize("shape,tile,sk", GEMM_CASES, ids=[f"{'x'.join(map(str, s))}-tile{(t & 15) + (16 if t & HI else 0)}-sk{k or 1}" for s, t, k in GEMM_CASES])
def test_gemm_takes_bias_per_frame(shape, tile, sk):
    x, w, b, ref = _gemm_case(*shape, seed=sum(shape))
    got = _gemm_run(x, w, tile, sk, bias_frames=_frames(b, 8, 2))
    e = rel_err(got.double(), ref)
    print(f"FRAME-BIAS gemm {shape} tile {tile} split_k {sk}: {e:.3e}")
    assert e < 2e-5
    v0 = b[0].contiguous()
    assert torch.equal(_gemm_run(x, w, tile, sk, bias_frames=(dv(v0), 0), act=N.ACT_RELU), _gemm_run(x, w, tile, sk, shared=v0, act=N.ACT_RELU))


def test_kernels_without_the_per_frame_form_refuse_it(planes_case):
    """VS_ERR_UNSUPPORTED (not frame 0's vector for every row): the patch kernels, the planes GEMM, the planes 3x3 kernel for `bias` without K
    slices, the wave-specialised GEMM when a 128-row tile could straddle frames, the generic kernel for bias2; a stride below N is a bad argument"""
    c = planes_case
    with pytest.raises(N.NativeError, match="unsupported"):
        eng = Eng(arith=2)
        xa = to_nhwc(c["x"])
        obuf, out = _guarded_out(eng, 3, 16, 16, 192)
        eng.conv(xa, conv_weights(c["w1"], None, xa.ld), out, pad=1, tile_hint=HI | 6, arith=2, in_pl=eng.to_planes(xa, "fb.xpl"),
                 bias_frames=_frames(c["b2"], 0, 3))
    x, w, b, _ = _gemm_case(3, 4, 4, 64, 64, seed=5)
    for tile in (HI | 1, HI | 2):                          # 16-row frames, no K slices
        with pytest.raises(N.NativeError, match="unsupported"):
            _gemm_run(x, w, tile, bias_frames=_frames(b, 0, 4))
    eng = Eng(arith=2)
    xa = to_nhwc(x)
    obuf, out = _guarded_out(eng, 3, 4, 4, 64)
    with pytest.raises(N.NativeError, match="unsupported"):       # planes GEMM (tile 24)
        eng.conv(xa, conv_weights(w, None, xa.ld), out, tile_hint=HI | 8, arith=2, in_pl=eng.to_planes(xa, "fb.gpl"), bias_frames=_frames(b, 0, 5))
    with pytest.raises(N.NativeError, match="unsupported"):       # generic kernel: bias2 per frame
        eng.conv(xa, conv_weights(w, None, xa.ld), out, tile_hint=2, in2=xa, w2=conv_weights(w, None, xa.ld), bias2_frames=_frames(b, 0, 6))
    x3 = torch.randn(2, 16, 16, 16)
    w3 = torch.randn(32, 16, 3, 3) / 12
    xa3 = to_nhwc(x3)
    obuf3, out3 = _guarded_out(eng, 2, 16, 16, 32)
    for tile in (10, 11, HI | 4):                          # 3x3 patch kernels, the thin persistent kernel
        with pytest.raises(N.NativeError, match="unsupported"):
            eng.conv(xa3, conv_weights(w3, None, xa3.ld), out3, pad=1, tile_hint=tile, bias_frames=_frames(torch.randn(2, 32), 0, 7))
    with pytest.raises(N.NativeError, match="bad argument"):
        eng.conv(xa, conv_weights(w, None, xa.ld), out, tile_hint=2, bias_frames=(dv(b), 32))
    torch.cuda.synchronize()
    assert float(out.t.min()) == 9.0 and float(out3.t.min()) == 9.0 and _guards_intact(obuf, -7.0) and _guards_intact(obuf3, -7.0)
