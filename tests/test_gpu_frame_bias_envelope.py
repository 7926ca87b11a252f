"""vs_conv_desc_t::bias_fs / bias2_fs -- one bias vector per frame -- in the split-envelope family (tests/_split_ref.py, SPLIT_MARGIN), on frames
whose row count is no power of two.  tests/test_gpu_frame_bias.py holds the same kernels to 2e-5 of the output range on randn operands with
frames of 16, 128 or 256 rows; the frame of a row is row / (Ho Wo), and a frame that does not divide a 32-row accumulator block or a 128-row
tile is where that arithmetic can go wrong:
    35-row frames (B = 3, 5 x 7): every 32-row block of the generic kernel straddles two frames at another offset (tiles 0-5, 13, 14), and the
        K-slice epilogue of the wave-specialised GEMM looks every row's frame up
    384-row frames (B = 3, 8 x 48): three whole 128-row tiles per frame, the wave-specialised GEMM's own epilogue (one vector per tile)
    960-row frames (B = 3, 24 x 40): the wave-specialised 3x3 kernel (tile 16) with ragged tiles, bias2 per frame behind the activation
    768-row frames (B = 3, 16 x 48): the planes 3x3 kernel (tile 22), bias2 per frame
each with and without 2 K slices where the kernel has them.  S is the emulated split sum plus the frame's vector (applied where
tests/test_gpu_frame_bias.py documents it: in front of the activation for `bias`, behind the activation and the second phase for `bias2`), P the
magnitudes of its terms, the metric R.units per element, the yardstick ATen's float32 on the same split operands.  The vectors sit inside a
wider row stride with NaN in the gaps; the output sits between guard bands.  tests/test_pixel_contract_cpu.py shows that a frame index taken as
row >> 5 falls outside on the 35-row frames."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _split_ref as R  # noqa: E402
from tests._envelope import check_units  # noqa: E402
from tests._gpu import DEV, Eng, conv_weights, dv, from_nhwc, to_nhwc  # noqa: E402
from tests._guards import _guarded, _guards_intact  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd.engine import A_MUL, Act  # noqa: E402

HI = N.CONV_TILE_HI
_check = functools.partial(check_units, "SPLIT-ENVELOPE", 66, R.SPLIT_MARGIN)


def envelope(case, got, S, P, ref32):
    got = got.detach().cpu()
    _check(case, float(R.units(got, S, P).max()), float(R.units(ref32, S, P).max()))
    assert torch.isfinite(got).all(), case


def arith_name(ar):
    return {2: "2xf16", 3: "3xbf16", 0: "fp32"}[ar]


def make_eng(arith):
    return Eng(use_split=(arith != 0), arith=(arith or 3))


def frame_vectors(B, Co, seed, pad):
    """([B][Co] hard bias vectors, (device tensor [B][Co + pad] with NaN in the gaps, row stride))"""
    vec = torch.stack([R.hard_bias(Co, seed + i) for i in range(B)])
    t = torch.full((B, Co + pad), float("nan"))
    t[:, :Co] = vec
    return vec, (dv(t), Co + pad)


def guarded_out(B, H, W, Co):
    buf, v = _guarded(torch.full((B, H, W, Co), 9.0, device=DEV), -7.0)
    return buf, Act(v, B, H, W, Co, Co)


def per_frame(vec, dtype):
    return vec.to(dtype)[:, :, None, None]


# ---------------------------------------------------------------------------------------------------------------- 1x1 GEMMs, bias per frame
# (B, H, W, K, Co), tile, K slices, arithmetics
GEMM_CASES = [((3, 5, 7, 32, 64), t, None, ((2, 3, 0) if t < 10 else (2, 3))) for t in (0, 1, 2, 3, 4, 5, 13, 14)] + \
             [((3, 5, 7, 64, 64), HI | 1, 2, (2, 3))] + \
             [((3, 8, 48, 64, 192), t, sk, (2, 3)) for t in (HI | 1, HI | 2) for sk in (None, 2)]
GEMM_PARAMS = [(s, t, sk, ar) for s, t, sk, ars in GEMM_CASES for ar in ars]


def _tile_name(t):
    return (t & 15) + (16 if t & HI else 0)


@pytest.mark.parametrize("shape,tile,sk,arith", GEMM_PARAMS,
                         ids=[f"{'x'.join(map(str, s))}-tile{_tile_name(t)}-sk{k or 1}-{arith_name(a)}" for s, t, k, a in GEMM_PARAMS])
def test_gemm_bias_per_frame_envelope(shape, tile, sk, arith):
    B, H, W, K, Co = shape
    seed = 8000 + sum(shape) + _tile_name(tile)
    x, w = R.hard_act(B, K, H, W, seed), R.hard_weights(Co, K, 1, seed + 1)
    vec, frames = frame_vectors(B, Co, seed + 2, 8)
    r = R.ideal(x, w, arith, A_MUL)
    S, P = R.epilogue(r.S + per_frame(vec, torch.float64), r.P + per_frame(vec, torch.float64).abs())
    ref = R.one_thread(lambda: R.epilogue(r.ref32 + per_frame(vec, torch.float32)))
    eng = make_eng(arith)
    xa = to_nhwc(x)
    obuf, out = guarded_out(B, H, W, Co)
    eng.conv(xa, conv_weights(w, None, xa.ld), out, tile_hint=tile, split_k=sk, bias_frames=frames)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0), "damaged band around the output"
    envelope(f"frame-bias gemm {shape} tile {_tile_name(tile)} sk {sk or 1} {arith_name(arith)}", from_nhwc(out), S, P, ref)


# ---------------------------------------------------------------------------------------------------------------- 3x3 + second phase, bias2 per frame
# (B, H, W, Cin, Co, Cin2), planes kernel?, K slices, arithmetic
CONV_CASES = [((3, 24, 40, 32, 192, 16), False, sk, ar) for sk in (1, 2) for ar in (2, 3)] + [((3, 16, 48, 32, 192, 16), True, sk, 2) for sk in (1, 2)]


@pytest.mark.parametrize("shape,planes,sk,arith", CONV_CASES,
                         ids=[f"{'planes-tile22' if p else 'wave-specialised-tile16'}-{s[1]}x{s[2]}-sk{k}-{arith_name(a)}" for s, p, k, a in CONV_CASES])
def test_conv3x3_second_phase_bias2_per_frame_envelope(shape, planes, sk, arith):
    """relu(conv3x3(x) + b1) + conv1x1(x2) + b2[frame]"""
    B, H, W, Cin, Co, Cin2 = shape
    seed = 8500 + H + W + sk
    x, x2 = R.hard_act(B, Cin, H, W, seed), R.hard_act(B, Cin2, H, W, seed + 1)
    w1, w2, b1 = R.hard_weights(Co, Cin, 3, seed + 2), R.hard_weights(Co, Cin2, 1, seed + 3), R.hard_bias(Co, seed + 4)
    vec, frames = frame_vectors(B, Co, seed + 5, 12)
    r1, r2 = R.ideal(x, w1, arith, A_MUL, pad=1), R.ideal(x2, w2, arith, A_MUL)
    S1, P1 = R.epilogue(r1.S, r1.P, b1, 1)
    S, P = S1 + r2.S + per_frame(vec, torch.float64), P1 + r2.P + per_frame(vec, torch.float64).abs()
    ref = R.one_thread(lambda: R.epilogue(r1.ref32, None, b1, 1) + r2.ref32 + per_frame(vec, torch.float32))
    eng = make_eng(arith)
    xa, xa2 = to_nhwc(x), to_nhwc(x2)
    cw1, cw2 = conv_weights(w1, b1, xa.ld), conv_weights(w2, None, xa2.ld)
    obuf, out = guarded_out(B, H, W, Co)
    kw = dict(tile_hint=HI | 6, arith=2, in_pl=eng.to_planes(xa, "fbe.xpl"), in2_pl=eng.to_planes(xa2, "fbe.x2pl")) if planes else dict(tile_hint=HI | 0)
    eng.conv(xa, cw1, out, pad=1, act=N.ACT_RELU, in2=xa2, w2=cw2, split_k=(sk if sk > 1 else None), bias2_frames=frames, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0), "damaged band around the output"
    envelope(f"frame-bias2 conv3x3 + 1x1 {'planes tile 22' if planes else 'tile 16'} {shape} sk {sk} {arith_name(arith)}", from_nhwc(out), S, P, ref)
