"""Entry points and branches that no other test calls directly: vs_absmax / vs_check_finite (they decide which layers may run the 2 x f16
split), vs_clamp01_bwd, vs_mask_mul, vs_nhwc_to_nchw_scaled, vs_patchify_s / vs_unpatch_s with overlapping patches (S != P), the 7 x 7
median and the Gaussian blur (+ adjoint) at the smallest legal frame.  Each against a plain torch restatement of the operation: exact where
the kernel selects or copies, with a written rounding bound where it sums.  Inputs sit between NaN bands and outputs between sentinels
(tests/_guards.py), so an access outside a tensor shows up as a wrong value or a damaged band, inside allocated memory."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import augment as A  # noqa: E402
from oracle.inputs import synthetic_frames  # noqa: E402
from tests._envelope import U32 as U  # noqa: E402  (unit round-off of float32)
from tests._gpu import _lib  # noqa: E402
from tests._guards import _guarded, _guards_intact  # noqa: E402

from videoseal_amd import native as N  # noqa: E402

NAN, INF = float("nan"), float("inf")
FLT_MAX = torch.finfo(torch.float32).max
DENORM = 1e-42                       # a float32 denormal (min normal = 1.18e-38)
SENT = 0x5A5A                        # band value around the integer outputs


def _bits(v: float) -> int:
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item()) & 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------- vs_absmax / vs_check_finite
# grid = ceil(n / 2048) blocks of 256 threads, capped at 2048 (absmax) / 1024 (check_finite): n = 256 * 8 * 2048 + 3 is past both caps, so
# every thread takes its stride loop more than once and the last three elements belong to the second sweep of block 0
NS = [1, 255, 2049, 256 * 8 * 2048 + 3]


def _positions(n):
    """first, last, and both sides of the first workgroup boundary (element 255 | 256), clipped to the tensor"""
    return sorted({0, n - 1, min(255, n - 1), min(256, n - 1)})


def _base(n):
    """finite data of magnitude < 1 with a -0.0 and a denormal among them"""
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, generator=g) - 0.5).cuda()
    x[n // 2] = -0.0
    x[n // 3] = DENORM
    return x


@pytest.mark.parametrize("n", NS)
def test_absmax_is_the_largest_magnitude_bit_pattern(n):
    L, st = _lib()
    xb, x = _guarded(_base(n), NAN)                              # a read past either end would return the NaN pattern
    bb, bits = _guarded(torch.zeros(1, dtype=torch.int32, device="cuda"), SENT)

    def run(prior):
        bits.fill_(prior)
        N.check(L.vs_absmax(N.ptr(x), n, N.ptr(bits), st), "vs_absmax")
        assert _guards_intact(bb, SENT) and _guards_intact(xb, NAN)
        return int(bits.item())

    def want():
        return int((x.view(torch.int32) & 0x7FFFFFFF).max().item())         # the restatement: max over the magnitudes' bit patterns

    assert run(0) == want() < _bits(0.5) + 1
    for pos in _positions(n):
        keep = x[pos].clone()
        for v in (-3.5, -FLT_MAX, INF, -INF, NAN):
            x[pos] = v
            exp = want()
            assert exp == _bits(v)                               # (sanity of the restatement: the planted value is the extreme one)
            assert run(0) == exp, (n, pos, v)
            assert run(exp + 5) == exp + 5, (n, pos, v)          # a larger prior value stays
            assert run(exp - 1) == exp, (n, pos, v)              # a smaller one is replaced
        x[pos] = keep
    # signed zeros only: nothing to record, the prior value (0 or not) stays; a lone denormal is recorded with its own bit pattern
    x.fill_(-0.0)
    assert run(0) == 0 and run(77) == 77
    x[n - 1] = -DENORM
    assert run(0) == _bits(DENORM) > 0


@pytest.mark.parametrize("n", NS)
def test_check_finite_sets_the_flag_on_inf_and_nan_only_and_never_clears_it(n):
    L, st = _lib()
    xb, x = _guarded(_base(n), NAN)                              # a read past either end would set the flag
    fb, flag = _guarded(torch.zeros(1, dtype=torch.int32, device="cuda"), SENT)

    def run(prior):
        flag.fill_(prior)
        N.check(L.vs_check_finite(N.ptr(x), n, N.ptr(flag), st), "vs_check_finite")
        assert _guards_intact(fb, SENT) and _guards_intact(xb, NAN)
        return int(flag.item())

    assert bool(torch.isfinite(x).all())
    assert run(0) == 0 and run(1) == 1 and run(2) == 2           # finite data: the flag keeps whatever it held
    for pos in _positions(n):
        keep = x[pos].clone()
        for v in (-FLT_MAX, FLT_MAX, -0.0, -DENORM):             # the finite extremes are finite
            x[pos] = v
            assert run(0) == 0, (n, pos, v)
        for v in (INF, -INF, NAN, -NAN):
            x[pos] = v
            assert not bool(torch.isfinite(x).all())
            assert run(0) == 1 and run(1) == 1 and run(2) == 3, (n, pos, v)      # |= 1
        x[pos] = keep
    assert run(0) == 0


# ---------------------------------------------------------------------------------------------------------- vs_clamp01_bwd
@pytest.mark.parametrize("n", [1, 255, 1000, 256 * 4096 + 7])              # 256 * 4096 + 7: past the 4096-block cap of the launch
def test_clamp01_bwd_passes_the_gradient_on_the_closed_interval(n):
    L, st = _lib()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(n, generator=g) * 1.6 - 0.3                   # a third of the elements outside [0, 1]
    zero, one = torch.tensor(0.0), torch.tensor(1.0)
    edge = [0.0, 1.0, -0.0, float(torch.nextafter(zero, -one)), float(torch.nextafter(one, one + one)), float(torch.nextafter(one, zero)),
            float(torch.nextafter(zero, one)), NAN, INF, -INF]
    for i, v in enumerate(edge):                                 # the edge values at the front and (where they fit) at the very end
        if i < n:
            x[i] = v
        if n - 1 - i > len(edge):
            x[n - 1 - i] = v
    dy = torch.randn(n, generator=g)
    dy[::7] = NAN                                                # a blocked gradient is dropped, not multiplied by zero
    want = torch.where((x >= 0) & (x <= 1), dy, torch.zeros(()))
    if n > 8:
        assert want[0] == dy[0] or dy[0] != dy[0]
        assert want[1] == dy[1] and want[2] == dy[2] and want[3] == 0 and want[4] == 0 and want[5] == dy[5] and want[6] == dy[6]
        assert want[7] == 0 and want[8] == 0                     # (NaN compares false; inf is outside)
    xb, xd = _guarded(x.cuda(), NAN)
    db, dd = _guarded(dy.cuda(), NAN)
    ob, od = _guarded(torch.full((n,), 3.0, device="cuda"), -7.0)
    N.check(L.vs_clamp01_bwd(N.ptr(xd), N.ptr(dd), N.ptr(od), n, st), "vs_clamp01_bwd")
    assert _guards_intact(ob, -7.0) and _guards_intact(xb, NAN) and _guards_intact(db, NAN)
    got = od.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=9.0), torch.nan_to_num(want, nan=9.0))


# ---------------------------------------------------------------------------------------------------------- vs_mask_mul
@pytest.mark.parametrize("complement", [0, 1])
@pytest.mark.parametrize("Fr,C,H,W", [(2, 1, 5, 7), (3, 3, 9, 29), (1, 3, 1, 1)])         # odd planes: 35, 261 (two blocks), 1
def test_mask_mul_broadcasts_the_mask_over_the_channels(Fr, C, H, W, complement):
    L, st = _lib()
    g = torch.Generator().manual_seed(5)
    dy, m = torch.randn(Fr, C, H, W, generator=g), torch.rand(Fr, 1, H, W, generator=g)
    m[0, 0, 0, 0], m[-1, 0, -1, -1] = 0.0, 1.0
    want = dy * ((1.0 - m) if complement else m)                 # augmenter.py:175 differentiated: fp32, one rounding per operation
    db, dd = _guarded(dy.cuda(), NAN)
    mb, md = _guarded(m.cuda(), NAN)
    ob, od = _guarded(torch.full((Fr, C, H, W), 3.0, device="cuda"), -7.0)
    N.check(L.vs_mask_mul(N.ptr(dd), N.ptr(md), N.ptr(od), Fr, C, H, W, complement, st), "vs_mask_mul")
    assert _guards_intact(ob, -7.0) and _guards_intact(db, NAN) and _guards_intact(mb, NAN)
    assert torch.equal(od.cpu(), want)


# ---------------------------------------------------------------------------------------------------------- vs_nhwc_to_nchw_scaled
@pytest.mark.parametrize("Fr,H,W,C,ld", [(2, 5, 7, 3, 4), (3, 9, 29, 5, 8), (1, 1, 1, 3, 4)])
def test_nhwc_to_nchw_scaled_transposes_and_scales(Fr, H, W, C, ld):
    L, st = _lib()
    src = torch.randn(Fr, H, W, ld, generator=torch.Generator().manual_seed(6))
    src[..., C:] = NAN                                           # lanes [C, ld) are not part of the gradient and must not be read into it
    want = 2.0 * src[..., :C].permute(0, 3, 1, 2).contiguous()
    sb, sd = _guarded(src.cuda(), NAN)
    ob, od = _guarded(torch.full((Fr, C, H, W), 3.0, device="cuda"), -7.0)
    N.check(L.vs_nhwc_to_nchw_scaled(N.ptr(sd), Fr, H, W, C, ld, 2.0, N.ptr(od), st), "vs_nhwc_to_nchw_scaled")
    assert _guards_intact(ob, -7.0) and _guards_intact(sb, NAN)
    assert torch.equal(od.cpu(), want)
    N.check(L.vs_nhwc_to_nchw_scaled(N.ptr(sd), Fr, H, W, C, ld, -0.3, N.ptr(od), st), "vs_nhwc_to_nchw_scaled")
    assert torch.equal(od.cpu(), torch.tensor(-0.3, dtype=torch.float32) * src[..., :C].permute(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------- vs_patchify_s / vs_unpatch_s
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("H,W", [(8, 12), (9, 7)])
@pytest.mark.parametrize("C,ld", [(3, 4), (6, 8)])
def test_patchify_s_is_the_im2col_of_a_strided_patch_conv_and_unpatch_s_its_adjoint(H, W, C, ld, S):
    """training.py runs the stem with P = 4 and S = stem_stride (2 on ChunkySeal: overlapping patches; convnext.py:100-109).  cols is the
    im2col of F.conv2d(stride = S) in the k order of the packed weights, k = ky * CP + kx * ld + c with CP = P * ld rounded up to 16
    (exact: a copy); vs_unpatch_s is its transpose (a sum of at most (P / S)^2 = 4 terms per pixel, fixed order)."""
    L, st = _lib()
    B, P, NO = 2, 4, 5
    Ho, Wo = (H - P) // S + 1, (W - P) // S + 1
    CP = (P * ld + 15) // 16 * 16
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, H, W, generator=g)
    xa = torch.zeros(B, H, W, ld)
    xa[..., :C] = x.permute(0, 2, 3, 1)
    xb, xd = _guarded(xa.cuda(), NAN)
    cb, cols = _guarded(torch.full((B * Ho * Wo, P * CP), 3.0, device="cuda"), -7.0)
    N.check(L.vs_patchify_s(N.ptr(xd), B, H, W, ld, P, S, N.ptr(cols), st), "vs_patchify_s")
    assert _guards_intact(cb, -7.0) and _guards_intact(xb, NAN)
    # restatement: the P x P windows at stride S, row (b, oy, ox), columns (ky, [kx, c] padded with zeros to CP)
    win = xa.unfold(1, P, S).unfold(2, P, S).permute(0, 1, 2, 4, 5, 3)                     # [B, Ho, Wo, ky, kx, ld]
    want = torch.zeros(B, Ho, Wo, P, CP)
    want[..., : P * ld] = win.reshape(B, Ho, Wo, P, P * ld)
    assert torch.equal(cols.cpu(), want.reshape(B * Ho * Wo, P * CP))
    # ... which is the patch matrix of the conv: cols @ packed weight == F.conv2d(stride = S), both in fp64
    w = torch.randn(NO, C, P, P, generator=g)
    wk = torch.zeros(NO, P, CP, dtype=torch.float64)
    tmp = torch.zeros(NO, P, P, ld, dtype=torch.float64)
    tmp[..., :C] = w.double().permute(0, 2, 3, 1)
    wk[:, :, : P * ld] = tmp.reshape(NO, P, P * ld)
    y = F.conv2d(x.double(), w.double(), stride=S).permute(0, 2, 3, 1).reshape(-1, NO)
    assert (cols.cpu().double() @ wk.reshape(NO, P * CP).t() - y).abs().max() < 1e-12
    # adjoint: <dcols, P x> == <P^T dcols, x> in fp64.  P^T sums at most (P / S)^2 fp32 terms per element: its rounding error is at most
    # ((P / S)^2 - 1) U times the sum of their magnitudes, i.e. <P^T |dcols|, |x|> in total.
    dcols = torch.randn(B * Ho * Wo, P * CP, generator=g)                                  # (the pad columns hold junk: the adjoint ignores them)
    db, dd = _guarded(dcols.cuda(), NAN)
    ob, dx = _guarded(torch.full((B, H, W, ld), 3.0, device="cuda"), -7.0)
    N.check(L.vs_unpatch_s(N.ptr(dd), B, H, W, ld, P, S, N.ptr(dx), st), "vs_unpatch_s")
    assert _guards_intact(ob, -7.0) and _guards_intact(db, NAN)
    xr = torch.randn(B, H, W, ld, dtype=torch.float64, generator=g).requires_grad_(True)   # every lane takes part: the operator acts on all ld
    px = torch.zeros(B, Ho, Wo, P, CP, dtype=torch.float64)
    px[..., : P * ld] = xr.unfold(1, P, S).unfold(2, P, S).permute(0, 1, 2, 4, 5, 3).reshape(B, Ho, Wo, P, P * ld)
    (px.reshape(-1, P * CP) * dcols.double()).sum().backward()
    ref = xr.grad                                                                            # P^T dcols by fp64 autograd of the restatement
    xr2 = torch.ones(B, H, W, ld, dtype=torch.float64, requires_grad=True)
    pa = torch.zeros(B, Ho, Wo, P, CP, dtype=torch.float64)
    pa[..., : P * ld] = xr2.unfold(1, P, S).unfold(2, P, S).permute(0, 1, 2, 4, 5, 3).reshape(B, Ho, Wo, P, P * ld)
    (pa.reshape(-1, P * CP) * dcols.double().abs()).sum().backward()
    nterm = (P // S) ** 2
    bound = (nterm - 1) * U * xr2.grad
    assert ((dx.cpu().double() - ref).abs() <= bound).all()
    if S == P:
        assert torch.equal(dx.cpu().double(), ref)                                         # one term per pixel: a copy
    lhs = float((px.detach().reshape(-1, P * CP) * dcols.double()).sum())
    rhs = float((dx.cpu().double() * xr.detach()).sum())
    assert abs(lhs - rhs) <= float((bound * xr.detach().abs()).sum()) + 1e-12 * abs(lhs)
    covered = torch.zeros(H, W, dtype=torch.bool)
    covered[: (Ho - 1) * S + P, : (Wo - 1) * S + P] = True
    assert (dx.cpu()[:, ~covered] == 0).all()                                              # pixels outside the last whole patch get no gradient


# ---------------------------------------------------------------------------------------------------------- vs_median_filter
def _median(x, k):
    L, st = _lib()
    planes, H, W = x.shape[0] * x.shape[1], x.shape[2], x.shape[3]
    xb, xd = _guarded(x.cuda(), NAN)
    ob, od = _guarded(torch.full(x.shape, 3.0, device="cuda"), -7.0)
    code = L.vs_median_filter(N.ptr(xd), N.ptr(od), planes, H, W, k, st)
    torch.cuda.synchronize()
    assert _guards_intact(ob, -7.0) and _guards_intact(xb, NAN)
    return code, od.cpu()


@pytest.mark.parametrize("shape", [(93, 118), (2, 3)])
def test_median_filter_7x7_and_the_unsupported_size(shape):
    """utils/image.py:60-84 (median of the row medians, zero padded): a selection, so exact.  2 x 3: the window is mostly padding."""
    x = synthetic_frames(3, 93, 118, seed=31) if shape == (93, 118) else torch.rand(2, 3, 2, 3, generator=torch.Generator().manual_seed(8))
    code, got = _median(x, 7)
    assert code == 0
    assert torch.equal(got, A.median_filter(x, 7))
    code, got = _median(x, 9)
    assert code == N.ERR_UNSUPPORTED
    assert (got == 3.0).all()                                    # and nothing was launched


# ---------------------------------------------------------------------------------------------------------- vs_gaussian_blur (+ adjoint)
def _blur64(x, k):
    """torchvision's gaussian_blur (valuemetric.py:209-219 -> _get_gaussian_kernel1d, reflect padding) in float64"""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    half = (k - 1) * 0.5
    t = torch.linspace(-half, half, steps=k, dtype=torch.float64)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    k1 = pdf / pdf.sum()
    C = x.shape[-3]
    xp = F.pad(x, [k // 2] * 4, mode="reflect") if k > 1 else x
    return F.conv2d(xp, torch.outer(k1, k1).expand(C, 1, k, k).contiguous(), groups=C)


def _blur_cases():
    out = []
    for k in (3, 17, 33):
        m = k // 2 + 1                                           # the smallest legal extent: reflection needs k / 2 < H, W
        out += [(k, m, 37), (k, 37, m), (k, m, m)]
    return out + [(1, 1, 1), (1, 5, 3)]


@pytest.mark.parametrize("k,H,W", _blur_cases())
def test_gaussian_blur_and_its_adjoint_at_the_smallest_legal_frame(k, H, W):
    """Every reflected index of a frame with H = k / 2 + 1 rows reaches the far border (row y - k/2 mirrors to k/2 - y <= H - 1, row
    y + k/2 to 2 H - 2 - y - k/2 >= 0): one row fewer and the single reflection of the kernel would leave the frame.
    Bound, in units of U = 2^-24: the tap position x = -half + 2 half i / (k - 1) carries 3 roundings, x / sigma 2 more (the division, sigma as
    a float), its square 2 * 5 + 1 = 11, an argument of magnitude < 4.6 ((16 / 5.3)^2 / 2 at k = 33, the largest): < 51 absolute, i.e. relative
    in the weight, + 2 of expf; the normalisation adds k (a sum of k terms and a division); a pass accumulates k products: k + 1.  Per pass
    53 + 2 k + 1, two passes: (4 k + 108) U, relative to the same blur of the magnitudes (the weights are positive) -- element-wise."""
    L, st = _lib()
    Fr, C = 2, 3
    g = torch.Generator().manual_seed(100 * k + H)
    x = torch.rand(Fr, C, H, W, generator=g) * 2 - 0.5
    dy = torch.randn(Fr, C, H, W, generator=g)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x64 = x.double().requires_grad_(True)
    y64 = _blur64(x64, k)
    y64.backward(dy.double())
    xa = x.double().abs().requires_grad_(True)
    ya = _blur64(xa, k)
    ya.backward(dy.double().abs())
    rel = (4 * k + 108) * U
    xb, xd = _guarded(x.cuda(), NAN)
    tb, tmp = _guarded(torch.full(x.shape, 3.0, device="cuda"), -7.0)
    ob, od = _guarded(torch.full(x.shape, 3.0, device="cuda"), -7.0)
    N.check(L.vs_gaussian_blur(N.ptr(xd), N.ptr(tmp), N.ptr(od), Fr * C, H, W, k, sigma, st), "vs_gaussian_blur")
    assert _guards_intact(ob, -7.0) and _guards_intact(tb, -7.0) and _guards_intact(xb, NAN)
    got = od.cpu()
    assert ((got.double() - y64.detach()).abs() <= rel * ya.detach()).all()
    plain_t, plain = torch.empty_like(x, device="cuda"), torch.empty_like(x, device="cuda")
    xc = x.cuda()
    N.check(L.vs_gaussian_blur(N.ptr(xc), N.ptr(plain_t), N.ptr(plain), Fr * C, H, W, k, sigma, st), "vs_gaussian_blur")
    assert torch.equal(plain.cpu(), got)
    # adjoint
    db, dd = _guarded(dy.cuda(), NAN)
    tb2, tmp2 = _guarded(torch.full(x.shape, 3.0, device="cuda"), -7.0)
    gb, gd = _guarded(torch.full(x.shape, 3.0, device="cuda"), -7.0)
    N.check(L.vs_gaussian_blur_bwd(N.ptr(dd), N.ptr(tmp2), N.ptr(gd), Fr * C, H, W, k, sigma, st), "vs_gaussian_blur_bwd")
    assert _guards_intact(gb, -7.0) and _guards_intact(tb2, -7.0) and _guards_intact(db, NAN)
    gx = gd.cpu()
    assert ((gx.double() - x64.grad).abs() <= rel * xa.grad).all()
    if k == 1:
        assert torch.equal(got, x) and torch.equal(gx, dy)       # one tap of weight 1
    # <blur(x), dy> == <x, blur^T(dy)> with the kernels' own outputs
    lhs, rhs = float((got.double() * dy.double()).sum()), float((gx.double() * x.double()).sum())
    assert abs(lhs - rhs) <= 2 * rel * float((ya.detach() * dy.double().abs()).sum())
