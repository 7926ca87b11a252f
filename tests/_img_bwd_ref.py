"""fp64 envelopes of the IMAGE-DOMAIN ADJOINT kernels (csrc/bwd_shell.hip: vs_resize_nchw_bwd, vs_gaussian_blur_bwd, vs_aug_warp_bwd, vs_embed_tail_bwd,
vs_tail_key_reduce, vs_aug_color_bwd, vs_percep_mse / _grad, vs_aug_window_average_bwd, vs_aug_gather_frames_bwd and the exact pointwise adjoints):
formulas, upstream gradients, cases, metrics and the margin shared by tests/test_img_bwd_contract_cpu.py (the envelope has teeth; no GPU) and
tests/test_gpu_img_bwd_envelope.py (every kernel against it).

As in tests/_img_ref.py, whose formulas, hard frames and case tables are the forward side of every adjoint here: the reference is the adjoint of the
_img_ref formula in float64, taken by autograd on the CPU from the same fp32 input and coefficient values the kernel receives; the yardstick is the
same autograd in float32 on one thread.  The error is max |got - ref64| / max(max |ref64|, tiny) per (case, upstream-gradient kind) -- for the colour
ops per band of rows of hard_pixels, because a nearly grey pixel's hue gradient is of order 1 / ulp and must not set the scale for the others.
A kernel may exceed the yardstick by IMG_BWD_FP64_MARGIN.

Gates (clamp: 0 <= v <= 1 passes the gradient, bounds included, as torch.clamp does) and hue sectors are discontinuities of the adjoint:
  * a pre-clamp value that is the bound itself in float64 AND in the fp32 evaluation (black / white pixels, dyadic factors, the cube's corners, a
    zero key frame) is an exact case: one answer, no band;
  * any other value within a band of a bound (GATE_BAND, HUE_*_BAND: derived from the operation counts below) is flagged: a flagged element of a
    pointwise gate may match the gradient with its gate open or closed (masked_err's `other`), a flagged hue pixel is left out; the flagged share
    of any band of rows is capped at FLAG_SHARE, a condition on the float64 reference alone.  Contrast, whose gate feeds a frame-wide sum, allows none.
The fp32 emulations of the kernels' own index rules (adjoint_range, the blur folds, the warp search box, the key-frame weights) carry the seeded
defects of the contract test."""
import functools

import torch

from tests import _img_ref as R
from tests._envelope import TINY, check_rows, one_thread

# Twice the largest ratio hip / max(yardstick, 2^-24) measured on an MI355X over every line of tests/test_gpu_img_bwd_envelope.py
# (profiles/img_bwd_fp64_envelope.txt lists them), never more than 8: a kernel that needs more has a defect.
IMG_BWD_FP64_MARGIN = 8.0      # min(2 x 4.105, cap): the largest ratio measured is vs_gaussian_blur_bwd, k = 33 on 17 x 40, `checker` (1627 lines)
F32, F64 = torch.float32, torch.float64
envelope = functools.partial(check_rows, "IMG-BWD-ENVELOPE", 58, "cpu-fp32", IMG_BWD_FP64_MARGIN)

# v = f x + (1 - f) ref (ref = 0, grey = 3 products + 2 sums, or the frame mean) and v = p + hm ((si p + sw d) - p): at most 12 roundings, each of
# 2^-24 relative to an intermediate value that is at most the sum `mag` of the terms' magnitudes: |fp32 v - v| <= 12 x 2^-24 x mag < GATE_BAND x mag
GATE_BAND = 2.0 ** -20
# h6 = 6 frac(frac(hsum / 6 + 1) + factor): two differences and two quotients of magnitude <= 1, then six operations on values of magnitude <= 6:
# 10 x 6 x 2^-24 < 2^-18 on h6 (a nearly grey pixel's quotients are exactly 0 or 1: the differences of neighbouring floats are exact)
HUE_SECTOR_BAND = 2.0 ** -18
# q, t = v (1 - s (1 - f)): the error of f (2^-18, times v s) and four roundings of magnitude <= v: v (2^-18 s + 2^-22) < 2^-17 v (s + 2^-5);
# p = v (1 - s) does not read f: s = cr / maxc, 1 - s, the product and their inputs' differences: 8 x 2^-24 v = 2^-21 v
HUE_GATE_BAND = 2.0 ** -17
HUE_P_BAND = 2.0 ** -21
FLAG_SHARE = 0.005             # the largest flagged share of any band of rows (a condition on the float64 reference alone)


def _k(v, dt):
    return torch.tensor(v, dtype=F32).to(dt)


# ------------------------------------------------------------------------------------------------------------------------ metric, autograd
def masked_err(got, own, other=None, amb=None, keep=None):
    """max |got - own| / max(max |own|, tiny) over the elements of `keep` (default: all); an element of `amb` may match `other` instead"""
    got, own = got.detach().double().cpu(), own.detach().double()
    assert got.shape == own.shape, (got.shape, own.shape)
    d = (got - own).abs()
    if amb is not None and amb.any():
        d = torch.where(amb, torch.minimum(d, (got - other.detach().double()).abs()), d)
    m = own.abs()
    if keep is not None:
        keep = keep.expand_as(d)
        d, m = d * keep, m * keep
    return float(d.max() / max(float(m.max()), TINY))


def adjoint(fn, x, dy, dt):
    """d <fn(x, dt), dy> / d x in dtype dt by autograd on one thread; fn(x, dt) is an _img_ref formula"""
    def run():
        xl = x.detach().to(dt).requires_grad_(True)
        (g,) = torch.autograd.grad(fn(xl, dt), xl, dy.to(dt))
        return g
    return one_thread(run)


def adjoint_pair(fn, x, dy):
    """(float64 reference, float32 yardstick)"""
    return adjoint(fn, x, dy, F64), adjoint(fn, x, dy, F32)


def near(v64, v32, bound, band):
    """flagged: the float64 value is within `band` of `bound` without being the bound itself in both precisions (the exact cases)"""
    return ((v64 - bound).abs() <= band) & ~((v64 == bound) & (v32.double() == bound))


def gate_flags(v64, v32, mag, band=GATE_BAND):
    """mag: the sum of the magnitudes of the expression's terms (float64), which its rounding errors are relative to"""
    return near(v64, v32, 0.0, band * mag) | near(v64, v32, 1.0, band * mag)


# ------------------------------------------------------------------------------------------------------------------------ upstream gradients
DY_KINDS = ("noise", "ones", "checker", "ramp", "impulse")


def hard_dy(shape, seed=0):
    """{kind: float32 `shape` = [..., H, W]}: signed noise, constant 1, +-1 checkerboard, a ramp through zero, impulses (the four corners, the
    midpoint of the top and of the left edge, an interior 7 x 5 lattice); plane p of every structured kind is scaled by 1 + p / 8 (exact)"""
    *lead, H, W = shape
    P = 1
    for n in lead:
        P *= n
    g = torch.Generator().manual_seed(2300 + 131 * H + W + seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pf = (1 + torch.arange(P).float() / 8).view(P, 1, 1)
    imp = torch.zeros(H, W)
    imp[2::5, 3::7] = 1.0
    imp[0, 0] = imp[0, -1] = imp[-1, 0] = imp[-1, -1] = imp[0, W // 2] = imp[H // 2, 0] = 1.0
    ramp = xx.float() / max(W - 1, 1) + yy.float() / max(H - 1, 1) - 1.0
    out = {"noise": torch.rand(P, H, W, generator=g) * 2 - 1, "ones": torch.ones(P, H, W), "checker": pf * (1 - 2 * ((yy + xx) % 2).float()),
           "ramp": pf * ramp, "impulse": pf * imp}
    return {k: v.reshape(*lead, H, W).contiguous() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------------ resize
# the transposes of the crop-free plane cases of _img_ref (H, W of the INPUT gradient, oh, ow of dy, antialias)
RESIZE_BWD_CASES = [(93, 118, 29, 37, 1), (64, 64, 1, 1, 1), (5, 7, 64, 64, 1), (5, 7, 64, 64, 0), (1, 9, 4, 33, 1), (93, 118, 130, 165, 1),
                    (31, 45, 64, 64, 0), (200, 12, 16, 3, 1), (104, 8, 8, 8, 1)]
assert all((h, w, None, oh, ow, aa) in R.PLANE_CASES for h, w, oh, ow, aa in RESIZE_BWD_CASES)


def adjoint_range(n_in, n_out, aa, defect=None):
    """(o_lo, o_hi) [n_in] long: csrc/resize_taps.h::adjoint_range in its own fp32 arithmetic.  DEFECTS: "no_i1" = without the rule that plain
    bilinear's clamp at 0 makes every early output read pixels 0 and 1; "no_slack" = the bounds of the filter's support alone, taken between pixel
    corners (|i - scale o| <= support) and rounded inward: the half-pixel error that 1.5 input pixels and one output index of slack would hide;
    "slack_only" = the slack alone removed, which is still the exact set of contributors (no defect: the contract test shows it stays inside)"""
    i = torch.arange(n_in, dtype=F32)
    scale = torch.tensor(float(n_in), dtype=F32) / torch.tensor(float(n_out), dtype=F32)
    support = scale if (aa and scale >= 1) else torch.ones((), dtype=F32)
    if defect == "no_slack":
        lo, hi = torch.ceil((i - support) / scale), torch.floor((i + support) / scale)
    elif defect == "slack_only":          # the 1.5 input pixels and the output index per side removed, nothing else: |i + 0.5 - centre| <= support
        lo, hi = torch.floor(((i + 0.5) - support) / scale - 0.5), torch.ceil(((i + 0.5) + support) / scale - 0.5)
    else:
        lo = torch.floor(((i + 0.5) - support - 1.5) / scale - 0.5) - 1
        hi = torch.ceil(((i + 0.5) + support + 1.5) / scale - 0.5) + 1
    if not aa and defect != "no_i1":
        lo[:2] = 0
    return lo.clamp_min(0).long(), hi.clamp_max(n_out - 1).long()


def resize_adjoint32(dy, H, W, aa, defect=None):
    """fp32 emulation of vs_resize_nchw_bwd: the transposed fp32 tap matrices restricted to adjoint_range, x taps first"""
    oh, ow = dy.shape[-2:]

    def A(n_in, n_out):
        lo, hi = adjoint_range(n_in, n_out, aa, defect)
        o = torch.arange(n_out)[:, None]
        return R.resize_matrix(n_in, n_out, aa, F32) * ((o >= lo[None]) & (o <= hi[None]))
    return one_thread(lambda: A(H, oh).t() @ (dy @ A(W, ow)))


# ------------------------------------------------------------------------------------------------------------------------ blur
BLUR_BWD_SHAPES = {3: [(2, 2), (33, 47)], 9: [(5, 40), (33, 47)], 17: [(9, 33), (33, 47)], 33: [(17, 40), (33, 47)]}          # k: (H, W); r + 1 on one axis


def blur_adjoint32(dy, k, defect=None):
    """fp32 emulation of vs_gaussian_blur_bwd: per axis, position u collects dxp[u] + dxp[-u] (1 <= u <= r) + dxp[2 (n - 1) - u]
    (n - 1 - r <= u <= n - 2), dxp[i] = sum_t w[t] dy[i - t + r].  DEFECTS: "no_far" = without the far-side fold; "one_fold" = the far fold
    only where the near one did not apply (else-if)"""
    sigma = _k(R.blur_sigma(k), F32)
    half = (k - 1) * 0.5
    pdf = torch.exp(-0.5 * (torch.linspace(-half, half, steps=k, dtype=F32) / sigma).pow(2))
    w = pdf / pdf.sum()
    r = k // 2

    def A(n):
        a = torch.zeros(n, n, dtype=F32)          # [u][o]

        def dxp(i):
            row = torch.zeros(n, dtype=F32)
            for t in range(k):
                o = i - t + r
                if 0 <= o < n:
                    row[o] += w[t]
            return row
        for u in range(n):
            a[u] = dxp(u)
            nearf = 1 <= u <= r
            if nearf:
                a[u] += dxp(-u)
            if n - 1 - r <= u <= n - 2 and defect != "no_far" and not (defect == "one_fold" and nearf):
                a[u] += dxp(2 * (n - 1) - u)
        return a
    H, W = dy.shape[-2:]
    return one_thread(lambda: (A(H) @ dy) @ A(W).t())


# ------------------------------------------------------------------------------------------------------------------------ warp
WHOLE_PERSP = ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.03, 0.0], 33, 47)
# (coeffs, H, W): x_in = ox / (1 + 0.03 ox) < 33.4: the input columns beyond have a homogeneous weight cw = 1 - 0.03 px <= 0 -- the `whole` fallback
ZOOM_PERSP = ([0.4, 0.0, 3.0, 0.0, 0.4, 2.0, 0.001, 0.0005], 33, 47)
# a 2.5 x zoom: one input pixel collects some 25 outputs, its footprint spans several output pixels (where a search box can be too small at all)


def warp_inverse(kind, t, H, W, oh, ow):
    """the nine floats that bound the adjoint's search (autograd.WarpFn): the inverse, in float64, of the map from an output pixel centre to the
    homogeneous input pixel-centre coordinates"""
    t = [float(v) for v in t]
    if kind == 0:
        M = torch.tensor([[0.5 * W * t[0], 0.5 * W * t[1], 0.5 * W * (t[2] + 1.0 - 0.5 * ow * t[0] - 0.5 * oh * t[1])],
                          [0.5 * H * t[3], 0.5 * H * t[4], 0.5 * H * (t[5] + 1.0 - 0.5 * ow * t[3] - 0.5 * oh * t[4])], [0.0, 0.0, 1.0]], dtype=F64)
    else:
        M = torch.tensor([[W / ow * t[0], W / ow * t[1], W / ow * t[2]], [H / oh * t[3], H / oh * t[4], H / oh * t[5]], [t[6], t[7], 1.0]], dtype=F64)
    inv = torch.linalg.inv(M)
    inv = inv / inv[2, 2] if abs(float(inv[2, 2])) > 1e-12 else inv
    return [float(v) for v in inv.reshape(-1)]


def warp_box(inv, ux, uy, margin=1.5, half=1.0):
    """(x0, x1, y0, y1, whole) of warp_bwd_kernel's search box for the input pixels (ux, uy) (float32 tensors), in its fp32 arithmetic: the box of
    the input square of half-width `half` around the pixel centre, widened by `margin` output pixels"""
    iv = [torch.tensor(v, dtype=F32) for v in inv]
    big = torch.full_like(ux, 1e30)
    lox, hix, loy, hiy, whole = big, -big, big, -big, torch.zeros_like(ux, dtype=torch.bool)
    for c in range(4):
        px, py = ux + 0.5 + (half if c & 1 else -half), uy + 0.5 + (half if c & 2 else -half)
        cw = iv[6] * px + iv[7] * py + iv[8]
        ok = cw > 1e-6
        whole = whole | ~ok
        cx, cy = (iv[0] * px + iv[1] * py + iv[2]) / cw - 0.5, (iv[3] * px + iv[4] * py + iv[5]) / cw - 0.5
        lox, hix = torch.where(ok, torch.minimum(lox, cx), lox), torch.where(ok, torch.maximum(hix, cx), hix)
        loy, hiy = torch.where(ok, torch.minimum(loy, cy), loy), torch.where(ok, torch.maximum(hiy, cy), hiy)
    return torch.floor(lox - margin), torch.ceil(hix + margin), torch.floor(loy - margin), torch.ceil(hiy + margin), whole


def warp_adjoint32(dy, kind, coeffs, H, W, bilinear, margin=1.5, half=1.0):
    """fp32 emulation of vs_aug_warp_bwd on dy [P, oh, ow]: every output pixel's taps from the fp32 grid, each added to its input pixel u only if
    the output pixel lies in u's search box.  margin = 0 alone loses nothing (the image of a square under a projective map is a convex quadrilateral:
    the corners' box is exact, the margin only covers the fp32 inverse); DEFECT: half = 0.5, margin = 0 (the pixel's own square).  Returns (dx [P, H, W], number of input pixels on the `whole` fallback)"""
    P, oh, ow = dy.shape
    ix, iy = R.warp_coords(kind, coeffs, H, W, oh, ow, F32)
    ix, iy = torch.broadcast_tensors(ix, iy)
    oy, ox = torch.meshgrid(torch.arange(oh, dtype=F32), torch.arange(ow, dtype=F32), indexing="ij")
    inv = warp_inverse(kind, coeffs, H, W, oh, ow)
    if bilinear:
        fx, fy = torch.floor(ix), torch.floor(iy)
        taps = [(fx + a, fy + b, (ix - fx if a else fx + 1 - ix) * (iy - fy if b else fy + 1 - iy)) for b in (0, 1) for a in (0, 1)]
    else:
        taps = [(torch.round(ix), torch.round(iy), torch.ones_like(ix))]
    dx = torch.zeros(P, H * W, dtype=F32)
    for ux, uy, wgt in taps:
        x0, x1, y0, y1, whole = warp_box(inv, ux, uy, margin, half)
        ok = (ux >= 0) & (ux <= W - 1) & (uy >= 0) & (uy <= H - 1) & (whole | ((ox >= x0) & (ox <= x1) & (oy >= y0) & (oy <= y1)))
        idx = (uy.clamp(0, H - 1) * W + ux.clamp(0, W - 1)).long().flatten()
        dx.index_add_(1, idx, (dy * (wgt * ok)).reshape(P, -1))
    gy, gx = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    return dx.view(P, H, W), int(warp_box(inv, gx, gy)[4].sum())


def scatter_adjoint(dy, index, H, W, dt):
    """dx [P, H, W] = sum of dy [P, oh, ow] over the output pixels whose source index (a flat pixel number, -1 = off the frame) is the pixel"""
    P = dy.shape[0]
    idx = index.reshape(-1).long()
    ok = idx >= 0
    dx = torch.zeros(P, H * W, dtype=dt)
    one_thread(lambda: dx.index_add_(1, idx[ok], dy.to(dt).reshape(P, -1)[:, ok]))
    return dx.view(P, H, W)


# ------------------------------------------------------------------------------------------------------------------------ embed tail
def key_matrix(Fn, step, mode, total_key, dt, defect=None):
    """[Fn, total_key]: the weights of _img_ref.key_expand (videoseal.py:80-118) as a matrix, so that the adjoint is its transpose.
    DEFECTS: "j_over_step" = interpolate weight j / step; "no_clamp" = a key index beyond total_key - 1 is not clamped: its frames reach no key"""
    Wk = torch.zeros(Fn, total_key, dtype=dt)
    for f in range(Fn):
        ka, kb, wa, wb = f // step, 0, torch.ones((), dtype=dt), torch.zeros((), dtype=dt)
        if mode == 1:
            wa = wa * (1.0 if f % step == 0 else 0.0)
        elif mode == 2:
            if f < ((Fn - 1) // step) * step:
                kb = ka + 1
                den = float(step if defect == "j_over_step" else step - 1)
                lin = (torch.tensor(float(f % step), dtype=F32) / torch.tensor(den, dtype=F32)) if step > 1 else torch.zeros(())
                wa = (1 - lin).to(dt)
                wb = (1 - (1 - lin)).to(dt)
            else:
                ka = total_key - 1
        for kk, w in ((ka, wa), (kb, wb)):
            if kk >= total_key:
                if defect == "no_clamp":
                    continue
                kk = total_key - 1
            Wk[f, kk] += w
    return Wk


def tail_linear(delta, Fn, H, W, cfg, hm_low, dt):
    """delta [total_key, Cd, S, S] -> d [Fn, Cd, H, W]: key-frame expansion, the low-resolution heat-map, the resize up (the linear part of
    _img_ref.embed_tail, from its own pieces)"""
    d = R.key_expand(delta, Fn, cfg["step"], cfg["mode"], cfg["total_key"], dt)
    if hm_low is not None:
        d = d * hm_low.to(dt)[:, None]
    return R.resize(d, (H, W), cfg["aa"], dt) if tuple(d.shape[-2:]) != (H, W) else d


def key_reduce32(g_low, hm_low, Fn, cfg, defect=None):
    """fp32 emulation of vs_tail_key_reduce: d_delta[k] = sum_f w(f, k) (hm_low[f] g_low[f])"""
    Wk = key_matrix(Fn, cfg["step"], cfg["mode"], cfg["total_key"], F32, defect)
    g = g_low if hm_low is None else g_low * hm_low[:, None]
    return one_thread(lambda: torch.einsum("fk,fcyx->kcyx", Wk, g))


def tail_pre(preds, imgs, hm, cfg, dt, mag=False):
    """the pre-clamp value of the tail's blend [F, 3, H, W] from the resized watermark `preds` [F, Cd, H, W] (an INPUT of vs_embed_tail_bwd);
    hm: the full-resolution heat-map [F, 1, H, W] or None -- the training order of wam.py:103-113 (_img_ref.embed_tail with attenuate = 2)"""
    p, d = imgs.to(dt), preds.to(dt)
    a, b = _k(cfg["si"], dt) * p, _k(cfg["sw"], dt) * d
    v, m = a + b, a.abs() + b.abs()
    if hm is not None:
        v, m = p + hm.to(dt) * (v - p), p.abs() + hm.to(dt).abs() * (m + p.abs())
    return (v, m) if mag else v


def tail_flags(preds, imgs, hm, cfg):
    """flagged elements [F, 3, H, W] of the tail's clamp"""
    with torch.no_grad():
        v64, m64 = tail_pre(preds, imgs, hm, cfg, F64, mag=True)
        return gate_flags(v64, tail_pre(preds, imgs, hm, cfg, F32), m64) & bool(cfg["clamp"])


def tail_out(preds, imgs, hm, cfg, dt):
    v = tail_pre(preds, imgs, hm, cfg, dt)
    return v.clamp(0, 1) if cfg["clamp"] else v


def tail_point_adjoint(preds, imgs, hm, d_out, d_preds, cfg, dt, flip=None, strict=False):
    """closed form of d <tail_out, d_out> / d preds + d_preds with the gates written out; flip: gates to invert (the other candidate of the
    flagged elements).  DEFECT: strict = 0 < v < 1"""
    Cd = preds.shape[1]
    g = torch.zeros_like(preds, dtype=dt)
    if d_out is not None:
        v = tail_pre(preds, imgs, hm, cfg, dt)
        gate = ((v > 0) & (v < 1)) if strict else ((v >= 0) & (v <= 1))
        if not cfg["clamp"]:
            gate = torch.ones_like(gate)
        if flip is not None:
            gate = gate ^ flip
        t = d_out.to(dt) * gate * (_k(cfg["sw"], dt) * (hm.to(dt) if hm is not None else 1.0))
        g = t if Cd == 3 else t.sum(1, keepdim=True)
    return g + d_preds.to(dt) if d_preds is not None else g


def sat_frames(Fn, H, W, seed=0):
    """the `sat` kind: noise with blocks of exactly 0.0 and exactly 1.0 (what saturated video pixels are)"""
    x = R.tail_frames(Fn, H, W, seed)["noise"].clone()
    x[:, :, : H // 3, : W // 2] = 0.0
    x[:, :, H // 2:, W // 3:] = 1.0
    return x


# (tag, F, H, W, S, Cd, low-res heat-map?, full heat-map?, cfg): the shapes and modes of _img_ref.TAIL_CASES (a full heat-map in the training
# order, the only one with an adjoint) plus F not a multiple of step with total_key clamping the last group
TAIL_BWD_CASES = [(tag, Fn, H, W, S, Cd, low, bool(cfg["attenuate"]) and not low, cfg) for tag, Fn, H, W, S, Cd, low, _, cfg in R.TAIL_CASES] + [
    ("interpolate step 2 total_key 2", 5, 24, 40, 16, 1, True, False, R._tc(step=2, mode=2, total_key=2, attenuate=1)),
    ("repeat step 2 total_key 2 Cd 3", 5, 24, 40, 16, 3, False, True, R._tc(step=2, mode=0, total_key=2, attenuate=2)),
    ("alternate step 3 total_key 1", 5, 9, 12, 16, 1, False, False, R._tc(step=3, mode=1, total_key=1, attenuate=0)),
    ("interpolate step 3 F 8", 8, 9, 12, 16, 3, False, False, R._tc(step=3, mode=2, total_key=3, attenuate=0)),
]


def tail_bwd_inputs(case, kind):
    """(imgs, delta, hm_low or None, hm_full or None, cfg, preds) of one case and frame kind; kind "sat": saturated frames, key frame 0 of delta all
    zero (v is the pixel itself: exactly on a bound inside the blocks, and the gradient must pass), sw = 3 so that both gates close elsewhere"""
    tag, Fn, H, W, S, Cd, low, full, cfg = case
    nkey = cfg["total_key"] or (Fn + cfg["step"] - 1) // cfg["step"]
    cfg = dict(cfg, total_key=nkey)
    delta, hm_low = R.tail_inputs(Fn, Cd, S, cfg["step"])
    delta = delta[:nkey].contiguous()
    if kind == "sat":
        imgs = sat_frames(Fn, H, W)
        delta[0] = 0.0
        cfg = dict(cfg, sw=3.0, si=1.0)
    else:
        imgs = R.tail_frames(Fn, H, W)[kind]
    hm_low = hm_low if low else None
    hm_full = R.jnd(imgs, F32)[0] if full else None          # an input of the adjoint: the values the kernel reads
    preds = tail_linear(delta, Fn, H, W, cfg, hm_low, F32)
    return imgs, delta, hm_low, hm_full, cfg, preds


TAIL_KINDS = ("noise", "flat", "jump", "sat")
TAIL_DY = {"noise": "noise", "flat": "checker", "jump": "ramp", "sat": "ones"}          # d_out per frame kind (ones on `sat`: the gates' own pattern)


def tail_dy(case, kind):
    """(d_out [F, 3, H, W], d_preds [F, Cd, H, W] = impulses) of one case and frame kind"""
    tag, Fn, H, W, S, Cd = case[:6]
    return hard_dy((Fn, 3, H, W))[TAIL_DY[kind]], hard_dy((Fn, Cd, H, W), seed=1)["impulse"]


# ------------------------------------------------------------------------------------------------------------------------ colour ops
HUE_BWD_FACTORS = (0.07, -0.07, 0.31, -0.31, 0.5, -0.5)
COLOR_BWD_CASES = R.COLOR_CASES + [("hue", R.OP_HUE, f) for f in HUE_BWD_FACTORS if f not in [c[2] for c in R.COLOR_CASES if c[1] == R.OP_HUE]]


def pixel_bands(H=160):
    """[(name, row indices)]: the bands of rows of _img_ref.hard_pixels, one kind of pixel each"""
    b = H // 10
    rows = lambda a, e: torch.arange(a, e)          # noqa: E731
    return [("random", torch.cat([rows(0, b), rows(5 * b + 3 * (b // 3), 6 * b)])), ("grey", rows(b, 2 * b)), ("tie01", rows(2 * b, 3 * b)),
            ("tie02", rows(3 * b, 4 * b)), ("tie12", rows(4 * b, 5 * b)), ("neargrey", rows(5 * b, 5 * b + 3 * (b // 3))),
            ("corners", rows(6 * b, 7 * b)), ("edge", rows(7 * b, 8 * b)), ("dark", rows(8 * b, H))]


def contrast_frames():
    """[3, 3, 300, 300] 8-bit noise, each frame a different mean: more than 65536 pixels (the strided pass of the contrast partial sums)"""
    g = torch.Generator().manual_seed(9)
    x = torch.rand(3, 3, 300, 300, generator=g) * torch.tensor([1.0, 0.7, 0.4]).view(3, 1, 1, 1)
    return (x * 255).round() / 255


def color_pre(x, op, factor, dt, gray0=0.2989, mag=False):
    """the pre-clamp value f x + (1 - f) ref of brightness / contrast / saturation (_img_ref._blend)"""
    x = x.to(dt)
    coef = (gray0,) + R.GRAY_TV[1:]
    f = _k(factor, dt)
    if op == R.OP_BRIGHTNESS:
        ref = torch.zeros_like(x)
    elif op == R.OP_CONTRAST:
        ref = one_thread(lambda: torch.mean(R._gray(x, dt, coef), dim=(-3, -2, -1), keepdim=True))
    else:
        ref = R._gray(x, dt, coef)
    return (f * x + (1 - f) * ref, f.abs() * x.abs() + (1 - f).abs() * ref.abs()) if mag else f * x + (1 - f) * ref


def color_flags(x, op, factor):
    """flagged elements of a blend op's gate (float64 value, fp32 witness of the exact cases, band relative to the terms' magnitudes)"""
    with torch.no_grad():
        v64, m64 = color_pre(x, op, factor, F64, mag=True)
        return gate_flags(v64, color_pre(x, op, factor, F32), m64)


def color_adjoint(x, dy, op, factor, dt, flip=None, strict=False, no_coupling=False, unmasked_sum=False, gray0=0.2989):
    """closed form of the adjoint of brightness / contrast / saturation / grayscale with the gates written out (bwd_shell.hip::color_bwd_kernel's
    expression); flip: gates to invert.  DEFECTS: strict = 0 < v < 1; no_coupling = contrast without the term through the frame mean;
    unmasked_sum = that term summed over closed gates too; gray0 = 0.299"""
    dy = dy.to(dt)
    f = _k(factor, dt)
    if op == R.OP_GRAYSCALE:
        return torch.stack([_k(c, dt) for c in (0.299, 0.587, 0.114)]).view(3, 1, 1) * dy.sum(1, keepdim=True)
    v = color_pre(x, op, factor, dt, gray0)
    gate = ((v > 0) & (v < 1)) if strict else ((v >= 0) & (v <= 1))
    if flip is not None:
        gate = gate ^ flip
    pg = dy * gate
    w = torch.stack([_k(c, dt) for c in (gray0,) + R.GRAY_TV[1:]]).view(3, 1, 1)
    if op == R.OP_BRIGHTNESS:
        return f * pg
    if op == R.OP_SATURATION:
        return f * pg + (1 - f) * w * pg.sum(1, keepdim=True)
    s = one_thread(lambda: (dy if unmasked_sum else pg).sum((1, 2, 3), keepdim=True))
    coup = torch.zeros_like(s) if no_coupling else (1 - f) * s / (x.shape[-1] * x.shape[-2])
    return f * pg + w * coup


def hue_fwd(x, factor, dt, tie_last=False, parts=False):
    """_img_ref.color_op's hue with the arg-max / arg-min channel written out (max and min send their gradient there: the first index on ties, as
    autograd does).  DEFECT: tie_last = the last index.  parts: (h6, [p, q, t] before their clamps) instead of the image"""
    x = x.to(dt)
    r, g, b = x.unbind(-3)
    xs = x.detach()
    imax, imin = (2 - xs.flip(-3).argmax(-3), 2 - xs.flip(-3).argmin(-3)) if tie_last else (xs.argmax(-3), xs.argmin(-3))
    maxc, minc = x.gather(-3, imax.unsqueeze(-3)).squeeze(-3), x.gather(-3, imin.unsqueeze(-3)).squeeze(-3)
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0) + _k(factor, dt)
    h = h - torch.floor(h)
    v = maxc
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.long() % 6
    pu, qu, tu = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    if parts:
        return h * 6.0, [pu, qu, tu], i, s
    p, q, t = pu.clamp(0, 1), qu.clamp(0, 1), tu.clamp(0, 1)
    tab = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    z = torch.zeros_like(v)
    out = [z, z, z]
    for k, rgb in enumerate(tab):
        out = [torch.where(i == k, rgb[c], out[c]) for c in range(3)]
    return torch.stack(out, -3)


def hue_flags(x, factor):
    """[F, 1, H, W] bool: pixels whose float64 h6 is within HUE_SECTOR_BAND of a sector boundary, or whose p, q or t -- where the sector reads
    it -- is within HUE_GATE_BAND of a clamp bound, without being exact in both precisions"""
    with torch.no_grad():
        h64, pqt64, i64, s64 = hue_fwd(x, factor, F64, parts=True)
        h32, pqt32, _, _ = hue_fwd(x, factor, F32, parts=True)
    flag = near(h64, h32, h64.round(), HUE_SECTOR_BAND)
    uses = [(0, 1, 2, 3, 4, 5), (1, 3, 5), (0, 2, 4)]          # sectors that read p, q, t
    vmax = x.double().amax(-3)
    mq = vmax * (s64 + 2.0 ** -5)
    for v64, v32, sec, band, mag in zip(pqt64, pqt32, uses, (HUE_P_BAND, HUE_GATE_BAND, HUE_GATE_BAND), (vmax, mq, mq)):
        used = torch.zeros_like(flag)
        for k in sec:
            used |= i64 == k
        flag |= used & gate_flags(v64, v32, mag, band)
    return flag.unsqueeze(-3)


def hue_pixels(factor):
    """(hard_pixels for this shift, names of the bands whose pixels were changed): where 6 x factor is an integer every tied pair and every corner
    of the cube sits on a sector boundary, so a band whose flagged share exceeds FLAG_SHARE gets fresh random pixels (the cap never moves)"""
    x = R.hard_pixels()
    flag = hue_flags(x, factor)
    g = torch.Generator().manual_seed(77)
    changed = []
    for name, rows in pixel_bands(x.shape[-2]):
        if float(flag[:, :, rows].float().mean()) > FLAG_SHARE:
            x[:, :, rows] = torch.rand(x.shape[0], 3, len(rows), x.shape[-1], generator=g)
            changed.append(name)
    return x, changed


def band_lines(got, own, rows_of, other=None, amb=None, keep=None):
    """[(band, error)] of masked_err per band of rows"""
    sl = lambda t, rows: None if t is None else t[:, :, rows]          # noqa: E731
    return [(name, masked_err(got[:, :, rows], own[:, :, rows], sl(other, rows), sl(amb, rows), sl(keep, rows))) for name, rows in rows_of]


def color_ref(x, dy, op, factor):
    """(own64, other64 or None, flagged elements or None, keep mask or None, yardstick32) of one colour adjoint: own and the yardstick by autograd
    of _img_ref.color_op; a flagged element of a pointwise gate may match the closed form with its gate inverted; flagged hue pixels are left out"""
    own, y32 = adjoint_pair(lambda t, dt: R.color_op(t, op, factor, dt), x, dy)
    if op == R.OP_GRAYSCALE:
        return own, None, None, None, y32
    if op == R.OP_HUE:
        return own, None, None, ~hue_flags(x, factor), y32
    amb = color_flags(x, op, factor)
    if op == R.OP_SATURATION:          # a pixel's channels share the masked sum: every channel of a flagged pixel may take either candidate
        amb_px = amb.any(1, keepdim=True).expand_as(amb)
        return own, color_adjoint(x, dy, op, factor, F64, flip=amb), amb_px, None, y32
    return own, color_adjoint(x, dy, op, factor, F64, flip=amb), amb, None, y32


# ------------------------------------------------------------------------------------------------------------------------ perceptual mse / yuv
YUV = (0.299, 0.587, 0.114, -0.14713, -0.28886, 0.436, 0.615, -0.51499, -0.10001)          # data/transforms.py:46-48, the kernel's fp32 values
PERCEP_SHAPES = [(3, 300, 300), (1, 5, 7)]          # 270000 pixels: beyond the 1024 blocks x 256 threads of the partial sums; one tiny frame


def percep(imgs, imgs_w, yuv, dt):
    """losses/perceptual.py:20-28, yuvloss.py:11-27: mean((T (imgs_w - imgs))^2)"""
    e = imgs_w.to(dt) - imgs.to(dt)
    if yuv:
        e = torch.einsum("rc,fchw->frhw", torch.tensor(YUV, dtype=F32).view(3, 3).to(dt), e)
    return one_thread(lambda: (e * e).mean())


def percep_grad32(imgs, imgs_w, yuv, transposed=True):
    """fp32 closed form 2 T^T T e / n.  DEFECT: transposed = False (T in place of T^T)"""
    e = imgs_w - imgs
    if yuv:
        T = torch.tensor(YUV, dtype=F32).view(3, 3)
        e = torch.einsum("cr,frhw->fchw", T.t() if transposed else T, torch.einsum("rc,fchw->frhw", T, e))
    return e * torch.tensor(2.0 / e.numel(), dtype=F32)


def percep_inputs(Fn, H, W, kind):
    """(imgs, imgs_w): "noise" = a 0.01 perturbation of random frames; "tiny" = differences of order 1e-7 on a 0.9 background; "same" = identical"""
    g = torch.Generator().manual_seed(2500 + Fn + H + W)
    if kind == "noise":
        imgs = torch.rand(Fn, 3, H, W, generator=g)
        return imgs, imgs + 0.01 * torch.randn(Fn, 3, H, W, generator=g)
    imgs = torch.full((Fn, 3, H, W), 0.9)
    return imgs, (imgs + 1e-7 * torch.randn(Fn, 3, H, W, generator=g)) if kind == "tiny" else imgs.clone()
