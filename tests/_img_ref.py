"""fp64 envelopes of the IMAGE-DOMAIN forward kernels (csrc/shell.hip: vs_resize_pre, vs_resize_pre_u8, vs_jnd_heatmap, vs_embed_tail; csrc/aug.hip:
colour ops, resizes, blur, median, warp, blends, temporal ops): formulas, hard frames, cases and the metric shared by
tests/test_img_contract_cpu.py (the envelope has teeth; no GPU) and tests/test_gpu_img_envelope.py (every kernel against it).

As in tests/_fwd_ref.py (the rule and the metrics frame_err / cand_err are tests/_envelope.py's): the reference is the formula in float64 on the
CPU from the same fp32 input values and the same fp32 coefficient values the kernel receives, the yardstick is the same formula in float32 on the CPU.  The error is taken PER (case, frame kind):
max |got - ref64| / max(max |ref64|, tiny) over the whole output, against the yardstick's figure for the same frame kind -- every kind has its own
line, so that noise's larger yardstick cannot hide an error on a structured frame.  A kernel may exceed the yardstick by IMG_FP64_MARGIN; no element
is excluded from any case: where the operation is discontinuous (nearest warp at a .5 boundary, the JND luminance mask at la = 127) a pixel inside a
band whose width follows from the fp32 coordinate error gets a candidate set instead (nearest_check, cand_err)."""
import functools
import math

import torch
import torch.nn.functional as F

from tests._envelope import check_rows, one_thread

# Twice the largest ratio hip / max(yardstick, 2^-24) measured on an MI355X over every line of tests/test_gpu_img_envelope.py
# (profiles/img_fp64_envelope.txt lists them), never more than 8: a kernel that needs more has a defect.
IMG_FP64_MARGIN = 8.0          # min(2 x 4.328, cap): the largest ratio measured is vs_aug_warp bilinear, rotate 45 on 8 x 300, `ramp` (996 lines)
F32, F64 = torch.float32, torch.float64
envelope = functools.partial(check_rows, "IMG-ENVELOPE", 58, "cpu-fp32", IMG_FP64_MARGIN)


def f32(v):
    """the fp32 value a `float` kernel argument holds, as a python float"""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------------------------------------------------------------ hard inputs
CONST = (0.3, 0.7)             # non-dyadic: a resampler must return them to within rounding, so any normalisation defect shows
FRAME_KINDS = ("noise", "checker", "const", "ramp", "impulse")


def hard_frames(H, W, seed=0):
    """{kind: [2, 3, H, W] float32}, the two frames of every kind different"""
    g = torch.Generator().manual_seed(1700 + 131 * H + W + seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = {"noise": torch.rand(2, 3, H, W, generator=g)}
    ck = ((yy + xx) % 2).float()
    out["checker"] = torch.stack([ck, 1 - ck])[:, None].expand(2, 3, H, W).contiguous()
    out["const"] = torch.stack([torch.full((3, H, W), CONST[0]), torch.full((3, H, W), CONST[1])])
    rx, ry = xx.float() / max(W - 1, 1), yy.float() / max(H - 1, 1)
    out["ramp"] = torch.stack([torch.stack([0.6 * rx + 0.3 * ry, 0.9 * rx, 0.9 * ry]), torch.stack([1 - rx, 1 - 0.5 * (rx + ry), 0.25 + 0.5 * ry])])
    imp = torch.zeros(2, 3, H, W)
    for f in range(2):
        imp[f, 0, f::5, (2 * f)::7] = 1.0          # ones on a 7 x 5 lattice (frame 1: shifted)
        imp[f, 1, 0] = imp[f, 1, -1] = 1.0         # first and last row
        imp[f, 2, :, 0] = imp[f, 2, :, -1] = 1.0   # first and last column: the output is the border taps' weights themselves
    imp[1] *= 0.75
    out["impulse"] = imp
    return out


def hard_pixels(Fn=3, H=160, W=256, seed=5):
    """[Fn, 3, H, W] for the colour ops: random pixels, grey pixels, each pair of channels tied, grey with one channel one ulp up or scaled by
    (1 - 1e-6), the cube's corners, values of 1e-6 and 1 - 1e-6 -- one kind per band of rows; each frame scaled differently (different means)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(Fn, 3, H, W, generator=g)
    b = H // 10
    gray = torch.rand(Fn, 1, H, W, generator=g)
    x[:, :, b:2 * b] = gray[:, :, b:2 * b]                                          # r = g = b
    for i, (p, q) in enumerate(((0, 1), (0, 2), (1, 2))):                            # pairs tied (the hue's maxc == r / maxc == g branches)
        x[:, q, (2 + i) * b:(3 + i) * b] = x[:, p, (2 + i) * b:(3 + i) * b]
    for c in range(3):                                                              # grey with one channel one ulp up / scaled by 1 - 1e-6
        band = slice(5 * b + c * (b // 3), 5 * b + (c + 1) * (b // 3))
        v = gray[:, 0, band].clamp(0.05, 0.95)
        x[:, :, band] = v[:, None]
        x[:, c, band, ::2] = torch.nextafter(v, torch.ones_like(v))[..., ::2]
        x[:, c, band, 1::2] = (v * (1 - 1e-6))[..., 1::2]
    corners = torch.tensor([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=F32)         # the cube's corners
    x[:, :, 6 * b:7 * b] = corners.t()[None, :, None, :].repeat(1, 1, 1, W // 8 + 1)[..., :W].expand(Fn, 3, b, W)
    x[:, :, 7 * b:8 * b] = torch.where(torch.rand(Fn, 3, b, W, generator=g) < 0.5, torch.tensor(1e-6), torch.tensor(1 - 1e-6))
    for f in range(Fn):                                                             # rows 8b..: random pixels, darker in later frames
        x[f, :, 8 * b:] *= 1.0 - 0.3 * f
    return x.contiguous()


def jnd_frames(H, W, seed=0):
    """frames for the JND heat-map: noise, checker, flat (two greys), black and `jump` = 0.498 + 0.01 randn (255 x ~ 127: the branch of jnd.py:66-68)"""
    g = torch.Generator().manual_seed(1800 + 131 * H + W + seed)
    hf = hard_frames(H, W, seed)
    return {"noise": hf["noise"], "checker": hf["checker"], "flat": hf["const"], "black": torch.zeros(2, 3, H, W),
            "jump": (0.498 + 0.01 * torch.randn(2, 3, H, W, generator=g)).clamp_(0, 1)}


# ------------------------------------------------------------------------------------------------------------------------ bilinear resize
def resize_matrix(n_in, n_out, aa, dt, defect=None):
    """[n_out, n_in]: ATen's separable bilinear weights (aten/native/cpu/UpSampleKernel.cpp; csrc/resize_taps.h) in dtype dt: antialias = triangle
    filter of support max(scale, 1), normalised over the taps inside the input; plain = two taps, align_corners=False, source clamped at 0.
    DEFECTS for the teeth test: "shift_last" = tap window shifted by one input pixel on the last output index only; "unclipped" = anti-alias
    weights normalised over the unclipped window; "nohalf" = src = scale i instead of scale (i + 0.5) - 0.5; "drop9" = the last tap dropped
    when the count exceeds 8"""
    scale = torch.tensor(float(n_in), dtype=dt) / torch.tensor(float(n_out), dtype=dt)
    i = torch.arange(n_out, dtype=dt)
    j = torch.arange(n_in, dtype=dt)
    half = 0.0 if defect == "nohalf" else 0.5
    if aa:
        support = scale if scale >= 1 else torch.ones((), dtype=dt)
        inv = 1 / scale if scale >= 1 else torch.ones((), dtype=dt)
        center = scale * (i + half) + (0.5 - half)
        lo_u, hi_u = (center - support + 0.5).trunc(), (center + support + 0.5).trunc()
        lo, hi = lo_u.clamp_min(0), hi_u.clamp_max(n_in)

        def tri(jj, l, h):
            t = ((jj[None, :] - center[:, None] + 0.5) * inv).abs()
            return torch.where((jj[None, :] >= l[:, None]) & (jj[None, :] < h[:, None]) & (t < 1), 1 - t, torch.zeros((), dtype=dt))
        w = tri(j, lo, hi)
        if defect == "unclipped":
            K = int(math.ceil(float(support))) + 2
            total = tri(torch.arange(-K, n_in + K, dtype=dt), lo_u, hi_u).sum(1, keepdim=True)
        else:
            total = w.sum(1, keepdim=True)
        M = w / total
        if defect == "drop9":
            n = (hi - lo).long()
            last = (hi - 1).long()
            rows = torch.nonzero(n > 8).flatten()
            M[rows, last[rows]] = 0
    else:
        src = (scale * (i + half) - half).clamp_min(0)
        i0 = src.trunc().clamp_max(n_in - 1)
        l1 = src - i0
        i0 = i0.long()
        M = torch.zeros(n_out, n_in, dtype=dt)
        r = torch.arange(n_out)
        inner = i0 < n_in - 1
        M[r, i0] = torch.where(inner, 1 - l1, torch.ones((), dtype=dt))
        M[r[inner], i0[inner] + 1] = l1[inner]
    if defect == "shift_last":
        M[-1] = torch.cat([M[-1, 1:], M[-1, :1] * 0])
    return M


def resize(x, size, aa, dt, defect=None, defect_axis="x"):
    """[..., H, W] -> [..., oh, ow] in dtype dt: rows first filtered horizontally, then vertically (the kernels' order); a defect applies to one axis"""
    H, W = x.shape[-2:]
    My = resize_matrix(H, size[0], aa, dt, defect if defect_axis == "y" else None)
    Mx = resize_matrix(W, size[1], aa, dt, defect if defect_axis == "x" else None)
    return one_thread(lambda: My @ (x.to(dt) @ Mx.t()))


def resize_ref(x, size, aa, **defect):
    """(float64 reference, float32 yardstick) of resize; with a defect keyword: (reference, defective fp32 emulation)"""
    return resize(x, size, aa, F64), resize(x, size, aa, F32, **defect)


YMAT = (0.299, 0.587, 0.114)


def resize_pre(x, size, aa, mul, add, step, ymat, dt, **defect):
    """vs_resize_pre: (rgb [B, C, oh, ow] * mul + add, key frames [ceil(B / step), 1 or 3, oh, ow] = Y (or rgb) * 2 - 1)"""
    r = resize(x, size, aa, dt, **defect)
    k = r[::step]
    if ymat is not None:
        y = [torch.tensor(v, dtype=F32).to(dt) for v in ymat]
        k = (y[0] * k[:, 0] + y[1] * k[:, 1] + y[2] * k[:, 2])[:, None]
    return r * torch.tensor(mul, dtype=F32).to(dt) + torch.tensor(add, dtype=F32).to(dt), k * 2 - 1


# (tag, H, W, oh, ow, antialias, development switches {key: value}): what each case reaches is in the tag
RESIZE_CASES = [
    ("stream<128> scalar loads 3.2:1", 93, 118, 29, 37, 1, {}),
    ("stream<128> 16-byte loads", 96, 128, 30, 40, 1, {}),
    ("stream<64> 3.9:1 vector loads", 100, 128, 25, 32, 1, {}),
    ("stream<64> 3.9:1 scalar loads", 101, 126, 26, 32, 1, {}),
    ("staged tile kernel", 93, 118, 29, 37, 1, {"RESIZE_FORM": 1}),
    ("unstaged tile path > 4:1", 70, 66, 13, 17, 1, {}),
    ("128 taps", 64, 64, 1, 1, 1, {}),
    ("up-scale aa", 5, 7, 64, 64, 1, {}),
    ("up-scale plain", 5, 7, 64, 64, 0, {}),
    ("one input row aa", 1, 9, 4, 33, 1, {}),
    ("one input row plain", 1, 9, 4, 33, 0, {}),
    ("up-scale where fp32 coordinates dominate", 93, 118, 130, 165, 1, {}),
    ("plain up", 31, 45, 64, 64, 0, {}),
    ("strip height 1", 96, 128, 30, 40, 1, {"RESIZE_STRIP": 1}),
    ("strip height 7", 96, 128, 30, 40, 1, {"RESIZE_STRIP": 7}),
    ("strip height 80 (taller than the weight table)", 96, 128, 30, 40, 1, {"RESIZE_STRIP": 80}),
]
RESIZE_IDENTITY = (33, 47)                                  # 33 x 47 -> 33 x 47: must be bit-equal to x * mul + add
RESIZE_U8_CASES = [(93, 118, 29, 37, 1), (94, 93, 30, 31, 1), (5, 7, 64, 64, 1)]
# vs_resize_nchw / vs_aug_crop_resize_color: (H, W, crop (i0, j0, ch, cw) or None, oh, ow, antialias)
PLANE_CASES = [(h, w, None, oh, ow, aa) for _, h, w, oh, ow, aa, sw in RESIZE_CASES if not sw] + [
    (96, 128, (5, 4, 64, 100), 40, 60, 1), (96, 128, (5, 5, 64, 100), 40, 60, 1), (96, 128, (5, 6, 64, 100), 40, 60, 1),
    (96, 128, (5, 7, 64, 100), 40, 60, 1),                  # j0 at residues 0-3 on a width-128 frame
    (96, 128, (33, 29, 63, 99), 50, 61, 1),                 # the crop's right / bottom edge is the frame's
    (200, 12, None, 16, 3, 1),                              # 12.5 : 1 and 4 : 1: both tap branches in one call (its tile window exceeds the LDS)
    (104, 8, None, 8, 8, 1),                                # 13 : 1 in y only, a window the tile form holds: its long-filter branch (27 taps) in y
]


# ------------------------------------------------------------------------------------------------------------------------ JND heat-map
JND_TAPS = ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1])
JND_DELTA = 127 * 2.0 ** -18   # band around the la = 127 jump: the fp32 la (a sum of 25 products of magnitude <= 255 x 2 / 32) is within 3.8e-5 of the float64 one
JND_SHAPES = [(70, 101), (5, 7), (33, 32), (32, 33)]


def jnd(x, dt, taps=JND_TAPS, thr=127.0, gy_sum=False):
    """jnd.py:24-108 on [B, 3, H, W] in dtype dt.  Returns (heat-map [B, 1, H, W] with each pixel on its own branch, the same with every pixel
    on the OTHER branch of the luminance mask, la before the branch).  DEFECTS: thr = the threshold (128); gy_sum = Sobel gy sign-symmetric"""
    x = x.to(dt)
    t = torch.tensor(taps, dtype=F32).to(dt)          # taps43: the fp32 values the kernel receives; the formula's own constants stay python numbers
    kl, kx, ky = t[:25].view(1, 1, 5, 5), t[25:34].view(1, 1, 3, 3), t[34:43].view(1, 1, 3, 3)
    if gy_sum:
        ky = ky.abs()
    lum = 0.299 * (255 * x[:, 0:1]) + 0.587 * (255 * x[:, 1:2]) + 0.114 * (255 * x[:, 2:3])
    la = one_thread(lambda: F.conv2d(lum, kl, padding=2)) / 32
    low = 17 * (1 - torch.sqrt(la / 127 + 1e-5))
    high = 3 / 128 * (la - 127) + 3
    gx, gy = one_thread(lambda: (F.conv2d(lum, kx, padding=1), F.conv2d(lum, ky, padding=1)))
    cm = torch.sqrt(gx ** 2 + gy ** 2)
    # (cm ** 2.4: in float32 ATen takes the exponent as 2.4f = 2.4 + 9.5e-8, which moves a Sobel magnitude of 700 by 6e-7 -- the yardstick's own
    # cost on frames with strong edges, and what the kernels' 2.4f * log2(cm) does as well)
    cm = 0.117 * (16 * cm ** 2.4 / (cm ** 2 + 26 ** 2))

    def fin(lv):
        return torch.clamp_min(lv + cm - 0.3 * torch.minimum(lv, cm), 0) / 255
    sel = la <= thr
    return fin(torch.where(sel, low, high)), fin(torch.where(sel, high, low)), la


def jnd_ref(x, **defect):
    """(own64, other64, ambiguous mask, yardstick fp32 own): a pixel whose float64 la is within JND_DELTA of 127 may match either branch"""
    own, other, la = jnd(x, F64)
    return own, other, (la - 127).abs() <= JND_DELTA, jnd(x, F32, **defect)[0]


# ------------------------------------------------------------------------------------------------------------------------ embed tail
def key_expand(delta, Fn, step, mode, total_key, dt, tail_weight_defect=False):
    """videoseal.py:80-118: [Fn, Cd, S, S] from the key frames [total_key, Cd, S, S]; mode 0 repeat, 1 alternate, 2 interpolate.
    DEFECT: key-frame weight j / step instead of j / (step - 1)"""
    delta = delta.to(dt)
    out = []
    for f in range(Fn):
        ka, kb, wa, wb = f // step, 0, 1.0, 0.0
        if mode == 1:
            wa = 1.0 if f % step == 0 else 0.0
        elif mode == 2:
            ninter = ((Fn - 1) // step) * step
            if f < ninter:
                kb = ka + 1
                j = f % step
                lin = (torch.tensor(float(j), dtype=F32) / torch.tensor(float(step if tail_weight_defect else step - 1), dtype=F32)) if step > 1 else torch.zeros(())
                wa = 1 - lin
                wb = 1 - wa
                wa, wb = wa.to(dt), wb.to(dt)
            else:
                ka = total_key - 1
        ka, kb = min(ka, total_key - 1), min(kb, total_key - 1)
        out.append(wa * delta[ka] + wb * delta[kb])
    return torch.stack(out)


def embed_tail(imgs, delta, hm_low, cfg, dt, branch="own", **defect):
    """wam.py:182-197 / videoseal.py:316-344 as vs_embed_tail states it.  cfg: dict(step, mode, total_key, attenuate, clamp, aa, si, sw).
    Returns (out [F, 3, H, W], preds_w [F, Cd, H, W]); branch = "other": every pixel's JND on the other side of the la = 127 jump.
    DEFECTS: tail_weight_defect (key_expand), no_clamp"""
    Fn, _, H, W = imgs.shape
    p = imgs.to(dt)
    d = key_expand(delta, Fn, cfg["step"], cfg["mode"], cfg["total_key"], dt, defect.get("tail_weight_defect", False))
    att = cfg["attenuate"]
    if att and hm_low is not None:
        d = d * hm_low.to(dt)[:, None]
    d = resize(d, (H, W), cfg["aa"], dt)
    si, sw = torch.tensor(cfg["si"], dtype=F32).to(dt), torch.tensor(cfg["sw"], dtype=F32).to(dt)
    full = att and hm_low is None
    hm = None
    if full:
        own, other, _ = jnd(imgs, dt)
        hm = own if branch == "own" else other
    if full and att != 2:
        d = hm * d
    v = si * p + sw * d
    if full and att == 2:
        v = p + hm * (v - p)
    if cfg["clamp"] and not defect.get("no_clamp", False):
        v = v.clamp(0, 1)
    return v, d


def tail_ref(imgs, delta, hm_low, cfg, **defect):
    """(own64 (out, preds), other64 (out, preds), ambiguous mask [F, 1, H, W] or None, fp32 yardstick (out, preds))"""
    own = embed_tail(imgs, delta, hm_low, cfg, F64)
    full = cfg["attenuate"] and hm_low is None
    if full:
        other = embed_tail(imgs, delta, hm_low, cfg, F64, branch="other")
        amb = (jnd(imgs, F64)[2] - 127).abs() <= JND_DELTA
    else:
        other, amb = own, torch.zeros(imgs.shape[0], 1, *imgs.shape[-2:], dtype=torch.bool)
    return own, other, amb, embed_tail(imgs, delta, hm_low, cfg, F32, **defect)


def tail_frames(Fn, H, W, seed=0):
    """{kind: [Fn, 3, H, W]}: noise, flat (a different grey per frame), jump"""
    g = torch.Generator().manual_seed(1900 + 131 * H + W + seed)
    flat = torch.stack([torch.full((3, H, W), 0.2 + 0.6 * f / max(Fn - 1, 1)) for f in range(Fn)])
    return {"noise": torch.rand(Fn, 3, H, W, generator=g), "flat": flat,
            "jump": (0.498 + 0.01 * torch.randn(Fn, 3, H, W, generator=g)).clamp_(0, 1)}


def tail_inputs(Fn, Cd, S, step, seed=0):
    g = torch.Generator().manual_seed(2000 + Fn + Cd + S + seed)
    nkey = (Fn + step - 1) // step
    return 0.3 * torch.randn(nkey, Cd, S, S, generator=g), torch.rand(Fn, S, S, generator=g)


def _tc(step=1, mode=0, total_key=None, attenuate=1, clamp=1, aa=1, si=1.0, sw=0.2):
    return dict(step=step, mode=mode, total_key=total_key, attenuate=attenuate, clamp=clamp, aa=aa, si=si, sw=sw)


# (tag, F, H, W, S, Cd, low-res heat-map?, preds_w?, cfg)
TAIL_CASES = [
    ("staged 2.8x full jnd", 5, 45, 301, 16, 1, False, False, _tc()),
    ("attenuate 2 + preds_w", 5, 45, 301, 16, 1, False, True, _tc(attenuate=2)),
    ("attenuate 0 Cd 3", 5, 45, 301, 16, 3, False, False, _tc(attenuate=0)),
    ("alternate step 2 lowres hmap", 5, 45, 301, 16, 1, True, False, _tc(step=2, mode=1, total_key=3)),
    ("interpolate step 2 Cd 3", 5, 45, 301, 16, 3, False, False, _tc(step=2, mode=2, total_key=3)),
    ("repeat step 2 both clamps act", 5, 45, 301, 16, 1, False, False, _tc(step=2, mode=0, total_key=3, attenuate=0, sw=3.0)),
    ("1.5x unstaged taps", 2, 24, 40, 16, 1, False, False, _tc()),
    ("delta down-resized", 2, 9, 12, 16, 1, False, False, _tc()),
    ("5x7 frames", 2, 5, 7, 16, 3, False, False, _tc(attenuate=0)),
]


# ------------------------------------------------------------------------------------------------------------------------ colour ops
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_GRAYSCALE = range(5)
GRAY_TV = (0.2989, 0.587, 0.114)
COLOR_CASES = ([("brightness", OP_BRIGHTNESS, v) for v in (0.1, 0.5, 1.5, 2.0)] + [("contrast", OP_CONTRAST, v) for v in (0.1, 0.5, 1.5, 2.0)]
               + [("saturation", OP_SATURATION, v) for v in (0.0, 0.5, 1.5, 2.0)]
               + [("hue", OP_HUE, v) for v in (-0.5, -0.4, -0.1, 0.1, 0.25, 1.0 / 3.0, 0.5)] + [("grayscale", OP_GRAYSCALE, 0.0)])
COLOR_CHAIN = [(OP_CONTRAST, 1.5), (OP_BRIGHTNESS, 0.5), (OP_SATURATION, 1.5), (OP_HUE, 0.1)]        # contrast leads: it needs the mean of its input
CROP_CHAIN = [(OP_BRIGHTNESS, 0.5), (OP_SATURATION, 1.4), (OP_HUE, 0.1)]                              # the epilogue of vs_aug_crop_resize_color


def _k(v, dt):
    return torch.tensor(v, dtype=F32).to(dt)


def _gray(x, dt, coef=GRAY_TV):
    r, g, b = x.unbind(-3)
    return (_k(coef[0], dt) * r + _k(coef[1], dt) * g + _k(coef[2], dt) * b).unsqueeze(-3)


def _blend(a, b, f, dt):
    f = _k(f, dt)
    return (f * a + (1 - f) * b).clamp(0, 1)


def color_op(x, op, factor, dt, gray0=0.2989, shared_mean=False, c_fmod=False):
    """torchvision _functional_tensor semantics (oracle/augment.py) in dtype dt with the kernel's fp32 constants.  DEFECTS: gray0 = 0.299 in
    saturation / contrast; shared_mean = contrast mean of frame 0 for all frames; c_fmod = C remainders (toward zero) in the hue shift: the hue
    fmod(h + f, 1) and the sector fmod(i, 6) stay negative for negative shifts"""
    x = x.to(dt)
    coef = (gray0,) + GRAY_TV[1:]
    if op == OP_BRIGHTNESS:
        return _blend(x, torch.zeros_like(x), factor, dt)
    if op == OP_CONTRAST:
        mean = one_thread(lambda: torch.mean(_gray(x, dt, coef), dim=(-3, -2, -1), keepdim=True))
        if shared_mean:
            mean = mean[:1].expand_as(mean)
        return _blend(x, mean, factor, dt)
    if op == OP_SATURATION:
        return _blend(x, _gray(x, dt, coef), factor, dt)
    if op == OP_GRAYSCALE:
        return _gray(x, dt, (0.299, 0.587, 0.114)).expand_as(x)
    r, g, b = x.unbind(-3)
    maxc, minc = x.max(-3).values, x.min(-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = h + _k(factor, dt)
    h = torch.fmod(h, 1.0) if c_fmod else h - torch.floor(h)
    v = maxc
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = torch.fmod(i, 6).long() if c_fmod else i.long() % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    z = torch.zeros_like(v)
    tab = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = [z, z, z]
    for k, rgb in enumerate(tab):
        out = [torch.where(i == k, rgb[c], out[c]) for c in range(3)]
    return torch.stack(out, -3)


def color_chain(x, ops, dt, **defect):
    for op, f in ops:
        x = color_op(x, op, f, dt, **defect)
    return x


# ------------------------------------------------------------------------------------------------------------------------ blur / median
BLUR_KS = (3, 9, 17, 33)


def blur_sigma(k):
    """valuemetric.py: torchvision's default when sigma is None"""
    return 0.3 * ((k - 1) * 0.5 - 1) + 0.8


def gaussian_blur(x, k, dt, pad_mode="reflect", sigma_from_k=False):
    """torchvision gaussian_blur (valuemetric.py:53-71) in dtype dt from the fp32 sigma the kernel receives, separable: rows, then columns.
    DEFECTS: pad_mode = "symmetric" (edge pixel repeated); sigma_from_k = sigma derived from k instead of (k - 1) / 2"""
    sigma = _k(0.3 * (k - 1) + 0.8 if sigma_from_k else blur_sigma(k), dt)
    half = (k - 1) * 0.5
    t = torch.linspace(-half, half, steps=k, dtype=dt)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    k1 = pdf / pdf.sum()
    x = x.to(dt)
    C = x.shape[-3]
    p = k // 2
    if pad_mode == "reflect":
        xp = F.pad(x, (p, p, p, p), mode="reflect")
    else:
        idx = lambda n: torch.cat([torch.arange(p - 1, -1, -1), torch.arange(n), torch.arange(n - 1, n - 1 - p, -1)])          # noqa: E731
        xp = x[..., idx(x.shape[-2]), :][..., idx(x.shape[-1])]
    return one_thread(lambda: F.conv2d(F.conv2d(xp, k1.view(1, 1, 1, k).expand(C, 1, 1, k), groups=C), k1.view(1, 1, k, 1).expand(C, 1, k, 1), groups=C))


def median_filter(x, k):
    """utils/image.py:60-84 in float64: median of the k row medians of the zero-padded window (selection only: exact in any dtype)"""
    p = k // 2
    xp = F.pad(x.double(), (p, p, p, p))
    return xp.unfold(2, k, 1).unfold(3, k, 1).median(dim=-1).values.median(dim=-1).values


# ------------------------------------------------------------------------------------------------------------------------ warp
ROT_ANGLES = (5, 10, 30, 45, -17, 100)
ROT_SHAPES = ((93, 118), (33, 47), (8, 300))
ROT90_SHAPES = ((93, 118), (92, 118))                       # odd x even: every coordinate is a tie; even x even: an exact permutation
PERSP_CASES = ((93, 118, 0.1), (93, 118, 0.5), (33, 47, 0.1), (33, 47, 0.5))
ROT_SHARE, JND_SHARE = 0.03, 0.01                            # conditions on the float64 reference alone: the largest ambiguous share allowed


def rotate_coeffs(angle, H, W):
    """the six fp32 coefficients augmentation.rotate hands to vs_aug_warp (torchvision _get_inverse_affine_matrix + _gen_affine_grid's rescale)"""
    rot = math.radians(-angle)
    a, b, c, d = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    th = torch.tensor([d, -b, 0.0, -c, a, 0.0], dtype=F32).view(2, 3)
    resc = th.t() / torch.tensor([0.5 * W, 0.5 * H], dtype=F32)
    return [float(resc[k][0]) for k in range(3)] + [float(resc[k][1]) for k in range(3)]


def rot90_size(H, W):
    """(oh, ow) of a 90-degree turn with expand=True (torchvision _compute_affine_output_size, restated in oracle/augment.py)"""
    from oracle import augment as A
    ow, oh = A._affine_output_size(A._inverse_rotate_matrix(90), W, H)
    return oh, ow


def perspective_points(W, H, scale, seed=3):
    """geometric.py:127-183 get_perspective_params under a fixed seed (the draws of tests/test_gpu_aug.py::test_perspective)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi, size=(1,), generator=g).item())          # noqa: E731
    hh, hw = H // 2, W // 2
    tl = [ri(0, int(scale * hw) + 1), ri(0, int(scale * hh) + 1)]
    tr = [ri(W - int(scale * hw) - 1, W), ri(0, int(scale * hh) + 1)]
    br = [ri(W - int(scale * hw) - 1, W), ri(H - int(scale * hh) - 1, H)]
    bl = [ri(0, int(scale * hw) + 1), ri(H - int(scale * hh) - 1, H)]
    return [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], [tl, tr, br, bl]


def perspective_coeffs(startpoints, endpoints):
    """torchvision _get_perspective_coeffs: least squares in float64, the eight results cast to fp32"""
    a = torch.zeros(8, 8, dtype=F64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b = torch.tensor(startpoints, dtype=F64).view(8)
    return torch.linalg.lstsq(a, b, driver="gels").solution.to(F32).tolist()


def warp_grid(kind, coeffs, H, W, oh, ow, dt):
    """(gx, gy) [oh, ow]: torchvision's normalised sampling grid (_gen_affine_grid / _perspective_grid) in dtype dt from the fp32 coefficients"""
    t = [torch.tensor(v, dtype=F32).to(dt) for v in coeffs]
    ox, oy = torch.arange(ow, dtype=dt)[None, :], torch.arange(oh, dtype=dt)[:, None]
    if kind == 0:
        bx, by = ox + (0.5 - ow * 0.5), oy + (0.5 - oh * 0.5)
        return (bx * t[0] + by * t[1]) + t[2], (bx * t[3] + by * t[4]) + t[5]
    bx, by = ox + 0.5, oy + 0.5
    n1 = (bx * (t[0] / (0.5 * ow)) + by * (t[1] / (0.5 * ow))) + t[2] / (0.5 * ow)
    n2 = (bx * (t[3] / (0.5 * oh)) + by * (t[4] / (0.5 * oh))) + t[5] / (0.5 * oh)
    den = (bx * t[6] + by * t[7]) + 1.0
    return n1 / den - 1.0, n2 / den - 1.0


def warp_coords(kind, coeffs, H, W, oh, ow, dt):
    """(ix, iy) [oh, ow]: source pixel coordinates of every output pixel (grid_sample's un-normalisation, align_corners=False)"""
    gx, gy = warp_grid(kind, coeffs, H, W, oh, ow, dt)
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2


def warp_bilinear(x, kind, coeffs, oh, ow, dt, clamp_taps=False):
    """[P, H, W] -> [P, oh, ow]: the grid in dtype dt + ATen grid_sample (bilinear, zeros, align_corners=False) on the CPU.
    DEFECT: clamp_taps = taps outside the frame clamped to the border instead of zero"""
    P, H, W = x.shape
    grid = torch.stack(torch.broadcast_tensors(*warp_grid(kind, coeffs, H, W, oh, ow, dt)), -1)[None]
    return one_thread(lambda: F.grid_sample(x.to(dt)[None], grid, mode="bilinear", padding_mode="border" if clamp_taps else "zeros", align_corners=False))[0]


def _pick(x, rx, ry):
    """x[:, ry, rx] with zero outside the frame"""
    H, W = x.shape[-2:]
    ok = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    v = x[:, ry.clamp(0, H - 1).long(), rx.clamp(0, W - 1).long()]
    return torch.where(ok[None], v, torch.zeros((), dtype=x.dtype))


def nearest_delta(H, W):
    """band around a .5 boundary in which the fp32 coordinate may round to either side: max(H, W) 2^-20 px (coordinates up to max(H, W), a few
    fp32 roundings of 2^-24 relative each; the fp32 oracle grid is at most 3.0e-5 px from the float64 one over the cases of this file)"""
    return max(H, W) * 2.0 ** -20


def nearest_candidates(x, kind, coeffs, oh, ow, delta=None):
    """(candidates [4, P, oh, ow], ambiguous mask [oh, ow]) of a nearest warp of x [P, H, W] from the float64 coordinates: a pixel farther than
    delta from every .5 boundary has four identical candidates (the float64-chosen source pixel, zero off the frame); a pixel within delta has
    the neighbouring choices"""
    P, H, W = x.shape
    ix, iy = warp_coords(kind, coeffs, H, W, oh, ow, F64)
    dl = nearest_delta(H, W) if delta is None else delta
    xs, ys = (torch.round(ix - dl), torch.round(ix + dl)), (torch.round(iy - dl), torch.round(iy + dl))
    amb = (xs[0] != xs[1]) | (ys[0] != ys[1])
    return torch.stack([_pick(x, rx, ry) for rx in xs for ry in ys]), amb


def nearest_check(got, cand):
    """number of pixels of got [P, oh, ow] that equal none of their candidates"""
    return int((~(got.cpu()[None] == cand).any(0)).sum())


def warp_nearest32(x, kind, coeffs, oh, ow, half_away=False):
    """the fp32 oracle: fp32 grid + nearest pick (nearbyint = half to even).  DEFECT: half_away = rounding half away from zero"""
    H, W = x.shape[-2:]
    ix, iy = warp_coords(kind, coeffs, H, W, oh, ow, F32)
    rnd = (lambda v: torch.sign(v) * torch.floor(v.abs() + 0.5)) if half_away else torch.round
    return _pick(x, rnd(ix), rnd(iy))


HALF_PIXEL_SHIFT = ([0.25, 0.0, 0.125, 0.0, 0.125, 0.0625], 16, 8)
# (coeffs, H, W): an affine map whose arithmetic is exact in fp32 AND float64 (dyadic coefficients, W = 8, H = 16): ix = ox + 0.5, iy = oy + 0.5 exactly
# -- every coordinate is an exact tie in both precisions, so there is no band: grid_sample's nearbyint (half to even) decides, and the result must
# equal the float64 choice bit for bit (delta = 0)


# ------------------------------------------------------------------------------------------------------------------------ pointwise / temporal
POINT_PLANES = [(1, 11), (93, 118), (1025, 1024)]           # a plane of 11 pixels, the fixture's, and one that gives the grid-stride loop a second pass


def window_average(x, half_window, alpha):
    """video.py:411-486 in fp32, written out: the window's frames summed in order, divided by the count, both products of the blend rounded"""
    Fn = x.shape[0]
    a32 = torch.tensor(alpha, dtype=F32)
    out = torch.empty_like(x)
    for i in range(Fn):
        a, b = max(0, i - half_window), min(Fn, i + half_window + 1)
        s = torch.zeros_like(x[0])
        for k in range(a, b):
            s = s + x[k]
        out[i] = (1 - a32) * x[i] + a32 * (s / float(b - a))
    return out


def crop_flip(x, i0, j0, h, w, flip):
    """geometric.py:94-124 / 186-196: window (i0, j0, h, w) of [P, H, W] with zero fill outside the frame, then the horizontal flip"""
    P, H, W = x.shape
    ry, rx = torch.arange(h) + i0, torch.arange(w) + j0
    if flip:
        rx = rx.flip(0)
    ok = ((ry >= 0) & (ry < H))[:, None] & ((rx >= 0) & (rx < W))[None, :]
    v = x[:, ry.clamp(0, H - 1)][:, :, rx.clamp(0, W - 1)]
    return torch.where(ok[None], v, torch.zeros(()))
