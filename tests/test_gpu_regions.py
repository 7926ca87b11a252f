"""Region-wise watermarks on the HIP path (include/videoseal_regions.h): vs_embed_tail_regions, vs_pixel_vote_regions (sized by
vs_pixel_vote_regions_partial_doubles), vs_label_boxes at the operator level; Videoseal.embed_regions / decode_regions / detect_regions at
the model level.

References: vs_embed_tail itself (a pixel of label r has the bits of the plain tail run with the plane sets of label r as delta; label 0 is
the input), vs_pixel_vote with the mask of one region, the float64 sum of the same fp32 logits, torch on the label map, `embed` /
`detect_images` of the model and the CPU oracle composed by videoseal_amd/regions.py.  Operands sit between red zones (tests/_guards.py).
Tail shapes (H, W, S): (37, 300, 16) two column tiles, a ragged last row band, an up-scale the row-streaming form of the plain tail takes;
(16, 16, 16) no resize; (9, 7, 16) a frame smaller than the maps; (40, 520, 24) three column tiles."""
import ctypes as C
import dataclasses
import itertools

import pytest
import torch

from oracle import videoseal_ref as O
from oracle.inputs import synthetic_frames, synthetic_msgs
from oracle.weights import make_state_dict, tiny_spec
from tests import _pixel_head_util as U
from tests import _pixel_ref as PR
from tests._guards import _guarded, _guards_intact, scratch, scratch_sentinel
from tests._model import TOL_IMG, cfg_of, make_model
from videoseal_amd import native as N
from videoseal_amd import regions as RG
from videoseal_amd.model import build_model
from videoseal_amd.pixel_head import pixel_vote

pytestmark = pytest.mark.gpu

SHAPES = [(37, 300, 16), (16, 16, 16), (9, 7, 16), (40, 520, 24)]
F_, STEP = 5, 2
KEYS = (F_ + STEP - 1) // STEP
MODES = (0, 1, 2)                                            # repeat, alternate, interpolate
ATTS = ("off", "lowres", "full")
VARIANTS = (1, 2, 4)                                         # 43-tap tiles, separable tiles, row-streaming (the plain tail's; the regions tail answers it with the separable tiles)
RS = (1, 3, 8)
PATTERNS = ("zeros", "all_r", "vstripes", "hstripes", "checker", "blocks", "missing", "above")
TAPS = (C.c_float * 43)(*([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1]))
OUT_FILL = {torch.float32: -7.0, torch.uint8: 0x5A}
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- tail
def _labels(pattern, H, W, R, k):
    """uint8 [F_, H, W]; k varies the pattern's free choice (which label, which one is missing)"""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    r = k % R + 1
    if pattern == "zeros":
        lab = torch.zeros(H, W, dtype=torch.int64)
    elif pattern == "all_r":
        lab = torch.full((H, W), r, dtype=torch.int64)
    elif pattern == "vstripes":
        lab = xx % (R + 1)
    elif pattern == "hstripes":
        lab = yy % (R + 1)
    elif pattern == "checker":
        lab = ((yy + xx) % 2) * ((yy // 2 + xx) % R + 1)
    elif pattern == "missing":                               # label r has no pixel (R = 1: nothing but background)
        lab = (yy + 2 * xx) % (R + 1)
        lab = torch.where(lab == r, torch.zeros_like(lab), lab)
    elif pattern == "above":                                 # R + 1 .. and 255 count as background
        lab = (3 * yy + xx) % (R + 4)
        lab = torch.where((yy + xx) % 11 == 0, torch.full_like(lab, 255), lab)
    else:
        lab = None
    if lab is not None:
        return lab.to(torch.uint8)[None].repeat(F_, 1, 1).contiguous()
    # blocks that end one pixel before, at and one pixel after the edge of a 16-row / 256-column tile, one offset per frame
    out = torch.zeros(F_, H, W, dtype=torch.uint8)
    for f in range(F_):
        o = f % 3 - 1
        out[f, : max(1, min(H, 16 + o)), : max(1, min(W, 256 + o))] = r
        out[f, min(H, 16 + o):, min(W, 256 + o):] = (r % R) + 1
    return out


def _tail_inputs(H, W, S, R, Cd, u8, seed):
    g = torch.Generator().manual_seed(seed)
    if u8:
        imgs = torch.randint(0, 256, (F_, H, W, 3), generator=g, dtype=torch.uint8)
    else:
        imgs = torch.rand(F_, 3, H, W, generator=g) * 1.4 - 0.2          # values outside [0, 1]: background is not clamped
    delta = torch.randn(KEYS * R, Cd, S, S, generator=g) * 0.1
    hm = torch.rand(F_ * S * S, generator=g)
    return imgs.cuda(), delta.cuda(), hm.cuda()


def _desc(imgs, out, pw, delta, hm, S, *, total_key, vm, att, clamp, variant):
    d = N.TailDesc()
    u8 = imgs.dtype == torch.uint8
    n, H, W = (imgs.shape[0], imgs.shape[1], imgs.shape[2]) if u8 else (imgs.shape[0], imgs.shape[2], imgs.shape[3])
    d.imgs, d.out, d.preds_w = N.ptr(imgs), N.ptr(out), N.ptr(pw)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), (N.ptr(hm) if att == "lowres" else None), C.cast(TAPS, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = n, H, W, S, S, delta.shape[1]
    d.step, d.video_mode, d.total_key = STEP, vm, total_key
    d.attenuate, d.clamp, d.antialias = int(att != "off"), int(clamp), 1
    d.scaling_i, d.scaling_w, d.io_u8, d.variant = 1.0, 0.9, int(u8), variant
    return d


def _plain_reference(L, imgs, delta, hm, S, R, labels, **kw):
    """R launches of vs_embed_tail, plane sets of label r as delta, composed by torch.where over imgs (preds_w over zeros)"""
    Cd = delta.shape[1]
    u8 = imgs.dtype == torch.uint8
    n, H, W = labels.shape
    sets = delta.view(KEYS, R, Cd, S, S)
    per_out, per_pw = [], []
    for r in range(R):
        out, pw = torch.full_like(imgs, OUT_FILL[imgs.dtype]), torch.full((n, Cd, H, W), -7.0, device="cuda")
        N.check(L.vs_embed_tail(C.byref(_desc(imgs, out, pw, sets[:, r].contiguous(), hm, S, total_key=KEYS, **kw)), N.stream()), "vs_embed_tail")
        per_out.append(out)
        per_pw.append(pw)
    return RG.compose(imgs, per_out, labels), RG.compose(per_pw[0], per_pw, labels, background=torch.zeros_like(per_pw[0]))


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_S%d" % s)
def test_regions_tail_is_the_plain_tail_of_each_pixels_label(shape, u8):
    """vs_embed_tail_regions against the composition of R vs_embed_tail launches, bit for bit: every video mode, Cd, attenuate form and variant
    with every R; the label patterns rotate through the combinations so that each meets each R and each attenuate form"""
    L = N.lib()
    H, W, S = shape
    seen = set()
    combos = list(itertools.product(MODES, (1, 3), ATTS, VARIANTS))
    for i, (vm, Cd, att, variant) in enumerate(combos):
        for j, R in enumerate(RS):
            pattern = PATTERNS[(i + 3 * j + i // len(PATTERNS)) % len(PATTERNS)]
            seen.add((pattern, R))
            seen.add((pattern, att))
            imgs, delta, hm = _tail_inputs(H, W, S, R, Cd, u8, 100 * i + R)
            labels = _labels(pattern, H, W, R, i).cuda()
            kw = dict(vm=vm, att=att, clamp=True if u8 else Cd == 3, variant=variant)
            if pattern == "zeros":                 # nothing of delta reaches the result: the frames are the input, bit for bit
                want_out, want_pw = imgs, torch.zeros(F_, Cd, H, W, device="cuda")
                delta = torch.full_like(delta, NAN)
            else:
                want_out, want_pw = _plain_reference(L, imgs, delta, hm, S, R, labels, **kw)
            ib, gi = _guarded(imgs, 0x33 if u8 else NAN)
            db, gd = _guarded(delta, NAN)
            lb, gl = _guarded(labels, 1)
            ob, out = _guarded(torch.full_like(imgs, OUT_FILL[imgs.dtype]), OUT_FILL[imgs.dtype])
            pb, pw = _guarded(torch.full((F_, Cd, H, W), -9.0, device="cuda"), -7.0)
            d = _desc(gi, out, pw, gd, hm, S, total_key=KEYS, **kw)
            N.check(L.vs_embed_tail_regions(C.byref(d), N.ptr(gl), R, N.stream()), "vs_embed_tail_regions")
            what = (shape, u8, vm, Cd, att, variant, R, pattern)
            assert torch.equal(out.view(torch.int32) if not u8 else out, want_out.view(torch.int32) if not u8 else want_out), what
            assert torch.equal(pw, want_pw), what
            assert _guards_intact(ob, OUT_FILL[imgs.dtype]) and _guards_intact(pb, -7.0), what
            if i % 9 == 0:                         # without preds_w: the same frames
                ob2, out2 = _guarded(torch.full_like(imgs, OUT_FILL[imgs.dtype]), OUT_FILL[imgs.dtype])
                N.check(L.vs_embed_tail_regions(C.byref(_desc(gi, out2, None, gd, hm, S, total_key=KEYS, **kw)), N.ptr(gl), R, N.stream()), "vs_embed_tail_regions")
                assert torch.equal(out2, out) and _guards_intact(ob2, OUT_FILL[imgs.dtype]), what
    assert seen >= set(itertools.product(PATTERNS, RS)) | set(itertools.product(PATTERNS, ATTS))


def test_background_keeps_nan_and_out_of_range_values_bit_for_bit():
    L = N.lib()
    H, W, S, R = 37, 300, 16, 3
    imgs, delta, hm = _tail_inputs(H, W, S, R, 3, False, 5)
    imgs[0, :, 3, 4], imgs[1, 0, 20, 296], imgs[2, 1, 36, 0] = NAN, -0.0, 7.5          # columns of label 0
    labels = _labels("vstripes", H, W, R, 0).cuda()
    out = torch.full_like(imgs, -7.0)
    d = _desc(imgs, out, None, delta, hm, S, total_key=KEYS, vm=0, att="full", clamp=True, variant=0)
    N.check(L.vs_embed_tail_regions(C.byref(d), N.ptr(labels), R, N.stream()), "vs_embed_tail_regions")
    bg = (labels == 0)[:, None].expand_as(imgs)
    assert bool(torch.isnan(imgs[bg]).any()) and bool((imgs[bg] > 1).any()) and bool((imgs[bg] < 0).any())
    assert torch.equal(out.view(torch.int32)[bg], imgs.view(torch.int32)[bg])
    fg = out[~bg]
    fg = fg[~torch.isnan(fg)]                                  # (the heat-map of the NaN pixel's neighbours is NaN, as in the plain tail)
    assert bool(((fg >= 0) & (fg <= 1)).all())


def test_regions_tail_refusals_launch_nothing():
    L = N.lib()
    H, W, S, R = 23, 29, 16, 2
    imgs, delta, hm = _tail_inputs(H, W, S, R, 1, False, 0)
    labels = _labels("checker", H, W, R, 0).cuda()
    ob, out = _guarded(torch.full_like(imgs, -7.0), -7.0)
    kw = dict(total_key=KEYS, vm=0, att="full", clamp=True, variant=0)

    def call(R_=R, lab=labels, **over):
        d = _desc(imgs, out, None, delta, hm, S, **{**kw, **{k: v for k, v in over.items() if k in kw}})
        for k, v in over.items():
            if k not in kw:
                setattr(d, k, v)
        return L.vs_embed_tail_regions(C.byref(d), N.ptr(lab), R_, N.stream())
    assert L.vs_embed_tail_regions(None, N.ptr(labels), R, N.stream()) == -1
    assert call(lab=None) == -1 and call(R_=0) == -1 and call(R_=-3) == -1 and call(R_=N.REGIONS_MAX + 1) == -1
    assert call(imgs=None) == -1 and call(out=None) == -1 and call(delta=None) == -1 and call(taps43=None) == -1
    assert call(F=0) == -1 and call(H=0) == -1 and call(W=-1) == -1 and call(S_h=0) == -1 and call(Cd=2) == -1
    assert call(step=0) == -1 and call(total_key=0) == -1 and call(video_mode=3) == -1
    assert call(variant=3) == N.ERR_UNSUPPORTED and call(attenuate=2) == N.ERR_UNSUPPORTED
    u8 = torch.zeros(F_, H, W, 3, dtype=torch.uint8, device="cuda")
    d = _desc(u8, torch.zeros_like(u8), None, delta, hm, S, total_key=KEYS, vm=0, att="off", clamp=False, variant=0)
    assert L.vs_embed_tail_regions(C.byref(d), N.ptr(labels), R, N.stream()) == -1          # uint8 frames need the clamp
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and _guards_intact(ob, -7.0)


# ---------------------------------------------------------------------------------------------------------------- vote
def _vote_regions(preds, labels, R, thr, fill=NAN):
    """one launch on guarded outputs and an exactly sized, poisoned workspace -> (votes, nsel, sums)"""
    L = N.lib()
    B, K, Sh, Sw = preds.shape
    bs = preds.stride(0) if B > 1 else K * Sh * Sw
    n = L.vs_pixel_vote_regions_partial_doubles(B, K, Sh * Sw, R)
    assert n > 0
    pb, part = scratch(n, torch.float64, fill)
    vb, votes = _guarded(torch.full((B, R, K), -5, dtype=torch.int32, device="cuda"), 0x5A)
    nb, nsel = _guarded(torch.full((B, R), -5, dtype=torch.int32, device="cuda"), 0x5A)
    sb, sums = _guarded(torch.full((B, R, K), -5.0, dtype=torch.float64, device="cuda"), -7.0)
    N.check(L.vs_pixel_vote_regions(N.ptr(preds), bs, N.ptr(labels), B, K, Sh, Sw, labels.shape[1], labels.shape[2], R, float(thr), N.ptr(votes),
                                    N.ptr(nsel), N.ptr(sums), N.ptr(part), N.stream()), "vs_pixel_vote_regions")
    torch.cuda.synchronize()
    assert _guards_intact(pb, scratch_sentinel(torch.float64)) and _guards_intact(vb, 0x5A) and _guards_intact(nb, 0x5A) and _guards_intact(sb, -7.0)
    return votes.clone(), nsel.clone(), sums.clone()


VOTE_MAPS = [((1, 1), None), ((7, 9), None), ((17, 241), None), ((16, 16), (37, 50))]       # HW = 1, 63, 64 * 64 + 1; labels at another size
VOTE_CASES = [(m, K) for m in VOTE_MAPS for K in (1, 5, 257)] + [(((3, 2731), None), 5)]       # HW = 8193: two chunks of partials, at one K


@pytest.mark.parametrize("maps,K", VOTE_CASES, ids=lambda v: str(v) if isinstance(v, int) else "%dx%d" % v[0] + ("_lab%dx%d" % v[1] if v[1] else ""))
def test_vote_regions_counts_are_pixel_vote_with_each_regions_mask(maps, K):
    (Sh, Sw), lab_size = maps
    B, R = 3, 3
    for thr in PR.VOTE_THRESHOLDS:
        x, _ = PR.vote_inputs(B, K + 1, Sh * Sw, thr)             # logits exactly at the threshold and one ulp either side on every other element
        full = _guarded(x.view(B, K + 1, Sh, Sw).cuda(), NAN)[1]
        preds = full[:, 1:]                                       # a strided channel slice, read in place
        g = torch.Generator().manual_seed(Sh * Sw + K)
        Hl, Wl = lab_size or (Sh, Sw)
        labels = torch.randint(0, R + 3, (B, Hl, Wl), generator=g, dtype=torch.uint8)          # R + 1, R + 2: background
        labels[B - 1][labels[B - 1] == 2] = 0                     # region 2 has no pixel in the last frame
        labels = _guarded(labels.cuda(), 1)[1]
        votes, nsel, sums = _vote_regions(preds, labels, R, thr)
        at_map = RG.labels_at_map(labels, Sh, Sw)
        for r in range(1, R + 1):
            v, n = pixel_vote(preds, (at_map == r)[:, None].float(), thr)
            assert torch.equal(votes[:, r - 1], v) and torch.equal(nsel[:, r - 1], n), (maps, K, thr, r)
        rv, rn, rs = RG.vote_regions(preds.cpu(), labels.cpu(), R, thr)
        assert torch.equal(votes.cpu().long(), rv) and torch.equal(nsel.cpu().long(), rn)
        assert int(nsel[B - 1, 1]) == 0 and bool((sums[B - 1, 1] == 0).all())
        again = _vote_regions(preds, labels, R, thr, fill=0.0)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((votes, nsel, sums), again))        # same bits, whatever the workspace held


@pytest.mark.parametrize("kind", ["mean30", "cancelling", "outlier"])
def test_vote_regions_sums_are_float64_sums(kind):
    """|sum - float64 sum of the same fp32 logits| <= n * 2^-53 * sum |terms| with n the pixels of the region: the error of n double additions
    in any order (every term is exact in float64), no measured constant"""
    B, K, R = 3, 5, 4
    for (Sh, Sw), lab_size in (((17, 241), None), ((16, 16), (37, 50)), ((3, 2731), None)):
        g = torch.Generator().manual_seed(Sh + len(kind))
        x = torch.randn(B, K, Sh, Sw, generator=g)
        if kind == "mean30":
            x = 30.0 + 0.5 * x
        elif kind == "cancelling":
            x = (1000.0 + x) * torch.where(torch.arange(Sh * Sw).view(Sh, Sw) % 2 == 0, 1.0, -1.0)
        else:
            x.view(B, K, -1)[:, :, (Sh * Sw) // 2] = 4e3
        Hl, Wl = lab_size or (Sh, Sw)
        labels = torch.randint(0, R + 1, (B, Hl, Wl), generator=g, dtype=torch.uint8)
        votes, nsel, sums = _vote_regions(x.cuda(), labels.cuda(), R, 0.0)
        rv, rn, rs = RG.vote_regions(x, labels, R, 0.0)
        lab = RG.labels_at_map(labels, Sh, Sw)
        for r in range(1, R + 1):
            mag = torch.where((lab == r)[:, None], x.double().abs(), torch.zeros((), dtype=torch.float64)).sum((-2, -1))
            bound = rn[:, r - 1, None].double() * 2.0 ** -53 * mag
            err = (sums[:, r - 1].cpu() - rs[:, r - 1]).abs()
            print(f"vote sums {kind} {Sh}x{Sw} r={r}: max err {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}")
            assert bool((err <= bound).all()), (kind, Sh, Sw, r, float(err.max()), float(bound.min()))
        assert torch.equal(votes.cpu().long(), rv) and torch.equal(nsel.cpu().long(), rn)


def test_vote_regions_refusals():
    L = N.lib()
    p = torch.zeros(1, 2, 4, 4, device="cuda")
    lab = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    v, n = torch.zeros(1, 2, 2, dtype=torch.int32, device="cuda"), torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    s, part = torch.zeros(1, 2, 2, dtype=torch.float64, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
    args = [N.ptr(p), 32, N.ptr(lab), 1, 2, 4, 4, 4, 4, 2, 0.0, N.ptr(v), N.ptr(n), N.ptr(s), N.ptr(part), N.stream()]
    assert L.vs_pixel_vote_regions(*args) == 0
    for i, bad in ((0, None), (2, None), (3, 0), (4, 0), (5, 0), (7, 0), (9, 0), (9, 9), (11, None), (12, None), (13, None), (14, None)):
        a = list(args)
        a[i] = bad
        assert L.vs_pixel_vote_regions(*a) == -1, i
    assert L.vs_pixel_vote_regions_partial_doubles(0, 1, 1, 1) == -1 and L.vs_pixel_vote_regions_partial_doubles(1, 1, 0, 1) == -1


# ---------------------------------------------------------------------------------------------------------------- boxes
def test_label_boxes_against_torch():
    L = N.lib()
    R = 4
    g = torch.Generator().manual_seed(11)
    cases = []
    lab = torch.zeros(3, 70, 300, dtype=torch.uint8)              # three row bands, more than one pass of 256 threads per row
    lab[0, 0, 0], lab[0, 69, 299], lab[0, 0, 299], lab[0, 69, 0] = 1, 2, 3, 4                       # one-pixel regions in the corners
    lab[1, :, :] = 1                                                                                # touches every border
    lab[1, 10:50, 17:230] = 3
    lab[2, 31:34, 255:258] = 2                                                                      # across a band edge and a 256-column edge
    lab[2, 5, 7] = 200                                                                              # above R: background
    cases.append(lab)
    cases.append(torch.zeros(2, 5, 3, dtype=torch.uint8))                                           # no label at all
    cases.append(torch.randint(0, R + 2, (4, 33, 65), generator=g, dtype=torch.uint8))
    sparse = torch.zeros(2, 64, 64, dtype=torch.uint8)
    sparse[0, 13, 40], sparse[1, 63, 63] = 4, 1
    cases.append(sparse)
    for lab in cases:
        lb, gl = _guarded(lab.cuda(), 1)
        bb, boxes = _guarded(torch.full((lab.shape[0], R, 4), -5, dtype=torch.int32, device="cuda"), 0x5A)
        N.check(L.vs_label_boxes(N.ptr(gl), lab.shape[0], lab.shape[1], lab.shape[2], R, N.ptr(boxes), N.stream()), "vs_label_boxes")
        assert torch.equal(boxes.cpu(), RG.label_boxes(lab, R)) and _guards_intact(bb, 0x5A), tuple(lab.shape)
    assert L.vs_label_boxes(None, 1, 1, 1, 1, N.ptr(boxes), N.stream()) == -1 and L.vs_label_boxes(N.ptr(gl), 1, 1, 1, 9, N.ptr(boxes), N.stream()) == -1


# ---------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def tiny():
    spec = tiny_spec()
    sd = make_state_dict(spec, seed=3)
    model = make_model(spec, sd)
    model.chunk_size, model.step_size = 2, 2
    return spec, sd, model


def _model_labels(n, H, W, R):
    lab = torch.zeros(n, H, W, dtype=torch.uint8)
    lab[:, : H // 2, : W // 2] = 1
    if R >= 2:
        lab[:, H // 3:, W // 2:] = 2
    if R >= 3:
        lab[:, H // 2:, 5: W // 2: 3] = 3                      # 1-pixel columns
    lab[:, 0, :] = R + 1                                       # above R: background
    return lab


@pytest.mark.parametrize("video_mode", ["repeat", "interpolate"])
def test_one_region_over_the_whole_frame_is_embed(tiny, video_mode):
    """R = 1 and an all-ones label map: the same U-Net batch and the same tail body as `embed`, so the same bits"""
    spec, sd, model = tiny
    model.video_mode = video_mode
    try:
        imgs = synthetic_frames(6, 96, 80, seed=42).cuda()
        msgs = synthetic_msgs(6, spec.nbits, seed=42)
        ones = torch.ones(6, 96, 80, dtype=torch.uint8, device="cuda")
        # video mode, fp32 and uint8
        want = model.embed(imgs, msgs[:1], is_video=True)
        got = model.embed_regions(imgs, ones, msgs[:1], is_video=True)
        assert torch.equal(got["imgs_w"], want["imgs_w"]) and "preds_w" not in got and tuple(got["msgs"].shape) == (6, 1, spec.nbits)
        clip = (imgs * 255).byte().permute(0, 2, 3, 1).contiguous()
        for lowres in (True, False):
            want8 = model.embed_u8(clip, msgs[:1], lowres_attenuation=lowres)
            got8 = model.embed_regions(clip, ones, msgs[:1], is_video=True, lowres_attenuation=lowres)
            assert got8["imgs_w"].dtype == torch.uint8 and torch.equal(got8["imgs_w"], want8["imgs_w"])
        # image mode: one message per frame, fp32 against embed and uint8 against embed_images
        want = model.embed(imgs, msgs, is_video=False)
        got = model.embed_regions(imgs, ones, msgs[:, None, :], is_video=False)
        assert torch.equal(got["imgs_w"], want["imgs_w"]) and torch.equal(got["preds_w"], want["preds_w"])
        want8 = model.embed_images(list(clip), msgs)
        got8 = model.embed_regions(clip, ones, msgs[:, None, :], is_video=False)
        assert torch.equal(got8["imgs_w"], torch.stack(want8["imgs_w"])) and torch.equal(got8["preds_w"], torch.stack(want8["preds_w"]))
    finally:
        model.video_mode = "repeat"


@pytest.mark.parametrize("is_video", [True, False], ids=["video", "image"])
def test_three_regions_against_the_oracle_composed_by_the_label_map(tiny, is_video):
    spec, sd, model = tiny
    n, H, W, R = 6, 96, 80, 3
    imgs = synthetic_frames(n, H, W, seed=42)
    msgs = synthetic_msgs(R, spec.nbits, seed=43)
    labels = _model_labels(n, H, W, R)
    if is_video:
        embed = lambda x, m: O.embed_video(sd, spec, x, m, chunk_size=2, step_size=2)["imgs_w"]        # noqa: E731
    else:
        embed = lambda x, m: O.embed_image(sd, spec, x, m.repeat(len(x), 1))["imgs_w"]                  # noqa: E731
    want = RG.embed_regions(embed, imgs, labels, msgs)
    got = model.embed_regions(imgs.cuda(), labels.cuda(), msgs, is_video=is_video)
    out = got["imgs_w"].cpu()
    err = float((out - want).abs().max())
    print(f"embed_regions R=3 {'video' if is_video else 'image'}: max |hip - oracle| = {err:.3e} (TOL_IMG {TOL_IMG})")
    assert err < TOL_IMG
    bg = (RG.clean_labels(labels, R) == 0)[:, None].expand_as(imgs)
    assert bg.any() and torch.equal(out[bg].view(torch.int32), imgs[bg].view(torch.int32))
    changed = [(out != imgs)[(labels == r)[:, None].expand_as(imgs)].float().mean() for r in (1, 2, 3)]
    assert all(c > 0.25 for c in changed), changed
    # frames (and labels) on the host: chunk by chunk to the device, the same result on the caller's device
    host = model.embed_regions(imgs, labels, msgs, is_video=is_video)
    assert not host["imgs_w"].is_cuda and torch.equal(host["imgs_w"], out)
    if not is_video:
        assert torch.equal(host["preds_w"], got["preds_w"].cpu()) and bool((got["preds_w"].cpu()[bg[:, :1].expand(-1, got["preds_w"].shape[1], -1, -1)] == 0).all())
    # regions differ: region 2 carries message 2, not message 1
    one = model.embed_regions(imgs.cuda(), labels.cuda(), msgs[:1].repeat(R, 1), is_video=is_video)["imgs_w"].cpu()
    s2 = (labels == 2)[:, None].expand_as(imgs)
    assert not torch.equal(one[s2], out[s2]) and torch.equal(one[(labels == 1)[:, None].expand_as(imgs)], out[(labels == 1)[:, None].expand_as(imgs)])


def test_embed_regions_graph_replay_matches_eager_and_the_key_carries_R(tiny):
    spec, sd, model = tiny
    n, H, W = 4, 96, 80
    n0 = len(model._graphs)
    outs = {}
    try:
        for use in (False, True):
            model.use_graphs = use
            res = []
            for R, seed in ((3, 1), (3, 2), (2, 3)):           # one chunk of 4 frames each: the second call replays, R = 2 is another graph
                imgs = synthetic_frames(n, H, W, seed=seed).cuda()
                msgs = synthetic_msgs(R, spec.nbits, seed=seed)
                res.append(model.embed_regions(imgs, _model_labels(n, H, W, R).cuda(), msgs, is_video=True)["imgs_w"])
            outs[use] = res
    finally:
        model.use_graphs = False
    assert len(model._graphs) == n0 + 2
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))


@pytest.fixture(scope="module")
def pw():
    spec = U.model_specs()["cnx"]
    sd = U.model_state_dict(spec, "cnx")
    cfg = dataclasses.replace(cfg_of(spec), head_stages=list(U.MODEL_STAGES["cnx"]), head_pixelwise=True)
    m = build_model(cfg)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    n, h, w, seed = U.MODEL_FRAMES
    return spec, m.eval().to("cuda"), synthetic_frames(n, h, w, seed=seed)


@pytest.mark.parametrize("method", ["hard", "semihard"])
def test_decode_regions_is_the_references_selection_on_the_same_maps(pw, method):
    """bit_accuracy_inference (evals/metrics.py:208-256) restated in torch on the maps `detect` returns: per region the mean over its pixels of
    `pred > threshold` (hard) or of the logit (semihard), in float64, then `> 0.5`"""
    spec, model, imgs = pw
    n, H, W = imgs.shape[0], imgs.shape[2], imgs.shape[3]
    R, thr = 3, 0.0
    labels = _model_labels(n, H, W, 2)                         # region 3 is empty
    preds = model.detect(imgs.cuda(), is_video=True)["preds"]
    got = model.decode_regions(imgs.cuda(), labels.cuda(), method=method, threshold=thr, R=R)
    assert tuple(got["msgs"].shape) == (n, R, spec.nbits) and got["msgs"].dtype == torch.bool and got["score"].dtype == torch.float64 and got["count"].dtype == torch.int32
    at_map = RG.labels_at_map(labels, preds.shape[-2], preds.shape[-1])
    p = preds[:, 1:].cpu()
    for f in range(n):
        for r in range(1, R + 1):
            mask = (at_map[f] == r)[None].expand_as(p[f])
            vals = ((p[f] > thr) if method == "hard" else p[f]).masked_select(mask).view(spec.nbits, -1)
            cnt = vals.shape[1]
            assert int(got["count"][f, r - 1]) == cnt
            if cnt == 0:
                assert r == 3 and bool(torch.isnan(got["score"][f, r - 1]).all()) and not bool(got["msgs"][f, r - 1].any())
                continue
            mean = vals.mean(dim=-1, dtype=float)
            score = got["score"][f, r - 1].cpu()
            if method == "hard":
                assert torch.equal(score, mean)                   # whole-number counts: the quotient is the same float64
            else:
                # both sides add cnt float64 terms in some order (2 x cnt * 2^-53 * sum |terms|) and round one division
                bound = 2 * cnt * 2.0 ** -53 * vals.double().abs().sum(-1) / cnt + 2.0 ** -52 * mean.abs()
                assert bool(((score - mean).abs() <= bound).all())
            sure = (mean - 0.5).abs() > 1e-9
            assert torch.equal(got["msgs"][f, r - 1].cpu()[sure], (mean > 0.5)[sure])
    auto = model.decode_regions(imgs.cuda(), RG.clean_labels(labels, 2).cuda(), method=method, threshold=thr)       # R from the label map's maximum: 2
    assert tuple(auto["msgs"].shape) == (n, 2, spec.nbits) and torch.equal(auto["msgs"], got["msgs"][:, :2])
    clip = model.decode_regions(imgs.cuda(), labels.cuda(), method=method, threshold=thr, per="clip", R=R)
    votes, nsel, sums = RG.vote_regions(p, labels, R, thr)
    want = RG.decide(votes, nsel, sums, method, "clip")
    assert tuple(clip["msgs"].shape) == (1, R, spec.nbits) and torch.equal(clip["count"].cpu(), want["count"])
    ok = ~torch.isnan(want["score"])
    assert torch.allclose(clip["score"].cpu()[ok], want["score"][ok], rtol=1e-12, atol=1e-12) and bool(torch.isnan(clip["score"].cpu()[~ok]).all())
    host = model.decode_regions(imgs, labels, method=method, threshold=thr, R=R)                # frames and labels on the host
    assert not host["msgs"].is_cuda and torch.equal(host["msgs"], got["msgs"].cpu()) and torch.equal(host["count"], got["count"].cpu())


def test_detect_regions_is_detect_images_on_the_boxes(tiny):
    spec, sd, model = tiny
    n, H, W, R = 4, 96, 80, 3
    imgs = synthetic_frames(n, H, W, seed=44).cuda()
    labels = torch.zeros(n, H, W, dtype=torch.uint8)
    labels[:, 10:50, 8:40] = 1
    labels[0, 60:90, 30:75] = 2
    labels[1, 0, 0] = 2
    labels[1, 95, 79] = 2                                      # two pixels in opposite corners: the box is the frame
    labels[3] = 0
    labels[3, 40:80, 20:60] = 3
    got = model.detect_regions(imgs, labels.cuda(), R)
    boxes = RG.label_boxes(labels, R)
    assert torch.equal(got["boxes"].cpu(), boxes) and tuple(got["preds"].shape) == (n, R, spec.nbits + 1)
    present = [(f, r) for f in range(n) for r in range(R) if boxes[f, r, 2] > boxes[f, r, 0]]
    crops = [imgs[f, :, boxes[f, r, 0]:boxes[f, r, 2], boxes[f, r, 1]:boxes[f, r, 3]] for f, r in present]
    want = model.detect_images(crops)["preds"]
    for i, (f, r) in enumerate(present):
        assert torch.equal(got["preds"][f, r], want[i]), (f, r)
    absent = [(f, r) for f in range(n) for r in range(R) if (f, r) not in present]
    assert absent and all(bool(torch.isnan(got["preds"][f, r]).all()) for f, r in absent)
    clip = (imgs * 255).byte().permute(0, 2, 3, 1).contiguous()
    got8 = model.detect_regions(clip, labels.cuda(), R)
    want8 = model.detect_images([clip[f, boxes[f, r, 0]:boxes[f, r, 2], boxes[f, r, 1]:boxes[f, r, 3]] for f, r in present])["preds"]
    assert all(torch.equal(got8["preds"][f, r], want8[i]) for i, (f, r) in enumerate(present))
