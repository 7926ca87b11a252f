"""Target PSNR for lists on the HIP path: vs_embed_tail_images_scaled / _energy, vs_embed_tail_clips_scaled / _energy and vs_psnr_scale_items
at the operator level (processing size S = 16), Videoseal.embed_images_psnr / embed_clips_psnr at the model level (the tiny model at its own
processing size).

References are the project's own fixed-strength entry points and float64 on the host: the scaled list tail at scale[i] = c is the fixed list
tail (images) or the scaled clip tail (slots) at that strength, bit for bit; the energy is the float64 sum of squares of the preds_w the fixed
list tail stores; the strengths follow the formula in float64; the model calls are `embed_images` / `embed_clips` at
blender.scaling_w = scaling_w[i], and videoseal_amd.metrics.psnr in float64 says whether the target is met.
Image shapes: 16 x 16 one tile; 23 x 29 and 17 x 19 two tile rows, ragged; 37 x 53 three tile rows; 40 x 150 a wide image in one column tile;
34 x 260 two column tiles with a ragged second one (workgroups whose columns lie outside the image take part in the energy reduction).  33
images need two launch groups."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from oracle.inputs import synthetic_msgs
from oracle.weights import make_state_dict, tiny_spec
from tests._guards import _guards_intact, scratch, scratch_sentinel
from tests._model import make_model
from videoseal_amd import native as N
from videoseal_amd.metrics import psnr

pytestmark = pytest.mark.gpu

S = 16
IMAGES5 = [(16, 16), (23, 29), (37, 53), (40, 150), (34, 260)]
IMAGES33 = [[(16, 16), (17, 19), (23, 29)][i % 3] for i in range(33)]
LISTS = {"5": IMAGES5, "33": IMAGES33}
CLIP_SIZES = [(5, 23, 29), (2, 37, 53), (1, 34, 260)]              # (F, H, W) of the slots
N_FRAMES = 11                                                      # frames of the processing-size tensors: three more than the slots cover
ATTS = ("off", "lowres", "full")
DISTINCT = (0.37, 1.0, 0.0, 2.5, 0.61)
TAPS = (C.c_float * 43)(*([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1]))
FILL = {torch.float32: -9.0, torch.uint8: 0xA5}                    # what an output holds before a call (the bands around it: scratch_sentinel)


def _out_like(t):
    """(buffer, view): an output of t's shape and dtype between two guard bands, pre-filled"""
    buf, v = scratch(t.numel(), t.dtype, FILL[t.dtype])
    return buf, v.view(t.shape)


def _pw_for(shape):
    buf, v = scratch(int(np.prod(shape)), torch.float32, -9.0)
    return buf, v.view(shape)


def _bands_ok(bufs):
    return all(_guards_intact(b, scratch_sentinel(b.dtype)) for b in bufs)


# ---------------------------------------------------------------------------------------------------- images
def _image_inputs(sizes, Cd, u8, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = [(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8) if u8 else torch.rand(3, H, W, generator=g)).cuda() for H, W in sizes]
    delta = (torch.randn(len(sizes), Cd, S, S, generator=g) * 0.1).cuda()
    hm = torch.rand(len(sizes) * S * S, generator=g).cuda()
    return imgs, delta, hm


def _images_desc(imgs, outs, pws, delta, hm, *, att, clamp, sw=1.0):
    """-> (descriptor, the HOST array it points into)"""
    arr = N.image_descs(imgs, outs, pws)
    d = N.TailImagesDesc()
    d.images, d.n = arr, len(imgs)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), (N.ptr(hm) if att == "lowres" else None), C.cast(TAPS, C.c_void_p)
    d.S_h, d.S_w, d.Cd = S, S, delta.shape[1]
    d.attenuate, d.clamp, d.antialias, d.io_u8 = int(att != "off"), int(clamp), 1, int(imgs[0].dtype == torch.uint8)
    d.scaling_i, d.scaling_w = 1.0, sw
    return d, arr


def _pw_shapes(imgs, Cd):
    return [(Cd,) + (tuple(t.shape[:2]) if t.dtype == torch.uint8 else tuple(t.shape[1:])) for t in imgs]


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("which", list(LISTS))
def test_scaled_image_list_is_the_fixed_tail_of_every_image_at_its_strength(which, u8):
    L = N.lib()
    sizes = LISTS[which]
    n = len(sizes)
    for seed, (Cd, att) in enumerate(itertools.product((1, 3), ATTS)):
        imgs, delta, hm = _image_inputs(sizes, Cd, u8, seed)
        clamp = True if u8 else Cd == 3                          # fp32: both settings over the combinations
        sc = torch.tensor([DISTINCT[i % 5] for i in range(n)], device="cuda")
        ob, outs = zip(*[_out_like(t) for t in imgs])
        pb, pws = zip(*[_pw_for(s) for s in _pw_shapes(imgs, Cd)])
        # (scaling_w of the descriptor is not looked at)
        d, keep = _images_desc(imgs, outs, pws, delta, hm, att=att, clamp=clamp, sw=99.0)
        N.check(L.vs_embed_tail_images_scaled(C.byref(d), N.ptr(sc), N.stream()), "vs_embed_tail_images_scaled")
        assert _bands_ok(ob) and _bands_ok(pb), (which, u8, Cd, att)
        for i in range(n):                                       # the one-image list [image i] at scaling_w = scale[i], frame i of delta / hmap_lowres
            ro, rp = torch.full_like(imgs[i], FILL[imgs[i].dtype]), torch.full_like(pws[i], -7.0)
            d1, keep1 = _images_desc([imgs[i]], [ro], [rp], delta[i:i + 1], hm[i * S * S:], att=att, clamp=clamp, sw=DISTINCT[i % 5])
            N.check(L.vs_embed_tail_images(C.byref(d1), N.stream()), "vs_embed_tail_images")
            assert torch.equal(outs[i], ro) and torch.equal(pws[i], rp), (which, u8, Cd, att, i)
        # without preds_w: the same images
        ob2, outs2 = zip(*[_out_like(t) for t in imgs])
        d, keep = _images_desc(imgs, outs2, None, delta, hm, att=att, clamp=clamp, sw=99.0)
        N.check(L.vs_embed_tail_images_scaled(C.byref(d), N.ptr(sc), N.stream()), "vs_embed_tail_images_scaled")
        assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and _bands_ok(ob2)


def _check_energy(e, r, elems, what):
    """relative difference <= N 2^-53, N = Cd H W: the linear bound of a float64 sum of N non-negative exact terms in any order (the product of
    two fp32 values is exact in float64) -- which also says that the energy pass computes the tail's d bit for bit"""
    worst = 0.0
    for i, (ei, ri, ni) in enumerate(zip(e.tolist(), r.tolist(), elems)):
        if ri == 0.0:
            assert ei == 0.0 and math.copysign(1.0, ei) > 0, (what, i, ei)
            continue
        rel = abs(ei - ri) / ri
        worst = max(worst, rel / (ni * 2.0 ** -53))
        assert rel <= ni * 2.0 ** -53, (what, i, ei, ri)
    return worst


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("which", list(LISTS))
def test_energy_of_an_image_list_is_the_float64_sum_of_squares_of_preds_w(which, u8):
    L = N.lib()
    sizes = LISTS[which]
    n = len(sizes)
    worst = 0.0
    for seed, (Cd, att) in enumerate(itertools.product((1, 3), ATTS)):
        imgs, delta, hm = _image_inputs(sizes, Cd, u8, 100 + seed)
        delta[2] = 0.0                                           # an image without a watermark
        outs = [torch.empty_like(t) for t in imgs]
        pws = [torch.full(s, -7.0, device="cuda") for s in _pw_shapes(imgs, Cd)]
        d, keep = _images_desc(imgs, outs, pws, delta, hm, att=att, clamp=True)
        N.check(L.vs_embed_tail_images(C.byref(d), N.stream()), "vs_embed_tail_images")
        ref = torch.stack([(3.0 / Cd) * p.double().square().sum() for p in pws]).cpu()
        npart = L.vs_tail_images_energy_partial_doubles(keep, n, int(u8), S, S, 1)
        assert npart == sum(((W + 255) // 256) * ((H + 15) // 16) for H, W in sizes)
        runs = []
        for fill in (float("nan"), 0.0):                         # what the workspace held before does not matter
            qb, part = scratch(npart, torch.float64, fill)
            eb, en = scratch(n, torch.float64, float("nan"))
            ob, keep_out = zip(*[_out_like(t) for t in imgs])
            pb, keep_pw = zip(*[_pw_for(s) for s in _pw_shapes(imgs, Cd)])
            # out, preds_w, scaling_w and clamp of the descriptor are ignored
            d, keep2 = _images_desc(imgs, keep_out, keep_pw, delta, hm, att=att, clamp=False, sw=123.0)
            N.check(L.vs_embed_tail_images_energy(C.byref(d), N.ptr(part), N.ptr(en), N.stream()), "vs_embed_tail_images_energy")
            assert _bands_ok([qb, eb]) and _bands_ok(ob) and _bands_ok(pb)
            assert all(bool((o == FILL[o.dtype]).all()) for o in keep_out) and all(bool((p == -9.0).all()) for p in keep_pw), "no image is stored"
            assert not bool(torch.isnan(part).any()), "every slot of the sized workspace belongs to a workgroup"
            runs.append(en.clone())
        assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64)), "two runs, two sets of bits"
        # images[i].out may be NULL
        eb, en = scratch(n, torch.float64, float("nan"))
        d, keep2 = _images_desc(imgs, None, None, delta, hm, att=att, clamp=True)
        N.check(L.vs_embed_tail_images_energy(C.byref(d), N.ptr(part), N.ptr(en), N.stream()), "vs_embed_tail_images_energy")
        assert torch.equal(en.view(torch.int64), runs[0].view(torch.int64))
        e = runs[0].cpu()
        assert float(ref[2]) == 0.0 and float(e[0]) > 0.0
        worst = max(worst, _check_energy(e, ref, [Cd * H * W for H, W in sizes], (which, u8, Cd, att)))
    print(f"image-list energy {which} u8={u8}: worst relative difference = {worst:.3f} of the bound")


# ---------------------------------------------------------------------------------------------------- clips
def _slots(step):
    """[(F, H, W, first_frame, first_key)]: at step 4 the key frames are packed (0, 2, 3), at step 1 every frame is a key frame"""
    if step == 4:
        return [(5, 23, 29, 0, 0), (2, 37, 53, 5, 2), (1, 34, 260, 7, 3)]
    return [(5, 23, 29, 0, 0), (2, 37, 53, 5, 5), (1, 34, 260, 7, 7)]


def _clip_inputs(step, Cd, u8, seed):
    g = torch.Generator().manual_seed(seed)
    slots = _slots(step)
    frames = [(torch.randint(0, 256, (F_, H, W, 3), generator=g, dtype=torch.uint8) if u8 else torch.rand(F_, 3, H, W, generator=g)).cuda()
              for F_, H, W, _, _ in slots]
    nk = max(fk + (F_ + step - 1) // step for F_, _, _, _, fk in slots)
    delta = (torch.randn(nk, Cd, S, S, generator=g) * 0.1).cuda()
    hm = torch.rand(N_FRAMES * S * S, generator=g).cuda()
    return slots, frames, delta, hm


def _clips_desc(slots, frames, outs, pws, delta, hm, *, step, vm, att, clamp, sw=1.0):
    arr = N.clip_descs([(fr, ff, fk) for fr, (_, _, _, ff, fk) in zip(frames, slots)], outs, pws)
    d = N.TailClipsDesc()
    d.clips, d.n = arr, len(slots)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), (N.ptr(hm) if att == "lowres" else None), C.cast(TAPS, C.c_void_p)
    d.S_h, d.S_w, d.Cd = S, S, delta.shape[1]
    d.attenuate, d.clamp, d.antialias, d.io_u8 = int(att != "off"), int(clamp), 1, int(frames[0].dtype == torch.uint8)
    d.scaling_i, d.scaling_w, d.step, d.video_mode = 1.0, sw, step, vm
    return d, arr


def _slot_desc(fr, out, pw, delta, hm, *, step, vm, att, clamp):
    """vs_tail_desc_t of one slot as a clip of its own (delta and hm already moved to the slot)"""
    d = N.TailDesc()
    u8 = fr.dtype == torch.uint8
    F_, H, W = (fr.shape[0], fr.shape[1], fr.shape[2]) if u8 else (fr.shape[0], fr.shape[2], fr.shape[3])
    d.imgs, d.out, d.preds_w = N.ptr(fr), N.ptr(out), N.ptr(pw)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), (N.ptr(hm) if att == "lowres" else None), C.cast(TAPS, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, delta.shape[1]
    d.step, d.video_mode, d.total_key = step, vm, (F_ + step - 1) // step
    d.attenuate, d.clamp, d.antialias = int(att != "off"), int(clamp), 1
    d.scaling_i, d.scaling_w, d.io_u8, d.variant = 1.0, 99.0, int(u8), 2       # the 16-row tiles, as the list kernels
    return d


def _clip_pw_shapes(slots, Cd):
    return [(F_, Cd, H, W) for F_, H, W, _, _ in slots]


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("step", [4, 1])
def test_scaled_clip_list_is_the_scaled_clip_tail_of_every_slot(step, u8):
    L = N.lib()
    for seed, (vm, Cd, att) in enumerate(itertools.product((0, 1, 2), (1, 3), ATTS)):
        slots, frames, delta, hm = _clip_inputs(step, Cd, u8, seed)
        clamp = True if u8 else Cd == 3
        sc = torch.tensor([DISTINCT[(2 * i + 1) % 5] for i in range(N_FRAMES)], device="cuda")
        ob, outs = zip(*[_out_like(t) for t in frames])
        pb, pws = zip(*[_pw_for(s) for s in _clip_pw_shapes(slots, Cd)])
        kw = dict(step=step, vm=vm, att=att, clamp=clamp)
        d, keep = _clips_desc(slots, frames, outs, pws, delta, hm, sw=99.0, **kw)
        N.check(L.vs_embed_tail_clips_scaled(C.byref(d), N.ptr(sc), N_FRAMES, N.stream()), "vs_embed_tail_clips_scaled")
        assert _bands_ok(ob) and _bands_ok(pb), (step, u8, vm, Cd, att)
        for s, (fr, (F_, H, W, ff, fk)) in enumerate(zip(frames, slots)):
            ro, rp = torch.full_like(fr, FILL[fr.dtype]), torch.full_like(pws[s], -7.0)
            d1 = _slot_desc(fr, ro, rp, delta[fk:], hm[ff * S * S:], **kw)
            N.check(L.vs_embed_tail_scaled(C.byref(d1), N.ptr(sc[ff:]), N.stream()), "vs_embed_tail_scaled")
            assert torch.equal(outs[s], ro) and torch.equal(pws[s], rp), (step, u8, vm, Cd, att, s)


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("step", [4, 1])
def test_energy_of_a_clip_list_is_the_float64_sum_of_squares_of_preds_w(step, u8):
    L = N.lib()
    worst = 0.0
    for seed, (vm, Cd, att) in enumerate(itertools.product((0, 1, 2), (1, 3), ATTS)):
        slots, frames, delta, hm = _clip_inputs(step, Cd, u8, 200 + seed)
        if step == 1:
            delta[6] = 0.0                                       # frame 1 of the second slot carries no watermark
        kw = dict(step=step, vm=vm, att=att)
        outs = [torch.empty_like(t) for t in frames]
        pws = [torch.full(s, -7.0, device="cuda") for s in _clip_pw_shapes(slots, Cd)]
        d, keep = _clips_desc(slots, frames, outs, pws, delta, hm, clamp=True, **kw)
        N.check(L.vs_embed_tail_clips(C.byref(d), N.stream()), "vs_embed_tail_clips")
        ref = torch.cat([(3.0 / Cd) * p.double().square().sum(dim=(1, 2, 3)) for p in pws]).cpu()
        npart = L.vs_tail_clips_energy_partial_doubles(keep, len(slots), int(u8), S, S, 1)
        assert npart == sum(F_ * ((W + 255) // 256) * ((H + 15) // 16) for F_, H, W, _, _ in slots)
        runs = []
        for fill in (float("nan"), 0.0):
            qb, part = scratch(npart, torch.float64, fill)
            eb, en = scratch(N_FRAMES, torch.float64, -5.0)
            ob, keep_out = zip(*[_out_like(t) for t in frames])
            pb, keep_pw = zip(*[_pw_for(s) for s in _clip_pw_shapes(slots, Cd)])
            d, keep2 = _clips_desc(slots, frames, keep_out, keep_pw, delta, hm, clamp=False, sw=123.0, **kw)
            N.check(L.vs_embed_tail_clips_energy(C.byref(d), N.ptr(part), N.ptr(en), N_FRAMES, N.stream()), "vs_embed_tail_clips_energy")
            assert _bands_ok([qb, eb]) and _bands_ok(ob) and _bands_ok(pb)
            assert all(bool((o == FILL[o.dtype]).all()) for o in keep_out) and all(bool((p == -9.0).all()) for p in keep_pw), "no frame is stored"
            assert not bool(torch.isnan(part).any())
            assert bool((en[8:] == -5.0).all()), "entries that no slot covers are left untouched"
            runs.append(en.clone())
        assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64)), "two runs, two sets of bits"
        e = runs[0][:8].cpu()
        if step == 1:
            assert float(ref[6]) == 0.0
        worst = max(worst, _check_energy(e, ref, [Cd * H * W for F_, H, W, _, _ in slots for _ in range(F_)], (step, u8, vm, Cd, att)))
    print(f"clip-list energy step={step} u8={u8}: worst relative difference = {worst:.3f} of the bound")


# ---------------------------------------------------------------------------------------------------- strengths
def _scale_ref(E, n, T, cap):
    if E == 0.0:
        return np.float32(0.0)
    s = 10.0 ** (-T / 20.0) * math.sqrt(n / E)
    return np.float32(cap) if (cap > 0 and s > np.float64(np.float32(cap))) else np.float32(s)


@pytest.mark.parametrize("grouped", [False, True], ids=["items", "groups"])
def test_item_strengths_follow_the_formula(grouped):
    L = N.lib()
    g = torch.Generator().manual_seed(5)
    n = 8
    prefix = [0, 3, 3, 8] if grouped else list(range(n + 1))       # an empty group in the middle
    for T in (36.0, 42.0, 48.5):
        E = (torch.rand(n, generator=g, dtype=torch.float64) * 10.0) ** 3 * 1e-3 * 256
        E[1] = 0.0
        elems = torch.tensor([3.0 * (16 + 7 * i) * (16 + 13 * i) for i in range(n)], dtype=torch.float64)
        sums = []
        for a, b in zip(prefix[:-1], prefix[1:]):                 # the group's sums: the items added in index order
            te, tn = 0.0, 0.0
            for i in range(a, b):
                te += float(E[i])
                tn += float(elems[i])
            sums.append((te, tn))
        group_of = [k for k, (a, b) in enumerate(zip(prefix[:-1], prefix[1:])) for _ in range(a, b)]
        free = sorted(float(_scale_ref(*sums[group_of[i]], T, 0.0)) for i in range(n))
        # no ceiling; one that binds for about half of the items (two groups: the geometric mean of their strengths binds for one of them)
        binding = float(np.float32(math.sqrt(free[0] * free[-1]))) if grouped else free[n // 2]
        for cap in (0.0, binding):
            sb, sc = scratch(n, torch.float32, float("nan"))
            Ed, nd = E.cuda(), elems.cuda()
            fi = torch.tensor(prefix, dtype=torch.int32, device="cuda") if grouped else None
            N.check(L.vs_psnr_scale_items(N.ptr(Ed), N.ptr(nd), N.ptr(fi), n, len(prefix) - 1 if grouped else 0, T, cap, N.ptr(sc), N.stream()),
                    "vs_psnr_scale_items")
            assert _guards_intact(sb, scratch_sentinel(torch.float32))
            got = sc.cpu().numpy()
            bound = 0
            for i in range(n):
                te, tn = sums[group_of[i]]
                ref = _scale_ref(te, tn, T, cap)
                if te == 0.0:
                    assert got[i] == 0.0 and not grouped
                elif cap > 0 and ref == np.float32(cap):
                    assert got[i] == np.float32(cap), (T, cap, i)          # the ceiling, exactly
                    bound += 1
                else:
                    assert abs(float(got[i]) - float(ref)) <= float(np.spacing(ref)), (T, cap, i, got[i], ref)
            if cap > 0:
                assert 0 < bound < n
            if grouped:
                assert (got[0:3] == got[0]).all() and (got[3:8] == got[3]).all()
    # a group without any watermark, and items no group covers
    sb, sc = scratch(6, torch.float32, float("nan"))
    Ed, nd = torch.zeros(6, dtype=torch.float64, device="cuda"), torch.full((6,), 768.0, dtype=torch.float64, device="cuda")
    fi = torch.tensor([1, 4], dtype=torch.int32, device="cuda") if grouped else None
    N.check(L.vs_psnr_scale_items(N.ptr(Ed), N.ptr(nd), N.ptr(fi), 6, 1 if grouped else 0, 42.0, 0.0, N.ptr(sc), N.stream()), "vs_psnr_scale_items")
    got = sc.cpu()
    if grouped:
        assert bool((got[1:4] == 0.0).all()) and bool(torch.isnan(got[0])) and bool(torch.isnan(got[4:]).all())
    else:
        assert bool((got == 0.0).all())
    assert _guards_intact(sb, scratch_sentinel(torch.float32))


# ---------------------------------------------------------------------------------------------------- model level
def psnr_bound(T):
    """dB: one fp32 rounding of s and of the blend (2^-23 relative to a pixel <= 1) against a perturbation of rms 10^(-T / 20)"""
    return 20.0 * math.log10(1.0 + 2.0 ** -23 / 10.0 ** (-T / 20.0)) + 1e-5


class _Settings:
    def __init__(self, model, **kw):
        self.model, self.kw = model, kw

    def __enter__(self):
        self.old = {k: getattr(self.model, k) for k in self.kw}
        self.sw = self.model.blender.scaling_w
        for k, v in self.kw.items():
            setattr(self.model, k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            setattr(self.model, k, v)
        self.model.blender.scaling_w = self.sw


@pytest.fixture(scope="module")
def tiny():
    s = tiny_spec()
    sd = make_state_dict(s, seed=3)
    return s, sd, make_model(s, sd)


def _images(sizes, seed, u8=False):
    g = torch.Generator().manual_seed(seed)
    xs = [(0.05 + 0.9 * torch.rand(3, H, W, generator=g)).cuda() for H, W in sizes]
    return [(x * 255.0).round().byte().permute(1, 2, 0).contiguous() for x in xs] if u8 else xs


def _clips(seed, u8=False, empty=False):
    g = torch.Generator().manual_seed(seed)
    xs = [(0.05 + 0.9 * torch.rand(F_, 3, H, W, generator=g)).cuda() for F_, H, W in CLIP_SIZES]
    if empty:
        xs.insert(1, torch.zeros(0, 3, 20, 24, device="cuda"))
    return [(x * 255.0).round().byte().permute(0, 2, 3, 1).contiguous() for x in xs] if u8 else xs


@pytest.mark.parametrize("lowres", [False, True], ids=["full", "lowres"])
@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_embed_images_psnr_gives_the_bits_of_embed_images_at_each_strength(tiny, u8, lowres):
    spec, sd, model = tiny
    imgs = _images(IMAGES5, 41, u8)
    msgs = synthetic_msgs(5, spec.nbits, seed=41)
    sw0 = model.blender.scaling_w
    with _Settings(model):
        model.embed_images(imgs, msgs, lowres_attenuation=lowres)       # (tile choices of a first call are made before anything is compared)
        r = model.embed_images_psnr(imgs, 42.0, msgs, lowres_attenuation=lowres)
        assert model.blender.scaling_w == sw0
        s, e = r["scaling_w"], r["energy"]
        assert s.dtype == torch.float32 and s.shape == (5,) and e.dtype == torch.float64 and e.shape == (5,) and s.is_cuda and e.is_cuda
        assert bool((s > 0).all()) and len(set(s.tolist())) > 1          # the content decides
        for i in range(5):
            model.blender.scaling_w = float(s[i])
            ref = model.embed_images(imgs, msgs, lowres_attenuation=lowres)
            assert r["imgs_w"][i].dtype == imgs[i].dtype and r["imgs_w"][i].shape == imgs[i].shape
            assert torch.equal(r["imgs_w"][i], ref["imgs_w"][i]) and torch.equal(r["preds_w"][i], ref["preds_w"][i]), (i, float(s[i]))
        cd = spec.out_ch
        want = torch.stack([(3.0 / cd) * p.double().square().sum() for p in r["preds_w"]]).cpu()
        _check_energy(e.cpu(), want, [cd * H * W for H, W in IMAGES5], "model images")


@pytest.mark.parametrize("per", ["frame", "clip"])
@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_embed_clips_psnr_gives_the_bits_of_embed_clips_at_each_strength(tiny, u8, per):
    spec, sd, model = tiny
    clips = _clips(43, u8, empty=(per == "clip" and not u8))
    n = len(clips)
    msgs = synthetic_msgs(n, spec.nbits, seed=43)
    lowres = per == "clip"
    # chunk_size 2 x step_size 2: the 5-frame clip is cut into a slot of four frames and a slot of one
    with _Settings(model, chunk_size=2, step_size=2, video_mode="interpolate"):
        model.embed_clips(clips, msgs, lowres_attenuation=lowres)
        r = model.embed_clips_psnr(clips, 40.0, msgs, per=per, lowres_attenuation=lowres)
        assert len(r["imgs_w"]) == len(r["scaling_w"]) == len(r["energy"]) == n
        for c, s, e, o in zip(clips, r["scaling_w"], r["energy"], r["imgs_w"]):
            assert s.dtype == torch.float32 and s.shape == (c.shape[0],) and e.dtype == torch.float64 and e.shape == (c.shape[0],)
            assert o.dtype == c.dtype and o.shape == c.shape and bool((s > 0).all()) and bool((e > 0).all())
            if per == "clip":
                assert bool((s == s[:1]).all())                  # one strength from all its slots
        allw = torch.cat(r["scaling_w"]).tolist()
        distinct = sorted(set(allw))
        assert len(distinct) == (3 if per == "clip" else 8)
        for w in distinct:
            model.blender.scaling_w = w
            ref = model.embed_clips(clips, msgs, lowres_attenuation=lowres)["imgs_w"]
            for c in range(n):
                for f in range(clips[c].shape[0]):
                    if float(r["scaling_w"][c][f]) == w:
                        assert torch.equal(r["imgs_w"][c][f], ref[c][f]), (per, c, f, w)


@pytest.mark.parametrize("T", [36.0, 42.0])
def test_the_target_is_met(tiny, T):
    spec, sd, model = tiny
    imgs, clips = _images(IMAGES5, 45), _clips(46)
    mi, mc = synthetic_msgs(5, spec.nbits, seed=45), synthetic_msgs(3, spec.nbits, seed=46)
    b = psnr_bound(T)
    with _Settings(model, chunk_size=2, step_size=2, clamp=False):
        for lowres in (False, True):
            r = model.embed_images_psnr(imgs, T, mi, lowres_attenuation=lowres)
            p = [float(psnr(o.double()[None], x.double()[None])) for o, x in zip(r["imgs_w"], imgs)]
            print(f"images T={T} lowres={lowres}: psnr - T = {[v - T for v in p]} bound {b:.3g}")
            assert max(abs(v - T) for v in p) <= b, (T, p, b)
            r = model.embed_clips_psnr(clips, T, mc, per="frame", lowres_attenuation=lowres)
            p = torch.cat([psnr(o.double(), x.double()) for o, x in zip(r["imgs_w"], clips)]).tolist()
            print(f"clips per frame T={T} lowres={lowres}: psnr - T = {[v - T for v in p]} bound {b:.3g}")
            assert max(abs(v - T) for v in p) <= b, (T, p, b)
            r = model.embed_clips_psnr(clips, T, mc, per="clip", lowres_attenuation=lowres)
            p = [float(psnr(o.double(), x.double(), is_video=True)) for o, x in zip(r["imgs_w"], clips)]
            print(f"clips per clip T={T} lowres={lowres}: psnr - T = {[v - T for v in p]} bound {b:.3g}")
            assert max(abs(v - T) for v in p) <= b, (T, p, b)
    with _Settings(model, chunk_size=2, step_size=2, clamp=True):
        r = model.embed_images_psnr(imgs, T, mi)
        assert min(float(psnr(o.double()[None], x.double()[None])) for o, x in zip(r["imgs_w"], imgs)) >= T - b
        r = model.embed_clips_psnr(clips, T, mc, per="clip")
        assert min(float(psnr(o.double(), x.double(), is_video=True)) for o, x in zip(r["imgs_w"], clips)) >= T - b
        r = model.embed_clips_psnr(clips, T, mc, per="frame")
        assert float(torch.cat([psnr(o.double(), x.double()) for o, x in zip(r["imgs_w"], clips)]).min()) >= T - b


def test_ceiling_host_lists_empty_lists_and_refusals(tiny):
    spec, sd, model = tiny
    imgs, clips = _images(IMAGES5, 47), _clips(48)
    mi, mc = synthetic_msgs(5, spec.nbits, seed=47), synthetic_msgs(3, spec.nbits, seed=48)
    with _Settings(model, chunk_size=2, step_size=2):
        free = model.embed_images_psnr(imgs, 30.0, mi)
        cap = float(free["scaling_w"].median())
        r = model.embed_images_psnr(imgs, 30.0, mi, max_scaling_w=cap)
        want = torch.minimum(free["scaling_w"], torch.tensor(cap, device="cuda"))
        assert torch.equal(r["scaling_w"], want) and torch.equal(r["energy"], free["energy"]) and int((want == cap).sum()) >= 2
        # host-resident images move one chunk at a time (chunk_size 2: three chunks): the same values, back on the caller's device
        h = model.embed_images_psnr([t.cpu() for t in imgs], 30.0, mi)
        assert h["scaling_w"].device.type == "cpu" and h["energy"].dtype == torch.float64 and h["imgs_w"][0].device.type == "cpu"
        assert torch.equal(h["scaling_w"], free["scaling_w"].cpu())
        assert all(torch.equal(a, b.cpu()) for a, b in zip(h["imgs_w"], free["imgs_w"]))
        # clips: the ceiling, per clip and per frame
        for per in ("frame", "clip"):
            fc = model.embed_clips_psnr(clips, 30.0, mc, per=per)
            capc = float(torch.cat(fc["scaling_w"]).median())
            rc = model.embed_clips_psnr(clips, 30.0, mc, per=per, max_scaling_w=capc)
            for a, b in zip(rc["scaling_w"], fc["scaling_w"]):
                assert torch.equal(a, torch.minimum(b, torch.tensor(capc, device="cuda")))
        hc = model.embed_clips_psnr([t.cpu() for t in clips], 30.0, mc, per="frame")
        fc = model.embed_clips_psnr(clips, 30.0, mc, per="frame")
        assert all(torch.equal(a, b.cpu()) for a, b in zip(hc["imgs_w"], fc["imgs_w"])) and hc["scaling_w"][0].device.type == "cpu"
        assert all(torch.equal(a, b.cpu()) for a, b in zip(hc["scaling_w"], fc["scaling_w"]))
        with pytest.raises(ValueError, match="resident"):
            model.embed_clips_psnr([t.cpu() for t in clips], 30.0, mc, per="clip")
        # empty lists, and a list of clips without frames
        e = model.embed_images_psnr([], 30.0)
        assert e["imgs_w"] == [] and e["scaling_w"].shape == (0,) and e["energy"].dtype == torch.float64
        e = model.embed_clips_psnr([], 30.0)
        assert e["imgs_w"] == [] and e["scaling_w"] == [] and e["energy"] == []
        e = model.embed_clips_psnr([clips[0][:0]], 30.0, per="clip")
        assert e["imgs_w"][0].shape == clips[0][:0].shape and e["scaling_w"][0].shape == (0,) and e["energy"][0].dtype == torch.float64
