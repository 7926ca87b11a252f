"""Embedding to a target PSNR on the HIP path: vs_embed_tail_energy / vs_psnr_scale / vs_embed_tail_scaled at the operator level,
Videoseal.embed_psnr and vs_model_embed_psnr at the model level.

References: vs_embed_tail itself (the scaled tail at scale[f] = c is the fixed tail at scaling_w = c, bit for bit; the energy is the float64
sum of squares of the preds_w the fixed tail stores), the strength formula in float64 on the host, `embed` / `embed_u8` at
blender.scaling_w = scaling_w[f], and videoseal_amd.metrics.psnr in float64.
Frame shapes (S = 16): 16 x 16 no resize; 23 x 29 tile form, ragged tiles; 37 x 53 row-streaming form, two row bands = several partials per
frame; 40 x 150 a wide frame in one column tile; 34 x 260 two column tiles with a ragged second one (both forms)."""
import ctypes as C
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.inputs import synthetic_msgs  # noqa: E402
from oracle.weights import make_state_dict, spec_from_card, tiny_spec  # noqa: E402
from tests._cases import CARDS  # noqa: E402
from tests._guards import _guards_intact, scratch, scratch_sentinel  # noqa: E402
from tests._model import cfg_of, make_model  # noqa: E402

from videoseal_amd import native as N  # noqa: E402
from videoseal_amd.metrics import psnr  # noqa: E402

pytestmark = pytest.mark.gpu

S = 16
SHAPES = [(16, 16), (23, 29), (37, 53), (40, 150), (34, 260)]
CLIPS = [(5, 4), (2, 1)]                                     # (F, step): a ragged last key group; every frame a key frame
MODES = (0, 1, 2)                                            # repeat, alternate, interpolate
ATTS = ("off", "lowres", "full")
VARIANTS = (0, 1, 2, 4)                                      # default, 43-tap tiles, separable tiles (what the default resolves to off the
                                                             # row-streaming form), row-streaming
CS = (0.0, 0.37, 1.0, 2.5)
DISTINCT = (0.37, 1.0, 0.0, 2.5, 0.61)
TAPS = (C.c_float * 43)(*([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1]))
SENT = {torch.float32: (-7.0, -9.0), torch.uint8: (0x5A, 0xA5)}


def _inputs(H, W, F_, step, Cd, u8, seed):
    g = torch.Generator().manual_seed(seed)
    nk = (F_ + step - 1) // step
    imgs = torch.randint(0, 256, (F_, H, W, 3), generator=g, dtype=torch.uint8) if u8 else torch.rand(F_, 3, H, W, generator=g)
    delta = torch.randn(nk, Cd, S, S, generator=g) * 0.1
    hm = torch.rand(F_ * S * S, generator=g)
    return imgs.cuda(), delta.cuda(), hm.cuda()


def _desc(imgs, out, pw, delta, hm, *, step, vm, att, clamp, variant, sw=1.0):
    d = N.TailDesc()
    u8 = imgs.dtype == torch.uint8
    F_, H, W = (imgs.shape[0], imgs.shape[1], imgs.shape[2]) if u8 else (imgs.shape[0], imgs.shape[2], imgs.shape[3])
    d.imgs, d.out, d.preds_w = N.ptr(imgs), N.ptr(out), N.ptr(pw)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), (N.ptr(hm) if att == "lowres" else None), C.cast(TAPS, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, delta.shape[1]
    d.step, d.video_mode, d.total_key = step, vm, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = int(att != "off"), int(clamp), 1
    d.scaling_i, d.scaling_w, d.io_u8, d.variant = 1.0, sw, int(u8), variant
    return d


def _combos():
    return itertools.product(CLIPS, (1, 3), MODES, ATTS)


# ---------------------------------------------------------------------------------------------------- 1. scaled tail against fixed tail
@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_scaled_tail_is_the_fixed_tail_at_that_strength(shape, u8):
    L = N.lib()
    H, W = shape
    for seed, ((F_, step), Cd, vm, att) in enumerate(_combos()):
        imgs, delta, hm = _inputs(H, W, F_, step, Cd, u8, seed)
        clamp = True if u8 else Cd == 3                      # fp32: both settings over the combinations
        fa, fb = SENT[imgs.dtype]
        for variant in VARIANTS:
            kw = dict(step=step, vm=vm, att=att, clamp=clamp, variant=variant)
            fixed = {}
            for c in sorted(set(CS + DISTINCT)):
                out, pw = torch.full_like(imgs, fa), torch.full((F_, Cd, H, W), -7.0, device="cuda")
                N.check(L.vs_embed_tail(C.byref(_desc(imgs, out, pw, delta, hm, sw=c, **kw)), N.stream()), "vs_embed_tail")
                fixed[c] = (out, pw)
            for c in CS:
                out, pw = torch.full_like(imgs, fb), torch.full((F_, Cd, H, W), -9.0, device="cuda")
                sc = torch.full((F_,), c, device="cuda")
                # (scaling_w of the descriptor is not looked at)
                N.check(L.vs_embed_tail_scaled(C.byref(_desc(imgs, out, pw, delta, hm, sw=99.0, **kw)), N.ptr(sc), N.stream()), "vs_embed_tail_scaled")
                assert torch.equal(out, fixed[c][0]) and torch.equal(pw, fixed[c][1]), (shape, u8, F_, Cd, vm, att, variant, c)
            out, pw = torch.full_like(imgs, fb), torch.full((F_, Cd, H, W), -9.0, device="cuda")
            sc = torch.tensor(DISTINCT[:F_], device="cuda")
            N.check(L.vs_embed_tail_scaled(C.byref(_desc(imgs, out, pw, delta, hm, sw=99.0, **kw)), N.ptr(sc), N.stream()), "vs_embed_tail_scaled")
            for f in range(F_):
                ref = fixed[DISTINCT[f]]
                assert torch.equal(out[f], ref[0][f]) and torch.equal(pw[f], ref[1][f]), (shape, u8, F_, Cd, vm, att, variant, f)
            # without preds_w: the same frames
            out2 = torch.full_like(imgs, fb)
            N.check(L.vs_embed_tail_scaled(C.byref(_desc(imgs, out2, None, delta, hm, sw=99.0, **kw)), N.ptr(sc), N.stream()), "vs_embed_tail_scaled")
            assert torch.equal(out2, out)


def test_scaled_tail_and_energy_refuse_the_training_order_and_the_8_row_form():
    L = N.lib()
    imgs, delta, hm = _inputs(23, 29, 2, 1, 1, False, 0)
    out, sc = torch.empty_like(imgs), torch.ones(2, device="cuda")
    pb, part = scratch(L.vs_tail_energy_partial_doubles(2, 23, 29), torch.float64, float("nan"))
    eb, en = scratch(2, torch.float64, float("nan"))
    d = _desc(imgs, out, None, delta, hm, step=1, vm=0, att="full", clamp=True, variant=3)
    assert L.vs_embed_tail_scaled(C.byref(d), N.ptr(sc), N.stream()) == N.ERR_UNSUPPORTED
    assert L.vs_embed_tail_energy(C.byref(d), N.ptr(part), N.ptr(en), N.stream()) == N.ERR_UNSUPPORTED
    d = _desc(imgs, out, None, delta, hm, step=1, vm=0, att="full", clamp=True, variant=0)
    d.attenuate = 2
    assert L.vs_embed_tail_scaled(C.byref(d), N.ptr(sc), N.stream()) == N.ERR_UNSUPPORTED
    assert L.vs_embed_tail_energy(C.byref(d), N.ptr(part), N.ptr(en), N.stream()) == N.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(en).all())              # nothing was launched


@pytest.mark.parametrize("form", [1, 3], ids=["v1", "keep"])
def test_under_the_process_wide_form_switch_all_three_still_agree(form):
    """VIDEOSEAL_TAIL=v1|keep (development switch TAIL_FORM) with variant 0: the new modes follow v1 as vs_embed_tail does and answer keep
    with the 16-row tiles of the same separable stencils -- either way the scaled frames are the fixed tail's under that switch, bit for
    bit, and the energy is that of its preds_w"""
    L = N.lib()
    for (H, W), att in itertools.product([(23, 29), (37, 53)], ATTS):
        imgs, delta, hm = _inputs(H, W, 2, 1, 1, False, 3)
        kw = dict(step=1, vm=0, att=att, clamp=True, variant=0)
        out, pw = torch.full_like(imgs, -7.0), torch.full((2, 1, H, W), -7.0, device="cuda")
        out2, pw2 = torch.full_like(imgs, -9.0), torch.full((2, 1, H, W), -9.0, device="cuda")
        sc = torch.full((2,), 0.37, device="cuda")
        pb, part = scratch(L.vs_tail_energy_partial_doubles(2, H, W), torch.float64, float("nan"))
        eb, en = scratch(2, torch.float64, float("nan"))
        with N.debug("TAIL_FORM", form):
            N.check(L.vs_embed_tail(C.byref(_desc(imgs, out, pw, delta, hm, sw=0.37, **kw)), N.stream()), "vs_embed_tail")
            N.check(L.vs_embed_tail_scaled(C.byref(_desc(imgs, out2, pw2, delta, hm, sw=99.0, **kw)), N.ptr(sc), N.stream()), "vs_embed_tail_scaled")
            N.check(L.vs_embed_tail_energy(C.byref(_desc(imgs, None, None, delta, hm, **kw)), N.ptr(part), N.ptr(en), N.stream()), "vs_embed_tail_energy")
        assert torch.equal(out2, out) and torch.equal(pw2, pw), (form, H, W, att)
        ref = 3.0 * pw.double().square().sum(dim=(1, 2, 3))
        assert float(((en - ref).abs() / ref).max()) <= H * W * 2.0 ** -53, (form, H, W, att)
        assert _guards_intact(pb, scratch_sentinel(torch.float64)) and _guards_intact(eb, scratch_sentinel(torch.float64))


# ---------------------------------------------------------------------------------------------------- 2. + 4. energy, guards
@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_energy_is_the_float64_sum_of_squares_of_preds_w(shape, u8):
    """relative difference <= N 2^-53, N = Cd H W: the linear bound of a float64 sum of N non-negative exact terms in any order -- which also
    says that the energy pass computes the tail's d bit for bit (one differing d moves the sum by ~2^-24 of a term)"""
    L = N.lib()
    H, W = shape
    worst = 0.0
    for seed, ((F_, step), Cd, vm, att) in enumerate(_combos()):
        imgs, delta, hm = _inputs(H, W, F_, step, Cd, u8, 100 + seed)
        npart = L.vs_tail_energy_partial_doubles(F_, H, W)
        for variant in VARIANTS:
            kw = dict(step=step, vm=vm, att=att, clamp=True, variant=variant)
            out, pw = torch.empty_like(imgs), torch.full((F_, Cd, H, W), -7.0, device="cuda")
            N.check(L.vs_embed_tail(C.byref(_desc(imgs, out, pw, delta, hm, **kw)), N.stream()), "vs_embed_tail")
            ref = (3.0 / Cd) * pw.double().square().sum(dim=(1, 2, 3))
            runs = []
            for fill in (float("nan"), 0.0):                  # what the workspace held before does not matter
                pb, part = scratch(npart, torch.float64, fill)
                eb, en = scratch(F_, torch.float64, float("nan"))
                keep_out = torch.full_like(imgs, SENT[imgs.dtype][0])
                keep_pw = torch.full((F_, Cd, H, W), -7.0, device="cuda")
                # out, preds_w, scaling_w and clamp of the descriptor are ignored
                d = _desc(imgs, keep_out, keep_pw, delta, hm, sw=123.0, **dict(kw, clamp=False))
                N.check(L.vs_embed_tail_energy(C.byref(d), N.ptr(part), N.ptr(en), N.stream()), "vs_embed_tail_energy")
                assert _guards_intact(pb, scratch_sentinel(torch.float64)) and _guards_intact(eb, scratch_sentinel(torch.float64))
                assert bool((keep_out == SENT[imgs.dtype][0]).all()) and bool((keep_pw == -7.0).all()), "the energy pass stores no frame"
                runs.append(en.clone())
            assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64)), "two runs, two sets of bits"
            e, r = runs[0].cpu(), ref.cpu()
            for f in range(F_):
                if float(r[f]) == 0.0:
                    assert float(e[f]) == 0.0 and not math.copysign(1.0, float(e[f])) < 0
                    continue
                rel = abs(float(e[f]) - float(r[f])) / float(r[f])
                worst = max(worst, rel / (Cd * H * W * 2.0 ** -53))
                assert rel <= Cd * H * W * 2.0 ** -53, (shape, u8, F_, Cd, vm, att, variant, f, float(e[f]), float(r[f]))
    print(f"energy {shape} u8={u8}: worst relative difference = {worst:.3f} of the bound")


@pytest.mark.parametrize("vm", MODES)
def test_energy_of_a_frame_without_a_watermark_is_exactly_zero(vm):
    L = N.lib()
    for H, W in SHAPES:
        for att in ATTS:
            imgs, delta, hm = _inputs(H, W, 2, 1, 3, False, 7)
            delta[1] = 0.0
            pb, part = scratch(L.vs_tail_energy_partial_doubles(2, H, W), torch.float64, float("nan"))
            eb, en = scratch(2, torch.float64, float("nan"))
            d = _desc(imgs, None, None, delta, hm, step=1, vm=vm, att=att, clamp=True, variant=0)
            N.check(L.vs_embed_tail_energy(C.byref(d), N.ptr(part), N.ptr(en), N.stream()), "vs_embed_tail_energy")
            e = en.cpu()
            assert float(e[0]) > 0.0 and float(e[1]) == 0.0 and math.copysign(1.0, float(e[1])) > 0, (H, W, att, e)


# ---------------------------------------------------------------------------------------------------- 3. + 4. strengths, guards
def _scale_ref(E, n, T, cap):
    if E == 0.0:
        return np.float32(0.0)
    s = 10.0 ** (-T / 20.0) * math.sqrt(n / E)
    return np.float32(cap) if (cap > 0 and s > np.float64(np.float32(cap))) else np.float32(s)


@pytest.mark.parametrize("per_clip", [0, 1])
def test_strengths_follow_the_formula(per_clip):
    L = N.lib()
    g = torch.Generator().manual_seed(5)
    for (H, W), F_, T in itertools.product([(16, 16), (37, 53), (768, 768)], (1, 5, 300), (36.0, 42.0, 48.5)):
        E = (torch.rand(F_, generator=g, dtype=torch.float64) * 10.0) ** 3 * 1e-3 * H * W
        if F_ > 1:
            E[1] = 0.0
        n = 3.0 * H * W
        free = [float(_scale_ref(float(sum(E.tolist())) if per_clip else float(e), n * F_ if per_clip else n, T, 0.0)) for e in E.tolist()]
        med = sorted(free)[len(free) // 2]
        for cap in (0.0, -1.0, med if med > 0 else 1.0):      # none, none, one that binds for about half of the frames
            sb, sc = scratch(F_, torch.float32, float("nan"))
            Ed = E.cuda()
            N.check(L.vs_psnr_scale(N.ptr(Ed), F_, H, W, per_clip, T, cap, N.ptr(sc), N.stream()), "vs_psnr_scale")
            assert _guards_intact(sb, scratch_sentinel(torch.float32))
            got = sc.cpu().numpy()
            tot = 0.0
            for e in E.tolist():                             # the clip's energy: the frames added in order
                tot += e
            for f, e in enumerate(E.tolist()):
                ref = _scale_ref(tot if per_clip else e, n * F_ if per_clip else n, T, cap)
                if (tot if per_clip else e) == 0.0:
                    assert got[f] == 0.0
                elif cap > 0 and ref == np.float32(cap):
                    assert got[f] == np.float32(cap), (H, W, F_, T, cap, f)      # the ceiling, exactly
                else:
                    assert abs(float(got[f]) - float(ref)) <= float(np.spacing(ref)), (H, W, F_, T, cap, f, got[f], ref)
            if per_clip:
                assert (got == got[0]).all()
    # a clip without any watermark
    sb, sc = scratch(3, torch.float32, float("nan"))
    Ed = torch.zeros(3, dtype=torch.float64, device="cuda")
    N.check(L.vs_psnr_scale(N.ptr(Ed), 3, 16, 16, per_clip, 42.0, 0.0, N.ptr(sc), N.stream()), "vs_psnr_scale")
    assert bool((sc == 0.0).all()) and _guards_intact(sb, scratch_sentinel(torch.float32))


# ---------------------------------------------------------------------------------------------------- model level
def psnr_bound(T):
    """dB: one fp32 rounding of s and of the blend (2^-23 relative to a pixel <= 1) against a perturbation of rms 10^(-T / 20)"""
    return 20.0 * math.log10(1.0 + 2.0 ** -23 / 10.0 ** (-T / 20.0)) + 1e-5


def _frames(F_, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.05 + 0.9 * torch.rand(F_, 3, H, W, generator=g)).cuda()


def _to_u8(x):
    return (x * 255.0).round().byte().permute(0, 2, 3, 1).contiguous()


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


@pytest.fixture(scope="module")
def vs10():
    s = spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml"))
    sd = make_state_dict(s, seed=0)
    return s, sd, make_model(s, sd)


def _check_bits(model, x, msgs, span, T, *, is_video, lowres):
    """imgs_w[f] of embed_psnr is `embed` of frame f's chunk at blender.scaling_w = scaling_w[f], bit for bit"""
    u8 = x.dtype == torch.uint8
    sw0 = model.blender.scaling_w

    def fixed(chunk, m):
        if u8:
            return model.embed_u8(chunk, m, lowres_attenuation=lowres)["imgs_w"]
        return model.embed(chunk, m, is_video=is_video, lowres_attenuation=lowres)["imgs_w"]

    fixed(x[:span], msgs if is_video else msgs[:span])           # (tile choices of a first call are made before anything is compared)
    r = model.embed_psnr(x, T, msgs, is_video=is_video, lowres_attenuation=lowres)
    assert model.blender.scaling_w == sw0
    out, s, e = r["imgs_w"], r["scaling_w"], r["energy"]
    assert out.dtype == x.dtype and out.shape == x.shape and out.device == x.device
    assert s.dtype == torch.float32 and s.shape == (x.shape[0],) and e.dtype == torch.float64 and e.shape == (x.shape[0],)
    assert bool((s > 0).all()) and bool((e > 0).all())
    try:
        for f in range(x.shape[0]):
            a = f // span * span
            model.blender.scaling_w = float(s[f])
            ref = fixed(x[a:a + span], msgs if is_video else msgs[a:a + span])
            assert torch.equal(out[f], ref[f - a]), (f, float(s[f]))
    finally:
        model.blender.scaling_w = sw0
    return r


@pytest.mark.parametrize("lowres", [False, True], ids=["full", "lowres"])
@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_tiny_embed_psnr_gives_the_bits_of_embed_at_that_strength(tiny, u8, lowres):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=21)
    x = _frames(5, 134, 202, 31)                                # two chunks of four frames, the last one ragged; row-streaming tail
    with _Settings(model, chunk_size=2, step_size=2, video_mode="interpolate"):
        r = _check_bits(model, _to_u8(x) if u8 else x, msgs, 4, 42.0, is_video=True, lowres=lowres)
        assert len(set(r["scaling_w"].tolist())) > 1             # the content decides
    if not u8:                                                  # image mode: a message per frame, tile form
        x = _frames(3, 72, 88, 32)
        with _Settings(model, chunk_size=2):
            _check_bits(model, x, synthetic_msgs(3, spec.nbits, seed=22), 2, 38.0, is_video=False, lowres=lowres)


def test_vs10_embed_psnr_gives_the_bits_of_embed_at_that_strength(vs10):
    spec, sd, model = vs10
    msgs = synthetic_msgs(1, spec.nbits, seed=23)
    x = _frames(2, 72, 88, 33)
    with _Settings(model):
        _check_bits(model, x, msgs, 2, 42.0, is_video=True, lowres=False)
        _check_bits(model, _to_u8(x), msgs, 2, 42.0, is_video=True, lowres=True)
        # the quality statement on the released card: unclamped, the frame sits at the target
    with _Settings(model, clamp=False):
        for T in (36.0, 42.0, 48.0):
            out = model.embed_psnr(x, T, msgs)["imgs_w"]
            p = psnr(out.double(), x.double())
            assert float((p - T).abs().max()) <= psnr_bound(T), (T, p.tolist(), psnr_bound(T))
            # per clip: the clip as one signal sits at the target, one strength for all frames
            r = model.embed_psnr(x, T, msgs, per="clip")
            pc = float(psnr(r["imgs_w"].double(), x.double(), is_video=True))
            assert abs(pc - T) <= psnr_bound(T), (T, pc)
            s = r["scaling_w"]
            assert bool((s == s[0]).all()) and float(s[0]) > 0
    with _Settings(model, clamp=True):
        for T in (36.0, 42.0, 48.0):
            p = psnr(model.embed_psnr(x, T, msgs)["imgs_w"].double(), x.double())
            assert float(p.min()) >= T - psnr_bound(T), (T, p.tolist())
            r = model.embed_psnr(x, T, msgs, per="clip")
            assert float(psnr(r["imgs_w"].double(), x.double(), is_video=True)) >= T - psnr_bound(T)
            assert bool((r["scaling_w"] == r["scaling_w"][0]).all())


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_vs10_model_level_c_api_psnr(u8, monkeypatch):
    """the released card (Cd = 1, a Y-channel embedder) through vs_model_embed_psnr: the bytes and the strengths of embed_psnr.  Both hosts
    take their K-slice and tile decisions from the library's plan with the tuner off (test_gpu_e2e.py: the condition under which the two
    hosts are torch.equal on this card), on a model of its own built under these switches"""
    from videoseal_amd.capi import CModel
    monkeypatch.setenv("VIDEOSEAL_AUTOTUNE", "0")
    monkeypatch.setenv("VIDEOSEAL_PLANES_SPLITK", "0")
    spec = spec_from_card(os.path.join(CARDS, "videoseal_1.0.yaml"))
    sd = make_state_dict(spec, seed=0)
    model, cm = make_model(spec, sd), CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=27)
    x = _frames(2, 72, 88, 37)
    x = _to_u8(x) if u8 else x
    step = int(model.step_size)
    for lowres, per in ((True, "frame"), (False, "frame"), (False, "clip")):
        py = model.embed_psnr(x, 42.0, msgs, per=per, lowres_attenuation=lowres)
        out, sc = cm.embed_psnr(x, msgs, 42.0, per_clip=(per == "clip"), step=step, video_mode=N.VIDEO_MODES[model.video_mode],
                                lowres_attenuation=lowres)
        assert torch.equal(sc, py["scaling_w"]) and torch.equal(out, py["imgs_w"]), (u8, lowres, per, sc.tolist(), py["scaling_w"].tolist())


def test_strided_and_permuted_clips_are_packed_first(tiny):
    """a uint8 clip as `(x * 255).byte().permute(0, 2, 3, 1)` leaves it (a view with permuted strides), every second frame of a longer clip,
    and fp32 frames held channels-last: the frames and strengths of the packed clip, in a packed result"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=28)
    x = _frames(5, 72, 88, 38)
    planar = (x * 255.0).round().byte()                       # [F, 3, H, W]
    view = planar.permute(0, 2, 3, 1)
    twice = torch.stack([view.contiguous(), torch.zeros_like(view)], dim=1).flatten(0, 1)      # frames interleaved with black ones
    xl = x.to(memory_format=torch.channels_last)
    assert not view.is_contiguous() and not twice[::2].is_contiguous() and not xl.is_contiguous()
    with _Settings(model, chunk_size=2, step_size=2):
        for per in ("frame", "clip"):
            want = model.embed_psnr(view.contiguous(), 40.0, msgs, per=per)
            for clip in (view, twice[::2]):
                got = model.embed_psnr(clip, 40.0, msgs, per=per)
                assert got["imgs_w"].is_contiguous() and got["imgs_w"].shape == view.shape
                assert torch.equal(got["imgs_w"], want["imgs_w"]) and torch.equal(got["scaling_w"], want["scaling_w"]), per
            assert not torch.equal(want["imgs_w"], view)
            wf = model.embed_psnr(x, 40.0, msgs, per=per)
            gf = model.embed_psnr(xl, 40.0, msgs, per=per)
            assert torch.equal(gf["imgs_w"], wf["imgs_w"]) and torch.equal(gf["scaling_w"], wf["scaling_w"]), per


@pytest.mark.parametrize("lowres", [False, True], ids=["full", "lowres"])
def test_tiny_psnr_meets_the_target(tiny, lowres):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=24)
    x = _frames(5, 134, 202, 34)
    for vm in ("repeat", "interpolate"):
        with _Settings(model, chunk_size=2, step_size=2, video_mode=vm, clamp=False):
            for T in (36.0, 42.0, 48.0):
                r = model.embed_psnr(x, T, msgs, lowres_attenuation=lowres)
                p = psnr(r["imgs_w"].double(), x.double())
                print(f"tiny {vm} lowres={lowres} T={T}: psnr - T = {[float(v) - T for v in p]} bound {psnr_bound(T):.3g}")
                assert float((p - T).abs().max()) <= psnr_bound(T), (vm, T, p.tolist(), psnr_bound(T))
                # per clip: the clip as one signal sits at the target, one strength for all frames
                r = model.embed_psnr(x, T, msgs, per="clip", lowres_attenuation=lowres)
                pc = float(psnr(r["imgs_w"].double(), x.double(), is_video=True))
                assert abs(pc - T) <= psnr_bound(T), (vm, T, pc)
                s = r["scaling_w"]
                assert bool((s == s[0]).all()) and float(s[0]) > 0
        with _Settings(model, chunk_size=2, step_size=2, video_mode=vm, clamp=True):
            for T in (36.0, 42.0, 48.0):
                p = psnr(model.embed_psnr(x, T, msgs, lowres_attenuation=lowres)["imgs_w"].double(), x.double())
                assert float(p.min()) >= T - psnr_bound(T), (vm, T, p.tolist())


def test_ceiling_host_frames_and_refusals(tiny):
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=25)
    x = _frames(5, 72, 88, 35)
    with _Settings(model, chunk_size=2, step_size=2):
        free = model.embed_psnr(x, 30.0, msgs)
        cap = float(free["scaling_w"].median())
        r = model.embed_psnr(x, 30.0, msgs, max_scaling_w=cap)
        want = torch.minimum(free["scaling_w"], torch.tensor(cap, device="cuda"))
        assert torch.equal(r["scaling_w"], want) and torch.equal(r["energy"], free["energy"])
        # host-resident frames move one chunk at a time: the same values, back on the caller's device
        h = model.embed_psnr(x.cpu(), 30.0, msgs)
        assert h["imgs_w"].device.type == "cpu" and h["scaling_w"].device.type == "cpu" and h["energy"].dtype == torch.float64
        assert torch.equal(h["imgs_w"], free["imgs_w"].cpu()) and torch.equal(h["scaling_w"], free["scaling_w"].cpu())
        with pytest.raises(ValueError, match="resident"):
            model.embed_psnr(x.cpu(), 30.0, msgs, per="clip")
        # an empty clip
        e = model.embed_psnr(x[:0], 30.0, msgs)
        assert e["imgs_w"].shape == x[:0].shape and e["scaling_w"].shape == (0,) and e["energy"].dtype == torch.float64


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_model_level_c_api_psnr(tiny, u8):
    """vs_model_embed_psnr returns the bytes and the strengths of embed_psnr on one chunk"""
    from videoseal_amd.capi import CModel
    spec, sd, model = tiny
    cm = CModel(cfg_of(spec), sd)
    msgs = synthetic_msgs(1, spec.nbits, seed=26)
    x = _frames(4, 134, 202, 36)
    x = _to_u8(x) if u8 else x
    for vm, lowres, per in (("repeat", True, "frame"), ("interpolate", False, "frame"), ("alternate", True, "clip")):
        with _Settings(model, chunk_size=2, step_size=2, video_mode=vm):
            py = model.embed_psnr(x, 40.0, msgs, per=per, max_scaling_w=50.0, lowres_attenuation=lowres)
        out, sc = cm.embed_psnr(x, msgs, 40.0, per_clip=(per == "clip"), max_scaling_w=50.0, step=2, video_mode=N.VIDEO_MODES[vm],
                                lowres_attenuation=lowres)
        assert torch.equal(out, py["imgs_w"]) and torch.equal(sc, py["scaling_w"]), (u8, vm, lowres, per)
    L = N.lib()
    # the workspace function covers a run: exactly `need` bytes between guard bands, with and without the low-resolution heat-map
    need = L.vs_model_embed_psnr_workspace_bytes(cm._h, 4, 134, 202, 2)
    assert need > 0
    mi = msgs.to(device="cuda", dtype=torch.int32)
    for lowres in (1, 0):
        with _Settings(model, chunk_size=2, step_size=2):
            py = model.embed_psnr(x, 40.0, msgs, lowres_attenuation=bool(lowres))
        wb, ws = scratch(need, torch.uint8, 0xFF)
        assert ws.data_ptr() % 256 == 0
        o, s4 = torch.empty_like(x), torch.empty(4, device="cuda")
        N.check(L.vs_model_embed_psnr(cm._h, N.ptr(x), N.ptr(mi), 1, 4, 134, 202, 2, 0, lowres, 1, int(u8), 40.0, 0, 0.0, N.ptr(o), None,
                                      N.ptr(s4), N.ptr(ws), need, N.stream()), "vs_model_embed_psnr")
        assert torch.equal(o, py["imgs_w"]) and torch.equal(s4, py["scaling_w"]), (u8, lowres)
        assert _guards_intact(wb, scratch_sentinel(torch.uint8))
    args = (N.ptr(x), N.ptr(mi), 1, 4, 134, 202, 2, 0, 1, 1)
    assert L.vs_model_embed_psnr(cm._h, *args, 2, 40.0, 0, 0.0, N.ptr(o), None, N.ptr(s4), N.ptr(ws), need, None) == N.ERR_UNSUPPORTED
    assert L.vs_model_embed_psnr(cm._h, *args, int(u8), float("nan"), 0, 0.0, N.ptr(o), None, N.ptr(s4), N.ptr(ws), need, None) == -1
    assert L.vs_model_embed_psnr(cm._h, *args, int(u8), 40.0, 0, 0.0, N.ptr(o), None, None, N.ptr(ws), need, None) == -1
    assert L.vs_model_embed_psnr(cm._h, *args, int(u8), 40.0, 0, 0.0, N.ptr(o), None, N.ptr(s4), N.ptr(ws), 256, None) == -1      # workspace too small
