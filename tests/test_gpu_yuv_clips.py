"""Lists of YUV clips on the HIP path: vs_resize_pre_yuv_clips / vs_embed_tail_yuv_clips against the per-slot calls vs_resize_pre_yuv /
vs_embed_tail_yuv (variant = 1), bit for bit, for the ten formats; Videoseal.embed_clips_yuv / detect_clips_yuv against the composition of
the engine pieces on the same passes (byte for byte), a one-span list against embed_yuv / detect_yuv (byte for byte), every clip against the
torch definition (the bound of tests/test_gpu_yuv.py), extract_messages_yuv against extract_message, host-resident lists.

Tiny cards, processing size 64, chunk_size 2, step_size 2.  Slot shapes (tests/_yuv_clips_util.py), each where the format allows it:
  D 18 x 34: a chroma row shorter than one 16-byte piece, a frame smaller than a tile      B 72 x 88: watermark up-resize below 2 x
  A 134 x 202: odd 4:2:2 chroma width        C 134 x 522: three 256-column tiles, a ragged last one, 8 : 1 resize
  E 67 x 202: odd H (4:2:2, 4:4:4)           G 131 x 259: odd H and W, row-streaming resize without antialias (4:4:4)
with 1, 3, 5 and 9 frames (nine: more than two spans).  Every plane is a strided view of its own poisoned buffer between GUARD bands, pitches
differ per plane (odd where the dtype allows), frames have spare rows."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.inputs import synthetic_frames, synthetic_msgs  # noqa: E402
from oracle.weights import make_state_dict, tiny_spec  # noqa: E402
from tests import _yuv_clips_util as U  # noqa: E402
from tests import _yuv_ref as R  # noqa: E402
from tests._model import TOL_IMG, TOL_LOGIT, make_model  # noqa: E402
from tests._util import DECISION_MARGIN, assert_decisions  # noqa: E402

from videoseal_amd import clips as CL  # noqa: E402
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import yuv  # noqa: E402
from videoseal_amd.engine import Act  # noqa: E402
from videoseal_amd.model import aggregate_bits  # noqa: E402

pytestmark = pytest.mark.gpu

S, PER, STEP, CK = U.S, U.PER, 2, 2
NAN = float("nan")
PRESET = R.PRESETS[4]
NA = {"mode": "bilinear", "align_corners": False, "antialias": False}


@pytest.fixture(scope="module")
def tiny():
    s = tiny_spec()
    sd = make_state_dict(s, seed=3)
    return s, sd, make_model(s, sd)


@pytest.fixture(scope="module")
def tinyc():
    s = tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16)
    sd = make_state_dict(s, seed=4)
    return s, sd, make_model(s, sd)


def _set(model, mode="repeat"):
    model.chunk_size, model.step_size, model.video_mode = CK, STEP, mode


def slots_of(fmt):
    """[(shape name, frames)]: the shapes the format allows, lengths 1, 3, 5, 9 in turn"""
    return [(n, U.LENGTHS[i % 4]) for i, n in enumerate(U.sizes_of(fmt))]


@functools.lru_cache(maxsize=None)
def clip_np(fmt, name, F_, kind, preset=PRESET):
    """the planes of one source clip (numpy, computed once and shared; never written)"""
    H, W = U.SIZES[name][:2]
    if kind == "random":
        return U.random_clip(F_, H, W, fmt, seed=F_ + H)
    return R.encode(synthetic_frames(F_, H, W, seed=F_ + W, kind=kind).numpy(), fmt, *preset)


def pitched(fmt, name, F_, kind="smooth", **kw):
    return U.Pitched(U.to_t(clip_np(fmt, name, F_, kind)), U.SIZES[name][2], U.SIZES[name][3], **kw)


def empty_like(fmt, name, F_, poison=0x5A):
    return U.Pitched(U.to_t(clip_np(fmt, name, F_, "smooth")), U.SIZES[name][2], U.SIZES[name][3], poison=poison, extra=4, fill=False)


def layout(slots, step):
    """first_frame / first_key of every slot: the list sits in the processing-size tensors in REVERSE order with a row nobody owns in front
    of every slot -> (first frames, first keys, rows of dst_rgb, rows of dst_key)"""
    ff, fk, at_f, at_k = {}, {}, 1, 2
    for i in reversed(range(len(slots))):
        ff[i], fk[i] = at_f, at_k
        at_f += slots[i][1] + 1
        at_k += U.cdiv(slots[i][1], step) + 1
    return ff, fk, at_f, at_k


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def run_resize(fmt, slots, srcs, aa, key_step, want_rgb=True, want_key=True):
    """the list call and the per-slot calls -> nothing; asserts the equalities of test 1"""
    lib = N.lib()
    dec = U.aff(PRESET, U.depth_of(fmt))[0]
    ymat = (C.c_float * 3)(*U.YMAT)
    ff, fk, nf, nk = layout(slots, key_step)
    rgb = torch.full((nf, S, S, 4), NAN, device="cuda")
    key = torch.full((nk, S, S, 4), NAN, device="cuda")
    descs = U.slot_descs(fmt, [(src, None, F_, *U.SIZES[n][:2], ff[i], fk[i]) for i, ((n, F_), src) in enumerate(zip(slots, srcs))])
    N.check(lib.vs_resize_pre_yuv_clips(descs, len(slots), dec, S, S, int(aa), N.ptr(rgb) if want_rgb else None, 2.0, -1.0,
                                        N.ptr(key) if want_key else None, key_step, ymat, None), "vs_resize_pre_yuv_clips")
    torch.cuda.synchronize()
    own_f, own_k = torch.zeros(nf, dtype=torch.bool), torch.zeros(nk, dtype=torch.bool)
    for i, ((n, F_), src) in enumerate(zip(slots, srcs)):
        H, W = U.SIZES[n][:2]
        keys = U.cdiv(F_, key_step)
        r1 = torch.full((F_, S, S, 4), NAN, device="cuda")
        k1 = torch.full((keys, S, S, 4), NAN, device="cuda")
        surf = src.surface(fmt)
        N.check(lib.vs_resize_pre_yuv(C.byref(surf), F_, H, W, dec, S, S, int(aa), N.ptr(r1) if want_rgb else None, 2.0, -1.0,
                                      N.ptr(k1) if want_key else None, key_step, ymat, None), "vs_resize_pre_yuv")
        torch.cuda.synchronize()
        if want_rgb:
            assert not bool(torch.isnan(r1).any()) and torch.equal(rgb[ff[i]:ff[i] + F_], r1), (fmt, n, F_, aa, key_step, "dst_rgb")
        if want_key:
            assert not bool(torch.isnan(k1).any()) and torch.equal(key[fk[i]:fk[i] + keys], k1), (fmt, n, F_, aa, key_step, "dst_key")
        assert not own_f[ff[i]:ff[i] + F_].any() and not own_k[fk[i]:fk[i] + keys].any()
        own_f[ff[i]:ff[i] + F_] = True
        own_k[fk[i]:fk[i] + keys] = True
    # rows no slot owns (and a destination that was not asked for) keep their fill
    assert bool(torch.isnan(rgb[~own_f.cuda()] if want_rgb else rgb).all()) and bool(torch.isnan(key[~own_k.cuda()] if want_key else key).all())


# ---------------------------------------------------------------------------------------------------- 1. resize, bit for bit
@pytest.mark.parametrize("fmt", U.FORMATS)
def test_resize_list_equals_the_per_slot_call(fmt):
    """vs_resize_pre_yuv_clips on the list == vs_resize_pre_yuv per slot (torch.equal on the slot's rows of dst_rgb and dst_key): antialias on
    and off, key_step 1 and 2, smooth and uniformly random words; rows of the destinations that no slot owns keep their NaN fill; the
    sources are unchanged.  The list holds slots of all three resize forms (the 8 : 1 shape takes the tile kernel, the small ones 128
    columns, the 3 x ones 64), so one call is three launch groups."""
    slots = slots_of(fmt)
    for kind in ("smooth", "random"):
        srcs = [pitched(fmt, n, F_, kind) for n, F_ in slots]
        keep = [[b.clone() for b in s.bufs] for s in srcs]
        for aa, key_step in itertools.product((True, False), (1, 2)):
            run_resize(fmt, slots, srcs, aa, key_step)
        run_resize(fmt, slots, srcs, True, 2, want_rgb=False)
        run_resize(fmt, slots, srcs, False, 1, want_key=False)
        assert all(torch.equal(a, b) for s, k in zip(srcs, keep) for a, b in zip(s.bufs, k))
    forms = {U.form_of(N.IMAGES_RESIZE, fmt, *U.SIZES[n][:2], S, S, True) for n, _ in slots}
    assert len(forms) == 3, forms


def run_tail(fmt, slots, srcs, eng, *, mode, Cd, full_jnd, seed):
    """the list call and the per-slot calls (variant = 1) -> nothing; asserts the equalities of test 2"""
    lib = N.lib()
    ff, fk, nf, nk = layout(slots, STEP)
    g = torch.Generator().manual_seed(seed)
    delta = torch.tanh(torch.randn(nk, Cd, S, S, generator=g)).cuda()
    hm = None if full_jnd else torch.rand(nf * S * S, generator=g).cuda()
    dsts = [empty_like(fmt, n, F_) for n, F_ in slots]
    descs = U.slot_descs(fmt, [(src, dst, F_, *U.SIZES[n][:2], ff[i], fk[i]) for i, ((n, F_), src, dst) in enumerate(zip(slots, srcs, dsts))])
    d = U.tail_clips_desc(descs, len(slots), fmt, PRESET, eng.taps43, delta, hm, step=STEP, video_mode=mode, Cd=Cd)
    N.check(lib.vs_embed_tail_yuv_clips(C.byref(d), None), "vs_embed_tail_yuv_clips")
    torch.cuda.synchronize()
    for i, ((n, F_), src, dst) in enumerate(zip(slots, srcs, dsts)):
        H, W = U.SIZES[n][:2]
        keys = U.cdiv(F_, STEP)
        ref = empty_like(fmt, n, F_)
        d1 = U.tail_desc(src.surface(fmt), ref.surface(fmt), F_, H, W, fmt, PRESET, eng.taps43, delta[fk[i]:fk[i] + keys].contiguous(),
                         None if hm is None else hm[ff[i] * S * S:(ff[i] + F_) * S * S], step=STEP, video_mode=mode, Cd=Cd)
        N.check(lib.vs_embed_tail_yuv(C.byref(d1), None), "vs_embed_tail_yuv")
        torch.cuda.synchronize()
        for p, (a, b) in enumerate(zip(dst.bviews, ref.bviews)):
            assert torch.equal(a, b), (fmt, n, F_, mode, Cd, full_jnd, "plane", p)
        assert not torch.equal(dst.bviews[0], src.bviews[0])                                      # the slot was watermarked
        assert dst.untouched_outside() and ref.untouched_outside(), (fmt, n, F_, mode, Cd, full_jnd)     # guards, pitch padding, spare rows


# ---------------------------------------------------------------------------------------------------- 2. tail, byte for byte
@pytest.mark.parametrize("fmt", U.FORMATS)
def test_tail_list_equals_the_per_slot_tile_call(fmt, tiny):
    """vs_embed_tail_yuv_clips == vs_embed_tail_yuv(variant = 1) per slot, byte for byte: the three video modes, Cd 1 and 3, the
    low-resolution heat-map and the full-resolution JND; sources unchanged; every guard byte, every pitch-padding byte and every spare row of
    the destinations still poison"""
    eng = tiny[2]._engine()
    slots = slots_of(fmt)
    srcs = [pitched(fmt, n, F_, "noise") for n, F_ in slots]
    keep = [[b.clone() for b in s.bufs] for s in srcs]
    for j, (mode, Cd, full_jnd) in enumerate(itertools.product((0, 1, 2), (1, 3), (False, True))):
        run_tail(fmt, slots, srcs, eng, mode=mode, Cd=Cd, full_jnd=full_jnd, seed=60 + j)
    assert all(torch.equal(a, b) for s, k in zip(srcs, keep) for a, b in zip(s.bufs, k))
    assert all(s.untouched_outside() for s in srcs)


# ---------------------------------------------------------------------------------------------------- 3. more slots than a launch holds
@pytest.mark.parametrize("fmt", ["nv12", "yuv422p10", "yuv444p"])
def test_more_slots_than_a_launch_holds(fmt, tiny):
    """PER_LAUNCH + 3 one-frame slots alternating 18 x 34 and 72 x 88 in one call: the equalities of tests 1 and 2 -- no slot is skipped
    (every slot equals its per-slot result) and none is written twice or elsewhere (the poison outside, the NaN rows nobody owns)"""
    eng = tiny[2]._engine()
    slots = [("DB"[i % 2], 1) for i in range(PER + 3)]
    assert len(N.yuv_clips_plan([(1, *U.SIZES[n][:2]) for n, _ in slots], fmt, N.IMAGES_TAIL, S, S, True)) == 2
    srcs = [U.Pitched(U.to_t(U.random_clip(1, *U.SIZES[n][:2], fmt, seed=100 + i)), U.SIZES[n][2], U.SIZES[n][3]) for i, (n, _) in enumerate(slots)]
    for aa, key_step in ((True, 2), (False, 1)):
        run_resize(fmt, slots, srcs, aa, key_step)
    run_tail(fmt, slots, srcs, eng, mode=2, Cd=1, full_jnd=False, seed=80)
    run_tail(fmt, slots, srcs, eng, mode=0, Cd=3, full_jnd=True, seed=81)


# ---------------------------------------------------------------------------------------------------- 4. refusals launch nothing
def test_refusals_launch_nothing(tiny):
    """every refusal of videoseal_yuv_clips.h: its code, and no output touched -- the bad descriptor is the LAST of the list, so a launcher
    that checked as it went would have written the first slots"""
    eng = tiny[2]._engine()
    lib = N.lib()
    BAD, UNS = -1, N.ERR_UNSUPPORTED
    slots = [("B", 3), ("D", 1), ("A", 2)]
    ff, fk, nf, nk = layout(slots, STEP)
    rgb = torch.full((nf, S, S, 4), NAN, device="cuda")
    key = torch.full((nk, S, S, 4), NAN, device="cuda")
    delta = torch.ones(nk, 1, S, S, device="cuda")
    hm = torch.ones(nf * S * S, device="cuda")
    made = {}

    def fresh(fmt="nv12"):
        if fmt not in made:
            made[fmt] = ([pitched(fmt, n, F_) for n, F_ in slots], [empty_like(fmt, n, F_) for n, F_ in slots])
        srcs, dsts = made[fmt]
        return U.slot_descs(fmt, [(s, d, F_, *U.SIZES[n][:2], ff[i], fk[i]) for i, ((n, F_), s, d) in enumerate(zip(slots, srcs, dsts))])

    def resize(arr, n=3, dec=U.aff(PRESET, 8)[0], oh=S, rgb_=rgb, key_=key, key_step=STEP):
        return lib.vs_resize_pre_yuv_clips(arr, n, dec, oh, S, 1, N.ptr(rgb_) if rgb_ is not None else None, 1.0, 0.0,
                                           N.ptr(key_) if key_ is not None else None, key_step, None, None)

    def tail(arr, n=3, fmt="nv12", **kw):
        d = U.tail_clips_desc(arr, n, fmt, PRESET, eng.taps43, delta, hm, step=STEP, video_mode=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.vs_embed_tail_yuv_clips(C.byref(d), None)

    def both(arr, want, **kw):
        assert resize(arr, **kw) == want and tail(arr, **kw) == want

    arr = fresh()
    assert resize(None) == BAD and resize(arr, n=0) == BAD and resize(arr, dec=None) == BAD and resize(arr, oh=0) == BAD
    assert resize(arr, rgb_=None, key_=None) == BAD and resize(arr, key_step=0) == BAD
    assert lib.vs_embed_tail_yuv_clips(None, None) == BAD and tail(None) == BAD and tail(arr, n=0) == BAD and tail(arr, delta=None) == BAD
    assert tail(arr, clamp=0) == BAD and tail(arr, step=0) == BAD and tail(arr, video_mode=3) == BAD and tail(arr, Cd=2) == BAD
    assert tail(arr, attenuate=2) == UNS and tail(arr, hmap_lowres=None, taps43=None) == BAD
    for member, value in (("F", 0), ("H", -1), ("W", 0), ("first_frame", -1), ("first_key", -2), ("H", 133), ("W", 201)):
        arr = fresh()
        setattr(arr[2], member, value)                                      # (133, 201: sizes the 4:2:0 rule forbids)
        both(arr, BAD)
    arr = fresh("nv16")
    arr[2].W = 201
    assert resize(arr) == BAD and tail(arr, fmt="nv16") == BAD              # 4:2:2 needs W even
    arr = fresh()
    arr[2].src.plane[1] = None
    both(arr, BAD)
    arr = fresh()
    arr[2].src.pitch[0] = 201                                               # shorter than a row
    both(arr, BAD)
    arr = fresh()
    arr[2].src.frame_stride[1] = arr[2].src.pitch[1] * 66 + 201             # frames overlap by one byte
    both(arr, BAD)
    arr = fresh()
    arr[2].dst.pitch[1] = 200
    assert tail(arr) == BAD
    arr = fresh()
    arr[2].dst.plane[0] = None
    assert tail(arr) == BAD
    arr = fresh()
    arr[0].src.depth = arr[0].dst.depth = 12                                # a format outside the ten
    both(arr, UNS)
    arr, other = fresh(), fresh("nv16")
    arr[2].src, arr[2].dst = other[2].src, other[2].dst                     # slots of different formats
    both(arr, UNS)
    arr = fresh()
    arr[2].dst = other[2].dst                                               # a slot whose src and dst formats differ
    assert tail(arr) == UNS
    torch.cuda.synchronize()
    assert bool(torch.isnan(rgb).all()) and bool(torch.isnan(key).all())
    for srcs, dsts in made.values():
        assert all(bool((b == d.poison).all()) for d in dsts for b in d.bufs)
    arr = fresh()                                                           # ... and the list itself is a good one
    assert resize(arr) == 0 and tail(arr) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(rgb[ff[0]:ff[0] + 3]).any())


# ---------------------------------------------------------------------------------------------------- model level
def model_clips(fmt, kind="smooth", names=None, preset=PRESET):
    """[(numpy planes, device views at their own pitches)] of the format's list"""
    out = []
    for n, F_ in (names or slots_of(fmt)):
        p = clip_np(fmt, n, F_, kind, preset)
        out.append((p, U.Pitched(U.to_t(p), U.SIZES[n][2], U.SIZES[n][3], even=True).views))
    return out


# ---------------------------------------------------------------------------------------------------- 5. the composition
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
@pytest.mark.parametrize("fmt", ["nv12", "yuv420p10", "p210", "yuv444p"])
def test_embed_and_detect_equal_the_composition(fmt, which, tiny, tinyc):
    """embed_clips_yuv == per pass of clips.embed_passes: eng.resize_pre per span on yuv.Clip slices, concatenated; ONE eng.embedder_forward
    with a message row per key frame; one eng.jnd_lowres; eng.embed_tail per span with eng.tail_variant = 1 -- byte for byte;
    detect_clips_yuv the same way against per-run resize + one extractor_forward per pass.  lowres_attenuation on and off, the three modes.
    The list is repeated until its key frames pass streaming.KEY_BATCH (twice over for six slots at 14 keys would stay at 28 <= 32: three
    times), so that the embed side needs two passes."""
    spec, sd, model = tiny if which == "tiny" else tinyc
    eng = model._engine()
    base = [v for _, v in model_clips(fmt)]
    reps = 2
    while len(CL.embed_passes([p[0].shape[0] for p in base * reps], STEP, CK)) < 2 and reps < 4:
        reps += 1
    planes = base * reps
    n = len(planes)
    color = (PRESET[0], PRESET[1])
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    lengths = [p[0].shape[0] for p in planes]
    passes = CL.embed_passes(lengths, STEP, CK)
    assert len(passes) >= 2
    att = model.attenuation is not None
    try:
        for lowres, mode in ((True, "repeat"), (False, "alternate"), (True, "interpolate"), (False, "interpolate")):
            _set(model, mode)
            got = model.embed_clips_yuv(planes, fmt, msgs, lowres_attenuation=lowres, matrix=PRESET[0], full_range=PRESET[1])
            assert torch.equal(got["msgs"], msgs) and len(got["planes_w"]) == n
            yc = [yuv.Clip(p, fmt, color) for p in planes]
            mi = model._msgs_dev(msgs, eng.dev)
            eng.tail_variant = 1
            for slots, rows in passes:
                keys, rgbs = [], []
                for c, a, f, _, _ in slots:
                    rgb, key = eng.resize_pre(yc[c][a:a + f], (S, S), True, want_rgb=(att and lowres), want_key=True, key_step=STEP)
                    keys.append(key.t.clone().view(-1, S, S, 4))
                    if rgb is not None:
                        rgbs.append(rgb.t.clone().view(-1, S, S, 4))
                key = Act(torch.cat(keys).contiguous(), len(rows), S, S, spec.in_ch, 4)
                delta = eng.embedder_forward(key, mi[torch.tensor(rows, device="cuda")].contiguous(), bn_train=False)
                hmap = eng.jnd_lowres(Act(torch.cat(rgbs).contiguous(), sum(s[2] for s in slots), S, S, 3, 4)) if rgbs else None
                for c, a, f, ff, fk in slots:
                    out = yc[c][a:a + f].empty_like()
                    eng.embed_tail(yc[c][a:a + f], out, delta[fk:fk + U.cdiv(f, STEP)], step=STEP, video_mode=N.VIDEO_MODES[mode],
                                   hmap_low=(hmap[ff * S * S:(ff + f) * S * S] if hmap is not None else None), attenuate=int(att), clamp=model.clamp,
                                   antialias=True, scaling_i=model.blender.scaling_i, scaling_w=model.blender.scaling_w)
                    for p, (o, w) in enumerate(zip(out.planes, got["planes_w"][c])):
                        assert _same(o, w[a:a + f]), (fmt, which, lowres, mode, c, a, "plane", p)
            eng.tail_variant = 0
            for c, (w, buf) in enumerate(zip(got["planes_w"], got["imgs_w"])):
                assert all(p.is_cuda and p.dtype == yuv.fmt_dtype(fmt) for p in w) and buf.shape[0] == lengths[c] and buf.is_contiguous()
                assert not _same(w[0], planes[c][0])
        # the results of device-resident clips are views of one allocation, clip after clip
        bufs = got["imgs_w"]
        assert all(b.untyped_storage().data_ptr() == bufs[0].untyped_storage().data_ptr() for b in bufs)
        assert all(b1.data_ptr() == b0.data_ptr() + b0.numel() * b0.element_size() for b0, b1 in zip(bufs, bufs[1:]))
        # detect
        got_w = got["planes_w"]
        got_p = [p.clone() for p in model.detect_clips_yuv(got_w, fmt, matrix=PRESET[0], full_range=PRESET[1])["preds"]]
        wc = [yuv.Clip(p, fmt, color) for p in got_w]
        preds = []
        for dslots in CL.detect_passes(lengths):
            rgbs = []
            for c, a, f, _ in dslots:
                rgb, _ = eng.resize_pre(wc[c][a:a + f], (S, S), True, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
                rgbs.append(rgb.t.clone().view(-1, S, S, 4))
            preds.append(eng.extractor_forward(Act(torch.cat(rgbs).contiguous(), sum(s[2] for s in dslots), S, S, 3, 4)).clone())
        assert torch.equal(torch.cat(preds), torch.cat(got_p))
        assert all(p.shape == (f, spec.nbits + 1) for p, f in zip(got_p, lengths))
    finally:
        eng.tail_variant = 0
        _set(model)


# ---------------------------------------------------------------------------------------------------- 6. one clip in one span
@pytest.mark.parametrize("fmt,name", [("nv12", "A"), ("p010", "C"), ("yuv422p", "E"), ("yuv444p10", "G"), ("i420", "D")])
def test_one_clip_in_one_span_equals_embed_yuv_and_detect_yuv(fmt, name, tiny):
    """a list of one clip that fits one span is the per-clip call with the same batch shape: byte for byte with the default low-resolution
    heat-map (there the tile tail of the list and the row-streaming tail of the per-clip call agree), the three modes"""
    spec, sd, model = tiny
    msgs = synthetic_msgs(1, spec.nbits, seed=21)
    kw = dict(matrix=PRESET[0], full_range=PRESET[1])
    (_, views), = model_clips(fmt, names=[(name, 3)])
    try:
        for mode in ("repeat", "alternate", "interpolate"):
            _set(model, mode)
            a = model.embed_clips_yuv([views], fmt, msgs, **kw)["planes_w"][0]
            b = model.embed_yuv(views, fmt, msgs, **kw)["planes_w"]
            assert all(_same(x, y) for x, y in zip(a, b)), (fmt, name, mode)
        two = tuple(p[:2] for p in a)
        assert torch.equal(model.detect_clips_yuv([two], fmt, **kw)["preds"][0], model.detect_yuv(two, fmt, **kw)["preds"])
        assert torch.equal(model.detect_clips_yuv([two], fmt, interpolation=NA, **kw)["preds"][0], model.detect_yuv(two, fmt, interpolation=NA, **kw)["preds"])
    finally:
        _set(model)


# ---------------------------------------------------------------------------------------------------- 7. the torch definition
@pytest.mark.parametrize("fmt", ["nv12", "p010", "yuv422p10", "yuv444p"])
def test_against_the_torch_definition(fmt, tiny):
    """per clip: every output code within 0.5 + (2^depth - 1) * TOL_IMG of the float64 code value of yuv.to_rgb -> embed(is_video=True) ->
    encode (rule and constant of test_embed_equals_the_composition in tests/test_gpu_yuv.py); logits within TOL_LOGIT of
    detect(yuv.to_rgb(...)); assert_decisions(min_sure = 0.99).  synthetic_frames clips."""
    spec, sd, model = tiny
    clips = model_clips(fmt)
    n = len(clips)
    msgs = synthetic_msgs(n, spec.nbits, seed=7)
    top = (1 << U.depth_of(fmt)) - 1
    kw = dict(matrix=PRESET[0], full_range=PRESET[1])
    worst = 0.0
    try:
        for lowres, mode in ((True, "repeat"), (False, "interpolate"), (True, "alternate")):
            _set(model, mode)
            got = model.embed_clips_yuv([v for _, v in clips], fmt, msgs, lowres_attenuation=lowres, **kw)["planes_w"]
            preds = model.detect_clips_yuv(got, fmt, **kw)["preds"]
            for i, (p, _) in enumerate(clips):
                rgb = yuv.to_rgb(U.to_t(p), fmt, *PRESET).cuda()
                w = model.embed(rgb, msgs[i:i + 1], is_video=True, lowres_attenuation=lowres)["imgs_w"]
                want = R.encode_values(w.cpu().double().numpy(), fmt, *PRESET)
                out = tuple(x.cpu().contiguous().view(torch.uint8).numpy().view(np.uint16 if x.element_size() == 2 else np.uint8) for x in got[i])
                for g, v in zip(R.codes_of(out, fmt), want):
                    err = np.abs(g.astype(np.float64) - v).max()
                    worst = max(worst, err)
                    assert g.shape == v.shape and err <= 0.5 + top * TOL_IMG, (fmt, i, lowres, mode, err)
                ref = model.detect(yuv.to_rgb(tuple(x.cpu() for x in got[i]), fmt, *PRESET).cuda(), is_video=True)["preds"]
                assert (preds[i] - ref).abs().max().item() < TOL_LOGIT, (fmt, i, lowres, mode)
                assert_decisions(preds[i], ref, what=f"detect_clips_yuv {fmt} clip {i}", min_sure=0.99)
    finally:
        _set(model)
    print(f"embed_clips_yuv {fmt}: max |code - v| = {worst:.4f}")


# ---------------------------------------------------------------------------------------------------- 8. extract_messages_yuv
def test_extract_messages_yuv(tiny):
    """row i == extract_message of clip i's RGB for the four aggregations, wherever the aggregated logit of that reference clears
    DECISION_MARGIN (assert_decisions: at most 1 % of the logits inside it); a zero-frame clip gives all-False"""
    spec, sd, model = tiny
    fmt = "p010"
    kw = dict(matrix=PRESET[0], full_range=PRESET[1])
    _set(model)
    clips = model_clips(fmt)
    msgs = synthetic_msgs(len(clips), spec.nbits, seed=9)
    w = model.embed_clips_yuv([v for _, v in clips], fmt, msgs, **kw)["planes_w"]
    rgbs = [yuv.to_rgb(tuple(x.cpu() for x in p), fmt, *PRESET).cuda() for p in w]
    logits = [model.detect(r, is_video=True, interpolation=NA)["preds"][:, 1:] for r in rgbs]
    empty = tuple(p[:0] for p in w[0])
    for aggregation in ("avg", "squared_avg", "l1norm_avg", "l2norm_avg"):
        got = model.extract_messages_yuv(list(w) + [empty], fmt, aggregation, **kw)
        assert got.dtype == torch.bool and got.shape == (len(w) + 1, spec.nbits) and got.is_cuda and not bool(got[-1].any())
        one = torch.cat([model.extract_message(r, aggregation) for r in rgbs])
        gold = torch.stack([aggregate_bits(lg, aggregation) for lg in logits]).cpu()
        assert_decisions(got[:-1].float() * 2 - 1, gold, what=f"extract_messages_yuv {aggregation}", min_sure=0.99)
        sure = gold.abs() > DECISION_MARGIN
        assert torch.equal(one.cpu().bool()[sure], got[:-1].cpu()[sure])


# ---------------------------------------------------------------------------------------------------- 9. host-resident lists
def test_host_resident_list_equals_the_device_resident_one(tiny):
    """a list of host-resident clips moves pass by pass and gives the bytes of the device-resident list; results live on the clips' devices"""
    spec, sd, model = tiny
    fmt = "yuv422p10"
    kw = dict(matrix=PRESET[0], full_range=PRESET[1])
    _set(model, "interpolate")
    try:
        clips = model_clips(fmt)
        msgs = synthetic_msgs(len(clips), spec.nbits, seed=5)
        none = tuple(v[:0] for v in clips[1][1])                                          # a clip of 0 frames is allowed, in either list
        msgs = synthetic_msgs(len(clips) + 1, spec.nbits, seed=5)
        dev = model.embed_clips_yuv([v for _, v in clips] + [none], fmt, msgs, **kw)
        host = model.embed_clips_yuv([U.to_t(p) for p, _ in clips] + [tuple(x.cpu() for x in none)], fmt, msgs, **kw)
        assert dev["planes_w"][-1][0].shape == none[0].shape and dev["imgs_w"][-1].shape[0] == 0 and host["imgs_w"][-1].shape[0] == 0
        for a, b in zip(dev["planes_w"], host["planes_w"]):
            assert all(not y.is_cuda and _same(x.cpu(), y) for x, y in zip(a, b))
        assert all(not b.is_cuda for b in host["imgs_w"])
        pd = model.detect_clips_yuv(dev["planes_w"], fmt, **kw)["preds"]
        ph = model.detect_clips_yuv(host["planes_w"], fmt, **kw)["preds"]
        assert all(not y.is_cuda and torch.equal(x.cpu(), y) for x, y in zip(pd, ph))
        assert torch.equal(model.extract_messages_yuv(host["planes_w"], fmt, **kw), model.extract_messages_yuv(dev["planes_w"], fmt, **kw).cpu())
        # surface slots take no per-frame strength and no preds_w
        eng = model._engine()
        c = yuv.Clip(clips[0][1], fmt, PRESET)
        with pytest.raises(NotImplementedError):
            eng.embed_tail_clips([(c, 0, 0)], [c.empty_like()], torch.zeros(1, 1, S, S, device="cuda"), step=2, video_mode=0, hmap_low=None, attenuate=0,
                                 clamp=True, antialias=True, scaling_i=1.0, scaling_w=0.2, frame_scale=torch.ones(1, device="cuda"))
    finally:
        _set(model)
