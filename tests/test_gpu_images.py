"""Lists of images of different sizes on the HIP path: vs_resize_pre_images / vs_embed_tail_images against the per-image calls (bit for bit),
embed_images / detect_images against the composition of the existing pieces (bit for bit), against embed / detect on equal sizes (bit for bit),
against the CPU oracle (the e2e tolerances of tests/_model.py) and against embed_u8 / detect_u8 (one byte, the criterion of
test_uint8_rgb24_clip_path).  Tiny model, processing size 64; the size list holds the smallest shapes at which each code path can go wrong."""
import ctypes as C

import pytest
import torch

from oracle import videoseal_ref as R
from oracle.inputs import synthetic_frames, synthetic_msgs
from oracle.weights import make_state_dict, tiny_spec
from tests._guards import GUARD
from tests._model import TOL_IMG, TOL_LOGIT, make_model
from tests._util import assert_decisions
from videoseal_amd import native as N
from videoseal_amd.engine import Act

pytestmark = pytest.mark.gpu

S = 64
# H x W                                                   why it is there
SIZES = [(5, 7),        # up-scaling; smaller than any tile
         (48, 40),      # up-scaling
         (64, 64),      # identity
         (9, 300),      # extreme aspect
         (130, 33),     # W % 4 != 0: rows start at every alignment
         (192, 200),    # scale 3: a streaming form
         (256, 256),    # scale 4: the 64-column streaming form
         (257, 191),    # just past scale 4: the tile form, <= MAXT fails
         (400, 70)]     # vertical scale 6.25 > LONG_TAPS / 2: compensated sums
ORDERS = {"table": list(range(9)), "reversed": list(range(9))[::-1], "35 images": (list(range(9)) * 4)[:35]}
TAPS = (C.c_float * 43)(*([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1]))
YMAT = (C.c_float * 3)(0.299, 0.587, 0.114)
SENT = {torch.float32: -7.0, torch.uint8: 0x5A}


def _images(u8: bool):
    """one seeded image per size (CPU): fp32 [3, H, W] in [0, 1] or uint8 [H, W, 3]"""
    out = []
    for i, (h, w) in enumerate(SIZES):
        x = synthetic_frames(1, h, w, seed=40 + i, kind="uniform" if min(h, w) < 16 else "smooth")[0]
        out.append((x * 255).to(torch.uint8).permute(1, 2, 0).contiguous() if u8 else x.contiguous())
    return out


def _carved(imgs, fill=None):
    """(buffer, views): the images inside ONE device allocation, each at an odd element offset behind a gap -- base pointers 4-byte aligned for
    fp32 and 1-byte aligned for uint8, nothing more -- between two GUARD-wide bands.  fill: the sentinel of an output buffer (views then hold
    it too), None: an input buffer (views hold the images, the gaps NaN / 0)"""
    dt = imgs[0].dtype
    offs, pos = [], GUARD
    for t in imgs:
        pos += 65                           # an odd offset, at least 65 elements behind the previous image
        pos += (pos % 2 == 0)
        offs.append(pos)
        pos += t.numel()
    total = pos + GUARD
    if fill is None:
        buf = torch.full((total,), float("nan") if dt.is_floating_point else 0, dtype=dt, device="cuda")
    else:
        buf = torch.full((total,), fill, dtype=dt, device="cuda")
    views = []
    for t, o in zip(imgs, offs):
        assert o % 2 == 1
        v = buf[o:o + t.numel()].view(t.shape)
        if fill is None:
            v.copy_(t)
        views.append(v)
    return buf, views


def _only_views_written(buf, views, fill) -> bool:
    """every element of the allocation outside the views still holds the sentinel: the bands around the whole allocation and around every image"""
    c = buf.clone()
    base = buf.data_ptr()
    for v in views:
        o = (v.data_ptr() - base) // buf.element_size()
        c[o:o + v.numel()] = fill
    return bool((c == fill).all())


def _guarded_frames(n, fill=-7.0):
    buf = torch.full((GUARD + n * S * S * 4 + GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + n * S * S * 4].view(n, S, S, 4)


def _bands_intact(buf, fill=-7.0) -> bool:
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


# ---------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("u8", [False, True])
def test_resize_pre_images_equals_the_per_image_call(u8, aa):
    """the whole list in one call: every output frame has the bits vs_resize_pre / vs_resize_pre_u8 gives that image alone (from an aligned
    allocation of its own); dst_rgb, dst_key with and without ymat3; the list reversed; the list repeated to 35 images (two launches per form
    past 32); inputs at odd offsets of one buffer; nothing written outside the n frames"""
    L = N.lib()
    host = _images(u8)
    alone = [t.cuda() for t in host]
    for ymat in (YMAT, None):
        ref = []
        for t in alone:          # the reference, once per size
            H, W = (t.shape[0], t.shape[1]) if u8 else (t.shape[1], t.shape[2])
            rgb, key = torch.full((1, S, S, 4), -7.0, device="cuda"), torch.full((1, S, S, 4), -7.0, device="cuda")
            if u8:
                N.check(L.vs_resize_pre_u8(N.ptr(t), 1, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), 1, ymat, N.stream()), "vs_resize_pre_u8")
            else:
                N.check(L.vs_resize_pre(N.ptr(t), 1, 3, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), 1, ymat, N.stream()), "vs_resize_pre")
            ref.append((rgb[0], key[0]))
        for name, order in ORDERS.items():
            _, views = _carved([host[i] for i in order])
            n = len(order)
            for want_rgb, want_key in ((True, True), (True, False), (False, True)):
                brgb, rgb = _guarded_frames(n)
                bkey, key = _guarded_frames(n)
                N.check(L.vs_resize_pre_images(N.image_descs(views), n, int(u8), S, S, aa, N.ptr(rgb) if want_rgb else None, 2.0, -1.0,
                                               N.ptr(key) if want_key else None, ymat, N.stream()), "vs_resize_pre_images")
                torch.cuda.synchronize()
                assert _bands_intact(brgb) and _bands_intact(bkey), (name, want_rgb, want_key)
                for k, i in enumerate(order):
                    if want_rgb:
                        assert torch.equal(rgb[k], ref[i][0]), (name, k, SIZES[i], "rgb", float((rgb[k] - ref[i][0]).abs().max()))
                    else:
                        assert bool((rgb[k] == -7.0).all())
                    if want_key:
                        assert torch.equal(key[k], ref[i][1]), (name, k, SIZES[i], "key", float((key[k] - ref[i][1]).abs().max()))
                    else:
                        assert bool((key[k] == -7.0).all())


def _tail_alone(L, t, out, pw, delta_i, hm_i, *, u8, att, clamp, aa, Cd):
    d = N.TailDesc()
    H, W = (t.shape[0], t.shape[1]) if u8 else (t.shape[1], t.shape[2])
    d.imgs, d.out, d.preds_w = N.ptr(t), N.ptr(out), N.ptr(pw)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta_i), N.ptr(hm_i), C.cast(TAPS, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = 1, H, W, S, S, Cd
    d.step, d.video_mode, d.total_key = 1, 0, 1
    d.attenuate, d.clamp, d.antialias = att, clamp, aa
    d.scaling_i, d.scaling_w, d.io_u8, d.variant = 1.0, 0.2, int(u8), 0
    N.check(L.vs_embed_tail(C.byref(d), N.stream()), "vs_embed_tail")


def _tail_images(L, views, outs, pws, delta, hm, *, u8, att, clamp, aa, Cd) -> int:
    d = N.TailImagesDesc()
    descs = N.image_descs(views, outs, pws)
    d.images, d.n = descs, len(views)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), N.ptr(hm), C.cast(TAPS, C.c_void_p)
    d.S_h, d.S_w, d.Cd = S, S, Cd
    d.attenuate, d.clamp, d.antialias, d.io_u8 = att, clamp, aa, int(u8)
    d.scaling_i, d.scaling_w = 1.0, 0.2
    return L.vs_embed_tail_images(C.byref(d), N.stream())


@pytest.mark.parametrize("Cd", [1, 3])
@pytest.mark.parametrize("u8", [False, True])
def test_embed_tail_images_equals_the_per_image_call(u8, Cd):
    """every output image (and preds_w) has the bits vs_embed_tail with F = 1 gives that image alone: hmap_lowres given or not, full-resolution
    JND on or off, clamp on and off (fp32), preds_w on and off, both antialias settings; the three lists.  Inputs and outputs are carved at odd
    offsets out of one allocation each; every element between and around the output images still holds the sentinel afterwards."""
    L = N.lib()
    host = _images(u8)
    alone = [t.cuda() for t in host]
    g = torch.Generator(device="cuda").manual_seed(17 + Cd)
    delta9 = (0.3 * torch.randn(9, Cd, S, S, device="cuda", generator=g)).contiguous()
    hm9 = torch.rand(9, S, S, device="cuda", generator=g).contiguous()
    odt = torch.uint8 if u8 else torch.float32
    pw_like = [torch.empty((Cd,) + tuple(hw)) for hw in SIZES]          # (shapes only)
    for att, low in ((1, False), (1, True), (0, False)):
        for clamp in ((1,) if u8 else (1, 0)):
            for aa in (1, 0):
                ref = []
                for i, t in enumerate(alone):          # the reference, once per size
                    out = torch.full_like(t, SENT[odt])
                    pw = torch.full((Cd,) + (t.shape[:2] if u8 else t.shape[1:]), -7.0, device="cuda")
                    _tail_alone(L, t, out, pw, delta9[i:i + 1], hm9[i:i + 1] if low else None, u8=u8, att=att, clamp=clamp, aa=aa, Cd=Cd)
                    ref.append((out, pw))
                for name, order in ORDERS.items():
                    n = len(order)
                    _, views = _carved([host[i] for i in order])
                    delta = delta9[order].contiguous()
                    hm = hm9[order].contiguous() if low else None
                    for want_pw in (True, False):
                        obuf, outs = _carved([host[i] for i in order], fill=SENT[odt])
                        pbuf, pws = _carved([pw_like[i] for i in order], fill=-7.0)
                        rc = _tail_images(L, views, outs, pws if want_pw else None, delta, hm, u8=u8, att=att, clamp=clamp, aa=aa, Cd=Cd)
                        torch.cuda.synchronize()
                        what = (name, att, low, clamp, aa, want_pw)
                        assert rc == 0, what
                        assert _only_views_written(obuf, outs, SENT[odt]), what
                        assert _only_views_written(pbuf, pws, -7.0) and (want_pw or bool((pbuf == -7.0).all())), what
                        for k, i in enumerate(order):
                            assert torch.equal(outs[k], ref[i][0]), what + (k, SIZES[i])
                            if want_pw:
                                assert torch.equal(pws[k], ref[i][1]), what + (k, SIZES[i], "preds_w")


def test_refusals_launch_nothing():
    """null pointers, n <= 0, H or W <= 0, uint8 without clamp, the training order: an error code, and no output touched -- the bad descriptor
    is the LAST of the list, so a launcher that checked as it went would have written the first images"""
    L = N.lib()
    host = _images(False)[:3]
    _, views = _carved(host)
    delta = torch.zeros(3, 1, S, S, device="cuda")

    def descs(**bad):
        d = N.image_descs(views, outs)
        for k, v in bad.items():
            setattr(d[2], k, v)
        return d

    obuf, outs = _carved(host, fill=-7.0)
    brgb, rgb = _guarded_frames(3)
    for n, bad in ((3, dict(img=None)), (3, dict(H=0)), (3, dict(W=-4)), (0, {}), (-1, {})):
        assert L.vs_resize_pre_images(descs(**bad), n, 0, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, None, N.stream()) == -1, (n, bad)
    assert L.vs_resize_pre_images(descs(), 3, 0, S, S, 1, None, 1.0, 0.0, None, None, N.stream()) == -1          # no destination
    assert L.vs_resize_pre_images(descs(), 3, 0, 0, S, 1, N.ptr(rgb), 1.0, 0.0, None, None, N.stream()) == -1

    def tail(dd, n, **kw):
        d = N.TailImagesDesc()
        d.images, d.n = dd, n
        d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), None, C.cast(TAPS, C.c_void_p)
        d.S_h, d.S_w, d.Cd, d.attenuate, d.clamp, d.antialias, d.io_u8 = S, S, 1, 1, 1, 1, 0
        d.scaling_i, d.scaling_w = 1.0, 0.2
        for k, v in kw.items():
            setattr(d, k, v)
        return L.vs_embed_tail_images(C.byref(d), N.stream())
    for n, bad in ((3, dict(img=None)), (3, dict(out=None)), (3, dict(H=0)), (3, dict(W=0)), (0, {}), (-2, {})):
        assert tail(descs(**bad), n) == -1, (n, bad)
    assert tail(descs(), 3, delta=None) == -1 and tail(descs(), 3, Cd=2) == -1 and tail(descs(), 3, taps43=None) == -1
    assert tail(descs(), 3, io_u8=1, clamp=0) == -1                      # (x * 255).byte() needs [0, 1]
    assert tail(descs(), 3, attenuate=2) == N.ERR_UNSUPPORTED            # the training forward's order: clips only
    torch.cuda.synchronize()
    assert bool((obuf == -7.0).all()) and bool((brgb == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- model level
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


@pytest.fixture(scope="module")
def mixed():
    """the mixed list (CPU, fp32) every model-level test shares; never written to"""
    return _images(False)


@pytest.mark.parametrize("lowres", [False, True])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_embed_and_detect_images_equal_the_composition(which, lowres, tiny, tinyc, mixed):
    """embed_images on the mixed list == per-image eng.resize_pre concatenated, ONE eng.embedder_forward over the batch, one eng.jnd_lowres,
    per-image eng.embed_tail -- bit for bit, which pins everything the image-list route adds; detect_images the same way against per-image
    resize_pre + one extractor_forward"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    model.chunk_size = 32
    imgs = [t.cuda() for t in mixed]
    n = len(imgs)
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    got = model.embed_images(imgs, msgs, lowres_attenuation=lowres)
    got_w = [t.clone() for t in got["imgs_w"]]
    got_pw = [t.clone() for t in got["preds_w"]]
    got_p = model.detect_images(got_w)["preds"].clone()
    assert torch.equal(got["msgs"], msgs) and all(w.shape == t.shape and w.is_cuda for w, t in zip(got_w, imgs))
    eng = model._engine()
    att = model.attenuation is not None
    keys, rgbs = [], []
    for t in imgs:
        rgb, key = eng.resize_pre(t[None], (S, S), True, want_rgb=(att and lowres), want_key=True)
        keys.append(key.t.clone().view(1, S, S, 4))
        if rgb is not None:
            rgbs.append(rgb.t.clone().view(1, S, S, 4))
    key = Act(torch.cat(keys).contiguous(), n, S, S, spec.in_ch, 4)
    delta = eng.embedder_forward(key, model._msgs_dev(msgs, eng.dev), bn_train=False)
    hmap = eng.jnd_lowres(Act(torch.cat(rgbs).contiguous(), n, S, S, 3, 4)) if rgbs else None
    for i, t in enumerate(imgs):
        out = torch.empty_like(t[None])
        pw = torch.empty(1, spec.out_ch, t.shape[1], t.shape[2], device="cuda")
        eng.embed_tail(t[None], out, delta[i:i + 1], step=1, video_mode=0, hmap_low=(hmap[i * S * S:(i + 1) * S * S] if hmap is not None else None),
                       attenuate=int(att), clamp=model.clamp, antialias=True, scaling_i=model.blender.scaling_i, scaling_w=model.blender.scaling_w,
                       preds_w=pw)
        assert torch.equal(out[0], got_w[i]), (i, SIZES[i], float((out[0] - got_w[i]).abs().max()))
        assert torch.equal(pw[0], got_pw[i]), (i, SIZES[i], "preds_w")
    rgbs = []
    for t in got_w:
        rgb, _ = eng.resize_pre(t[None], (S, S), True, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
        rgbs.append(rgb.t.clone().view(1, S, S, 4))
    preds = eng.extractor_forward(Act(torch.cat(rgbs).contiguous(), n, S, S, 3, 4))
    assert torch.equal(preds, got_p)


@pytest.mark.parametrize("lowres", [False, True])
def test_equal_sizes_equal_embed_and_detect_on_the_stacked_batch(tiny, lowres):
    spec, sd, model = tiny
    model.chunk_size = 32
    x = synthetic_frames(5, 96, 80, seed=21).cuda()
    msgs = synthetic_msgs(5, spec.nbits, seed=21)
    a = model.embed_images(list(x), msgs, lowres_attenuation=lowres)
    b = model.embed(x, msgs, is_video=False, lowres_attenuation=lowres)
    assert torch.equal(torch.stack(a["imgs_w"]), b["imgs_w"]) and torch.equal(torch.stack(a["preds_w"]), b["preds_w"])
    assert torch.equal(model.detect_images(a["imgs_w"])["preds"], model.detect(b["imgs_w"], is_video=False)["preds"])
    na = {"mode": "bilinear", "align_corners": False, "antialias": False}
    assert torch.equal(model.detect_images(a["imgs_w"], interpolation=na)["preds"], model.detect(b["imgs_w"], is_video=False, interpolation=na)["preds"])


@pytest.mark.parametrize("lowres", [False, True])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_images_against_the_oracle(which, lowres, tiny, tinyc, mixed):
    """per image R.embed_image / R.detect of the CPU oracle: the bounds every e2e test uses (tests/_model.py), decisions through assert_decisions"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    model.chunk_size = 32
    n = len(mixed)
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    got = model.embed_images([t.cuda() for t in mixed], msgs, lowres_attenuation=lowres)
    preds = model.detect_images(got["imgs_w"])["preds"].cpu()
    clean = model.detect_images([t.cuda() for t in mixed])["preds"].cpu()
    pref, cref = [], []
    for i, t in enumerate(mixed):
        ref = R.embed_image(sd, spec, t[None], msgs[i:i + 1], lowres_attenuation=lowres)
        err = (got["imgs_w"][i].cpu() - ref["imgs_w"][0]).abs().max().item()
        assert err < TOL_IMG, (i, SIZES[i], err)
        perr = (got["preds_w"][i].cpu() - ref["preds_w"][0]).abs().max().item()
        assert perr < TOL_IMG, (i, SIZES[i], "preds_w", perr)
        pref.append(R.detect(sd, spec, ref["imgs_w"])["preds"])
        cref.append(R.detect(sd, spec, t[None])["preds"])
    pref, cref = torch.cat(pref), torch.cat(cref)
    assert (preds - pref).abs().max().item() < TOL_LOGIT and (clean - cref).abs().max().item() < TOL_LOGIT
    assert_decisions(preds, pref, what=f"{which} images lowres={lowres}", min_sure=0.99)
    assert_decisions(clean, cref, what=f"{which} clean images", min_sure=0.99)


@pytest.mark.parametrize("lowres", [True, False])
def test_uint8_images_against_the_clip_entry_points(tiny, lowres):
    """uint8 RGB24 lists against embed_u8 / detect_u8 on each image as a one-frame clip: bytes differ by at most 1 (the criterion of
    test_uint8_rgb24_clip_path -- a batch-1 and a batch-n network pass differ in summation order), logits within the e2e bound"""
    spec, sd, model = tiny
    model.chunk_size, model.step_size, model.video_mode = 32, 1, "repeat"
    imgs = [t.cuda() for t in _images(True)]
    msgs = synthetic_msgs(1, spec.nbits, seed=5)
    got = model.embed_images(imgs, msgs.repeat(len(imgs), 1), lowres_attenuation=lowres)
    preds = model.detect_images(imgs)["preds"]
    for i, t in enumerate(imgs):
        assert got["imgs_w"][i].dtype == torch.uint8 and got["imgs_w"][i].shape == t.shape and got["preds_w"][i].shape == (spec.out_ch,) + t.shape[:2]
        ref = model.embed_u8(t[None], msgs, lowres_attenuation=lowres)["imgs_w"][0]
        diff = (ref.int() - got["imgs_w"][i].int()).abs()
        assert diff.max().item() <= 1, (i, SIZES[i], int(diff.max()))
        p = model.detect_u8(t[None])["preds"][0]
        assert (p - preds[i]).abs().max().item() < TOL_LOGIT, (i, SIZES[i])


def test_inputs_chunks_and_errors(tiny, mixed):
    spec, sd, model = tiny
    model.chunk_size = 32
    dev = [t.cuda() for t in mixed]
    n = len(dev)
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    want = model.embed_images(dev, msgs)
    want_p = model.detect_images(dev)["preds"]
    # one allocation per call for device-resident images
    base = want["imgs_w"][0].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for t in want["imgs_w"])
    assert len({t.untyped_storage().data_ptr() for t in want["preds_w"]}) == 1
    # host images round-trip: results on the host, same bits
    host = model.embed_images(mixed, msgs)
    for a, b, c, d in zip(host["imgs_w"], want["imgs_w"], host["preds_w"], want["preds_w"]):
        assert a.device.type == "cpu" and c.device.type == "cpu" and torch.equal(a, b.cpu()) and torch.equal(c, d.cpu())
    hp = model.detect_images(mixed)["preds"]
    assert hp.device.type == "cpu" and torch.equal(hp, want_p.cpu())
    # [1, 3, H, W] entries; a channel-last strided view gives the bits of its contiguous copy
    alt = [t[None] if i % 2 else t.permute(1, 2, 0).contiguous().permute(2, 0, 1) for i, t in enumerate(dev)]
    assert not alt[0].is_contiguous()
    got = model.embed_images(alt, msgs)
    for i, (a, b, c, d) in enumerate(zip(got["imgs_w"], want["imgs_w"], got["preds_w"], want["preds_w"])):
        assert a.shape == alt[i].shape and c.shape == alt[i].shape[:-3] + d.shape
        assert torch.equal(a.reshape(b.shape), b) and torch.equal(c.reshape(d.shape), d)
    assert torch.equal(model.detect_images(alt)["preds"], want_p)
    # the empty list
    e = model.embed_images([], None)
    assert e["imgs_w"] == [] and e["preds_w"] == [] and e["msgs"].shape[0] == 0
    assert tuple(model.detect_images([])["preds"].shape) == (0, spec.nbits + 1)
    # random messages when none are given
    assert model.embed_images(dev[:2])["msgs"].shape == (2, spec.nbits)
    # 35 images, chunk_size 32: two chunks, each what a call on it alone gives
    order = ORDERS["35 images"]
    many = [dev[i] for i in order]
    m35 = synthetic_msgs(35, spec.nbits, seed=35)
    got = model.embed_images(many, m35)
    first, rest = model.embed_images(many[:32], m35[:32]), model.embed_images(many[32:], m35[32:])
    for a, b in zip(got["imgs_w"], first["imgs_w"] + rest["imgs_w"]):
        assert torch.equal(a, b)
    p35 = model.detect_images(got["imgs_w"])["preds"]
    assert p35.shape[0] == 35 and torch.equal(p35[32:], model.detect_images(got["imgs_w"][32:])["preds"])
    # loud errors
    u8 = [(t * 255).to(torch.uint8).permute(1, 2, 0).contiguous() for t in dev[:2]]
    with pytest.raises(ValueError, match="all fp32"):
        model.embed_images([dev[0], u8[1]], msgs[:2])
    with pytest.raises(ValueError, match="all fp32"):
        model.detect_images([dev[0], u8[1]])
    with pytest.raises(ValueError, match="rows"):
        model.embed_images(dev, msgs[:3])
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        model.embed_images([torch.rand(4, 20, 20, device="cuda")], msgs[:1])
    with pytest.raises(ValueError, match="RGB24"):
        model.embed_images([torch.zeros(20, 20, 4, dtype=torch.uint8, device="cuda")], msgs[:1])
    model.clamp = False
    try:
        with pytest.raises(NotImplementedError, match="clamp=True"):
            model.embed_images(u8, msgs[:2])
    finally:
        model.clamp = True
