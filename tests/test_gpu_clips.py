"""Lists of clips on the HIP path: vs_resize_pre_clips / vs_embed_tail_clips against the per-clip / per-span calls (bit for bit), embed_clips /
detect_clips against the composition of the engine pieces on the same passes (bit for bit), a one-span list against embed / detect (bit for
bit), every clip against the CPU oracle (the e2e tolerances of tests/_model.py), uint8 lists against embed_u8 / detect_u8 (one code),
extract_messages against the oracle's decisions, vs_aggregate_clips inside the fp64 envelope.  Tiny cards, processing size 64; the size list
holds the smallest shapes at which each kernel can go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import videoseal_ref as R
from oracle.inputs import synthetic_frames, synthetic_msgs
from oracle.weights import make_state_dict, tiny_spec
from tests import _envelope as E
from tests._guards import GUARD
from tests._model import TOL_IMG, TOL_LOGIT, make_model
from tests._util import DECISION_MARGIN, assert_decisions
from videoseal_amd import clips as CL
from videoseal_amd import native as N
from videoseal_amd.engine import Act
from videoseal_amd.model import aggregate_bits

pytestmark = pytest.mark.gpu

S = 64
CK = 2                  # chunk_size of every test: a span is 2 * step frames
# H x W                                                   why it is there
SIZES = [(5, 7),        # below any tile
         (48, 40),      # up-scaling
         (64, 64),      # identity
         (9, 300),      # two tail tile columns
         (130, 33),     # W % 4 != 0: rows start at every alignment
         (257, 191),    # just past scale 4: the tile form of the resize
         (18, 260)]     # two tile rows x two tile columns of the tail
LENGTHS = (1, 2, 3, 4, 5, 9)
LENS = [int(v) for v in np.random.RandomState(3).permutation(LENGTHS)] + [9]          # one length per size, every length present, 9 twice
TAPS = (C.c_float * 43)(*([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1]))
YMAT = (C.c_float * 3)(0.299, 0.587, 0.114)
SENT = {torch.float32: -7.0, torch.uint8: 0x5A}
NA = {"mode": "bilinear", "align_corners": False, "antialias": False}

# margin of the aggregation envelope (tests/_envelope.py states the rule): twice the largest ratio measured on an MI355X, never above the cap.
# 2 x 0.924: `avg` of the clip with one 1e4 row among 1e-3 rows, F = 2, nbits = 16 -- the kernel's one fp32 rounding against the floor of the
# yardstick (profiles/clips_fp64_envelope.txt lists every case; no kernel error exceeds 2^-24, so no yardstick can raise a ratio past it)
AGG_MARGIN = min(E.CAP, 1.85)
agg_envelope = functools.partial(E.check_rows, "CLIPS-ENVELOPE", 34, "aten-fp32", AGG_MARGIN)


@functools.lru_cache(maxsize=None)
def _clips(u8: bool):
    """one seeded clip per size (CPU, never written to): fp32 [F, 3, H, W] in [0, 1] or uint8 [F, H, W, 3]"""
    out = []
    for i, ((h, w), f) in enumerate(zip(SIZES, LENS)):
        x = synthetic_frames(f, h, w, seed=60 + i, kind="uniform" if min(h, w) < 16 else "smooth")
        out.append((x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() if u8 else x.contiguous())
    return tuple(out)


def _carved(tensors, fill=None):
    """(buffer, views): the tensors inside ONE device allocation, each at an odd element offset behind a gap -- base pointers 4-byte aligned for
    fp32 and 1-byte aligned for uint8, nothing more -- between two GUARD-wide bands.  fill: the sentinel of an output buffer (views then hold
    it too), None: an input buffer (views hold the tensors, the gaps NaN / 0)"""
    dt = tensors[0].dtype
    offs, pos = [], GUARD
    for t in tensors:
        pos += 65
        pos += (pos % 2 == 0)
        offs.append(pos)
        pos += t.numel()
    total = pos + GUARD
    if fill is None:
        buf = torch.full((total,), float("nan") if dt.is_floating_point else 0, dtype=dt, device="cuda")
    else:
        buf = torch.full((total,), fill, dtype=dt, device="cuda")
    views = []
    for t, o in zip(tensors, offs):
        v = buf[o:o + t.numel()].view(t.shape)
        if fill is None:
            v.copy_(t)
        views.append(v)
    return buf, views


def _only_views_written(buf, views, fill) -> bool:
    c = buf.clone()
    base = buf.data_ptr()
    for v in views:
        o = (v.data_ptr() - base) // buf.element_size()
        c[o:o + v.numel()] = fill
    return bool((c == fill).all())


def _guarded_frames(n, fill=-7.0):
    buf = torch.full((GUARD + n * S * S * 4 + GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + n * S * S * 4].view(n, S, S, 4)


def _slots(step, lens=LENS):
    """every span of the list as one pass: [(clip, start, frames, first_frame, first_key)], frames and key frames of the pass"""
    (slots, rows), = CL.embed_passes(lens, step, CK, key_batch=1 << 20)
    return slots, sum(s[2] for s in slots), len(rows)


# ---------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("u8", [False, True])
def test_resize_pre_clips_equals_the_per_clip_call(u8, aa):
    """every frame of dst_rgb and every key frame of dst_key has the bits vs_resize_pre / vs_resize_pre_u8 gives its clip alone (from an aligned
    allocation of its own, key_step = step); key frames land at first_key + f / step and nowhere else (dst_key has exactly the key frames of the
    list between two bands); steps 2 and 4; with and without ymat3; 35 one-frame slots cross the launch limit; inputs at odd offsets"""
    L = N.lib()
    host = _clips(u8)
    alone = [t.cuda() for t in host]
    _, views = _carved(host)
    for step in (2, 4):
        slots, nf, nk = _slots(step)
        for ymat in (YMAT, None):
            ref = []
            for t in alone:
                F_ = t.shape[0]
                H, W = (t.shape[1], t.shape[2]) if u8 else (t.shape[2], t.shape[3])
                rgb, key = torch.full((F_, S, S, 4), -7.0, device="cuda"), torch.full(((F_ + step - 1) // step, S, S, 4), -7.0, device="cuda")
                if u8:
                    N.check(L.vs_resize_pre_u8(N.ptr(t), F_, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), step, ymat, N.stream()), "vs_resize_pre_u8")
                else:
                    N.check(L.vs_resize_pre(N.ptr(t), F_, 3, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), step, ymat, N.stream()), "vs_resize_pre")
                ref.append((rgb, key))
            descs = N.clip_descs([(views[c][a:a + n], ff, fk) for c, a, n, ff, fk in slots])
            for want_rgb, want_key in ((True, True), (True, False), (False, True)):
                brgb, rgb = _guarded_frames(nf)
                bkey, key = _guarded_frames(nk)
                N.check(L.vs_resize_pre_clips(descs, len(slots), int(u8), S, S, aa, N.ptr(rgb) if want_rgb else None, 2.0, -1.0,
                                              N.ptr(key) if want_key else None, step, ymat, N.stream()), "vs_resize_pre_clips")
                torch.cuda.synchronize()
                what = (step, ymat is not None, want_rgb, want_key)
                assert bool((brgb[:GUARD] == -7.0).all() and (brgb[-GUARD:] == -7.0).all() and (bkey[:GUARD] == -7.0).all() and (bkey[-GUARD:] == -7.0).all()), what
                if not want_rgb:
                    assert bool((brgb == -7.0).all()), what
                if not want_key:
                    assert bool((bkey == -7.0).all()), what
                for c, a, n, ff, fk in slots:
                    k = (n + step - 1) // step
                    if want_rgb:
                        assert torch.equal(rgb[ff:ff + n], ref[c][0][a:a + n]), what + (c, a, SIZES[c], "rgb")
                    if want_key:
                        assert torch.equal(key[fk:fk + k], ref[c][1][a // step:a // step + k]), what + (c, a, SIZES[c], "key")
    # 35 one-frame slots (frame 0 of clip k % 7): two launches per form
    order = [k % 7 for k in range(35)]
    descs = N.clip_descs([(views[c][0:1], k, k) for k, c in enumerate(order)])
    brgb, rgb = _guarded_frames(35)
    bkey, key = _guarded_frames(35)
    N.check(L.vs_resize_pre_clips(descs, 35, int(u8), S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), 4, None, N.stream()), "vs_resize_pre_clips")
    torch.cuda.synchronize()
    assert bool((brgb[:GUARD] == -7.0).all() and (brgb[-GUARD:] == -7.0).all() and (bkey[:GUARD] == -7.0).all() and (bkey[-GUARD:] == -7.0).all())
    for k, c in enumerate(order):
        assert torch.equal(rgb[k], ref[c][0][0]) and torch.equal(key[k], ref[c][1][0]), (k, c)


def _tail_alone(L, t, out, pw, delta, hm, *, u8, att, clamp, aa, Cd, step, mode):
    d = N.TailDesc()
    F_ = t.shape[0]
    H, W = (t.shape[1], t.shape[2]) if u8 else (t.shape[2], t.shape[3])
    d.imgs, d.out, d.preds_w = N.ptr(t), N.ptr(out), N.ptr(pw)
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), N.ptr(hm), C.cast(TAPS, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, Cd
    d.step, d.video_mode, d.total_key = step, mode, delta.shape[0]
    d.attenuate, d.clamp, d.antialias = att, clamp, aa
    d.scaling_i, d.scaling_w, d.io_u8, d.variant = 1.0, 0.2, int(u8), 0
    N.check(L.vs_embed_tail(C.byref(d), N.stream()), "vs_embed_tail")


def _tail_clips(L, descs, n, delta, hm, *, u8, att, clamp, aa, Cd, step, mode, **over) -> int:
    d = N.TailClipsDesc()
    d.clips, d.n = descs, n
    d.delta, d.hmap_lowres, d.taps43 = N.ptr(delta), N.ptr(hm), C.cast(TAPS, C.c_void_p)
    d.S_h, d.S_w, d.Cd = S, S, Cd
    d.attenuate, d.clamp, d.antialias, d.io_u8 = att, clamp, aa, int(u8)
    d.scaling_i, d.scaling_w, d.step, d.video_mode = 1.0, 0.2, step, mode
    for k, v in over.items():
        setattr(d, k, v)
    return L.vs_embed_tail_clips(C.byref(d), N.stream())


@pytest.mark.parametrize("Cd", [1, 3])
@pytest.mark.parametrize("u8", [False, True])
def test_embed_tail_clips_equals_the_per_span_call(u8, Cd):
    """every span of the output (and of preds_w) has the bits vs_embed_tail gives that span alone on its own piece of delta / hmap_lowres: the
    three video modes, steps 2 and 4, the low-resolution heat-map, the full-resolution JND and no attenuation, clamp off once (fp32),
    antialias off once, preds_w given and NULL.  Inputs and outputs are carved at odd offsets out of one allocation each; every element
    between and around the output clips still holds the sentinel afterwards."""
    L = N.lib()
    host = _clips(u8)
    alone = [t.cuda() for t in host]
    _, views = _carved(host)
    g = torch.Generator(device="cuda").manual_seed(23 + Cd)
    odt = torch.uint8 if u8 else torch.float32
    pw_like = [torch.empty((f, Cd) + hw) for hw, f in zip(SIZES, LENS)]          # (shapes only)
    for step in (2, 4):
        slots, nf, nk = _slots(step)
        delta = (0.3 * torch.randn(nk, Cd, S, S, device="cuda", generator=g)).contiguous()
        hm_all = torch.rand(nf, S, S, device="cuda", generator=g).contiguous()
        for mode in (0, 1, 2):
            for att, low, clamp, aa in ((1, False, 1, 1), (1, True, 1, 1), (0, False, 1, 1), (1, True, 1, 0)) + (() if u8 else ((1, False, 0, 1),)):
                hm = hm_all if low else None
                ref = []
                for c, a, n, ff, fk in slots:          # the reference, once per span
                    t = alone[c][a:a + n]
                    out = torch.full_like(t, SENT[odt])
                    pw = torch.full((n, Cd) + SIZES[c], -7.0, device="cuda")
                    _tail_alone(L, t, out, pw, delta[fk:fk + (n + step - 1) // step], hm[ff:ff + n] if low else None, u8=u8, att=att, clamp=clamp,
                                aa=aa, Cd=Cd, step=step, mode=mode)
                    ref.append((out, pw))
                for want_pw in (True, False):
                    obuf, outs = _carved(host, fill=SENT[odt])
                    pbuf, pws = _carved(pw_like, fill=-7.0)
                    descs = N.clip_descs([(views[c][a:a + n], ff, fk) for c, a, n, ff, fk in slots], [outs[c][a:a + n] for c, a, n, _, _ in slots],
                                         [pws[c][a:a + n] for c, a, n, _, _ in slots] if want_pw else None)
                    rc = _tail_clips(L, descs, len(slots), delta, hm, u8=u8, att=att, clamp=clamp, aa=aa, Cd=Cd, step=step, mode=mode)
                    torch.cuda.synchronize()
                    what = (step, mode, att, low, clamp, aa, want_pw)
                    assert rc == 0, what
                    assert _only_views_written(obuf, outs, SENT[odt]), what
                    assert _only_views_written(pbuf, pws, -7.0) and (want_pw or bool((pbuf == -7.0).all())), what
                    for (c, a, n, _, _), (ro, rp) in zip(slots, ref):
                        assert torch.equal(outs[c][a:a + n], ro), what + (c, a, SIZES[c])
                        if want_pw:
                            assert torch.equal(pws[c][a:a + n], rp), what + (c, a, SIZES[c], "preds_w")


def test_refusals_launch_nothing():
    """null pointers, n <= 0, F, H or W <= 0, no destination, uint8 without clamp, the training order: an error code, and no output touched --
    the bad descriptor is the LAST of the list, so a launcher that checked as it went would have written the first slots"""
    L = N.lib()
    host = _clips(False)[:3]
    _, views = _carved(host)
    obuf, outs = _carved(host, fill=-7.0)
    nf = sum(t.shape[0] for t in host)
    firsts = [sum(t.shape[0] for t in host[:i]) for i in range(3)]
    delta = torch.zeros(nf, 1, S, S, device="cuda")

    def descs(**bad):
        d = N.clip_descs([(v, ff, ff) for v, ff in zip(views, firsts)], outs)
        for k, v in bad.items():
            setattr(d[2], k, v)
        return d

    brgb, rgb = _guarded_frames(nf)
    for n, bad in ((3, dict(frames=None)), (3, dict(F=0)), (3, dict(H=0)), (3, dict(W=-4)), (0, {}), (-1, {})):
        assert L.vs_resize_pre_clips(descs(**bad), n, 0, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, N.stream()) == -1, (n, bad)
    assert L.vs_resize_pre_clips(descs(), 3, 0, S, S, 1, None, 1.0, 0.0, None, 1, None, N.stream()) == -1          # no destination
    assert L.vs_resize_pre_clips(None, 3, 0, S, S, 1, N.ptr(rgb), 1.0, 0.0, None, 1, None, N.stream()) == -1
    assert L.vs_resize_pre_clips(descs(), 3, 0, S, S, 1, None, 1.0, 0.0, N.ptr(rgb), 0, None, N.stream()) == -1    # key frames every 0 frames

    kw = dict(u8=False, att=1, clamp=1, aa=1, Cd=1, step=1, mode=0)
    for n, bad in ((3, dict(frames=None)), (3, dict(out=None)), (3, dict(F=-1)), (3, dict(H=0)), (3, dict(W=0)), (0, {}), (-2, {})):
        assert _tail_clips(L, descs(**bad), n, delta, None, **kw) == -1, (n, bad)
    assert L.vs_embed_tail_clips(None, N.stream()) == -1
    assert _tail_clips(L, None, 3, delta, None, **kw) == -1 and _tail_clips(L, descs(), 3, None, None, **kw) == -1
    assert _tail_clips(L, descs(), 3, delta, None, **dict(kw, Cd=2)) == -1
    assert _tail_clips(L, descs(), 3, delta, None, **kw, taps43=None) == -1
    assert _tail_clips(L, descs(), 3, delta, None, **dict(kw, step=0)) == -1 and _tail_clips(L, descs(), 3, delta, None, **dict(kw, mode=3)) == -1
    assert _tail_clips(L, descs(), 3, delta, None, **dict(kw, u8=True, clamp=0)) == -1          # (x * 255).byte() needs [0, 1]
    assert _tail_clips(L, descs(), 3, delta, None, **dict(kw, att=2)) == N.ERR_UNSUPPORTED        # the training forward's order: single clips only
    ob, o = torch.full((40,), -7.0, device="cuda"), None
    fr = torch.zeros(3, dtype=torch.int32, device="cuda")
    lg = torch.zeros(4, 17, device="cuda")
    for args in ((None, 17, N.ptr(fr), 2, 16, 0, N.ptr(ob)), (N.ptr(lg), 17, None, 2, 16, 0, N.ptr(ob)), (N.ptr(lg), 17, N.ptr(fr), 2, 16, 0, o),
                 (N.ptr(lg), 17, N.ptr(fr), 0, 16, 0, N.ptr(ob)), (N.ptr(lg), 17, N.ptr(fr), 2, 0, 0, N.ptr(ob)), (N.ptr(lg), 16, N.ptr(fr), 2, 16, 0, N.ptr(ob)),
                 (N.ptr(lg), 17, N.ptr(fr), 2, 16, 4, N.ptr(ob))):
        assert L.vs_aggregate_clips(*args, N.stream()) == -1, args
    torch.cuda.synchronize()
    assert bool((obuf == -7.0).all()) and bool((brgb == -7.0).all()) and bool((ob == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- aggregation
def _agg_case(F_, nbits, seed):
    """(logits [rows, 1+nbits] CPU, lengths): randn rows | one row of magnitude 1e4 among rows of 1e-3 | an all-zero clip | a clip without rows"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(F_, nbits, generator=g)
    b = 1e-3 * torch.randn(F_, nbits, generator=g)
    b[F_ // 2] = 1e4 * torch.randn(nbits, generator=g)
    z = torch.zeros(F_, nbits)
    bits = torch.cat([a, b, z])
    return torch.cat([torch.randn(bits.shape[0], 1, generator=g) * 50.0, bits], dim=1).contiguous(), [F_, F_, F_, 0]


@pytest.mark.parametrize("nbits", [16, 256])
@pytest.mark.parametrize("F_", [1, 2, 129])
def test_aggregate_clips_inside_the_fp64_envelope(F_, nbits):
    """vs_aggregate_clips against aggregate_bits in float64 per clip, the four modes; the yardstick is aggregate_bits in float32 on one CPU
    thread; the error is per clip, relative to the clip's largest aggregated magnitude; the all-zero clip is reproduced exactly and the clip
    without rows gives zeros.  Every line is printed before anything is asserted (profiles/clips_fp64_envelope.txt is a recording)."""
    logits, lens = _agg_case(F_, nbits, seed=100 * F_ + nbits)
    first = CL.first_rows(lens)
    eng_first = torch.tensor(first, dtype=torch.int32, device="cuda")
    dev = logits.cuda()
    names = ("randn", "1e4 in 1e-3", "zeros", "no rows")
    for mode in N.AGGREGATIONS:
        out = torch.full((GUARD + len(lens) * nbits + GUARD,), -7.0, device="cuda")
        N.check(N.lib().vs_aggregate_clips(N.ptr(dev), dev.stride(0), N.ptr(eng_first), len(lens), nbits, N.AGGREGATIONS[mode],
                                           N.ptr(out[GUARD:]), N.stream()), "vs_aggregate_clips")
        torch.cuda.synchronize()
        assert bool((out[:GUARD] == -7.0).all() and (out[-GUARD:] == -7.0).all())
        got = out[GUARD:-GUARD].view(len(lens), nbits).cpu()
        rows = []
        for i, name in enumerate(names):
            bits = logits[first[i]:first[i + 1], 1:]
            if bits.shape[0] == 0:
                ref, yard = torch.zeros(nbits, dtype=torch.float64), torch.zeros(nbits)
            else:
                ref, yard = E.one_thread(lambda: (aggregate_bits(bits.double(), mode), aggregate_bits(bits, mode)))
            rows.append((name, E.group_err(got[i][None], ref[None], 1), E.group_err(yard[None], ref[None], 1)))
            if name in ("zeros", "no rows"):
                assert bool((got[i] == 0).all()), (mode, name)
        agg_envelope(f"F {F_:3d} nbits {nbits:3d} {mode}", rows)


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


def _set(model, step, mode="repeat"):
    model.chunk_size, model.step_size, model.video_mode = CK, step, mode


@functools.lru_cache(maxsize=None)
def _oracle_clean(which):
    """the oracle's logits of the clean clips (CPU; a function of the card alone)"""
    s = tiny_spec() if which == "tiny" else tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16)
    sd = make_state_dict(s, seed=3 if which == "tiny" else 4)
    return tuple(R.detect(sd, s, t)["preds"] for t in _clips(False))


@pytest.mark.parametrize("step", [2, 4])
@pytest.mark.parametrize("lowres", [False, True])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_embed_and_detect_clips_equal_the_composition(which, lowres, step, tiny, tinyc):
    """embed_clips on the list twice over (38 key frames at step 2: two passes) == per pass: per-span eng.resize_pre concatenated, ONE
    eng.embedder_forward with a message row per key frame, one eng.jnd_lowres, per-span eng.embed_tail -- bit for bit, which pins everything
    the clip-list route adds; detect_clips the same way against per-run resize_pre + one extractor_forward per pass"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    mode = ("repeat", "alternate", "interpolate")[(step // 2 + int(lowres)) % 3]
    _set(model, step, mode)
    clips = [t.cuda() for t in _clips(False)]
    clips = clips + clips[::-1]
    n = len(clips)
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    got = model.embed_clips(clips, msgs, lowres_attenuation=lowres)
    got_w = [t.clone() for t in got["imgs_w"]]
    got_p = [p.clone() for p in model.detect_clips(got_w)["preds"]]
    assert torch.equal(got["msgs"], msgs) and all(w.shape == t.shape and w.is_cuda and w.dtype == t.dtype for w, t in zip(got_w, clips))
    eng = model._engine()
    att = model.attenuation is not None
    mi = model._msgs_dev(msgs, eng.dev)
    passes = CL.embed_passes([t.shape[0] for t in clips], step, CK)
    assert len(passes) == (2 if step == 2 else 1)
    for slots, rows in passes:
        keys, rgbs = [], []
        for c, a, f, _, _ in slots:
            rgb, key = eng.resize_pre(clips[c][a:a + f], (S, S), True, want_rgb=(att and lowres), want_key=True, key_step=step)
            keys.append(key.t.clone().view(-1, S, S, 4))
            if rgb is not None:
                rgbs.append(rgb.t.clone().view(-1, S, S, 4))
        key = Act(torch.cat(keys).contiguous(), len(rows), S, S, spec.in_ch, 4)
        delta = eng.embedder_forward(key, mi[torch.tensor(rows, device="cuda")].contiguous(), bn_train=False)
        hmap = eng.jnd_lowres(Act(torch.cat(rgbs).contiguous(), sum(s[2] for s in slots), S, S, 3, 4)) if rgbs else None
        for c, a, f, ff, fk in slots:
            out = torch.empty_like(clips[c][a:a + f])
            eng.embed_tail(clips[c][a:a + f], out, delta[fk:fk + (f + step - 1) // step], step=step, video_mode=N.VIDEO_MODES[mode],
                           hmap_low=(hmap[ff * S * S:(ff + f) * S * S] if hmap is not None else None), attenuate=int(att), clamp=model.clamp,
                           antialias=True, scaling_i=model.blender.scaling_i, scaling_w=model.blender.scaling_w)
            assert torch.equal(out, got_w[c][a:a + f]), (c, a, float((out - got_w[c][a:a + f]).abs().max()))
    (dslots,), first = CL.detect_passes([t.shape[0] for t in clips]), CL.first_rows([t.shape[0] for t in clips])
    rgbs = []
    for c, a, f, _ in dslots:
        rgb, _ = eng.resize_pre(got_w[c][a:a + f], (S, S), True, want_rgb=True, mul=2.0, add=-1.0, tag="det.in")
        rgbs.append(rgb.t.clone().view(-1, S, S, 4))
    preds = eng.extractor_forward(Act(torch.cat(rgbs).contiguous(), first[-1], S, S, 3, 4))
    assert torch.equal(preds, torch.cat(got_p))
    assert all(p.shape == (t.shape[0], spec.nbits + 1) for p, t in zip(got_p, clips))


@pytest.mark.parametrize("mode", ["repeat", "alternate", "interpolate"])
def test_one_clip_in_one_span_equals_embed_and_detect(tiny, mode):
    """a list of one clip that fits one span is the per-clip call with the same batch shape: bit for bit (4 frames, step 2: two key frames, one
    span; the detect side on 2 frames = one chunk of chunk_size frames)"""
    spec, sd, model = tiny
    _set(model, 2, mode)
    x = synthetic_frames(4, 96, 80, seed=21).cuda()
    msgs = synthetic_msgs(1, spec.nbits, seed=21)
    for lowres in (False, True):
        a = model.embed_clips([x], msgs, lowres_attenuation=lowres)["imgs_w"][0]
        b = model.embed(x, msgs, is_video=True, lowres_attenuation=lowres)["imgs_w"]
        assert torch.equal(a, b), (lowres, float((a - b).abs().max()))
    assert torch.equal(model.detect_clips([a[:2]])["preds"][0], model.detect(a[:2], is_video=True)["preds"])
    assert torch.equal(model.detect_clips([a[:2]], interpolation=NA)["preds"][0], model.detect(a[:2], is_video=True, interpolation=NA)["preds"])


@pytest.mark.parametrize("mode", ["repeat", "alternate", "interpolate"])
@pytest.mark.parametrize("lowres", [False, True])
@pytest.mark.parametrize("which", ["tiny", "tinyc"])
def test_clips_against_the_oracle(which, lowres, mode, tiny, tinyc):
    """per clip R.embed_video(clip_i, msgs[i:i+1]) / R.detect of the CPU oracle: the bounds every e2e test uses (tests/_model.py); the 9-frame
    clips are longer than two spans of 4 frames"""
    spec, sd, model = tiny if which == "tiny" else tinyc
    _set(model, 2, mode)
    host = _clips(False)
    n = len(host)
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    got = model.embed_clips([t.cuda() for t in host], msgs, lowres_attenuation=lowres)
    preds = model.detect_clips(got["imgs_w"])["preds"]
    clean = model.detect_clips([t.cuda() for t in host])["preds"]
    cref = _oracle_clean(which)
    for i, t in enumerate(host):
        ref = R.embed_video(sd, spec, t, msgs[i:i + 1], lowres_attenuation=lowres, chunk_size=CK, step_size=2, video_mode=mode)
        err = (got["imgs_w"][i].cpu() - ref["imgs_w"]).abs().max().item()
        assert err < TOL_IMG, (i, SIZES[i], LENS[i], err)
        pref = R.detect(sd, spec, ref["imgs_w"])["preds"]
        assert (preds[i].cpu() - pref).abs().max().item() < TOL_LOGIT, (i, SIZES[i], "watermarked")
        assert (clean[i].cpu() - cref[i]).abs().max().item() < TOL_LOGIT, (i, SIZES[i], "clean")


@pytest.mark.parametrize("lowres", [True, False])
def test_uint8_clips_against_the_clip_entry_points(tiny, lowres):
    """uint8 RGB24 lists against embed_u8 / detect_u8 per clip: codes differ by at most 1 (the criterion of
    test_uint8_images_against_the_clip_entry_points -- network passes of different batch shapes differ in summation order), logits within the e2e bound"""
    spec, sd, model = tiny
    _set(model, 2, "interpolate" if lowres else "repeat")
    clips = [t.cuda() for t in _clips(True)]
    msgs = synthetic_msgs(len(clips), spec.nbits, seed=5)
    got = model.embed_clips(clips, msgs, lowres_attenuation=lowres)
    preds = model.detect_clips(clips)["preds"]
    for i, t in enumerate(clips):
        assert got["imgs_w"][i].dtype == torch.uint8 and got["imgs_w"][i].shape == t.shape
        ref = model.embed_u8(t, msgs[i:i + 1], lowres_attenuation=lowres)["imgs_w"]
        diff = (ref.int() - got["imgs_w"][i].int()).abs()
        assert diff.max().item() <= 1, (i, SIZES[i], int(diff.max()))
        p = model.detect_u8(t)["preds"]
        assert (p - preds[i]).abs().max().item() < TOL_LOGIT, (i, SIZES[i])


@functools.lru_cache(maxsize=None)
def _watermarked_by_the_oracle():
    """(clips watermarked by the CPU oracle, the oracle's logits of them at antialias=False): the input of the extract_messages test.  The
    seeds are chosen so that the oracle's own aggregated logits clear DECISION_MARGIN in every mode (checked on the CPU, see the test)."""
    s = tiny_spec()
    sd = make_state_dict(s, seed=3)
    msgs = synthetic_msgs(len(SIZES), s.nbits, seed=9)
    w = tuple(R.embed_video(sd, s, t, msgs[i:i + 1], chunk_size=CK, step_size=2)["imgs_w"].contiguous() for i, t in enumerate(_clips(False)))
    return w, tuple(R.detect(sd, s, t, NA)["preds"] for t in w)


@pytest.mark.parametrize("aggregation", ["avg", "squared_avg", "l1norm_avg", "l2norm_avg"])
def test_extract_messages_against_extract_message_and_the_oracle(tiny, aggregation):
    """row i of extract_messages against the oracle's aggregated logits of clip i (assert_decisions: DECISION_MARGIN, at most one logit of the
    list inside it) and against extract_message(clip_i) wherever the oracle is sure; an empty clip gives an all-False row"""
    spec, sd, model = tiny
    _set(model, 2)
    w, plog = _watermarked_by_the_oracle()
    gold = torch.stack([R.aggregate(p[:, 1:], aggregation) for p in plog])
    dev = [t.cuda() for t in w]
    got = model.extract_messages(dev + [dev[0][:0]], aggregation)
    assert got.dtype == torch.bool and got.shape == (len(w) + 1, spec.nbits) and not bool(got[-1].any())
    assert_decisions(got[:-1].float() * 2 - 1, gold, what=f"extract_messages {aggregation}", min_sure=0.99)
    one = torch.cat([model.extract_message(t, aggregation) for t in dev]).cpu()
    sure = gold.abs() > DECISION_MARGIN
    assert torch.equal(one[sure], got[:-1].cpu()[sure])
    assert torch.equal(model.extract_messages(list(w), aggregation), got[:-1].cpu())          # CPU clips: same decisions, on the CPU


def test_inputs_devices_and_errors(tiny, tinyc):
    spec, sd, model = tiny
    _set(model, 2, "interpolate")
    host = list(_clips(False))
    dev = [t.cuda() for t in host]
    n = len(dev)
    msgs = synthetic_msgs(n, spec.nbits, seed=9)
    want = model.embed_clips(dev, msgs)
    want_p = model.detect_clips(dev)["preds"]
    # one allocation per call for device-resident clips
    base = want["imgs_w"][0].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for t in want["imgs_w"])
    # host clips round-trip: results on the host, same bits; a clip without frames takes no part and comes back empty
    empty = torch.zeros(0, 3, 20, 24)
    hostr = model.embed_clips(host[:3] + [empty] + host[3:], torch.cat([msgs[:3], msgs[:1], msgs[3:]]))
    res = hostr["imgs_w"][:3] + hostr["imgs_w"][4:]
    assert hostr["imgs_w"][3].shape == empty.shape and all(a.device.type == "cpu" and torch.equal(a, b.cpu()) for a, b in zip(res, want["imgs_w"]))
    hp = model.detect_clips(host[:3] + [empty] + host[3:])["preds"]
    assert tuple(hp[3].shape) == (0, spec.nbits + 1) and all(a.device.type == "cpu" and torch.equal(a, b.cpu()) for a, b in zip(hp[:3] + hp[4:], want_p))
    # a strided view gives the bits of its contiguous copy
    alt = [t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in dev]
    assert not alt[-1].is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(model.embed_clips(alt, msgs)["imgs_w"], want["imgs_w"]))
    # the empty list, random messages
    e = model.embed_clips([], None)
    assert e["imgs_w"] == [] and e["msgs"].shape[0] == 0 and model.detect_clips([])["preds"] == [] and tuple(model.extract_messages([]).shape) == (0, spec.nbits)
    assert model.embed_clips(dev[:2])["msgs"].shape == (2, spec.nbits)
    # loud errors
    u8 = [(t * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in dev[:2]]
    for fn in (lambda c: model.embed_clips(c, msgs[:2]), model.detect_clips, model.extract_messages):
        with pytest.raises(ValueError, match="all fp32"):
            fn([dev[0], u8[1]])
        with pytest.raises(ValueError, match=r"\[F, 3, H, W\]"):
            fn([dev[0], dev[1][0]])                                             # a 3-D tensor
    with pytest.raises(ValueError, match="rows"):
        model.embed_clips(dev, msgs[:3])
    with pytest.raises(ValueError, match="RGB24"):
        model.embed_clips([torch.zeros(2, 20, 20, 4, dtype=torch.uint8, device="cuda")], msgs[:1])
    with pytest.raises(ValueError, match="unknown aggregation"):
        model.extract_messages(dev, "median")
    model.clamp = False
    try:
        with pytest.raises(NotImplementedError, match="clamp=True"):
            model.embed_clips(u8, msgs[:2])
    finally:
        model.clamp = True
    # a pixel-wise detector has no rows of logits to aggregate
    cfg = model.detector.cfg
    import dataclasses
    model.detector.cfg = dataclasses.replace(cfg, head_pixelwise=True)
    try:
        with pytest.raises(NotImplementedError, match="pixel-wise"):
            model.extract_messages(dev)
    finally:
        model.detector.cfg = cfg
