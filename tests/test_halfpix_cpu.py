"""videoseal_amd.halfpix (the torch definition of half-precision clips) against tests/_halfpix_ref.py (numpy, float64 + explicit roundings),
its round-trip statement by enumeration, check_clip's acceptances and refusals, and the entry points of include/videoseal_half.h.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _halfpix_ref as R  # noqa: E402

from videoseal_amd import halfpix  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def _clip(words, typ):
    """uint16 words [n] -> an nchw clip [1, 3, 1, n] holding them in every plane"""
    t = torch.from_numpy(np.ascontiguousarray(words).view(np.int16)).view(DT[typ])
    return t.reshape(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()


def _words(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("rng", R.RANGES)
@pytest.mark.parametrize("typ", R.TYPES)
def test_decode_of_every_finite_word(typ, rng):
    w = R.all_words()
    w = w[R.finite(w, typ)]
    got = halfpix.to_rgb(_clip(w, typ), "nchw", rng)
    assert got.dtype == torch.float32 and got.shape == (1, 3, 1, w.size)
    want = R.decode(w, typ, rng)
    for c in range(3):
        assert np.array_equal(got[0, c, 0].numpy().view(np.uint32), want.view(np.uint32)), (typ, rng)


def _encode_grid(typ, rng):
    """fp32 inputs: every exact tie between neighbouring representable stored values of the range (built from the words), values whose
    result is an fp16 subnormal, the clamp bounds, values just outside them, both zeros"""
    w = R.all_words()
    w = w[R.finite(w, typ)]
    y = np.unique(R.words_to_f64(w, typ))
    lo = -1.0 if rng == "signed" else 0.0
    y = y[(y >= lo) & (y <= 1.0)]
    mid = (y[:-1] + y[1:]) / 2                                # exact in float64; a tie of the stored value
    v = (mid + 1.0) / 2 if rng == "signed" else mid           # the component that maps onto it
    v32 = v.astype(np.float32)
    exact = (v32.astype(np.float64) * 2 - 1 == mid) if rng == "signed" else (v32.astype(np.float64) == mid)      # fp32 holds the component exactly
    ties = v32[exact]
    assert ties.size > 3000
    one, zero = np.float32(1.0), np.float32(0.0)
    sub = np.float32(2.0 ** -14) * np.linspace(0.0, 1.0, 4097, dtype=np.float64).astype(np.float32)        # results in (0, 2^-14)
    if rng == "signed":
        sub = np.float32(0.5) + sub / 2
    edges = np.array([zero, -zero, one, np.nextafter(zero, -one), np.nextafter(one, np.float32(2)), np.nextafter(one, zero), -0.25, 1.25,
                      np.nextafter(zero, one), 0.5, np.nextafter(np.float32(0.5), zero), np.nextafter(np.float32(0.5), one)], dtype=np.float32)
    rnd = np.random.default_rng(3).uniform(-0.3, 1.3, 20000).astype(np.float32)
    return np.concatenate([ties, np.nextafter(ties, one), np.nextafter(ties, -one), sub, edges, rnd]), ties.size


@pytest.mark.parametrize("rng", R.RANGES)
@pytest.mark.parametrize("typ", R.TYPES)
def test_encode_on_ties_subnormals_and_bounds(typ, rng):
    v, nties = _encode_grid(typ, rng)
    x = torch.from_numpy(v).reshape(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()
    for layout in halfpix.LAYOUTS:
        got = halfpix.from_rgb(x, layout=layout, value_range=rng, dtype=DT[typ])
        assert got.dtype == DT[typ] and got.is_contiguous()
        px = got if layout == "nhwc" else got.permute(0, 2, 3, 1)
        want = R.encode(v, typ, rng)
        for c in range(3):
            assert np.array_equal(_words(px[0, 0, :, c]), want), (typ, rng, layout)
    # the ties really are ties: not representable, and the result is half a step away
    t = v[:nties].astype(np.float64)
    stored = t * 2 - 1 if rng == "signed" else t
    out = R.words_to_f64(R.encode(v[:nties], typ, rng), typ)
    assert np.all(out != stored) and np.all(np.abs(out - stored) <= R.ulp(stored, typ) / 2)
    assert np.all((R.encode(v[:nties], typ, rng) & 1) == 0)   # ... and went to the even word
    if typ == "f16" and rng == "unit":
        sub = np.float32(2.0 ** -15)
        assert R.encode(np.array([sub]), typ, rng)[0] == 0x0200 and R.encode(np.array([np.float32(2.0 ** -24)]), typ, rng)[0] == 1


@pytest.mark.parametrize("rng", R.RANGES)
@pytest.mark.parametrize("typ", R.TYPES)
def test_round_trip_set_is_what_the_docstring_states(typ, rng):
    w = R.all_words()
    fin = R.finite(w, typ)
    ws = np.where(fin, w, 0).astype(np.uint16)
    clip = _clip(ws, typ)
    back = _words(halfpix.from_rgb(halfpix.to_rgb(clip, "nchw", rng), like=clip, layout="nchw", value_range=rng)[0, 1, 0])
    same = (back == w) & fin
    assert int(same.sum()) == halfpix.ROUND_TRIP[(DT[typ], rng)]
    assert np.array_equal(back, R.encode(R.decode(ws, typ, rng), typ, rng))
    y = R.words_to_f64(ws, typ)
    neg0 = w == 0x8000
    if rng == "unit":                                         # every finite word in [0, 1] but -0.0, and no other
        assert np.array_equal(same, fin & (y >= 0) & (y <= 1) & ~neg0)
        assert {"f16": "15 361", "bf16": "16 257"}[typ] in halfpix.__doc__
    else:                                                     # the words of [-1, 1] whose y * 0.5 + 0.5 is exact in fp32
        s_ = y * 0.5 + 0.5                                      # (float64 does not hold the sum for the tiniest bf16 words: only its binade is used)
        spacing = np.exp2(np.floor(np.log2(np.where(s_ > 0, s_, 1.0))) - 23)
        exact = (y * 0.5 / spacing) == np.rint(y * 0.5 / spacing)
        assert np.array_equal(same, fin & (np.abs(y) <= 1) & exact & ~neg0)
        lost = np.abs(y[fin & (np.abs(y) <= 1) & ~same])
        assert lost.max() <= (2.0 ** -13 if typ == "f16" else 2.0 ** -16)
        assert {"f16": "29 697", "bf16": "4 481"}[typ] in halfpix.__doc__


def test_check_clip_acceptances_and_refusals():
    F_, H, W = 3, 6, 10
    for dt in DT.values():
        x = torch.zeros(F_, 3, H, W, dtype=dt)
        assert halfpix.check_clip(x) == (F_, H, W) and halfpix.memory_form(x, "nchw") == (halfpix.PLANAR, 3)
        cl = x.contiguous(memory_format=torch.channels_last)
        assert cl.stride() == (3 * H * W, 1, 3 * W, 3)
        assert halfpix.check_clip(cl) == (F_, H, W) and halfpix.memory_form(cl, "nchw") == (halfpix.PACKED, 3)
        big = torch.zeros(F_, 3, H + 2, W + 5, dtype=dt)
        v = big[:, :, :H, :W]                                  # a pitched planar view stays a view
        assert halfpix.check_clip(v) == (F_, H, W) and halfpix.memory_form(v, "nchw") == (halfpix.PLANAR, 3)
        pm = torch.zeros(3, F_, H, W, dtype=dt).permute(1, 0, 2, 3)        # plane-major storage: frames below the plane stride
        assert halfpix.check_clip(pm) == (F_, H, W)
        for C_ in (3, 4):
            p = torch.zeros(F_, H + 1, W + 3, C_, dtype=dt)[:, :H, :W]
            assert halfpix.check_clip(p, "nhwc") == (F_, H, W) and halfpix.memory_form(p, "nhwc") == (halfpix.PACKED, C_)
        clv = torch.zeros(F_, H + 1, W + 3, 3, dtype=dt)[:, :H, :W].permute(0, 3, 1, 2)     # pitched channels-last
        assert halfpix.check_clip(clv) == (F_, H, W) and halfpix.memory_form(clv, "nchw") == (halfpix.PACKED, 3)
        assert halfpix.check_clip(x[:0]) == (0, H, W)
        o = halfpix.empty_like(cl)
        assert o.shape == cl.shape and o.stride() == cl.stride() and o.dtype == dt
        assert halfpix.empty_like(v).is_contiguous()
        bad = [
            (x[0:1].expand(F_, 3, H, W), "nchw"),              # overlapping frames
            (x[:, 0:1].expand(F_, 3, H, W), "nchw"),           # overlapping planes
            (x[:, :, 0:1].expand(F_, 3, H, W), "nchw"),        # overlapping rows
            (x[:, :, :, ::2], "nchw"),                         # neither planar nor channels-last
            (torch.zeros(F_, 4, H, W, dtype=dt), "nchw"),      # four planes
            (torch.zeros(F_, H, W, 2, dtype=dt), "nhwc"),
            (torch.zeros(F_, H, W, 4, dtype=dt)[..., :3], "nhwc"),         # pixel stride 4 with 3 components
            (torch.zeros(F_, H, W, 3, dtype=dt)[:, 0:1].expand(F_, H, W, 3), "nhwc"),
            (torch.zeros(1, H, W, 3, dtype=dt).expand(F_, H, W, 3), "nhwc"),
            (x[0], "nchw"),
            (x, "nchw4"),
            ((x,), "nchw"),
        ]
        for t, layout in bad:
            with pytest.raises(ValueError):
                halfpix.check_clip(t, layout)
    with pytest.raises(ValueError, match="value_range"):
        halfpix.check_clip(torch.zeros(1, 3, 2, 2, dtype=torch.float16), "nchw", "full")
    for t in (torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2, dtype=torch.uint8), torch.zeros(1, 3, 2, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="float16 or bfloat16"):
            halfpix.check_clip(t)


def test_alpha_words_and_memory_form_follow_like():
    g = torch.Generator().manual_seed(2)
    a = torch.randint(-32768, 32768, (2, 5, 7, 4), generator=g, dtype=torch.int32).to(torch.int16)
    a[0, 0, 0, 3], a[0, 0, 1, 3], a[0, 0, 2, 3] = 0x7E01, 0x7C00, -1       # a NaN with a payload, +Inf, another NaN
    for dt in DT.values():
        like = a.view(dt)
        x = torch.rand(2, 3, 5, 7, generator=g)
        out = halfpix.from_rgb(x, like=like, layout="nhwc")
        assert torch.equal(out.view(torch.int16)[..., 3], a[..., 3])
        assert torch.equal(out[..., :3], x.permute(0, 2, 3, 1).to(dt))
        assert torch.equal(halfpix.from_rgb(x, layout="nhwc", dtype=dt)[..., :3], out[..., :3])
        cl = torch.zeros(2, 3, 5, 7, dtype=dt).contiguous(memory_format=torch.channels_last)
        o = halfpix.from_rgb(x, like=cl)
        assert o.stride() == cl.stride() and torch.equal(o, x.to(dt))
        c = halfpix.Clip(cl, "nchw", "signed")
        assert c.shape == (2, 5, 7) and c[0:1].shape == (1, 5, 7) and c.empty_like().tensor.stride() == cl.stride()
        assert c.fmt.endswith("signed.packed3") and halfpix.Clip(like, "nhwc").fmt.endswith("unit.packed4")


# ---------------------------------------------------------------------------------------------------------------- the header
def _declared(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.findall(r"(?m)^\s*(?:const\s+)?[A-Za-z_]\w*(?:\s*\*)?\s+\*?(vs_\w+)\s*\(", text)


def test_every_declaration_of_the_half_header_is_exported_bound_and_tested():
    decl = _declared("videoseal_half.h")
    assert sorted(decl) == sorted(N.HALF_EXPORTS) and len(set(decl)) == len(decl) == 6
    main = set(_declared("videoseal_hip.h"))
    assert len(main) > 150 and not main & set(decl) and not set(N.EXPORTS) & set(decl)
    assert not re.search(r"vs_\w*half", open(os.path.join(ROOT, "include", "videoseal_hip.h")).read())
    header = open(os.path.join(ROOT, "include", "videoseal_half.h")).read()
    for name, value in (("VS_HALF_FP16", 0), ("VS_HALF_BF16", 1), ("VS_HALF_PLANAR", 0), ("VS_HALF_PACKED", 1), ("VS_HALF_UNIT", 0), ("VS_HALF_SIGNED", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header)
    assert halfpix.DTYPES == {torch.float16: 0, torch.bfloat16: 1} and halfpix.RANGES == {"unit": 0, "signed": 1}
    assert (halfpix.PLANAR, halfpix.PACKED) == (0, 1)
    lib = N.lib()
    from videoseal_amd import capi
    capi._bind(lib)                                           # (the model-level signatures live with the other vs_model_* ones)
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_halfpix.py")).read()
    for sym in decl:
        assert hasattr(lib, sym), f"{sym} is declared but not exported"
        assert sym.startswith("vs_sizeof") or getattr(lib, sym).argtypes, f"{sym} has no ctypes signature in native.py"
        assert sym.startswith("vs_sizeof") or re.search(r"\b" + sym + r"\b", gpu_test), f"{sym} is not named in tests/test_gpu_halfpix.py"
    import ctypes as C
    assert lib.vs_sizeof_half_surface() == C.sizeof(N.HalfSurface) and lib.vs_sizeof_tail_half_desc() == C.sizeof(N.TailHalfDesc)
    assert "HALF_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    # argument checks happen on the host before any launch: refused without a GPU
    s, d = N.HalfSurface(), N.TailHalfDesc()
    assert lib.vs_resize_pre_half(None, 1, 1, 1, 1, 1, 0, None, 1.0, 0.0, None, 1, None, None) == -1
    assert lib.vs_resize_pre_half(C.byref(s), 1, 0, 1, 1, 1, 0, None, 1.0, 0.0, None, 1, None, None) == -1
    assert lib.vs_embed_tail_half(None, None) == -1 and lib.vs_embed_tail_half(C.byref(d), None) == -1
    assert lib.vs_model_embed_half(None, C.byref(s), C.byref(s), None, 1, 1, 1, 1, 1, 0, 0, 1, None, 0, None) == -1
    assert lib.vs_model_detect_half(None, C.byref(s), 1, 1, 1, 1, None, None, 0, None) == -1
