"""SHA-256 of every output buffer of the shell entry points (vs_resize_pre*, vs_embed_tail*) over a fixed case list.

The shell kernels promise bits, not tolerances: a refactor of them is checked by recording the digests with the library of the parent
commit and asking the library under test to reproduce them,

    VIDEOSEAL_LIB=<parent build>/libvideoseal_hip.so python tools/shell_digests.py --write tests/golden/shell_digests.json
    python tools/shell_digests.py --check tests/golden/shell_digests.json          (tests/test_gpu_shell_digests.py does the same)

Every case calls a C-level entry point directly.  Inputs are seeded on the CPU (numpy, one generator per named input); an output buffer is
poisoned first and hashed whole -- pitch padding, spare rows and the bytes around a surface included.  Surfaces (YUV planes, packed RGB) have
odd byte pitches and a base one byte past a 16-byte boundary.  Shapes (F x H x W; S = 64):
  A = 5 x 134 x 202   C = 3 x 134 x 522 (ragged third tile, 8 : 1 resize: long taps)   D = 2 x 18 x 34 (smaller than a tile)
  G = 2 x 131 x 259 (odd H and W, a partial last piece)   H = 1 x 3 x 5; sub-sampled chroma takes the next even size down (G) or up (H).
A call the library refuses is recorded as "refused:<code>", so a changed return code shows as well; the recorded set holds none.
"""
import argparse
import ctypes as C
import functools
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoseal_amd import native as N  # noqa: E402
from videoseal_amd import rgbpack as P  # noqa: E402
from videoseal_amd import yuv as Y  # noqa: E402

S = 64
SHAPES = {"A": (5, 134, 202), "C": (3, 134, 522), "D": (2, 18, 34), "G": (2, 131, 259), "H": (1, 3, 5)}
STREAMS = ("A", "C", "G")                                    # H, W >= 2 S: the row-streaming tail applies
STEP = 2
MODES = (0, 1, 2)                                            # VS_VIDEO_REPEAT, _ALTERNATE, _INTERPOLATE
ATTS = {"off": (0, False), "lowres": (1, True), "full": (1, False), "fwd": (2, False)}      # attenuate, with a low-resolution heat-map
YUV_FMTS = ("nv12", "i420", "p010", "yuv420p10", "nv16", "yuv422p", "p210", "yuv422p10", "yuv444p", "yuv444p10")      # all ten
RGB_FMTS = ("rgb24", "bgra", "rgb48", "rgba64", "x2rgb10")   # one format of each of the five layouts
YMAT = (C.c_float * 3)(0.299, 0.587, 0.114)
TAPS43 = (C.c_float * 43)(*([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1]       # jnd.py:24-41
                            + [-1, 0, 1, -2, 0, 2, -1, 0, 1] + [1, 2, 1, 0, 0, 0, -1, -2, -1]))
OFF = 33                                                     # bytes before a surface: one past a 16-byte boundary


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(key, *shape):
    return _dev(_rng(*key).random(shape, dtype=np.float32))


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _ceil(a, b):
    return (a + b - 1) // b


@functools.lru_cache(maxsize=None)
def _watermark(key, nk, Cd, frames):
    """(delta [nk, Cd, S, S] in (-1, 1), low-resolution heat-map [frames * S * S] in [0, 1)); made once, read only"""
    return _dev(np.tanh(_rng(key, "delta").standard_normal((nk, Cd, S, S)).astype(np.float32))), _rand((key, "hm"), frames * S * S)


class Plane:
    """[F, R, rowb] bytes as a strided view of a poisoned device buffer: odd pitch, two spare rows per frame, base one byte off alignment"""

    def __init__(self, F_, R_, rowb, pad, data=None, poison=0x5A):
        pitch = rowb + pad
        pitch += 1 - pitch % 2
        n = F_ * (R_ + 2) * pitch
        self.buf = torch.full((OFF + n + 32,), poison, dtype=torch.uint8, device="cuda")
        self.view = self.buf[OFF:OFF + n].view(F_, R_ + 2, pitch)[:, :R_, :rowb]
        assert self.view.data_ptr() % 16 == 1
        if data is not None:
            self.view.copy_(_dev(np.ascontiguousarray(data).view(np.uint8).reshape(F_, R_, rowb)))
        self.ptr, self.pitch, self.fs, self.poison = self.view.data_ptr(), pitch, (R_ + 2) * pitch, poison

    def reset(self):
        self.buf.fill_(self.poison)


def _tail_fields(d, F_, H, W, delta, hm, att, Cd, mode, variant, clamp=1):
    attenuate, low = ATTS[att]
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm) if low else None
    d.taps43 = C.cast(TAPS43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, Cd
    d.step, d.video_mode, d.total_key = STEP, mode, _ceil(F_, STEP)
    d.attenuate, d.clamp, d.antialias = attenuate, clamp, 1
    d.scaling_i, d.scaling_w = 1.0, 0.2
    d.variant = variant


# ---------------------------------------------------------------------------------------------------- fp32 NCHW and uint8 RGB24
@functools.lru_cache(maxsize=None)
def _frames(sh, u8):
    F_, H, W = SHAPES[sh]
    if u8:
        return _dev(_rng(sh, "u8").integers(0, 256, size=(F_, H, W, 3), dtype=np.uint8))
    return _rand((sh, "f32"), F_, 3, H, W)


def resize_plain(sh, u8, aa, what, tile):
    """what: "both" (rgb + luma key through ymat), "rgb", "key" (rgb key frames, no ymat)"""
    F_, H, W = SHAPES[sh]
    src = _frames(sh, u8)
    rgb = _nan(F_, S, S, 4) if what != "key" else None
    key = _nan(_ceil(F_, STEP), S, S, 4) if what != "rgb" else None
    ymat = YMAT if what == "both" else None
    L = N.lib()
    with N.debug("RESIZE_FORM", 1 if tile else 0):
        if u8:
            N.check(L.vs_resize_pre_u8(N.ptr(src), F_, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), STEP, ymat, None), "vs_resize_pre_u8")
        else:
            N.check(L.vs_resize_pre(N.ptr(src), F_, 3, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), STEP, ymat, None), "vs_resize_pre")
    return [rgb, key]


def tail_plain(sh, u8, att, Cd, mode, variant, entry="plain", preds=False, clamp=1):
    """entry: plain (vs_embed_tail), scaled, energy, regions"""
    F_, H, W = SHAPES[sh]
    R_ = 3 if entry == "regions" else 1
    src = _frames(sh, u8)
    delta, hm = _watermark((sh, Cd, R_), _ceil(F_, STEP) * R_, Cd, F_)
    out = torch.full(src.shape, 0x5A, dtype=torch.uint8, device="cuda") if u8 else _nan(*src.shape)
    pw = _nan(F_, Cd, H, W) if preds else None
    d = N.TailDesc()
    _tail_fields(d, F_, H, W, delta, hm, att, Cd, mode, variant, clamp)
    d.imgs, d.out, d.preds_w, d.io_u8 = N.ptr(src), N.ptr(out), N.ptr(pw), int(u8)
    L = N.lib()
    if entry == "plain":
        N.check(L.vs_embed_tail(C.byref(d), None), "vs_embed_tail")
    elif entry == "scaled":
        scale = _rand((sh, "scale"), F_)
        N.check(L.vs_embed_tail_scaled(C.byref(d), N.ptr(scale), None), "vs_embed_tail_scaled")
    elif entry == "energy":
        d.out = None
        part = torch.full((int(L.vs_tail_energy_partial_doubles(F_, H, W)),), -1.0, dtype=torch.float64, device="cuda")
        energy = _nan(F_, dtype=torch.float64)
        N.check(L.vs_embed_tail_energy(C.byref(d), N.ptr(part), N.ptr(energy), None), "vs_embed_tail_energy")
        return [part, energy]
    else:
        labels = _dev(_rng(sh, "labels").integers(0, R_ + 2, size=(F_, H, W), dtype=np.uint8))       # (R + 1: out of range, background)
        N.check(L.vs_embed_tail_regions(C.byref(d), N.ptr(labels), R_, None), "vs_embed_tail_regions")
    return [out, pw]


LISTS = {"images": ("A", "D", "G", "H", "C"), "clips": ("A", "D", "G")}


def _list_frames(kind, u8):
    """images: frame 0 of each shape; clips: every frame"""
    ts = [_frames(sh, u8) for sh in LISTS[kind]]
    return [t[0].contiguous() for t in ts] if kind == "images" else ts


def resize_list(kind, u8, aa, what):
    ts = _list_frames(kind, u8)
    ymat = YMAT if what == "both" else None
    L = N.lib()
    if kind == "images":
        n = len(ts)
        rgb, key = (_nan(n, S, S, 4) if what != "key" else None), (_nan(n, S, S, 4) if what != "rgb" else None)
        N.check(L.vs_resize_pre_images(N.image_descs(ts), n, int(u8), S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), ymat, None), "vs_resize_pre_images")
        return [rgb, key]
    slots, ff, fk = [], 0, 0
    for t in ts:
        slots.append((t, ff, fk))
        ff, fk = ff + t.shape[0], fk + _ceil(t.shape[0], STEP)
    rgb, key = (_nan(ff, S, S, 4) if what != "key" else None), (_nan(fk, S, S, 4) if what != "rgb" else None)
    N.check(L.vs_resize_pre_clips(N.clip_descs(slots), len(slots), int(u8), S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), STEP, ymat, None),
            "vs_resize_pre_clips")
    return [rgb, key]


def tail_list(kind, u8, att, Cd, mode, preds):
    ts = _list_frames(kind, u8)
    outs = [torch.full(t.shape, 0x5A, dtype=torch.uint8, device="cuda") if u8 else _nan(*t.shape) for t in ts]
    attenuate, low = ATTS[att]
    L = N.lib()
    if kind == "images":
        n = len(ts)
        delta, hm = _watermark((kind, Cd), n, Cd, n)
        pws = [_nan(Cd, *(t.shape[:2] if u8 else t.shape[1:])) for t in ts] if preds else None
        d = N.TailImagesDesc()
        descs = N.image_descs(ts, outs, pws)
        d.images, d.n = descs, n
    else:
        slots, ff, fk = [], 0, 0
        for t in ts:
            slots.append((t, ff, fk))
            ff, fk = ff + t.shape[0], fk + _ceil(t.shape[0], STEP)
        delta, hm = _watermark((kind, Cd), fk, Cd, ff)
        pws = [_nan(t.shape[0], Cd, *(t.shape[1:3] if u8 else t.shape[2:])) for t in ts] if preds else None
        d = N.TailClipsDesc()
        descs = N.clip_descs(slots, outs, pws)
        d.clips, d.n = descs, len(slots)
        d.step, d.video_mode = STEP, mode
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm) if low else None
    d.taps43 = C.cast(TAPS43, C.c_void_p)
    d.S_h, d.S_w, d.Cd = S, S, Cd
    d.attenuate, d.clamp, d.antialias, d.io_u8 = attenuate, 1, 1, int(u8)
    d.scaling_i, d.scaling_w = 1.0, 0.2
    N.check((L.vs_embed_tail_images if kind == "images" else L.vs_embed_tail_clips)(C.byref(d), None), f"vs_embed_tail_{kind}")
    return outs + (pws or [])


# ---------------------------------------------------------------------------------------------------- surfaces
def surf_shape(sh, sx, sy):
    """the shape a surface with chroma shifts (sx, sy) can have: G rounds down, H up"""
    F_, H, W = SHAPES[sh]
    r = (lambda v, s: v) if sh not in ("G", "H") else (lambda v, s: (v >> s << s) if sh == "G" else ((v + (1 << s) - 1) >> s << s))
    return F_, r(H, sy), r(W, sx)


_cache = {}


def yuv_clip(fmt, sh, data=True):
    """(planes, F, H, W): random words (most triples out of gamut, low bits of msb-aligned words set, 10-bit words past 1023)"""
    planar, depth, msb, chroma = Y.fmt_info(fmt)
    F_, H, W = surf_shape(sh, *Y.SHIFTS[chroma])
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    planes = []
    for i, (f, r, w) in enumerate(Y.plane_shapes(fmt, F_, H, W)):
        words = _rng(fmt, sh, i).integers(0, top, size=(f, r, w)).astype(dt) if data else None
        planes.append(Plane(f, r, w * np.dtype(dt).itemsize, (54, 7, 12)[i], words, 0xA5 if data else 0x5A))
    return planes, F_, H, W


def yuv_surface(fmt, planes):
    planar, depth, msb, chroma = Y.fmt_info(fmt)
    s = N.YuvSurface()
    for i, p in enumerate(planes):
        s.plane[i], s.pitch[i], s.frame_stride[i] = p.ptr, p.pitch, p.fs
    s.planar, s.depth, s.msb_aligned, s.chroma = int(planar), depth, int(msb), chroma
    return s


def yuv_affines(fmt):
    fwd, inv = Y.color_affine("bt709", False, Y.fmt_info(fmt)[1])
    return (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)]), (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])


def _cached(kind, fmt, sh):
    """source (and re-poisoned destination) surfaces of a format and shape, made once"""
    k = (kind, fmt, sh)
    if k not in _cache:
        make = yuv_clip if kind == "yuv" else rgb_clip
        _cache.clear()                                         # cases come grouped by (format, shape): one pair alive at a time
        _cache[k] = (make(fmt, sh), make(fmt, sh, data=False))
    return _cache[k]


def resize_yuv(fmt, sh, aa, tile):
    (planes, F_, H, W), _ = _cached("yuv", fmt, sh)
    surf = yuv_surface(fmt, planes)
    rgb, key = _nan(F_, S, S, 4), _nan(_ceil(F_, STEP), S, S, 4)
    with N.debug("RESIZE_FORM", 1 if tile else 0):
        N.check(N.lib().vs_resize_pre_yuv(C.byref(surf), F_, H, W, yuv_affines(fmt)[0], S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), STEP, YMAT, None),
                "vs_resize_pre_yuv")
    return [rgb, key]


def tail_yuv(fmt, sh, att, Cd, mode, variant):
    (planes, F_, H, W), (outs, _, _, _) = _cached("yuv", fmt, sh)
    for p in outs:
        p.reset()
    delta, hm = _watermark((sh, Cd, 1), _ceil(F_, STEP), Cd, F_)
    d = N.TailYuvDesc()
    d.src, d.dst = yuv_surface(fmt, planes), yuv_surface(fmt, outs)
    _tail_fields(d, F_, H, W, delta, hm, att, Cd, mode, variant)
    d.yuv2rgb12, d.rgb2yuv12 = yuv_affines(fmt)
    N.check(N.lib().vs_embed_tail_yuv(C.byref(d), None), "vs_embed_tail_yuv")
    return [p.buf for p in outs]


def rgb_clip(fmt, sh, data=True):
    F_, H, W = SHAPES[sh]
    _, depth, comps, _, _ = P.fmt_info(fmt)
    words = None
    if data and comps == 0:
        words = _rng(fmt, sh).integers(0, 1 << 32, size=(F_, H, W), dtype=np.uint64).astype(np.uint32)
    elif data:
        words = _rng(fmt, sh).integers(0, 1 << depth, size=(F_, H, W, comps)).astype(np.uint8 if depth == 8 else np.uint16)
    return Plane(F_, H, W * P.pixel_bytes(fmt), 54, words, 0xA5 if data else 0x5A), F_, H, W


def rgb_surface(fmt, p):
    s = N.RgbSurface()
    s.data, s.pitch, s.frame_stride, s.format = p.ptr, p.pitch, p.fs, P.fmt_info(fmt)[0]
    return s


def resize_rgb(fmt, sh, aa, tile):
    (p, F_, H, W), _ = _cached("rgb", fmt, sh)
    surf = rgb_surface(fmt, p)
    rgb, key = _nan(F_, S, S, 4), _nan(_ceil(F_, STEP), S, S, 4)
    with N.debug("RESIZE_FORM", 1 if tile else 0):
        N.check(N.lib().vs_resize_pre_rgb(C.byref(surf), F_, H, W, S, S, aa, N.ptr(rgb), 2.0, -1.0, N.ptr(key), STEP, YMAT, None), "vs_resize_pre_rgb")
    return [rgb, key]


def tail_rgb(fmt, sh, att, Cd, mode, variant):
    (p, F_, H, W), (out, _, _, _) = _cached("rgb", fmt, sh)
    out.reset()
    delta, hm = _watermark((sh, Cd, 1), _ceil(F_, STEP), Cd, F_)
    d = N.TailRgbDesc()
    d.src, d.dst = rgb_surface(fmt, p), rgb_surface(fmt, out)
    _tail_fields(d, F_, H, W, delta, hm, att, Cd, mode, variant)
    N.check(N.lib().vs_embed_tail_rgb(C.byref(d), None), "vs_embed_tail_rgb")
    return [out.buf]


# ---------------------------------------------------------------------------------------------------- the case list
def cases():
    """[(name, thunk)]: fixed, in a fixed order"""
    out = []

    def add(fn, *args, **kw):
        name = fn.__name__ + "(" + ",".join([str(a) for a in args] + [f"{k}={v}" for k, v in kw.items()]) + ")"
        out.append((name, lambda: fn(*args, **kw)))

    for sh in SHAPES:
        for aa in (1, 0):
            for what in ("both", "rgb", "key"):
                add(resize_plain, sh, False, aa, what, False)
            add(resize_plain, sh, False, aa, "both", True)
            add(resize_plain, sh, True, aa, "both", False)
            add(resize_plain, sh, True, aa, "key", False)
        for att in ("off", "lowres", "full"):
            for Cd in (1, 3):
                for mode in MODES:
                    for variant in (1,) + ((2, 3) if att == "full" else ()) + ((4,) if sh in STREAMS else ()):
                        add(tail_plain, sh, False, att, Cd, mode, variant)
                    add(tail_plain, sh, True, att, Cd, mode, 0)
                for variant in (1, 4) if sh in STREAMS else (1,):
                    add(tail_plain, sh, False, att, Cd, 2, variant, preds=True)
                    add(tail_plain, sh, False, att, Cd, 2, variant, clamp=0)
                    for entry in ("scaled", "energy"):
                        add(tail_plain, sh, False, att, Cd, 2, variant, entry=entry)
                add(tail_plain, sh, True, att, Cd, 2, 0, entry="scaled")
                add(tail_plain, sh, True, att, Cd, 2, 0, entry="energy")
                for u8, variant in ((False, 1), (False, 0), (True, 0)):
                    add(tail_plain, sh, u8, att, Cd, 2, variant, entry="regions", preds=not u8)
        for Cd in (1, 3):
            for variant in (1, 2, 3) + ((4,) if sh in STREAMS else ()):
                add(tail_plain, sh, False, "fwd", Cd, 2, variant, preds=True)
    for kind in LISTS:
        for u8 in (False, True):
            for aa in (1, 0):
                for what in ("both", "key"):
                    add(resize_list, kind, u8, aa, what)
            for att in ("off", "lowres", "full"):
                for Cd in (1, 3):
                    for mode in MODES if kind == "clips" else (0,):
                        add(tail_list, kind, u8, att, Cd, mode, False)
                    add(tail_list, kind, u8, att, Cd, 2 if kind == "clips" else 0, True)
    # surfaces: both resize forms; both tail forms x attenuation, with Cd = 1 interpolated and Cd = 3 in a mode that differs per attenuation
    for kind, fmts, resize, tail in (("yuv", YUV_FMTS, resize_yuv, tail_yuv), ("rgb", RGB_FMTS, resize_rgb, tail_rgb)):
        for fmt in fmts:
            for sh in SHAPES:
                for aa in (1, 0):
                    for tile in (False, True):
                        add(resize, fmt, sh, aa, tile)
                for i, att in enumerate(("off", "lowres", "full")):
                    for variant in (1, 4) if sh in STREAMS else (1,):
                        add(tail, fmt, sh, att, 1, 2, variant)
                        add(tail, fmt, sh, att, 3, i, variant)
    return out


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def digests():
    """{case name: SHA-256 of its output buffers}"""
    res = {}
    for name, thunk in cases():
        try:
            res[name] = digest(thunk())
        except N.NativeError as e:
            res[name] = "refused:" + str(e).rsplit("code", 1)[-1].strip(" )")
    _cache.clear()
    return res


def compare(got, want):
    """names whose digests differ, or that one side lacks"""
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="JSON", help="record the digests")
    ap.add_argument("--check", metavar="JSON", help="compare with a record; exit status 1 if any case differs")
    ap.add_argument("--list", action="store_true", help="print the case names (no GPU needed)")
    a = ap.parse_args()
    if a.list:
        print("\n".join(n for n, _ in cases()))
        return 0
    got = digests()
    refused = [k for k, v in got.items() if v.startswith("refused")]
    print(f"{len(got)} cases with {N.LIB_PATH}, {len(refused)} refused", file=sys.stderr)
    if a.write:
        with open(a.write, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
    if a.check:
        with open(a.check) as f:
            bad = compare(got, json.load(f))
        for k in bad:
            print("differs:", k)
        print(f"{len(got) - len(bad)} of {len(got)} cases match {a.check}")
        return 1 if bad else 0
    if not a.write:
        for k, v in got.items():
            print(v, k)
    return 0


if __name__ == "__main__":
    sys.exit(main())
