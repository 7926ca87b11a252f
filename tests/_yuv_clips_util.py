"""Helpers of the YUV clip-list tests (tests/test_yuv_clips_cpu.py, tests/test_gpu_yuv_clips.py): the slot shapes, the launch plan restated
in Python, pitched clips between guard bands and the descriptors of the two C entry points.  Nothing here touches a GPU at import."""
import ctypes as C

import numpy as np
import torch

from tests import _yuv_ref as R
from tests._guards import GUARD
from videoseal_amd import native as N
from videoseal_amd import yuv

PER = N.YUV_CLIPS_PER_LAUNCH
S = 64                                                                          # img_size of the tiny models
f32 = np.float32
FORMATS = ("nv12", "i420", "p010", "yuv420p10", "yuv422p", "yuv422p10", "nv16", "p210", "yuv444p", "yuv444p10")
# the slot shapes of tests/test_gpu_yuv.py: (H, W, spare rows per frame, bytes after a row's end per plane)
SIZES = {"A": (134, 202, 7, (54, 7, 12)), "B": (72, 88, 0, (0, 3, 8)), "C": (134, 522, 3, (1, 5, 2)), "D": (18, 34, 1, (13, 1, 6)),
         "E": (67, 202, 5, (9, 5, 3)), "G": (131, 259, 2, (11, 2, 7))}
LENGTHS = (1, 3, 5, 9)
YMAT = [float(f32(v)) for v in (0.299, 0.587, 0.114)]


def sizes_of(fmt, names="DBACEG"):
    """the shapes of `names` that `fmt` can have"""
    _, _, _, sx, sy = R.FORMATS[fmt]
    return [n for n in names if SIZES[n][0] % (1 << sy) == 0 and SIZES[n][1] % (1 << sx) == 0]


def chroma_of(fmt):
    return {(1, 1): 420, (1, 0): 422, (0, 0): 444}[R.FORMATS[fmt][3:5]]


def depth_of(fmt):
    return R.FORMATS[fmt][1]


# ---- the plan, restated (resize_pick.h::rs_pick in float32 with the format's margin, images_plan.h, yuv_clips_plan.h)
def align_of(fmt):
    planar, depth, _, sx, _ = R.FORMATS[fmt]
    return 32 if (planar and sx == 1 and depth == 8) else 16


def rs_pick(H, W, oh, ow, aa, margin):
    sx, sy = f32(W) / f32(ow), f32(H) / f32(oh)
    supx = max(sx, f32(1)) if aa else f32(1)
    supy = max(sy, f32(1)) if aa else f32(1)
    for OW, INW, MT, RING in ((128, 448, 8, 16), (64, 288, 10, 32)):
        if f32(2) * supx + f32(2) <= f32(MT) and f32(2) * supy + f32(2) <= f32(MT) and \
                f32(OW) * sx + f32(2) * supx + f32(4) + f32(margin) <= f32(INW) and f32(2) * supy + f32(2) + f32(8) <= f32(RING):
            return OW
    return 0


def form_of(kind, fmt, H, W, oh, ow, aa):
    if kind == N.IMAGES_RESIZE:
        return {128: N.IMAGES_FORM_STREAM128, 64: N.IMAGES_FORM_STREAM64, 0: N.IMAGES_FORM_TILE}[rs_pick(H, W, oh, ow, aa, align_of(fmt))]
    return N.IMAGES_FORM_TILE


def cdiv(a, b):
    return (a + b - 1) // b


def tiles_of(kind, form, strip, H, W, oh, ow):
    if kind == N.IMAGES_TAIL:
        return cdiv(W, 256) * cdiv(H, 16)
    if form == N.IMAGES_FORM_TILE:
        return cdiv(ow, 32) * cdiv(oh, 8)
    return cdiv(ow, 128 if form == N.IMAGES_FORM_STREAM128 else 64) * cdiv(oh, strip)


def plan_ref(sizes, fmt, kind, oh, ow, aa):
    """[(form, strip, [slot indices], [first workgroups ..., grid])] of a list of (F, H, W)"""
    out = []
    for form in (N.IMAGES_FORM_TILE, N.IMAGES_FORM_STREAM128, N.IMAGES_FORM_STREAM64):
        idx = [i for i, (_, H, W) in enumerate(sizes) if form_of(kind, fmt, H, W, oh, ow, aa) == form]
        for a in range(0, len(idx), PER):
            grp = idx[a:a + PER]
            strip = 0
            if kind == N.IMAGES_RESIZE and form != N.IMAGES_FORM_TILE:
                OW = 128 if form == N.IMAGES_FORM_STREAM128 else 64
                frames = sum(sizes[i][0] for i in grp)
                strip = next((c for c in (64, 48, 32, 24, 16) if cdiv(ow, OW) * cdiv(oh, c) * frames >= 512), 32)
            first = [0]
            for i in grp:
                F_, H, W = sizes[i]
                first.append(first[-1] + F_ * tiles_of(kind, form, strip, H, W, oh, ow))
            out.append((form, strip, grp, first))
    return out


# ---- clips
def aff(preset, depth):
    fwd, inv = yuv.color_affine(preset[0], preset[1], depth)
    return (C.c_float * 12)(*[float(v) for v in inv.reshape(-1)]), (C.c_float * 12)(*[float(v) for v in fwd.reshape(-1)])


def to_t(planes):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)) for p in planes)


def random_clip(F_, H, W, fmt, seed=9):
    """uniformly random words: most (Y, Cb, Cr) triples are out of gamut, msb-aligned words carry non-zero low bits, the others pass 1023"""
    planar, depth, _, sx, sy = R.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    shapes = [(F_, H, W)] + ([(F_, H >> sy, W >> sx)] * 2 if planar else [(F_, H >> sy, W)])
    return tuple(rng.integers(0, top, size=s).astype(dt) for s in shapes)


class Pitched:
    """a clip whose planes are strided views of their own poisoned device buffers between GUARD bands.  `bviews`: the planes as bytes
    [F, R, row bytes] (what the C level sees: any pitch, odd ones included); `views`: the same memory as tensors of the planes' dtype (16-bit
    planes need `even` pads for that); `masks`: the bytes of each buffer no plane row owns (guards, pitch padding, spare rows)"""

    def __init__(self, planes, spare, pads, poison=0xA5, even=False, extra=0, fill=True):
        self.bufs, self.bviews, self.views, self.masks = [], [], [], []
        self.poison = poison
        for p, pad in zip(planes, pads):
            F_, R_, W = p.shape
            es = p.element_size()
            rowb = W * es
            pitch = rowb + (pad + extra) * (2 if (even and es == 2) else 1)
            n = F_ * (R_ + spare) * pitch
            buf = torch.full((GUARD + n + GUARD,), poison, dtype=torch.uint8, device="cuda")
            bv = buf[GUARD:GUARD + n].view(F_, R_ + spare, pitch)[:, :R_, :rowb]
            if fill:
                bv.copy_(p.contiguous().view(torch.uint8).view(F_, R_, rowb).cuda())
            m = torch.ones(F_, R_ + spare, pitch, dtype=torch.bool, device="cuda")
            m[:, :R_, :rowb] = False
            g = torch.ones(GUARD, dtype=torch.bool, device="cuda")
            self.bufs.append(buf)
            self.bviews.append(bv)
            self.views.append(bv if es == 1 else (bv.view(torch.uint16) if pitch % 2 == 0 else None))
            self.masks.append(torch.cat([g, m.flatten(), g]))
        self.views = tuple(self.views)

    def surface(self, fmt, first=0, count=None):
        """vs_yuv_surface_t of frames [first, first + count) of the planes"""
        planar, depth, msb, sx, sy = R.FORMATS[fmt]
        s = N.YuvSurface()
        for i, bv in enumerate(self.bviews):
            s.plane[i], s.pitch[i], s.frame_stride[i] = bv.data_ptr() + first * bv.stride(0), bv.stride(1), bv.stride(0)
        s.planar, s.depth, s.msb_aligned, s.chroma = int(planar), depth, int(msb), chroma_of(fmt)
        return s

    def untouched_outside(self):
        return all(bool(torch.all(buf[mask] == self.poison)) for buf, mask in zip(self.bufs, self.masks))

    def payload(self):
        return [bv.clone() for bv in self.bviews]


def slot_descs(fmt, slots):
    """vs_yuv_clip_desc_t array of [(src Pitched, dst Pitched or None, F, H, W, first_frame, first_key)]"""
    arr = (N.YuvClipDesc * max(1, len(slots)))()
    for i, (src, dst, F_, H, W, ff, fk) in enumerate(slots):
        arr[i].src = src.surface(fmt)
        if dst is not None:
            arr[i].dst = dst.surface(fmt)
        arr[i].F, arr[i].H, arr[i].W, arr[i].first_frame, arr[i].first_key = F_, H, W, ff, fk
    return arr


def tail_clips_desc(descs, n, fmt, preset, taps43, delta, hm, *, step, video_mode, Cd=1, attenuate=1, clamp=1, antialias=1, scaling_w=0.2):
    d = N.TailYuvClipsDesc()
    d.clips, d.n = descs, n
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(taps43, C.c_void_p) if taps43 is not None else None
    d.S_h, d.S_w, d.Cd = S, S, Cd
    d.attenuate, d.clamp, d.antialias = attenuate, clamp, antialias
    d.scaling_i, d.scaling_w = 1.0, scaling_w
    d.step, d.video_mode = step, video_mode
    d.yuv2rgb12, d.rgb2yuv12 = aff(preset, depth_of(fmt))
    return d


def tail_desc(src_surf, dst_surf, F_, H, W, fmt, preset, taps43, delta, hm, *, step, video_mode, Cd=1, attenuate=1, scaling_w=0.2):
    """vs_tail_yuv_desc_t of one slot with variant = 1 (the tile kernel)"""
    d = N.TailYuvDesc()
    d.src, d.dst = src_surf, dst_surf
    d.delta, d.hmap_lowres = N.ptr(delta), N.ptr(hm)
    d.taps43 = C.cast(taps43, C.c_void_p)
    d.F, d.H, d.W, d.S_h, d.S_w, d.Cd = F_, H, W, S, S, Cd
    d.step, d.video_mode, d.total_key = step, video_mode, (F_ + step - 1) // step
    d.attenuate, d.clamp, d.antialias = attenuate, 1, 1
    d.scaling_i, d.scaling_w = 1.0, scaling_w
    d.variant = 1
    d.yuv2rgb12, d.rgb2yuv12 = aff(preset, depth_of(fmt))
    return d
