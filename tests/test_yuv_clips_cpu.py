"""Lists of YUV clips on the CPU: the entry points of include/videoseal_yuv_clips.h are declared there (and not in videoseal_hip.h), built
and bound; the launch plan both launchers walk (csrc/yuv_clips_plan.h, exported as vs_yuv_clips_plan) is checked against a Python
restatement (tests/_yuv_clips_util.py) and through a stand-alone program under -fsanitize=address,undefined (nothing sanitized is loaded into
Python); every refusal that is decided before HIP is touched returns its code; Videoseal.*_yuv list methods validate before the engine
exists.  The library loads without a GPU and none of this touches one."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle.weights import tiny_spec
from tests import _yuv_clips_util as U
from tests import _yuv_ref as R
from tests._model import cfg_of
from videoseal_amd import native as N
from videoseal_amd import yuv
from videoseal_amd.model import Videoseal, build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = U.PER
RNG = np.random.RandomState(11)


def _seeded(n):
    """(F, H, W) with even sides: small frames (tile form at 64, streaming at 256), mid-sized ones (128 columns) and 4 x ones (64 columns)"""
    out = []
    for i in range(n):
        lo, hi = ((16, 140), (200, 520), (130, 260))[i % 3]
        h, w = (int(v) * 2 for v in RNG.randint(lo // 2, hi // 2, size=2))
        out.append((int(RNG.choice([1, 3, 5, 9])), h, w))
    return out


LISTS = {"none": [], "one": _seeded(1), "PER": _seeded(PER), "PER + 1": _seeded(PER + 1), "2 PER + 3": _seeded(2 * PER + 3),
         "PER + 1 of one size": [(3, 72, 88)] * (PER + 1),
         "table": [(f, U.SIZES[n][0] & ~1, U.SIZES[n][1] & ~1) for n, f in zip("DBACEG", (1, 3, 5, 9, 1, 3))]}
CASES = [(name, fmt, kind, S, aa) for name in LISTS for fmt in ("nv12", "i420", "yuv444p10") for kind in (N.IMAGES_RESIZE, N.IMAGES_TAIL)
         for S in (64, 256) for aa in (True, False)]
DECLS = ("vs_sizeof_yuv_clip_desc", "vs_sizeof_tail_yuv_clips_desc", "vs_sizeof_yuv_clips_group", "vs_resize_pre_yuv_clips",
         "vs_embed_tail_yuv_clips", "vs_yuv_clips_plan")


# ---------------------------------------------------------------------------------------------------- header and bindings
def test_the_header_is_exported_bound_and_apart():
    header = open(os.path.join(ROOT, "include", "videoseal_yuv_clips.h")).read()
    main = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    declared = re.findall(r"^int (vs_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(DECLS) == sorted(N.YUV_CLIPS_EXPORTS)
    lib = N.lib()
    for sym in declared:
        assert hasattr(lib, sym) and sym not in main and sym not in N.EXPORTS, sym
    assert "vs_yuv_clip_desc" not in main and "VS_YUV_CLIPS_PER_LAUNCH" not in main
    m = re.search(r"#define VS_YUV_CLIPS_PER_LAUNCH (\d+)", header)
    assert m and int(m.group(1)) == PER == 16
    assert lib.vs_sizeof_yuv_clip_desc() == C.sizeof(N.YuvClipDesc)
    assert lib.vs_sizeof_tail_yuv_clips_desc() == C.sizeof(N.TailYuvClipsDesc)
    assert lib.vs_sizeof_yuv_clips_group() == C.sizeof(N.YuvClipsGroup)
    assert lib.vs_version() == 3


def test_ctypes_mirrors_match_the_header():
    header = open(os.path.join(ROOT, "include", "videoseal_yuv_clips.h")).read()
    for name, cls in (("vs_yuv_clip_desc", N.YuvClipDesc), ("vs_tail_yuv_clips_desc", N.TailYuvClipsDesc), ("vs_yuv_clips_group", N.YuvClipsGroup)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + "_t;", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        body = re.sub(r"\[[^\]]*\]", "", body)                                # array extents
        members = [m.strip().split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()
                   for m in re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip()).split(",")]
        assert members == [f for f, _ in cls._fields_], (name, members)


# ---------------------------------------------------------------------------------------------------- the plan
def test_the_lists_take_every_form():
    forms = {U.form_of(N.IMAGES_RESIZE, fmt, H, W, S, S, aa) for name, fmt, kind, S, aa in CASES for _, H, W in LISTS[name]}
    assert forms == {N.IMAGES_FORM_TILE, N.IMAGES_FORM_STREAM128, N.IMAGES_FORM_STREAM64}
    # the margin matters: a size at which nv12 (16 columns) streams and i420 (32 columns) does not
    assert any(U.rs_pick(H, W, 64, 64, aa, 16) != U.rs_pick(H, W, 64, 64, aa, 32) for H in (64,) for W in range(190, 230, 2) for aa in (True, False))


@pytest.mark.parametrize("name", list(LISTS))
def test_plan_equals_the_restated_rules(name):
    sizes = LISTS[name]
    for _, fmt, kind, S, aa in (c for c in CASES if c[0] == name):
        assert N.yuv_clips_plan(sizes, fmt, kind, S, S, aa) == U.plan_ref(sizes, fmt, kind, S, S, aa), (name, fmt, kind, S, aa)


@pytest.mark.parametrize("name", list(LISTS))
def test_every_slot_once_bounded_groups_prefix_sums_and_strips(name):
    """stated on the plan alone: workgroup w of a launch belongs to the slot k with first_wg[k] <= w < first_wg[k + 1], and is tile
    (w - first_wg[k]) % tiles of frame (w - first_wg[k]) // tiles of it"""
    sizes = LISTS[name]
    for _, fmt, kind, S, aa in (c for c in CASES if c[0] == name):
        plan = N.yuv_clips_plan(sizes, fmt, kind, S, S, aa)
        seen = {}
        for form, strip, slot, first in plan:
            assert 1 <= len(slot) <= PER and len(first) == len(slot) + 1 and first[0] == 0
            assert slot == sorted(slot)                                      # list order inside a group
            frames = sum(sizes[i][0] for i in slot)
            if kind == N.IMAGES_RESIZE and form != N.IMAGES_FORM_TILE:       # the strip follows the group's frame count
                OW = 128 if form == N.IMAGES_FORM_STREAM128 else 64
                assert strip == next((c for c in (64, 48, 32, 24, 16) if U.cdiv(S, OW) * U.cdiv(S, c) * frames >= 512), 32)
            else:
                assert strip == 0
            for k, i in enumerate(slot):
                F_, H, W = sizes[i]
                assert U.form_of(kind, fmt, H, W, S, S, aa) == form
                assert first[k + 1] - first[k] == F_ * U.tiles_of(kind, form, strip, H, W, S, S) >= 1, (name, i)
                assert i not in seen
                seen[i] = form
        assert sorted(seen) == list(range(len(sizes)))                       # every slot in exactly one launch
        per_form = {}
        for f in seen.values():
            per_form[f] = per_form.get(f, 0) + 1
        assert len(plan) == sum(U.cdiv(c, PER) for c in per_form.values())


def test_group_counts_at_the_launch_limit_and_refusals_of_the_plan():
    for n, groups in ((0, 0), (1, 1), (PER, 1), (PER + 1, 2), (2 * PER + 3, 3)):
        plan = N.yuv_clips_plan([(3, 96, 80)] * n, "p010", N.IMAGES_TAIL, 64, 64, True)
        assert len(plan) == groups and [len(g[2]) for g in plan] == [min(PER, n - a) for a in range(0, n, PER)]
    (_, _, slot, first), = N.yuv_clips_plan([(2, 64, 64), (3, 2048, 2048)], "nv12", N.IMAGES_TAIL, 256, 256, True)
    assert slot == [0, 1] and first == [0, 2 * 4, 2 * 4 + 3 * 8 * 128]
    lib, n = N.lib(), C.c_int(-1)
    d = (N.YuvClipDesc * 2)()
    for i in range(2):
        d[i].F, d[i].H, d[i].W = 2, 1 << 24, 1 << 18
        d[i].src.planar, d[i].src.depth, d[i].src.msb_aligned, d[i].src.chroma = 0, 8, 0, 420
    assert lib.vs_yuv_clips_plan(d, 2, N.IMAGES_TAIL, 64, 64, 1, None, 0, C.byref(n)) == N.ERR_UNSUPPORTED       # past 2^31 - 1 workgroups
    d[0].H = d[0].W = d[1].H = d[1].W = 64
    assert lib.vs_yuv_clips_plan(d, 2, N.IMAGES_TAIL, 64, 64, 1, None, 0, C.byref(n)) == 0 and n.value == 1
    assert lib.vs_yuv_clips_plan(None, 0, N.IMAGES_TAIL, 64, 64, 1, None, 0, C.byref(n)) == 0 and n.value == 0  # an empty plan
    assert lib.vs_yuv_clips_plan(None, 1, N.IMAGES_TAIL, 64, 64, 1, None, 0, C.byref(n)) == -1
    assert lib.vs_yuv_clips_plan(d, 2, N.IMAGES_TAIL, 64, 64, 1, None, 0, None) == -1
    assert lib.vs_yuv_clips_plan(d, 2, 7, 64, 64, 1, None, 0, C.byref(n)) == -1
    assert lib.vs_yuv_clips_plan(d, 2, N.IMAGES_TAIL, 0, 64, 1, None, 0, C.byref(n)) == -1
    d[1].F = 0
    assert lib.vs_yuv_clips_plan(d, 2, N.IMAGES_TAIL, 64, 64, 1, None, 0, C.byref(n)) == -1
    d[1].F, d[0].src.depth = 1, 12
    assert lib.vs_yuv_clips_plan(d, 2, N.IMAGES_TAIL, 64, 64, 1, None, 0, C.byref(n)) == N.ERR_UNSUPPORTED


def test_plan_unit_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/yuv_clips_plan_walk.cpp + csrc/yuv_clips_plan.hip compiled as plain C++ with -fsanitize=address,undefined: every list again, the
    plans it prints equal the restated rules, and no report from either sanitizer"""
    lists = tmp_path / "lists.txt"
    rows = []
    for name, fmt, kind, S, aa in CASES:
        planar, depth, msb, _, _ = R.FORMATS[fmt]
        rows.append(f"{kind} {int(planar)} {depth} {int(msb)} {U.chroma_of(fmt)} {S} {S} {int(aa)} {len(LISTS[name])} "
                    + " ".join(f"{f} {h} {w}" for f, h, w in LISTS[name]) + "\n")
    lists.write_text("".join(rows))
    exe = tmp_path / "yuv_clips_plan_walk"
    cc = shutil.which("hipcc") or "hipcc"
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "videoseal_amd", "csrc"),
                    os.path.join(ROOT, "videoseal_amd", "csrc", "yuv_clips_plan.hip"), os.path.join(ROOT, "tests", "yuv_clips_plan_walk.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(lists)], capture_output=True, text=True)
    assert r.returncode == 0 and f"{len(CASES)} lists, 0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-2000:])
    got, cur = [], None
    for ln in r.stdout.splitlines():
        if ln.startswith("list "):
            cur = []
            got.append(cur)
        elif ln.startswith("g "):
            head, slot, first = ln[2:].split("|")
            form, strip, count = map(int, head.split())
            slot, first = list(map(int, slot.split())), list(map(int, first.split()))
            assert len(slot) == count
            cur.append((form, strip, slot, first))
    assert got == [U.plan_ref(LISTS[name], fmt, kind, S, S, aa) for name, fmt, kind, S, aa in CASES]


# ---------------------------------------------------------------------------------------------------- refusals before HIP is touched
def _host_slots(fmt, sizes):
    """descriptors over HOST memory of the right sizes: every refusal below is decided before a pointer is used"""
    planar, depth, msb, sx, sy = R.FORMATS[fmt]
    keep, arr = [], (N.YuvClipDesc * len(sizes))()
    for i, (F_, H, W) in enumerate(sizes):
        es = 2 if depth > 8 else 1
        shapes = [(H, W)] + ([(H >> sy, W >> sx)] * 2 if planar else [(H >> sy, W)])
        for which in ("src", "dst"):
            s = getattr(arr[i], which)
            for p, (r, w) in enumerate(shapes):
                buf = np.zeros(F_ * r * w * es, dtype=np.uint8)
                keep.append(buf)
                s.plane[p], s.pitch[p], s.frame_stride[p] = buf.ctypes.data, w * es, r * w * es
            s.planar, s.depth, s.msb_aligned, s.chroma = int(planar), depth, int(msb), U.chroma_of(fmt)
        arr[i].F, arr[i].H, arr[i].W, arr[i].first_frame, arr[i].first_key = F_, H, W, 3 * i, 2 * i
    return arr, keep


def test_refusals_that_need_no_gpu():
    lib = N.lib()
    BAD, UNS = -1, N.ERR_UNSUPPORTED
    dec, enc = U.aff(("bt709", False), 8)
    out = C.cast((C.c_float * 4)(), C.c_void_p)           # never written: every call below is refused before a launch

    def resize(arr, n=2, dec_=dec, oh=64, rgb=out, key=None, key_step=1):
        return lib.vs_resize_pre_yuv_clips(arr, n, dec_, oh, 64, 1, rgb, 1.0, 0.0, key, key_step, None, None)

    def tail(arr, n=2, **kw):
        d = N.TailYuvClipsDesc()
        d.clips, d.n, d.delta = arr, n, out
        d.S_h, d.S_w, d.Cd, d.attenuate, d.clamp, d.antialias, d.step, d.video_mode = 64, 64, 1, 0, 1, 1, 2, 0
        d.yuv2rgb12, d.rgb2yuv12 = dec, enc
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.vs_embed_tail_yuv_clips(C.byref(d), None)

    def both(arr, want, **kw):
        assert resize(arr, **kw) == want and tail(arr, **kw) == want

    sizes = [(3, 18, 34), (1, 72, 88)]
    arr, keep = _host_slots("nv12", sizes)
    assert resize(None) == BAD and resize(arr, n=0) == BAD and resize(arr, n=-1) == BAD and resize(arr, dec_=None) == BAD
    assert resize(arr, oh=0) == BAD and resize(arr, rgb=None) == BAD and resize(arr, rgb=None, key=out, key_step=0) == BAD
    assert lib.vs_embed_tail_yuv_clips(None, None) == BAD and tail(None) == BAD and tail(arr, n=0) == BAD and tail(arr, delta=None) == BAD
    assert tail(arr, clamp=0) == BAD and tail(arr, step=0) == BAD and tail(arr, video_mode=3) == BAD and tail(arr, video_mode=-1) == BAD
    assert tail(arr, Cd=2) == BAD and tail(arr, S_h=0) == BAD and tail(arr, attenuate=2) == UNS
    assert tail(arr, attenuate=1, hmap_lowres=None, taps43=None) == BAD          # the full-resolution heat-map needs its taps
    for member, value in (("F", 0), ("H", 0), ("W", -2), ("first_frame", -1), ("first_key", -1)):
        arr, keep = _host_slots("nv12", sizes)
        setattr(arr[1], member, value)
        both(arr, BAD)
    for fmt, H, W in (("nv12", 19, 34), ("i420", 18, 35), ("nv16", 18, 35), ("yuv422p10", 19, 35)):       # a size the chroma rule forbids
        arr, keep = _host_slots(fmt, [(1, H + (H & 1), W + (W & 1)), (2, 20, 36)])
        arr[0].H, arr[0].W = H, W                                           # (the planes hold the next even size: pitches and strides suffice)
        both(arr, BAD)
    arr, keep = _host_slots("i420", sizes)
    arr[1].src.plane[2] = None
    both(arr, BAD)
    arr, keep = _host_slots("i420", sizes)
    arr[0].src.pitch[1] = 16                                                # 17 samples per chroma row
    both(arr, BAD)
    arr, keep = _host_slots("p010", sizes)
    arr[0].src.frame_stride[0] = 17 * 68 + 67                               # frames of a plane overlap by one byte
    both(arr, BAD)
    arr, keep = _host_slots("nv12", sizes)
    arr[1].dst.pitch[0] = 87
    assert tail(arr) == BAD                                                 # (the resize ignores dst)
    # formats
    arr, keep = _host_slots("nv12", sizes)
    arr[0].src.depth = arr[0].dst.depth = 12
    both(arr, UNS)
    arr, keep = _host_slots("nv12", sizes)
    arr[0].src.chroma = arr[0].dst.chroma = 444                             # semi-planar 4:4:4
    both(arr, UNS)
    arr, keep = _host_slots("nv12", sizes)
    a2, k2 = _host_slots("nv16", sizes)
    arr[1].src, arr[1].dst = a2[1].src, a2[1].dst                           # slots of different formats
    both(arr, UNS)
    arr, keep = _host_slots("nv12", sizes)
    arr[1].dst = a2[1].dst                                                  # a slot whose src and dst formats differ
    assert tail(arr) == UNS


# ---------------------------------------------------------------------------------------------------- Python validation
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(cfg_of(tiny_spec())).eval()          # stays on the CPU: no engine is ever created


def _planes(fmt, F_, H, W):
    return tuple(torch.zeros(s, dtype=yuv.fmt_dtype(fmt)) for s in yuv.plane_shapes(fmt, F_, H, W))


def test_python_validation_happens_before_the_engine(cpu_model, monkeypatch):
    m = cpu_model
    monkeypatch.setattr(Videoseal, "_engine", lambda self: pytest.fail("the engine was touched"))
    for name in ("embed_clips_yuv", "detect_clips_yuv", "extract_messages_yuv"):
        assert callable(getattr(Videoseal, name, None))
    good = [_planes("nv12", 3, 18, 34), _planes("nv12", 0, 72, 88)]
    k = m.embedder.cfg.nbits
    for call in (lambda c, f, **kw: m.embed_clips_yuv(c, f, torch.zeros(len(c), k), **kw), m.detect_clips_yuv, m.extract_messages_yuv):
        with pytest.raises(ValueError):                                        # mixed formats: an i420 clip in an nv12 list
            call(good + [_planes("i420", 1, 18, 34)], "nv12")
        with pytest.raises(ValueError):
            call([yuv.Clip(_planes("nv16", 1, 18, 34), "nv16")], "nv12")
        with pytest.raises(ValueError, match="matrix"):
            call(good, "nv12", matrix="bt470")
        with pytest.raises(ValueError):
            call(good, "nv21")
        with pytest.raises(ValueError):                                        # odd H for 4:2:0, odd W for 4:2:2
            call([tuple(torch.zeros(s, dtype=torch.uint8) for s in ((1, 19, 34), (1, 9, 34)))], "nv12")
        with pytest.raises(ValueError):
            call([tuple(torch.zeros(s, dtype=torch.uint8) for s in ((1, 18, 35), (1, 18, 34)))], "nv16")
    with pytest.raises(TypeError, match=r"\bembed_clips\b"):
        m.embed_clips_yuv([torch.zeros(2, 3, 18, 34)], "nv12")
    with pytest.raises(TypeError, match=r"\bdetect_clips\b"):
        m.detect_clips_yuv([torch.zeros(2, 18, 34, 3, dtype=torch.uint8)], "nv12")
    with pytest.raises(TypeError, match=r"\bextract_messages\b"):
        m.extract_messages_yuv([torch.zeros(2, 3, 18, 34)], "nv12")
    with pytest.raises(ValueError, match="rows"):
        m.embed_clips_yuv(good, "nv12", torch.zeros(3, k))
    with pytest.raises(ValueError):
        m.extract_messages_yuv(good, "nv12", aggregation="median")
    msgs = torch.zeros(0, k)
    out = m.embed_clips_yuv([], "p010", msgs)
    assert out["planes_w"] == [] and out["imgs_w"] == [] and out["msgs"] is msgs
    assert m.detect_clips_yuv([], "p010") == {"preds": []}
    e = m.extract_messages_yuv([], "p010")
    assert e.shape == (0, k) and e.dtype == torch.bool
    m.clamp = False
    try:
        with pytest.raises(NotImplementedError, match="clamp"):
            m.embed_clips_yuv(good, "nv12", torch.zeros(2, k))
    finally:
        m.clamp = True
