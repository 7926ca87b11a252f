"""Target PSNR for lists on the CPU: the entry points of include/videoseal_lists_psnr.h are listed, declared and built and refuse bad arguments
on the host before any launch; the sizing functions against the launch plan and a hand-computed case; the argument checks of
Videoseal.embed_images_psnr / embed_clips_psnr, which run before the model asks for a device.  The library loads without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from oracle.weights import tiny_spec
from tests._model import cfg_of
from videoseal_amd import native as N
from videoseal_amd.model import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_SYMBOLS = ("vs_embed_tail_images_energy", "vs_embed_tail_images_scaled", "vs_embed_tail_clips_energy", "vs_embed_tail_clips_scaled",
               "vs_psnr_scale_items")
I64_SYMBOLS = ("vs_tail_images_energy_partial_doubles", "vs_tail_clips_energy_partial_doubles")
S = 16
IMAGES5 = [(16, 16), (23, 29), (37, 53), (40, 150), (34, 260)]
IMAGES33 = [[(16, 16), (17, 19), (23, 29)][i % 3] for i in range(33)]
SLOTS = [(5, 23, 29), (2, 37, 53), (1, 34, 260)]                    # (F, H, W)
ONE = C.c_void_p(256)                                             # a non-null address nothing ever follows: every call below stops before a launch


def _strip(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_symbols_are_listed_declared_and_built():
    header = open(os.path.join(ROOT, "include", "videoseal_lists_psnr.h")).read()
    main = _strip(open(os.path.join(ROOT, "include", "videoseal_hip.h")).read())
    lib = N.lib()
    assert sorted(N.LIST_PSNR_EXPORTS) == sorted(INT_SYMBOLS + I64_SYMBOLS) and len(set(N.LIST_PSNR_EXPORTS)) == 7
    decl = re.findall(r"(?m)^\s*(?:int|int64_t)\s+(vs_\w+)\s*\(", _strip(header))
    assert sorted(decl) == sorted(N.LIST_PSNR_EXPORTS)              # the header declares these and nothing else
    for sym, ret in [(s, "int") for s in INT_SYMBOLS] + [(s, "int64_t") for s in I64_SYMBOLS]:
        assert re.search(r"(?m)^" + ret + " " + sym + r"\(", header), sym
        assert hasattr(lib, sym), f"{sym} is declared but not exported"
        assert getattr(lib, sym).argtypes, f"{sym} has no ctypes signature in native.py"
        assert getattr(lib, sym).restype is (C.c_int if ret == "int" else C.c_int64), sym
        assert sym not in N.EXPORTS and sym not in N.REGION_EXPORTS and not re.search(r"\b" + sym + r"\b", main), sym
    # the opening comment says why the header stands alone, and that the regions header is arranged the same way
    opening = header.split("#ifndef")[0]
    assert "tests/_ledger.py" in opening and "videoseal_regions.h" in opening
    # the descriptors are reused unchanged
    assert "typedef" not in _strip(header)
    # the build's missing-symbol check covers the list
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "LIST_PSNR_EXPORTS" in entry


def _images_desc(sizes, att=1):
    arr = (N.ImageDesc * len(sizes))()
    for i, (H, W) in enumerate(sizes):
        arr[i].img, arr[i].out, arr[i].H, arr[i].W = 256, 256, H, W
    d = N.TailImagesDesc()
    d.images, d.n, d.delta, d.hmap_lowres, d.taps43 = arr, len(sizes), 256, 256, 256
    d.S_h, d.S_w, d.Cd, d.attenuate, d.clamp, d.antialias, d.io_u8 = S, S, 1, att, 1, 1, 0
    d.scaling_i, d.scaling_w = 1.0, 1.0
    return d, arr


def _clips_desc(slots, att=1):
    arr = (N.ClipDesc * len(slots))()
    ff = fk = 0
    for i, (F_, H, W) in enumerate(slots):
        arr[i].frames, arr[i].out, arr[i].F, arr[i].H, arr[i].W, arr[i].first_frame, arr[i].first_key = 256, 256, F_, H, W, ff, fk
        ff, fk = ff + F_, fk + F_
    d = N.TailClipsDesc()
    d.clips, d.n, d.delta, d.hmap_lowres, d.taps43 = arr, len(slots), 256, 256, 256
    d.S_h, d.S_w, d.Cd, d.attenuate, d.clamp, d.antialias, d.io_u8 = S, S, 1, att, 1, 1, 0
    d.scaling_i, d.scaling_w, d.step, d.video_mode = 1.0, 1.0, 1, 0
    return d, arr, ff


def test_bad_arguments_are_refused_on_the_host():
    lib = N.lib()
    d, keep = _images_desc(IMAGES5)
    assert lib.vs_embed_tail_images_energy(None, ONE, ONE, None) == -1
    assert lib.vs_embed_tail_images_energy(C.byref(d), None, ONE, None) == -1
    assert lib.vs_embed_tail_images_energy(C.byref(d), ONE, None, None) == -1
    assert lib.vs_embed_tail_images_scaled(None, ONE, None) == -1
    assert lib.vs_embed_tail_images_scaled(C.byref(d), None, None) == -1
    d.n = 0
    assert lib.vs_embed_tail_images_energy(C.byref(d), ONE, ONE, None) == -1
    assert lib.vs_embed_tail_images_scaled(C.byref(d), ONE, None) == -1
    d, keep = _images_desc(IMAGES5, att=2)
    assert lib.vs_embed_tail_images_energy(C.byref(d), ONE, ONE, None) == N.ERR_UNSUPPORTED
    assert lib.vs_embed_tail_images_scaled(C.byref(d), ONE, None) == N.ERR_UNSUPPORTED
    d, keep = _images_desc(IMAGES5)
    keep[2].H = 0
    assert lib.vs_embed_tail_images_energy(C.byref(d), ONE, ONE, None) == -1
    d, keep = _images_desc(IMAGES5)
    d.delta = None
    assert lib.vs_embed_tail_images_scaled(C.byref(d), ONE, None) == -1

    d, keep, nf = _clips_desc(SLOTS)
    assert nf == 8
    assert lib.vs_embed_tail_clips_energy(None, ONE, ONE, nf, None) == -1
    assert lib.vs_embed_tail_clips_energy(C.byref(d), None, ONE, nf, None) == -1
    assert lib.vs_embed_tail_clips_energy(C.byref(d), ONE, None, nf, None) == -1
    assert lib.vs_embed_tail_clips_scaled(None, ONE, nf, None) == -1
    assert lib.vs_embed_tail_clips_scaled(C.byref(d), None, nf, None) == -1
    # first_frame + F > n_frames: the last slot ends at frame 8
    assert lib.vs_embed_tail_clips_energy(C.byref(d), ONE, ONE, nf - 1, None) == -1
    assert lib.vs_embed_tail_clips_scaled(C.byref(d), ONE, nf - 1, None) == -1
    assert lib.vs_embed_tail_clips_energy(C.byref(d), ONE, ONE, 0, None) == -1
    d.n = 0
    assert lib.vs_embed_tail_clips_energy(C.byref(d), ONE, ONE, nf, None) == -1
    assert lib.vs_embed_tail_clips_scaled(C.byref(d), ONE, nf, None) == -1
    d, keep, nf = _clips_desc(SLOTS, att=2)
    assert lib.vs_embed_tail_clips_energy(C.byref(d), ONE, ONE, nf, None) == N.ERR_UNSUPPORTED
    assert lib.vs_embed_tail_clips_scaled(C.byref(d), ONE, nf, None) == N.ERR_UNSUPPORTED

    assert lib.vs_psnr_scale_items(None, ONE, None, 3, 0, 42.0, 0.0, ONE, None) == -1
    assert lib.vs_psnr_scale_items(ONE, None, None, 3, 0, 42.0, 0.0, ONE, None) == -1
    assert lib.vs_psnr_scale_items(ONE, ONE, None, 3, 0, 42.0, 0.0, None, None) == -1
    assert lib.vs_psnr_scale_items(ONE, ONE, None, 0, 0, 42.0, 0.0, ONE, None) == -1
    assert lib.vs_psnr_scale_items(ONE, ONE, ONE, 3, 0, 42.0, 0.0, ONE, None) == -1           # a prefix without groups
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.vs_psnr_scale_items(ONE, ONE, None, 3, 0, bad, 0.0, ONE, None) == -1
        assert lib.vs_psnr_scale_items(ONE, ONE, ONE, 3, 2, bad, 0.0, ONE, None) == -1


def _sizes_arr(sizes):
    arr = (N.ImageDesc * len(sizes))()
    for i, (H, W) in enumerate(sizes):
        arr[i].H, arr[i].W = H, W
    return arr


def _slots_arr(slots):
    arr = (N.ClipDesc * len(slots))()
    for i, (F_, H, W) in enumerate(slots):
        arr[i].F, arr[i].H, arr[i].W = F_, H, W
    return arr


def test_sizing_functions_follow_the_plan():
    lib = N.lib()
    for u8 in (0, 1):
        for sizes in (IMAGES5, IMAGES33):
            plan = N.images_plan(sizes, N.IMAGES_TAIL, bool(u8), S, S, True)
            assert len(plan) == (2 if len(sizes) > N.IMAGES_PER_LAUNCH else 1)
            assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr(sizes), len(sizes), u8, S, S, 1) == sum(g[3][-1] for g in plan)
        plan = N.clips_plan(SLOTS, N.IMAGES_TAIL, bool(u8), S, S, True)
        assert lib.vs_tail_clips_energy_partial_doubles(_slots_arr(SLOTS), len(SLOTS), u8, S, S, 1) == sum(g[3][-1] for g in plan)
    # by hand: tiles of 256 columns x 16 rows
    tiles = {(16, 16): 1, (23, 29): 2, (37, 53): 3, (40, 150): 3, (34, 260): 2 * 3, (17, 19): 2}
    assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr([(34, 260)]), 1, 0, S, S, 1) == 6
    assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr(IMAGES5), 5, 0, S, S, 1) == sum(tiles[s] for s in IMAGES5) == 15
    assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr(IMAGES33), 33, 0, S, S, 1) == sum(tiles[s] for s in IMAGES33)
    assert lib.vs_tail_clips_energy_partial_doubles(_slots_arr(SLOTS), 3, 0, S, S, 1) == 5 * 2 + 2 * 3 + 1 * 6
    # bad arguments
    assert lib.vs_tail_images_energy_partial_doubles(None, 1, 0, S, S, 1) == -1
    assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr(IMAGES5), -1, 0, S, S, 1) == -1
    assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr(IMAGES5), 5, 0, 0, S, 1) == -1
    assert lib.vs_tail_images_energy_partial_doubles(_sizes_arr([(16, 0)]), 1, 0, S, S, 1) == -1
    assert lib.vs_tail_clips_energy_partial_doubles(None, 1, 0, S, S, 1) == -1
    assert lib.vs_tail_clips_energy_partial_doubles(_slots_arr([(0, 16, 16)]), 1, 0, S, S, 1) == -1
    assert lib.vs_tail_clips_energy_partial_doubles(_slots_arr(SLOTS), 3, 0, S, -2, 1) == -1
    assert lib.vs_tail_images_energy_partial_doubles(None, 0, 0, S, S, 1) == 0                # an empty list needs nothing


def test_the_python_calls_refuse_before_they_need_a_device():
    model = build_model(cfg_of(tiny_spec())).eval()
    nb = model.embedder.cfg.nbits
    imgs = [torch.rand(3, 16, 16), torch.rand(3, 23, 29)]
    clips = [torch.rand(5, 3, 23, 29), torch.rand(2, 3, 37, 53)]
    for call, items in ((model.embed_images_psnr, imgs), (model.embed_clips_psnr, clips)):
        for bad in (float("nan"), float("inf"), 0, -3.0, "42", None, True):
            with pytest.raises(ValueError, match="target_psnr"):
                call(items, bad)
        for bad in (0.0, -1.0, float("nan"), "2", True):
            with pytest.raises(ValueError, match="max_scaling_w"):
                call(items, 42.0, max_scaling_w=bad)
        with pytest.raises(ValueError, match="rows"):
            call(items, 42.0, msgs=torch.zeros(3, nb))
        with pytest.raises(ValueError, match="all fp32"):
            call([items[0], (items[1] * 255).byte()], 42.0)
        with pytest.raises(TypeError, match="sequence of tensors"):
            call([items[0], None], 42.0)
    with pytest.raises(ValueError, match="per must be"):
        model.embed_clips_psnr(clips, 42.0, per="chunk")
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        model.embed_images_psnr([torch.rand(4, 16, 16)], 42.0)
    with pytest.raises(ValueError, match=r"\[F, 3, H, W\]"):
        model.embed_clips_psnr([torch.rand(3, 16, 16)], 42.0)
    model.clamp = False
    with pytest.raises(ValueError, match="clamp"):
        model.embed_images_psnr([torch.zeros(16, 16, 3, dtype=torch.uint8)], 42.0)
    with pytest.raises(ValueError, match="clamp"):
        model.embed_clips_psnr([torch.zeros(2, 16, 16, 3, dtype=torch.uint8)], 42.0)
    # the signatures: the new calls as the issue states them, the existing ones as they were
    assert list(inspect.signature(model.embed_images_psnr).parameters) == ["imgs", "target_psnr", "msgs", "max_scaling_w", "interpolation",
                                                                           "lowres_attenuation"]
    assert list(inspect.signature(model.embed_clips_psnr).parameters) == ["clips", "target_psnr", "msgs", "per", "max_scaling_w", "interpolation",
                                                                          "lowres_attenuation"]
    assert list(inspect.signature(model.embed_images).parameters) == ["imgs", "msgs", "interpolation", "lowres_attenuation"]
    assert list(inspect.signature(model.embed_clips).parameters) == ["clips", "msgs", "interpolation", "lowres_attenuation"]
