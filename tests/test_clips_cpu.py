"""Lists of clips on the CPU: the new entry points are listed, declared and built; the launch plan both launchers walk (csrc/clips_plan.h,
exported as vs_clips_plan) is checked on seeded slot lists; the packing of clips into passes (videoseal_amd/clips.py) is checked on plain
data.  The library loads without a GPU; neither the planner nor the packing touches one."""
import ctypes as C
import os
import re

import numpy as np

from videoseal_amd import clips as CL
from videoseal_amd import native as N
from videoseal_amd.streaming import DET_BATCH, KEY_BATCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = N.IMAGES_PER_LAUNCH
SYMBOLS = ("vs_resize_pre_clips", "vs_embed_tail_clips", "vs_clips_plan", "vs_aggregate_clips")

# the sizes of the kernel tests (tests/test_gpu_clips.py) and their lengths
SIZES = [(5, 7), (48, 40), (64, 64), (9, 300), (130, 33), (257, 191), (18, 260)]
LENGTHS = (1, 2, 3, 4, 5, 9)
RNG = np.random.RandomState(11)
LISTS = {
    "table": [(LENGTHS[i % 6], h, w) for i, (h, w) in enumerate(SIZES)],
    "reversed": [(LENGTHS[i % 6], h, w) for i, (h, w) in enumerate(SIZES)][::-1],
    "35 one-frame slots": [(1,) + SIZES[i % 7] for i in range(35)],
    "one": [(9, 130, 33)],
    "none": [],
    "seeded": [(int(f), int(h), int(w)) for f, h, w in zip(RNG.randint(1, 20, 70), RNG.randint(1, 1100, 70), RNG.randint(1, 1100, 70))],
}
CASES = [(name, kind, u8, S, aa) for name in LISTS for kind in (N.IMAGES_RESIZE, N.IMAGES_TAIL) for u8 in (False, True)
         for S in (64, 256) for aa in (True, False)]


def cdiv(a, b):
    return (a + b - 1) // b


def tiles_of(kind, form, strip, H, W, S):
    if kind == N.IMAGES_TAIL:
        return cdiv(W, 256) * cdiv(H, 16)
    if form == N.IMAGES_FORM_TILE:
        return cdiv(S, 32) * cdiv(S, 8)
    return cdiv(S, 128 if form == N.IMAGES_FORM_STREAM128 else 64) * cdiv(S, strip)


def test_the_symbols_are_listed_declared_and_built():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    lib = N.lib()
    for sym in SYMBOLS:
        assert sym in N.EXPORTS and re.search(r"\bint " + sym + r"\(", header) and hasattr(lib, sym), sym
    assert "typedef struct vs_clip_desc {" in header and "typedef struct vs_tail_clips_desc {" in header
    # argument validation happens on the host before any launch: refused without a GPU
    n = C.c_int(-1)
    assert lib.vs_resize_pre_clips(None, 1, 0, 64, 64, 1, None, 1.0, 0.0, None, 1, None, None) == -1
    assert lib.vs_embed_tail_clips(None, None) == -1
    assert lib.vs_aggregate_clips(None, 17, None, 1, 16, 0, None, None) == -1
    assert lib.vs_clips_plan(None, 1, 0, 0, 64, 64, 1, None, 0, C.byref(n)) == -1
    assert lib.vs_clips_plan(None, 0, 0, 0, 64, 64, 1, None, 0, None) == -1
    assert lib.vs_clips_plan(None, 0, 7, 0, 64, 64, 1, None, 0, C.byref(n)) == -1
    d = (N.ClipDesc * 1)()
    d[0].H, d[0].W = 8, 8
    assert lib.vs_clips_plan(d, 1, 0, 0, 64, 64, 1, None, 0, C.byref(n)) == -1          # F = 0
    assert lib.vs_clips_plan(None, 0, 0, 0, 64, 64, 1, None, 0, C.byref(n)) == 0 and n.value == 0      # n = 0: an empty plan


def test_ctypes_mirrors_match_the_header():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    for name, cls in (("vs_clip_desc", N.ClipDesc), ("vs_tail_clips_desc", N.TailClipsDesc)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + "_t;", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = [m.strip().split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()
                   for m in re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip()).split(",")]
        assert members == [f for f, _ in cls._fields_], (name, members)
    assert C.sizeof(N.ClipDesc) == 48 and N.AGGREGATIONS == {"avg": 0, "squared_avg": 1, "l1norm_avg": 2, "l2norm_avg": 3}
    for name, v in N.AGGREGATIONS.items():
        assert re.search(r"#define VS_AGG_\w+ %d\b" % v, header), name


def test_plan_every_slot_frame_tile_once():
    """stated on the plan alone: workgroup w of a launch belongs to the slot k with first_wg[k] <= w < first_wg[k + 1]; inside it, frame
    (w - first_wg[k]) // tiles and tile (w - first_wg[k]) % tiles -- frame-major, so neighbouring workgroups share a frame"""
    for name, kind, u8, S, aa in CASES:
        slots = LISTS[name]
        plan = N.clips_plan(slots, kind, u8, S, S, aa)
        if not slots:
            assert plan == []
            continue
        seen, total = set(), 0
        per_form = {}
        for form, strip, idx, first in plan:
            assert 1 <= len(idx) <= PER and len(first) == len(idx) + 1 and first[0] == 0
            assert idx == sorted(idx)                                          # list order inside a group
            assert all(b >= a for a, b in zip(first, first[1:]))               # non-decreasing
            per_form[form] = per_form.get(form, 0) + len(idx)
            for k, i in enumerate(idx):
                F_, H, W = slots[i]
                tiles = tiles_of(kind, form, strip, H, W, S)
                if kind == N.IMAGES_RESIZE and form != N.IMAGES_FORM_TILE:
                    assert strip >= 1 and not u8
                assert first[k + 1] - first[k] == F_ * tiles and tiles >= 1, (name, i)
                for w in range(first[k], first[k + 1]):                        # every (slot, frame, tile) exactly once
                    item = (i, (w - first[k]) // tiles, (w - first[k]) % tiles)
                    assert item not in seen and item[1] < F_
                    seen.add(item)
            total += first[len(idx)]                                           # first_wg[count] is the grid
        assert len(seen) == total == sum(F_ * tiles_of(kind, f, st, H, W, S) for f, st, idx, _ in plan for F_, H, W in (slots[i] for i in idx))
        assert sorted({i for i, _, _ in seen}) == list(range(len(slots)))
        assert len(plan) == sum(cdiv(c, PER) for c in per_form.values())      # launches: per form, never a function of n itself


def test_plan_at_the_launch_limit_and_against_the_image_plan():
    S = 64
    # 35 one-frame slots: two groups per form
    for kind in (N.IMAGES_RESIZE, N.IMAGES_TAIL):
        for u8 in (False, True):
            plan = N.clips_plan(LISTS["35 one-frame slots"], kind, u8, S, S, True)
            forms = {}
            for form, _, idx, _ in plan:
                forms.setdefault(form, []).append(len(idx))
            n_of = {}
            for f, (_, H, W) in ((N.images_plan([(H, W)], kind, u8, S, S, True)[0][0], (1, H, W)) for _, H, W in LISTS["35 one-frame slots"]):
                n_of[f] = n_of.get(f, 0) + 1
            assert {f: sum(v) for f, v in forms.items()} == n_of
            assert all(len(v) == cdiv(n_of[f], PER) and all(c <= PER for c in v) for f, v in forms.items())
    plan = N.clips_plan([(1, 96, 80)] * 35, N.IMAGES_TAIL, False, S, S, True)
    assert [len(g[2]) for g in plan] == [32, 3]
    # a one-frame slot has the workgroups of the image plan (strip equal where the frame counts are: one slot of one frame, one image)
    for H, W in SIZES + [(192, 200), (256, 256)]:
        for kind in (N.IMAGES_RESIZE, N.IMAGES_TAIL):
            for u8 in (False, True):
                for aa in (True, False):
                    assert N.clips_plan([(1, H, W)], kind, u8, S, S, aa) == N.images_plan([(H, W)], kind, u8, S, S, aa), (H, W, kind, u8, aa)
    # F frames: F times the tiles of the image plan at the same strip
    (form, strip, idx, first), = N.clips_plan([(7, 9, 300)], N.IMAGES_TAIL, False, S, S, True)
    assert idx == [0] and first == [0, 7 * 2 * 1]
    # a launch that would pass 2^31 - 1 workgroups is refused, not wrapped
    d = (N.ClipDesc * 1)()
    d[0].F, d[0].H, d[0].W = 1 << 12, 1 << 20, 1 << 12
    n = C.c_int(0)
    assert N.lib().vs_clips_plan(d, 1, N.IMAGES_TAIL, 0, 64, 64, 1, None, 0, C.byref(n)) == N.ERR_UNSUPPORTED
    # room for one group only: one is written, the count is still the full one
    arr = (N.ClipDesc * 35)()
    for i in range(35):
        arr[i].F, arr[i].H, arr[i].W = 2, 96, 80
    g = (N.ImagesGroup * 2)()
    g[1].count = -5
    assert N.lib().vs_clips_plan(arr, 35, N.IMAGES_TAIL, 0, S, S, 1, g, 1, C.byref(n)) == 0 and n.value == 2
    assert g[0].count == 32 and g[1].count == -5 and g[0].first_wg[32] == 32 * 2 * cdiv(96, 16)


# ---------------------------------------------------------------------------------------------------------------- packing
PACK_LENGTHS = (1, 2, 3, 4, 5, 9, 0, 17)


def test_spans_and_embed_passes():
    step, ck = 2, 2
    sp = CL.spans(PACK_LENGTHS, step, ck)
    assert all(a % (ck * step) == 0 and 1 <= n <= ck * step and a + n <= PACK_LENGTHS[c] for c, a, n in sp)
    assert all(c != 6 for c, _, _ in sp)                                       # the empty clip takes no slot
    assert sp == sorted(sp)                                                    # list order, clip after clip
    for c, F_ in enumerate(PACK_LENGTHS):                                      # the spans of a clip tile it
        assert sum(n for cc, _, n in sp if cc == c) == F_
    for key_batch in (KEY_BATCH, 8, 3, 1):
        passes = CL.embed_passes(PACK_LENGTHS, step, ck, key_batch) if key_batch != KEY_BATCH else CL.embed_passes(PACK_LENGTHS, step, ck)
        assert [(c, a, n) for slots, _ in passes for c, a, n, _, _ in slots] == sp        # every span once, in list order
        keys_of = {c: [] for c in range(len(PACK_LENGTHS))}
        for slots, rows in passes:
            assert slots
            nk = nf = 0
            for c, a, n, first_frame, first_key in slots:
                assert first_frame == nf and first_key == nk                   # slots are laid out back to back
                k = cdiv(n, step)
                assert rows[nk:nk + k] == [c] * k                              # each key frame's message row is its clip's
                keys_of[c] += [a + j * step for j in range(k)]
                nk, nf = nk + k, nf + n
            assert len(rows) == nk
            assert nk <= key_batch or len(slots) == 1                          # no pass past the batch unless it is a single span
        for c, F_ in enumerate(PACK_LENGTHS):
            assert keys_of[c] == list(range(0, F_, step)), c                   # exactly the key frames of the per-clip call, in order
        # greedy: a pass is closed only before the span that would take it past the batch
        for (slots, rows), (nxt, _) in zip(passes, passes[1:]):
            assert len(rows) + cdiv(nxt[0][2], step) > key_batch
    assert len(CL.embed_passes(PACK_LENGTHS, step, ck)) == 1 and CL.embed_passes([0, 0], step, ck) == [] and CL.embed_passes([], step, ck) == []


def test_detect_passes():
    total = sum(PACK_LENGTHS)
    for det_batch in (DET_BATCH, 8, 5, 1):
        passes = CL.detect_passes(PACK_LENGTHS, det_batch) if det_batch != DET_BATCH else CL.detect_passes(PACK_LENGTHS)
        flat = []
        for slots in passes:
            nf = 0
            for c, a, n, first_frame in slots:
                assert n >= 1 and first_frame == nf and c != 6
                flat += [(c, a + j) for j in range(n)]
                nf += n
            assert 1 <= nf <= det_batch
        assert all(sum(s[2] for s in p) == det_batch for p in passes[:-1])      # only the last run is short
        assert flat == [(c, f) for c, F_ in enumerate(PACK_LENGTHS) for f in range(F_)]      # every frame once, in list order
        assert len(passes) == cdiv(total, det_batch)
    assert CL.detect_passes([0]) == [] and CL.first_rows(PACK_LENGTHS) == [0, 1, 3, 6, 10, 15, 24, 24, 41]
