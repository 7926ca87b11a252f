"""Lists of images of different sizes on the CPU: the three entry points are listed, declared and built, and the launch plan both launchers
walk (csrc/images_plan.h, exported as vs_images_plan) is checked against a Python restatement of its rules -- the library loads without a GPU
and the planner never touches one.  The last test walks the same lists through a stand-alone program that links the unit alone, built with
-fsanitize=address,undefined (nothing sanitized is loaded into Python)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from videoseal_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = N.IMAGES_PER_LAUNCH
f32 = np.float32

# the sizes of the kernel tests (tests/test_gpu_images.py): the smallest shapes at which each code path can go wrong
SIZES = [(5, 7), (48, 40), (64, 64), (9, 300), (130, 33), (192, 200), (256, 256), (257, 191), (400, 70)]
RNG = np.random.RandomState(7)
LISTS = {
    "table": SIZES,
    "reversed": SIZES[::-1],
    "35 images": (SIZES * 4)[:35],
    "35 of one size": [(192, 200)] * 35,
    "32 of one size": [(96, 80)] * 32,
    "33 of one size": [(96, 80)] * 33,
    "one": [(130, 33)],
    "none": [],
    "64 beside 2048": [(64, 64), (2048, 2048)],
    "seeded": [(int(h), int(w)) for h, w in RNG.randint(1, 1100, size=(70, 2))],
}


# ---- the rules, restated (resize_pick.h::rs_pick in float32, images_plan.h)
def rs_pick(H, W, oh, ow, aa):
    sx, sy = f32(W) / f32(ow), f32(H) / f32(oh)
    supx = max(sx, f32(1)) if aa else f32(1)
    supy = max(sy, f32(1)) if aa else f32(1)
    for OW, INW, MT, RING in ((128, 448, 8, 16), (64, 288, 10, 32)):
        if f32(2) * supx + f32(2) <= f32(MT) and f32(2) * supy + f32(2) <= f32(MT) and \
                f32(OW) * sx + f32(2) * supx + f32(4) + f32(3) <= f32(INW) and f32(2) * supy + f32(2) + f32(8) <= f32(RING):
            return OW
    return 0


def form_of(kind, u8, H, W, oh, ow, aa):
    if kind == N.IMAGES_RESIZE and not u8:
        return {128: N.IMAGES_FORM_STREAM128, 64: N.IMAGES_FORM_STREAM64, 0: N.IMAGES_FORM_TILE}[rs_pick(H, W, oh, ow, aa)]
    return N.IMAGES_FORM_TILE


def cdiv(a, b):
    return (a + b - 1) // b


def plan_ref(sizes, kind, u8, oh, ow, aa):
    out = []
    for form in (N.IMAGES_FORM_TILE, N.IMAGES_FORM_STREAM128, N.IMAGES_FORM_STREAM64):
        idx = [i for i, (H, W) in enumerate(sizes) if form_of(kind, u8, H, W, oh, ow, aa) == form]
        for a in range(0, len(idx), PER):
            grp = idx[a:a + PER]
            strip = 0
            if kind == N.IMAGES_RESIZE and form != N.IMAGES_FORM_TILE:
                OW = 128 if form == N.IMAGES_FORM_STREAM128 else 64
                strip = next((c for c in (64, 48, 32, 24, 16) if cdiv(ow, OW) * cdiv(oh, c) * len(grp) >= 512), 32)
            first = [0]
            for i in grp:
                H, W = sizes[i]
                if kind == N.IMAGES_TAIL:
                    t = cdiv(W, 256) * cdiv(H, 16)
                elif form == N.IMAGES_FORM_TILE:
                    t = cdiv(ow, 32) * cdiv(oh, 8)
                else:
                    t = cdiv(ow, OW) * cdiv(oh, strip)
                first.append(first[-1] + t)
            out.append((form, strip, grp, first))
    return out


CASES = [(name, kind, u8, S, aa) for name in LISTS for kind in (N.IMAGES_RESIZE, N.IMAGES_TAIL) for u8 in (False, True)
         for S in (64, 256) for aa in (True, False)]


def test_the_three_symbols_are_listed_declared_and_built():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    lib = N.lib()
    for sym in ("vs_resize_pre_images", "vs_embed_tail_images", "vs_images_plan"):
        assert sym in N.EXPORTS and re.search(r"\bint " + sym + r"\(", header) and hasattr(lib, sym), sym
    m = re.search(r"#define VS_IMAGES_PER_LAUNCH (\d+)", header)
    assert m and int(m.group(1)) == PER and PER >= 32
    # argument validation happens on the host before any launch: refused without a GPU
    n = C.c_int(-1)
    assert lib.vs_resize_pre_images(None, 1, 0, 64, 64, 1, None, 1.0, 0.0, None, None, None) == -1
    assert lib.vs_embed_tail_images(None, None) == -1
    assert lib.vs_images_plan(None, 1, 0, 0, 64, 64, 1, None, 0, C.byref(n)) == -1
    assert lib.vs_images_plan(None, 0, 0, 0, 64, 64, 1, None, 0, None) == -1
    assert lib.vs_images_plan(None, 0, 7, 0, 64, 64, 1, None, 0, C.byref(n)) == -1
    d = (N.ImageDesc * 1)()
    assert lib.vs_images_plan(d, 1, 0, 0, 64, 64, 1, None, 0, C.byref(n)) == -1          # H = W = 0
    assert lib.vs_images_plan(None, 0, 0, 0, 64, 64, 1, None, 0, C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("name", list(LISTS))
def test_plan_equals_the_restated_rules(name):
    sizes = LISTS[name]
    for _, kind, u8, S, aa in (c for c in CASES if c[0] == name):
        assert N.images_plan(sizes, kind, u8, S, S, aa) == plan_ref(sizes, kind, u8, S, S, aa), (name, kind, u8, S, aa)


@pytest.mark.parametrize("name", list(LISTS))
def test_every_tile_once_no_empty_workgroup_and_bounded_groups(name):
    """stated on the plan alone (not through the restatement): a workgroup w of a launch belongs to the image k with first_wg[k] <= w <
    first_wg[k + 1] and is tile w - first_wg[k] of it"""
    sizes = LISTS[name]
    for _, kind, u8, S, aa in (c for c in CASES if c[0] == name):
        plan = N.images_plan(sizes, kind, u8, S, S, aa)
        seen = {}
        for form, strip, image, first in plan:
            assert 1 <= len(image) <= PER and len(first) == len(image) + 1 and first[0] == 0
            assert image == sorted(image)                                    # list order inside a group
            for k, i in enumerate(image):
                H, W = sizes[i]
                if kind == N.IMAGES_TAIL:
                    tiles = cdiv(W, 256) * cdiv(H, 16)
                elif form == N.IMAGES_FORM_TILE:
                    tiles = cdiv(S, 32) * cdiv(S, 8)
                else:
                    assert strip >= 1 and not u8 and rs_pick(H, W, S, S, aa) == (128 if form == N.IMAGES_FORM_STREAM128 else 64)
                    tiles = cdiv(S, 128 if form == N.IMAGES_FORM_STREAM128 else 64) * cdiv(S, strip)
                assert first[k + 1] - first[k] == tiles >= 1, (name, i)      # exactly the image's tiles: none missing, none empty
                assert i not in seen
                seen[i] = form
        assert sorted(seen) == list(range(len(sizes)))                       # every image in exactly one launch
        # launches: ceil(images of a form / PER) summed over the forms present -- never a function of n itself
        per_form = {}
        for f in seen.values():
            per_form[f] = per_form.get(f, 0) + 1
        assert len(plan) == sum(cdiv(c, PER) for c in per_form.values())


def test_group_counts_at_the_launch_limit():
    S = 64
    for n, groups in ((0, 0), (1, 1), (32, 1), (33, 2), (35, 2), (64, 2), (65, 3)):
        plan = N.images_plan([(96, 80)] * n, N.IMAGES_TAIL, False, S, S, True)
        assert len(plan) == groups and [len(g[2]) for g in plan] == [min(PER, n - a) for a in range(0, n, PER)]
    # a 64^2 picture beside a 2048^2 one: 4 + 1024 workgroups, not a rectangle of 2 x 1024
    (_, _, image, first), = N.images_plan([(64, 64), (2048, 2048)], N.IMAGES_TAIL, False, 256, 256, True)
    assert image == [0, 1] and first == [0, 4, 4 + 8 * 128]
    # a launch that would pass 2^31 - 1 workgroups is refused, not wrapped
    d = (N.ImageDesc * 2)()
    for i in range(2):
        d[i].H, d[i].W = 1 << 24, 1 << 19
    n = C.c_int(0)
    assert N.lib().vs_images_plan(d, 2, N.IMAGES_TAIL, 0, 64, 64, 1, None, 0, C.byref(n)) == N.ERR_UNSUPPORTED


def test_ctypes_mirrors_match_the_header():
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    for name, cls in (("vs_image_desc", N.ImageDesc), ("vs_tail_images_desc", N.TailImagesDesc), ("vs_images_group", N.ImagesGroup)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + "_t;", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        body = re.sub(r"\[[^\]]*\]", "", body)                                # array extents
        members = [m.strip().split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()
                   for m in re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip()).split(",")]
        assert members == [f for f, _ in cls._fields_], (name, members)


def test_plan_unit_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/images_plan_walk.cpp + csrc/images_plan.hip compiled as plain C++ with -fsanitize=address,undefined: every list again, the plans it
    prints equal the restated rules, and no report from either sanitizer"""
    lists = tmp_path / "lists.txt"
    lists.write_text("".join(f"{kind} {int(u8)} {S} {S} {int(aa)} {len(LISTS[name])} " + " ".join(f"{h} {w}" for h, w in LISTS[name]) + "\n"
                             for name, kind, u8, S, aa in CASES))
    exe = tmp_path / "images_plan_walk"
    cc = shutil.which("hipcc") or "hipcc"
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "videoseal_amd", "csrc"),
                    os.path.join(ROOT, "videoseal_amd", "csrc", "images_plan.hip"), os.path.join(ROOT, "tests", "images_plan_walk.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(lists)], capture_output=True, text=True)
    assert r.returncode == 0 and f"{len(CASES)} lists, 0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-2000:])
    got, cur = [], None
    for ln in r.stdout.splitlines():
        if ln.startswith("list "):
            cur = []
            got.append(cur)
        elif ln.startswith("g "):
            head, image, first = ln[2:].split("|")
            form, strip, count = map(int, head.split())
            image, first = list(map(int, image.split())), list(map(int, first.split()))
            assert len(image) == count
            cur.append((form, strip, image, first))
    assert got == [plan_ref(LISTS[name], kind, u8, S, S, aa) for name, kind, u8, S, aa in CASES]
