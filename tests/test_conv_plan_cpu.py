"""The launch rules of the dense layers (csrc/conv_plan.hip: vs_conv_plan, vs_cnx_stage_plan) on the CPU: the library loads without a GPU and
these functions never touch one.

tests/golden/conv_plan.json was written by the PYTHON rules of the commit before they moved into the library (make_golden_conv_plan.py:
recorded from the engine's own launches for every dense layer of the four cards and of the small test architectures, every switch combination,
seeded random shapes around each threshold); every field of every row must be reproduced exactly.  The cases the code comments name are
stated by hand below, so the table cannot be regenerated into agreement with a bug.  The last test walks the same rows through a stand-alone
program that links the unit alone, built with -fsanitize=address,undefined."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from videoseal_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 16        # a non-null "address": the rules read pointers as flags and never dereference them
PTRS = ("a_scale", "in2", "wt_split", "wt_blk", "wt2_blk", "in_pl", "in2_pl", "sumsq_part")
HI = N.CONV_TILE_HI


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as f:
        return json.load(f)


def conv_plan(**kw):
    """vs_conv_plan on a descriptor given by field names (pointer fields as flags; grn_hw / grn_c4 beside them) -> dict of the plan"""
    d = N.ConvDesc()
    grn = kw.pop("grn_hw", 0), kw.pop("grn_c4", 0)
    for k, v in kw.items():
        setattr(d, k, (FAKE if v else None) if k in PTRS else v)
    d.wt2 = FAKE if kw.get("wt2", kw.get("in2") or kw.get("in2_pl")) else None          # a second phase always comes with its weights
    p = N.ConvPlan()
    assert N.lib().vs_conv_plan(C.byref(d), *grn, C.byref(p)) == 0
    return {k: getattr(p, k) for k, _ in N.ConvPlan._fields_}


def stage_plan(rows, HW, Cc, h_ld, pw1_cinp, arith=2, flags=0):
    p = N.CnxStagePlan()
    assert N.lib().vs_cnx_stage_plan(rows, HW, Cc, h_ld, pw1_cinp, arith, flags, C.byref(p)) == 0
    return {k: getattr(p, k) for k, _ in N.CnxStagePlan._fields_}


def gemm(B, H, W, K, n, **kw):
    """a dense 1x1 layer with split weights (pwconv2 with the GRN transform on its A path: a_scale=1, a_scale_ld=K)"""
    return dict(B=B, H=H, W=W, Cin=K, CinP=K, N=n, n_store=n, KH=1, KW=1, SH=1, SW=1, Ho=H, Wo=W, in_sx=K, in_sy=W * K, in_sb=H * W * K,
                wt_split=1, wt_blk=1, **kw)


def conv3(B, H, W, K, n, **kw):
    return dict(B=B, H=H, W=W, Cin=K, CinP=K, N=n, n_store=n, KH=3, KW=3, SH=1, SW=1, PH=1, PW=1, Ho=H, Wo=W, in_sx=K, in_sy=W * K,
                in_sb=H * W * K, wt_split=1, wt_blk=1, **kw)


def test_every_golden_conv_row_is_reproduced(golden):
    cin, cout = golden["conv_in"], golden["conv_out"]
    assert 1500 <= len(golden["conv"]) <= 4000
    for row in golden["conv"]:
        got = conv_plan(**dict(zip(cin, row)))
        assert [got[k] for k in cout] == row[len(cin):], dict(zip(cin + cout, row))


def test_every_golden_stage_row_is_reproduced(golden):
    sin, sout = golden["stage_in"], golden["stage_out"]
    assert 1000 <= len(golden["stage"]) <= 4000
    assert {r[sin.index("flags")] for r in golden["stage"]} == set(range(32))         # every switch combination
    for row in golden["stage"]:
        got = stage_plan(*row[:len(sin)])
        assert [got[k] for k in sout] == row[len(sin):], dict(zip(sin + sout, row))


def test_videoseal_stage3_pwconv2_is_four_slices_on_the_wave_specialised_gemm():
    """32 frames x 8 x 8 = 2048 rows, K = 3072: not on planes, 4 K slices of the wave-specialised GEMM (tile 18: N % 192 == 0), GRN finish folded"""
    sp = stage_plan(2048, 64, 768, 3072, 768)
    assert (sp["pl2"], sp["pw2_narrow"]) == (0, 0)
    p = conv_plan(**gemm(32, 8, 8, 3072, 768, a_scale=1, a_scale_ld=3072), grn_hw=64, grn_c4=3072)
    assert p == dict(routes=N.ROUTE_GEMM_PC, split_k=4, tile_hint=HI | 2, ws_slices=4, grn_fold=1)
    # the development switch that keeps it on planes: 8 slices there
    sp = stage_plan(2048, 64, 768, 3072, 768, flags=N.CNX_NO_PW2_SMALL_PC)
    assert (sp["pl2"], sp["sk2"], sp["tile2"]) == (1, 8, HI | 8)


def test_convnext_base_stage3_is_two_slices_of_2048():
    """K = 4096 with GRN: the 3072 cap applies to the slice the rule picks, not to K"""
    assert stage_plan(2048, 64, 1024, 4096, 1024)["pl2"] == 0
    p = conv_plan(**gemm(32, 8, 8, 4096, 1024, a_scale=1, a_scale_ld=4096), grn_hw=64, grn_c4=4096)
    assert (p["split_k"], p["ws_slices"], p["tile_hint"], p["grn_fold"]) == (2, 2, HI | 1, 1)
    # K = 8192, 4 x 32 blocks: the rule picks 2 slices of 4096 > 3072 -> unsplit (vs_conv_gemm's generic dispatch), no fold
    p = conv_plan(**gemm(8, 8, 8, 8192, 4096, a_scale=1, a_scale_ld=8192), grn_hw=64, grn_c4=8192)
    assert (p["split_k"], p["ws_slices"], p["tile_hint"], p["grn_fold"]) == (1, 0, 0, 0)
    assert conv_plan(**gemm(8, 8, 8, 8192, 4096))["split_k"] == 2          # (no GRN rows: no cap)


def test_stage2_pwconv2_of_the_32_frame_detect_is_tile_26_unsplit():
    """8192 rows, 384 channels, K = 1536: 128 x 96 tiles with the whole K instead of the 2 slices the K-slice rule gives"""
    sp = stage_plan(32 * 256, 256, 384, 1536, 384)
    assert (sp["pl1"], sp["pl2"], sp["pw2_narrow"]) == (1, 0, 1)
    pw2 = gemm(32, 16, 16, 1536, 384, a_scale=1, a_scale_ld=1536)
    assert conv_plan(**pw2, tile_hint=HI | 10, split_k=1, grn_hw=256, grn_c4=1536) == \
        dict(routes=N.ROUTE_GEMM_PC, split_k=1, tile_hint=HI | 10, ws_slices=0, grn_fold=1)
    assert conv_plan(**pw2, grn_hw=256, grn_c4=1536)["split_k"] == 2
    assert stage_plan(32 * 256, 256, 384, 1536, 384, flags=N.CNX_NO_PW2_NARROW)["pw2_narrow"] == 0
    assert stage_plan(32 * 256, 256, 384, 1536, 384, arith=3) == dict(pl1=0, pl2=0, sk2=1, tile1=HI | 8, tile2=HI | 8, pw2_narrow=0)
    # 17 partial rows per frame do not fit the fold
    assert conv_plan(**gemm(8, 17, 32, 1536, 384, a_scale=1, a_scale_ld=1536), tile_hint=HI | 10, grn_hw=17 * 32, grn_c4=1536)["grn_fold"] == 0


def test_a_3x3_layer_with_sumsq_part_is_never_sliced():
    wide = conv3(4, 32, 32, 384, 384)          # 4 key frames: 64 workgroups -> 3 slices of 8 chunks
    assert conv_plan(**wide) == dict(routes=N.ROUTE_PATCH | N.ROUTE_PATCH_PC, split_k=3, tile_hint=HI | 0, ws_slices=3, grn_fold=0)
    assert conv_plan(**wide, sumsq_part=1)["split_k"] == 1
    assert conv_plan(**wide, sumsq_part=1, split_k=4)["split_k"] == 1
    assert conv_plan(**gemm(32, 8, 8, 3072, 768), sumsq_part=1)["split_k"] == 1


def test_a_second_phase_on_the_patch_kernel_takes_one_more_workspace_slice():
    two = conv3(4, 32, 32, 256, 256, in2=1, Cin2P=256, wt2_blk=1)      # 64 workgroups, 16 chunks: 2 -> 128, 4 -> 256 workgroups
    p = conv_plan(**two)
    assert p["split_k"] == 4 and p["ws_slices"] == 5 and p["tile_hint"] == 15
    assert conv_plan(**conv3(4, 32, 32, 256, 256))["ws_slices"] == 4
    # a host that only counts workspace has the second phase's weights but no activations yet: the same plan
    assert conv_plan(**conv3(4, 32, 32, 256, 256, Cin2P=256, wt2_blk=1, wt2=1)) == p
    # the planes chain brings its own slice count and tile 22: kept, workspace still sized here
    pl = conv3(4, 32, 32, 384, 384, in_pl=1, in2_pl=1, Cin2P=384, wt2_blk=1, tile_hint=HI | 6, split_k=6)
    assert conv_plan(**pl) == dict(routes=N.ROUTE_PATCH | N.ROUTE_PATCH_PC, split_k=6, tile_hint=HI | 6, ws_slices=7, grn_fold=0)
    # a caller's tile hint without a slice count: unsplit
    assert conv_plan(**conv3(4, 32, 32, 256, 256), tile_hint=15)["split_k"] == 1


def test_thresholds_of_the_k_slice_rules():
    """256 workgroups of 128 x 128 (1x1), 192 of the patch kernel, >= 4 K pairs resp. >= 2 chunks per slice"""
    assert conv_plan(**gemm(32, 8, 8, 768, 2048))["split_k"] == 1           # 16 x 16 = 256 blocks
    assert conv_plan(**gemm(32, 8, 8, 768, 2047))["split_k"] == 1           # (2047 -> 16 column tiles as well)
    assert conv_plan(**gemm(32, 8, 8, 768, 1920))["split_k"] == 2           # 240 blocks
    assert conv_plan(**gemm(1, 8, 8, 256, 128))["split_k"] == 2             # 8 pairs: a slice keeps >= 4
    assert conv_plan(**gemm(1, 8, 8, 224, 128))["split_k"] == 1             # 7 pairs: odd
    assert conv_plan(**gemm(1, 8, 8, 240, 128))["routes"] == 0              # Cin % 32 != 0: not this kernel
    assert conv_plan(**conv3(6, 32, 32, 384, 384))["split_k"] == 2          # 96 workgroups
    assert conv_plan(**conv3(12, 32, 32, 384, 384))["split_k"] == 1         # 192
    assert conv_plan(**conv3(1, 32, 32, 128, 128))["split_k"] == 4          # 8 chunks: candidates 2, 4 (3, 6 do not divide; 8 leaves one chunk)
    assert conv_plan(**conv3(1, 32, 32, 112, 128))["split_k"] == 1          # CinP < 128
    thin = conv3(2, 24, 40, 16, 32)
    assert conv_plan(**thin)["routes"] == N.ROUTE_SMALL                      # (W % 16 != 0: no patch route)


def test_bad_arguments_and_struct_sizes():
    L = N.lib()
    assert L.vs_conv_plan(None, 0, 0, C.byref(N.ConvPlan())) == -1 and L.vs_conv_plan(C.byref(N.ConvDesc()), 0, 0, None) == -1
    assert L.vs_cnx_stage_plan(1, 1, 1, 1, 1, 2, 0, None) == -1
    assert L.vs_sizeof_conv_plan() == C.sizeof(N.ConvPlan) and L.vs_sizeof_cnx_stage_plan() == C.sizeof(N.CnxStagePlan)


def test_plan_unit_alone_under_address_and_ub_sanitizers(golden, tmp_path):
    """tests/conv_plan_walk.cpp + csrc/conv_plan.hip compiled as plain C++ with -fsanitize=address,undefined (no GPU code in the unit, nothing
    loaded into Python): every golden row again, and no report from either sanitizer"""
    rows = tmp_path / "rows.txt"
    rows.write_text("".join("c " + " ".join(map(str, r)) + "\n" for r in golden["conv"]) +
                    "".join("s " + " ".join(map(str, r)) + "\n" for r in golden["stage"]))
    exe = tmp_path / "conv_plan_walk"
    cc = shutil.which("hipcc") or "hipcc"
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "videoseal_amd", "csrc"),
                    os.path.join(ROOT, "videoseal_amd", "csrc", "conv_plan.hip"), os.path.join(ROOT, "tests", "conv_plan_walk.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
