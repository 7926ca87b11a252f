"""The two switch tables without a GPU: key numbers and environment seeding of the library's development switches (csrc/vs_common.h,
csrc/api.hip) through ctypes, and the engine's table of environment flags (videoseal_amd/switches.py, engine.ENGINE_SWITCHES)."""
import os
import re
import subprocess
import sys

import pytest

from videoseal_amd import native, switches
from videoseal_amd.engine import ENGINE_SWITCHES, engine_switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_KEYS = ["RESIZE_FORM", "RESIZE_STRIP", "TAIL_STRIP", "JPEG_FORM", "CROP_RESIZE_FORM", "TO_PLANES_FORM", "DWCONV_ROWS", "LN_FORM", "SPLITK_EPI",
            "UPCONV_FORM"]


def test_the_ten_old_keys_keep_their_numbers_and_the_header_lists_every_key():
    lib = native.lib()
    assert [lib.vs_debug_key(n.encode()) for n in OLD_KEYS] == list(range(10))
    header = open(os.path.join(ROOT, "include", "videoseal_hip.h")).read()
    listed = re.findall(r"^ \*\s+(\d+) ([A-Z0-9_]+)\s+(-|(?:VIDEOSEAL|VS)_[A-Z0-9_]+)", header, re.M)
    common = open(os.path.join(ROOT, "videoseal_amd", "csrc", "vs_common.h")).read()
    rows = re.findall(r'^\s*X\((\w+), (?:"(\w+)"|nullptr), ', common, re.M)
    assert [(int(k), n, e) for k, n, e in listed] == [(k, n, e or "-") for k, (n, e) in enumerate(rows)]
    assert [lib.vs_debug_key(n.encode()) for n, _ in rows] == list(range(len(rows)))
    assert lib.vs_debug_key(b"NO_SUCH_KEY") == -1 and lib.vs_debug_key(b"VS_DBG_RESIZE_FORM") == -1 and lib.vs_debug_key(None) == -1


_CHILD = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
key = lambda n: L.vs_debug_key(n.encode())
get = lambda n: L.vs_debug_get(key(n))
# seeded from the environment, each under the variable's own rule
assert get("RESIZE_FORM") == 1, get("RESIZE_FORM")
assert get("TAIL_STRIP") == 40
assert get("RESIZE_STRIP") == 0                   # VS_RESIZE_STRIP=1 is below the variable's threshold of 2: ignored, as it always was
assert get("ARITH") == 3 and get("WGRAD") == 2
for n in ("JPEG_FORM", "CROP_RESIZE_FORM", "TO_PLANES_FORM", "DWCONV_ROWS", "LN_FORM", "SPLITK_EPI", "UPCONV_FORM", "TAIL_FORM", "VIT_ATTN", "DWCONV",
          "GEMM_GRID", "GEMM_PL_RASTER", "CNX_PIPE", "CNX_ABL", "UPCONV_ABL", "STEM_FUSED"):
    assert get(n) == 0, n
# an override wins, and resetting it returns to the environment default, not to the library's choice
for n, v, seeded in (("RESIZE_FORM", 2, 1), ("TAIL_STRIP", 8, 40), ("RESIZE_STRIP", 1, 0), ("WGRAD", 1, 2), ("ARITH", 2, 3), ("LN_FORM", 1, 0)):
    assert L.vs_debug_set(key(n), v) == 0 and get(n) == v, n
    assert get("TAIL_STRIP") == (8 if n == "TAIL_STRIP" else 40)           # ... and touches no other key
    assert L.vs_debug_set(key(n), 0) == 0 and get(n) == seeded, n
# the environment is read once: a later change of the variable is not seen
import os
os.environ["VS_TAIL_STRIP"] = "48"
assert get("TAIL_STRIP") == 40
# unknown names and keys out of range
assert key("VS_TAIL_STRIP") == -1 and key("") == -1
for bad in (-1, key("ARITH") + 1, 1 << 20):                                # ARITH is the last key
    assert L.vs_debug_get(bad) == -1 and L.vs_debug_set(bad, 1) == -1, bad
print("switches ok")
"""


def test_environment_defaults_are_seeded_once_and_survive_a_reset_of_the_key():
    """one fresh CPU-only process (ctypes, no torch): the seeded values, override, fall-back of vs_debug_set(key, 0), unknown names / keys"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("VS_", "VIDEOSEAL_"))}
    env.update(VIDEOSEAL_RESIZE="tile", VS_TAIL_STRIP="40", VS_RESIZE_STRIP="1", VIDEOSEAL_CONV="bf16x3", VS_WGRAD="fma")
    r = subprocess.run([sys.executable, "-c", _CHILD, native.LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "switches ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# what HipEngine.__init__ computed from os.environ before the table existed, written out: attribute -> expression of e = the environment
PARENT = {
    "per_layer_arith": lambda e: e.get("VIDEOSEAL_LAYER_ARITH", "1") != "0",
    "upconv_lowres": lambda e: e.get("VIDEOSEAL_UPCONV", "lowres") != "direct",
    "upconv_fused": lambda e: e.get("VIDEOSEAL_UPCONV", "lowres") != "unfused",
    "msg_table_conv": lambda e: e.get("VIDEOSEAL_MSG_TABLE", "1") != "0",
    "planes_chain": lambda e: e.get("VIDEOSEAL_PLANES", "1") != "0",
    "msg0_planes": lambda e: e.get("VIDEOSEAL_MSG0_PLANES", "1") != "0",
    "gemm_big": lambda e: e.get("VIDEOSEAL_GEMM_BIG", "0") == "1",
    "stem_fused": lambda e: e.get("VIDEOSEAL_STEM_FUSED", "0") == "1",
    "down_patch": lambda e: e.get("VIDEOSEAL_DOWN_PATCH", "1") != "0",
    "grn_straddle": lambda e: e.get("VIDEOSEAL_GRN_STRADDLE", "1") != "0",
    "grn_fold": lambda e: e.get("VIDEOSEAL_GRN_FOLD", "1") != "0",
    "pw2_narrow": lambda e: e.get("VIDEOSEAL_PW2_NARROW", "1") != "0",
    "pw2_small_pc": lambda e: e.get("VIDEOSEAL_PW2_SMALL_PC", "1") != "0",
    "planes_gemm": lambda e: e.get("VIDEOSEAL_PLANES", "1") != "0",
    "fused_blocks": lambda e: e.get("VIDEOSEAL_CNX_FUSED", "1") != "0",
    "thin_fused": lambda e: e.get("VIDEOSEAL_THIN_FUSED", "1") != "0",
    "planes_splitk": lambda e: e.get("VIDEOSEAL_PLANES_SPLITK", "1") != "0",
    "check_finite": lambda e: e.get("VIDEOSEAL_CHECK_FINITE", "0") == "1",
    "autotune": lambda e: e.get("VIDEOSEAL_AUTOTUNE", "1") != "0",
}


def test_engine_switch_table_equals_the_expressions_it_replaced():
    assert [a for a, _, _ in ENGINE_SWITCHES] == list(PARENT) and len({a for a, _, _ in ENGINE_SWITCHES}) == len(ENGINE_SWITCHES)
    names = sorted({n for _, n, _ in ENGINE_SWITCHES})
    assert all(n in switches.REGISTRY for n in names)
    fed = {n: [a for a, m, _ in ENGINE_SWITCHES if m == n] for n in names}
    assert fed["VIDEOSEAL_UPCONV"] == ["upconv_lowres", "upconv_fused"] and fed["VIDEOSEAL_PLANES"] == ["planes_chain", "planes_gemm"]
    assert all(len(v) == 1 for n, v in fed.items() if n not in ("VIDEOSEAL_UPCONV", "VIDEOSEAL_PLANES"))
    envs = [{}] + [{n: v} for n in names for v in ("0", "1", "", "2", "direct", "unfused", "lowres")]
    for env in envs:
        assert engine_switches(env) == {a: f(env) for a, f in PARENT.items()}, env
    # defaults, and each variable flipped
    d = engine_switches({})
    assert d == {a: a not in ("gemm_big", "stem_fused", "check_finite") for a in PARENT}
    for attr, name, default in ENGINE_SWITCHES:
        flip = default if isinstance(default, str) else ("0" if default else "1")
        got = engine_switches({name: flip})
        assert got[attr] is (not d[attr]), (attr, name)
        assert {a for a in got if got[a] != d[a]} <= set(fed[name])
    assert engine_switches({"VIDEOSEAL_PLANES": "0"})["planes_chain"] is False and engine_switches({"VIDEOSEAL_PLANES": "0"})["planes_gemm"] is False
    assert engine_switches({"VIDEOSEAL_UPCONV": "direct"}) == dict(d, upconv_lowres=False)
    assert engine_switches({"VIDEOSEAL_UPCONV": "unfused"}) == dict(d, upconv_fused=False)


def test_readers_refuse_an_unregistered_name_and_read_at_call_time(monkeypatch):
    for reader, args in ((switches.flag, (True,)), (switches.choice, ("a",)), (switches.integer, (0,)), (switches.path, ())):
        with pytest.raises(KeyError):
            reader("VIDEOSEAL_NO_SUCH_SWITCH", *args)
    monkeypatch.delenv("VIDEOSEAL_GRAPHS", raising=False)
    assert switches.flag("VIDEOSEAL_GRAPHS", False) is False
    monkeypatch.setenv("VIDEOSEAL_GRAPHS", "1")
    assert switches.flag("VIDEOSEAL_GRAPHS", False) is True                      # nothing is cached
    assert switches.integer("VIDEOSEAL_PLANES_SK", 0, {"VIDEOSEAL_PLANES_SK": "3"}) == 3 and switches.integer("VIDEOSEAL_PLANES_SK", 0, {}) == 0
    assert switches.path("VIDEOSEAL_TILE_CACHE", {}) is None and switches.path("VIDEOSEAL_TILE_CACHE", {"VIDEOSEAL_TILE_CACHE": "/x.json"}) == "/x.json"
    assert switches.choice("VIDEOSEAL_CODEC", "proxy", ("proxy", "pyav"), {}) == "proxy"
    with pytest.raises(ValueError, match="VIDEOSEAL_CODEC='x264': expected 'proxy' or 'pyav'"):
        switches.choice("VIDEOSEAL_CODEC", "proxy", ("proxy", "pyav"), {"VIDEOSEAL_CODEC": "x264"})
