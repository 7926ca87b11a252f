#!/usr/bin/env python
"""Golden table of the dense-layer launch rules, written by the PYTHON rules of the commit BEFORE they moved into the library.

    git checkout d40517b && make -C videoseal_amd/csrc          # the parent of the commit that added vs_conv_plan / vs_cnx_stage_plan
    VIDEOSEAL_AUTOTUNE=0 python tests/golden/make_golden_conv_plan.py      # no GPU needed; writes tests/golden/conv_plan.json

It runs AT THAT COMMIT ONLY: it calls HipEngine._gemm_pc_ok / _patch_pc_ok / _split_k_rule / _split_k_rule_patch / _static_split_tile,
which exist nowhere later.  tests/test_conv_plan_cpu.py asks the library for the same rows and demands equal fields.

Two sources of rows:
  * RECORDED: the real HipEngine of every card (and of the small test architectures) runs embedder_forward / extractor_forward on
    meta tensors against a library stand-in that records every vs_conv_gemm descriptor: what engine.conv decided (split_k, tile_hint,
    the size of splitk.ws, whether the GRN finish rode along) is read off the launch, not recomputed.  Batches: 32 (image / detect), 8 and 4
    key frames (32-frame video at step 4 / 8, the 16-frame stream chunk), 16 (ChunkySeal detect, the stream chunk), 1 2 3 6 (the small tests).
  * FUNCTIONS: `conv_decision` / `stage_plan` below restate engine.conv's decision path and _extractor_forward's stage planning as
    functions of a row (they call the engine's own rule methods); every recorded launch must agree with them (asserted here), then they
    are evaluated on every switch combination and on seeded random shapes around each threshold.
"""
import itertools
import json
import os
import random
import sys

os.environ["VIDEOSEAL_AUTOTUNE"] = "0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch                                                              # noqa: E402
from oracle.weights import legacy_tiny_spec, spec_from_card, state_dict_layout, tiny_spec   # noqa: E402
from tests._model import cfg_of                                           # noqa: E402
from videoseal_amd import engine as E, native as N                       # noqa: E402

META = torch.device("meta")
FAKE = 1 << 16        # a non-null, 16-byte aligned "address": the rules read pointers as flags only
CONV_IN = ["B", "H", "W", "Cin", "KH", "KW", "SH", "SW", "PH", "PW", "Ho", "Wo", "CinP", "N", "n_store", "Cin2P", "in_sb", "in_sy", "in_sx",
           "a_scale_ld", "a_scale", "in2", "wt_split", "wt_blk", "wt2_blk", "in_pl", "in2_pl", "sumsq_part", "tile_hint", "split_k", "grn_hw", "grn_c4"]
CONV_OUT = ["routes", "split_k", "tile_hint", "ws_slices", "grn_fold"]
STAGE_IN = ["rows", "HW", "C", "h_ld", "pw1_cinp", "arith", "flags"]
STAGE_OUT = ["pl1", "pl2", "sk2", "tile1", "tile2", "pw2_narrow"]
PTRS = ("a_scale", "in2", "wt_split", "wt_blk", "wt2_blk", "in_pl", "in2_pl", "sumsq_part")
ROUTE_GEMM_PC, ROUTE_PATCH, ROUTE_PATCH_PC, ROUTE_SMALL = 1, 2, 4, 8
# vs_cnx_stage_plan flags: 0 = the shipped defaults
NO_PLANES_GEMM, NO_PW2_SMALL_PC, NO_PW2_NARROW, GEMM_BIG, NO_SPLIT = 1, 2, 4, 8, 16


class Switches:
    """the engine attributes the stage planning reads"""
    def __init__(self, flags, arith):
        self.planes_gemm, self.pw2_small_pc, self.pw2_narrow = not flags & NO_PLANES_GEMM, not flags & NO_PW2_SMALL_PC, not flags & NO_PW2_NARROW
        self.gemm_big, self.use_split, self.arith = bool(flags & GEMM_BIG), not flags & NO_SPLIT, arith

    _gemm_planes_ok = E.HipEngine._gemm_planes_ok


def desc_of(row):
    d = N.ConvDesc()
    for k in CONV_IN[:20]:
        setattr(d, k, row[k])
    for k in PTRS:
        setattr(d, k, FAKE if row[k] else None)
    d.inp = d.wt = d.out = FAKE
    d.wt2 = FAKE if (row["in2"] or row["in2_pl"]) else None      # (engine.conv sets wt2 whenever it is given `in2`)
    d.tile_hint, d.split_k = row["tile_hint"], row["split_k"]
    return d


def routes_of(d):
    """_gemm_pc_ok, _patch_pc_ok and the locals `patch` / `small` of _pick_tile"""
    H = E.HipEngine
    patch = (bool(d.wt_split) and d.KH == 3 and d.KW == 3 and d.SH == 1 and d.SW == 1 and d.PH == 1 and d.PW == 1 and
             d.Ho == d.H and d.Wo == d.W and not d.a_scale and d.W % 16 == 0 and d.H % 8 == 0)
    small = (bool(d.wt_split) and d.KH == 3 and d.KW == 3 and d.SH == 1 and d.SW == 1 and d.PH == 1 and d.PW == 1 and d.Ho == d.H
             and d.Wo == d.W and not d.a_scale and d.CinP == 16 and d.N <= 32 and d.n_store <= 32 and (not d.in2 or d.Cin2P == 16)
             and d.split_k <= 1 and not d.sumsq_part)
    return ((ROUTE_GEMM_PC if H._gemm_pc_ok(d) else 0) | (ROUTE_PATCH if patch else 0) | (ROUTE_PATCH_PC if H._patch_pc_ok(d) else 0) |
            (ROUTE_SMALL if small else 0))


def conv_decision(row):
    """engine.conv from `if sumsq is not None` to the fold test, autotune off and grn_fold switched on (row["split_k"] == 0: the caller
    left it None; row["grn_hw"] == 0: no grn_fold argument)"""
    H = E.HipEngine
    d = desc_of(row)
    routes = routes_of(d)
    tile_hint, split_k = row["tile_hint"], (row["split_k"] or None)
    if d.sumsq_part:
        split_k = 1
    patch_pc = H._patch_pc_ok(d)
    if split_k is None:
        split_k = 1
        if tile_hint == 0 and H._gemm_pc_ok(d):
            sk = H._split_k_rule(d)
            if not d.a_scale or d.CinP // sk <= 3072:
                split_k = sk
        elif tile_hint == 0 and patch_pc:
            split_k = H._split_k_rule_patch(d)
    slices = 0
    if split_k > 1:
        slices = split_k + (1 if ((patch_pc or d.in_pl) and (d.in2 or d.in2_pl)) else 0)
        d.split_k = split_k
        if tile_hint == 0:
            d.tile_hint = H._static_split_tile(d)
    fold = 0
    if row["grn_hw"]:
        HW_, C4 = row["grn_hw"], row["grn_c4"]
        pc_tile = (d.tile_hint & 0xf) + (16 if d.tile_hint & N.CONV_TILE_HI else 0)
        fold = int(pc_tile in (17, 18, 26) and HW_ % 32 == 0 and HW_ // 32 <= 16 and d.CinP == d.a_scale_ld == C4)
    return dict(routes=routes, split_k=split_k, tile_hint=d.tile_hint, ws_slices=slices, grn_fold=fold)


def stage_plan(row):
    """_extractor_forward from `pw1w = ...` to `ptile2 = ...`, and the tile-26 test of its pwconv2 branch (cur.rows -> rows, hh.ld -> h_ld,
    pw1w.CinP -> pw1_cinp, a2 -> the network's arithmetic)"""
    self = Switches(row["flags"], row["arith"])
    rows, HW, Cc, h_ld = row["rows"], row["HW"], row["C"], row["h_ld"]
    pl1 = self._gemm_planes_ok(rows, 4 * Cc) and row["pw1_cinp"] % 16 == 0
    pl2, sk2 = False, 1
    if self.planes_gemm and self.use_split and self.arith == 2 and h_ld >= 2048 and h_ld % 16 == 0:
        tiles2 = ((rows + 255) // 256) * ((Cc + 191) // 192)
        steps2 = h_ld // 16
        while tiles2 * sk2 < 200 and steps2 // (sk2 * 2) >= 24 and steps2 % (sk2 * 2) == 0:
            sk2 *= 2
        pl2 = tiles2 * sk2 >= 128
        if pl2 and rows <= 2048 and HW % 64 == 0 and h_ld % 32 == 0 and self.pw2_small_pc:
            skp = 1
            blocks = ((rows + 127) // 128) * ((Cc + 127) // 128)
            pairs = h_ld // 32
            while blocks * skp < 256 and pairs % (skp * 2) == 0 and pairs // (skp * 2) >= 4:
                skp *= 2
            if h_ld // skp <= 3072:
                pl2 = False
    elif (self.planes_gemm and self.use_split and self.arith == 2 and h_ld % 16 == 0 and HW % 64 != 0
          and ((rows + 255) // 256) * ((Cc + 191) // 192) >= 200):
        pl2, sk2 = True, 1
    ptile = N.CONV_TILE_HI | 8
    big1 = self.gemm_big and pl1 and ((rows + 255) // 256) * ((4 * Cc + 255) // 256) >= 3 * 256
    big2 = self.gemm_big and pl2 and sk2 == 1 and ((rows + 255) // 256) * ((Cc + 255) // 256) >= 3 * 256
    # the pwconv2 launch takes the tile-26 form in the branch `not pl2 and HW % 64 == 0` only
    narrow = (not pl2 and HW % 64 == 0 and
              self.pw2_narrow and self.use_split and self.arith == 2 and ((rows + 127) // 128) * ((Cc + 127) // 128) < 256
              and ((rows + 127) // 128) * ((Cc + 95) // 96) >= 200 and Cc % 96 == 0 and HW >= 128
              and h_ld <= 3072 and h_ld % 32 == 0 and h_ld == 4 * Cc)
    return dict(pl1=int(bool(pl1)), pl2=int(pl2), sk2=sk2, tile1=(N.CONV_TILE_HI | 11) if big1 else ptile,
                tile2=(N.CONV_TILE_HI | 11) if big2 else ptile, pw2_narrow=int(bool(narrow)))


# ---------------------------------------------------------------------------------------------- the recorder
def _with_split(self, arith=3):          # (weights on the meta device: the operand planes exist as flags only)
    if self.split is None or self.arith != arith:
        self.arith, self.w_mul = arith, 1.0
        self.split = self.blk = torch.empty(1, dtype=torch.int16, device=META)
    return self


class Recorder:
    """stands in for the shared library: host-only queries go to the real one, conv launches are recorded, every other launch is a no-op"""
    def __init__(self, real):
        self.real, self.launches = real, []

    def __getattr__(self, name):
        if name.endswith(("_supported", "_preferred", "_bytes", "_floats", "_doubles")):
            return getattr(self.real, name)
        if name == "vs_conv_gemm":
            return lambda dref, st: self.launches.append({f: getattr(dref._obj, f) for f, _ in N.ConvDesc._fields_}) or 0
        return lambda *a: 0


def make_engine(spec, flags=0, arith=2):
    N.ptr = lambda t: None if t is None else FAKE
    N.stream = lambda: 0
    torch.cuda.is_current_stream_capturing = lambda: False
    E.ConvW.with_split = E.ConvW.with_blk = _with_split
    E.pack_cnx_block = lambda w1, b1, w2, beta, dev: (torch.empty(1, dtype=torch.uint8, device=META), 1.0, 1.0)
    E.HipEngine._pack_misc = lambda self: None
    E.HipEngine._guard = lambda self, net, out: True
    sd = {k: torch.empty(v, device=META) for k, v in state_dict_layout(spec).items()}
    eng = E.HipEngine(cfg_of(spec), sd, META)
    assert not eng.autotune
    sw = Switches(flags, arith)
    for k in ("planes_gemm", "pw2_small_pc", "pw2_narrow", "gemm_big", "use_split", "arith"):
        setattr(eng, k, getattr(sw, k))
    eng.arith_net = {"E": arith, "X": arith}
    eng.lib = Recorder(eng.lib)
    return eng


def record(spec, B, flags=0, arith=2, fused=True):
    """one embedder + one extractor pass of B frames: (conv rows, stage rows), each row inputs + what the engine did"""
    eng = make_engine(spec, flags, arith)
    eng.fused_blocks = fused
    calls, ws = [], {}
    conv0, buf0 = eng.conv, eng.buf

    def conv(x, w, out, **kw):
        n0 = len(eng.lib.launches)
        ws.clear()
        r = conv0(x, w, out, **kw)
        assert len(eng.lib.launches) == n0 + 1
        calls.append((w, out, kw, eng.lib.launches[-1], dict(ws)))
        return r

    def buf(tag, numel, zero=False):
        if tag.startswith("splitk.ws"):
            ws["numel"] = numel
        return torch.empty(numel, device=META)

    eng.conv, eng.buf = conv, buf
    S = spec.img_size
    eng.embedder_forward(E.Act(torch.empty(B * S * S * 4, device=META), B, S, S, spec.in_ch, 4), torch.empty(1, spec.nbits, dtype=torch.int32, device=META))
    n_embed = len(calls)
    eng.extractor_forward(E.Act(torch.empty(B * S * S * 4, device=META), B, S, S, 3, 4))
    conv_rows, stage_seen = [], {}
    which = {id(blk[k]): (sti, k) for sti, st in enumerate((eng.X or {}).get("stages", [])) for blk in st for k in ("pw1", "pw2")}
    for i, (w, out, kw, d, wsd) in enumerate(calls):
        row = {k: d[k] for k in CONV_IN[:20]}
        row.update({k: int(bool(d[k])) for k in PTRS})
        row["tile_hint"], row["split_k"] = kw.get("tile_hint", 0), kw.get("split_k") or 0
        fold = kw.get("grn_fold")
        row["grn_hw"], row["grn_c4"] = (fold[3], fold[4]) if fold is not None else (0, 0)
        got = dict(routes=routes_of(desc_of(row)), split_k=max(1, d["split_k"]), tile_hint=d["tile_hint"],
                   ws_slices=(wsd["numel"] // (out.rows * d["splitk_ld"]) if d["split_k"] > 1 else 0), grn_fold=int(bool(d["grn_part"])))
        assert got == conv_decision(row), (row, got, conv_decision(row))
        conv_rows.append({**row, **got})
        if i >= n_embed and id(w) in which:
            stage_seen.setdefault(which[id(w)][0], {})[which[id(w)][1]] = (d, out)
    stage_rows = []
    for sti, seen in sorted(stage_seen.items()):
        d1, hh = seen["pw1"]
        d2, cur = seen["pw2"]
        row = dict(rows=cur.rows, HW=cur.H * cur.W, C=cur.C, h_ld=hh.ld, pw1_cinp=d1["CinP"], arith=arith, flags=flags)
        p = stage_plan(row)
        # what the launches show of the plan
        assert bool(d1["in_pl"]) == bool(p["pl1"]) and bool(d2["in_pl"]) == bool(p["pl2"]), (row, p)
        assert not p["pl1"] or d1["tile_hint"] == p["tile1"], (row, p)
        assert not p["pl2"] or (d2["tile_hint"] == p["tile2"] and max(1, d2["split_k"]) == p["sk2"]), (row, p)
        assert (d2["tile_hint"] == (N.CONV_TILE_HI | 10)) == bool(p["pw2_narrow"]), (row, p)
        stage_rows.append({**row, **p})
    return conv_rows, stage_rows


# ---------------------------------------------------------------------------------------------- random shapes around the thresholds
def rup(x, m):
    return (x + m - 1) // m * m


def base_row(B, H, W, cin, cinp, n, k=1):
    return dict(B=B, H=H, W=W, Cin=cin, KH=k, KW=k, SH=1, SW=1, PH=k // 2, PW=k // 2, Ho=H, Wo=W, CinP=cinp, N=n, n_store=rup(n, 4), Cin2P=0,
                in_sb=H * W * cin, in_sy=W * cin, in_sx=cin, a_scale_ld=0, a_scale=0, in2=0, wt_split=1, wt_blk=1, wt2_blk=0, in_pl=0, in2_pl=0,
                sumsq_part=0, tile_hint=0, split_k=0, grn_hw=0, grn_c4=0)


def random_conv_rows(rng, n_each=320):
    rows = []
    frames = [(31, 31), (63, 63), (8, 8), (8, 12), (8, 16), (16, 16), (32, 32), (4, 4), (16, 8), (1, 1)]          # HW 961, 3969, 64, 96, 128, ...
    for _ in range(n_each):      # small-M 1x1 GEMM: blocks * sk near 256, K per slice near 3072, GRN on the A path, Cin % 32 != 0
        H, W = rng.choice(frames)
        B = rng.choice([1, 2, 3, 4, 6, 8, 16, 32])
        pairs = rng.choice([3, 4, 7, 8, 12, 16, 24, 32, 48, 64, 96, 97, 128, 192, 193, 216, 256, 362])
        cinp = 32 * pairs - rng.choice([0, 0, 0, 16])
        mb = (B * H * W + 127) // 128
        want = rng.choice([256, 128, 64, 32]) + rng.choice([-1, 0, 1])       # blocks just below / at / above 256 / sk
        n = max(1, min(4096, want // mb)) * 128 - rng.choice([0, 0, 32, 64, 127]) if rng.random() < 0.7 else rng.choice([96, 192, 384, 768, 362, 724, 2896])
        r = base_row(B, H, W, cinp - rng.choice([0, 0, 0, 4]), cinp, max(1, n))
        if rng.random() < 0.5:
            r.update(a_scale=1, a_scale_ld=rng.choice([cinp, cinp, cinp + 32]))
            if rng.random() < 0.7:
                r.update(grn_hw=H * W, grn_c4=rng.choice([cinp, cinp, cinp - 8]))
        if rng.random() < 0.1:
            r.update(sumsq_part=1)
        if rng.random() < 0.1:
            r.update(in_sy=W * r["Cin"] + 32, in_sb=H * (W * r["Cin"] + 32))           # rows not dense
        if rng.random() < 0.15:
            r.update(tile_hint=rng.choice([N.CONV_TILE_HI | 1, N.CONV_TILE_HI | 2, N.CONV_TILE_HI | 10, 1, N.CONV_FORCE_F32]), split_k=rng.choice([0, 1, 1, 2]))
        if rng.random() < 0.05:
            r.update(wt_blk=0)
        rows.append(r)
    for _ in range(n_each):      # 3x3 patch kernel: workgroups * slices near 192, N % 192, chunks per slice >= 2, a second phase
        H, W = rng.choice([(16, 16), (32, 32), (8, 16), (24, 16), (32, 48), (16, 24), (31, 31), (64, 64), (8, 8)])
        nn = rng.choice([64, 96, 128, 160, 192, 256, 320, 384, 576, 768])
        cinp = 16 * rng.choice([1, 2, 4, 6, 8, 9, 10, 12, 16, 18, 24, 32, 36, 48])
        per = max(1, (H // 8) * (W // 16) * ((nn + 191) // 192 if nn % 192 == 0 else (nn + 127) // 128))
        want = rng.choice([192, 96, 64, 48, 32, 24]) + rng.choice([-1, 0, 1])
        B = max(1, want // per) if rng.random() < 0.7 else rng.choice([1, 2, 4, 8, 32])
        r = base_row(B, H, W, cinp, cinp, nn, 3)
        if rng.random() < 0.4:
            r.update(in2=1, Cin2P=rng.choice([cinp, 16]), wt2_blk=int(rng.random() < 0.9))
        if rng.random() < 0.1:
            r.update(sumsq_part=1)
        if rng.random() < 0.1:
            r.update(a_scale=1, a_scale_ld=9 * nn, tile_hint=(N.CONV_TILE_HI if nn % 192 == 0 else 15) | N.CONV_PRE)
        if rng.random() < 0.15:      # the planes chain: the caller brings tile 22 and its own slice count
            r.update(in_pl=1, in2=0, in2_pl=r["in2"], tile_hint=N.CONV_TILE_HI | 6, split_k=rng.choice([0, 2, 3, 4]))
        if rng.random() < 0.1:       # thin layers (tile 20)
            r.update(CinP=16, Cin=rng.choice([4, 16]), N=rng.choice([16, 32, 48]), n_store=rng.choice([16, 32, 36]))
            r.update(in_sx=r["Cin"], in_sy=W * r["Cin"], in_sb=H * W * r["Cin"], Cin2P=16 if r["in2"] else 0)
        rows.append(r)
    return rows


def random_stage_rows(rng, n=400):
    out = []
    for _ in range(n):
        HW = rng.choice([31 * 31, 63 * 63, 127 * 127, 64, 96, 128, 256, 1024, 4096, 16, 4])
        C = rng.choice([96, 192, 384, 768, 362, 724, 1448, 2896, 128, 256, 512, 1024, 48, 90, 640, 672])
        xld = lambda c: rup(c, 32) if c >= 128 else rup(c, 4)
        # batch sizes that put the 256-row / 128-row tile counts next to 200, 128, 256 and 3 * 256
        want = rng.choice([200, 128, 256, 768, 64]) * rng.choice([256, 128]) // max(1, rng.choice([(C + 191) // 192, (4 * C + 191) // 192, (C + 127) // 128, (C + 95) // 96, 1]))
        B = max(1, (want + rng.choice([-256, -128, 0, 128, 256])) // HW) if rng.random() < 0.7 else rng.choice([1, 2, 4, 8, 16, 32])
        out.append(dict(rows=B * HW, HW=HW, C=C, h_ld=xld(4 * C), pw1_cinp=rup(xld(C), 16), arith=rng.choice([2, 2, 2, 3]), flags=rng.randrange(32)))
    return out


def main():
    cards = os.path.join(ROOT, "videoseal_amd", "cards")
    specs = [(n, spec_from_card(os.path.join(cards, n + ".yaml"))) for n in ("videoseal_1.0", "pixelseal", "chunkyseal", "videoseal_0.0")]
    specs += [("tiny", tiny_spec()), ("tinyc", tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16)),
              ("tinyv", legacy_tiny_spec())]
    conv_rows, stage_rows = [], []
    for name, spec in specs:
        for B in (32, 16, 8, 4, 1, 2, 3, 6):
            for fused in (True, False):          # (False: the stage-0 / 1 GEMMs of the unfused block form)
                c, s = record(spec, B, fused=fused)
                conv_rows += c
                stage_rows += s
        print(name, len(conv_rows), len(stage_rows))
    for name, spec in specs[:3]:                 # every switch combination on the real engine, benchmark batches
        for flags, B in itertools.product(range(32), (32, 16)):
            c, s = record(spec, B, flags=flags)
            conv_rows += c
            stage_rows += s
        c, s = record(spec, 32, arith=3)
        conv_rows += c
        stage_rows += s
    base = {tuple(r[k] for k in STAGE_IN[:5]) for r in stage_rows}
    for r, flags, arith in itertools.product(sorted(base), range(32), (2, 3)):        # ... and on the functions, every recorded stage shape
        if (arith == 2 and r[0] // r[1] in (32, 16, 8, 4) and r[2] >= 96) or flags == 0:      # (all 32 at the cards' benchmark batches)
            row = {**dict(zip(STAGE_IN[:5], r)), "arith": arith, "flags": flags}
            stage_rows.append({**row, **stage_plan(row)})
    rng = random.Random(20261019)
    for r in random_conv_rows(rng):
        conv_rows.append({**r, **conv_decision(r)})
    for r in random_stage_rows(rng):
        stage_rows.append({**r, **stage_plan(r)})

    def table(rows, cols):
        return sorted({tuple(int(r[k]) for k in cols) for r in rows})
    out = dict(conv_in=CONV_IN, conv_out=CONV_OUT, conv=table(conv_rows, CONV_IN + CONV_OUT),
               stage_in=STAGE_IN, stage_out=STAGE_OUT, stage=table(stage_rows, STAGE_IN + STAGE_OUT))
    path = os.path.join(HERE, "conv_plan.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{path}: {len(out['conv'])} conv rows, {len(out['stage'])} stage rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
