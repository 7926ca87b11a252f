"""Scratch-size contracts of the C ABI.  About twenty entry points take a caller-allocated workspace whose size comes from a companion
function; the sizing rule and the launch geometry are written twice (size function, launcher) and both branch.  Every other test hands over
`torch.empty(size)` from the caching allocator, where an overrun lands in slack and a reducer that sums a slot no producer wrote reads whatever
was there.

Here every case runs its entry point three times:
  nan   scratch of EXACTLY the stated size between sentinel bands (tests/_guards.py), interior filled with NaN; inputs between NaN bands,
        outputs between sentinels
  zero  the same with the interior zeroed
  plain ordinary tensors
and asserts: every band intact; the outputs of `nan` and `zero` bit-identical (no result may depend on what the scratch held: a reducer that
read an unwritten slot would turn NaN into the output); both equal to `plain`.  The shapes are the smallest that reach each branch of each
sizing rule; the comment of a case names the branch (figures checked against the size functions on the host)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._gpu import _contract, _lib as _L, r4  # noqa: E402
from videoseal_amd import native as N  # noqa: E402

# ====================================================================================================== vs_gemm_wgrad_partial_floats
# wgrad_splits: matrix cores (N >= 64 and K >= 64): 512 / (tilesN128 * tilesK128); else thin: ceil(1024 / (tilesN64 * tilesK64)); both capped by
# ceil(rows / 256), floor 1.  The launcher rounds rows-per-slice up to 32 and launches used = ceil(rows / rps) <= splits slices.
GEMM_WGRAD = [
    (7, 5, 70),               # thin path, quota 512 > cap ceil(7/256) = 1: one slice
    (300, 64, 64),            # matrix cores, quota 512 > cap 2: splits = 2 = used (rps 150 -> 160)
    (2400, 1024, 1024),       # matrix cores, 64 tiles: quota 8 < cap 10: splits = 8 = used (rps 300 -> 320)
    (8200, 64, 2048),         # matrix cores, 16 tiles: quota 32 < cap 33; rps 257 -> 288: used = 29 < splits = 32
    (8500, 32, 2048),         # thin path, 32 tiles: quota 32 < cap 34; rps 266 -> 288: used = 30 < splits = 32
    (300, 2944, 2944),        # matrix cores, 23 x 23 = 529 tiles: quota 512 / 529 = 0 -> the floor of one slice
]


@pytest.mark.parametrize("rows,n,k", GEMM_WGRAD)
def test_gemm_wgrad(rows, n, k):
    L, st = _L()
    ldn, ldk = r4(n), r4(k)

    def case(a):
        dy, x = a.rand("dy", rows, ldn, lanes=n), a.rand("x", rows, ldk, lanes=k)
        part = a.scratch(L.vs_gemm_wgrad_partial_floats(rows, n, k))
        dw = a.out(n, k)
        N.check(L.vs_gemm_wgrad(N.ptr(dy), ldn, n, N.ptr(x), ldk, k, rows, N.ptr(part), N.ptr(dw), st), "vs_gemm_wgrad")
        return [dw]
    _contract(case)


# ====================================================================================================== vs_conv3x3_wgrad_partial_floats
# matrix cores (N >= 64 and ld >= 64): the GEMM rule on rows = B * Ho * Wo, K = 9 ld.  Thin kernel: one slot per workgroup, nwg = min(ntiles, 512),
# ntiles = B * ceil(Wo / 16) * ceil(Ho / TH), TH = 16 halved while the tile exceeds 40 KiB of LDS.
CONV3_WGRAD = [   # B, H, W, ci, co, stride, reflect
    (2, 12, 10, 64, 64, 1, 0),         # matrix cores, 240 rows: one slice
    (2, 16, 24, 512, 128, 1, 1),       # matrix cores, 768 rows: 3 slices (cap), reflection padding
    (2, 20, 18, 16, 16, 1, 0),         # thin, TH = 16: ntiles = 2 * 2 * 2 = 8 < 512
    (3, 256, 256, 4, 4, 1, 0),         # thin, ntiles = 3 * 16 * 16 = 768 > 512: 512 workgroups stride over the tiles
    (2, 40, 24, 32, 32, 1, 0),         # thin, TH halved to 8 (18 * 18 * 32 + 256 * 32 floats > 40 KiB): ntiles = 2 * 2 * 5 = 20
    (2, 33, 31, 16, 32, 2, 0),         # thin, stride 2, TH halved twice to 4: ntiles = 2 * 1 * 5 = 10
    (1, 19, 35, 20, 12, 1, 1),         # thin, reflection padding, odd map: ntiles = 3 * 2 = 6
    (1, 2, 2, 8, 4, 1, 1),             # thin, reflection at H = W = 2: every border pixel mirrors onto the other one
]


@pytest.mark.parametrize("B,H,W,ci,co,stride,reflect", CONV3_WGRAD)
def test_conv3x3_wgrad(B, H, W, ci, co, stride, reflect):
    L, st = _L()
    ld, ldn = r4(ci), r4(co)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert L.vs_conv3x3_wgrad_supported(co, ld, stride)

    def case(a):
        x, dy = a.rand("x", B * H * W, ld, lanes=ci), a.rand("dy", B * Ho * Wo, ldn, lanes=co)
        part = a.scratch(L.vs_conv3x3_wgrad_partial_floats(co, ld, B, H, W, stride))
        dw = a.out(co, 9 * ld)
        N.check(L.vs_conv3x3_wgrad(N.ptr(dy), ldn, co, N.ptr(x), ld, B, H, W, stride, N.PAD_REFLECT if reflect else N.PAD_ZERO, N.ptr(part), N.ptr(dw), st),
                "vs_conv3x3_wgrad")
        return [dw]
    _contract(case)


# ====================================================================================================== vs_dwconv7_wgrad_partial_floats
# one chunk per (frame, band of RB rows), RB = ceil(B * H / 2048)
@pytest.mark.parametrize("B,H,W,C,ld", [
    (2, 9, 11, 6, 8),                  # B * H = 18 <= 2048: RB = 1, a chunk per image row
    (33, 65, 5, 4, 4),                 # B * H = 2145 > 2048: RB = 2, 33 bands per frame, the last one a single row (65 % 2 = 1)
])
def test_dwconv7_wgrad(B, H, W, C, ld):
    L, st = _L()

    def case(a):
        x, dy = a.rand("x", B * H * W, ld, lanes=C), a.rand("dy", B * H * W, ld, lanes=C)
        part = a.scratch(L.vs_dwconv7_wgrad_partial_floats(B, H, ld))
        dw = a.out(49, ld)
        N.check(L.vs_dwconv7_wgrad(N.ptr(x), ld, N.ptr(dy), ld, B, H, W, C, N.ptr(part), N.ptr(dw), st), "vs_dwconv7_wgrad")
        return [dw]
    _contract(case)


# ====================================================================================================== vs_colreduce_partial_floats
# (B * ceil(HW / 64) + 1) * 3 * ld: chunks of 64 rows that never straddle a frame (+ one slot for the totals of vs_layernorm_bwd)
@pytest.mark.parametrize("rows,C,ld", [
    (100, 18, 24),                     # two chunks, the second ragged (36 rows); C % 4 != 0 and ld > 4 ceil(C / 4)
    (64, 16, 16),                      # exactly one chunk
    (1, 4, 4),                         # a single row
    (130, 1100, 1100),                 # 275 channel groups > 256: two sweeps of the column reduction (blockIdx.y)
])
def test_layernorm_bwd(rows, C, ld):
    L, st = _L()

    def case(a):
        x, dy, w = a.rand("x", rows, ld, lanes=C, scale=2.0, shift=0.3), a.rand("dy", rows, ld, lanes=C), a.rand("w", C)
        part = a.scratch(L.vs_colreduce_partial_floats(1, rows, ld))
        dx, stats, dw, db = a.out(rows, ld), a.out(2 * rows), a.out(C), a.out(C)
        N.check(L.vs_layernorm_bwd(N.ptr(x), ld, N.ptr(dy), ld, N.ptr(w), rows, C, 1e-6, N.ptr(dx), ld, N.ptr(stats), N.ptr(part), N.ptr(dw), N.ptr(db), st),
                "vs_layernorm_bwd")
        return [dx, stats, dw, db]
    _contract(case)


@pytest.mark.parametrize("B,HW,C,ld", [
    (3, 100, 18, 24),                  # two chunks per frame, the second ragged; C % 4 != 0, ld > 4 ceil(C / 4)
    (2, 64, 8, 8),                     # exactly one chunk per frame
    (1, 70, 1100, 1100),               # two sweeps of the column reduction, five workgroups of the per-channel sums
])
def test_gelu_grn_bwd(B, HW, C, ld):
    L, st = _L()

    def case(a):
        h1, d3, gamma = a.rand("h1", B * HW, ld, lanes=C), a.rand("d3", B * HW, ld, lanes=C), a.rand("gamma", C)
        part = a.scratch(L.vs_colreduce_partial_floats(B, HW, ld))
        coef = a.scratch(6 * B * ld)                                   # (the header's figure for the second workspace)
        dh1, dg, db = a.out(B * HW, ld), a.out(C), a.out(C)
        N.check(L.vs_gelu_grn_bwd(N.ptr(h1), ld, N.ptr(d3), ld, N.ptr(gamma), B, HW, C, N.ptr(part), N.ptr(coef), N.ptr(dh1), ld, N.ptr(dg), N.ptr(db), st),
                "vs_gelu_grn_bwd")
        return [dh1, dg, db]
    _contract(case)


# ====================================================================================================== vs_bn_partial_doubles
# ceil(rows / chunk) * 2 * ld doubles, chunk = bn_chunk_rows(ld) = 16 * (256 / G) rows with G = min(ld / 4, 64) channel groups per workgroup
BN_FWD = [   # rows, C, ld
    (2100, 8, 8),                      # G = 2: chunk 2048; two chunks, the second ragged
    (2048, 8, 8),                      # exactly one chunk
    (70, 6, 12),                       # G = 3 (256 % 3 != 0: one idle thread), chunk 1360 > rows; C % 4 != 0, ld > 4 ceil(C / 4)
    (900, 18, 20),                     # G = 5: 51 row lanes, 255 live threads; chunk 816, two chunks
    (67, 1100, 1100),                  # G = 64: chunk 64, two chunks; 275 groups = five workgroups across the channels, the last one partial
]


@pytest.mark.parametrize("rows,C,ld", BN_FWD)
def test_bn_partial_sums_and_batch_stats(rows, C, ld):
    L, st = _L()

    def case(a):
        x = a.rand("x", rows, ld, lanes=C, scale=1.5, shift=0.2)
        part = a.scratch(L.vs_bn_partial_doubles(rows, ld), torch.float64)
        sums = a.out(2 * ld + 1, dtype=torch.float64)
        N.check(L.vs_bn_partial_sums(N.ptr(x), rows, C, ld, N.ptr(part), N.ptr(sums), st), "vs_bn_partial_sums")
        gamma, beta = a.rand("gamma", C, shift=1.0, scale=0.2), a.rand("beta", C)
        part2 = a.scratch(L.vs_bn_partial_doubles(rows, ld), torch.float64)
        rm, rv, scale, shift = a.out(C, init=0), a.out(C, init=1), a.out(C), a.out(C)
        N.check(L.vs_bn_batch_stats(N.ptr(x), rows, C, ld, N.ptr(gamma), N.ptr(beta), 1e-5, 0.1, N.ptr(rm), N.ptr(rv), N.ptr(part2), N.ptr(scale), N.ptr(shift),
                                    st), "vs_bn_batch_stats")
        return [sums, rm, rv, scale, shift]          # (the pad lanes of `sums` hold the sums of the zero pad lanes)
    _contract(case)


# ====================================================================================================== vs_bn_bwd_partial_floats
# ceil(rows / 256) * 2 * ldp floats with ldp = 4 ceil(C / 4) (what the kernel strides by, whatever the tensors' ld); mean / rstd / scale / shift
# are read in whole float4: 4 ceil(C / 4) entries each
@pytest.mark.parametrize("rows,C,ld", [
    (300, 6, 8),                       # two chunks, the second ragged; C % 4 != 0: the parameter vectors are read two entries past C
    (256, 8, 8),                       # exactly one chunk
    (70, 6, 12),                       # ld > 4 ceil(C / 4)
    (600, 1100, 1100),                 # 275 channel groups > 256: the workgroup walks the channels twice
])
def test_bn_relu_bwd_sums(rows, C, ld):
    L, st = _L()
    ldp = r4(C)

    def case(a):
        raw, dy = a.rand("raw", rows, ld, lanes=C, scale=1.5, shift=0.2), a.rand("dy", rows, ld, lanes=C)
        mean, rstd = a.rand("mean", ldp, scale=0.1, shift=0.2, lanes=C), a.rand("rstd", ldp, uniform=True, shift=0.5, lanes=C)
        scale, shift = a.rand("scale", ldp, uniform=True, shift=0.5, lanes=C), a.rand("shift", ldp, scale=0.3, lanes=C)
        part = a.scratch(L.vs_bn_bwd_partial_floats(rows, ldp))
        sums = a.out(2 * ldp + 1, dtype=torch.float64)
        dg, db = a.out(C), a.out(C)
        N.check(L.vs_bn_relu_bwd_sums(N.ptr(raw), ld, N.ptr(dy), ld, N.ptr(mean), N.ptr(rstd), N.ptr(scale), N.ptr(shift), 1, rows, C, N.ptr(part), N.ptr(sums),
                                      N.ptr(dg), N.ptr(db), st), "vs_bn_relu_bwd_sums")
        return [sums, dg, db]
    _contract(case)


# ====================================================================================================== vs_vit_attention_bwd_scratch_floats
# frames * H * W * heads * (RP + 2 TMAX) + the fixed block of relative-position partial sums (read only with tables)
@pytest.mark.parametrize("B,H,W,heads,hd,win,rel", [
    (2, 8, 8, 2, 16, 4, True),         # 4 x 4 windows, tables
    (2, 8, 8, 2, 16, 4, False),        # windows, no tables: the partial-sum block stays untouched
    (1, 8, 12, 3, 32, 0, True),        # global attention over a non-square grid, tables [2 H - 1] and [2 W - 1]
    (2, 4, 4, 1, 16, 0, False),        # global, no tables
    (1, 16, 16, 2, 64, 0, True),       # 256 tokens: the largest group, 16 = TMAX per side
])
def test_vit_attention_bwd(B, H, W, heads, hd, win, rel):
    L, st = _L()
    D = heads * hd
    Th, Tw = (win, win) if win else (H, W)

    def case(a):
        qkv = a.rand("qkv", B, H, W, 3 * D)
        rh = a.rand("rh", 2 * Th - 1, hd, scale=0.3) if rel else None
        rw = a.rand("rw", 2 * Tw - 1, hd, scale=0.3) if rel else None
        if "out" not in a.store:
            o = torch.empty(B, H, W, D, device="cuda")
            N.check(L.vs_vit_attention(N.ptr(a.store["qkv"]), B, H, W, heads, hd, win, N.ptr(a.store.get("rh")), N.ptr(a.store.get("rw")), N.ptr(o), st),
                    "vs_vit_attention")
            a.store["out"] = o
        out, dout = a.inp(a.store["out"]), a.rand("dout", B, H, W, D)
        scr = a.scratch(L.vs_vit_attention_bwd_scratch_floats(B, H, W, heads, win))
        dqkv = a.out(B, H, W, 3 * D)
        drh = a.out(2 * Th - 1, hd) if rel else None
        drw = a.out(2 * Tw - 1, hd) if rel else None
        N.check(L.vs_vit_attention_bwd(N.ptr(qkv), N.ptr(out), N.ptr(dout), B, H, W, heads, hd, win, N.ptr(rh), N.ptr(rw), N.ptr(dqkv), N.ptr(scr), N.ptr(drh),
                                       N.ptr(drw), st), "vs_vit_attention_bwd")
        return [dqkv] + ([drh, drw] if rel else [])
    _contract(case)


# ====================================================================================================== vs_aug_color(_bwd)_scratch_floats
# contrast only: one partial per workgroup, gridx(plane, 256, cap 256) workgroups per frame (+ the F frame means / sums)
COLOR = [
    (2, 100, 90),                      # plane 9000: 36 workgroups, below the cap
    (2, 257, 256),                     # plane 65 792 = 257 * 256: capped at 256 workgroups, every thread strides twice
    (1, 3, 5),                         # a plane smaller than one workgroup
]


@pytest.mark.parametrize("Fr,H,W", COLOR)
def test_aug_color_contrast_and_its_adjoint(Fr, H, W):
    L, st = _L()
    CONTRAST = 1

    def case(a):
        x = a.rand("x", Fr, 3, H, W, uniform=True)
        scr = a.scratch(L.vs_aug_color_scratch_floats(Fr, H, W))
        y = a.out(Fr, 3, H, W)
        N.check(L.vs_aug_color(N.ptr(x), N.ptr(y), Fr, H, W, CONTRAST, 1.4, N.ptr(scr), st), "vs_aug_color")
        means = a.inp(scr[-Fr:].clone())                               # the frame means the forward left at the end of its scratch
        dy = a.rand("dy", Fr, 3, H, W)
        scr2 = a.scratch(L.vs_aug_color_bwd_scratch_floats(Fr, H, W))
        dx = a.out(Fr, 3, H, W)
        N.check(L.vs_aug_color_bwd(N.ptr(x), N.ptr(dy), N.ptr(dx), Fr, H, W, CONTRAST, 1.4, N.ptr(means), N.ptr(scr2), st), "vs_aug_color_bwd")
        return [y, scr[-Fr:], dx]
    _contract(case)


# ====================================================================================================== vs_percep / vs_jnd_loss _partial_doubles
# one double per workgroup, gridx(n, 256, cap 1024) workgroups: n = F * H * W pixels (percep), 3 * F * H * W elements (JND loss)
@pytest.mark.parametrize("Fr,H,W,yuv", [
    (2, 37, 41, 1),                    # 3034 pixels: 12 workgroups, the last ragged
    (1, 513, 512, 0),                  # 262 656 pixels = 1026 workgroups' worth: capped at 1024
    (1, 1, 1, 1),
])
def test_percep_mse(Fr, H, W, yuv):
    L, st = _L()

    def case(a):
        x, y = a.rand("x", Fr, 3, H, W, uniform=True), a.rand("y", Fr, 3, H, W, uniform=True)
        part = a.scratch(L.vs_percep_partial_doubles(Fr, H, W), torch.float64)
        loss = a.out(1)
        N.check(L.vs_percep_mse(N.ptr(x), N.ptr(y), Fr, H, W, yuv, N.ptr(part), N.ptr(loss), st), "vs_percep_mse")
        return [loss]
    _contract(case)


@pytest.mark.parametrize("Fr,H,W", [
    (2, 37, 41),                       # 9102 elements: 36 workgroups
    (1, 296, 296),                     # 262 848 elements = 1027 workgroups' worth: capped at 1024
])
def test_jnd_loss(Fr, H, W):
    L, st = _L()

    def case(a):
        x, y = a.rand("x", Fr, 3, H, W, uniform=True), a.rand("y", Fr, 3, H, W, uniform=True)
        hm = a.rand("hm", Fr, 1, H, W, uniform=True, scale=0.1)
        part = a.scratch(L.vs_jnd_loss_partial_doubles(Fr, H, W), torch.float64)
        loss = a.out(1)
        N.check(L.vs_jnd_loss(N.ptr(x), N.ptr(y), N.ptr(hm), Fr, H, W, N.ptr(part), N.ptr(loss), st), "vs_jnd_loss")
        return [loss]
    _contract(case)


# ====================================================================================================== vs_ssim_partial_doubles
# 2 * P * strips * chunks, strips = ceil((W - 10) / 128), chunks = ceil((H - 10) / rows), rows = 96 halved (down to 24) while the grid has fewer
# than 1024 workgroups
@pytest.mark.parametrize("P,H,W", [
    (6, 50, 139),                      # rows 24: 2 strips (129 valid columns: the second holds one) x 2 chunks (40 valid rows)
    (400, 107, 21),                    # rows 48: 400 x 2 = 800 < 1024 at 96, 400 x 3 = 1200 at 48
    (600, 107, 21),                    # rows 96 kept: 600 x 2 = 1200 workgroups; the second chunk holds one row
    (1, 11, 11),                       # the smallest legal plane: one valid pixel
])
def test_ssim_stats(P, H, W):
    from videoseal_amd import autograd as AG
    L, st = _L()

    def case(a):
        x = a.rand("x", P, H, W, uniform=True)
        y = a.rand("y", P, H, W, uniform=True)
        part = a.scratch(L.vs_ssim_partial_doubles(P, H, W), torch.float64)
        out = a.out(2, P, dtype=torch.float64)
        N.check(L.vs_ssim_stats(N.ptr(x), N.ptr(y), P, H, W, 1.0, AG._win11(), N.ptr(part), N.ptr(out), st), "vs_ssim_stats")
        return [out]
    _contract(case)


# ====================================================================================================== JPEG / H.264-proxy workspaces (bytes)
@pytest.mark.parametrize("Fr,H,W", [
    (2, 37, 53),                       # neither a multiple of 16 (nor of 8): padded planes 48 x 64, the scalar kernels
    (1, 64, 48),                       # whole MCUs: the vector kernels
    (3, 16, 17),                       # one column past an MCU
])
def test_jpeg_roundtrip(Fr, H, W):
    L, st = _L()

    def case(a):
        x = a.rand("x", Fr, 3, H, W, uniform=True, scale=1.2, shift=-0.1)
        ws = a.scratch(L.vs_jpeg_workspace_bytes(Fr, H, W), torch.uint8)
        y = a.out(Fr, 3, H, W)
        N.check(L.vs_jpeg_roundtrip(N.ptr(x), N.ptr(y), Fr, H, W, 60, N.ptr(ws), st), "vs_jpeg_roundtrip")
        return [y]
    _contract(case)


@pytest.mark.parametrize("rgb", [0, 1])
@pytest.mark.parametrize("Fr,H,W", [(2, 37, 53), (1, 64, 48), (3, 9, 7)])
def test_h264_proxy_roundtrip(Fr, H, W, rgb):
    """planes padded to multiples of 8: F * H8 * W8 * 3 bytes cover the three full planes of rgb_mode (+ 256 spare); 4:2:0 uses half of it"""
    L, st = _L()

    def case(a):
        x = a.rand("x", Fr, 3, H, W, uniform=True, scale=1.2, shift=-0.1)
        ws = a.scratch(L.vs_h264_proxy_workspace_bytes(Fr, H, W), torch.uint8)
        y = a.out(Fr, 3, H, W)
        N.check(L.vs_h264_proxy_roundtrip(N.ptr(x), N.ptr(y), Fr, H, W, 30, rgb, N.ptr(ws), st), "vs_h264_proxy_roundtrip")
        return [y]
    _contract(case)


# ====================================================================================================== discriminator
# vs_groupnorm_partial_doubles: B * nch * 2 C + B * 2 C + B * 8 + B * nch * 8 with nch = ceil(HW / 64) (forward and backward share the rule)
@pytest.mark.parametrize("C,B,H,W", [
    (64, 2, 9, 13),                    # the suite's smallest case: 117 rows = two chunks, the second ragged
    (16, 1, 1, 5),                     # fewer rows than one chunk, the narrowest legal C
    (32, 2, 8, 8),                     # exactly one chunk per frame
])
def test_groupnorm_lrelu_and_its_adjoint(C, B, H, W):
    L, st = _L()
    ld, HW = C + 4, H * W

    def case(a):
        x, dy = a.rand("x", B * HW, ld, lanes=C, scale=1.5, shift=0.3), a.rand("dy", B * HW, ld, lanes=C)
        gamma, beta = a.rand("gamma", C, scale=0.2, shift=1.0), a.rand("beta", C, scale=0.2)
        part = a.scratch(L.vs_groupnorm_partial_doubles(B, HW, C), torch.float64)
        mean, rstd, y = a.out(4 * B, dtype=torch.float64), a.out(4 * B, dtype=torch.float64), a.out(B * HW, ld)
        N.check(L.vs_groupnorm_lrelu(N.ptr(x), ld, B, HW, C, 4, N.ptr(gamma), N.ptr(beta), 1e-5, 0.2, N.ptr(part), N.ptr(mean), N.ptr(rstd), N.ptr(y), ld, st),
                "vs_groupnorm_lrelu")
        part2 = a.scratch(L.vs_groupnorm_partial_doubles(B, HW, C), torch.float64)
        dx, dg, db = a.out(B * HW, ld), a.out(C), a.out(C)
        N.check(L.vs_groupnorm_lrelu_bwd(N.ptr(dy), ld, N.ptr(x), ld, B, HW, C, 4, N.ptr(gamma), N.ptr(beta), N.ptr(mean), N.ptr(rstd), 0.2, N.ptr(part2),
                                         N.ptr(dx), ld, N.ptr(dg), N.ptr(db), st), "vs_groupnorm_lrelu_bwd")
        return [mean, rstd, y, dx, dg, db]
    _contract(case)


# vs_conv4x4_wgrad_partial_floats: N = 1: ceil(rows / 128) slices; else 512 / (tilesN128 * tiles(16 ld / 128)) capped by ceil(rows / 256), rows per
# slice rounded up to 16
@pytest.mark.parametrize("ld,ci,n,stride,B,H,W", [
    (4, 1, 32, 1, 3, 23, 19),          # the suite's smallest pair: 1188 rows, quota 512 > cap 5: five slices of 240 rows, the last ragged
    (4, 3, 32, 2, 3, 23, 19),          # stride 2: 297 rows, two slices of 160
    (128, 128, 1, 1, 3, 23, 19),       # N = 1: the reduction kernel, ceil(1188 / 128) = 10 slices, dense dy
    (256, 256, 1, 2, 1, 2, 2),         # N = 1 on the smallest legal map: one output pixel
    (64, 64, 128, 1, 9, 40, 40),       # 13 689 rows: quota 512 / 8 = 64 > cap 54; rps 254 -> 256: used = 54
    (256, 256, 256, 1, 4, 34, 34),     # 4356 rows: 2 x 32 tiles: quota 8 < cap 18; rps 545 -> 560: used = 8
])
def test_conv4x4_wgrad(ld, ci, n, stride, B, H, W):
    L, st = _L()
    Ho, Wo = (H - 2) // stride + 1, (W - 2) // stride + 1
    dyl = 1 if n == 1 else n + 4
    assert L.vs_conv4x4_wgrad_supported(n, ld, stride)

    def case(a):
        x = a.rand("x", B * H * W, ld, lanes=ci)
        dy = a.rand("dy", B * Ho * Wo, dyl, lanes=n)
        part = a.scratch(L.vs_conv4x4_wgrad_partial_floats(n, ld, B, H, W, stride))
        dw = a.out(n, 16 * ld)
        N.check(L.vs_conv4x4_wgrad(N.ptr(dy), dyl, n, N.ptr(x), ld, B, H, W, stride, N.ptr(part), N.ptr(dw), st), "vs_conv4x4_wgrad")
        return [dw]
    _contract(case)


# ====================================================================================================== pixel-wise head
# vs_pixel_linear_bwd_partial_floats: nb * K * (C + 4), nb = min(ceil(rows / 256), 512) workgroups of whole 32-row tiles
@pytest.mark.parametrize("B,hh,ww,K,C", [
    (2, 12, 20, 17, 24),               # the suite's smallest case: 480 rows, two workgroups of 256 rows, the second ragged
    (2, 5, 7, 6, 24),                  # 70 rows: one workgroup, the last tile ragged (HW % 4 != 0)
    (1, 363, 363, 2, 4),               # 131 769 rows: 515 workgroups' worth, capped at 512; rows per workgroup 258 -> 288
])
def test_pixel_linear_bwd(B, hh, ww, K, C):
    L, st = _L()
    HW = hh * ww

    def case(a):
        x, w = a.rand("x", B * HW, C), a.rand("w", K, C)
        dp, y = a.rand("dp", B, K, HW), a.rand("y", B, K, HW, uniform=True)
        part = a.scratch(L.vs_pixel_linear_bwd_partial_floats(B * HW, K, C))
        dx, dw, db = a.out(B * HW, C), a.out(K, C), a.out(K)
        N.check(L.vs_pixel_linear_bwd(N.ptr(dp), N.ptr(y), N.ptr(x), C, B, HW, C, N.ptr(w), K, N.ptr(dx), C, N.ptr(dw), N.ptr(db), N.ptr(part), st),
                "vs_pixel_linear_bwd")
        return [dx, dw, db]
    _contract(case)


# vs_pixel_bce_partial_doubles: 3 * chunks * B, chunks = ceil(HW / 1024) when HW % 4 == 0 (four pixels per lane), else ceil(HW / 256)
@pytest.mark.parametrize("B,K,HW", [
    (2, 17, 240),                      # the suite's smallest case: HW % 4 == 0, one chunk
    (2, 6, 35),                        # HW % 4 != 0: one pixel per lane, one ragged chunk
    (1, 3, 2050),                      # HW % 4 != 0: nine chunks of 256, the last holds two pixels
    (2, 3, 4100),                      # HW % 4 == 0: five chunks of 1024, the last holds four pixels
])
def test_pixel_bce(B, K, HW):
    L, st = _L()

    def case(a):
        preds = a.rand("preds", B, K, HW)
        if "masks" not in a.store:
            a.store["masks"] = (torch.rand(B, HW, generator=torch.Generator().manual_seed(1)) > 0.4).float().cuda()
            a.store["msgs"] = torch.randint(0, 2, (B, K - 1), generator=torch.Generator().manual_seed(2)).to(torch.int32).cuda()
        masks, msgs = a.inp(a.store["masks"]), a.inp(a.store["msgs"])
        part = a.scratch(L.vs_pixel_bce_partial_doubles(B, K, HW), torch.float64)
        dpr, loss = a.out(B, K, HW), a.out(2)
        N.check(L.vs_pixel_bce(N.ptr(preds), N.ptr(masks), N.ptr(msgs), B, B, K, HW, 1.5, 1.0, 0.5, N.ptr(dpr), N.ptr(part), N.ptr(loss), st), "vs_pixel_bce")
        return [dpr, loss]
    _contract(case)


# ====================================================================================================== vs_model_workspace_bytes
@pytest.fixture(scope="module")
def cmodels():
    from oracle.weights import make_state_dict, tiny_spec
    from tests._model import cfg_of
    from videoseal_amd.capi import CModel
    out = {}
    for which, spec, seed in (("tiny", tiny_spec(), 3),
                              ("tinyc", tiny_spec(yuv=False, in_ch=3, out_ch=3, dims=[18, 36, 54, 90], stem_stride=2, hidden=32, nbits=16), 4)):
        out[which] = (spec, CModel(cfg_of(spec), make_state_dict(spec, seed=seed)))
    return out


@pytest.mark.parametrize("which", ["tiny", "tinyc"])            # the image and the ChunkySeal-shaped models of test_model_level_c_api
@pytest.mark.parametrize("Fr,H,W,step", [(6, 96, 80, 2), (3, 50, 71, 1)])      # its video clip (one message, key frames), and odd frames in image mode
def test_model_embed_and_detect_inside_their_workspace(cmodels, which, Fr, H, W, step):
    from oracle.inputs import synthetic_frames, synthetic_msgs
    spec, cm = cmodels[which]
    L, h = cm._L, cm._h
    imgs = synthetic_frames(Fr, H, W, seed=33)
    msgs = synthetic_msgs(1 if step > 1 else Fr, spec.nbits, seed=33).to(torch.int32)

    def case(a):
        x, m = a.inp(imgs), a.inp(msgs)
        nb = int(L.vs_model_workspace_bytes(h, Fr, H, W, step))
        ws = a.scratch(nb, torch.uint8)
        assert ws.data_ptr() % 256 == 0                            # the alignment the header asks of the caller
        out, pw = a.out(Fr, 3, H, W), a.out(Fr, spec.out_ch, H, W)
        N.check(L.vs_model_embed(h, N.ptr(x), N.ptr(m), m.shape[0], Fr, H, W, step, 0, 1, 1, 0, N.ptr(out), N.ptr(pw), N.ptr(ws), nb, N.stream()),
                "vs_model_embed")
        nb2 = int(L.vs_model_workspace_bytes(h, Fr, H, W, 1))
        ws2 = a.scratch(nb2, torch.uint8)
        logits = a.out(Fr, spec.nbits + 1)
        N.check(L.vs_model_detect(h, N.ptr(out), Fr, H, W, 1, 0, N.ptr(logits), N.ptr(ws2), nb2, N.stream()), "vs_model_detect")
        return [out, pw, logits]
    _contract(case)
    # a workspace that is far too small is refused before anything is launched
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((Fr, 3, H, W), 3.0, device="cuda")
    code = L.vs_model_embed(h, N.ptr(imgs.cuda()), N.ptr(msgs.cuda()), msgs.shape[0], Fr, H, W, step, 0, 1, 1, 0, N.ptr(out), None, N.ptr(ws), 256, N.stream())
    torch.cuda.synchronize()
    assert code != 0 and bool((out == 3.0).all()) and bool((ws == 0).all())
