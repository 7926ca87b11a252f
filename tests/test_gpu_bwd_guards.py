"""Every backward entry point that takes no scratch (include/videoseal_hip.h from vs_pad_embed1 to vs_outc_tanh_bwd and from vs_resize_nchw_bwd
to vs_percep_mse_grad; the ones with a workspace are in tests/test_gpu_scratch_contracts.py, vs_clamp01_bwd / vs_mask_mul /
vs_nhwc_to_nchw_scaled / vs_patchify_s / vs_unpatch_s / vs_gaussian_blur_bwd in tests/test_gpu_entry_points.py) between red zones: inputs
between NaN bands, outputs between -7.0 bands, every buffer exactly as large as the header says -- parameter vectors included -- and the pad
lanes [C, ld) of the inputs zero, as the engine keeps them.  The result must equal the unguarded call bit for bit (a value read from a band
would make it NaN) and every band must survive.  Values are checked by the unit tests of tests/test_gpu_bwd*.py / test_gpu_train.py and, for the
U-Net glue that runs here for memory safety only (vs_relu_bwd, vs_pad_embed1, vs_reflect_fold1, vs_col2im3x3_reflect, vs_dilate2,
vs_im2col3x3_strided, vs_upcat2x_bwd, vs_msg_table_grad, vs_outc_tanh_bwd), by tests/test_gpu_unet_envelope.py on hard inputs; the
shapes here are ragged on purpose: rows no multiple of 4, W odd and below 4, C in {1, 3, 6, 130} with ld = 4 ceil(C / 4) and larger, 2 x 2
maps for the reflection kernels, one frame."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._gpu import _contract, _lib as _L, r4  # noqa: E402

from videoseal_amd import native as N  # noqa: E402

MODES = ("plain", "nan")
CL = [(1, 4), (3, 4), (6, 8), (130, 132), (6, 12), (130, 160)]          # (C, ld): ld = 4 ceil(C / 4) and larger
ROWS_CL = [(7, C, ld) for C, ld in CL] + [(301, 130, 132), (1, 3, 4)]


def _run(case):
    _contract(case, MODES)


# ---------------------------------------------------------------------------------------------------------- row-wise adjoints
@pytest.mark.parametrize("rows,C,ld", ROWS_CL)
def test_activation_adjoints(rows, C, ld):
    """vs_gelu_bwd, vs_relu_bwd, vs_act_bwd (every activation): z, dy, dz = [rows][ld]"""
    L, st = _L()

    def case(a):
        z, dy = a.rand("z", rows, ld, lanes=C), a.rand("dy", rows, ld, lanes=C)
        outs = [a.out(rows, ld) for _ in range(6)]
        N.check(L.vs_gelu_bwd(N.ptr(z), ld, N.ptr(dy), ld, rows, C, N.ptr(outs[0]), ld, st), "vs_gelu_bwd")
        N.check(L.vs_relu_bwd(N.ptr(z), ld, N.ptr(dy), ld, rows, C, N.ptr(outs[1]), ld, st), "vs_relu_bwd")
        for o, act in zip(outs[2:], (N.ACT_RELU, N.ACT_GELU, N.ACT_TANH, N.ACT_SILU)):
            N.check(L.vs_act_bwd(N.ptr(z), ld, N.ptr(dy), ld, rows, C, act, N.ptr(o), ld, st), "vs_act_bwd")
        return outs
    _run(case)


@pytest.mark.parametrize("rows,C,ld", [(7, 4, 4), (5, 20, 24), (3, 132, 132), (2, 260, 264), (1, 64, 64)])      # 4 / 16 / 64 lanes per row
def test_rmsnorm_act_bwd(rows, C, ld):
    """x, dy, dx, term = [rows][ld]; gamma = [C] (C % 4 == 0: read in whole float4)"""
    L, st = _L()

    def case(a):
        x, dy, gamma = a.rand("x", rows, ld, lanes=C, scale=1.5), a.rand("dy", rows, ld, lanes=C), a.rand("g", C, scale=0.3, shift=1.0)
        dx, term = a.out(rows, ld), a.out(rows, ld)
        N.check(L.vs_rmsnorm_act_bwd(N.ptr(x), rows, C, ld, N.ptr(gamma), N.ACT_SILU, N.ptr(dy), ld, N.ptr(dx), ld, N.ptr(term), ld, st), "vs_rmsnorm_act_bwd")
        return [dx, term]
    _run(case)


@pytest.mark.parametrize("C,ld", CL)
@pytest.mark.parametrize("B,HW", [(2, 7), (1, 1)])
def test_colmean_and_pool_gelu_bwd(B, HW, C, ld):
    """vs_colmean: x [B * HW][ld] -> out [B][ld]; vs_pool_gelu_bwd: z [B * HW][ld], dpooled [B][ld] -> dz [B * HW][ld]"""
    L, st = _L()

    def case(a):
        z, dp = a.rand("z", B * HW, ld, lanes=C), a.rand("dp", B, ld, lanes=C)
        pooled, dz = a.out(B, ld), a.out(B * HW, ld)
        N.check(L.vs_colmean(N.ptr(z), B, HW, ld, N.ptr(pooled), st), "vs_colmean")
        N.check(L.vs_pool_gelu_bwd(N.ptr(z), ld, N.ptr(dp), ld, B, HW, C, N.ptr(dz), ld, st), "vs_pool_gelu_bwd")
        return [pooled, dz]
    _run(case)


@pytest.mark.parametrize("rows,C,ld", ROWS_CL)
def test_bn_mean_rstd_and_bn_relu_bwd_apply(rows, C, ld):
    """vs_bn_mean_rstd: sums = 2 ld + 1 doubles -> mean, rstd = ld floats each (entries [C, ld) written as zeros).
    vs_bn_relu_bwd_apply: raw, dy, dx = [rows][ld]; mean, rstd, scale, shift = 4 ceil(C / 4) floats; sums = 2 * 4 ceil(C / 4) + 1 doubles"""
    L, st = _L()
    ldp = r4(C)

    def case(a):
        raw, dy = a.rand("raw", rows, ld, lanes=C, scale=1.5, shift=0.2), a.rand("dy", rows, ld, lanes=C)
        x64 = a.store["raw"].double()
        fsums = a.inp(torch.cat([x64.sum(0), (x64 * x64).sum(0), torch.tensor([float(rows)], dtype=torch.float64, device="cuda")]))
        mean, rstd = a.out(ld), a.out(ld)
        N.check(L.vs_bn_mean_rstd(N.ptr(fsums), C, ld, 1e-5, N.ptr(mean), N.ptr(rstd), st), "vs_bn_mean_rstd")
        mu, rs = a.rand("mean", ldp, scale=0.1, shift=0.2, lanes=C), a.rand("rstd", ldp, uniform=True, shift=0.5, lanes=C)
        sc, sh = a.rand("scale", ldp, uniform=True, shift=0.5, lanes=C), a.rand("shift", ldp, scale=0.3, lanes=C)
        if "bs" not in a.store:
            bs = torch.randn(2 * ldp + 1, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
            bs[-1] = rows
            a.store["bs"] = bs.cuda()
        bsums = a.inp(a.store["bs"])
        dx = a.out(rows, ld)
        N.check(L.vs_bn_relu_bwd_apply(N.ptr(raw), ld, N.ptr(dy), ld, N.ptr(mu), N.ptr(rs), N.ptr(sc), N.ptr(sh), 1, N.ptr(bsums), rows, C, N.ptr(dx), ld, st),
                "vs_bn_relu_bwd_apply")
        return [mean, rstd, dx]
    _run(case)


# ---------------------------------------------------------------------------------------------------------- NHWC map adjoints
MAPS = [(1, 2, 2, 1, 4), (2, 5, 3, 3, 4), (1, 3, 7, 6, 8), (1, 2, 3, 130, 132), (2, 3, 2, 6, 12)]         # B, H, W, C, ld (H, W >= 2: reflection)


@pytest.mark.parametrize("B,H,W,C,ld", MAPS)
def test_reflection_adjoints(B, H, W, C, ld):
    """vs_pad_embed1: dy [B H W][ld] -> canvas [B (H + 2) (W + 2)][ld]; vs_reflect_fold1: the reverse; vs_col2im3x3_reflect: dcols
    [B H W][9 ld] -> dx [B H W][ld]"""
    L, st = _L()

    def case(a):
        dy = a.rand("dy", B * H * W, ld, lanes=C)
        canvas = a.out(B * (H + 2) * (W + 2), ld)
        N.check(L.vs_pad_embed1(N.ptr(dy), B, H, W, ld, N.ptr(canvas), st), "vs_pad_embed1")
        dxp = a.rand("dxp", B * (H + 2) * (W + 2), ld, lanes=C)
        fold = a.out(B * H * W, ld)
        N.check(L.vs_reflect_fold1(N.ptr(dxp), B, H, W, ld, N.ptr(fold), st), "vs_reflect_fold1")
        if "dcols" not in a.store:
            t = torch.randn(B * H * W, 9, ld, generator=torch.Generator().manual_seed(4))
            t[..., C:] = 0
            a.store["dcols"] = t.reshape(B * H * W, 9 * ld).cuda()
        dcols = a.inp(a.store["dcols"])
        dx = a.out(B * H * W, ld)
        N.check(L.vs_col2im3x3_reflect(N.ptr(dcols), B, H, W, ld, N.ptr(dx), st), "vs_col2im3x3_reflect")
        return [canvas, fold, dx]
    _run(case)


@pytest.mark.parametrize("B,H,W,C,ld", MAPS + [(2, 3, 1, 3, 4), (1, 1, 1, 1, 4)])
def test_stride2_conv_adjoint_pieces(B, H, W, C, ld):
    """vs_dilate2: dy [B Ho Wo][ld] -> [B H W][ld]; vs_im2col3x3_strided (stride 1 and 2): x [B H W][ld] -> cols [B Ho Wo][9 ld]"""
    L, st = _L()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1

    def case(a):
        dy = a.rand("dy", B * Ho * Wo, ld, lanes=C)
        dil = a.out(B * H * W, ld)
        N.check(L.vs_dilate2(N.ptr(dy), B, Ho, Wo, ld, H, W, N.ptr(dil), st), "vs_dilate2")
        x = a.rand("x", B * H * W, ld, lanes=C)
        c1, c2 = a.out(B * H * W, 9 * ld), a.out(B * Ho * Wo, 9 * ld)
        N.check(L.vs_im2col3x3_strided(N.ptr(x), B, H, W, ld, 1, N.ptr(c1), st), "vs_im2col3x3_strided")
        N.check(L.vs_im2col3x3_strided(N.ptr(x), B, H, W, ld, 2, N.ptr(c2), st), "vs_im2col3x3_strided")
        return [dil, c1, c2]
    _run(case)


@pytest.mark.parametrize("B,H,W,C,ld", [(1, 2, 3, 1, 4), (2, 5, 1, 3, 4), (1, 3, 7, 6, 8), (1, 4, 5, 130, 132), (1, 1, 9, 6, 12)])
def test_dwconv7_forward_and_flipped(B, H, W, C, ld):
    """x, add, out = [B H W][ld]; w = [49][ld]; bias = [ld] (both read in whole float4 up to ld).  W = 1, 3, 5, 7, 9: the four-pixel strips of
    the kernel end ragged"""
    L, st = _L()
    rows = B * H * W

    def case(a):
        x, w, bias, add = a.rand("x", rows, ld, lanes=C), a.rand("w", 49, ld, lanes=C, scale=0.2), a.rand("b", ld, lanes=C), a.rand("add", rows, ld, lanes=C)
        y, dx = a.out(rows, ld), a.out(rows, ld)
        N.check(L.vs_dwconv7(N.ptr(x), B, H, W, C, ld, N.ptr(w), N.ptr(bias), 0, None, 0, N.ptr(y), ld, st), "vs_dwconv7")
        N.check(L.vs_dwconv7(N.ptr(x), B, H, W, C, ld, N.ptr(w), None, 1, N.ptr(add), ld, N.ptr(dx), ld, st), "vs_dwconv7")
        return [y, dx]
    _run(case)


@pytest.mark.parametrize("B,H,W,C,ld,P", [(2, 8, 12, 3, 4, 4), (1, 7, 9, 6, 8, 2), (1, 5, 3, 1, 4, 2), (1, 4, 4, 130, 132, 4)])
def test_patchify_and_unpatch(B, H, W, C, ld, P):
    """x, dx = [B H W][ld]; cols, dcols = [B (H / P) (W / P)][P * CP], CP = P ld rounded up to 16"""
    L, st = _L()
    Ho, Wo = H // P, W // P
    CP = (P * ld + 15) // 16 * 16

    def case(a):
        x = a.rand("x", B * H * W, ld, lanes=C)
        cols = a.out(B * Ho * Wo, P * CP)
        N.check(L.vs_patchify(N.ptr(x), B, H, W, ld, P, N.ptr(cols), st), "vs_patchify")
        dcols = a.rand("dcols", B * Ho * Wo, P * CP)
        dx = a.out(B * H * W, ld)
        N.check(L.vs_unpatch(N.ptr(dcols), B, H, W, ld, P, N.ptr(dx), st), "vs_unpatch")
        return [cols, dx]
    _run(case)


@pytest.mark.parametrize("B,H,W,C1,C2,ld1,ld2,hld", [(1, 1, 1, 4, 4, 4, 4, 8), (2, 3, 1, 4, 8, 8, 8, 12), (1, 2, 5, 8, 4, 8, 4, 16), (1, 7, 3, 4, 4, 4, 8, 8)])
def test_upcat2x_bwd(B, H, W, C1, C2, ld1, ld2, hld):
    """dhi [B 2H 2W][hi_ld] -> dx [B H W][ld1], dskip [B H W][ld2]"""
    L, st = _L()

    def case(a):
        dhi = a.rand("dhi", B * 4 * H * W, hld, lanes=C1 + C2)
        dx, dsk = a.out(B * H * W, ld1), a.out(B * H * W, ld2)
        N.check(L.vs_upcat2x_bwd(N.ptr(dhi), hld, B, H, W, C1, C2, 2 ** -0.5, N.ptr(dx), ld1, N.ptr(dsk), ld2, st), "vs_upcat2x_bwd")
        return [dx, dsk]
    _run(case)


# ---------------------------------------------------------------------------------------------------------- head, message table, output conv
@pytest.mark.parametrize("M,Nn,K,lda,ldb,ldc", [(3, 5, 7, 7, 5, 5), (1, 1, 1, 1, 1, 1), (10, 130, 3, 4, 132, 130), (300, 3, 6, 6, 3, 4)])
def test_matmul_small(M, Nn, K, lda, ldb, ldc):
    """A [M][lda], B [K][ldb], C [M][ldc]"""
    L, st = _L()

    def case(a):
        A, Bm = a.rand("A", M, lda), a.rand("B", K, ldb)
        Cc = a.out(M, ldc)
        N.check(L.vs_matmul_small(N.ptr(A), lda, N.ptr(Bm), ldb, M, Nn, K, N.ptr(Cc), ldc, st), "vs_matmul_small")
        return [Cc]
    _run(case)


@pytest.mark.parametrize("B,k,msg_rows", [(3, 9, 3), (5, 1, 1), (300, 17, 300), (1, 1, 1)])
def test_bce_logits(B, k, msg_rows):
    """preds, dpreds [B][k + 1]; msgs int32 [msg_rows][k]; loss [1]"""
    L, st = _L()

    def case(a):
        preds = a.rand("p", B, k + 1)
        if "m" not in a.store:
            a.store["m"] = torch.randint(0, 2, (msg_rows, k), generator=torch.Generator().manual_seed(5)).to(torch.int32).cuda()
        msgs = a.inp(a.store["m"])
        dp, loss = a.out(B, k + 1), a.out(1)
        N.check(L.vs_bce_logits(N.ptr(preds), N.ptr(msgs), msg_rows, B, k, 1.7, 0.5, N.ptr(dp), N.ptr(loss), st), "vs_bce_logits")
        return [dp, loss]
    _run(case)


@pytest.mark.parametrize("Bm,nbits,hidden", [(1, 1, 1), (3, 7, 12), (2, 16, 130)])
def test_msg_table_grad(Bm, nbits, hidden):
    """dlat [Bm][hidden], msgs int32 [Bm][nbits] -> dtable [2 nbits][hidden]"""
    L, st = _L()

    def case(a):
        dlat = a.rand("dlat", Bm, hidden)
        if "m" not in a.store:
            a.store["m"] = torch.randint(0, 2, (Bm, nbits), generator=torch.Generator().manual_seed(6)).to(torch.int32).cuda()
        msgs = a.inp(a.store["m"])
        dt = a.out(2 * nbits, hidden)
        N.check(L.vs_msg_table_grad(N.ptr(dlat), N.ptr(msgs), Bm, nbits, hidden, N.ptr(dt), st), "vs_msg_table_grad")
        return [dt]
    _run(case)


@pytest.mark.parametrize("B,rpf,C,Cout,dx_ld,use_tanh", [(1, 1, 1, 1, 4, 1), (2, 30, 8, 3, 8, 1), (1, 257, 6, 4, 8, 0), (2, 5, 130, 2, 132, 1)])
def test_outc_tanh_bwd(B, rpf, C, Cout, dx_ld, use_tanh):
    """delta, ddelta planar [B][Cout][rows_per_frame]; w [Cout][C]; dx [rows][dx_ld]; dv [rows][4]"""
    L, st = _L()
    rows = B * rpf

    def case(a):
        delta, dd, w = a.rand("delta", B, Cout, rpf, uniform=True, scale=1.6, shift=-0.8), a.rand("dd", B, Cout, rpf), a.rand("w", Cout, C)
        dx, dv = a.out(rows, dx_ld), a.out(rows, 4)
        N.check(L.vs_outc_tanh_bwd(N.ptr(delta), N.ptr(dd), rpf, B, C, N.ptr(w), Cout, use_tanh, N.ptr(dx), dx_ld, N.ptr(dv), st), "vs_outc_tanh_bwd")
        return [dx, dv]
    _run(case)


# ---------------------------------------------------------------------------------------------------------- shell and augmentation adjoints
@pytest.mark.parametrize("planes,H,W,oh,ow,aa", [
    (2, 5, 7, 9, 3, 1),                # oh above H, ow below W
    (1, 6, 4, 3, 11, 0),               # oh below H, ow above W
    (1, 8, 8, 2, 2, 1),                # both below (antialias: wide taps)
    (1, 3, 3, 7, 9, 0),                # both above
    (3, 1, 1, 4, 4, 1),                # a single source pixel
    (1, 70, 3, 5, 130, 1),             # W < 4 with more than one 64-column block of the output, H over one 4-row group
])
def test_resize_nchw_bwd(planes, H, W, oh, ow, aa):
    """dy [planes][oh][ow] -> dx [planes][H][W]; tmp = planes * oh * W floats"""
    L, st = _L()

    def case(a):
        dy = a.rand("dy", planes, oh, ow)
        dx, tmp = a.out(planes, H, W), a.out(planes * oh * W)
        N.check(L.vs_resize_nchw_bwd(N.ptr(dy), N.ptr(dx), planes, H, W, oh, ow, aa, N.ptr(tmp), st), "vs_resize_nchw_bwd")
        return [dx, tmp]
    _run(case)


@pytest.mark.parametrize("Fr,H,W,Cd,hmap,dpreds,clamp", [(1, 3, 5, 1, True, False, 1), (2, 7, 3, 3, False, True, 1), (1, 1, 1, 3, True, True, 0),
                                                          (2, 9, 29, 1, True, True, 1)])
def test_embed_tail_bwd(Fr, H, W, Cd, hmap, dpreds, clamp):
    """imgs, d_imgs_w [F][3][H][W]; preds, d_preds_w, g_full [F][Cd][H][W]; hmap_full [F][H][W]"""
    L, st = _L()

    def case(a):
        imgs, preds = a.rand("imgs", Fr, 3, H, W, uniform=True), a.rand("preds", Fr, Cd, H, W, scale=0.3)
        hm = a.rand("hm", Fr, H, W, uniform=True) if hmap else None
        dw = a.rand("dw", Fr, 3, H, W)
        dpw = a.rand("dpw", Fr, Cd, H, W) if dpreds else None
        g = a.out(Fr, Cd, H, W)
        N.check(L.vs_embed_tail_bwd(N.ptr(imgs), N.ptr(preds), N.ptr(hm), N.ptr(dw), N.ptr(dpw), Fr, H, W, Cd, clamp, 1.0, 0.8, N.ptr(g), st), "vs_embed_tail_bwd")
        return [g]
    _run(case)


@pytest.mark.parametrize("Fr,Cd,Sh,Sw,step,vm,hmap", [(1, 1, 3, 5, 1, 0, True), (5, 3, 4, 4, 2, 0, False), (5, 1, 4, 4, 2, 1, True), (7, 3, 3, 3, 3, 2, True),
                                                      (4, 1, 2, 2, 4, 2, False), (3, 1, 9, 29, 1, 2, True)])
def test_tail_key_reduce(Fr, Cd, Sh, Sw, step, vm, hmap):
    """g_low [F][Cd][S_h][S_w], hmap_low [F][S_h][S_w] -> d_delta [total_key][Cd][S_h][S_w], total_key = ceil(F / step)"""
    L, st = _L()
    nkey = (Fr + step - 1) // step

    def case(a):
        g = a.rand("g", Fr, Cd, Sh, Sw)
        hm = a.rand("hm", Fr, Sh, Sw, uniform=True) if hmap else None
        dd = a.out(nkey, Cd, Sh, Sw)
        N.check(L.vs_tail_key_reduce(N.ptr(g), N.ptr(hm), Fr, Cd, Sh, Sw, step, vm, nkey, N.ptr(dd), st), "vs_tail_key_reduce")
        return [dd]
    _run(case)


@pytest.mark.parametrize("planes,H,W,i0,j0,h,w,flip", [
    (3, 9, 7, 2, 1, 7, 6, 0),          # the crop touches the last row and the last column
    (1, 5, 3, 0, 0, 5, 3, 1),          # the whole frame, mirrored
    (2, 4, 4, 1, 1, 2, 2, 1),          # interior window
    (1, 1, 1, 0, 0, 1, 1, 0),
    (1, 9, 29, 8, 28, 1, 1, 1),        # a one-pixel window in the last corner
])
def test_aug_crop_flip_bwd(planes, H, W, i0, j0, h, w, flip):
    """dy [planes][h][w] -> dx [planes][H][W]"""
    L, st = _L()

    def case(a):
        dy = a.rand("dy", planes, h, w)
        dx = a.out(planes, H, W)
        N.check(L.vs_aug_crop_flip_bwd(N.ptr(dy), N.ptr(dx), planes, H, W, i0, j0, h, w, flip, st), "vs_aug_crop_flip_bwd")
        return [dx]
    _run(case)


@pytest.mark.parametrize("op", [0, 2, 3, 4])                # brightness, saturation, hue, grayscale (contrast takes a scratch: the contracts suite)
@pytest.mark.parametrize("Fr,H,W", [(1, 3, 5), (2, 9, 29)])
def test_aug_color_bwd_without_scratch(Fr, H, W, op):
    """x, dy, dx [F][3][H][W]; means and scratch may be NULL for every op but contrast"""
    L, st = _L()

    def case(a):
        x, dy = a.rand("x", Fr, 3, H, W, uniform=True), a.rand("dy", Fr, 3, H, W)
        dx = a.out(Fr, 3, H, W)
        N.check(L.vs_aug_color_bwd(N.ptr(x), N.ptr(dy), N.ptr(dx), Fr, H, W, op, 0.2 if op == 3 else 1.3, None, None, st), "vs_aug_color_bwd")
        return [dx]
    _run(case)


@pytest.mark.parametrize("n_src,idx,fsz", [(4, [0, 0, 2, 3, 3, 3], 35), (1, [0], 1), (3, [2, 2], 261), (2, [1, 0, 1], 7)])
def test_aug_gather_frames_bwd(n_src, idx, fsz):
    """dy [n_out][frame_floats]; start int32 [n_src + 1], outs int32 [n_out] (CSR of the outputs that copied each source frame) -> dx
    [n_src][frame_floats]; a source frame nobody copied gets zeros"""
    L, st = _L()
    lists = [[o for o, f in enumerate(idx) if f == s] for s in range(n_src)]
    start, outs = [0], []
    for l in lists:
        outs += l
        start.append(len(outs))

    def case(a):
        dy = a.rand("dy", len(idx), fsz)
        st_t, ou_t = a.inp(torch.tensor(start, dtype=torch.int32)), a.inp(torch.tensor(outs, dtype=torch.int32))
        dx = a.out(n_src, fsz)
        N.check(L.vs_aug_gather_frames_bwd(N.ptr(dy), N.ptr(st_t), N.ptr(ou_t), N.ptr(dx), n_src, fsz, st), "vs_aug_gather_frames_bwd")
        return [dx]
    _run(case)


@pytest.mark.parametrize("Fr,fsz,hw,alpha", [(1, 35, 3, 0.5), (5, 261, 1, 0.3), (3, 7, 5, 1.0), (4, 1, 0, 0.7)])      # F = 1 and half_window >= F included
def test_aug_window_average_bwd(Fr, fsz, hw, alpha):
    """dy, dx [F][frame_floats]"""
    L, st = _L()

    def case(a):
        dy = a.rand("dy", Fr, fsz)
        dx = a.out(Fr, fsz)
        N.check(L.vs_aug_window_average_bwd(N.ptr(dy), N.ptr(dx), Fr, fsz, hw, alpha, st), "vs_aug_window_average_bwd")
        return [dx]
    _run(case)


def _warp_inverse(kind, t, H, W, oh, ow):
    """the 3 x 3 map from input to output pixel-centre coordinates that bounds the adjoint's search (videoseal_amd.autograd.WarpFn)"""
    if kind == 0:
        M = np.array([[0.5 * W * t[0], 0.5 * W * t[1], 0.5 * W * (t[2] + 1.0 - 0.5 * ow * t[0] - 0.5 * oh * t[1])],
                      [0.5 * H * t[3], 0.5 * H * t[4], 0.5 * H * (t[5] + 1.0 - 0.5 * ow * t[3] - 0.5 * oh * t[4])], [0.0, 0.0, 1.0]], dtype=np.float64)
    else:
        M = np.array([[W / ow * t[0], W / ow * t[1], W / ow * t[2]], [H / oh * t[3], H / oh * t[4], H / oh * t[5]], [t[6], t[7], 1.0]], dtype=np.float64)
    inv = np.linalg.inv(M)
    return [float(v) for v in (inv / inv[2, 2]).reshape(-1)]


@pytest.mark.parametrize("kind,bilinear", [(0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("planes,H,W,oh,ow", [(2, 9, 13, 9, 13), (1, 3, 2, 5, 7), (1, 1, 1, 1, 1), (1, 10, 37, 7, 3)])
def test_aug_warp_bwd(planes, H, W, oh, ow, kind, bilinear):
    """dy [planes][oh][ow] -> dx [planes][H][W]; coeffs and inv are host arrays.  A 20-degree rotation (nearest / bilinear) and a mild perspective"""
    L, st = _L()
    c, s = float(np.cos(np.radians(20.0))), float(np.sin(np.radians(20.0)))
    t = [c / (0.5 * W), s / (0.5 * W), 0.0, -s / (0.5 * H), c / (0.5 * H), 0.0] if kind == 0 else [1.05, 0.02, -0.5, 0.01, 0.97, 0.3, 1e-3, -5e-4]
    inv = _warp_inverse(kind, t, H, W, oh, ow)
    ct, ci = (ctypes.c_float * len(t))(*t), (ctypes.c_float * 9)(*inv)

    def case(a):
        dy = a.rand("dy", planes, oh, ow)
        dx = a.out(planes, H, W)
        N.check(L.vs_aug_warp_bwd(N.ptr(dy), N.ptr(dx), planes, H, W, oh, ow, kind, ct, bilinear, ci, st), "vs_aug_warp_bwd")
        return [dx]
    _run(case)


@pytest.mark.parametrize("Fr,H,W,yuv", [(1, 1, 1, 0), (2, 9, 29, 1), (1, 3, 5, 1)])
def test_percep_mse_grad(Fr, H, W, yuv):
    """imgs, imgs_w, d_imgs_w [F][3][H][W]"""
    L, st = _L()

    def case(a):
        x, y = a.rand("x", Fr, 3, H, W, uniform=True), a.rand("y", Fr, 3, H, W, uniform=True)
        d = a.out(Fr, 3, H, W)
        N.check(L.vs_percep_mse_grad(N.ptr(x), N.ptr(y), Fr, H, W, yuv, 0.7, N.ptr(d), st), "vs_percep_mse_grad")
        return [d]
    _run(case)
