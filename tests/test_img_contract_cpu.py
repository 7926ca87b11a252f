"""The envelope of tests/test_gpu_img_envelope.py has teeth: on the very frames and shapes the GPU file uses, seeded fp32 emulations (plain torch,
tests/_img_ref.py) of the defects that the older fixed-tolerance and form-against-form tests accept fall outside  max(yardstick, 2^-24) x 8 on at
least one named frame kind -- the yardstick's own ratio is 1, so no IMG_FP64_MARGIN up to the cap admits them -- while the correct fp32 formula
stays inside; the restated formulas agree with ATen in float64; and the two conditions on the candidate rules (share of ambiguous pixels) hold on
the float64 references alone.  Nothing here needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import _envelope as E
from tests import _img_ref as R

F32, F64 = torch.float32, torch.float64


def _teeth(tag, ref64_by_kind, yard_by_kind, bad_by_kind):
    """prints every figure; True when the defect is outside the envelope on at least one frame kind; the yardstick is inside with ratio 1 by construction"""
    hit = []
    for kind in ref64_by_kind:
        yard = E.frame_err(yard_by_kind[kind], ref64_by_kind[kind])
        bad = E.frame_err(bad_by_kind[kind], ref64_by_kind[kind])
        print(f"TEETH {tag:<60s} {kind:<8s} yardstick {yard:.3e}  defect {bad:.3e}")
        assert not E.outside(yard, yard)
        if E.outside(bad, yard):
            hit.append(kind)
    return hit


# ------------------------------------------------------------------------------------------------------------------------ resize
def _aa_cases():
    return [c for c in R.RESIZE_CASES if not c[6]]


@pytest.mark.parametrize("case", _aa_cases(), ids=[c[0] for c in _aa_cases()])
def test_resize_restatement_is_atens_formula_and_the_yardstick_is_small(case):
    tag, H, W, oh, ow, aa, _ = case
    for kind, x in R.hard_frames(H, W).items():
        r64, r32 = R.resize_ref(x, (oh, ow), aa)
        at = F.interpolate(x.double(), size=(oh, ow), mode="bilinear", align_corners=False, antialias=bool(aa))
        assert (r64 - at).abs().max() < 1e-13, (tag, kind)
        # fp32 coordinates times the local gradient: 2^-24 x (coordinate <= 165) x (gradient <= 1 per pixel) = 1e-5 at most
        assert E.frame_err(r32, r64) < 2e-5, (tag, kind)


def test_a_resampler_returns_a_constant_frame():
    for tag, H, W, oh, ow, aa, _ in _aa_cases():
        x = R.hard_frames(H, W)["const"]
        r64 = R.resize(x, (oh, ow), aa, F64)
        assert (r64[0] - R.CONST[0]).abs().max() < 1e-7 and (r64[1] - R.CONST[1]).abs().max() < 1e-7, tag          # (0.3f is 1e-8 from 0.3)


RESIZE_DEFECTS = [
    # (defect, axis, cases it must be caught on: (H, W, oh, ow, aa))
    ("shift_last", "x", [(93, 118, 29, 37, 1), (96, 128, 30, 40, 1), (5, 7, 64, 64, 1), (31, 45, 64, 64, 0), (93, 118, 130, 165, 1)]),
    ("unclipped", "x", [(93, 118, 29, 37, 1), (70, 66, 13, 17, 1), (5, 7, 64, 64, 1), (93, 118, 130, 165, 1)]),
    ("unclipped", "y", [(93, 118, 29, 37, 1), (100, 128, 25, 32, 1)]),
    ("nohalf", "x", [(93, 118, 29, 37, 1), (5, 7, 64, 64, 0), (31, 45, 64, 64, 0), (1, 9, 4, 33, 0)]),
    # a window holds floor(2 scale) or floor(2 scale) + 1 taps: up to 4 : 1 (the 3.9 : 1 and 4 : 1 cases included) never more than 8, so nothing is
    # dropped there and the emulation is the identity; the cases beyond 4 : 1 are the ones with a ninth tap
    ("drop9", "x", [(64, 64, 1, 1, 1)]),          # (70 x 66 -> 13 x 17 is 3.9 : 1 in x, 5.4 : 1 in y)
    ("drop9", "y", [(70, 66, 13, 17, 1), (200, 12, 16, 3, 1)]),
]


@pytest.mark.parametrize("defect,axis,cases", RESIZE_DEFECTS, ids=[f"{d}-{a}" for d, a, _ in RESIZE_DEFECTS])
def test_resize_defects_fall_outside_the_envelope(defect, axis, cases):
    for H, W, oh, ow, aa in cases:
        fr = R.hard_frames(H, W)
        r64 = {k: R.resize(x, (oh, ow), aa, F64) for k, x in fr.items()}
        r32 = {k: R.resize(x, (oh, ow), aa, F32) for k, x in fr.items()}
        bad = {k: R.resize(x, (oh, ow), aa, F32, defect=defect, defect_axis=axis) for k, x in fr.items()}
        hit = _teeth(f"resize {defect}/{axis} {H}x{W}->{oh}x{ow} aa={aa}", r64, r32, bad)
        assert hit, (defect, axis, H, W, oh, ow, aa)
        if defect in ("unclipped", "drop9"):          # a normalisation defect shows on the constant frame (noise alone may hide it)
            assert "const" in hit, (defect, hit)
        if defect == "shift_last":                    # the border taps themselves: the impulse frame (ones on the last column / row)
            assert "impulse" in hit, (defect, hit)


# ------------------------------------------------------------------------------------------------------------------------ JND
@pytest.mark.parametrize("H,W", R.JND_SHAPES)
def test_jnd_conditions_and_defects(H, W):
    hit = {"thr": [], "gy": []}
    for kind, x in R.jnd_frames(H, W).items():
        own, other, amb, y32 = R.jnd_ref(x)
        share = float(amb.float().mean())
        yard = E.cand_err(y32, own, other, amb)
        print(f"TEETH jnd {H}x{W} {kind:<8s} ambiguous share {share:.4f}  yardstick {yard:.3e}")
        assert share <= R.JND_SHARE, (kind, share)                                   # condition on the float64 reference alone
        assert yard < 2e-6                                                           # no fp32 branch flips outside the band
        for name, kw in (("thr", dict(thr=128.0)), ("gy", dict(gy_sum=True))):
            bad = E.cand_err(R.jnd(x, F32, **kw)[0], own, other, amb)
            print(f"TEETH jnd {H}x{W} {kind:<8s} {name} defect {bad:.3e}")
            if E.outside(bad, yard):
                hit[name].append(kind)
    if min(H, W) >= 32:                      # (on 5 x 7 no window of the jump frame need fall between 127 and 128)
        assert "jump" in hit["thr"], hit
    assert "noise" in hit["gy"] and "checker" in hit["gy"], hit


def test_a_jnd_threshold_at_128_shows_only_on_frames_at_the_jump():
    """why `jump` is a frame kind of its own: a threshold at 128 instead of 127 changes nothing on a black frame (bit for bit) and moves the heat-map
    of the jump frame by more than 1e-3 -- the bound that tests/test_gpu_kernels.py::test_embed_tail_forms_are_bit_identical grants two kernel
    forms on that frame, 8 % of the jump itself (3 / 255)"""
    x = R.jnd_frames(70, 101)["jump"]
    good, bad = R.jnd(x, F32)[0], R.jnd(x, F32, thr=128.0)[0]
    d = float((good - bad).abs().max())
    print(f"GAP jnd threshold 128 on the jump frame: max difference {d:.3e}")
    assert d > 1e-3
    xn = R.jnd_frames(70, 101)["black"]
    assert torch.equal(R.jnd(xn, F32)[0], R.jnd(xn, F32, thr=128.0)[0])


# ------------------------------------------------------------------------------------------------------------------------ embed tail
def _tail(case):
    tag, Fn, H, W, S, Cd, low, want_pw, cfg = case
    delta, hm = R.tail_inputs(Fn, Cd, S, cfg["step"])
    cfg = dict(cfg, total_key=cfg["total_key"] or delta.shape[0])
    return delta, (hm if low else None), cfg


@pytest.mark.parametrize("case", R.TAIL_CASES, ids=[c[0] for c in R.TAIL_CASES])
def test_tail_conditions_and_defects(case):
    tag, Fn, H, W = case[:4]
    delta, hm, cfg = _tail(case)
    for kind, imgs in R.tail_frames(Fn, H, W).items():
        own, other, amb, y32 = R.tail_ref(imgs, delta, hm, cfg)
        share = float(amb.float().mean())
        yard = E.cand_err(y32[0], own[0], other[0], amb)
        print(f"TEETH tail {tag:<34s} {kind:<6s} ambiguous share {share:.4f}  yardstick {yard:.3e}")
        assert share <= R.JND_SHARE and yard < 1e-5
        if cfg["mode"] == 2:
            bad = R.tail_ref(imgs, delta, hm, cfg, tail_weight_defect=True)[3]
            e = E.cand_err(bad[0], own[0], other[0], amb)
            print(f"TEETH tail {tag:<34s} {kind:<6s} key weight j/step {e:.3e}")
            assert E.outside(e, yard)
        if cfg["sw"] > 1:
            bad = R.tail_ref(imgs, delta, hm, cfg, no_clamp=True)[3]
            e = E.cand_err(bad[0], own[0], other[0], amb)
            print(f"TEETH tail {tag:<34s} {kind:<6s} clamp skipped {e:.3e}")
            assert E.outside(e, yard)
            assert float(bad[0].min()) < 0 and float(bad[0].max()) > 1          # both clamps act


# ------------------------------------------------------------------------------------------------------------------------ colour ops
def test_colour_defects_fall_outside_the_envelope():
    x = R.hard_pixels()
    noise = torch.rand(3, 3, 300, 300, generator=torch.Generator().manual_seed(9)) * torch.tensor([1.0, 0.7, 0.4]).view(3, 1, 1, 1)

    def err(op, f, inp, **kw):
        r64 = R.color_op(inp, op, f, F64)
        yard = E.frame_err(R.color_op(inp, op, f, F32), r64)
        bad = E.frame_err(R.color_op(inp, op, f, F32, **kw), r64)
        print(f"TEETH colour op {op} factor {f} {kw}: yardstick {yard:.3e}  defect {bad:.3e}")
        assert yard < 4e-6
        return E.outside(bad, yard)
    for f in (-0.5, -0.4, -0.1):
        assert err(R.OP_HUE, f, x, c_fmod=True)
    for op in (R.OP_SATURATION, R.OP_CONTRAST):
        for f in (0.5, 1.5, 2.0):
            assert err(op, f, x, gray0=0.299), (op, f)
    assert err(R.OP_SATURATION, 0.0, x, gray0=0.299)
    for f in (0.1, 0.5, 1.5, 2.0):
        assert err(R.OP_CONTRAST, f, noise, shared_mean=True)
        assert err(R.OP_CONTRAST, f, x, shared_mean=True)


# ------------------------------------------------------------------------------------------------------------------------ blur
@pytest.mark.parametrize("k", R.BLUR_KS)
def test_blur_defects_fall_outside_the_envelope(k):
    for H, W in ((93, 118), (k // 2 + 1, 40), (40, k // 2 + 1)):
        fr = R.hard_frames(H, W)
        r64 = {n: R.gaussian_blur(x, k, F64) for n, x in fr.items()}
        r32 = {n: R.gaussian_blur(x, k, F32) for n, x in fr.items()}
        if (H, W) == (93, 118):          # the restatement is oracle/augment.py's (k x k kernel, fp32): to rounding
            from oracle import augment as A
            assert (r32["noise"] - A.gaussian_blur(fr["noise"], k)).abs().max() < 2e-6
        hit = _teeth(f"blur k={k} {H}x{W} symmetric padding", r64, r32, {n: R.gaussian_blur(x, k, F32, pad_mode="symmetric") for n, x in fr.items()})
        assert "impulse" in hit and "ramp" in hit, hit
        hit = _teeth(f"blur k={k} {H}x{W} sigma from k", r64, r32, {n: R.gaussian_blur(x, k, F32, sigma_from_k=True) for n, x in fr.items()})
        assert "noise" in hit and "checker" in hit, hit
        for v in r64["const"]:           # a constant frame comes back
            assert (v - v.mean()).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------ warp
def _warp_cases():
    out = [("rot", a, H, W, 0, R.rotate_coeffs(a, H, W)) for H, W in R.ROT_SHAPES for a in R.ROT_ANGLES]
    out += [("persp", s, H, W, 1, R.perspective_coeffs(*R.perspective_points(W, H, s))) for H, W, s in R.PERSP_CASES]
    return out


def test_nearest_warp_conditions_and_the_fp32_oracle_obeys_the_candidate_rule():
    worst = 0.0
    for name, p, H, W, kind, co in _warp_cases():
        x = R.hard_frames(H, W)["noise"][0]
        cand, amb = R.nearest_candidates(x, kind, co, H, W)
        share = float(amb.float().mean())
        ix64, iy64 = R.warp_coords(kind, co, H, W, H, W, F64)
        ix32, iy32 = R.warp_coords(kind, co, H, W, H, W, F32)
        inside = (ix64 > -2) & (ix64 < W + 1) & (iy64 > -2) & (iy64 < H + 1)
        dist = float(torch.maximum((ix32.double() - ix64).abs(), (iy32.double() - iy64).abs())[inside].max())
        worst = max(worst, dist / R.nearest_delta(H, W))
        print(f"TEETH nearest {name} {p} {H}x{W}: ambiguous share {share:.4f}  fp32 grid within {dist:.2e} px (delta {R.nearest_delta(H, W):.2e})")
        assert share <= R.ROT_SHARE, (name, p, H, W, share)                      # condition on the float64 reference alone
        assert R.nearest_check(R.warp_nearest32(x, kind, co, H, W), cand) == 0   # the fp32 oracle: zero mismatches outside the band
    assert worst < 0.5         # the band is at least twice the fp32 grid's distance from the float64 grid


def test_nearest_warp_quarter_turn_of_an_odd_by_even_frame_is_all_ties():
    """Rotate.forward turns by 90 degrees with expand=True: an odd x even frame comes out one pixel larger each way and every source coordinate
    sits on a .5 boundary (to the 1e-7 px that the fp32 coefficients are off), so only the candidate rule applies; even x even: no pixel is ambiguous"""
    for (H, W), all_ties in zip(R.ROT90_SHAPES, (True, False)):
        oh, ow = R.rot90_size(H, W)
        assert (oh, ow) == ((W + 1, H + 1) if all_ties else (W, H))
        x = R.hard_frames(H, W)["noise"][0]
        co = R.rotate_coeffs(90, H, W)
        cand, amb = R.nearest_candidates(x, 0, co, oh, ow)
        ix, iy = R.warp_coords(0, co, H, W, oh, ow, F64)
        if all_ties:
            assert ((ix - ix.floor() - 0.5).abs() < 1e-6).all() and ((iy - iy.floor() - 0.5).abs() < 1e-6).all()
        assert float(amb.float().mean()) == (1.0 if all_ties else 0.0)
        assert R.nearest_check(R.warp_nearest32(x, 0, co, oh, ow), cand) == 0
        if not all_ties:
            assert torch.equal(cand[0].float(), torch.rot90(x, 1, dims=(-2, -1)))


def test_nearest_warp_rounding_half_away_from_zero_violates_the_exact_rule_on_exact_ties():
    """A tie inside the band admits both neighbours by construction, so the candidate rule alone cannot tell nearbyint from roundf: the case whose
    arithmetic is exact in both precisions (R.HALF_PIXEL_SHIFT: every coordinate an exact tie, no band) does -- there the float64 choice is
    grid_sample's half-to-even and rounding half away from zero picks the other pixel"""
    co, H, W = R.HALF_PIXEL_SHIFT
    x = R.hard_frames(H, W)["noise"][0]
    ix, iy = R.warp_coords(0, co, H, W, H, W, F64)
    ix32, iy32 = R.warp_coords(0, co, H, W, H, W, F32)
    assert torch.equal(ix, torch.arange(W, dtype=F64)[None] + 0.5 + 0 * iy) and torch.equal(ix32.double(), ix) and torch.equal(iy32.double(), iy)
    cand, amb = R.nearest_candidates(x, 0, co, H, W, delta=0.0)
    assert not amb.any()
    assert R.nearest_check(R.warp_nearest32(x, 0, co, H, W), cand) == 0
    assert R.nearest_check(R.warp_nearest32(x, 0, co, H, W, half_away=True), cand) > 0
    ref = one = F.grid_sample(x[None], torch.stack(torch.broadcast_tensors(*R.warp_grid(0, co, H, W, H, W, F32)), -1)[None], mode="nearest",
                              padding_mode="zeros", align_corners=False)[0]
    assert torch.equal(one, cand[0].float()) and ref is one          # ATen's own nearest pick is the float64 choice here


def test_bilinear_warp_defect_falls_outside_the_envelope():
    for name, p, H, W, kind, co in _warp_cases():
        fr = R.hard_frames(H, W)
        r64 = {n: R.warp_bilinear(x[0], kind, co, H, W, F64) for n, x in fr.items()}
        r32 = {n: R.warp_bilinear(x[0], kind, co, H, W, F32) for n, x in fr.items()}
        bad = {n: R.warp_bilinear(x[0], kind, co, H, W, F32, clamp_taps=True) for n, x in fr.items()}
        hit = _teeth(f"bilinear warp {name} {p} {H}x{W} clamped taps", r64, r32, bad)
        assert "const" in hit, (name, p, H, W, hit)


# ------------------------------------------------------------------------------------------------------------------------ pointwise
def test_window_average_expression_is_atens():
    x = torch.rand(5, 3, 7, 9, generator=torch.Generator().manual_seed(2))
    for hw, alpha in ((0, 0.4), (1, 1.0), (4, 0.6)):
        ref = x.clone()
        for i in range(5):
            a, b = max(0, i - hw), min(5, i + hw + 1)
            ref[i] = (1 - alpha) * x[i] + alpha * torch.mean(x[a:b], dim=0)
        assert (R.window_average(x, hw, alpha) - ref).abs().max() <= 1.2e-7
