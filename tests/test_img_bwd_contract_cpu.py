"""The envelope of tests/test_gpu_img_bwd_envelope.py has teeth: on the very inputs the GPU file uses, seeded fp32 emulations (plain torch,
tests/_img_bwd_ref.py) of the defects that the fixed-tolerance adjoint tests of tests/test_gpu_train.py accept fall outside
max(yardstick, 2^-24) x 8 on at least one line -- no IMG_BWD_FP64_MARGIN up to the cap admits them -- while the unseeded emulation stays inside;
the closed forms and restatements agree with autograd of the _img_ref formulas in float64; and the conditions on the flagged shares hold on the
float64 references alone.  Nothing here needs a GPU."""
import pytest
import torch

from tests import _envelope as E
from tests import _img_bwd_ref as B
from tests import _img_ref as R

F32, F64 = torch.float32, torch.float64


def _teeth(tag, lines):
    """lines: (name, yardstick error, unseeded emulation's error, seeded defect's error); prints them; the names on which the defect is outside"""
    hit = []
    for name, yard, good, bad in lines:
        print(f"TEETH {tag:<56s} {name:<9s} yardstick {yard:.3e}  emulation {good:.3e}  defect {bad:.3e}")
        assert not E.outside(good, yard), (tag, name, good, yard)
        if E.outside(bad, yard):
            hit.append(name)
    return hit


# ------------------------------------------------------------------------------------------------------------------------ resize
def _resize_lines(H, W, oh, ow, aa, defect):
    lines = []
    for kind, dy in B.hard_dy((2, 3, oh, ow)).items():
        r64, r32 = B.adjoint_pair(lambda t, dt: R.resize(t, (oh, ow), aa, dt), torch.zeros(2, 3, H, W), dy)
        lines.append((kind, E.frame_err(r32, r64), E.frame_err(B.resize_adjoint32(dy, H, W, aa), r64),
                      E.frame_err(B.resize_adjoint32(dy, H, W, aa, defect), r64)))
    return lines


@pytest.mark.parametrize("case", B.RESIZE_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_adjoint_range_is_a_superset_on_every_case(case):
    """the emulation restricted to adjoint_range equals the unrestricted transpose: no contributor is outside the range"""
    H, W, oh, ow, aa = case
    assert all(not E.outside(good, yard) for _, yard, good, _ in _resize_lines(H, W, oh, ow, aa, None))


def test_the_i_le_1_rule_of_adjoint_range_never_changes_the_range():
    """`!antialias && i <= 1 -> l = 0` cannot be given teeth: for i <= 1 the lower bound ((i + 0.5) - 1 - 1.5) / scale - 0.5 is negative for every
    scale, so the clamp at 0 already yields 0 and an emulation without the rule is the same operator.  Pinned here so that a change of the slack
    that makes the rule matter is noticed."""
    for n_in, n_out in [(h, oh) for h, w, oh, ow, aa in B.RESIZE_BWD_CASES] + [(w, ow) for h, w, oh, ow, aa in B.RESIZE_BWD_CASES] + [(2, 1), (3, 1000), (1000, 3)]:
        a, b = B.adjoint_range(n_in, n_out, 0), B.adjoint_range(n_in, n_out, 0, "no_i1")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (n_in, n_out)


def test_adjoint_range_defects_fall_outside_the_envelope():
    """removing the slack alone loses no contributor (|i + 0.5 - centre| <= support is the forward window itself; a tap at its edge has weight 0),
    so the seeded defect is the slack-free range between pixel corners"""
    for H, W, oh, ow, aa in B.RESIZE_BWD_CASES:
        assert all(not E.outside(bad, yard) for _, yard, _, bad in _resize_lines(H, W, oh, ow, aa, "slack_only")), (H, W, oh, ow, aa)
    for H, W, oh, ow, aa in ((93, 118, 29, 37, 1), (5, 7, 64, 64, 1), (31, 45, 64, 64, 0)):
        assert _teeth(f"resize {H}x{W}->{oh}x{ow} aa={aa}, range without slack", _resize_lines(H, W, oh, ow, aa, "no_slack")), (H, W)


# ------------------------------------------------------------------------------------------------------------------------ blur
def _blur_lines(k, H, W, defect):
    lines = []
    for kind, dy in B.hard_dy((2, 3, H, W)).items():
        r64, r32 = B.adjoint_pair(lambda t, dt: R.gaussian_blur(t, k, dt), torch.zeros(2, 3, H, W), dy)
        lines.append((kind, E.frame_err(r32, r64), E.frame_err(B.blur_adjoint32(dy, k), r64), E.frame_err(B.blur_adjoint32(dy, k, defect), r64)))
    return lines


def test_blur_fold_defects_fall_outside_the_envelope():
    for k, shapes in B.BLUR_BWD_SHAPES.items():
        for H, W in shapes:
            hit = _teeth(f"blur k={k} {H}x{W} without the far-side fold", _blur_lines(k, H, W, "no_far"))
            assert "ones" in hit and "impulse" in hit, (k, H, W, hit)
        H, W = shapes[0]                                  # one axis at r + 1: both folds land on the same pixels
        hit = _teeth(f"blur k={k} {H}x{W} one fold only at n = r + 1", _blur_lines(k, H, W, "one_fold"))
        assert hit or k == 3, (k, H, W)                   # (k = 3, n = 2: the near fold lands on u = 1, the far one on u = 0 -- no pixel takes both)


# ------------------------------------------------------------------------------------------------------------------------ warp
def _nearest_index(kind, co, H, W, oh, ow):
    """the fp32 oracle's source index of every output pixel (stands in for the HIP forward on the index image)"""
    idx = torch.arange(H * W, dtype=F32).view(1, H, W) + 1
    return R.warp_nearest32(idx, kind, co, oh, ow)[0] - 1


def test_warp_search_box_defect_falls_outside_and_the_whole_branch_runs():
    """the +-1.5 margin alone cannot be given teeth: without it the box of the 2 x 2 footprint's corners still holds every contributor (the
    emulation with margin 0 stays inside, asserted); the seeded defect is the box of the pixel's own square without margin, which loses bilinear taps"""
    hits = 0
    for tag, kind, co, H, W, bilinear in ([(f"rotate {a}", 0, R.rotate_coeffs(a, H, W), H, W, 0) for a in R.ROT_ANGLES for H, W in R.ROT_SHAPES[1:]]
                                          + [(f"perspective {s}", 1, R.perspective_coeffs(*R.perspective_points(W, H, s)), H, W, 1) for H, W, s in R.PERSP_CASES[2:]]
                                          + [("zoom", 1, B.ZOOM_PERSP[0], B.ZOOM_PERSP[1], B.ZOOM_PERSP[2], 1)]):
        lines = []
        for name, dy in B.hard_dy((6, H, W)).items():
            if bilinear:
                r64, r32 = B.adjoint_pair(lambda t, dt: R.warp_bilinear(t, kind, co, H, W, dt), torch.zeros(6, H, W), dy)
            else:
                index = _nearest_index(kind, co, H, W, H, W)
                r64, r32 = B.scatter_adjoint(dy, index, H, W, F64), B.scatter_adjoint(dy, index, H, W, F32)
            assert not E.outside(E.frame_err(B.warp_adjoint32(dy, kind, co, H, W, bilinear, margin=0.0)[0], r64), E.frame_err(r32, r64))
            lines.append((name, E.frame_err(r32, r64), E.frame_err(B.warp_adjoint32(dy, kind, co, H, W, bilinear)[0], r64),
                          E.frame_err(B.warp_adjoint32(dy, kind, co, H, W, bilinear, margin=0.0, half=0.5)[0], r64)))
        hit = _teeth(f"warp {tag} {H}x{W} box of the pixel's own square", lines)
        hits += bool(hit)
    assert hit and hits == 1, hits          # the zoom: only where an input pixel's footprint spans several output pixels can the box be too small
    co, H, W = B.WHOLE_PERSP
    dx, n_whole = B.warp_adjoint32(B.hard_dy((6, H, W))["ones"], 1, co, H, W, 1)
    assert n_whole > 0 and n_whole < H * W, n_whole


# ------------------------------------------------------------------------------------------------------------------------ embed tail
def test_key_matrix_is_key_expand_and_its_defects_fall_outside():
    hit = {"j_over_step": [], "no_clamp": []}
    for case in B.TAIL_BWD_CASES:
        tag, Fn, H, W, S, Cd, low, full, _ = case
        imgs, delta, hm_low, hm_full, cfg, preds = B.tail_bwd_inputs(case, "noise")
        Wk = B.key_matrix(Fn, cfg["step"], cfg["mode"], cfg["total_key"], F64)
        assert torch.equal(torch.einsum("fk,kcyx->fcyx", Wk, delta.double()), R.key_expand(delta, Fn, cfg["step"], cfg["mode"], cfg["total_key"], F64)), tag
        for defect in hit:
            lines = []
            for kind, g in B.hard_dy((Fn, Cd, S, S)).items():
                fn = lambda t, dt: B.tail_linear(t, Fn, S, S, cfg, hm_low, dt)          # noqa: E731
                r64, r32 = B.adjoint_pair(fn, delta, g)
                lines.append((kind, E.frame_err(r32, r64), E.frame_err(B.key_reduce32(g, hm_low, Fn, cfg), r64),
                              E.frame_err(B.key_reduce32(g, hm_low, Fn, cfg, defect), r64)))
            if _teeth(f"key_reduce {tag} {defect}", lines):
                hit[defect].append(tag)
    assert any("interpolate" in t for t in hit["j_over_step"]), hit
    assert any("total_key" in t for t in hit["no_clamp"]), hit


def _tail_point(case, kind):
    tag, Fn, H, W, S, Cd, low, full, _ = case
    imgs, delta, hm_low, hm_full, cfg, preds = B.tail_bwd_inputs(case, kind)
    d_out = B.tail_dy(case, kind)[0]
    own = B.adjoint(lambda t, dt: B.tail_out(t, imgs, hm_full, cfg, dt), preds, d_out, F64)
    amb = B.tail_flags(preds, imgs, hm_full, cfg)
    return imgs, hm_full, cfg, preds, d_out, own, amb


@pytest.mark.parametrize("case", B.TAIL_BWD_CASES, ids=[c[0] for c in B.TAIL_BWD_CASES])
def test_tail_closed_form_is_autograd_flag_shares_and_strict_gates(case):
    for kind in B.TAIL_KINDS:
        imgs, hm, cfg, preds, d_out, own, amb = _tail_point(case, kind)
        Cd = preds.shape[1]
        assert (B.tail_point_adjoint(preds, imgs, hm, d_out, None, cfg, F64) - own).abs().max() <= 1e-15 * float(own.abs().max()), (case[0], kind)
        share = float(amb.float().mean())
        print(f"TEETH tail {case[0]} {kind}: flagged share {share:.5f}")
        assert share <= B.FLAG_SHARE, (case[0], kind, share)
        if kind == "sat":
            v = B.tail_pre(preds, imgs, hm, cfg, F64)
            assert ((v == 0) | (v == 1)).float().mean() > 0.01 and not amb[(v == 0) | (v == 1)].any()          # exact cases: no band
            other = B.tail_point_adjoint(preds, imgs, hm, d_out, None, cfg, F64, flip=amb.expand_as(v))
            ambg = amb if Cd == 3 else amb.any(1, keepdim=True)
            yard = B.masked_err(B.tail_point_adjoint(preds, imgs, hm, d_out, None, cfg, F32), own, other, ambg)
            bad = B.masked_err(B.tail_point_adjoint(preds, imgs, hm, d_out, None, cfg, F32, strict=True), own, other, ambg)
            print(f"TEETH tail {case[0]} sat strict gates: yardstick {yard:.3e} defect {bad:.3e}")
            assert not E.outside(yard, yard) and E.outside(bad, yard)


# ------------------------------------------------------------------------------------------------------------------------ colour ops
@pytest.fixture(scope="module")
def pixels():
    x = R.hard_pixels()
    return x, B.hard_dy(tuple(x.shape))["noise"], B.pixel_bands(x.shape[-2])


def test_closed_forms_and_the_hue_restatement_are_autograd_of_the_formulas(pixels):
    x, dy, bands = pixels
    for name, op, f in [c for c in R.COLOR_CASES if c[1] != R.OP_HUE]:
        own = B.adjoint(lambda t, dt: R.color_op(t, op, f, dt), x, dy, F64)
        assert (B.color_adjoint(x, dy, op, f, F64) - own).abs().max() <= 1e-14 * float(own.abs().max()), (name, f)
    for f in (0.07, -0.31):
        assert torch.equal(B.hue_fwd(x, f, F64), R.color_op(x, R.OP_HUE, f, F64))
        own = B.adjoint(lambda t, dt: R.color_op(t, R.OP_HUE, f, dt), x, dy, F64)
        assert torch.equal(B.adjoint(lambda t, dt: B.hue_fwd(t, f, dt), x, dy, F64), own), f          # autograd sends a tie to the first index


@pytest.mark.parametrize("name,op,f", B.COLOR_BWD_CASES, ids=[f"{n}{f:g}" for n, _, f in B.COLOR_BWD_CASES])
def test_flagged_shares_are_capped_and_contrast_flags_nothing(name, op, f):
    if op == R.OP_GRAYSCALE:
        return
    if op == R.OP_HUE:
        x, changed = B.hue_pixels(f)
        flag = B.hue_flags(x, f).expand(-1, 3, -1, -1)
        assert not changed or abs(6 * f - round(6 * f)) < 1e-6, changed          # only where 6 x factor is an integer: structured pixels sit on sector boundaries
    else:
        x = R.hard_pixels()
        flag = B.color_flags(x, op, f)
    for band, rows in B.pixel_bands(x.shape[-2]):
        share = float(flag[:, :, rows].float().mean())
        print(f"TEETH {name} {f:g} {band}: flagged share {share:.5f}")
        assert share <= (0.0 if op == R.OP_CONTRAST else B.FLAG_SHARE), (name, f, band, share)
    if op == R.OP_CONTRAST:
        assert not B.color_flags(B.contrast_frames(), op, f).any()


def _colour_teeth(tag, x, dy, bands, op, f, **defect):
    own, other, amb, keep, y32 = B.color_ref(x, dy, op, f)
    good = B.color_adjoint(x, dy, op, f, F32)
    bad = B.color_adjoint(x, dy, op, f, F32, **defect)
    lines = [(b, yd, gd, bd) for (b, yd), (_, gd), (_, bd) in zip(B.band_lines(y32, own, bands, other, amb, keep), B.band_lines(good, own, bands, other, amb, keep),
                                                              B.band_lines(bad, own, bands, other, amb, keep))]
    return _teeth(tag, lines)


def test_colour_defects_fall_outside_the_envelope(pixels):
    x, dy, bands = pixels
    hit = _colour_teeth("brightness 0.5 strict gates", x, dy, bands, R.OP_BRIGHTNESS, 0.5, strict=True)
    assert "corners" in hit, hit          # f x = 0 exactly on the black channels, 0.5 x 2 = 1 exactly nowhere: the bound at 0
    assert "corners" in _colour_teeth("saturation 0.5 strict gates", x, dy, bands, R.OP_SATURATION, 0.5, strict=True)
    for f in (0.5, 1.5):
        assert _colour_teeth(f"contrast {f} without the mean coupling", x, dy, bands, R.OP_CONTRAST, f, no_coupling=True)
    assert _colour_teeth("contrast 2 unmasked sum", x, dy, bands, R.OP_CONTRAST, 2.0, unmasked_sum=True)
    assert _colour_teeth("saturation 0.5 with 0.299", x, dy, bands, R.OP_SATURATION, 0.5, gray0=0.299)


def test_hue_tie_sent_to_the_last_index_falls_outside(pixels):
    _, dy, bands = pixels
    x, changed = B.hue_pixels(0.07)
    assert not changed
    own, _, _, keep, y32 = B.color_ref(x, dy, R.OP_HUE, 0.07)
    bad = B.adjoint(lambda t, dt: B.hue_fwd(t, 0.07, dt, tie_last=True), x, dy, F32)
    lines = [(b, yd, yd, bd) for (b, yd), (_, bd) in zip(B.band_lines(y32, own, bands, keep=keep), B.band_lines(bad, own, bands, keep=keep))]
    hit = _teeth("hue 0.07 tie to the last index", lines)
    assert {"tie01", "tie02", "tie12"} <= set(hit) and "random" not in hit, hit


# ------------------------------------------------------------------------------------------------------------------------ perceptual
def test_yuv_gradient_with_t_in_place_of_its_transpose_falls_outside():
    for Fn, H, W in B.PERCEP_SHAPES:
        lines = []
        for kind in ("noise", "tiny"):
            a, b = B.percep_inputs(Fn, H, W, kind)
            r64, r32 = B.adjoint_pair(lambda t, dt: B.percep(a, t, 1, dt), b, torch.ones(()))
            lines.append((kind, E.frame_err(r32, r64), E.frame_err(B.percep_grad32(a, b, 1), r64), E.frame_err(B.percep_grad32(a, b, 1, transposed=False), r64)))
        assert len(_teeth(f"percep yuv {Fn}x{H}x{W} T for T^T", lines)) == 2
