"""The metric of tests/test_gpu_fused_envelope.py on the CPU: on the operands of every GPU case the float32 yardstick (tests/_fused_ref.py) gives a
finite r_ref, and each seeded defect of the emulation falls outside  CAP max(r_ref, 1)  -- with any margin up to the cap of 8 -- in at least one
of the checks the GPU file makes on those operands.  Nothing here needs a GPU.

Seeded defects, vs_cnx_block: the scale row of the neighbouring frame for the last 32 pixels of a 128-pixel group; two hidden channels exchanged
inside one k(s, half, v) group of the packed W2; the low plane of the second split dropped; the same plane with f16 denormals read as zero;
l_a h_w dropped on the last k-step of pwconv1.  vs_resblock_thin: t outside the image taken as conv0 of zero-padded data; the halo ring of every
tile's t read one pixel to the right.  For each the test prints whether the older criterion (max |got - ref| < 2e-5 max |ref| on randn
operands) would have accepted it; only the envelope's rejection is asserted."""
import pytest
import torch

from tests import _fused_ref as Q
from tests import _split_ref as R
from tests._envelope import outside


def rmax(got, S, unit, skip=None):
    r = Q.ratio_units(got, S, unit)
    return float((r if skip is None else r.masked_fill(skip, 0.0)).max())


def old_accepts(S_def, S):
    return bool((S_def - S).abs().max() < R.OLD_TOL * S.abs().max())


@pytest.mark.parametrize("kw", [dict(pad=1), dict()], ids=["conv3x3", "gemm"])
def test_stage_is_the_ideal_of_the_split_envelope(kw):
    """_fused_ref.stage (F.conv2d, no patch matrix) forms the S, P and ref32 of _split_ref.ideal"""
    a = R.hard_act(2, 16, 9, 14, 21) if kw else R.gemm_as_conv(R.hard_rows(131, 144, 13))
    w = R.hard_weights(12, a.shape[1], 3 if kw else 1, 22)
    for arith in (2, 3):
        i, s = R.ideal(a, w, arith, Q.A_MUL, **kw), Q.stage(a, w, arith, Q.A_MUL, **kw)
        assert ((i.S - s.S).abs() <= 1e-12 * i.P).all() and ((i.P - s.P).abs() <= 1e-12 * i.P).all()
        assert torch.equal(i.ref32, s.ref32)


# ---------------------------------------------------------------------------------------------------------------- vs_cnx_block
def cnx_checks(o, f, *, ref=False, rows64=None, wmap=None, low=None):
    """{check: (S, unit, ref)} of the statistics launch, the hidden tensor through the first one-hot W2 and the apply launch.
    low: 'drop' / 'flush' = the defective low plane of the second split"""
    out = {"stats": (f.part, f.part_unit, f.part32)}
    for name, w2, kw in (("hidden", Q.one_hot_w2(o.C, 0), {}), ("apply", o.w2, dict(bias2=o.bias2, res=o.res))):
        e = Q.cnx_second(o, f, wmap(w2) if wmap else w2, rows64=rows64, want_ref=ref, **kw)
        S = e.S
        if low:
            S = S - e.low + (e.low_flush if low == "flush" else 0.0)
        out[name] = (S, e.unit, e.ref if ref else None)
    return out


def cnx_defects(o):
    yield "neighbouring frame's scale row", lambda: cnx_checks(o, Q.cnx_first(o), rows64=Q.neighbour_frame_rows(o.scale, o.HW, o.rows))
    yield "two hidden channels exchanged in W2", lambda: cnx_checks(o, Q.cnx_first(o), wmap=Q.swap_in_k_group)
    yield "low plane of the second split dropped", lambda: cnx_checks(o, Q.cnx_first(o), low="drop")
    yield "its f16 denormals read as zero", lambda: cnx_checks(o, Q.cnx_first(o), low="flush")
    yield "l_a h_w dropped on pwconv1's last k-step", lambda: cnx_checks(o, Q.cnx_first(o, drop_tail=True))


@pytest.fixture(scope="module")
def cnx_old_criterion():
    """{defect: the older criterion accepts it} on randn operands, apply launch"""
    o = Q.cnx_randn_operands()
    good = cnx_checks(o, Q.cnx_first(o))["apply"][0]
    return {name: old_accepts(make()["apply"][0], good) for name, make in cnx_defects(o)}


@pytest.mark.parametrize("shape", Q.CNX_SHAPES, ids=str)
def test_cnx_yardstick_is_finite_and_the_seeded_defects_fall_outside(shape, cnx_old_criterion):
    o = Q.cnx_operands(*shape)
    f = Q.cnx_first(o)
    good = cnx_checks(o, f, ref=True)
    r_ref = {k: rmax(ref, S, unit) for k, (S, unit, ref) in good.items()}
    for sel in range(1, Q.NSEL):          # the other selections of the hidden tensor
        e = Q.cnx_second(o, f, Q.one_hot_w2(o.C, sel))
        r_ref[f"hidden {sel}"] = rmax(e.ref, e.S, e.unit)
    print(f"FUSED-TEETH cnx_block {shape}: yardstick " + ", ".join(f"{k} {v:.2f}" for k, v in r_ref.items()))
    assert all(v == v and v < float("inf") for v in r_ref.values())
    for name, make in cnx_defects(o):
        if o.B == 1 and name.startswith("neighbouring"):
            continue                                   # a single frame has no neighbour
        bad = make()
        r = {k: rmax(bad[k][0], S, unit) for k, (S, unit, _) in good.items()}
        print(f"FUSED-TEETH cnx_block {shape}: {name}: " + ", ".join(f"{k} {v:.1f}" for k, v in r.items())
              + f"; older criterion on randn operands {'ACCEPTS' if cnx_old_criterion[name] else 'rejects'} it")
        assert any(outside(r[k], r_ref[k], 1.0) for k in r), (name, r, r_ref)


@pytest.mark.parametrize("shape", Q.CNX_SHAPES, ids=str)
def test_cnx_whole_block_and_overflow_yardsticks_are_finite(shape):
    o = Q.cnx_block_operands(*shape)
    f = Q.cnx_first(o)
    s64, u_s = Q.grn_scale64(f.part, o.gamma.double(), o.B, f.part_unit)
    s32 = R.one_thread(lambda: Q.grn_scale64(f.part32, o.gamma, o.B))
    fr = torch.arange(o.rows) // o.HW
    e = Q.cnx_second(o, f, o.w2, rows64=s64[fr], rows32=s32[fr], u_scale=u_s[fr], bias2=o.bias2, res=o.res)
    r = [rmax(s32, s64, u_s), rmax(e.ref, e.S, e.unit)]
    o = Q.cnx_operands(*shape)
    f = Q.cnx_first(o)
    fr0, k, p, s = Q.overflow_plant(o, f)
    scale = o.scale.clone()
    scale[fr0, k] = s
    e = Q.cnx_second(o, f, o.w2, rows64=Q.scale_rows_of(scale, o.HW, o.rows), bias2=o.bias2, res=o.res, zero=(p, k))
    skip = torch.zeros_like(e.S, dtype=torch.bool)
    skip[p] = True
    r.append(rmax(e.ref, e.S, e.unit, skip))
    print(f"FUSED-TEETH cnx_block {shape}: yardstick GRN scale {r[0]:.2f}, block out {r[1]:.2f}, with a planted overflow {r[2]:.2f}")
    assert all(v == v and v < float("inf") for v in r)


# ---------------------------------------------------------------------------------------------------------------- vs_resblock_thin
RB_PARAMS = ([(f, m) for f in Q.RB_FORMS for m in Q.RB_SMALL] + [(f, m) for f in ((16, 2, 16), (16, 3, 4), (32, 2, 32)) for m in Q.RB_LARGE])


@pytest.fixture(scope="module")
def rb_old_criterion():
    o = Q.rb_randn_operands()
    good = Q.rb_chain(o, 2, want_ref=False).S
    return {k: old_accepts(Q.rb_chain(o, 2, want_ref=False, **{k: True}).S, good) for k in ("padded_conv0", "halo_shift")}


@pytest.mark.parametrize("p", RB_PARAMS, ids=str)
def test_resblock_yardstick_is_finite_and_the_seeded_defects_fall_outside(p, rb_old_criterion):
    (c, arith, cin), m = p
    o = Q.rb_operands(c, cin, *m)
    e = Q.rb_chain(o, arith)
    r_ref = rmax(e.ref, e.S, e.unit)
    shift = rmax(Q.rb_chain(o, arith, halo_shift=True).S, e.S, e.unit)
    small = m in Q.RB_SMALL
    msg = f"FUSED-TEETH resblock_thin {p}: yardstick block {r_ref:.2f}"
    assert r_ref == r_ref and r_ref < float("inf")
    if small:                              # the on-chip-t cases run on the small maps
        pos = Q.with_positive_ring(o)
        for tap in (4, 0, 8):
            q = Q.with_t_observable(pos, tap)
            et = Q.rb_chain(q, arith)
            rt = rmax(et.ref, et.S, et.unit)
            assert rt == rt and rt < float("inf")
            msg += f", t through tap {tap} {rt:.2f}"
            if tap == 0:
                padded = rmax(Q.rb_chain(q, arith, padded_conv0=True, want_ref=False).S, et.S, et.unit)
                assert outside(padded, rt, 1.0), (padded, rt)
    else:
        padded = rmax(Q.rb_chain(o, arith, padded_conv0=True, want_ref=False).S, e.S, e.unit)
        assert outside(padded, r_ref, 1.0), (padded, r_ref)
    print(msg)
    print(f"FUSED-TEETH resblock_thin {p}: t outside the image = conv0 of padded data {padded:.3g} (older criterion on randn operands "
          f"{'ACCEPTS' if rb_old_criterion['padded_conv0'] else 'rejects'} it), halo ring shifted by one pixel {shift:.3g} "
          f"({'ACCEPTS' if rb_old_criterion['halo_shift'] else 'rejects'})")
    assert outside(shift, r_ref, 1.0), (shift, r_ref)


@pytest.mark.parametrize("p", [(f, m) for f in ((16, 2, 1), (16, 2, 16), (32, 2, 20)) for m in ((2, 7, 15), (2, 17, 33))], ids=str)
def test_resblock_overflow_yardstick_is_finite(p):
    (c, arith, cin), m = p
    q, (b, n, y, x) = Q.rb_overflow_operands(Q.rb_operands(c, cin, *m))
    e = Q.rb_chain(q, arith, zero=(b, n, y, x))
    assert float(F_t(q)[b, n, y, x]) * Q.A_MUL >= Q.F16_OVERFLOW
    skip = torch.zeros_like(e.S, dtype=torch.bool)
    skip[b, :, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    r = rmax(e.ref, e.S, e.unit, skip)
    print(f"FUSED-TEETH resblock_thin {p}: yardstick with t[{n}] at ({y}, {x}) beyond the f16 range {r:.2f}")
    assert r == r and r < float("inf")


def F_t(q):
    """t of the fp32 operands in float64"""
    return torch.relu(torch.nn.functional.conv2d(q.x.double(), q.w0.double(), padding=1) + q.b0.double().view(1, -1, 1, 1))
