"""The fp64-envelope rule, stated once (a plain CPU module: torch and the standard library only, no pytest in it).

A kernel's error against the float64 reference may exceed the error of a float32 yardstick on the same inputs by a MARGIN:
    hip error <= MARGIN * max(yardstick error, floor),     MARGIN = twice the largest ratio measured on an MI355X, never above CAP = 8.
Every figure is printed before anything is asserted (profiles/*_fp64_envelope.txt are recordings of those lines).  Two forms:
    check_rows   errors per named group of a case, floor U32 = 2^-24 (the final rounding of an fp32 result): the bwd, fwd, img and loss families
    check_units  errors already in units of 2^-24 of the terms' magnitudes, floor 1: the split, fused and detector-backward (_det_bwd_ref) families
Each family binds a check to its tag and its margin in its own module (functools.partial) and keeps its margin, cases and metrics there (the
backward family, which has no module of its own besides its two test files, at the end of this one);
`outside` is the rule at the cap, for the CPU contract tests that show a seeded defect falls outside whatever the margin.  The yardsticks run
through `one_thread`.  The asserts carry explicit messages: pytest does not rewrite assertions outside test modules."""
import functools

import torch

U32 = 2.0 ** -24            # floor of the yardstick: the final rounding of an fp32 result is unavoidable even where ATen happens to be exact
CAP = 8.0                   # the standing rule itself: what the CPU contract tests use ("with any margin up to the cap")
TINY = 1e-30
ENV_SHAPES = [(37, 18, 20), (301, 130, 160), (67, 1100, 1100)]          # (rows, C, ld): C % 4 != 0 twice, ld > 4 ceil(C / 4) once


def one_thread(fn):
    """fn() with ATen on one thread: the summation order of its reductions (and the yardstick with it) must not depend on the host's core count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


def cpu_autograd(fn):
    """(float64 reference, ATen float32 yardstick) of `fn(dtype)` on the CPU.  One thread: the summation order of ATen's reductions -- and with it
    the yardstick, whose worst channel is a cancelling sum -- would otherwise change with the number of cores the host happens to grant"""
    return one_thread(lambda: (fn(torch.float64), fn(torch.float32)))


def hard_matrix(rows, C, seed, groups):
    """[rows][C] float32 (CPU), fixed seed.  groups = "rows": every row is a group of mean 30 and std 0.5, row 1 is constant (variance 0), row 2
    holds a single 4e3 outlier, row 3 has magnitude 1e-3; groups = "cols": the same for the columns (channels)"""
    g = torch.Generator().manual_seed(seed)
    x = 30.0 + 0.5 * torch.randn(rows, C, generator=g)
    if groups == "rows":
        x[1] = 30.25
        x[2, C // 2] = 4e3
        x[3] = 1e-3 * torch.randn(C, generator=g)
    else:
        x[:, 1] = 30.25
        x[rows // 2, 2] = 4e3
        x[:, 3] = 1e-3 * torch.randn(rows, generator=g)
    return x


def group_err(got, ref, dim, keep=None):
    """worst group of max |got - ref| / max |ref|, groups = slices along `dim` (dim = None: every element is its own group); `keep`: mask of the
    elements that take part.  A group whose reference is all zero must be reproduced exactly."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d, m = (got - ref).abs(), ref.abs()
    if keep is not None:
        d, m = d * keep, m * keep
    if dim is not None:
        d, m = d.amax(dim), m.amax(dim)
    e = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(e.max())


def frame_err(got, ref):
    """max |got - ref| / max(max |ref|, tiny) over the whole tensor"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), TINY))


def cand_err(got, own, other, amb):
    """frame_err where a pixel of the mask `amb` may match either `own` or `other` (the two sides of a discontinuity); every other pixel must match `own`"""
    got, own, other = got.detach().double().cpu(), own.double(), other.double()
    d = (got - own).abs()
    d = torch.where(amb.expand_as(d), torch.minimum(d, (got - other).abs()), d)
    return float(d.max() / max(float(own.abs().max()), TINY))


def check_rows(tag, width, label, margin, case, rows):
    """rows: (name, hip error, yardstick error).  Prints every figure, then asserts hip <= margin * max(yardstick, U32) for each."""
    bad = []
    for name, hip, yard in rows:
        ratio = hip / max(yard, U32)
        print(f"{tag} {case:<{width}s} {name:<10s} hip {hip:.3e}  {label} {yard:.3e}  ratio {ratio:6.3f}")
        if not ratio <= margin:
            bad.append((name, hip, yard, ratio))
    assert not bad, (case, bad)


def check_units(tag, width, margin, case, r, r_ref):
    """r, r_ref: the worst error of the kernel and of the yardstick in units (floats).  Prints the figures, then asserts r <= margin * max(r_ref, 1)."""
    ratio = r / max(r_ref, 1.0)
    print(f"{tag} {case:<{width}s} hip {r:9.3f}  aten-fp32 {r_ref:9.3f}  ratio {ratio:6.3f}")
    assert ratio <= margin, (case, r, r_ref, ratio)


def outside(err, yard, floor=U32):
    """True when an error falls outside the envelope at the cap: the yardstick's own ratio is 1, no margin up to 8 admits the defect"""
    return not err <= CAP * max(yard, floor)


# ---- the backward family (tests/test_gpu_bwd.py, tests/test_gpu_bwd_unet.py; profiles/bwd_fp64_envelope.txt lists every case)
FP64_MARGIN = 6.94          # 2 x 3.468, the largest ratio measured: d bias of vs_layernorm_bwd at rows = 301, C = 130 (64-row fp32 chunks vs ATen's order)
bwd_envelope = functools.partial(check_rows, "ENVELOPE", 44, "aten-fp32", FP64_MARGIN)
