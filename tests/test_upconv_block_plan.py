"""The sharing rules that csrc/upconv_gather.h builds on (no GPU): along one axis, with A / B the source tables of the two output positions
2 * cell and 2 * cell + 1 (computed as the kernels compute them: ReflectionPad2d(1) on the up-sampled grid, align_corners=False, the second
source clamped to the map), for EVERY map size and cell

    tap 0:  B == A
    tap 1:  B's first source is A's second or A's first
    tap 2:  B's second source is A's second;  A's first source is B's first or A's second

so seven (tap, source) items per axis serve both positions, and replaying the kernel's walk over those items gives every pixel exactly its
six (tap, source, weight) terms per axis in the per-pixel order."""
import numpy as np

f32 = np.float32


def axis_table(pos, n):
    """[(s0, s1), ...], [(w0, w1), ...] of output position `pos` on a low-resolution axis of n sources (net_ops.hip: upconv_gather_ln_kernel)"""
    n2, src, wgt = 2 * n, [], []
    for k in range(3):
        r = pos + k - 1
        r = -r if r < 0 else (2 * n2 - 2 - r if r >= n2 else r)
        sf = max(f32(f32(f32(r) + f32(0.5)) * f32(0.5)) - f32(0.5), f32(0))
        i0 = int(sf)
        w1 = f32(sf - f32(i0))
        src.append((i0, i0 + (1 if i0 < n - 1 else 0)))
        wgt.append((f32(1) - w1, w1))
    return src, wgt


def blocked_walk(n, cell):
    """the terms each of the two positions receives from upconv_gather_2x2's walk along one axis, in order: [(tap, source, weight), ...] x 2"""
    (A, wa), (B, wb) = axis_table(2 * cell, n), axis_table(2 * cell + 1, n)
    s, w = (A, B), (wa, wb)
    k1_b0_is_a1 = B[1][0] == A[1][1]
    k2_a0_is_b0 = A[2][0] == B[2][0]
    items = {0: [A[0][0], A[0][1]], 1: [A[1][0], A[1][1], B[1][1]], 2: [B[2][0], A[2][1]]}
    visits = {(0, 0): [(0, 0, True), (1, 0, True)], (0, 1): [(0, 1, True), (1, 1, True)],
              (1, 0): [(0, 0, True), (1, 0, not k1_b0_is_a1)], (1, 1): [(0, 1, True), (1, 0, k1_b0_is_a1)], (1, 2): [(1, 1, True)],
              (2, 0): [(1, 0, True), (0, 0, k2_a0_is_b0)], (2, 1): [(0, 0, not k2_a0_is_b0), (0, 1, True), (1, 1, True)]}
    got = ([], [])
    for k in range(3):
        for i, source in enumerate(items[k]):
            for p, a, on in visits[(k, i)]:
                if on:
                    got[p].append((k, source, w[p][k][a]))
    return got


def test_seven_items_per_axis_serve_both_positions_everywhere():
    for n in range(1, 70):
        for cell in range(n):
            (A, _), (B, _) = axis_table(2 * cell, n), axis_table(2 * cell + 1, n)
            assert A[0] == B[0]
            assert B[1][0] in (A[1][1], A[1][0])
            assert B[2][1] == A[2][1]
            assert A[2][0] in (B[2][0], A[2][1])
            near = {max(cell - 1, 0), cell, min(cell + 1, n - 1)}
            assert {v for t in (A, B) for pair in t for v in pair} <= near


def test_the_walk_gives_every_position_its_terms_in_the_per_pixel_order():
    for n in range(1, 70):
        for cell in range(n):
            got = blocked_walk(n, cell)
            for p in range(2):
                src, wgt = axis_table(2 * cell + p, n)
                want = [(k, src[k][a], wgt[k][a]) for k in range(3) for a in range(2)]
                assert got[p] == want, (n, cell, p)


def test_duplicated_and_zero_weight_terms_are_kept():
    """the last cell hits one source twice at tap 2 (weights 0.75 / 0.25); cell 0 carries a term of weight 0 at tap 1"""
    got = blocked_walk(5, 4)
    assert [t for t in got[0] if t[0] == 2] == [(2, 4, f32(0.75)), (2, 4, f32(0.25))]
    got = blocked_walk(5, 0)
    assert [t for t in got[0] if t[0] == 1] == [(1, 0, f32(1.0)), (1, 1, f32(0.0))]
