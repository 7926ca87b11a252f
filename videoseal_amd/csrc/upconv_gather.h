// The 36-term gather of the Upsample groups (net_ops.hip: upconv_gather_ln_kernel, upconv_fused.hip: phase 3) for a 2 x 2 BLOCK of
// output pixels: the four pixels (2y + p, 2x + q), p, q in {0, 1}, of one low-resolution cell (y, x).
//
// Per output pixel the gather is   acc += (wy[ky][a] * wx[kx][c]) * z[ys[ky][a]][xs[kx][c]][tap ky, kx]   over (ky, a, kx, c) ascending --
// 36 16-byte loads per lane and f32x4.  Along one axis the two pixels of a cell draw from overlapping sources: with A the table of phase 0
// and B the table of phase 1 (source pairs per tap, as the per-pixel kernels compute them),
//     tap 0:  B == A                                          -> items {A0, A1}
//     tap 1:  B0 is A1 (interior, last cell) or A0 (cell 0)    -> items {A0, A1, B1}
//     tap 2:  B1 == A1;  A0 is B0 (interior, cell 0) or A1 (last cell: the pair that hits the same source twice) -> items {B0, A1}
// for every map size and every cell, borders and the 1-wide map included (tests/test_upconv_block_plan.py enumerates them).  That is 7
// (tap, source) items per axis instead of 2 x 6, so a block loads 7 x 7 = 49 vectors where four pixels loaded 144.
//
// Exactness: every pixel receives exactly its 36 terms, each as `acc + w * z` with the weight product and the (ky, a, kx, c) order of the
// per-pixel form (terms of weight 0 and the duplicated source of the last row / column included), so the results are the same bit for bit.
// Only the loads are shared.  The walk is one SWEEP over (kx, c) per (row item, pixel row p, a): the sweeps of one pixel run in (ky, a)
// order.  The two terms per axis whose item depends on the position are resolved without a branch -- along x by selecting the loaded
// vector, along y by running the sweep on both candidate items and keeping the accumulator of the one that applies -- so interior and
// border cells execute the same instruction stream and a wave that holds an edge cell pays nothing extra.
#pragma once
#include <utility>

#include "vs_common.h"

// source indices and weights of the two output positions 2 * cell + p of one axis (n = size of the low-resolution map along it): the
// tables of the per-pixel form, computed the same way
struct UpAxis {
  int s[2][3][2];
  float w[2][3][2];
  bool k1_b0_is_a1;      // tap 1: phase 1's first source is phase 0's second one (else its first)
  bool k2_a0_is_b0;      // tap 2: phase 0's first source is phase 1's first one (else phase 0's second)
};

__device__ __forceinline__ void upconv_axis(const int cell, const int n, UpAxis& ax) {
  const int n2 = 2 * n;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int r = 2 * cell + p + k - 1;
      r = r < 0 ? -r : (r >= n2 ? 2 * n2 - 2 - r : r);                 // ReflectionPad2d(1) on the up-sampled grid
      const float sf = fmaxf((r + 0.5f) * 0.5f - 0.5f, 0.f);           // align_corners=False
      const int i0 = (int)sf;
      ax.s[p][k][0] = i0; ax.s[p][k][1] = i0 + (i0 < n - 1);
      ax.w[p][k][1] = sf - i0; ax.w[p][k][0] = 1.f - ax.w[p][k][1];
    }
  ax.k1_b0_is_a1 = ax.s[1][1][0] == ax.s[0][1][1];
  ax.k2_a0_is_b0 = ax.s[0][2][0] == ax.s[1][2][0];
}

// items of tap k along one axis, in ascending source order
__device__ __forceinline__ int upconv_item(const UpAxis& ax, const int k, const int i) {
  return k == 0 ? ax.s[0][0][i] : k == 1 ? (i < 2 ? ax.s[0][1][i] : ax.s[1][1][1]) : (i == 0 ? ax.s[1][2][0] : ax.s[0][2][1]);
}

// acc[p][q][j] of the 2 x 2 block += the 36 terms of pixel (p, q), channels 4 j .. 4 j + 3 of this lane.
// zb: this lane's channels of source (0, 0), tap (0, 0); rs / cs: offset of one source row / column in floats; Co: tap (ky, kx) lies at
// (ky * 3 + kx) * Co.  ay.s / ax.s must be relative to the source that zb points to.
template <class F, int... I>
__device__ __forceinline__ void upconv_static_for(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }

template <int NV, class Off>
__device__ __forceinline__ void upconv_gather_2x2(const float* __restrict__ zb, const Off rs, const Off cs, const int Co, const UpAxis& ay,
                                                  const UpAxis& ax, f32x4 (&acc)[2][2][NV]) {
  // Step t = (row item 0..6, j): the 7 vectors of one source row and one f32x4 of this lane's channels, each loaded once.  The steps are kept
  // apart on purpose: left to itself hipcc issues the 49 NV loads early and sinks the terms to the end of the block (228 registers at NV = 1,
  // 468 at NV = 2, spills at NV = 4), so a scheduling barrier closes every step and an empty asm pins its accumulators before it.  Unrolled
  // through an index sequence (a `#pragma unroll` of 28 such steps is past the unroller's size limit and leaves the accumulators in scratch).
  // The loads of step t + 1 are in flight during the terms of step t where the registers allow it: NV = 1 / 2 compile to 158 / 210 registers
  // with that, NV = 4 to 250 without it (281 with: one wave per SIMD instead of two).
  constexpr int NSTEP = 7 * NV;
  constexpr bool AHEAD = NV <= 2;
  f32x4 zbuf[AHEAD ? 2 : 1][3][3];
  auto load = [&](const int t, f32x4 (&zc)[3][3]) __attribute__((always_inline)) {
    const int r7 = t / NV, j = t % NV;
    const int ky = r7 < 2 ? 0 : (r7 < 5 ? 1 : 2), ri = r7 - (ky == 0 ? 0 : (ky == 1 ? 2 : 5));
    const float* zr = zb + (Off)upconv_item(ay, ky, ri) * rs + ky * 3 * Co + 4 * j;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int ci = 0; ci < (kx == 1 ? 3 : 2); ++ci) zc[kx][ci] = *reinterpret_cast<const f32x4*>(zr + (Off)upconv_item(ax, kx, ci) * cs + kx * Co);
  };
  if (AHEAD) load(0, zbuf[0]);
  upconv_static_for([&](auto tc) __attribute__((always_inline)) {
    constexpr int t = decltype(tc)::value;
    constexpr int cur = AHEAD ? (t & 1) : 0;
    if (!AHEAD) load(t, zbuf[0]);
    else if (t + 1 < NSTEP) load(t + 1, zbuf[AHEAD ? ((t + 1) & 1) : 0]);
    __builtin_amdgcn_sched_barrier(0);
    constexpr int r7 = t / NV, j = t % NV;
    constexpr int ky = r7 < 2 ? 0 : (r7 < 5 ? 1 : 2), ri = r7 - (ky == 0 ? 0 : (ky == 1 ? 2 : 5));
    const f32x4 (&zc)[3][3] = zbuf[cur];
    const f32x4 z_k1b0 = ax.k1_b0_is_a1 ? zc[1][1] : zc[1][0];
    const f32x4 z_k2a0 = ax.k2_a0_is_b0 ? zc[2][0] : zc[2][1];
    // one pixel row's terms (ky, a, kx = 0..2, c = 0..1) for both pixels of that row; `on`: the sweep applies to this lane
    auto sweep = [&](const int p, const int a, const bool on) __attribute__((always_inline)) {
      const float wyv = ay.w[p][ky][a];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const f32x4 z0 = c == 1 ? zc[kx][1] : (kx == 2 ? z_k2a0 : zc[kx][0]);
          const f32x4 z1 = kx == 1 ? (c == 1 ? zc[1][2] : z_k1b0) : zc[kx][c];
          const f32x4 t0 = acc[p][0][j] + (wyv * ax.w[0][kx][c]) * z0;
          const f32x4 t1 = acc[p][1][j] + (wyv * ax.w[1][kx][c]) * z1;
          acc[p][0][j] = on ? t0 : acc[p][0][j];
          acc[p][1][j] = on ? t1 : acc[p][1][j];
        }
    };
    if (ky == 0) {                     // items {A0, A1}, both phases alike
      sweep(0, ri, true);
      sweep(1, ri, true);
    } else if (ky == 1) {              // items {A0, A1, B1}
      if (ri == 0) { sweep(0, 0, true); sweep(1, 0, !ay.k1_b0_is_a1); }
      if (ri == 1) { sweep(0, 1, true); sweep(1, 0, ay.k1_b0_is_a1); }
      if (ri == 2) sweep(1, 1, true);
    } else {                           // items {B0, A1}
      if (ri == 0) { sweep(1, 0, true); sweep(0, 0, ay.k2_a0_is_b0); }
      if (ri == 1) { sweep(0, 0, !ay.k2_a0_is_b0); sweep(0, 1, true); sweep(1, 1, true); }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) asm volatile("" : "+v"(acc[p][0][j]), "+v"(acc[p][1][j]));
    __builtin_amdgcn_sched_barrier(0);
  }, std::make_integer_sequence<int, NSTEP>{});
}
