// SSIM / MS-SSIM statistics and their adjoint, the 2 x 2 pyramid pooling, and the JND term of the perceptual loss (losses/ssim.py, losses/jndloss.py).
//
// Shape of the two streaming kernels: a workgroup of 128 threads owns a strip of columns of one plane and walks down a chunk of rows.  Every thread owns ONE
// column and keeps the last 11 horizontally filtered rows of the five moments (x, y, x^2, y^2, xy) in REGISTERS (a ring, statically indexed: the row loop is
// unrolled by 11), so the vertical filter needs no memory at all; only the horizontal filter goes through LDS (one raw row of x and y, 138 floats each).  The
// adjoint adds a second register ring, 10 rows behind the first: the three coefficient rows A, B, Cc of the map, filtered horizontally through LDS.
// Nothing but x, y (and the gradient) touches HBM; there are no atomics anywhere: the statistics are per-block partial sums in double, summed in a fixed
// order by a second tiny launch, and the adjoint is a gather.
//
// Conditioning: the variances are shift invariant, so the moments are taken of x - c, c = the smallest pixel of x and y among the rows and columns the
// WORKGROUP reads (block_shift: one more pass over its input, a min through LDS; a function of the data and the grid alone, so two launches still agree bit
// for bit).  0 <= x - c <= x: the cancellation error of E[x^2] - mu^2 against C2 = 9e-4 is never above that of the reference's own unshifted fp32 formula, on
// black frames and letterbox bars (c = 0: the reference's arithmetic itself) as on any other, and far below it on bright flat regions (c ~ the level).  A
// constant shift of data_range / 2 (what this file did before) quarters the error at mid-grey but turns a black window into 0.25 - 0.25: 100 x the
// reference's error there (tests/test_gpu_loss_envelope.py, kinds `dark` and `dark-bars`).  The luminance factor adds the shift back, and the terms the
// shift leaves behind because the fp32 window does not sum to exactly 1 are restored (ssim_point): the same function in exact arithmetic.
#include "vs_common.h"

namespace {

constexpr int TAPS = 11;
constexpr int HALO = TAPS - 1;
constexpr int NT = 128;                  // threads per workgroup = columns a workgroup holds
constexpr int RAWW = NT + HALO;          // input columns a workgroup reads per row
constexpr int GRAD_TW = NT - HALO;       // gradient columns a workgroup of the adjoint produces

struct SsimWin { float w[TAPS]; };

inline unsigned gridx(int64_t n, int per = 256, int64_t cap = 4096) {
  int64_t g = (n + per - 1) / per;
  return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}

// horizontal 11-tap filter of the five moments at column t of the raw row in LDS.  The fused multiply-adds are written out, here and in the vertical
// filter (vfilter5): left to the compiler's contraction the fifth moment, which has no partner for a packed instruction, was rounded differently from
// the other four, and for x == y the three second moments must be the same number (cs = 1 to an ulp, as in the reference's fp32 formula).
__device__ __forceinline__ void hfilter5(const float* __restrict__ rx, const float* __restrict__ ry, int t, const SsimWin& g, float (&h)[5]) {
  h[0] = h[1] = h[2] = h[3] = h[4] = 0.f;
#pragma unroll
  for (int j = 0; j < TAPS; ++j) {
    const float xv = rx[t + j], yv = ry[t + j];
    const float px = g.w[j] * xv, py = g.w[j] * yv;
    h[0] += px;
    h[1] += py;
    h[2] = __builtin_fmaf(px, xv, h[2]);
    h[3] = __builtin_fmaf(py, yv, h[3]);
    h[4] = __builtin_fmaf(px, yv, h[4]);
  }
}
// vertical 11-tap filter: the ring's rows s + 1 .. s + 11 (mod 11), oldest first
__device__ __forceinline__ void vfilter5(const float (&ring)[5][TAPS], int s, const SsimWin& g, float (&m)[5]) {
  m[0] = m[1] = m[2] = m[3] = m[4] = 0.f;
#pragma unroll
  for (int k = 0; k < TAPS; ++k) {
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = __builtin_fmaf(g.w[k], ring[q][(s + 1 + k) % TAPS], m[q]);
  }
}

// SSIM and contrast-structure value of one map position from the five filtered moments of the SHIFTED frames (losses/ssim.py:94-103)
struct SsimPoint { float ssim, cs, l, inv_dc, inv_dl, M1, M2; };
// The fp32 window does not sum to 1 exactly (S = (sum w)^2 of the separable filter = 1 - O(1e-8)) and the reference's sigmas are sum(w x^2) - (sum(w x))^2 with THAT window, so in
// terms of the shifted moments (c = shift):  mu = m' + c S,  sigma = (e' - m'^2) + 2 c (1 - S) m' + c^2 S (1 - S)  (k1 = c (1 - S), k2 = c^2 S (1 - S), in
// double from the workgroup's c and the host's S: make_shift).  The correction is ~1e-8, but it is divided by sigma_x^2 + sigma_y^2 + C2 >= 9e-4: without it the mean SSIM is off by ~1e-6.
struct SsimShift { float c, cS, k1, k2; };
__device__ __forceinline__ SsimShift make_shift(float c, double S) {
  const double cd = (double)c;
  return SsimShift{c, (float)(cd * S), (float)(cd * (1.0 - S)), (float)(cd * cd * S * (1.0 - S))};
}
// the workgroup's shift: the smallest value of x and y in rows [row0, row1) at the columns ca (where va) and cb (where vb) of its NT threads -- the very
// pixels its row loop reads.  lds: NT floats, free again on return.  A plane of NaNs or infinities gets no shift.
__device__ __forceinline__ float block_shift(const float* __restrict__ xp, const float* __restrict__ yp, int W, int row0, int row1, int ca, bool va, int cb,
                                             bool vb, float* lds) {
  const int t = threadIdx.x;
  float mn = __builtin_inff();
  for (int r = row0; r < row1; ++r) {
    const int64_t o = (int64_t)r * W;
    if (va) mn = fminf(mn, fminf(xp[o + ca], yp[o + ca]));
    if (vb) mn = fminf(mn, fminf(xp[o + cb], yp[o + cb]));
  }
  lds[t] = mn;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (t < o) lds[t] = fminf(lds[t], lds[t + o]);
    __syncthreads();
  }
  const float c = lds[0];
  __syncthreads();
  return fabsf(c) < __builtin_inff() ? c : 0.f;
}
__device__ __forceinline__ SsimPoint ssim_point(const float (&m)[5], const SsimShift sh, float C1, float C2) {
  SsimPoint p;
  // the three (co)variances by the same fused operations, the three products of the means rounded alike: for x == y numerator and denominator of
  // both factors are the same number
  const float s1 = __builtin_fmaf(-m[0], m[0], m[2]) + __builtin_fmaf(2.f * sh.k1, m[0], sh.k2);
  const float s2 = __builtin_fmaf(-m[1], m[1], m[3]) + __builtin_fmaf(2.f * sh.k1, m[1], sh.k2);
  const float s12 = __builtin_fmaf(-m[0], m[1], m[4]) + __builtin_fmaf(sh.k1, m[0] + m[1], sh.k2);
  p.M1 = m[0] + sh.cS;
  p.M2 = m[1] + sh.cS;
  const float q11 = __fmul_rn(p.M1, p.M1), q22 = __fmul_rn(p.M2, p.M2), q12 = __fmul_rn(p.M1, p.M2);
  p.inv_dc = 1.0f / (s1 + s2 + C2);
  p.inv_dl = 1.0f / (__fadd_rn(q11, q22) + C1);
  p.cs = (__fadd_rn(s12, s12) + C2) * p.inv_dc;
  p.l = (__fadd_rn(q12, q12) + C1) * p.inv_dl;
  p.ssim = p.l * p.cs;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------------------- statistics
// grid: (strips of NT map columns, chunks of `rows` map rows, planes).  partial[((plane * chunks + chunk) * strips + strip) * 2 + {ssim, cs}]
__global__ __launch_bounds__(NT) void ssim_stats_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int rows, SsimWin g,
                                                        double S, float C1, float C2, double* __restrict__ partial) {
  __shared__ float raw[2][2][RAWW];
  __shared__ double red[2][NT];
  const int t = threadIdx.x;
  const int Hm = H - HALO, Wm = W - HALO;
  const int m0 = blockIdx.x * NT;                                  // first map column of the strip
  const int o0 = blockIdx.y * rows;                                // first map row of the chunk
  const int o1 = min(o0 + rows, Hm);
  const int nin = (o1 - o0) + HALO;                                // input rows o0 .. o1 + 9
  const int64_t base = (int64_t)blockIdx.z * H * W;
  const float* __restrict__ xp = x + base;
  const float* __restrict__ yp = y + base;
  const int ca = m0 + t, cb = m0 + NT + t;
  const bool va = ca < W, vb = t < HALO && cb < W;
  const bool mvalid = ca < Wm;
  const SsimShift sh = make_shift(block_shift(xp, yp, W, o0, o0 + nin, ca, va, cb, vb, raw[0][0]), S);
  const float shift = sh.c;
  float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;                    // the next row, in flight
  {
    const int64_t r = (int64_t)o0 * W;
    if (va) { ax = xp[r + ca] - shift; ay = yp[r + ca] - shift; }
    if (vb) { bx = xp[r + cb] - shift; by = yp[r + cb] - shift; }
  }
  float ring[5][TAPS];
  double acc_s = 0.0, acc_c = 0.0;
  for (int i0 = 0; i0 < nin; i0 += TAPS) {
#pragma unroll
    for (int s = 0; s < TAPS; ++s) {
      const int i = i0 + s;
      if (i >= nin) continue;                                       // uniform over the workgroup (no `break`: an early exit keeps the loop rolled)
      float* rx = raw[i & 1][0];
      float* ry = raw[i & 1][1];
      rx[t] = ax; ry[t] = ay;
      if (t < HALO) { rx[NT + t] = bx; ry[NT + t] = by; }
      if (i + 1 < nin) {
        const int64_t r = (int64_t)(o0 + i + 1) * W;
        if (va) { ax = xp[r + ca] - shift; ay = yp[r + ca] - shift; }
        if (vb) { bx = xp[r + cb] - shift; by = yp[r + cb] - shift; }
      }
      __syncthreads();                                              // (two raw buffers: the one written two steps back is free by now)
      float h[5];
      hfilter5(rx, ry, t, g, h);
#pragma unroll
      for (int q = 0; q < 5; ++q) ring[q][s] = h[q];
      if (i >= HALO) {
        float m[5];
        vfilter5(ring, s, g, m);
        const SsimPoint p = ssim_point(m, sh, C1, C2);
        if (mvalid) { acc_s += (double)p.ssim; acc_c += (double)p.cs; }
      }
    }
  }
  red[0][t] = acc_s;
  red[1][t] = acc_c;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    const int64_t k = (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    partial[k] = red[0][0];
    partial[k + 1] = red[1][0];
  }
}

// one thread per plane: the partial sums of the plane in their fixed order -> out[plane] = mean SSIM, out[P + plane] = mean cs
__global__ __launch_bounds__(64) void ssim_finish_kernel(const double* __restrict__ partial, int P, int per_plane, double n_map, double* __restrict__ out) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= P) return;
  double s = 0.0, c = 0.0;
  for (int k = 0; k < per_plane; ++k) {
    s += partial[((int64_t)p * per_plane + k) * 2];
    c += partial[((int64_t)p * per_plane + k) * 2 + 1];
  }
  out[p] = s / n_map;
  out[P + p] = c / n_map;
}

// ------------------------------------------------------------------------------------------------------------------------------- adjoint
// d loss / d y of  sum_planes (g_ssim[p] mean(ssim map) + g_cs[p] mean(cs map)), plus 0.25 g_coarse[(r + pad) / 2][(c + pad) / 2] (the pooling adjoint
// of the next MS-SSIM level).  grid: (strips of GRAD_TW gradient columns, chunks of `rows` gradient rows, planes).  Thread t stands for column
// c0 - 10 + t twice: as a map column (moments, coefficients) and, 10 columns later in the filter, as a gradient column (t >= 10).
__global__ __launch_bounds__(NT) void ssim_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g_ssim,
                                                       const float* __restrict__ g_cs, const float* __restrict__ g_coarse, int H, int W, int rows,
                                                       SsimWin g, double S, float C1, float C2, float inv_n, float* __restrict__ dy) {
  __shared__ float raw[2][2][RAWW];
  __shared__ float coef[3][NT];
  const int t = threadIdx.x;
  const int Hm = H - HALO, Wm = W - HALO;
  const int cm = blockIdx.x * GRAD_TW - HALO + t;                  // this thread's column
  const int r0 = blockIdx.y * rows;
  const int r1 = min(r0 + rows, H);
  const int rin0 = r0 - HALO;                                      // gradient rows r0 .. r1 - 1 <- map rows r0 - 10 .. r1 - 1 <- input rows r0 - 10 .. r1 + 9
  const int nin = (r1 - r0) + 2 * HALO;
  const int64_t base = (int64_t)blockIdx.z * H * W;
  const float* __restrict__ xp = x + base;
  const float* __restrict__ yp = y + base;
  const float gs = g_ssim[blockIdx.z], gc = g_cs[blockIdx.z];
  const int cb = cm + NT;
  const bool va = cm >= 0 && cm < W, vb = t < HALO && cb < W;
  const bool mcol = cm >= 0 && cm < Wm;
  const bool gcol = t >= HALO && cm < W;
  const int padh = H & 1, padw = W & 1, Wc = (W + padw) / 2, Hc = (H + padh) / 2;
  const SsimShift sh = make_shift(block_shift(xp, yp, W, max(rin0, 0), min(rin0 + nin, H), cm, va, cb, vb, raw[0][0]), S);
  const float shift = sh.c;
  float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;                    // the next row, in flight (rows outside the plane: zeros, their map rows are masked)
  if (rin0 >= 0) {
    const int64_t r = (int64_t)rin0 * W;
    if (va) { ax = xp[r + cm] - shift; ay = yp[r + cm] - shift; }
    if (vb) { bx = xp[r + cb] - shift; by = yp[r + cb] - shift; }
  }
  float ring[5][TAPS], ring2[3][TAPS];
  for (int i0 = 0; i0 < nin; i0 += TAPS) {
#pragma unroll
    for (int s = 0; s < TAPS; ++s) {
      const int i = i0 + s;
      if (i >= nin) continue;                                       // uniform over the workgroup (no `break`: an early exit keeps the loop rolled)
      float* rx = raw[i & 1][0];
      float* ry = raw[i & 1][1];
      rx[t] = ax; ry[t] = ay;
      if (t < HALO) { rx[NT + t] = bx; ry[NT + t] = by; }
      ax = ay = bx = by = 0.f;
      const int rn = rin0 + i + 1;
      if (i + 1 < nin && rn >= 0 && rn < H) {
        const int64_t r = (int64_t)rn * W;
        if (va) { ax = xp[r + cm] - shift; ay = yp[r + cm] - shift; }
        if (vb) { bx = xp[r + cb] - shift; by = yp[r + cb] - shift; }
      }
      __syncthreads();
      float h[5];
      hfilter5(rx, ry, t, g, h);
#pragma unroll
      for (int q = 0; q < 5; ++q) ring[q][s] = h[q];
      if (i >= HALO) {                                              // uniform
        const int mo = rin0 + i - HALO;                            // map row finished by this input row; also the gradient row of this step
        float m[5];
        vfilter5(ring, s, g, m);
        const SsimPoint p = ssim_point(m, sh, C1, C2);
        // T = gs ssim + gc cs at this position; A = dT/d mu_y, B = dT/d E[y^2], Cc = dT/d E[xy] (moments of the shifted frames)
        const float qv = gs * p.l + gc;                             // dT / d cs
        const float B = -qv * p.cs * p.inv_dc;
        const float Cc = 2.f * qv * p.inv_dc;
        const float A = 2.f * gs * p.cs * (p.M1 - p.l * p.M2) * p.inv_dl + 2.f * qv * (p.cs * m[1] - m[0] + sh.k1 * (1.f - p.cs)) * p.inv_dc;
        const bool ok = mcol && mo >= 0 && mo < Hm;
        coef[0][t] = ok ? A : 0.f;                                  // (free: every thread is past the previous step's reads at the barrier above)
        coef[1][t] = ok ? B : 0.f;
        coef[2][t] = ok ? Cc : 0.f;
        __syncthreads();
        float fa = 0.f, fb = 0.f, fc = 0.f;
        if (t >= HALO) {
#pragma unroll
          for (int j = 0; j < TAPS; ++j) {
            fa += g.w[j] * coef[0][t - j];
            fb += g.w[j] * coef[1][t - j];
            fc += g.w[j] * coef[2][t - j];
          }
        }
        ring2[0][s] = fa; ring2[1][s] = fb; ring2[2][s] = fc;
        if (i >= 2 * HALO) {                                        // uniform: gradient row mo in [r0, r1)
          float ta = 0.f, tb = 0.f, tc = 0.f;
#pragma unroll
          for (int k = 0; k < TAPS; ++k) {
            ta += g.w[k] * ring2[0][(s + TAPS - k) % TAPS];
            tb += g.w[k] * ring2[1][(s + TAPS - k) % TAPS];
            tc += g.w[k] * ring2[2][(s + TAPS - k) % TAPS];
          }
          if (gcol) {
            const int64_t o = (int64_t)mo * W + cm;
            const float xs = xp[o] - shift, ys = yp[o] - shift;
            float v = (ta + 2.f * ys * tb + xs * tc) * inv_n;
            if (g_coarse) v += 0.25f * g_coarse[((int64_t)blockIdx.z * Hc + (mo + padh) / 2) * Wc + (cm + padw) / 2];
            dy[base + o] = v;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------- pooling
// F.avg_pool2d(kernel 2, padding side % 2), zeros counted (losses/ssim.py:237-239), of x and y in one launch
__global__ __launch_bounds__(256) void avgpool2_pad_kernel(const float* __restrict__ x, const float* __restrict__ y, int P, int H, int W, int Hc, int Wc,
                                                           float* __restrict__ xo, float* __restrict__ yo) {
  const int ph = H & 1, pw = W & 1;
  const int64_t n = (int64_t)P * Hc * Wc;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int oc = (int)(q % Wc);
    const int64_t q2 = q / Wc;
    const int orow = (int)(q2 % Hc);
    const int64_t p = q2 / Hc;
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr) {
#pragma unroll
      for (int dc = 0; dc < 2; ++dc) {
        const int r = 2 * orow - ph + dr, c = 2 * oc - pw + dc;
        if (r >= 0 && r < H && c >= 0 && c < W) {
          const int64_t o = (p * H + r) * W + c;
          sx += x[o];
          sy += y[o];
        }
      }
    }
    xo[q] = sx * 0.25f;
    yo[q] = sy * 0.25f;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ JND term
// mean((|imgs_w - imgs| - h)^2) over [F, 3, H, W], h [F, 1, H, W] broadcast over the channels (jndloss.py:27-31)
__global__ __launch_bounds__(256) void jnd_loss_partial_kernel(const float* __restrict__ imgs, const float* __restrict__ imgs_w,
                                                               const float* __restrict__ hmap, int64_t n, int64_t plane, double* __restrict__ partial) {
  __shared__ double red[256];
  double acc = 0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int64_t f = q / (3 * plane), i = q % plane;
    const float e = fabsf(imgs_w[q] - imgs[q]) - hmap[f * plane + i];
    acc += (double)e * e;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void jnd_loss_finish_kernel(const double* __restrict__ partial, int nblk, double n_elem, float* __restrict__ loss) {
  __shared__ double red[256];
  double acc = 0;
  for (int k = threadIdx.x; k < nblk; k += 256) acc += partial[k];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / n_elem);
}
// 2 (|d| - h) sign(d) / N with sign(0) = 0 (torch's abs has derivative 0 at 0, and clamped pixels give d = 0 exactly)
__global__ __launch_bounds__(256) void jnd_loss_grad_kernel(const float* __restrict__ imgs, const float* __restrict__ imgs_w, const float* __restrict__ hmap,
                                                            int64_t n, int64_t plane, float gscale, float* __restrict__ d_imgs_w) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int64_t f = q / (3 * plane), i = q % plane;
    const float d = imgs_w[q] - imgs[q];
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    d_imgs_w[q] = gscale * (fabsf(d) - hmap[f * plane + i]) * sg;
  }
}

// rows per chunk: start from `want`, halve while the grid would leave most of the 256 CUs without a workgroup
int pick_rows(int want, int lo, int64_t strips_planes, int total_rows) {
  int rows = want;
  while (rows > lo && strips_planes * ((total_rows + rows - 1) / rows) < 1024) rows /= 2;
  return rows;
}
constexpr int STATS_ROWS = 96, STATS_ROWS_MIN = 24, GRAD_ROWS = 128, GRAD_ROWS_MIN = 32;

struct StatsGrid { int strips, chunks, rows; };
StatsGrid stats_grid(int P, int H, int W) {
  StatsGrid q;
  q.strips = (W - HALO + NT - 1) / NT;
  q.rows = pick_rows(STATS_ROWS, STATS_ROWS_MIN, (int64_t)q.strips * P, H - HALO);
  q.chunks = (H - HALO + q.rows - 1) / q.rows;
  return q;
}

double window_sum(const SsimWin& g) {
  double S = 0.0;
  for (int k = 0; k < TAPS; ++k) S += (double)g.w[k];
  return S * S;                            // the separable filter's 2-D weights sum to (sum w)^2
}

bool ssim_shape_ok(int P, int H, int W) { return P > 0 && P <= 65535 && H >= TAPS && W >= TAPS && H <= (1 << 20) && W <= (1 << 20); }

}  // namespace

// ===================================================================================================== C-ABI
extern "C" int64_t vs_ssim_partial_doubles(int P, int H, int W) {
  if (!ssim_shape_ok(P, H, W)) return 0;
  const StatsGrid q = stats_grid(P, H, W);
  return 2 * (int64_t)P * q.strips * q.chunks;
}

extern "C" int vs_ssim_stats(const float* x, const float* y, int P, int H, int W, float data_range, const float* win11, double* partial, double* out,
                             void* stream) {
  VS_REQUIRE(x && y && win11 && partial && out && ssim_shape_ok(P, H, W) && data_range > 0.f);
  SsimWin g;
  for (int k = 0; k < TAPS; ++k) g.w[k] = win11[k];
  const StatsGrid q = stats_grid(P, H, W);
  const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
  hipLaunchKernelGGL(ssim_stats_kernel, dim3(q.strips, q.chunks, P), dim3(NT), 0, (hipStream_t)stream, x, y, H, W, q.rows, g, window_sum(g), C1, C2,
                     partial);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((P + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)partial, P, q.strips * q.chunks,
                     (double)(H - HALO) * (double)(W - HALO), out);
  return vs_launch_status();
}

extern "C" int vs_ssim_grad(const float* x, const float* y, const float* g_ssim, const float* g_cs, const float* g_coarse, int P, int H, int W,
                            float data_range, const float* win11, float* dy, void* stream) {
  VS_REQUIRE(x && y && g_ssim && g_cs && win11 && dy && ssim_shape_ok(P, H, W) && data_range > 0.f);
  SsimWin g;
  for (int k = 0; k < TAPS; ++k) g.w[k] = win11[k];
  const int strips = (W + GRAD_TW - 1) / GRAD_TW;
  const int rows = pick_rows(GRAD_ROWS, GRAD_ROWS_MIN, (int64_t)strips * P, H);
  const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
  const float inv_n = (float)(1.0 / ((double)(H - HALO) * (double)(W - HALO)));
  hipLaunchKernelGGL(ssim_grad_kernel, dim3(strips, (H + rows - 1) / rows, P), dim3(NT), 0, (hipStream_t)stream, x, y, g_ssim, g_cs, g_coarse, H, W, rows, g,
                     window_sum(g), C1, C2, inv_n, dy);
  return vs_launch_status();
}

extern "C" int vs_avgpool2_pad(const float* x, const float* y, int P, int H, int W, float* xo, float* yo, void* stream) {
  VS_REQUIRE(x && y && xo && yo && P > 0 && H > 0 && W > 0);
  const int Hc = (H + (H & 1)) / 2, Wc = (W + (W & 1)) / 2;
  hipLaunchKernelGGL(avgpool2_pad_kernel, dim3(gridx((int64_t)P * Hc * Wc)), dim3(256), 0, (hipStream_t)stream, x, y, P, H, W, Hc, Wc, xo, yo);
  return vs_launch_status();
}

extern "C" int64_t vs_jnd_loss_partial_doubles(int F, int H, int W) { return gridx((int64_t)F * 3 * H * W, 256, 1024); }

extern "C" int vs_jnd_loss(const float* imgs, const float* imgs_w, const float* hmap, int F, int H, int W, double* partial, float* loss, void* stream) {
  VS_REQUIRE(imgs && imgs_w && hmap && partial && loss && F > 0 && H > 0 && W > 0);
  const int64_t plane = (int64_t)H * W, n = 3 * (int64_t)F * plane;
  const int nblk = (int)gridx(n, 256, 1024);
  hipLaunchKernelGGL(jnd_loss_partial_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, imgs, imgs_w, hmap, n, plane, partial);
  hipLaunchKernelGGL(jnd_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partial, nblk, (double)n, loss);
  return vs_launch_status();
}

extern "C" int vs_jnd_loss_grad(const float* imgs, const float* imgs_w, const float* hmap, int F, int H, int W, float upstream, float* d_imgs_w,
                                void* stream) {
  VS_REQUIRE(imgs && imgs_w && hmap && d_imgs_w && F > 0 && H > 0 && W > 0);
  const int64_t plane = (int64_t)H * W, n = 3 * (int64_t)F * plane;
  hipLaunchKernelGGL(jnd_loss_grad_kernel, dim3(gridx(n)), dim3(256), 0, (hipStream_t)stream, imgs, imgs_w, hmap, n, plane,
                     (float)((double)upstream * 2.0 / (double)n), d_imgs_w);
  return vs_launch_status();
}
