// PatchGAN discriminator of the adversarial term (modules/discriminator.py:89-148, losses/videosealloss.py:16-31, 128-135, 192-214): what the
// 4 x 4 convolution stack needs besides vs_conv_gemm (dense forward convolutions, backward-data on flipped weights).  gfx950 only.
//   disc_input / disc_input_bwd      NCHW frames -> the NHWC rows of layer 1 (RGB, or Y = M[0] . rgb) and the adjoint
//   groupnorm_lrelu (+ _bwd)         GroupNorm(4, C) over (C / 4, H, W) per frame + affine + LeakyReLU on NHWC rows; a plain LeakyReLU form
//   conv4x4_wgrad                    dw[n][tap * ld + c] of a 4 x 4 conv (zero pad 1, stride 1 | 2) straight from the image: fp32 matrix cores
//                                    (v_mfma_f32_32x32x2_f32) on the implicit patch matrix; a reduction kernel for the one-column last layer
//   conv4x4_n1 (+ _bwd)              the last layer (C -> 1, stride 1): one wave per logit; its backward-data as a 16-tap gather
//   disc_loss                        -mean(fake) | hinge loss, their gradients and the two logit means in one workgroup
// Every reduction is deterministic: fixed chunks, fixed summation order, fp64 across chunks, plain vector stores, no atomics.
#include "vs_common.h"

namespace {

constexpr int GN_ROWS = 64;        // rows per chunk of the GroupNorm reductions (chunks never straddle a frame)
constexpr int W1_ROWS = 128;       // output pixels per chunk of the one-column weight gradient

static inline unsigned blocks_for(int64_t n) { return (unsigned)cdiv64(n, 256); }

// out[i] = sum_k partial[k][i] (fp64, order fixed by nchunk): 64 elements x 4 chunk lanes per workgroup
__global__ __launch_bounds__(256) void disc_reduce_chunks_kernel(const float* __restrict__ partial, int nchunk, int64_t n, float* __restrict__ out) {
  __shared__ double sh[4][64];
  const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + e;
  double s = 0;
  if (i < n)
    for (int k = g; k < nchunk; k += 4) s += (double)partial[(int64_t)k * n + i];
  sh[g][e] = s;
  __syncthreads();
  if (g == 0 && i < n) out[i] = (float)(((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e]);
}

// ---------------------------------------------------------------------------------------------------
// input rows: [B][3][H][W] -> [B * H * W][4] = (r, g, b, 0), or (y, 0, 0, 0) with y = m0 . rgb (discriminator.py:146-147: the [0, 1] image as it is)
__global__ __launch_bounds__(256) void disc_input_kernel(const float* __restrict__ imgs, int HW, int64_t total, const float* __restrict__ m0,
                                                         float* __restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / HW, p = idx - b * HW;
  const float* s = imgs + b * 3 * HW + p;
  const float r = s[0], g = s[HW], bl = s[2 * (int64_t)HW];
  f32x4 o = {r, g, bl, 0.f};
  if (m0) o = f32x4{m0[0] * r + m0[1] * g + m0[2] * bl, 0.f, 0.f, 0.f};
  *reinterpret_cast<f32x4*>(rows + 4 * idx) = o;
}
__global__ __launch_bounds__(256) void disc_input_bwd_kernel(const float* __restrict__ drows, int HW, int64_t total, const float* __restrict__ m0,
                                                             float* __restrict__ dimgs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / HW, p = idx - b * HW;
  const f32x4 d = *reinterpret_cast<const f32x4*>(drows + 4 * idx);
  float* o = dimgs + b * 3 * HW + p;
  o[0] = m0 ? m0[0] * d[0] : d[0];
  o[HW] = m0 ? m0[1] * d[0] : d[1];
  o[2 * (int64_t)HW] = m0 ? m0[2] * d[0] : d[2];
}

// ---------------------------------------------------------------------------------------------------
// GroupNorm statistics.  Workgroup = (frame, chunk of GN_ROWS rows); thread = (row lane, 4 channels): C4 = C / 4 divides 256 and a 4-channel
// piece lies in one group (C % 16 == 0).  Per thread fp64 sums over its rows, then per group a fixed-order sum over the threads of the group.
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, int64_t ld, int HW, int nch, int C4, double* __restrict__ part) {
  __shared__ double sh[256][2];
  const int frame = blockIdx.x / nch, ch = blockIdx.x - frame * nch;
  const int c4 = threadIdx.x % C4, lr = threadIdx.x / C4, R = 256 / C4;
  const int r0 = ch * GN_ROWS, r1 = r0 + GN_ROWS < HW ? r0 + GN_ROWS : HW;
  double s = 0, ss = 0;
  for (int r = r0 + lr; r < r1; r += R) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((int64_t)frame * HW + r) * ld + 4 * c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { s += (double)v[e]; ss += (double)v[e] * (double)v[e]; }
  }
  sh[threadIdx.x][0] = s;
  sh[threadIdx.x][1] = ss;
  __syncthreads();
  if (threadIdx.x < 8) {
    const int g = threadIdx.x >> 1, v = threadIdx.x & 1, G4 = C4 / 4;       // group g = pieces g * G4 .. (g + 1) * G4 - 1
    double t = 0;
    for (int l = 0; l < R; ++l)
      for (int q = 0; q < G4; ++q) t += sh[l * C4 + g * G4 + q][v];
    part[((int64_t)blockIdx.x * 4 + g) * 2 + v] = t;
  }
}
// one thread per (frame, group): chunks in order -> mean, 1 / sqrt(biased variance + eps).  Both stay fp64: rounded to fp32 they would move every value of
// a (frame, group) the same way, an error that does not average out in the sums over a frame (the logit means, the hinge step's cancelling halves)
__global__ __launch_bounds__(256) void gn_finish_kernel(const double* __restrict__ part, int B, int nch, double count, float eps, double* __restrict__ mean,
                                                        double* __restrict__ rstd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * B) return;
  const int frame = i >> 2, g = i & 3;
  double s = 0, ss = 0;
  for (int k = 0; k < nch; ++k) {
    s += part[(((int64_t)frame * nch + k) * 4 + g) * 2];
    ss += part[(((int64_t)frame * nch + k) * 4 + g) * 2 + 1];
  }
  const double m = s / count;
  double var = ss / count - m * m;
  if (var < 0) var = 0;
  mean[i] = m;
  rstd[i] = 1.0 / sqrt(var + (double)eps);
}
// y = (x - mean) * rstd * gamma + beta (or y = x without a norm), out = y > 0 ? y : slope * y; pad columns of the output row are zeroed
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, int64_t ld, int HW, int C, int O4, int64_t total,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, const double* __restrict__ mean,
                                                       const double* __restrict__ rstd, float slope, float* __restrict__ out, int64_t out_ld) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (row, c4 of the output row)
  if (idx >= total) return;
  const int c4 = (int)(idx % O4);
  const int64_t r = idx / O4;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (4 * c4 < C) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ld + 4 * c4);
    double m = 0, rs = 1;
    if (mean) {
      const int64_t f = r / HW;
      const int g = (4 * c4) / (C >> 2);
      m = mean[4 * f + g];
      rs = rstd[4 * f + g];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * c4 + e < C) {
        float y = v[e];
        if (mean) y = (float)(((double)v[e] - m) * rs) * gamma[4 * c4 + e] + beta[4 * c4 + e];
        o[e] = y > 0.f ? y : slope * y;
      }
  }
  *reinterpret_cast<f32x4*>(out + r * out_ld + 4 * c4) = o;
}

// backward, first pass: per (frame, chunk) the column sums of dyh * xhat and dyh, dyh = dy * (y > 0 ? 1 : slope)
__global__ __launch_bounds__(256) void gn_bwd_cols_kernel(const float* __restrict__ x, int64_t ld, const float* __restrict__ dy, int64_t dy_ld, int HW, int nch,
                                                          int C4, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const double* __restrict__ mean, const double* __restrict__ rstd, float slope,
                                                          double* __restrict__ part) {
  __shared__ double sh[256][8];
  const int frame = blockIdx.x / nch, ch = blockIdx.x - frame * nch;
  const int c4 = threadIdx.x % C4, lr = threadIdx.x / C4, R = 256 / C4;
  const int r0 = ch * GN_ROWS, r1 = r0 + GN_ROWS < HW ? r0 + GN_ROWS : HW;
  const int g = c4 / (C4 / 4);
  const double m = mean[4 * frame + g], rs = rstd[4 * frame + g];
  const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + 4 * c4), be = *reinterpret_cast<const f32x4*>(beta + 4 * c4);
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0 + lr; r < r1; r += R) {
    const int64_t row = (int64_t)frame * HW + r;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * ld + 4 * c4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + row * dy_ld + 4 * c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double xh = ((double)v[e] - m) * rs;
      const float y = (float)xh * ga[e] + be[e];
      const float dh = y > 0.f ? d[e] : slope * d[e];
      a[e] += (double)dh * xh;
      a[4 + e] += (double)dh;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sh[threadIdx.x][e] = a[e];
  __syncthreads();
  // part[block][v][C]: v = 0 -> sum dyh * xhat, v = 1 -> sum dyh; the row lanes are added in lane order
  for (int o = threadIdx.x; o < 8 * C4; o += 256) {
    const int q = o >> 3, j = o & 7;
    double t = 0;
    for (int l = 0; l < R; ++l) t += sh[l * C4 + q][j];
    part[((int64_t)blockIdx.x * 2 + (j >> 2)) * (4 * C4) + 4 * q + (j & 3)] = t;
  }
}
// second pass, one workgroup per frame: chunks in order -> the frame's column sums fcols[frame][2][C]; then the group sums
// gsum[frame][group][2] = (sum_c gamma_c * sum dyh, sum_c gamma_c * sum dyh xhat): sum dxhat and sum dxhat * xhat of the group
__global__ __launch_bounds__(256) void gn_bwd_frame_kernel(const double* __restrict__ part, int nch, int C, const float* __restrict__ gamma,
                                                           double* __restrict__ fcols, double* __restrict__ gsum) {
  const int frame = blockIdx.x;
  for (int o = threadIdx.x; o < 2 * C; o += 256) {
    double t = 0;
    for (int k = 0; k < nch; ++k) t += part[((int64_t)frame * nch + k) * 2 * C + o];
    fcols[(int64_t)frame * 2 * C + o] = t;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int g = threadIdx.x >> 1, v = threadIdx.x & 1, Cg = C >> 2;
    double t = 0;
    for (int c = g * Cg; c < (g + 1) * Cg; ++c) t += (double)gamma[c] * fcols[(int64_t)frame * 2 * C + (v ? 0 : C) + c];
    gsum[((int64_t)frame * 4 + g) * 2 + v] = t;
  }
}
// d gamma[c] = sum_frames fcols[f][0][c], d beta[c] = sum_frames fcols[f][1][c]
__global__ __launch_bounds__(256) void gn_bwd_param_kernel(const double* __restrict__ fcols, int B, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0, b = 0;
  for (int f = 0; f < B; ++f) {
    a += fcols[(int64_t)f * 2 * C + c];
    b += fcols[(int64_t)f * 2 * C + C + c];
  }
  dgamma[c] = (float)a;
  dbeta[c] = (float)b;
}
// dx = rstd * (dxhat - S1 / n - xhat * S2 / n), dxhat = dyh * gamma; without a norm dx = dy * (x > 0 ? 1 : slope).  Pad columns of dx are zeroed.
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, int64_t ld, const float* __restrict__ dy, int64_t dy_ld, int HW, int C,
                                                           int O4, int64_t total, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const double* __restrict__ mean, const double* __restrict__ rstd, const double* __restrict__ gsum,
                                                           double inv_n, float slope, float* __restrict__ dx, int64_t dx_ld) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % O4);
  const int64_t r = idx / O4;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (4 * c4 < C) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ld + 4 * c4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + r * dy_ld + 4 * c4);
    if (!mean) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * c4 + e < C) o[e] = v[e] > 0.f ? d[e] : slope * d[e];
    } else {
      const int64_t f = r / HW;
      const int g = (4 * c4) / (C >> 2);
      const double m = mean[4 * f + g], rs = rstd[4 * f + g];
      const double s1 = gsum[(4 * f + g) * 2] * inv_n, s2 = gsum[(4 * f + g) * 2 + 1] * inv_n;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double xh = ((double)v[e] - m) * rs;
        const float ga = gamma[4 * c4 + e];
        const float y = (float)xh * ga + beta[4 * c4 + e];
        const float dh = y > 0.f ? d[e] : slope * d[e];
        o[e] = (float)(rs * ((double)dh * (double)ga - s1 - xh * s2));
      }
    }
  }
  *reinterpret_cast<f32x4*>(dx + r * dx_ld + 4 * c4) = o;
}

// ---------------------------------------------------------------------------------------------------
// Weight gradient of a 4 x 4 conv (zero padding 1, stride cs) on the fp32 matrix cores: dw[n][tap * ld + c] = sum over output pixels r = (b, oy, ox)
// of dy[r][n] * x[b, oy * cs + ky - 1, ox * cs + kx - 1, c].  The reduction index of v_mfma_f32_32x32x2_f32 is the pixel, so both fragments are plain
// reads of 32 consecutive columns of two rows; the X operand is the implicit patch matrix (column kc = tap * ld + c; ld % 4 == 0 keeps a
// 16-byte piece inside one tap).  Workgroup = 128 (n) x 128 (kc) outputs, 4 waves of 64 x 64, 16 pixels per LDS step, the next step's rows are
// fetched while the matrix cores work; pixels are split over blockIdx.z and the slices' partial results summed by disc_reduce_chunks_kernel.
struct c4w_t { int H, W, Ho, Wo, cs; };
__global__ __launch_bounds__(256) void conv4x4_wgrad_mfma_kernel(const float* __restrict__ dy, int64_t dy_ld, int N, const float* __restrict__ x, int64_t ld,
                                                                 int K16, int64_t rows, int64_t rows_per_split, float* __restrict__ partial, const c4w_t cv) {
  __shared__ __attribute__((aligned(16))) float sa[16][128], sb[16][128];
  const int n0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
  const int64_t r_begin = (int64_t)blockIdx.z * rows_per_split;
  const int64_t r_end = r_begin + rows_per_split < rows ? r_begin + rows_per_split : rows;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wy = wave >> 1, wx = wave & 1;
  const int lr = threadIdx.x >> 5, lc = (threadIdx.x & 31) * 4;       // staging: rows lr and lr + 8, 4 floats at column lc
  const int kq = lane >> 5, c = lane & 31;
  const bool a_ok = n0 + lc + 4 <= dy_ld;                             // columns past N only feed outputs that are never stored
  const int kc = k0 + lc;
  const bool b_ok = kc + 4 <= K16;
  const int tap = b_ok ? kc / (int)ld : 0;
  const int cc = b_ok ? kc - tap * (int)ld : 0;
  const int ky = tap >> 2, kx = tap & 3;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  f32x4 va[2], vb[2];
  auto fetch = [&](const int64_t r0) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t r = r0 + lr + 8 * h;
      va[h] = f32x4{0.f, 0.f, 0.f, 0.f};
      vb[h] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (r < r_end) {
        if (a_ok) va[h] = *reinterpret_cast<const f32x4*>(dy + r * dy_ld + n0 + lc);
        if (b_ok) {
          const unsigned rf = (unsigned)r;
          const unsigned q = rf / (unsigned)cv.Wo;
          const int ox = (int)(rf - q * (unsigned)cv.Wo);
          const unsigned b = q / (unsigned)cv.Ho;
          const int oy = (int)(q - b * (unsigned)cv.Ho);
          const int iy = oy * cv.cs + ky - 1, ix = ox * cv.cs + kx - 1;
          if (iy >= 0 && iy < cv.H && ix >= 0 && ix < cv.W)
            vb[h] = *reinterpret_cast<const f32x4*>(x + (((int64_t)b * cv.H + iy) * cv.W + ix) * ld + cc);
        }
      }
    }
  };
  fetch(r_begin);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += 16) {
    __syncthreads();                       // the previous step's fragment reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<f32x4*>(&sa[lr + 8 * h][lc]) = va[h];
      *reinterpret_cast<f32x4*>(&sb[lr + 8 * h][lc]) = vb[h];
    }
    __syncthreads();
    if (r0 + 16 < r_end) fetch(r0 + 16);
#pragma unroll
    for (int rr = 0; rr < 16; rr += 2) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = sa[rr + kq][wy * 64 + i * 32 + c];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = sb[rr + kq][wx * 64 + j * 32 + c];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // D[m][n]: lane holds column n = lane & 31 and rows m = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  float* p = partial + (int64_t)blockIdx.z * N * K16;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wx * 64 + j * 32 + c;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = n0 + wy * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kq;
        if (n < N && k < K16) p[(int64_t)n * K16 + k] = acc[i][j][e];
      }
    }
}

// The one-column layer (N = 1): dw[tap * ld + c] = sum_r dy[r] * x[patch(r)][tap * ld + c].  Workgroup = (chunk of W1_ROWS pixels, 256 16-byte
// column pieces); a thread walks the chunk's pixels in order with its piece in registers.
__global__ __launch_bounds__(256) void conv4x4_wgrad_n1_kernel(const float* __restrict__ dy, int64_t dy_ld, const float* __restrict__ x, int64_t ld, int K16,
                                                               int64_t rows, float* __restrict__ partial, const c4w_t cv) {
  const int kc = 4 * (blockIdx.y * 256 + threadIdx.x);
  if (kc >= K16) return;
  const int tap = kc / (int)ld, cc = kc - tap * (int)ld;
  const int ky = tap >> 2, kx = tap & 3;
  const int64_t r0 = (int64_t)blockIdx.x * W1_ROWS;
  const int64_t r1 = r0 + W1_ROWS < rows ? r0 + W1_ROWS : rows;
  const unsigned q = (unsigned)r0 / (unsigned)cv.Wo;
  int ox = (int)((unsigned)r0 - q * (unsigned)cv.Wo);
  unsigned b = q / (unsigned)cv.Ho;
  int oy = (int)(q - b * (unsigned)cv.Ho);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0; r < r1; ++r) {
    const int iy = oy * cv.cs + ky - 1, ix = ox * cv.cs + kx - 1;
    if (iy >= 0 && iy < cv.H && ix >= 0 && ix < cv.W)
      acc += dy[r * dy_ld] * *reinterpret_cast<const f32x4*>(x + (((int64_t)b * cv.H + iy) * cv.W + ix) * ld + cc);
    if (++ox == cv.Wo) { ox = 0; if (++oy == cv.Ho) { oy = 0; ++b; } }
  }
  *reinterpret_cast<f32x4*>(partial + (int64_t)blockIdx.x * K16 + kc) = acc;
}

// ---------------------------------------------------------------------------------------------------
// last layer forward: out[b, oy, ox] = bias + sum_{tap, c} w[tap * ld + c] * x[b, oy + ky - 1, ox + kx - 1, c]; one wave per output pixel
__global__ __launch_bounds__(256) void conv4x4_n1_kernel(const float* __restrict__ x, int64_t ld, int H, int W, int Ho, int Wo, int64_t rows,
                                                         const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                   // (whole waves leave: no barrier follows)
  const int lane = threadIdx.x & 63;
  const unsigned q = (unsigned)r / (unsigned)Wo;
  const int ox = (int)((unsigned)r - q * (unsigned)Wo);
  const unsigned b = q / (unsigned)Ho;
  const int oy = (int)(q - b * (unsigned)Ho);
  const int L4 = (int)(ld >> 2);
  // fp64 sums: a logit is a sum of 16 * C products of both signs, several times larger in total than the result; fp32 accumulation leaves an
  // error of ~1e-6 per logit (torch's fp32 convolution does) that the means over a frame do not average out.  The layer is 1 % of the network.
  double s = 0;
  for (int tap = 0; tap < 16; ++tap) {
    const int iy = oy + (tap >> 2) - 1, ix = ox + (tap & 3) - 1;
    if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
    const float* px = x + (((int64_t)b * H + iy) * W + ix) * ld;
    const float* pw = w + (int64_t)tap * ld;
    for (int c4 = lane; c4 < L4; c4 += 64) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(px + 4 * c4), k = *reinterpret_cast<const f32x4*>(pw + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += (double)v[e] * (double)k[e];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) out[r] = (float)(s + (bias ? (double)bias[0] : 0.0));
}
// its backward-data: dx[b, iy, ix, c] = sum_tap dy[b, iy - ky + 1, ix - kx + 1] * w[tap * ld + c] (gather over the 16 taps, fixed order)
__global__ __launch_bounds__(256) void conv4x4_n1_bwd_kernel(const float* __restrict__ dy, int H, int W, int Ho, int Wo, int64_t ld, int64_t total,
                                                             const float* __restrict__ w, float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (pixel, c4)
  if (idx >= total) return;
  const int L4 = (int)(ld >> 2);
  const int c4 = (int)(idx % L4);
  const int64_t pix = idx / L4;
  const int ix = (int)(pix % W);
  const int64_t t = pix / W;
  const int iy = (int)(t % H);
  const int64_t b = t / H;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 16; ++tap) {
    const int oy = iy - (tap >> 2) + 1, ox = ix - (tap & 3) + 1;
    if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) continue;
    acc += dy[(b * Ho + oy) * Wo + ox] * *reinterpret_cast<const f32x4*>(w + (int64_t)tap * ld + 4 * c4);
  }
  *reinterpret_cast<f32x4*>(dx + pix * ld + 4 * c4) = acc;
}

// ---------------------------------------------------------------------------------------------------
// 256-thread fp64 sum, lanes combined in a fixed order; every thread gets the total
__device__ __forceinline__ double disc_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}
// hinge = 0: loss = -mean(fake), d fake = -gscale / n_f (videosealloss.py:133-134).  hinge = 1: loss = 0.5 (mean relu(1 - real) + mean relu(1 + fake)),
// d real = -0.5 gscale / n_r where 1 - real > 0, d fake = 0.5 gscale / n_f where 1 + fake > 0 (videosealloss.py:16-23).  out = (loss, mean real,
// mean fake, 0); the loss itself is not multiplied with gscale.
__global__ __launch_bounds__(256) void disc_loss_kernel(const float* __restrict__ real, int64_t n_r, const float* __restrict__ fake, int64_t n_f, int hinge,
                                                        float gscale, float* __restrict__ dreal, float* __restrict__ dfake, float* __restrict__ out) {
  __shared__ double sh[256];
  double s_r = 0, s_f = 0, h_r = 0, h_f = 0;
  const float gr = n_r > 0 ? -0.5f * gscale / (float)n_r : 0.f;
  const float gf = hinge ? 0.5f * gscale / (float)n_f : -gscale / (float)n_f;
  for (int64_t i = threadIdx.x; i < n_r; i += 256) {
    const float v = real[i];
    s_r += (double)v;
    const float m = 1.f - v;
    h_r += m > 0.f ? (double)m : 0.0;
    if (dreal) dreal[i] = m > 0.f ? gr : 0.f;
  }
  for (int64_t i = threadIdx.x; i < n_f; i += 256) {
    const float v = fake[i];
    s_f += (double)v;
    const float m = 1.f + v;
    h_f += m > 0.f ? (double)m : 0.0;
    if (dfake) dfake[i] = hinge ? (m > 0.f ? gf : 0.f) : gf;
  }
  s_r = disc_block_sum(s_r, sh);
  s_f = disc_block_sum(s_f, sh);
  h_r = disc_block_sum(h_r, sh);
  h_f = disc_block_sum(h_f, sh);
  if (threadIdx.x == 0) {
    const double mr = n_r > 0 ? s_r / (double)n_r : 0.0, mf = s_f / (double)n_f;
    out[0] = hinge ? (float)(0.5 * (h_r / (double)n_r + h_f / (double)n_f)) : (float)(-mf);
    out[1] = (float)mr;
    out[2] = (float)mf;
    out[3] = 0.f;
  }
}

// sum of n floats (the last layer's bias gradient: its dy is dense, not a matrix of 16-byte rows); one workgroup, fp64, fixed order
__global__ __launch_bounds__(256) void disc_sum_kernel(const float* __restrict__ v, int64_t n, float* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  s = disc_block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = (float)s;
}

static bool gn_shape_ok(int C) { return C >= 16 && C <= 1024 && (C & 15) == 0 && 256 % (C >> 2) == 0; }
static bool c4w_ok(int N, int64_t ld, int stride) { return (stride == 1 || stride == 2) && N >= 1 && ld >= 4 && ld <= 1024 && (ld & 3) == 0; }
// slices of the pixel range: a function of the shape only (the summation order never depends on the launch)
static int64_t c4w_splits(int N, int64_t ld, int64_t rows) {
  if (N == 1) return cdiv64(rows, W1_ROWS);
  int64_t s = 512 / (cdiv64(N, 128) * cdiv64(16 * ld, 128)), maxs = cdiv64(rows, 256);
  if (s > maxs) s = maxs;
  return s < 1 ? 1 : s;
}

}  // namespace

// ===================================================================================================== C-ABI
extern "C" int vs_disc_input(const float* imgs, int B, int H, int W, const float* m0, float* rows, void* stream) {
  VS_REQUIRE(imgs && rows && B > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && (((uintptr_t)rows) & 15) == 0);
  const int64_t total = (int64_t)B * H * W;
  hipLaunchKernelGGL(disc_input_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, imgs, H * W, total, m0, rows);
  return vs_launch_status();
}

extern "C" int vs_disc_input_bwd(const float* drows, int B, int H, int W, const float* m0, float* dimgs, void* stream) {
  VS_REQUIRE(drows && dimgs && B > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && (((uintptr_t)drows) & 15) == 0);
  const int64_t total = (int64_t)B * H * W;
  hipLaunchKernelGGL(disc_input_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, drows, H * W, total, m0, dimgs);
  return vs_launch_status();
}

extern "C" int64_t vs_groupnorm_partial_doubles(int B, int HW, int C) {
  if (B <= 0 || HW <= 0 || C <= 0) return 0;
  const int64_t nch = cdiv64(HW, GN_ROWS);
  return (int64_t)B * nch * 2 * C + (int64_t)B * 2 * C + (int64_t)B * 8 + (int64_t)B * nch * 8;
}

extern "C" int vs_groupnorm_lrelu(const float* x, int64_t ld, int B, int HW, int C, int groups, const float* gamma, const float* beta, float eps,
                                  float slope, double* partial, double* mean, double* rstd, float* out, int64_t out_ld, void* stream) {
  VS_REQUIRE(x && out && B > 0 && HW > 0 && C > 0 && ld >= C && out_ld >= C && (ld & 3) == 0 && (out_ld & 3) == 0 && (groups == 0 || groups == 4));
  VS_REQUIRE((((uintptr_t)x) & 15) == 0 && (((uintptr_t)out) & 15) == 0 && (int64_t)B * HW < ((int64_t)1 << 31));
  VS_REQUIRE(4 * ((C + 3) >> 2) <= ld);
  hipStream_t st = (hipStream_t)stream;
  if (groups) {
    VS_REQUIRE(gamma && beta && partial && mean && rstd && gn_shape_ok(C) && (((uintptr_t)gamma) & 15) == 0 && (((uintptr_t)beta) & 15) == 0);
    const int nch = (int)cdiv64(HW, GN_ROWS);
    hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)(B * nch)), dim3(256), 0, st, x, ld, HW, nch, C >> 2, partial);
    hipLaunchKernelGGL(gn_finish_kernel, dim3(blocks_for(4 * B)), dim3(256), 0, st, partial, B, nch, (double)HW * (C >> 2), eps, mean, rstd);
  }
  const int O4 = (int)(out_ld >> 2);
  const int64_t total = (int64_t)B * HW * O4;
  hipLaunchKernelGGL(gn_apply_kernel, dim3(blocks_for(total)), dim3(256), 0, st, x, ld, HW, C, O4, total, gamma, beta, groups ? mean : (const double*)nullptr,
                     rstd, slope, out, out_ld);
  return vs_launch_status();
}

extern "C" int vs_groupnorm_lrelu_bwd(const float* dy, int64_t dy_ld, const float* x, int64_t ld, int B, int HW, int C, int groups, const float* gamma,
                                      const float* beta, const double* mean, const double* rstd, float slope, double* partial, float* dx,
                                      int64_t dx_ld, float* dgamma, float* dbeta, void* stream) {
  VS_REQUIRE(dy && x && dx && B > 0 && HW > 0 && C > 0 && ld >= C && dy_ld >= C && dx_ld >= C && (ld & 3) == 0 && (dy_ld & 3) == 0 && (dx_ld & 3) == 0);
  VS_REQUIRE((groups == 0 || groups == 4) && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)dy) & 15) == 0 && (((uintptr_t)dx) & 15) == 0);
  VS_REQUIRE((int64_t)B * HW < ((int64_t)1 << 31) && 4 * ((C + 3) >> 2) <= ld && 4 * ((C + 3) >> 2) <= dy_ld);
  hipStream_t st = (hipStream_t)stream;
  const double* gsum = nullptr;
  if (groups) {
    VS_REQUIRE(gamma && beta && mean && rstd && partial && dgamma && dbeta && gn_shape_ok(C) && (((uintptr_t)gamma) & 15) == 0 &&
               (((uintptr_t)beta) & 15) == 0);
    const int nch = (int)cdiv64(HW, GN_ROWS);
    double* fcols = partial + (int64_t)B * nch * 2 * C;
    double* gs = fcols + (int64_t)B * 2 * C;
    hipLaunchKernelGGL(gn_bwd_cols_kernel, dim3((unsigned)(B * nch)), dim3(256), 0, st, x, ld, dy, dy_ld, HW, nch, C >> 2, gamma, beta, mean, rstd, slope,
                       partial);
    hipLaunchKernelGGL(gn_bwd_frame_kernel, dim3((unsigned)B), dim3(256), 0, st, partial, nch, C, gamma, fcols, gs);
    hipLaunchKernelGGL(gn_bwd_param_kernel, dim3(blocks_for(C)), dim3(256), 0, st, fcols, B, C, dgamma, dbeta);
    gsum = gs;
  }
  const int O4 = (int)(dx_ld >> 2);
  const int64_t total = (int64_t)B * HW * O4;
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(blocks_for(total)), dim3(256), 0, st, x, ld, dy, dy_ld, HW, C, O4, total, gamma, beta,
                     groups ? mean : (const double*)nullptr, rstd, gsum, 1.0 / ((double)HW * (C >> 2)), slope, dx, dx_ld);
  return vs_launch_status();
}

extern "C" int vs_conv4x4_wgrad_supported(int N, int64_t ld, int stride) { return c4w_ok(N, ld, stride) ? 1 : 0; }

extern "C" int64_t vs_conv4x4_wgrad_partial_floats(int N, int64_t ld, int B, int H, int W, int stride) {
  if (B <= 0 || H < 2 || W < 2 || !c4w_ok(N, ld, stride)) return 0;
  const int64_t rows = (int64_t)B * ((H - 2) / stride + 1) * ((W - 2) / stride + 1);
  return c4w_splits(N, ld, rows) * N * 16 * ld;
}

extern "C" int vs_conv4x4_wgrad(const float* dy, int64_t dy_ld, int N, const float* x, int64_t ld, int B, int H, int W, int stride, float* partial,
                                float* dw, void* stream) {
  VS_REQUIRE(dy && x && partial && dw && c4w_ok(N, ld, stride) && B > 0 && H >= 2 && W >= 2 && dy_ld >= N);
  VS_REQUIRE((((uintptr_t)x) & 15) == 0 && (((uintptr_t)partial) & 15) == 0 && (N == 1 || ((dy_ld & 3) == 0 && (((uintptr_t)dy) & 15) == 0)));
  const int Ho = (H - 2) / stride + 1, Wo = (W - 2) / stride + 1;          // (H + 2 - 4) / stride + 1
  const int64_t rows = (int64_t)B * Ho * Wo;
  VS_REQUIRE(rows < ((int64_t)1 << 31));
  const int K16 = (int)(16 * ld);
  const c4w_t cv{H, W, Ho, Wo, stride};
  const int64_t splits = c4w_splits(N, ld, rows);
  int64_t used;
  hipStream_t st = (hipStream_t)stream;
  if (N == 1) {
    used = splits;
    hipLaunchKernelGGL(conv4x4_wgrad_n1_kernel, dim3((unsigned)used, (unsigned)cdiv64(K16 / 4, 256)), dim3(256), 0, st, dy, dy_ld, x, ld, K16, rows, partial,
                       cv);
  } else {
    int64_t rps = cdiv64(rows, splits);
    rps = cdiv64(rps, 16) * 16;
    used = cdiv64(rows, rps);                  // <= splits
    hipLaunchKernelGGL(conv4x4_wgrad_mfma_kernel, dim3((unsigned)cdiv64(K16, 128), (unsigned)cdiv64(N, 128), (unsigned)used), dim3(256), 0, st, dy, dy_ld, N,
                       x, ld, K16, rows, rps, partial, cv);
  }
  hipLaunchKernelGGL(disc_reduce_chunks_kernel, dim3((unsigned)cdiv64((int64_t)N * K16, 64)), dim3(256), 0, st, partial, (int)used, (int64_t)N * K16, dw);
  return vs_launch_status();
}

extern "C" int vs_conv4x4_n1(const float* x, int64_t ld, int B, int H, int W, const float* w, const float* bias, float* out, void* stream) {
  VS_REQUIRE(x && w && out && B > 0 && H >= 2 && W >= 2 && ld >= 4 && (ld & 3) == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)w) & 15) == 0);
  const int Ho = H - 1, Wo = W - 1;
  const int64_t rows = (int64_t)B * Ho * Wo;
  VS_REQUIRE(rows < ((int64_t)1 << 31));
  hipLaunchKernelGGL(conv4x4_n1_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ld, H, W, Ho, Wo, rows, w, bias, out);
  return vs_launch_status();
}

extern "C" int vs_conv4x4_n1_bwd(const float* dy, int B, int H, int W, int64_t ld, const float* w, float* dx, void* stream) {
  VS_REQUIRE(dy && w && dx && B > 0 && H >= 2 && W >= 2 && ld >= 4 && (ld & 3) == 0 && (((uintptr_t)dx) & 15) == 0 && (((uintptr_t)w) & 15) == 0);
  const int64_t total = (int64_t)B * H * W * (ld >> 2);
  hipLaunchKernelGGL(conv4x4_n1_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, dy, H, W, H - 1, W - 1, ld, total, w, dx);
  return vs_launch_status();
}

extern "C" int vs_conv4x4_n1_bias_grad(const float* dy, int64_t n, float* db, void* stream) {
  VS_REQUIRE(dy && db && n > 0);
  hipLaunchKernelGGL(disc_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dy, n, db);
  return vs_launch_status();
}

extern "C" int vs_disc_loss(const float* real, int64_t n_real, const float* fake, int64_t n_fake, int hinge, float gscale, float* dreal, float* dfake,
                            float* out, void* stream) {
  VS_REQUIRE(fake && out && n_fake > 0 && n_real >= 0 && (hinge == 0 || hinge == 1) && (!hinge || (real && n_real > 0)) && (n_real == 0 || real));
  hipLaunchKernelGGL(disc_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, real, n_real, fake, n_fake, hinge, gscale, dreal, dfake, out);
  return vs_launch_status();
}
