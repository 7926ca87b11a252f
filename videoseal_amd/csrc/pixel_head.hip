// Pixel-wise extractor head (modules/pixel_decoder.py:43-83 with upscale_stages of 2 / 4 and `pixelwise: True`): the Upsample group at
// factor 2 or 4 without the up-sampled tensor and its adjoint, the per-pixel linear layer (NHWC in, NCHW logits out) and its backward,
// the detection / masked decoding losses on [B][1+nbits][H][W] logits (videosealloss.py:138-167) and the pixel vote of the bit metrics
// (evals/metrics.py:150-206).  Everything is deterministic: no atomics, cross-block sums are fixed-order partials finished in double.
#include "vs_common.h"

namespace {

static inline unsigned blocks_for(int64_t n) { return (unsigned)cdiv64(n, 256); }

// bilinear source of destination index d on an axis of n source elements, nn.Upsample(scale_factor=f, align_corners=False):
// src = max((d + 0.5) / f - 0.5, 0), upper neighbour clamped
__device__ __forceinline__ void up_src(int d, float inv_f, int n, int& i0, int& i1, float& w0, float& w1) {
  const float s = fmaxf((d + 0.5f) * inv_f - 0.5f, 0.f);
  i0 = (int)s;
  if (i0 > n - 1) i0 = n - 1;                 // (never taken for d < f * n; keeps every address inside the map whatever the caller passes)
  i1 = i0 + (i0 < n - 1);
  w1 = s - (float)i0;
  w0 = 1.f - w1;
}
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }      // ReflectionPad2d(1), n >= 2

// ---------------------------------------------------------------------------------------------------
// Upsample group at integer factor f (common.py:45-52: bilinear xf -> ReflectionPad2d(1) -> Conv3x3 (no bias) -> LayerNorm over C -> act).
// As in vs_upconv_gather_ln (net_ops.hip) the interpolation, the padding and the tap shift commute with the channel mixing:
//     conv3x3(pad(up_f(v)))[Y,X,c] = sum_t up_f(z_t)[refl(Y+ky-1), refl(X+kx-1), c],     z_t[y,x,c] = sum_ci W[c,ci,t] v[y,x,ci]
// z ([rows][9*Co], columns ordered (tap, channel)) comes from one vs_conv_gemm launch on the LOW-resolution rows; this kernel does the
// 9-tap x 4-neighbour gather, and, unless `raw`, the LayerNorm (biased variance) and the activation.
// Thread = (output pixel, group of CG channels); the TPP lanes of a pixel are adjacent (TPP a power of two <= 64, so a pixel never
// straddles a wave) and reduce with xor shuffles.  Channel vectors at or beyond Co (widths such as 20 = 2 lanes x 12) are masked.
template <int CG>
__global__ __launch_bounds__(256) void pixel_upgather_kernel(const float* __restrict__ z, int64_t zld, int H, int W, int Co, int f, float inv_f,
                                                             int tpp_log2, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                             float eps, int act, int raw, float* __restrict__ out, int64_t old, int64_t npix,
                                                             int nblk) {
  // workgroup b runs on XCD b % 8: give every XCD one contiguous range of output rows so that the low-resolution z rows shared by
  // neighbouring output rows stay in that XCD's L2 (as vs_upconv_gather_ln)
  const int per = (nblk + 7) >> 3;
  const int64_t vb = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int64_t gid = vb * 256 + threadIdx.x;
  const int64_t pq = gid >> tpp_log2;
  const int g = (int)(gid & ((1 << tpp_log2) - 1));
  const bool live = pq < npix && vb < nblk;
  const int64_t p = live ? pq : 0;           // dead lanes still take part in the shuffles
  constexpr int NV = CG / 4;
  bool on[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) on[j] = g * CG + 4 * j < Co;
  const int Wf = f * W, Hf = f * H;
  const int X = (int)(p % Wf);
  const int64_t t0 = p / Wf;
  const int Y = (int)(t0 % Hf);
  const int64_t b = t0 / Hf;
  int ys[3][2], xs[3][2];
  float wy[3][2], wx[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    up_src(reflect1(Y + k - 1, Hf), inv_f, H, ys[k][0], ys[k][1], wy[k][0], wy[k][1]);
    up_src(reflect1(X + k - 1, Wf), inv_f, W, xs[k][0], xs[k][1], wx[k][0], wx[k][1]);
  }
  f32x4 acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* zb = z + b * H * W * zld + g * CG;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float* zr = zb + (int64_t)ys[ky][a] * W * zld + ky * 3 * Co;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float w = wy[ky][a] * wx[kx][c];
          const float* q = zr + (int64_t)xs[kx][c] * zld + kx * Co;
#pragma unroll
          for (int j = 0; j < NV; ++j)
            if (on[j]) acc[j] += w * *reinterpret_cast<const f32x4*>(q + 4 * j);
        }
    }
  if (raw) {
    if (!live) return;
    float* orow = out + p * old + g * CG;
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (on[j]) *reinterpret_cast<f32x4*>(orow + 4 * j) = acc[j];
    return;
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);      // masked vectors are zero
  for (int o = 1; o < (1 << tpp_log2); o <<= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)Co;
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (on[j]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float dl = acc[j][e] - mean; v += dl * dl; }
    }
  for (int o = 1; o < (1 << tpp_log2); o <<= 1) v += __shfl_xor(v, o, 64);
  const float den = sqrtf(v / (float)Co + eps);
  if (!live) return;
  float* orow = out + p * old + g * CG;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (on[j]) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(lnw + g * CG + 4 * j), bv = *reinterpret_cast<const f32x4*>(lnb + g * CG + 4 * j);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = vs_apply_act(wv[e] * ((acc[j][e] - mean) / den) + bv[e], act);
      *reinterpret_cast<f32x4*>(orow + 4 * j) = o;
    }
}

// Adjoint of the raw gather, in gather form: dz[b][y][x][t*Co + c] = sum over the high-resolution pixels (Y, X) that read z_t[y][x],
//     dz_t[y][x] = sum_Y sum_X  cy(refl(Y+ky-1); y) cx(refl(X+kx-1); x) dg[Y][X],     c(r; i) = the bilinear weight with which row r reads i
// (both neighbours when they coincide at a clamped edge).  A destination row r reads source i only for r in [f i - f/2, f i + 3f/2 - 1]
// (and from 0 for i = 0), the tap shift moves that by one and the reflection maps -1 -> 1 and fH -> fH - 2, which stay inside: the 2f + 2
// rows Y = f y - f/2 - 1 ... f y + 3f/2 hold every contribution, and c() is exactly 0 for a row of that window that does not read y.
// Thread = (low-resolution pixel, 4 channels): each dg vector of the window is loaded once and feeds the nine tap accumulators.
template <int F>
__global__ __launch_bounds__(256) void pixel_upgather_bwd_kernel(const float* __restrict__ dg, int64_t gld, int H, int W, int Co, float* __restrict__ dz,
                                                                 int64_t zld, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  constexpr int NW = 2 * F + 2;
  constexpr float inv_f = 1.0f / F;
  const int C4 = Co >> 2;
  const int c4 = (int)(i % C4);
  int64_t r = i / C4;
  const int x = (int)(r % W);
  r /= W;
  const int y = (int)(r % H);
  const int64_t b = r / H;
  const int Hf = F * H, Wf = F * W;
  const int X0 = F * x - F / 2 - 1, Y0 = F * y - F / 2 - 1;
  float cx[NW][3];
  int xo[NW];
#pragma unroll
  for (int ix = 0; ix < NW; ++ix) {
    const int X = X0 + ix;
    const bool in = X >= 0 && X < Wf;
    xo[ix] = in ? X : (X < 0 ? 0 : Wf - 1);                 // an address inside the map; its coefficients are zero
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int i0, i1;
      float w0, w1;
      up_src(reflect1(xo[ix] + k - 1, Wf), inv_f, W, i0, i1, w0, w1);
      cx[ix][k] = in ? (i0 == x ? w0 : 0.f) + (i1 == x ? w1 : 0.f) : 0.f;
    }
  }
  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* gb = dg + b * Hf * Wf * gld + 4 * c4;
  for (int iy = 0; iy < NW; ++iy) {
    const int Y = Y0 + iy;
    if (Y < 0 || Y >= Hf) continue;
    float cy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int i0, i1;
      float w0, w1;
      up_src(reflect1(Y + k - 1, Hf), inv_f, H, i0, i1, w0, w1);
      cy[k] = (i0 == y ? w0 : 0.f) + (i1 == y ? w1 : 0.f);
    }
    const float* gr = gb + (int64_t)Y * Wf * gld;
#pragma unroll
    for (int ix = 0; ix < NW; ++ix) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(gr + (int64_t)xo[ix] * gld);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx] += (cy[ky] * cx[ix][kx]) * v;
    }
  }
  float* zr = dz + ((b * H + y) * W + x) * zld + 4 * c4;
#pragma unroll
  for (int t = 0; t < 9; ++t) *reinterpret_cast<f32x4*>(zr + (int64_t)t * Co) = acc[t];
}

// ---------------------------------------------------------------------------------------------------
// Per-pixel linear layer (pixel_decoder.py:53,78-83: Conv2d 1x1 C -> 1+nbits, optional sigmoid): x NHWC [B*HW][ld] -> out NCHW [B][K][HW].
// C is 24-32 on the cards and K 17-257: the launch is bound by its stores.  A lane owns PX consecutive pixels of one frame with their
// C inputs in registers, the weights are wave-uniform (scalar loads), and every channel plane is written in 16-byte pieces (PX = 4;
// PX = 1 where HW is no multiple of 4: 4-byte stores, still consecutive over the lanes).  K needs no padding.
template <int NVT, int PX>
__global__ __launch_bounds__(256) void pixel_linear_kernel(const float* __restrict__ x, int64_t ld, int64_t HW, int C, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int K, int sigmoid, float* __restrict__ out,
                                                           int64_t groups) {
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gi >= groups) return;
  const int64_t gpf = HW / PX;               // groups per frame
  const int64_t b = gi / gpf, p0 = (gi % gpf) * PX;
  f32x4 xv[PX][NVT];
#pragma unroll
  for (int q = 0; q < PX; ++q) {
    const float* xr = x + (b * HW + p0 + q) * ld;
#pragma unroll
    for (int j = 0; j < NVT; ++j) xv[q][j] = 4 * j < C ? *reinterpret_cast<const f32x4*>(xr + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float* ob = out + b * K * HW + p0;
  for (int k = 0; k < K; ++k) {
    const float* wr = w + (int64_t)k * C;
    const float bk = bias ? bias[k] : 0.f;
    float a[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) a[q] = bk;
#pragma unroll
    for (int j = 0; j < NVT; ++j)
      if (4 * j < C) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int q = 0; q < PX; ++q) a[q] = __builtin_fmaf(wv[e], xv[q][j][e], a[q]);
      }
    if (sigmoid) {
#pragma unroll
      for (int q = 0; q < PX; ++q) a[q] = 1.0f / (1.0f + __expf(-a[q]));
    }
    float* o = ob + (int64_t)k * HW;
    if constexpr (PX == 4) *reinterpret_cast<f32x4*>(o) = f32x4{a[0], a[1], a[2], a[3]};
    else o[0] = a[0];
  }
}

// d of the logits that the linear map sees: dpreds, times y (1 - y) behind a sigmoid output
__device__ __forceinline__ float lin_dlogit(const float* __restrict__ dp, const float* __restrict__ y, int64_t idx) {
  const float d = dp[idx];
  if (!y) return d;
  const float s = y[idx];
  return d * s * (1.f - s);
}

// dx NHWC [B*HW][dx_ld] = sum_k d[b][k][p] W[k][:]: thread = pixel (lanes on consecutive pixels: every plane read is one contiguous piece)
template <int NVT>
__global__ __launch_bounds__(256) void pixel_linear_bwd_x_kernel(const float* __restrict__ dp, const float* __restrict__ y, int64_t HW, int K, int C,
                                                                 const float* __restrict__ w, float* __restrict__ dx, int64_t dld, int64_t rows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int64_t b = r / HW, p = r % HW;
  f32x4 acc[NVT];
#pragma unroll
  for (int j = 0; j < NVT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t base = b * K * HW + p;
  for (int k = 0; k < K; ++k) {
    const float d = lin_dlogit(dp, y, base + (int64_t)k * HW);
    const float* wr = w + (int64_t)k * C;
#pragma unroll
    for (int j = 0; j < NVT; ++j)
      if (4 * j < C) acc[j] += d * *reinterpret_cast<const f32x4*>(wr + 4 * j);
  }
  float* o = dx + r * dld;
#pragma unroll
  for (int j = 0; j < NVT; ++j)
    if (4 * j < C) *reinterpret_cast<f32x4*>(o + 4 * j) = acc[j];
}

// dW [K][C] and db [K] as one [K][C/4 + 1] grid of 4-wide outputs (the extra column multiplies a constant {1, 0, 0, 0} "input": db).
// A workgroup takes a fixed range of rows in tiles of LIN_TR: d [K][LIN_TR] and x [LIN_TR][C + 4] staged in LDS, thread t owns outputs
// t, t + 256, ... (at most MAXO) and sums its rows in ascending order; the per-workgroup sums go to part[blk][K][C + 4] and a second
// kernel adds the workgroups in ascending order in double.
constexpr int LIN_TR = 32;
template <int MAXO>
__global__ __launch_bounds__(256) void pixel_linear_wgrad_kernel(const float* __restrict__ dp, const float* __restrict__ y, const float* __restrict__ x,
                                                                 int64_t ld, int64_t HW, int K, int C, int64_t rows, int64_t rows_per_blk,
                                                                 float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lin_sh[];
  const int CP = C + 4, C4 = CP >> 2;
  float* sd = lin_sh;                       // [K][LIN_TR]
  float* sx = lin_sh + (size_t)K * LIN_TR;  // [LIN_TR][CP]
  const int nout = K * C4;
  f32x4 acc[MAXO];
#pragma unroll
  for (int o = 0; o < MAXO; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t r_lo = (int64_t)blockIdx.x * rows_per_blk;
  int64_t r_hi = r_lo + rows_per_blk;
  if (r_hi > rows) r_hi = rows;
  for (int64_t r0 = r_lo; r0 < r_hi; r0 += LIN_TR) {
    const int n = (int)((r_hi - r0) < LIN_TR ? (r_hi - r0) : LIN_TR);
    __syncthreads();
    for (int idx = threadIdx.x; idx < K * LIN_TR; idx += 256) {
      const int k = idx / LIN_TR, i = idx % LIN_TR;
      float d = 0.f;
      if (i < n) {
        const int64_t r = r0 + i, b = r / HW, p = r % HW;
        d = lin_dlogit(dp, y, (b * K + k) * HW + p);
      }
      sd[idx] = d;
    }
    for (int idx = threadIdx.x; idx < LIN_TR * C4; idx += 256) {
      const int i = idx / C4, j = idx % C4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < n) v = j < C4 - 1 ? *reinterpret_cast<const f32x4*>(x + (r0 + i) * ld + 4 * j) : f32x4{1.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(sx + (size_t)i * CP + 4 * j) = v;
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
      const int oi = threadIdx.x + 256 * o;
      if (oi < nout) {
        const int k = oi / C4, j = oi % C4;
        const float* dk = sd + (size_t)k * LIN_TR;
        const float* xj = sx + 4 * j;
        f32x4 a = acc[o];
#pragma unroll 8
        for (int i = 0; i < LIN_TR; ++i) a += dk[i] * *reinterpret_cast<const f32x4*>(xj + (size_t)i * CP);
        acc[o] = a;
      }
    }
  }
  float* pb = part + (int64_t)blockIdx.x * nout * 4;
#pragma unroll
  for (int o = 0; o < MAXO; ++o) {
    const int oi = threadIdx.x + 256 * o;
    if (oi < nout) *reinterpret_cast<f32x4*>(pb + (int64_t)oi * 4) = acc[o];
  }
}

__global__ __launch_bounds__(256) void pixel_linear_wgrad_finish_kernel(const float* __restrict__ part, int nblk, int K, int C, float* __restrict__ dw,
                                                                        float* __restrict__ db) {
  const int CP = C + 4;
  const int i = blockIdx.x * 256 + threadIdx.x;      // (k, c) with c < C, or c == C: the bias
  if (i >= K * (C + 1)) return;
  const int k = i / (C + 1), c = i % (C + 1);
  double s = 0;
  for (int bk = 0; bk < nblk; ++bk) s += (double)part[((int64_t)bk * K + k) * CP + c];
  if (c < C) dw[(int64_t)k * C + c] = (float)s;
  else if (db) db[k] = (float)s;
}

// ---------------------------------------------------------------------------------------------------
// block-wide sums in a fixed order (wave butterfly, then the four waves in order)
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double block_sum64(double v, double* sh4) {
  v = wave_sum64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
__device__ __forceinline__ int block_sum_int(int v, int* sh4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

// Losses on pixel-wise logits (videosealloss.py:138-167).  preds [B][K][HW], masks [B][HW] float, msgs int32 [msg_rows][K - 1].
//   detect = mean over (b, p) of bce(preds[b][0][p], masks[b][p])
//   decode = mean over the selected pixels (masks != 0, `masks.bool()`) and the K - 1 bits of bce(preds[b][1 + j][p] / T, msgs[b][j])
// bce(z, t) = max(z, 0) - z t + log1p(exp(-|z|)).  dpreds = w_det d detect + w_dec d decode, written for every element (zeros where no
// term reaches).  With no pixel selected decode is 0 / 0 = NaN, as the reference's mean over nothing, and its gradient is zero.
// Grid (chunks of 256 * PX pixels, B); part (doubles): [0, nblk) selected pixels per workgroup, then nblk x {detect sum, decode sum}.
template <int PX>
__global__ __launch_bounds__(256) void pixel_mask_count_kernel(const float* __restrict__ masks, int64_t HW, double* __restrict__ part) {
  __shared__ int sh[4];
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PX;
  int n = 0;
  if (p0 < HW) {
    const float* m = masks + (int64_t)blockIdx.y * HW + p0;
#pragma unroll
    for (int q = 0; q < PX; ++q) n += m[q] != 0.f;
  }
  n = block_sum_int(n, sh);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (double)n;
}

template <int PX>
__global__ __launch_bounds__(256) void pixel_bce_kernel(const float* __restrict__ preds, const float* __restrict__ masks, const int* __restrict__ msgs,
                                                        int msg_rows, int B, int K, int64_t HW, float inv_t, float w_det, float w_dec,
                                                        float* __restrict__ dpreds, double* __restrict__ part) {
  __shared__ double sh[4];
  const int nblk = gridDim.x * gridDim.y;
  double cnt = 0;                                            // whole numbers: exact in any order
  for (int i = threadIdx.x; i < nblk; i += 256) cnt += part[i];
  const double nsel = block_sum64(cnt, sh);
  const int nb = K - 1;
  const float g_det = w_det / (float)((double)B * (double)HW);
  const float g_dec = nsel > 0 ? (float)((double)w_dec * (double)inv_t / (nsel * (double)nb)) : 0.f;
  const int b = blockIdx.y;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PX;
  const bool live = p0 < HW;
  double s_det = 0, s_dec = 0;
  if (live) {
    float m[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) m[q] = masks[(int64_t)b * HW + p0 + q];
    const float* pb = preds + (int64_t)b * K * HW + p0;
    float* db = dpreds + (int64_t)b * K * HW + p0;
    {
      float z[PX], d[PX];
#pragma unroll
      for (int q = 0; q < PX; ++q) z[q] = pb[q];
#pragma unroll
      for (int q = 0; q < PX; ++q) {
        s_det += (double)(fmaxf(z[q], 0.f) - z[q] * m[q] + log1pf(__expf(-fabsf(z[q]))));
        d[q] = g_det * (1.0f / (1.0f + __expf(-z[q])) - m[q]);
      }
      if constexpr (PX == 4) *reinterpret_cast<f32x4*>(db) = f32x4{d[0], d[1], d[2], d[3]};
      else db[0] = d[0];
    }
    const int* mr = msgs + (int64_t)(msg_rows == 1 ? 0 : b) * nb;
    for (int j = 0; j < nb; ++j) {
      const float t = (float)mr[j];
      const float* pj = pb + (int64_t)(1 + j) * HW;
      float z[PX], d[PX];
      if constexpr (PX == 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(pj); z[0] = v[0]; z[1] = v[1]; z[2] = v[2]; z[3] = v[3]; }
      else z[0] = pj[0];
      float sj = 0.f;
#pragma unroll
      for (int q = 0; q < PX; ++q) {
        const float zz = z[q] * inv_t;
        const bool sel = m[q] != 0.f;
        sj += sel ? fmaxf(zz, 0.f) - zz * t + log1pf(__expf(-fabsf(zz))) : 0.f;
        d[q] = sel ? g_dec * (1.0f / (1.0f + __expf(-zz)) - t) : 0.f;
      }
      s_dec += (double)sj;
      float* dj = db + (int64_t)(1 + j) * HW;
      if constexpr (PX == 4) *reinterpret_cast<f32x4*>(dj) = f32x4{d[0], d[1], d[2], d[3]};
      else dj[0] = d[0];
    }
  }
  const double t_det = block_sum64(s_det, sh);
  const double t_dec = block_sum64(s_dec, sh);
  if (threadIdx.x == 0) {
    const int64_t bi = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[nblk + 2 * bi] = t_det;
    part[nblk + 2 * bi + 1] = t_dec;
  }
}

__global__ __launch_bounds__(256) void pixel_bce_finish_kernel(const double* __restrict__ part, int nblk, int B, int K, int64_t HW,
                                                               float* __restrict__ loss) {
  __shared__ double sh[4];
  double c = 0, a = 0, d = 0;
  for (int i = threadIdx.x; i < nblk; i += 256) {          // a fixed partition of the workgroups over the threads, ascending within a thread
    c += part[i];
    a += part[nblk + 2 * i];
    d += part[nblk + 2 * i + 1];
  }
  c = block_sum64(c, sh);
  a = block_sum64(a, sh);
  d = block_sum64(d, sh);
  if (threadIdx.x == 0) {
    loss[0] = (float)(a / ((double)B * (double)HW));
    loss[1] = (float)(d / (c * (double)(K - 1)));          // 0 / 0 = NaN with nothing selected
  }
}

// Pixel vote of bit_accuracy / bit_accuracy_1msg (evals/metrics.py:150-206): votes[b][k] = selected pixels of frame b with
// preds[b][k][p] > threshold, nsel[b] = selected pixels (all of them without a mask).  One workgroup per (b, k): one read of the logits.
__global__ __launch_bounds__(256) void pixel_vote_kernel(const float* __restrict__ preds, int64_t bstride, const float* __restrict__ masks, int K,
                                                         int64_t HW, float threshold, int* __restrict__ votes, int* __restrict__ nsel) {
  __shared__ int sh[4];
  const int k = blockIdx.x, b = blockIdx.y;
  const float* pr = preds + (int64_t)b * bstride + (int64_t)k * HW;
  const float* m = masks ? masks + (int64_t)b * HW : nullptr;
  int v = 0, n = 0;
  for (int64_t p = threadIdx.x; p < HW; p += 256) {
    const bool sel = m ? m[p] != 0.f : true;
    n += sel;
    v += sel && pr[p] > threshold;
  }
  v = block_sum_int(v, sh);
  if (threadIdx.x == 0) votes[(int64_t)b * K + k] = v;
  if (k == 0) {
    n = block_sum_int(n, sh);
    if (threadIdx.x == 0) nsel[b] = n;
  }
}

// channel group CG (floats per lane) and lanes per pixel (a power of two) for a stage width: the least padding, then the wider group
static bool upgather_split(int Co, int* cg_out, int* tpp_log2_out) {
  if (Co <= 0 || Co % 4 || Co > 256) return false;
  int best = -1, best_cg = 0, best_l2 = 0;
  for (int cg = 16; cg >= 4; cg -= 4) {
    const int need = (Co + cg - 1) / cg;
    int l2 = 0;
    while ((1 << l2) < need) ++l2;
    if (l2 > 6) continue;
    const int waste = cg * (1 << l2) - Co;
    if (best < 0 || waste < best) { best = waste; best_cg = cg; best_l2 = l2; }
  }
  if (best < 0) return false;
  *cg_out = best_cg;
  *tpp_log2_out = best_l2;
  return true;
}

static inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static inline int64_t bce_chunks(int64_t HW) { return cdiv64(HW, 256 * (HW % 4 == 0 ? 4 : 1)); }
static inline int64_t lin_wgrad_blocks(int64_t rows) {
  const int64_t nb = cdiv64(rows, 8 * LIN_TR);             // at least eight tiles per workgroup, at most 512 workgroups
  return nb > 512 ? 512 : nb;
}

}  // namespace

// ===================================================================================================== C-ABI
extern "C" int vs_pixel_upgather_supported(int Co, int f) {
  int cg, l2;
  return (f == 2 || f == 4) && upgather_split(Co, &cg, &l2) ? 1 : 0;
}

extern "C" int vs_pixel_upgather(const float* z, int64_t z_ld, int B, int H, int W, int Co, int f, const float* lnw, const float* lnb, float eps,
                                 int act, float* out, int64_t out_ld, void* stream) {
  VS_REQUIRE(z && out && B > 0 && H > 0 && W > 0 && Co > 0 && (!lnw == !lnb) && al16(z) && al16(out) && (!lnw || (al16(lnw) && al16(lnb))));
  int cg, l2;
  if (!(f == 2 || f == 4) || !upgather_split(Co, &cg, &l2)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(z_ld >= 9 * (int64_t)Co && z_ld % 4 == 0 && out_ld >= Co && out_ld % 4 == 0);
  const int64_t npix = (int64_t)B * f * H * f * W;
  VS_REQUIRE(npix <= (int64_t)1 << 40);
  const int64_t nblk = cdiv64(npix << l2, 256);
  VS_REQUIRE(nblk < ((int64_t)1 << 31) - 8);
  const dim3 grid((unsigned)(cdiv64(nblk, 8) * 8));
  const int raw = lnw ? 0 : 1;
  hipStream_t st = (hipStream_t)stream;
#define VS_PIX_UP(CG_)                                                                                                                        \
  hipLaunchKernelGGL(pixel_upgather_kernel<CG_>, grid, dim3(256), 0, st, z, z_ld, H, W, Co, f, 1.0f / (float)f, l2, lnw, lnb, eps, act, raw, out, \
                     out_ld, npix, (int)nblk)
  switch (cg) {
    case 4: VS_PIX_UP(4); break;
    case 8: VS_PIX_UP(8); break;
    case 12: VS_PIX_UP(12); break;
    default: VS_PIX_UP(16); break;
  }
#undef VS_PIX_UP
  return vs_launch_status();
}

extern "C" int vs_pixel_upgather_bwd(const float* dg, int64_t dg_ld, int B, int H, int W, int Co, int f, float* dz, int64_t dz_ld, void* stream) {
  VS_REQUIRE(dg && dz && B > 0 && H > 0 && W > 0 && Co > 0 && al16(dg) && al16(dz));
  if (!(f == 2 || f == 4) || Co % 4 || Co > 256) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(dz_ld >= 9 * (int64_t)Co && dz_ld % 4 == 0 && dg_ld >= Co && dg_ld % 4 == 0);
  const int64_t total = (int64_t)B * H * W * (Co / 4);
  VS_REQUIRE(cdiv64(total, 256) < ((int64_t)1 << 31));
  hipStream_t st = (hipStream_t)stream;
  if (f == 2)
    hipLaunchKernelGGL(pixel_upgather_bwd_kernel<2>, dim3(blocks_for(total)), dim3(256), 0, st, dg, dg_ld, H, W, Co, dz, dz_ld, total);
  else
    hipLaunchKernelGGL(pixel_upgather_bwd_kernel<4>, dim3(blocks_for(total)), dim3(256), 0, st, dg, dg_ld, H, W, Co, dz, dz_ld, total);
  return vs_launch_status();
}

extern "C" int vs_pixel_linear(const float* x, int64_t ld, int B, int64_t HW, int C, const float* w, const float* bias, int K, int sigmoid,
                               float* out, void* stream) {
  VS_REQUIRE(x && w && out && B > 0 && HW > 0 && C > 0 && K > 0 && ld >= C && ld % 4 == 0 && al16(x) && al16(w) && al16(out));
  if (C % 4 || C > 64) return VS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int px = HW % 4 == 0 && C <= 32 ? 4 : 1;       // (wider inputs: one pixel per lane, the four-pixel form would not fit the register file)
  const int64_t groups = (int64_t)B * HW / px;
  VS_REQUIRE(cdiv64(groups, 256) < ((int64_t)1 << 31));
  const dim3 grid(blocks_for(groups));
#define VS_PIX_LIN(NVT_, PX_) \
  hipLaunchKernelGGL((pixel_linear_kernel<NVT_, PX_>), grid, dim3(256), 0, st, x, ld, HW, C, w, bias, K, sigmoid, out, groups)
  if (px == 4) {
    if (C <= 16) VS_PIX_LIN(4, 4);
    else if (C <= 24) VS_PIX_LIN(6, 4);
    else VS_PIX_LIN(8, 4);
  } else {
    if (C <= 16) VS_PIX_LIN(4, 1);
    else if (C <= 32) VS_PIX_LIN(8, 1);
    else VS_PIX_LIN(16, 1);
  }
#undef VS_PIX_LIN
  return vs_launch_status();
}

extern "C" int64_t vs_pixel_linear_bwd_partial_floats(int64_t rows, int K, int C) {
  if (rows <= 0 || K <= 0 || C <= 0 || C % 4) return 0;
  return lin_wgrad_blocks(rows) * K * (int64_t)(C + 4);
}

extern "C" int vs_pixel_linear_bwd(const float* dpreds, const float* y, const float* x, int64_t ld, int B, int64_t HW, int C, const float* w, int K,
                                   float* dx, int64_t dx_ld, float* dw, float* db, float* partial, void* stream) {
  VS_REQUIRE(dpreds && w && B > 0 && HW > 0 && C > 0 && K > 0 && al16(w) && (!dx || (al16(dx) && dx_ld >= C && dx_ld % 4 == 0)) &&
             (!dw || (x && partial && al16(x) && al16(partial) && ld >= C && ld % 4 == 0)) && (dx || dw));
  if (C % 4 || C > 64) return VS_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)B * HW;
  const int nout = K * (C / 4 + 1);
  const size_t lds = ((size_t)K * LIN_TR + (size_t)LIN_TR * (C + 4)) * sizeof(float);
  if (dw && (nout > 256 * 20 || lds > 64 * 1024)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(cdiv64(rows, 256) < ((int64_t)1 << 31));
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    const dim3 grid(blocks_for(rows));
    if (C <= 16) hipLaunchKernelGGL(pixel_linear_bwd_x_kernel<4>, grid, dim3(256), 0, st, dpreds, y, HW, K, C, w, dx, dx_ld, rows);
    else if (C <= 32) hipLaunchKernelGGL(pixel_linear_bwd_x_kernel<8>, grid, dim3(256), 0, st, dpreds, y, HW, K, C, w, dx, dx_ld, rows);
    else hipLaunchKernelGGL(pixel_linear_bwd_x_kernel<16>, grid, dim3(256), 0, st, dpreds, y, HW, K, C, w, dx, dx_ld, rows);
  }
  if (dw) {
    const int64_t nb = lin_wgrad_blocks(rows);
    const int64_t rpb = cdiv64(cdiv64(rows, nb), LIN_TR) * LIN_TR;
    const dim3 grid((unsigned)nb);
#define VS_PIX_WG(MAXO_) \
  hipLaunchKernelGGL(pixel_linear_wgrad_kernel<MAXO_>, grid, dim3(256), lds, st, dpreds, y, x, ld, HW, K, C, rows, rpb, partial)
    if (nout <= 256 * 2) VS_PIX_WG(2);
    else if (nout <= 256 * 4) VS_PIX_WG(4);
    else if (nout <= 256 * 8) VS_PIX_WG(8);
    else VS_PIX_WG(20);
#undef VS_PIX_WG
    hipLaunchKernelGGL(pixel_linear_wgrad_finish_kernel, dim3(blocks_for((int64_t)K * (C + 1))), dim3(256), 0, st, partial, (int)nb, K, C, dw, db);
  }
  return vs_launch_status();
}

extern "C" int64_t vs_pixel_bce_partial_doubles(int B, int K, int64_t HW) {
  if (B <= 0 || K < 2 || HW <= 0) return 0;
  return 3 * bce_chunks(HW) * B;
}

extern "C" int vs_pixel_bce(const float* preds, const float* masks, const int32_t* msgs, int msg_rows, int B, int K, int64_t HW, float temperature,
                            float w_det, float w_dec, float* dpreds, double* partial, float* loss, void* stream) {
  VS_REQUIRE(preds && masks && msgs && dpreds && partial && loss && B > 0 && K >= 2 && HW > 0 && temperature > 0.f &&
             (msg_rows == 1 || msg_rows == B) && al16(preds) && al16(dpreds));
  const int64_t chunks = bce_chunks(HW);
  VS_REQUIRE(B <= 65535 && chunks * B < ((int64_t)1 << 30));
  const dim3 grid((unsigned)chunks, (unsigned)B);
  const int nblk = (int)(chunks * B);
  hipStream_t st = (hipStream_t)stream;
  if (HW % 4 == 0) {
    hipLaunchKernelGGL(pixel_mask_count_kernel<4>, grid, dim3(256), 0, st, masks, HW, partial);
    hipLaunchKernelGGL(pixel_bce_kernel<4>, grid, dim3(256), 0, st, preds, masks, msgs, msg_rows, B, K, HW, 1.0f / temperature, w_det, w_dec, dpreds,
                       partial);
  } else {
    hipLaunchKernelGGL(pixel_mask_count_kernel<1>, grid, dim3(256), 0, st, masks, HW, partial);
    hipLaunchKernelGGL(pixel_bce_kernel<1>, grid, dim3(256), 0, st, preds, masks, msgs, msg_rows, B, K, HW, 1.0f / temperature, w_det, w_dec, dpreds,
                       partial);
  }
  hipLaunchKernelGGL(pixel_bce_finish_kernel, dim3(1), dim3(256), 0, st, partial, nblk, B, K, HW, loss);
  return vs_launch_status();
}

extern "C" int vs_pixel_vote(const float* preds, int64_t batch_stride, const float* masks, int B, int K, int64_t HW, float threshold, int32_t* votes,
                             int32_t* nsel, void* stream) {
  VS_REQUIRE(preds && votes && nsel && B > 0 && K > 0 && HW > 0 && HW < ((int64_t)1 << 31) && batch_stride >= (int64_t)K * HW && B <= 65535);
  hipLaunchKernelGGL(pixel_vote_kernel, dim3((unsigned)K, (unsigned)B), dim3(256), 0, (hipStream_t)stream, preds, batch_stride, masks, K, HW, threshold,
                     votes, nsel);
  return vs_launch_status();
}
