// Full-resolution "shell" of the VideoSeal path: the kernels that touch every pixel of every frame.
//   vs_resize_pre    : (anti-aliased) bilinear resize NCHW -> NHWC fused with RGB->Y and the x*2-1 preprocess
//   vs_jnd_heatmap   : JND heat-map at the processing resolution (low-res attenuation)
//   vs_embed_tail    : delta up-resize x JND(img) -> blend -> clamp, one pass over the frame
// These are the HBM-bound kernels (7.08 MB read + 7.08 MB written per 768x768 frame in the tail).
#include "shell_common.h"
#include "images_plan.h"
#include "clips_plan.h"
#include "videoseal_regions.h"
#include "videoseal_lists_psnr.h"
#include <cmath>
#include <type_traits>

namespace {

using namespace vs_taps;

// ---- modes of the tail bodies.  BLEND is vs_embed_tail.  SCALED (vs_embed_tail_scaled) takes the watermark's strength of frame f from
// frame_scale[f] in device memory instead of scaling_w.  ENERGY (vs_embed_tail_energy) computes the same d and stores no frame: every thread
// adds d * d of its pixels in float64 (the product of two fp32 values is exact there) and the workgroup writes ONE partial sum into
// partials[f][blockIdx.y][blockIdx.x]; no atomics, the order of every addition is fixed, so two runs give the same bits.
// The new members ride behind TailArgs in a derived struct, so the kernel arguments of the BLEND instantiations are what they were.
// REGIONS (vs_embed_tail_regions) reads a label per pixel: label r in 1..R takes the watermark of plane set key * R + r - 1, label 0 keeps the
// pixel of imgs bit for bit.  The tile body runs once per label present in the tile (a workgroup-uniform walk, embed_tail_regions_kernel), each
// time with that label's source window in the one LDS window, and stores the pixels of its label only: LDS does not grow with R.
// (The walk is over workgroups, not a loop in one: see embed_tail_regions_kernel.)
constexpr int TAIL_BLEND = 0, TAIL_SCALED = 1, TAIL_ENERGY = 2, TAIL_REGIONS = 3;
struct TailArgsX : TailArgs { const float* frame_scale; double* partials; };
struct TailArgsR : TailArgs { const unsigned char* labels; int R; };
template <int MODE> using tail_args_t = std::conditional_t<MODE == TAIL_BLEND, TailArgs, TailArgsX>;      // (REGIONS: TailArgsR, named by its kernel)

// first plane set of key frame `key`: [total_key][Cd] planes, or [total_key * R][Cd] with the region's set behind its key frame
template <int MODE, class Args>
__device__ __forceinline__ int64_t tail_plane_set(const Args& a, const int key, const int region) {
  if constexpr (MODE == TAIL_REGIONS) return (int64_t)key * a.R + (region - 1);
  else return (int64_t)key;
}

template <int MODE, class Args>
__device__ __forceinline__ float tail_strength(const Args& a, const int f) {
  if constexpr (MODE == TAIL_SCALED) return a.frame_scale[f];
  else return a.scaling_w;
}

// the workgroup's partial of a clip kernel (grid = tile columns x tile rows x frames): lanes, then the four waves, in a fixed order
// (FLAT: the list kernels, whose grid is a flat run of (item, tile) workgroups -- the slot is the workgroup's place in that run)
template <bool FLAT = false>
__device__ __forceinline__ void tail_energy_store(const double e, double* __restrict__ partials, const int f) {
  __shared__ double red[4];
  double v = e;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[FLAT ? (int64_t)blockIdx.x : ((int64_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- frame element access: fp32 NCHW planes, or uint8 RGB24 (HWC, what inference_streaming.py:26 reads from the ffmpeg
// pipe).  uint8 -> float is exactly `torch.tensor(clip, dtype=float32) / 255.0`; float -> uint8 is `(x * 255.0).byte()`
// (truncation) of inference_streaming.py:31.
// float(u) / 255.0f, correctly rounded, for u in 0..255: one Newton correction of u * (1/255) (checked exhaustively against IEEE
// division in tests/test_gpu_kernels.py::test_u8_unit_conversion_is_exact); 3 VALU ops instead of the 13 of a true division
__device__ __forceinline__ float u8_unit(float u) {
  const float r = 1.0f / 255.0f;
  const float q = u * r;
  const float rem = __builtin_fmaf(-q, 255.0f, u);
  return __builtin_fmaf(rem, r, q);
}
template <typename T> struct Px;
template <> struct Px<float> {
  static __device__ __forceinline__ float ld(const float* img, int64_t plane, int c, int64_t pix) { return img[c * plane + pix]; }
  static __device__ __forceinline__ void st(float* img, int64_t plane, int c, int64_t pix, float v) { img[c * plane + pix] = v; }
};
template <> struct Px<unsigned char> {
  static __device__ __forceinline__ float ld(const unsigned char* img, int64_t, int c, int64_t pix) { return u8_unit((float)img[pix * 3 + c]); }
  static __device__ __forceinline__ void st(unsigned char* img, int64_t, int c, int64_t pix, float v) { img[pix * 3 + c] = (unsigned char)(v * 255.0f); }
};


// One 32 x 8 tile of resize_pre: output columns from ox0, rows from oy0 of the frame at `base`, stored as frame b of the destinations.
// (ox0, oy0, b, base) are workgroup-uniform: blockIdx for a clip (resize_pre_kernel), a table look-up for a list of images (the *_images kernels below).
template <typename T>
__device__ __forceinline__ void resize_pre_tile(float* __restrict__ Lw, const T* __restrict__ base, const int b, const int ox0, const int oy0,
                                                int C, int H, int W, int oh, int ow, int antialias, float* __restrict__ dst_rgb, float mul,
                                                float add, float* __restrict__ dst_key, int key_step, int key_mode, float y0, float y1,
                                                float y2) {
  // The block's 32 x 8 outputs read an input window of about (32*scale + support) x (8*scale + support) pixels.  Reading it
  // tap by tap from global memory is L1-bound (4-byte loads 12 bytes apart, every line touched ~7 times), so the window is
  // staged once through LDS with coalesced loads whenever it fits; the arithmetic (and its order) is the same either way.
  const int64_t plane = (int64_t)H * W;
  int x_lo, y_lo, x_hi, y_hi, n_;
  tap_range(ox0, W, ow, antialias, x_lo, n_);
  tap_range(min(ox0 + 31, ow - 1), W, ow, antialias, x_hi, n_);
  const int ww = x_hi + n_ - x_lo;
  tap_range(oy0, H, oh, antialias, y_lo, n_);
  tap_range(min(oy0 + 7, oh - 1), H, oh, antialias, y_hi, n_);
  const int wh = y_hi + n_ - y_lo;
  const bool staged = C == 3 && ww <= RS_WW && wh <= RS_WH;          // block-uniform
  if (staged) {
    // division-free thread -> element maps, every thread's loads issued back to back (the staging is latency-bound otherwise)
    if (sizeof(T) == 1) {            // RGB24: the 3*ww bytes of a window row are contiguous, (x, c) interleaved
      // aligned 4-byte loads (thread = (dword column, row parity)), unpacked into the three LDS planes
      const int jd = threadIdx.x & 127, y0r = threadIdx.x >> 7;
      const unsigned char* fb = reinterpret_cast<const unsigned char*>(base);
      unsigned wrd[RS_WH / 2];
      int mis[RS_WH / 2];
#pragma unroll
      for (int k = 0; k < RS_WH / 2; ++k) {
        wrd[k] = 0u; mis[k] = 0;
        if (y0r + 2 * k < wh) {
          const unsigned char* rowp = fb + ((int64_t)(y_lo + y0r + 2 * k) * W + x_lo) * 3;
          const int m = (int)(reinterpret_cast<uintptr_t>(rowp) & 3);
          mis[k] = m;
          if (4 * jd < 3 * ww + m) wrd[k] = *reinterpret_cast<const unsigned*>(rowp - m + 4 * jd);
        }
      }
#pragma unroll
      for (int k = 0; k < RS_WH / 2; ++k)
        if (y0r + 2 * k < wh) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int bo = 4 * jd + q - mis[k];
            if (bo >= 0 && bo < 3 * ww) {
              const int xx = bo / 3, c = bo - xx * 3;
              Lw[(c * RS_WH + y0r + 2 * k) * RS_WW + xx] = u8_unit((float)((wrd[k] >> (8 * q)) & 0xffu));
            }
          }
        }
    } else {                         // planar: thread = (column, row parity); 3 channels x wh/2 rows each
      const int xx = threadIdx.x & 127, y0r = threadIdx.x >> 7;
      if (xx < ww) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float v[RS_WH / 2];
#pragma unroll
          for (int k = 0; k < RS_WH / 2; ++k)
            if (y0r + 2 * k < wh) v[k] = Px<T>::ld(base, plane, c, (int64_t)(y_lo + y0r + 2 * k) * W + x_lo + xx);
#pragma unroll
          for (int k = 0; k < RS_WH / 2; ++k)
            if (y0r + 2 * k < wh) Lw[(c * RS_WH + y0r + 2 * k) * RS_WW + xx] = v[k];
        }
      }
    }
    __syncthreads();
  }
  const int ox = ox0 + (threadIdx.x & 31);
  const int oy = oy0 + (threadIdx.x >> 5);
  if (ox >= ow || oy >= oh) return;
  const Taps ty = make_taps(oy, H, oh, antialias), tx = make_taps(ox, W, ow, antialias);
  float acc[3] = {0.f, 0.f, 0.f};
  if (staged && tx.n <= MAXT) {
    float wxs[MAXT];
#pragma unroll
    for (int jx = 0; jx < MAXT; ++jx) wxs[jx] = jx < tx.n ? tap_w(tx, jx) : 0.f;
    const float* Lp = Lw + (ty.lo - y_lo) * RS_WW + (tx.lo - x_lo);
    for (int jy = 0; jy < ty.n; ++jy) {
      const float wy = tap_w(ty, jy);
      float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int jx = 0; jx < MAXT; ++jx)
        if (jx < tx.n) {
#pragma unroll
          for (int c = 0; c < 3; ++c) r[c] = __builtin_fmaf(wxs[jx], Lp[(c * RS_WH + jy) * RS_WW + jx], r[c]);     // (explicit fma chains: see tail_taps)
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, r[c], acc[c]);
    }
  } else if (tx.n > LONG_TAPS || ty.n > LONG_TAPS) {        // long filters: compensated sums (resize_taps.h)
    CompSum a3[3];
    for (int jy = 0; jy < ty.n; ++jy) {
      const float wy = tap_w(ty, jy);
      const int64_t row = (int64_t)(ty.lo + jy) * W + tx.lo;
      CompSum r3[3];
      for (int jx = 0; jx < tx.n; ++jx) {
        const float wx = tap_w(tx, jx);
        for (int c = 0; c < 3; ++c)
          if (c < C) r3[c].add(wx, Px<T>::ld(base, plane, c, row + jx));
      }
      for (int c = 0; c < 3; ++c) a3[c].add(wy, r3[c].value());
    }
    for (int c = 0; c < 3; ++c) acc[c] = a3[c].value();
  } else {
    for (int jy = 0; jy < ty.n; ++jy) {
      const float wy = tap_w(ty, jy);
      const int64_t row = (int64_t)(ty.lo + jy) * W + tx.lo;
      float r[3] = {0.f, 0.f, 0.f};
      for (int jx = 0; jx < tx.n; ++jx) {
        const float wx = tap_w(tx, jx);
        for (int c = 0; c < 3; ++c)
          if (c < C) r[c] = __builtin_fmaf(wx, Px<T>::ld(base, plane, c, row + jx), r[c]);
      }
      for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, r[c], acc[c]);
    }
  }
  const int64_t opix = ((int64_t)oy * ow + ox);
  if (dst_rgb) {
    f32x4 v = {acc[0] * mul + add, C > 1 ? acc[1] * mul + add : 0.f, C > 2 ? acc[2] * mul + add : 0.f, 0.f};
    *reinterpret_cast<f32x4*>(dst_rgb + ((int64_t)b * oh * ow + opix) * 4) = v;
  }
  if (dst_key && (b % key_step) == 0) {
    f32x4 v;
    if (key_mode == 0) {
      const float y = y0 * acc[0] + y1 * acc[1] + y2 * acc[2];
      v = f32x4{y * 2.f - 1.f, 0.f, 0.f, 0.f};
    } else {
      v = f32x4{acc[0] * 2.f - 1.f, acc[1] * 2.f - 1.f, acc[2] * 2.f - 1.f, 0.f};
    }
    *reinterpret_cast<f32x4*>(dst_key + ((int64_t)(b / key_step) * oh * ow + opix) * 4) = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void resize_pre_kernel(const T* __restrict__ src, int B, int C, int H, int W, int oh, int ow,
                                                         int antialias, float* __restrict__ dst_rgb, float mul, float add,
                                                         float* __restrict__ dst_key, int key_step, int key_mode, float y0,
                                                         float y1, float y2) {
  __shared__ float Lw[3 * RS_WH * RS_WW];
  const int b = blockIdx.z;
  resize_pre_tile<T>(Lw, src + (int64_t)b * C * H * W, b, blockIdx.x * 32, blockIdx.y * 8, C, H, W, oh, ow, antialias, dst_rgb, mul, add,
                     dst_key, key_step, key_mode, y0, y1, y2);
}

// ---- row-streaming separable form of resize_pre (round 4) -------------------------------------------------------------------------------
// The tile kernel above stages a (32 scale + support) x (8 scale + support) window per 32 x 8 outputs: at 768 -> 256 that is 102 x 30 pixels for
// 96 x 24 useful ones, and a 408-byte row piece at an arbitrary offset touches 4-5 cache lines -- 1.51 x the frame through HBM (calibrated
// counters, profiles/r03r_hbm_counter_calibration.md) and the horizontal filter of an input row is recomputed by every output row that uses it.
// Here a workgroup owns 128 output columns x a strip of output rows and walks the INPUT rows of the strip top to bottom, eight at a time:
//   1. the eight rows x three planes x (128 scale + support) columns go to LDS with coalesced loads (the next eight are requested first);
//   2. horizontal pass: every (input row, output column) pair is filtered ONCE into a 16-row ring of horizontally resized rows;
//   3. vertical pass: every output row whose tap window is complete is combined from the ring and stored (NHWC rgb / Y key frames).
// The expressions and their order are those of the tile kernel (r += wx * pixel over the taps, then acc += wy * r): bit-identical outputs.
// An input row is fetched once per 128-column tile (+ the strip's first window): ~1.15 x the frame.
template <int OW>
__global__ __launch_bounds__(256) void resize_pre_stream_kernel(const float* __restrict__ src, int B, int H, int W, int oh, int ow, int antialias,
                                                                ResizePreEpi epi, int strip) {
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  vs_rs::resize_stream_body<OW>(rs_smem, src, H, W, 0, 0, H, W, oh, ow, antialias, strip, epi);
}


// luminance of 255*img (jnd.py:86-89), zero outside the image (conv zero padding)
__device__ __forceinline__ void load_lum_tile(float* L, const float* img, int64_t sc, int64_t sy, int64_t sx, int H, int W,
                                              int x0, int y0) {
  for (int i = threadIdx.x; i < LW * LH; i += 256) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gx = x0 + lx - HALO, gy = y0 + ly - HALO;
    float v = 0.f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const float* p = img + (int64_t)gy * sy + (int64_t)gx * sx;
      v = lum255(p[0], p[sc], p[2 * sc]);
    }
    L[i] = v;
  }
}

template <typename T, int ROWS>
__device__ __forceinline__ void load_lum_tile_px(float* L, const T* img, int64_t plane, int H, int W, int x0, int y0) {
  for (int i = threadIdx.x; i < LW * (ROWS + 2 * HALO); i += 256) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gx = x0 + lx - HALO, gy = y0 + ly - HALO;
    float v = 0.f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const int64_t pix = (int64_t)gy * W + gx;
      v = lum255(Px<T>::ld(img, plane, 0, pix), Px<T>::ld(img, plane, 1, pix), Px<T>::ld(img, plane, 2, pix));
    }
    L[i] = v;
  }
}

__global__ __launch_bounds__(256) void jnd_heatmap_kernel(const float* __restrict__ img, int H, int W, int64_t sb, int64_t sc,
                                                          int64_t sy, int64_t sx, JndTaps k, float* __restrict__ hmap) {
  __shared__ float L[LW * LH];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, b = blockIdx.z;
  load_lum_tile(L, img + (int64_t)b * sb, sc, sy, sx, H, W, x0, y0);
  __syncthreads();
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x = x0 + lx, y = y0 + ly;
  if (x < W && y < H) hmap[((int64_t)b * H + y) * W + x] = jnd_at(L, LW, lx + HALO, ly + HALO, k);
}




// Workgroup = 256 consecutive columns x TTH rows of one frame: every wave touches 256 contiguous bytes (fp32) per row and
// plane -- 32-pixel-wide tiles (128-byte pieces at a 3 KB stride) ran at ~1.3 TB/s, a quarter of what a plain copy reaches.
// Each thread owns one column: its horizontal taps are computed once and reused for the TTH rows; the vertical taps
// of the TTH rows are computed by TTH threads into LDS; the source window of delta (x low-res heat-map, x key-frame
// weights) is staged in LDS so the 4..9 taps per pixel are LDS reads.
// TH = rows per tile; KEEP: the tile's own pixels are parked in LDS by the luminance phase and the blend phase reads them from there -- the frame is
// fetched from HBM ONCE.  (Calibrated counters, profiles/r03r_hbm_counter_calibration.md: with the second read from global memory the kernel fetches
// 543 MiB per launch for a 216 MiB batch -- the re-read does not hit in L2 -- and runs at the 4 TB/s the HBM delivers for that traffic; KEEP with
// 8-row tiles (24 KiB of pixels + 12 luminance rows: still three workgroups per CU) fetches 1.5 x the frame instead of 2.27 x.)
// (the tile's body: columns from x0, rows from y0 of the frame `img` -> `outf` / `predf`; f names the frame's key frame and its rows of
// hmap_lowres.  All of them workgroup-uniform: blockIdx for a clip (embed_tail_kernel), a table look-up for a list of images, each with its
// own a.H x a.W (the *_images kernels below).)
// REGIONS: `region` is the label this pass blends, bit ly of `sel` says that row ly of this thread's column carries it; nothing else is stored.
template <typename T, bool SEP, int TH, bool KEEP, int MODE = TAIL_BLEND, class Args = tail_args_t<MODE>, bool FLAT = false>
__device__ __forceinline__ void embed_tail_tile(const Args& a, const JndTaps& k, const int x0, const int y0, const int f,
                                                const T* __restrict__ img, T* __restrict__ outf, float* __restrict__ predf,
                                                const int region = 0, const unsigned sel = 0) {
  constexpr int TTH = TH;
  constexpr int DWH = TH == 8 ? 8 : DW_H;              // rows of the watermark's source window (8-row tiles at >= 2x up-scale need <= 8)
  __shared__ float Pk[KEEP ? 3 * TH * TTW : 4];
  __shared__ float L[TLW * (TTH + 2 * HALO)];
  __shared__ float Dw[3 * DW_W * DWH];
  __shared__ int ty_lo[TTH], ty_n[TTH];
  __shared__ float ty_w[TTH][4];
  __shared__ int s_xhi, s_nmax, s_xlo;
  const int64_t plane = (int64_t)a.H * a.W;
  const bool full_jnd = a.attenuate && !a.hmap_lowres;
  if (threadIdx.x == 0) { s_xhi = 0; s_nmax = 0; }
  __syncthreads();
  if (full_jnd) {       // luminance of the tile + 2-pixel halo: thread = column (4 extra halo columns on threads 0-3), all rows
    constexpr int NR = TTH + 2 * HALO;
    auto lum_column = [&](const int lxx) __attribute__((always_inline)) {      // lxx: column inside the LDS tile
      const int gx = x0 + lxx - HALO;
      float v[NR][3];
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) {
        const int gy = y0 + rr - HALO;
        const bool ok = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
        const int cx = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx), cy = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy);
        const int64_t pix = (int64_t)cy * a.W + cx;          // always a valid address: unconditional loads, zeroed afterwards
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float t = Px<T>::ld(img, plane, c, pix);
          v[rr][c] = ok ? t : 0.f;
        }
      }
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) {
        L[rr * TLW + lxx] = lum255(v[rr][0], v[rr][1], v[rr][2]);
        if (KEEP && rr >= HALO && rr < HALO + TTH && lxx >= HALO && lxx < HALO + TTW)
#pragma unroll
          for (int c = 0; c < 3; ++c) Pk[(c * TTH + rr - HALO) * TTW + lxx - HALO] = v[rr][c];
      }
    };
    lum_column(threadIdx.x + HALO);
    if (threadIdx.x < 2 * HALO) lum_column(threadIdx.x < HALO ? threadIdx.x : TTW + threadIdx.x);
  }
  // taps: own column (registers), rows of the tile (LDS)
  const int lx = threadIdx.x;
  const int x = x0 + lx;
  const Taps tx = make_taps(x < a.W ? x : a.W - 1, a.Sw, a.W, a.antialias);
  float wxs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wxs[j] = j < tx.n ? tap_w(tx, j) : 0.f;
  if (x < a.W) { atomicMax(&s_xhi, tx.lo + tx.n); atomicMax(&s_nmax, tx.n); }
  if (threadIdx.x == 0) s_xlo = tx.lo;        // taps start monotonically: column 0 / row 0 of the tile come first
  if (threadIdx.x < TTH) {
    const int yy = y0 + threadIdx.x;
    const Taps tp = make_taps(yy < a.H ? yy : a.H - 1, a.Sh, a.H, a.antialias);
    ty_lo[threadIdx.x] = tp.lo;
    ty_n[threadIdx.x] = tp.n;
#pragma unroll
    for (int j = 0; j < 4; ++j) ty_w[threadIdx.x][j] = j < tp.n ? tap_w(tp, j) : 0.f;
    if (yy < a.H) atomicMax(&s_nmax, tp.n);
  }
  __syncthreads();

  // key-frame expansion (videoseal.py:80-118): value = wa*key[ka] + wb*key[kb]   (second spelling: key_mix of tail_phases.h, which the
  // surface kernels call -- a change to the rule is made in both)
  int ka = 0, kb = 0;
  float wa = 1.f, wb = 0.f;
  if (a.video_mode == VS_VIDEO_REPEAT) {
    ka = f / a.step;
  } else if (a.video_mode == VS_VIDEO_ALTERNATE) {
    ka = f / a.step;
    wa = (f % a.step) == 0 ? 1.f : 0.f;
  } else {
    const int ninter = ((a.F - 1) / a.step) * a.step;
    if (f < ninter) {
      ka = f / a.step; kb = ka + 1;
      const int j = f % a.step;
      const float lin = a.step > 1 ? (float)j / (float)(a.step - 1) : 0.f;
      wa = 1.f - lin; wb = 1.f - wa;
    } else {
      ka = a.total_key - 1;
    }
  }
  if (ka >= a.total_key) ka = a.total_key - 1;
  if (kb >= a.total_key) kb = a.total_key - 1;
  const int splane = a.Sh * a.Sw;
  const float* dka = a.delta + tail_plane_set<MODE>(a, ka, region) * a.Cd * splane;
  const float* dkb = a.delta + tail_plane_set<MODE>(a, kb, region) * a.Cd * splane;
  const float* hml = a.hmap_lowres ? a.hmap_lowres + (int64_t)f * splane : nullptr;

  // source window -> LDS, already combined: Dw[c] = hm * (wa*key_a + wb*key_b)  (the per-tap operand of wam.py:184-190)
  const int lasty = min(TTH, a.H - y0) - 1;
  const int wx0 = s_xlo, wy0 = ty_lo[0];
  const int dww = s_xhi - wx0, dwh = ty_lo[lasty] + ty_n[lasty] - wy0;
  const int blk_n = s_nmax;
  const bool staged = blk_n <= 4 && dww <= DW_W && dwh <= DWH;
  const int wx0b = wx0;
  if (staged) {
    for (int i = threadIdx.x; i < dwh * dww; i += 256) {
      const int yy = i / dww, xx = i - yy * dww;
      const int sp = (wy0 + yy) * a.Sw + wx0b + xx;
      const float hm = hml ? hml[sp] : 1.f;
      for (int c = 0; c < a.Cd; ++c) {
        float v = wa * dka[c * splane + sp];
        if (wb != 0.f) v = __builtin_fmaf(wb, dkb[c * splane + sp], v);
        Dw[c * (DW_W * DWH) + yy * DW_W + xx] = hm * v;
      }
    }
  }
  __syncthreads();      // L, Dw
  if (MODE != TAIL_ENERGY && MODE != TAIL_REGIONS && x >= a.W) return;
  const float sw = tail_strength<MODE>(a, f);
  double e = 0.0;                                     // ENERGY: this thread's sum of d * d
  // (ENERGY: every thread stays for the workgroup's sum.  REGIONS: every thread stays for the barriers of the next label's pass; a column
  // without a pixel of this label has nothing to do)
  const int lasty_t = (MODE == TAIL_ENERGY && x >= a.W) || (MODE == TAIL_REGIONS && sel == 0u) ? -1 : lasty;

  auto tap = [&](const int sp, const float wx, float (&r)[3]) __attribute__((always_inline)) {
    const float hm = hml ? hml[sp] : 1.f;
    for (int c = 0; c < a.Cd; ++c) {
      float v = wa * dka[c * splane + sp];
      if (wb != 0.f) v += wb * dkb[c * splane + sp];
      r[c] += wx * (hm * v);
    }
  };
  // rows in groups of RG: the frame loads of a whole group are issued before any of it is consumed -- with one row (3 loads) in
  // flight per wave and ~16 waves per CU the kernel cannot cover the HBM latency (measured 2 TB/s)
  constexpr int RG = 4;
  for (int lyg = 0; lyg <= lasty_t; lyg += RG) {      // no workgroup barrier below this line
    if (MODE == TAIL_REGIONS && ((sel >> lyg) & ((1u << RG) - 1u)) == 0u) continue;
    float px[RG][3];
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (MODE != TAIL_ENERGY && lyg + q <= lasty) {
        const int64_t pix = (int64_t)(y0 + lyg + q) * a.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[q][c] = (KEEP && full_jnd) ? Pk[(c * TTH + lyg + q) * TTW + lx] : Px<T>::ld(img, plane, c, pix);
      }
    float hmg[RG] = {1.f, 1.f, 1.f, 1.f};
    if (SEP && full_jnd) {                 // separable stencils for the RG rows of the group: RG + 4 luminance rows, 5 LDS reads each
      float la_s[RG], gxs[RG], gys[RG];
#pragma unroll
      for (int q = 0; q < RG; ++q) { la_s[q] = 0.f; gxs[q] = 0.f; gys[q] = 0.f; }
#pragma unroll
      for (int r8 = 0; r8 < RG + 2 * HALO; ++r8) {
        const float* row = L + (lyg + r8) * TLW + lx + HALO;
        const float m2 = row[-2], m1 = row[-1], c0 = row[0], p1 = row[1], p2 = row[2];
        const float h3 = m1 + c0 + p1;
        const float h5 = h3 + m2 + p2;
        const float sd = p1 - m1;
        const float tt = m1 + 2.f * c0 + p1;
#pragma unroll
        for (int q = 0; q < RG; ++q) {
          const int dy = r8 - (q + HALO);       // row offset of this luminance row relative to output row lyg + q
          if (dy >= -2 && dy <= 2) la_s[q] += h5;
          if (dy >= -1 && dy <= 1) la_s[q] += h3;
          if (dy == 0) la_s[q] -= 2.f * c0;
          if (dy == -1 || dy == 1) gxs[q] += sd;
          if (dy == 0) gxs[q] += 2.f * sd;
          if (dy == -1) gys[q] += tt;
          if (dy == 1) gys[q] -= tt;
        }
      }
#pragma unroll
      for (int q = 0; q < RG; ++q) {
        if (fabsf(la_s[q] * (1.f / 32.f) - 127.f) < 0.02f) hmg[q] = jnd_at(L, TLW, lx + HALO, min(lyg + q, TTH - 1) + HALO, k);   // at the jump: the 25-tap order decides
        else hmg[q] = jnd_finish(la_s[q], gxs[q], gys[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const int ly = lyg + q;
      if (ly > lasty) break;
      if (MODE == TAIL_REGIONS && !((sel >> ly) & 1u)) continue;
      const int y = y0 + ly;
      float d[3] = {0.f, 0.f, 0.f};
      const int ylo = ty_lo[ly], yn = ty_n[ly];
      if (staged) {
        const int basep = (ylo - wy0) * DW_W + (tx.lo - wx0b);
        if (blk_n <= 3) tail_taps<3, DWH>(d, Dw, a.Cd, basep, tx.n, yn, wxs, ty_w[ly]);
        else tail_taps<4, DWH>(d, Dw, a.Cd, basep, tx.n, yn, wxs, ty_w[ly]);
      } else {
        const Taps ty = make_taps(y, a.Sh, a.H, a.antialias);
        for (int jy = 0; jy < ty.n; ++jy) {
          const float wy = tap_w(ty, jy);
          float r[3] = {0.f, 0.f, 0.f};
          for (int jx = 0; jx < tx.n; ++jx) tap((ty.lo + jy) * a.Sw + tx.lo + jx, tap_w(tx, jx), r);
          for (int c = 0; c < a.Cd; ++c) d[c] += wy * r[c];
        }
      }
      // attenuate == 2: the training forward's order of operations (wam.py:103-113): blend first, then
      // imgs + hmaps * (imgs_w - imgs) (jnd.py:110-114); preds_w stays the un-attenuated resized delta
      const bool fwd_order = full_jnd && a.attenuate == 2;
      float hm = 1.f;
      if (full_jnd) {
        hm = SEP ? hmg[q] : jnd_at(L, TLW, lx + HALO, ly + HALO, k);
        if (!fwd_order)
          for (int c = 0; c < a.Cd; ++c) d[c] = hm * d[c];
      }
      if (MODE == TAIL_ENERGY) {
        for (int c = 0; c < a.Cd; ++c) e += (double)d[c] * (double)d[c];
        continue;
      }
      const int64_t pix = (int64_t)y * a.W + x;
      if (predf)
        for (int c = 0; c < a.Cd; ++c) predf[c * plane + pix] = d[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = blend_px(a.scaling_i, sw, px[q][c], d[a.Cd == 1 ? 0 : c], hm, fwd_order);
        if (a.clamp) v = v <= 0.f ? 0.f : (v >= 1.f ? 1.f : v);      // (NaN passes: fminf / fmaxf would turn it into 0)
        Px<T>::st(outf, plane, c, pix, v);
      }
    }
  }
  if constexpr (MODE == TAIL_ENERGY) tail_energy_store<FLAT>(e, a.partials, f);      // (the slot is the workgroup's place in the grid)
}

template <typename T, bool SEP, int TH, bool KEEP, int MODE = TAIL_BLEND>
__global__ __launch_bounds__(256) void embed_tail_kernel(tail_args_t<MODE> a, JndTaps k) {
  const int f = blockIdx.z;
  const int64_t plane = (int64_t)a.H * a.W;
  embed_tail_tile<T, SEP, TH, KEEP, MODE>(a, k, blockIdx.x * TTW, blockIdx.y * TH, f, static_cast<const T*>(a.imgs) + (int64_t)f * 3 * plane,
                                    static_cast<T*>(a.out) + (int64_t)f * 3 * plane,
                                    a.preds_w ? a.preds_w + (int64_t)f * a.Cd * plane : nullptr);
}

// Region-wise tail (vs_embed_tail_regions): the 16-row tile of embed_tail_kernel with a label per pixel.  A tile belongs to R workgroups, one per
// label (blockIdx.x = tile column * R + r - 1: the R of a tile are dispatched together and share its lines in L2).  Every thread reads the labels
// of its column (16 bytes), the workgroup ORs the set of labels present, and the workgroup of a label that is absent from the tile ends there
// -- before it forms an address into delta.  The workgroup of a present label runs the tile body with that label's plane set behind a.delta --
// the same body, the same expressions, so a pixel of label r has the bits vs_embed_tail gives it with plane set r as delta -- and stores
// the pixels of its label only.  Background pixels are copied by the workgroup of label 1 (no clamp, no arithmetic), their preds_w is 0.
// (A loop over the present labels around the body in ONE workgroup was built first: hipcc hoists the body's frame loads out of that loop and
// the kernel needs 232 - 256 VGPRs, one wave per SIMD, against 108 - 119 for this form.)
template <typename T>
__device__ __forceinline__ int64_t raw_index(const int64_t plane, const int c, const int64_t pix) {
  return sizeof(T) == 1 ? pix * 3 + c : c * plane + pix;
}

template <typename T, bool SEP>
__global__ __launch_bounds__(256) void embed_tail_regions_kernel(TailArgsR a, JndTaps k) {
  __shared__ unsigned s_present;
  const int col = blockIdx.x / a.R, r = blockIdx.x - col * a.R + 1;
  const int f = blockIdx.z, x0 = col * TTW, y0 = blockIdx.y * TTH;
  const int64_t plane = (int64_t)a.H * a.W;
  const T* img = static_cast<const T*>(a.imgs) + (int64_t)f * 3 * plane;
  T* outf = static_cast<T*>(a.out) + (int64_t)f * 3 * plane;
  float* predf = a.preds_w ? a.preds_w + (int64_t)f * a.Cd * plane : nullptr;
  const unsigned char* lab = a.labels + (int64_t)f * plane;
  const int x = x0 + (int)threadIdx.x;
  if (threadIdx.x == 0) s_present = 0u;
  __syncthreads();
  unsigned sel = 0u, bg = 0u, present = 0u;       // bit ly: row ly of this thread's column carries label r / is background
  if (x < a.W) {
    unsigned l[TTH];
#pragma unroll
    for (int ly = 0; ly < TTH; ++ly) l[ly] = y0 + ly < a.H ? lab[(int64_t)(y0 + ly) * a.W + x] : 0u;      // guarded: the last band is ragged
#pragma unroll
    for (int ly = 0; ly < TTH; ++ly)
      if (y0 + ly < a.H) {
        const unsigned v = l[ly] > (unsigned)a.R ? 0u : l[ly];
        sel |= (v == (unsigned)r ? 1u : 0u) << ly;
        bg |= (v == 0u ? 1u : 0u) << ly;
        present |= 1u << v;
      }
  }
  if (present) atomicOr(&s_present, present);
  __syncthreads();
  const unsigned mask = __builtin_amdgcn_readfirstlane(s_present);      // workgroup-uniform: the body's barriers sit behind a uniform branch
  if (r == 1 && (mask & 1u)) {
#pragma unroll
    for (int ly = 0; ly < TTH; ++ly)
      if ((bg >> ly) & 1u) {
        const int64_t pix = (int64_t)(y0 + ly) * a.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) outf[raw_index<T>(plane, c, pix)] = img[raw_index<T>(plane, c, pix)];
        if (predf)
          for (int c = 0; c < a.Cd; ++c) predf[c * plane + pix] = 0.f;
      }
  }
  if (!((mask >> r) & 1u)) return;
  embed_tail_tile<T, SEP, TTH, false, TAIL_REGIONS, TailArgsR>(a, k, x0, y0, f, img, outf, predf, r, sel);
}

// ---------------------------------------------------------------------------------------------------
// Row-streaming form of the tail (round 4): workgroup = 256 columns x a STRIP of `strip` rows of one frame, walked top to bottom in groups
// of SG = 4 rows.  What the 16-row-tile kernel above pays per tile is paid once per strip: the column taps, the key-frame expansion, the
// pipeline fill; the frame is fetched ONCE (the 16-row form reads every tile for the luminance phase and again for the blend: 2.27 x the
// frame through HBM, profiles/r03r_hbm_counter_calibration.md) and the halo is 4 rows per strip instead of 4 per 16.
//   * every thread owns one column; the pixels of the next group (SG rows x 3 planes) are requested before the current group is consumed;
//   * JND: the luminance of an incoming row goes into a 12-row LDS ring (the only cross-thread traffic: 5 reads per pixel); its horizontal sums
//     (box5, box3, centre, Sobel pair) are added straight into the accumulators of the five output rows it touches -- eight accumulator sets
//     per thread, rotated by four per group -- in the SAME order (top row first) and with the same expressions as the separable 16-row form,
//     so the heat-map is bit-identical to it; an output row is finished two rows behind the incoming one, its pixels wait in registers;
//   * a pixel whose luminance mask lands within 0.02 of the la = 127 jump is re-evaluated in the 25-tap order from the ring (jnd.py:66-68);
//   * the watermark's source window (x low-res heat-map, x key-frame weights) is staged per 16 output rows into a double-buffered LDS window
//     one group ahead of its first use; ONE barrier per group covers ring, window and row taps (three-slot ring / two-slot window: a writer
//     is always at least one barrier behind the last reader of the slot it overwrites).
// Needs an up-scale by >= 2 in both directions (<= 3 taps per direction, window <= 136 x 12); everything else takes the tile kernel.


// (No waves-per-SIMD hint and no wrapper around the body: `__launch_bounds__(256, 3 | 4)` as well as a __forceinline__ body called from two
// __global__ wrappers made hipcc spill 16-40 bytes per lane; a scratch reload waits for every older global load -- the row prefetch -- and the
// JND form ran 40 % slower: 175-180 -> 245-265 us at 32 x 768^2, profiles/r04_tail_forms.md.)
template <bool JND, int CD, int MODE = TAIL_BLEND>
__global__ __launch_bounds__(256) void embed_tail_stream_kernel(tail_args_t<MODE> a, JndTaps k, const int strip) {
  extern __shared__ float dyn_smem[];
  float* Lr = dyn_smem;                                        // [RING][TLW] luminance ring (JND only)
  float* DwB = dyn_smem + (JND ? RING * TLW : 0);              // [2][Cd][DW_H][DW_W] watermark source windows
  __shared__ int ty_lo[2][SUBR], ty_n[2][SUBR], s_wy0[2];
  __shared__ float ty_w[2][SUBR][4];
  __shared__ int s_xhi, s_xlo;
  constexpr int dwsz = CD * DW_W * DW_H;
  const int x0 = blockIdx.x * TTW, y0 = blockIdx.y * strip, f = blockIdx.z;
  const int ys_end = min(a.H, y0 + strip);
  const int64_t plane = (int64_t)a.H * a.W;
  const float* img = static_cast<const float*>(a.imgs) + (int64_t)f * 3 * plane;
  float* outf = static_cast<float*>(a.out) + (int64_t)f * 3 * plane;
  const int lx = threadIdx.x;
  const int x = x0 + lx;
  const bool xin = x < a.W;
  const int cx = xin ? x : a.W - 1;
  if (threadIdx.x == 0) s_xhi = 0;
  __syncthreads();
  const Taps tx = make_taps(cx, a.Sw, a.W, a.antialias);
  float wxs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wxs[j] = j < tx.n ? tap_w(tx, j) : 0.f;
  if (xin) atomicMax(&s_xhi, tx.lo + tx.n);
  if (threadIdx.x == 0) s_xlo = tx.lo;
  // halo columns of the luminance ring: threads 0 .. 3 carry one extra column each (x0 - 2, x0 - 1, x0 + 256, x0 + 257)
  const bool hal = JND && lx < 2 * HALO;
  const int hgx = lx < HALO ? x0 - HALO + lx : x0 + TTW + (lx - HALO);
  const int hl = lx < HALO ? lx : TTW + lx;
  const bool hin = hal && hgx >= 0 && hgx < a.W;
  const int hcx = hgx < 0 ? 0 : (hgx >= a.W ? a.W - 1 : hgx);

  // key-frame expansion (videoseal.py:80-118): value = wa*key[ka] + wb*key[kb]   (same as the tile kernel; second spelling: key_mix of tail_phases.h)
  int ka = 0, kb = 0;
  float wa = 1.f, wb = 0.f;
  if (a.video_mode == VS_VIDEO_REPEAT) {
    ka = f / a.step;
  } else if (a.video_mode == VS_VIDEO_ALTERNATE) {
    ka = f / a.step;
    wa = (f % a.step) == 0 ? 1.f : 0.f;
  } else {
    const int ninter = ((a.F - 1) / a.step) * a.step;
    if (f < ninter) {
      ka = f / a.step; kb = ka + 1;
      const int j = f % a.step;
      const float lin = a.step > 1 ? (float)j / (float)(a.step - 1) : 0.f;
      wa = 1.f - lin; wb = 1.f - wa;
    } else {
      ka = a.total_key - 1;
    }
  }
  if (ka >= a.total_key) ka = a.total_key - 1;
  if (kb >= a.total_key) kb = a.total_key - 1;
  const int splane = a.Sh * a.Sw;
  const float* dka = a.delta + (int64_t)ka * CD * splane;
  const float* dkb = a.delta + (int64_t)kb * CD * splane;
  const float* hml = a.hmap_lowres ? a.hmap_lowres + (int64_t)f * splane : nullptr;
  __syncthreads();                                             // s_xlo / s_xhi
  const int wx0 = s_xlo, dww = s_xhi - s_xlo;

  auto stage = [&](const int sub, const int b) __attribute__((always_inline)) {      // source window + row taps of output rows [16 sub, 16 sub + 16)
    // (embed_tail_yuv_stream_kernel and embed_tail_rgb_stream_kernel carry this lambda, the accumulate / shift of acc_la, acc_gx, acc_gy and
    // the jump test below word for word: a change here is made there as well)
    const int sy0 = y0 + SUBR * sub;
    const int lasty = min(SUBR, ys_end - sy0) - 1;
    int wy0, n0, wyl, nl;
    tap_range(sy0, a.Sh, a.H, a.antialias, wy0, n0);
    tap_range(sy0 + lasty, a.Sh, a.H, a.antialias, wyl, nl);
    const int dwh = wyl + nl - wy0;
    if (threadIdx.x < SUBR) {
      const int yy = sy0 + threadIdx.x;
      const Taps tp = make_taps(yy < a.H ? yy : a.H - 1, a.Sh, a.H, a.antialias);
      ty_lo[b][threadIdx.x] = tp.lo;
      ty_n[b][threadIdx.x] = tp.n;
#pragma unroll
      for (int j = 0; j < 4; ++j) ty_w[b][threadIdx.x][j] = j < tp.n ? tap_w(tp, j) : 0.f;
      if (threadIdx.x == 0) s_wy0[b] = wy0;
    }
    float* Dw = DwB + b * dwsz;
    // the window (<= 136 x 12 elements) in batches of four per thread: every load of a batch is issued before the first value is used -- a loop
    // that loads, combines and stores one element at a time is a chain of dependent L2 round trips, and hipcc guards the registers such a loop
    // re-uses with `s_waitcnt vmcnt(0)`, which also waits for the row prefetch issued just before
    const int nel = dwh * dww;
    for (int i0 = 0; i0 < nel; i0 += 4 * 256) {
      int sp[4], lo[4];
      float hmv[4], da[4][CD], db[4][CD];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(i0 + q * 256 + (int)threadIdx.x, nel - 1);
        const int yy = i / dww, xx = i - yy * dww;
        sp[q] = (wy0 + yy) * a.Sw + wx0 + xx;
        lo[q] = yy * DW_W + xx;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hmv[q] = hml ? hml[sp[q]] : 1.f;
#pragma unroll
        for (int c = 0; c < CD; ++c) {
          da[q][c] = dka[c * splane + sp[q]];
          db[q][c] = wb != 0.f ? dkb[c * splane + sp[q]] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + q * 256 + (int)threadIdx.x < nel) {
#pragma unroll
          for (int c = 0; c < CD; ++c) {
            float v = wa * da[q][c];
            if (wb != 0.f) v = __builtin_fmaf(wb, db[q][c], v);
            Dw[c * (DW_W * DW_H) + lo[q]] = hmv[q] * v;
          }
        }
    }
  };
  const int ymax_need = min(a.H - 1, ys_end + (JND ? HALO - 1 : -1));     // last row any thread of this strip reads
  float pf[SG][3], pfh[SG][3];
  auto load_rows = [&](const int r0) __attribute__((always_inline)) {     // rows r0 .. r0 + SG - 1 of the own (and halo) column -> pf / pfh
#pragma unroll
    for (int q = 0; q < SG; ++q) {
      if constexpr (MODE == TAIL_ENERGY && !JND) {          // d does not depend on the frame: nothing of it is read
#pragma unroll
        for (int c = 0; c < 3; ++c) pf[q][c] = 0.f;
        continue;
      }
      const int gy = r0 + q;
      const int cy = gy < 0 ? 0 : (gy > ymax_need ? ymax_need : gy);       // always a valid address; rows outside are zeroed when used
      const int64_t pix = (int64_t)cy * a.W;
#pragma unroll
      for (int c = 0; c < 3; ++c) pf[q][c] = img[c * plane + pix + cx];
      if (hal) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pfh[q][c] = img[c * plane + pix + hcx];
      }
    }
  };

  const int nrows = ys_end - y0;
  const int niter = (nrows + SG - 1) / SG;
  float acc_la[2 * SG], acc_gx[2 * SG], acc_gy[2 * SG];
#pragma unroll
  for (int i = 0; i < 2 * SG; ++i) { acc_la[i] = 0.f; acc_gx[i] = 0.f; acc_gy[i] = 0.f; }
  float hist[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  const float sw = tail_strength<MODE>(a, f);
  double e = 0.0;                                              // ENERGY: this thread's sum of d * d
  load_rows(y0 - HALO);
  stage(0, 0);
  for (int it = -1; it < niter; ++it) {
    const int r0 = y0 + SG * it + HALO;                       // first incoming row of this group; its output rows are r0 - 2 .. r0 + 1
    const int slot0 = ((it + 1) % 3) * SG;
    float cu[SG][3];
#pragma unroll
    for (int q = 0; q < SG; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) cu[q][c] = pf[q][c];
    if (JND) {
#pragma unroll
      for (int q = 0; q < SG; ++q) {
        const int gy = r0 + q;
        const bool rok = gy >= 0 && gy < a.H;
        Lr[(slot0 + q) * TLW + lx + HALO] = (rok && xin) ? lum255(cu[q][0], cu[q][1], cu[q][2]) : 0.f;
        if (hal) Lr[(slot0 + q) * TLW + hl] = (rok && hin) ? lum255(pfh[q][0], pfh[q][1], pfh[q][2]) : 0.f;
      }
    }
    if (it + 1 < niter) {
      load_rows(r0 + SG);                                      // in flight while this group is consumed
      if (((it + 1) & 3) == 0 && it + 1 > 0) stage((it + 1) >> 2, ((it + 1) >> 2) & 1);
    }
    __syncthreads();
    const int sb = (it >> 2) & 1;
    const float* Dw = DwB + sb * dwsz;
#pragma unroll
    for (int j = 0; j < SG; ++j) {
      if (JND) {
        const float* row = Lr + (slot0 + j) * TLW + lx + HALO;
        const float m2 = row[-2], m1 = row[-1], c0 = row[0], p1 = row[1], p2 = row[2];
        const float h3 = m1 + c0 + p1;
        const float h5 = h3 + m2 + p2;
        const float sd = p1 - m1;
        const float tt = m1 + 2.f * c0 + p1;
#pragma unroll
        for (int i = j; i <= j + 4; ++i) {
          const int dy = 2 + j - i;                            // incoming row - output row
          if (dy >= -2 && dy <= 2) acc_la[i] += h5;
          if (dy >= -1 && dy <= 1) acc_la[i] += h3;
          if (dy == 0) acc_la[i] -= 2.f * c0;
          if (dy == -1 || dy == 1) acc_gx[i] += sd;
          if (dy == 0) acc_gx[i] += 2.f * sd;
          if (dy == -1) acc_gy[i] += tt;
          if (dy == 1) acc_gy[i] -= tt;
        }
      }
      const int y = r0 - HALO + j;                             // the output row this incoming row completes
      if (it >= 0 && y < ys_end && xin) {
        float hm = 1.f;
        if (JND) {
          if (fabsf(acc_la[j] * (1.f / 32.f) - 127.f) < 0.02f) hm = jnd_at_ring(Lr, (slot0 + j + RING - HALO) % RING, lx + HALO, k);
          else hm = jnd_finish(acc_la[j], acc_gx[j], acc_gy[j]);
        }
        const int ly = (SG * it + j) & (SUBR - 1);
        float d[3] = {0.f, 0.f, 0.f};
        const int basep = (ty_lo[sb][ly] - s_wy0[sb]) * DW_W + (tx.lo - wx0);
        tail_taps<3, DW_H>(d, Dw, CD, basep, tx.n, ty_n[sb][ly], wxs, ty_w[sb][ly]);
        const bool fwd_order = JND && a.attenuate == 2;
        if (JND && !fwd_order)
#pragma unroll
          for (int c = 0; c < CD; ++c) d[c] = hm * d[c];
        if (MODE == TAIL_ENERGY) {
#pragma unroll
          for (int c = 0; c < CD; ++c) e += (double)d[c] * (double)d[c];
          continue;
        }
        const int64_t pix = (int64_t)y * a.W + x;
        if (a.preds_w)
#pragma unroll
          for (int c = 0; c < CD; ++c) a.preds_w[((int64_t)f * CD + c) * plane + pix] = d[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float p = j < 2 ? hist[j][c] : cu[j - 2][c];
          float v = blend_px(a.scaling_i, sw, p, d[CD == 1 ? 0 : c], hm, fwd_order);
          if (a.clamp) v = v <= 0.f ? 0.f : (v >= 1.f ? 1.f : v);      // (NaN passes)
          outf[c * plane + pix] = v;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < SG; ++i) {
      acc_la[i] = acc_la[i + SG]; acc_gx[i] = acc_gx[i + SG]; acc_gy[i] = acc_gy[i + SG];
      acc_la[i + SG] = 0.f; acc_gx[i + SG] = 0.f; acc_gy[i + SG] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { hist[0][c] = cu[2][c]; hist[1][c] = cu[3][c]; }
  }
  if constexpr (MODE == TAIL_ENERGY) tail_energy_store(e, a.partials, f);
}

// (no waves-per-SIMD hint on the JND form: with `__launch_bounds__(256, 3)` or `(256, 4)` hipcc schedules the same body 40 % slower -- 132
// VGPRs and three waves per SIMD either way, measured 175 -> 245-260 us at 32 x 768^2, profiles/r04_tail_forms.md)

// ---------------------------------------------------------------------------------------------------
// Lists of images of different sizes (vs_resize_pre_images, vs_embed_tail_images).  The tile bodies above with another way of finding the
// tile: a launch is a flat list of (image, tile) items, one workgroup each, over at most VS_IMAGES_PER_LAUNCH images whose descriptors and
// prefix table of first workgroups travel in the kernel arguments (images_plan.h).  The look-up is a function of blockIdx.x and kernel
// arguments only -- scalar loads and five scalar compare steps -- so the image's pointer, size and frame number stay in SGPRs, as the
// launch scalars of the clip kernels do.
static_assert(VS_IMG_RS_TW == 32 && VS_IMG_RS_TH == 8 && VS_IMG_TAIL_TW == TTW && VS_IMG_TAIL_TH == TTH, "images_plan.h counts the tiles of these kernels");
static_assert(VS_IMAGES_PER_LAUNCH == 32, "images_find: five halving steps");

struct ImgSlot { const void* img; void* out; float* preds_w; int H, W, frame, cols; };      // cols: tiles per tile row of this image
struct ImagesArgs {
  int first_wg[VS_IMAGES_PER_LAUNCH + 1];      // entries past the launch's image count hold the grid size: never reached by a workgroup
  int pad_;
  ImgSlot slot[VS_IMAGES_PER_LAUNCH];
};
static_assert(sizeof(ImagesArgs) + sizeof(TailArgsX) + sizeof(JndTaps) <= 3072, "descriptors + tail arguments (every mode) stay well inside the 4 KiB of kernel arguments");

// the image (or clip slot) of workgroup wg: the last k with first_wg[k] <= wg
template <class Args>
__device__ __forceinline__ int images_find(const Args& g, const int wg) {
  int k = 0;
#pragma unroll
  for (int s = VS_IMAGES_PER_LAUNCH / 2; s >= 1; s >>= 1)
    if (wg >= g.first_wg[k + s]) k += s;
  return k;
}

template <typename T>
__global__ __launch_bounds__(256) void resize_pre_images_kernel(const ImagesArgs g, const int oh, const int ow, const int antialias,
                                                                const ResizePreEpi o) {
  __shared__ float Lw[3 * RS_WH * RS_WW];
  const int k = images_find(g, blockIdx.x);
  const int t = blockIdx.x - g.first_wg[k];
  const int cols = g.slot[k].cols;
  const int by = t / cols, bx = t - by * cols;
  resize_pre_tile<T>(Lw, static_cast<const T*>(g.slot[k].img), g.slot[k].frame, bx * VS_IMG_RS_TW, by * VS_IMG_RS_TH, 3, g.slot[k].H,
                     g.slot[k].W, oh, ow, antialias, o.dst_rgb, o.mul, o.add, o.dst_key, 1, o.key_mode, o.y0c, o.y1c, o.y2c);
}

template <int OW>
__global__ __launch_bounds__(256) void resize_pre_images_stream_kernel(const ImagesArgs g, const int oh, const int ow, const int antialias,
                                                                       const ResizePreEpi epi, const int strip) {
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  const int k = images_find(g, blockIdx.x);
  const int t = blockIdx.x - g.first_wg[k];
  const int cols = g.slot[k].cols;
  const int by = t / cols, bx = t - by * cols;
  const int H = g.slot[k].H, W = g.slot[k].W;
  vs_rs::resize_stream_tile<OW>(rs_smem, static_cast<const float*>(g.slot[k].img), H, W, 0, 0, H, W, oh, ow, antialias, strip, epi, bx, by,
                                g.slot[k].frame);
}

// MODE (vs_embed_tail_images_scaled / _energy, videoseal_lists_psnr.h): SCALED reads the strength of the image at frame_scale[its index in the
// caller's list] -- the body's frame number, a scalar load; ENERGY writes the workgroup's partial at partials[blockIdx.x], the launch's flat
// grid (the launcher moves `partials` to the launch's first slot), and stores no image.
template <typename T, bool SEP, int MODE = TAIL_BLEND>
__global__ __launch_bounds__(256) void embed_tail_images_kernel(const ImagesArgs g, tail_args_t<MODE> a, const JndTaps k) {
  const int i = images_find(g, blockIdx.x);
  const int t = blockIdx.x - g.first_wg[i];
  const int cols = g.slot[i].cols;
  const int by = t / cols, bx = t - by * cols;
  a.H = g.slot[i].H;
  a.W = g.slot[i].W;
  embed_tail_tile<T, SEP, TTH, false, MODE, tail_args_t<MODE>, true>(a, k, bx * TTW, by * TTH, g.slot[i].frame, static_cast<const T*>(g.slot[i].img),
                                                                     static_cast<T*>(g.slot[i].out), g.slot[i].preds_w);
}

// kernel arguments of one group of the plan
inline ImagesArgs images_args(const vs_image_desc_t* images, const vs_images_group_t& grp, const int kind, const int oh, const int ow) {
  ImagesArgs g{};
  for (int k = 0; k <= VS_IMAGES_PER_LAUNCH; ++k) g.first_wg[k] = grp.first_wg[k];
  for (int k = 0; k < grp.count; ++k) {
    const vs_image_desc_t& d = images[grp.image[k]];
    int cols = (d.W + TTW - 1) / TTW;
    if (kind == VS_IMAGES_RESIZE) {
      const int tw = grp.form == VS_IMAGES_FORM_TILE ? VS_IMG_RS_TW : (grp.form == VS_IMAGES_FORM_STREAM128 ? 128 : 64);
      cols = (ow + tw - 1) / tw;
    }
    g.slot[k] = ImgSlot{d.img, d.out, d.preds_w, d.H, d.W, grp.image[k], cols};
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------
// Lists of clips (vs_resize_pre_clips, vs_embed_tail_clips): the image lists with a frame dimension.  A slot is F frames of one size; its
// workgroups are F x tiles, frame-major (clips_plan.h), and it carries where its frames and its key frames sit in the processing-size
// tensors.  The tile bodies see a slot as a clip of its own: the slot-local frame number with the destinations (resize) or delta / hmap_lowres
// (tail) moved to the slot's first frame / first key frame -- all of it workgroup-uniform, so the bodies and their bits are the clip kernels'.
struct ClipSlot { const void* frames; void* out; float* preds_w; int F, H, W, first_frame, first_key, cols, tiles; };      // tiles: per frame
struct ClipsArgs {
  int first_wg[VS_IMAGES_PER_LAUNCH + 1];      // entries past the launch's slot count hold the grid size: never reached by a workgroup
  int pad_;
  ClipSlot slot[VS_IMAGES_PER_LAUNCH];
};
static_assert(sizeof(ClipsArgs) + sizeof(TailArgsX) + sizeof(JndTaps) <= 3072, "descriptors + tail arguments (every mode) stay well inside the 4 KiB of kernel arguments");
static_assert(sizeof(ClipsArgs) + sizeof(ResizePreEpi) <= 3072, "descriptors + resize epilogue stay well inside the 4 KiB of kernel arguments");

// (slot k, frame f of it, tile column bx, tile row by) of workgroup wg
__device__ __forceinline__ void clips_item(const ClipsArgs& g, const int wg, int& k, int& f, int& bx, int& by) {
  k = images_find(g, wg);
  const int t = wg - g.first_wg[k];
  const int tiles = g.slot[k].tiles, cols = g.slot[k].cols;
  f = t / tiles;
  const int r = t - f * tiles;
  by = r / cols;
  bx = r - by * cols;
}

template <typename T>
__global__ __launch_bounds__(256) void resize_pre_clips_kernel(const ClipsArgs g, const int oh, const int ow, const int antialias,
                                                               const ResizePreEpi o) {
  __shared__ float Lw[3 * RS_WH * RS_WW];
  int k, f, bx, by;
  clips_item(g, blockIdx.x, k, f, bx, by);
  const int H = g.slot[k].H, W = g.slot[k].W;
  const int64_t fo = (int64_t)oh * ow * 4;
  resize_pre_tile<T>(Lw, static_cast<const T*>(g.slot[k].frames) + (int64_t)f * 3 * H * W, f, bx * VS_IMG_RS_TW, by * VS_IMG_RS_TH, 3, H, W, oh, ow,
                     antialias, o.dst_rgb ? o.dst_rgb + g.slot[k].first_frame * fo : nullptr, o.mul, o.add,
                     o.dst_key ? o.dst_key + g.slot[k].first_key * fo : nullptr, o.key_step, o.key_mode, o.y0c, o.y1c, o.y2c);
}

template <int OW>
__global__ __launch_bounds__(256) void resize_pre_clips_stream_kernel(const ClipsArgs g, const int oh, const int ow, const int antialias,
                                                                      ResizePreEpi epi, const int strip) {
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  int k, f, bx, by;
  clips_item(g, blockIdx.x, k, f, bx, by);
  const int H = g.slot[k].H, W = g.slot[k].W;
  const int64_t fo = (int64_t)oh * ow * 4;
  if (epi.dst_rgb) epi.dst_rgb += g.slot[k].first_frame * fo;
  if (epi.dst_key) epi.dst_key += g.slot[k].first_key * fo;
  vs_rs::resize_stream_tile<OW>(rs_smem, static_cast<const float*>(g.slot[k].frames) + (int64_t)f * 3 * H * W, H, W, 0, 0, H, W, oh, ow, antialias,
                                strip, epi, bx, by, f);
}

// MODE (vs_embed_tail_clips_scaled / _energy): SCALED moves frame_scale to the slot's first frame, as hmap_lowres is moved, so the body's
// frame_scale[f] is the caller's frame_scale[first_frame + f]; ENERGY as in embed_tail_images_kernel, one partial per workgroup of the flat grid.
template <typename T, bool SEP, int MODE = TAIL_BLEND>
__global__ __launch_bounds__(256) void embed_tail_clips_kernel(const ClipsArgs g, tail_args_t<MODE> a, const JndTaps k) {
  int i, f, bx, by;
  clips_item(g, blockIdx.x, i, f, bx, by);
  a.F = g.slot[i].F;
  a.H = g.slot[i].H;
  a.W = g.slot[i].W;
  a.total_key = (a.F + a.step - 1) / a.step;
  const int64_t splane = (int64_t)a.Sh * a.Sw, plane = (int64_t)a.H * a.W;
  a.delta += g.slot[i].first_key * splane * a.Cd;
  if (a.hmap_lowres) a.hmap_lowres += g.slot[i].first_frame * splane;
  if constexpr (MODE == TAIL_SCALED) a.frame_scale += g.slot[i].first_frame;
  embed_tail_tile<T, SEP, TTH, false, MODE, tail_args_t<MODE>, true>(a, k, bx * TTW, by * TTH, f,
                                                                     static_cast<const T*>(g.slot[i].frames) + f * 3 * plane,
                                                                     static_cast<T*>(g.slot[i].out) + f * 3 * plane,
                                                                     g.slot[i].preds_w ? g.slot[i].preds_w + f * a.Cd * plane : nullptr);
}

// kernel arguments of one group of the plan
inline ClipsArgs clips_args(const vs_clip_desc_t* clips, const vs_images_group_t& grp, const int kind, const int oh, const int ow) {
  ClipsArgs g{};
  for (int k = 0; k <= VS_IMAGES_PER_LAUNCH; ++k) g.first_wg[k] = grp.first_wg[k];
  for (int k = 0; k < grp.count; ++k) {
    const vs_clip_desc_t& d = clips[grp.image[k]];
    int cols = (d.W + TTW - 1) / TTW;
    if (kind == VS_IMAGES_RESIZE) {
      const int tw = grp.form == VS_IMAGES_FORM_TILE ? VS_IMG_RS_TW : (grp.form == VS_IMAGES_FORM_STREAM128 ? 128 : 64);
      cols = (ow + tw - 1) / tw;
    }
    g.slot[k] = ClipSlot{d.frames, d.out, d.preds_w, d.F, d.H, d.W, d.first_frame, d.first_key, cols,
                         (int)vs_images_tiles(kind, grp.form, grp.strip, d.H, d.W, oh, ow)};
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------
// Target PSNR on the lists (videoseal_lists_psnr.h).  The energy pass of a launch group leaves one partial per workgroup in the group's run of
// `partials`; one finish launch per group adds the partials of every item of the group: an image owns [first_wg[k], first_wg[k + 1]), frame f
// of a clip slot owns [first_wg[k] + f * tiles, + tiles).  One wave per item, lane l adds partials l, l + 64, ... in that order, then the
// lanes in a fixed tree (tail_energy_finish_kernel's order): no atomics, every slot of a range was written by the pass before it is read.
struct ListFinishArgs {
  int first_wg[VS_IMAGES_PER_LAUNCH];      // first partial of item k of the group
  int frames[VS_IMAGES_PER_LAUNCH];        // 1 for an image
  int tiles[VS_IMAGES_PER_LAUNCH];         // partials per frame
  int dst[VS_IMAGES_PER_LAUNCH];           // energy[dst + f]: the image's index in the list, the slot's first_frame
};
static_assert(sizeof(ListFinishArgs) <= 3072, "the finish kernel's table travels in the kernel arguments");

// grid = (most frames of an item of the group, items of the group)
__global__ __launch_bounds__(64) void tail_list_energy_finish_kernel(const ListFinishArgs g, const double* __restrict__ partials, const double mul,
                                                                     double* __restrict__ energy) {
  const int k = blockIdx.y, f = blockIdx.x;
  if (f >= g.frames[k]) return;
  const int n = g.tiles[k];
  const double* p = partials + g.first_wg[k] + (int64_t)f * n;
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) v += p[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  if (threadIdx.x == 0) energy[g.dst[k] + f] = mul * v;
}

// scale[i] = amp * sqrt(n_g / E_g) in float64, rounded once: E_g, n_g the sums of energy / elems over the items of i's group, added in index
// order by one thread (the values come through LDS 256 at a time, so the loads of a long group are not a dependent chain).  One workgroup per
// group [first_item[g], first_item[g + 1]); an empty group writes nothing.
__global__ __launch_bounds__(256) void psnr_scale_groups_kernel(const double* __restrict__ energy, const double* __restrict__ elems,
                                                                const int* __restrict__ first_item, const int n_items, const double amp,
                                                                const float max_scale, float* __restrict__ scale) {
  __shared__ double s_e[256], s_n[256], s_E, s_N;
  // (workgroup-uniform; held inside [0, n_items]: a prefix that is wrong on the device must not turn into an access outside the arrays)
  const int lo = max(0, first_item[blockIdx.x]), hi = min(n_items, first_item[blockIdx.x + 1]);
  double E = 0.0, n = 0.0;
  for (int base = lo; base < hi; base += 256) {
    const int i = base + (int)threadIdx.x;
    if (i < hi) { s_e[threadIdx.x] = energy[i]; s_n[threadIdx.x] = elems[i]; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(256, hi - base);
      for (int j = 0; j < m; ++j) { E += s_e[j]; n += s_n[j]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { s_E = E; s_N = n; }
  __syncthreads();
  const double Eg = s_E, ng = s_N;
  const double s = Eg == 0.0 ? 0.0 : amp * sqrt(ng / Eg);
  const float r = (max_scale > 0.f && s > (double)max_scale) ? max_scale : (float)s;
  for (int i = lo + (int)threadIdx.x; i < hi; i += 256) scale[i] = r;
}

// (first_item == NULL: every item is a group of its own)
__global__ __launch_bounds__(256) void psnr_scale_items_kernel(const double* __restrict__ energy, const double* __restrict__ elems, const int n_items,
                                                               const double amp, const float max_scale, float* __restrict__ scale) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n_items) return;
  const double E = energy[i];
  const double s = E == 0.0 ? 0.0 : amp * sqrt(elems[i] / E);
  scale[i] = (max_scale > 0.f && s > (double)max_scale) ? max_scale : (float)s;
}

}  // namespace

extern "C" int vs_resize_pre(const float* src, int B, int C, int H, int W, int oh, int ow, int antialias, float* dst_rgb,
                             float mul, float add, float* dst_key, int key_step, const float* ymat3, void* stream) {
  VS_REQUIRE(src && B > 0 && C >= 1 && C <= 3 && H > 0 && W > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_key));
  VS_REQUIRE(!dst_key || key_step >= 1);
  const int key_mode = ymat3 ? 0 : 1;
  const float y0 = ymat3 ? ymat3[0] : 0.f, y1 = ymat3 ? ymat3[1] : 0.f, y2 = ymat3 ? ymat3[2] : 0.f;
  // row-streaming separable kernel (default) where its windows fit: 3 planes, <= 8 taps per direction, <= 448 input columns per 128 outputs
  // (scales up to 3.4); VIDEOSEAL_RESIZE=tile keeps the 32 x 8 tile kernel, VS_RESIZE_STRIP=<output rows> overrides the strip height
  const bool tile_only = vs_debug_get(VS_DBG_RESIZE_FORM) == 1;
  // two tile shapes (resize_stream.h): 128 output columns for scales up to 3.4 (<= 8 taps), 64 columns for scales up to 4 (<= 10 taps, 1024 -> 256)
  const int OWsel = vs_rs::rs_pick(H, W, oh, ow, antialias);
  if (!tile_only && C == 3 && OWsel) {
    const int cols = (ow + OWsel - 1) / OWsel;
    int strip = 32;
    for (int cand : {64, 48, 32, 24, 16})            // tallest strip that still gives every CU two workgroups (one round at two resident per CU)
      if ((int64_t)cols * ((oh + cand - 1) / cand) * B >= 512) { strip = cand; break; }
    if (const int v = vs_debug_get(VS_DBG_RESIZE_STRIP); v >= 1) strip = v;       // tests: any strip height, per call
    dim3 gs(cols, (oh + strip - 1) / strip, B);
    const size_t lds = OWsel == 128 ? vs_rs::rs_lds_bytes<128>() : vs_rs::rs_lds_bytes<64>();
    const ResizePreEpi epi{dst_rgb, dst_key, mul, add, key_step < 1 ? 1 : key_step, key_mode, y0, y1, y2, oh, ow};
    if ((int64_t)lds <= vs_max_lds_bytes()) {           // 68 KiB: beyond the 64 KiB of pre-gfx950 parts -> the tile kernel below
      if (OWsel == 128) hipLaunchKernelGGL(resize_pre_stream_kernel<128>, gs, dim3(256), lds, (hipStream_t)stream, src, B, H, W, oh, ow, antialias, epi, strip);
      else hipLaunchKernelGGL(resize_pre_stream_kernel<64>, gs, dim3(256), lds, (hipStream_t)stream, src, B, H, W, oh, ow, antialias, epi, strip);
      return vs_launch_status();
    }
  }
  dim3 grid((ow + 31) / 32, (oh + 7) / 8, B);
  hipLaunchKernelGGL(resize_pre_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src, B, C, H, W, oh, ow, antialias, dst_rgb, mul,
                     add, dst_key, key_step < 1 ? 1 : key_step, key_mode, y0, y1, y2);
  return vs_launch_status();
}

extern "C" int vs_resize_pre_u8(const unsigned char* src, int B, int H, int W, int oh, int ow, int antialias, float* dst_rgb,
                                float mul, float add, float* dst_key, int key_step, const float* ymat3, void* stream) {
  VS_REQUIRE(src && B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_key));
  VS_REQUIRE(!dst_key || key_step >= 1);
  const int key_mode = ymat3 ? 0 : 1;
  const float y0 = ymat3 ? ymat3[0] : 0.f, y1 = ymat3 ? ymat3[1] : 0.f, y2 = ymat3 ? ymat3[2] : 0.f;
  dim3 grid((ow + 31) / 32, (oh + 7) / 8, B);
  hipLaunchKernelGGL(resize_pre_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, src, B, 3, H, W, oh, ow, antialias,
                     dst_rgb, mul, add, dst_key, key_step < 1 ? 1 : key_step, key_mode, y0, y1, y2);
  return vs_launch_status();
}

extern "C" int vs_jnd_heatmap(const float* img, int B, int H, int W, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                              const float* taps43, float* hmap, void* stream) {
  VS_REQUIRE(img && taps43 && hmap && B > 0 && H > 0 && W > 0);
  dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
  hipLaunchKernelGGL(jnd_heatmap_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, H, W, sb, sc, sy, sx, taps_from(taps43),
                     hmap);
  return vs_launch_status();
}

namespace {

// The one dispatch of the clip tail for its three modes (vs_embed_tail, vs_embed_tail_scaled, vs_embed_tail_energy): the same rule picks the
// form in every mode, so the energy pass and the scaled tail compute the d of the tail they stand beside.  `slots`: partials per frame.
template <int MODE>
int tail_launch(const vs_tail_desc_t* d, const float* frame_scale, double* partials, int* slots, void* stream) {
  VS_REQUIRE(d && d->imgs && (MODE == TAIL_ENERGY || d->out) && d->delta && d->F > 0 && d->H > 0 && d->W > 0 && d->S_h > 0 && d->S_w > 0);
  VS_REQUIRE((d->Cd == 1 || d->Cd == 3) && d->step >= 1 && d->total_key >= 1);
  VS_REQUIRE(d->video_mode >= 0 && d->video_mode <= 2);
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  int form = d->variant >= 1 && d->variant <= 4 ? d->variant : vs_debug_get(VS_DBG_TAIL_FORM);
  if (MODE != TAIL_BLEND) {
    // the training order of operations; the 8-row A/B form asked per call.  (The 8-row body is not built in the new modes: with them beside
    // it hipcc allocates the registers of its BLEND instantiation differently, 125 -> 126 VGPRs.)
    if (d->attenuate == 2 || d->variant == 3) return VS_ERR_UNSUPPORTED;
    if (form == 3) form = 2;      // process-wide VIDEOSEAL_TAIL=keep: the 16-row tiles with the same separable stencils, the same bits
  }
  const TailArgs base{d->imgs, MODE == TAIL_ENERGY ? nullptr : d->out, MODE == TAIL_ENERGY ? nullptr : d->preds_w, d->delta,
                      d->attenuate ? d->hmap_lowres : nullptr, d->F, d->H, d->W, d->S_h, d->S_w,
                      d->Cd, d->step, d->video_mode, d->total_key, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  tail_args_t<MODE> a;
  if constexpr (MODE == TAIL_BLEND) a = base;
  else a = TailArgsX{base, frame_scale, partials};
  JndTaps k{};
  if (d->taps43) k = taps_from(d->taps43);
  dim3 grid((d->W + TTW - 1) / TTW, (d->H + TTH - 1) / TTH, d->F);
  dim3 grid8((d->W + TTW - 1) / TTW, (d->H + 7) / 8, d->F);
  // full-resolution heat-map with the standard kernels: separable stencil evaluation on 16-row tiles (default).  VIDEOSEAL_TAIL=v1 keeps the 43-tap
  // form, =keep selects 8-row tiles whose pixels stay in LDS between the luminance and the blend phase -- it fetches 1.5 x the frame instead of
  // 2.27 x but runs at 281 us against 215 us (32 x 768^2): twice the workgroups, and the per-workgroup set-up (taps, watermark window, two
  // barriers before the first output row), not HBM traffic, is what the tail pays for (profiles/r03s_shell_keep_form.log)
  // VIDEOSEAL_TAIL: stream (default) = the row-streaming kernel where it applies, sep = separable stencils on 16-row tiles (round 3's default),
  // v1 = 43-tap form, keep = 8-row tiles with the pixels parked in LDS.  d->variant (1 = v1, 2 = sep, 3 = keep, 4 = stream) overrides it per call.
  const int mode = form >= 1 && form <= 4 ? form - 1 : 3;
  const bool full_jnd = d->attenuate && !d->hmap_lowres;
  const bool sep = mode > 0 && full_jnd && d->taps43 && standard_jnd_taps(d->taps43);
  if (mode == 3 && !d->io_u8 && tail_can_stream(full_jnd, d->taps43, d->H, d->W, d->S_h, d->S_w)) {
    const int64_t cols = (d->W + TTW - 1) / TTW;
    const int strip = tail_strip(full_jnd, d->F, d->H, d->W);
    dim3 gs((unsigned)cols, (d->H + strip - 1) / strip, d->F);
    if (slots) *slots = (int)(gs.x * gs.y);
    const size_t lds_w = (size_t)2 * d->Cd * DW_W * DW_H * sizeof(float);
    const size_t lds_j = lds_w + RING * TLW * sizeof(float);
    if (full_jnd && d->Cd == 1) hipLaunchKernelGGL((embed_tail_stream_kernel<true, 1, MODE>), gs, dim3(256), lds_j, (hipStream_t)stream, a, k, strip);
    else if (full_jnd) hipLaunchKernelGGL((embed_tail_stream_kernel<true, 3, MODE>), gs, dim3(256), lds_j, (hipStream_t)stream, a, k, strip);
    else if (d->Cd == 1) hipLaunchKernelGGL((embed_tail_stream_kernel<false, 1, MODE>), gs, dim3(256), lds_w, (hipStream_t)stream, a, k, strip);
    else hipLaunchKernelGGL((embed_tail_stream_kernel<false, 3, MODE>), gs, dim3(256), lds_w, (hipStream_t)stream, a, k, strip);
    return vs_launch_status();
  }
  if (slots) *slots = (int)(grid.x * grid.y);
  if (d->io_u8) {
    VS_REQUIRE(MODE == TAIL_ENERGY || d->clamp);        // (x * 255).byte() is only defined for x in [0, 1]
    // (uint8 frames keep the 43-tap form: measured 215 us against 248 us for the separable one, profiles/r03i_shell_separable.log)
    hipLaunchKernelGGL((embed_tail_kernel<unsigned char, false, 16, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, a, k);
  } else {
    if constexpr (MODE == TAIL_BLEND) {
      if (sep && mode == 2) {
        hipLaunchKernelGGL((embed_tail_kernel<float, true, 8, true>), grid8, dim3(256), 0, (hipStream_t)stream, a, k);
        return vs_launch_status();
      }
    }
    if (sep) hipLaunchKernelGGL((embed_tail_kernel<float, true, 16, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, a, k);
    else hipLaunchKernelGGL((embed_tail_kernel<float, false, 16, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, a, k);
  }
  return vs_launch_status();
}

// one wave per frame: lane l adds the frame's partials l, l + 64, ... in that order, then the lanes are added in a fixed tree
__global__ __launch_bounds__(64) void tail_energy_finish_kernel(const double* __restrict__ partials, const int slots, const double mul,
                                                                double* __restrict__ energy) {
  const double* p = partials + (int64_t)blockIdx.x * slots;
  double v = 0.0;
  for (int i = threadIdx.x; i < slots; i += 64) v += p[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  if (threadIdx.x == 0) energy[blockIdx.x] = mul * v;
}

// scale[f] = amp * sqrt(n / E) in float64, rounded once; E = energy[f] over n = 3 H W elements, or the clip's sum over 3 F H W
__global__ __launch_bounds__(256) void psnr_scale_kernel(const double* __restrict__ energy, const int F, const double n_frame, const int per_clip,
                                                         const double amp, const float max_scale, float* __restrict__ scale) {
  __shared__ double s_tot;
  if (per_clip) {
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int f = 0; f < F; ++f) t += energy[f];
      s_tot = t;
    }
    __syncthreads();
  }
  for (int f = threadIdx.x; f < F; f += 256) {
    const double E = per_clip ? s_tot : energy[f];
    const double n = per_clip ? n_frame * (double)F : n_frame;
    const double s = E == 0.0 ? 0.0 : amp * sqrt(n / E);
    scale[f] = (max_scale > 0.f && s > (double)max_scale) ? max_scale : (float)s;
  }
}

}  // namespace

extern "C" int vs_embed_tail(const vs_tail_desc_t* d, void* stream) { return tail_launch<TAIL_BLEND>(d, nullptr, nullptr, nullptr, stream); }

// The region-wise tail is built on the 16-row tiles (43-tap and separable stencils; uint8 keeps the 43-tap form, as the plain tail does).  The
// row-streaming form is not built for it: variant 0 and 4 take the separable tiles, which give the bits of the streaming form.
extern "C" int vs_embed_tail_regions(const vs_tail_desc_t* d, const uint8_t* labels, int R, void* stream) {
  VS_REQUIRE(labels && R >= 1 && R <= VS_REGIONS_MAX);
  VS_REQUIRE(d && d->imgs && d->out && d->delta && d->F > 0 && d->H > 0 && d->W > 0 && d->S_h > 0 && d->S_w > 0);
  VS_REQUIRE((d->Cd == 1 || d->Cd == 3) && d->step >= 1 && d->total_key >= 1);
  VS_REQUIRE(d->video_mode >= 0 && d->video_mode <= 2);
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  VS_REQUIRE(!d->io_u8 || d->clamp);        // (x * 255).byte() is only defined for x in [0, 1]
  if (d->attenuate == 2 || d->variant == 3) return VS_ERR_UNSUPPORTED;
  const int form = d->variant >= 1 && d->variant <= 4 ? d->variant : vs_debug_get(VS_DBG_TAIL_FORM);
  const TailArgs base{d->imgs, d->out, d->preds_w, d->delta, d->attenuate ? d->hmap_lowres : nullptr, d->F, d->H, d->W, d->S_h, d->S_w,
                      d->Cd, d->step, d->video_mode, d->total_key, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  const TailArgsR a{base, labels, R};
  JndTaps k{};
  if (d->taps43) k = taps_from(d->taps43);
  const bool full_jnd = d->attenuate && !d->hmap_lowres;
  const bool sep = form != 1 && full_jnd && d->taps43 && standard_jnd_taps(d->taps43);
  VS_REQUIRE(d->F <= 65535 && (d->H + TTH - 1) / TTH <= 65535);
  dim3 grid(((d->W + TTW - 1) / TTW) * R, (d->H + TTH - 1) / TTH, d->F);
  if (d->io_u8) hipLaunchKernelGGL((embed_tail_regions_kernel<unsigned char, false>), grid, dim3(256), 0, (hipStream_t)stream, a, k);
  else if (sep) hipLaunchKernelGGL((embed_tail_regions_kernel<float, true>), grid, dim3(256), 0, (hipStream_t)stream, a, k);
  else hipLaunchKernelGGL((embed_tail_regions_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream, a, k);
  return vs_launch_status();
}

extern "C" int vs_embed_tail_scaled(const vs_tail_desc_t* d, const float* frame_scale, void* stream) {
  VS_REQUIRE(frame_scale);
  return tail_launch<TAIL_SCALED>(d, frame_scale, nullptr, nullptr, stream);
}

// strips of the row-streaming form are at least four rows tall (tail_strip), tiles sixteen: the bound holds for every form.  Four rows is the
// floor of the VS_TAIL_STRIP development switch; the strips the library picks are 32 - 96 rows and tiles 16, so a launch uses a 4th to a 24th
// of this workspace (768^2: 576 doubles per frame sized, 24 - 144 written).  Small next to a frame, and a size function may not depend on a switch.
extern "C" int64_t vs_tail_energy_partial_doubles(int F, int H, int W) {
  if (F <= 0 || H <= 0 || W <= 0) return -1;
  return (int64_t)F * ((W + TTW - 1) / TTW) * ((H + 3) / 4);
}

extern "C" int vs_embed_tail_energy(const vs_tail_desc_t* d, double* partials, double* energy, void* stream) {
  VS_REQUIRE(partials && energy);
  int slots = 0;
  if (const int rc = tail_launch<TAIL_ENERGY>(d, nullptr, partials, &slots, stream); rc != VS_OK) return rc;
  hipLaunchKernelGGL(tail_energy_finish_kernel, dim3(d->F), dim3(64), 0, (hipStream_t)stream, partials, slots, 3.0 / d->Cd, energy);
  return vs_launch_status();
}

extern "C" int vs_psnr_scale(const double* energy, int F, int H, int W, int per_clip, float target_db, float max_scale, float* scale,
                             void* stream) {
  VS_REQUIRE(energy && scale && F > 0 && H > 0 && W > 0 && std::isfinite(target_db));
  const double amp = std::pow(10.0, -(double)target_db / 20.0);      // (host libm: the device evaluates one division and one square root)
  hipLaunchKernelGGL(psnr_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, energy, F, 3.0 * H * W, per_clip ? 1 : 0, amp, max_scale, scale);
  return vs_launch_status();
}

extern "C" int vs_resize_pre_images(const vs_image_desc_t* images, int n, int io_u8, int oh, int ow, int antialias, float* dst_rgb, float mul,
                                    float add, float* dst_key, const float* ymat3, void* stream) {
  VS_REQUIRE(images && n > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_key));
  for (int i = 0; i < n; ++i) VS_REQUIRE(images[i].img && images[i].H > 0 && images[i].W > 0);
  if ((int64_t)vs_rs::rs_lds_bytes<128>() > vs_max_lds_bytes() || (int64_t)vs_rs::rs_lds_bytes<64>() > vs_max_lds_bytes()) return VS_ERR_UNSUPPORTED;
  int n_groups = 0;      // a dry walk first: a list the plan refuses launches nothing
  if (const int rc = vs_images_plan(images, n, VS_IMAGES_RESIZE, io_u8, oh, ow, antialias, nullptr, 0, &n_groups); rc != VS_OK) return rc;
  const int key_mode = ymat3 ? 0 : 1;
  const float y0 = ymat3 ? ymat3[0] : 0.f, y1 = ymat3 ? ymat3[1] : 0.f, y2 = ymat3 ? ymat3[2] : 0.f;
  const ResizePreEpi epi{dst_rgb, dst_key, mul, add, 1, key_mode, y0, y1, y2, oh, ow};
  const int aa = antialias ? 1 : 0;
  return vs_images_walk(images, n, VS_IMAGES_RESIZE, io_u8 ? 1 : 0, oh, ow, aa, [&](const vs_images_group_t& grp) {
    const ImagesArgs g = images_args(images, grp, VS_IMAGES_RESIZE, oh, ow);
    const dim3 grid((unsigned)grp.first_wg[grp.count]);
    if (grp.form == VS_IMAGES_FORM_STREAM128)
      hipLaunchKernelGGL(resize_pre_images_stream_kernel<128>, grid, dim3(256), vs_rs::rs_lds_bytes<128>(), (hipStream_t)stream, g, oh, ow, aa, epi, grp.strip);
    else if (grp.form == VS_IMAGES_FORM_STREAM64)
      hipLaunchKernelGGL(resize_pre_images_stream_kernel<64>, grid, dim3(256), vs_rs::rs_lds_bytes<64>(), (hipStream_t)stream, g, oh, ow, aa, epi, grp.strip);
    else if (io_u8)
      hipLaunchKernelGGL(resize_pre_images_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, g, oh, ow, aa, epi);
    else
      hipLaunchKernelGGL(resize_pre_images_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, g, oh, ow, aa, epi);
    return vs_launch_status();
  });
}

namespace {

// The one dispatch of the image-list tail for its three modes (vs_embed_tail_images, vs_embed_tail_images_scaled, vs_embed_tail_images_energy):
// the same checks, the same plan and the same choice of stencils, so the energy pass and the scaled tail compute the d of the tail they stand
// beside.  ENERGY: the partials of a launch group follow those of the groups before it, and a finish launch follows every group's pass.
template <int MODE>
int tail_images_launch(const vs_tail_images_desc_t* d, const float* scale, double* partials, double* energy, void* stream) {
  VS_REQUIRE(d && d->images && d->n > 0 && d->delta && d->S_h > 0 && d->S_w > 0 && (d->Cd == 1 || d->Cd == 3));
  for (int i = 0; i < d->n; ++i)
    VS_REQUIRE(d->images[i].img && (MODE == TAIL_ENERGY || d->images[i].out) && d->images[i].H > 0 && d->images[i].W > 0);
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  VS_REQUIRE(MODE == TAIL_ENERGY || !d->io_u8 || d->clamp);        // (x * 255).byte() is only defined for x in [0, 1]
  if (d->attenuate != 0 && d->attenuate != 1) return VS_ERR_UNSUPPORTED;      // (2: the training forward's order, clips only)
  int n_groups = 0;
  if (const int rc = vs_images_plan(d->images, d->n, VS_IMAGES_TAIL, d->io_u8, d->S_h, d->S_w, d->antialias, nullptr, 0, &n_groups); rc != VS_OK) return rc;
  // F = total_key = n, step 1, 'repeat': frame i of delta / hmap_lowres belongs to image i; H and W are the image's (set per workgroup)
  const TailArgs base{nullptr, nullptr, nullptr, d->delta, d->attenuate ? d->hmap_lowres : nullptr, d->n, 0, 0, d->S_h, d->S_w, d->Cd, 1,
                      VS_VIDEO_REPEAT, d->n, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  tail_args_t<MODE> a;
  if constexpr (MODE == TAIL_BLEND) a = base;
  else a = TailArgsX{base, scale, partials};
  JndTaps k{};
  if (d->taps43) k = taps_from(d->taps43);
  const bool full_jnd = d->attenuate && !d->hmap_lowres;
  const bool sep = full_jnd && standard_jnd_taps(d->taps43);
  return vs_images_walk(d->images, d->n, VS_IMAGES_TAIL, d->io_u8 ? 1 : 0, d->S_h, d->S_w, d->antialias ? 1 : 0, [&](const vs_images_group_t& grp) {
    ImagesArgs g = images_args(d->images, grp, VS_IMAGES_TAIL, d->S_h, d->S_w);
    if (MODE == TAIL_ENERGY)
      for (int s = 0; s < grp.count; ++s) g.slot[s].out = nullptr, g.slot[s].preds_w = nullptr;
    const dim3 grid((unsigned)grp.first_wg[grp.count]);
    // (uint8 images keep the 43-tap form, as uint8 clips do)
    if (d->io_u8) hipLaunchKernelGGL((embed_tail_images_kernel<unsigned char, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, g, a, k);
    else if (sep) hipLaunchKernelGGL((embed_tail_images_kernel<float, true, MODE>), grid, dim3(256), 0, (hipStream_t)stream, g, a, k);
    else hipLaunchKernelGGL((embed_tail_images_kernel<float, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, g, a, k);
    if constexpr (MODE == TAIL_ENERGY) {
      if (const int rc = vs_launch_status(); rc != VS_OK) return rc;
      ListFinishArgs fa{};
      for (int s = 0; s < grp.count; ++s) {
        fa.first_wg[s] = grp.first_wg[s];
        fa.frames[s] = 1;
        fa.tiles[s] = grp.first_wg[s + 1] - grp.first_wg[s];
        fa.dst[s] = grp.image[s];
      }
      hipLaunchKernelGGL(tail_list_energy_finish_kernel, dim3(1, grp.count), dim3(64), 0, (hipStream_t)stream, fa, a.partials, 3.0 / d->Cd, energy);
      a.partials += grp.first_wg[grp.count];
    }
    return vs_launch_status();
  });
}

}  // namespace

extern "C" int vs_embed_tail_images(const vs_tail_images_desc_t* d, void* stream) {
  return tail_images_launch<TAIL_BLEND>(d, nullptr, nullptr, nullptr, stream);
}

extern "C" int vs_embed_tail_images_scaled(const vs_tail_images_desc_t* d, const float* image_scale, void* stream) {
  VS_REQUIRE(image_scale);
  return tail_images_launch<TAIL_SCALED>(d, image_scale, nullptr, nullptr, stream);
}

extern "C" int vs_embed_tail_images_energy(const vs_tail_images_desc_t* d, double* partials, double* energy, void* stream) {
  VS_REQUIRE(partials && energy);
  return tail_images_launch<TAIL_ENERGY>(d, nullptr, partials, energy, stream);
}

extern "C" int64_t vs_tail_images_energy_partial_doubles(const vs_image_desc_t* images, int n, int io_u8, int S_h, int S_w, int antialias) {
  if (n < 0 || (n > 0 && !images) || S_h <= 0 || S_w <= 0) return -1;
  for (int i = 0; i < n; ++i)
    if (images[i].H <= 0 || images[i].W <= 0) return -1;
  int64_t total = 0;
  const int rc = vs_images_walk(images, n, VS_IMAGES_TAIL, io_u8 ? 1 : 0, S_h, S_w, antialias ? 1 : 0, [&](const vs_images_group_t& grp) {
    total += grp.first_wg[grp.count];
    return (int)VS_OK;
  });
  return rc == VS_OK ? total : -1;
}

extern "C" int vs_resize_pre_clips(const vs_clip_desc_t* clips, int n, int io_u8, int oh, int ow, int antialias, float* dst_rgb, float mul,
                                   float add, float* dst_key, int key_step, const float* ymat3, void* stream) {
  VS_REQUIRE(clips && n > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_key));
  VS_REQUIRE(!dst_key || key_step >= 1);
  for (int i = 0; i < n; ++i)
    VS_REQUIRE(clips[i].frames && clips[i].F > 0 && clips[i].H > 0 && clips[i].W > 0 && clips[i].first_frame >= 0 && clips[i].first_key >= 0);
  if ((int64_t)vs_rs::rs_lds_bytes<128>() > vs_max_lds_bytes() || (int64_t)vs_rs::rs_lds_bytes<64>() > vs_max_lds_bytes()) return VS_ERR_UNSUPPORTED;
  int n_groups = 0;      // a dry walk first: a list the plan refuses launches nothing
  if (const int rc = vs_clips_plan(clips, n, VS_IMAGES_RESIZE, io_u8, oh, ow, antialias, nullptr, 0, &n_groups); rc != VS_OK) return rc;
  const int key_mode = ymat3 ? 0 : 1;
  const float y0 = ymat3 ? ymat3[0] : 0.f, y1 = ymat3 ? ymat3[1] : 0.f, y2 = ymat3 ? ymat3[2] : 0.f;
  const ResizePreEpi epi{dst_rgb, dst_key, mul, add, key_step < 1 ? 1 : key_step, key_mode, y0, y1, y2, oh, ow};
  const int aa = antialias ? 1 : 0;
  return vs_clips_walk(clips, n, VS_IMAGES_RESIZE, io_u8 ? 1 : 0, oh, ow, aa, [&](const vs_images_group_t& grp) {
    const ClipsArgs g = clips_args(clips, grp, VS_IMAGES_RESIZE, oh, ow);
    const dim3 grid((unsigned)grp.first_wg[grp.count]);
    if (grp.form == VS_IMAGES_FORM_STREAM128)
      hipLaunchKernelGGL(resize_pre_clips_stream_kernel<128>, grid, dim3(256), vs_rs::rs_lds_bytes<128>(), (hipStream_t)stream, g, oh, ow, aa, epi, grp.strip);
    else if (grp.form == VS_IMAGES_FORM_STREAM64)
      hipLaunchKernelGGL(resize_pre_clips_stream_kernel<64>, grid, dim3(256), vs_rs::rs_lds_bytes<64>(), (hipStream_t)stream, g, oh, ow, aa, epi, grp.strip);
    else if (io_u8)
      hipLaunchKernelGGL(resize_pre_clips_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, g, oh, ow, aa, epi);
    else
      hipLaunchKernelGGL(resize_pre_clips_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, g, oh, ow, aa, epi);
    return vs_launch_status();
  });
}

namespace {

// tail_images_launch for slots.  n_frames (SCALED, ENERGY): the length of frame_scale / energy; a slot that reaches past it is refused before
// any launch.
template <int MODE>
int tail_clips_launch(const vs_tail_clips_desc_t* d, const float* scale, double* partials, double* energy, int n_frames, void* stream) {
  VS_REQUIRE(d && d->clips && d->n > 0 && d->delta && d->S_h > 0 && d->S_w > 0 && (d->Cd == 1 || d->Cd == 3));
  VS_REQUIRE(d->step >= 1 && d->video_mode >= 0 && d->video_mode <= 2);
  for (int i = 0; i < d->n; ++i) {
    const vs_clip_desc_t& c = d->clips[i];
    VS_REQUIRE(c.frames && (MODE == TAIL_ENERGY || c.out) && c.F > 0 && c.H > 0 && c.W > 0 && c.first_frame >= 0 && c.first_key >= 0);
    VS_REQUIRE(MODE == TAIL_BLEND || (int64_t)c.first_frame + c.F <= n_frames);
  }
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  VS_REQUIRE(MODE == TAIL_ENERGY || !d->io_u8 || d->clamp);        // (x * 255).byte() is only defined for x in [0, 1]
  if (d->attenuate != 0 && d->attenuate != 1) return VS_ERR_UNSUPPORTED;      // (2: the training forward's order, single clips only)
  int n_groups = 0;
  if (const int rc = vs_clips_plan(d->clips, d->n, VS_IMAGES_TAIL, d->io_u8, d->S_h, d->S_w, d->antialias, nullptr, 0, &n_groups); rc != VS_OK) return rc;
  // F, H, W, total_key and the first frames of delta / hmap_lowres are the slot's (set per workgroup)
  const TailArgs base{nullptr, nullptr, nullptr, d->delta, d->attenuate ? d->hmap_lowres : nullptr, 0, 0, 0, d->S_h, d->S_w, d->Cd, d->step,
                      d->video_mode, 0, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  tail_args_t<MODE> a;
  if constexpr (MODE == TAIL_BLEND) a = base;
  else a = TailArgsX{base, scale, partials};
  JndTaps k{};
  if (d->taps43) k = taps_from(d->taps43);
  const bool full_jnd = d->attenuate && !d->hmap_lowres;
  const bool sep = full_jnd && standard_jnd_taps(d->taps43);
  return vs_clips_walk(d->clips, d->n, VS_IMAGES_TAIL, d->io_u8 ? 1 : 0, d->S_h, d->S_w, d->antialias ? 1 : 0, [&](const vs_images_group_t& grp) {
    ClipsArgs g = clips_args(d->clips, grp, VS_IMAGES_TAIL, d->S_h, d->S_w);
    if (MODE == TAIL_ENERGY)
      for (int s = 0; s < grp.count; ++s) g.slot[s].out = nullptr, g.slot[s].preds_w = nullptr;
    const dim3 grid((unsigned)grp.first_wg[grp.count]);
    // (uint8 clips keep the 43-tap form, as vs_embed_tail does)
    if (d->io_u8) hipLaunchKernelGGL((embed_tail_clips_kernel<unsigned char, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, g, a, k);
    else if (sep) hipLaunchKernelGGL((embed_tail_clips_kernel<float, true, MODE>), grid, dim3(256), 0, (hipStream_t)stream, g, a, k);
    else hipLaunchKernelGGL((embed_tail_clips_kernel<float, false, MODE>), grid, dim3(256), 0, (hipStream_t)stream, g, a, k);
    if constexpr (MODE == TAIL_ENERGY) {
      if (const int rc = vs_launch_status(); rc != VS_OK) return rc;
      ListFinishArgs fa{};
      int most = 1;
      for (int s = 0; s < grp.count; ++s) {
        fa.first_wg[s] = grp.first_wg[s];
        fa.frames[s] = g.slot[s].F;
        fa.tiles[s] = g.slot[s].tiles;
        fa.dst[s] = g.slot[s].first_frame;
        most = g.slot[s].F > most ? g.slot[s].F : most;
      }
      hipLaunchKernelGGL(tail_list_energy_finish_kernel, dim3(most, grp.count), dim3(64), 0, (hipStream_t)stream, fa, a.partials, 3.0 / d->Cd, energy);
      a.partials += grp.first_wg[grp.count];
    }
    return vs_launch_status();
  });
}

}  // namespace

extern "C" int vs_embed_tail_clips(const vs_tail_clips_desc_t* d, void* stream) {
  return tail_clips_launch<TAIL_BLEND>(d, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int vs_embed_tail_clips_scaled(const vs_tail_clips_desc_t* d, const float* frame_scale, int n_frames, void* stream) {
  VS_REQUIRE(frame_scale && n_frames > 0);
  return tail_clips_launch<TAIL_SCALED>(d, frame_scale, nullptr, nullptr, n_frames, stream);
}

extern "C" int vs_embed_tail_clips_energy(const vs_tail_clips_desc_t* d, double* partials, double* energy, int n_frames, void* stream) {
  VS_REQUIRE(partials && energy && n_frames > 0);
  return tail_clips_launch<TAIL_ENERGY>(d, nullptr, partials, energy, n_frames, stream);
}

extern "C" int64_t vs_tail_clips_energy_partial_doubles(const vs_clip_desc_t* clips, int n, int io_u8, int S_h, int S_w, int antialias) {
  if (n < 0 || (n > 0 && !clips) || S_h <= 0 || S_w <= 0) return -1;
  for (int i = 0; i < n; ++i)
    if (clips[i].F <= 0 || clips[i].H <= 0 || clips[i].W <= 0) return -1;
  int64_t total = 0;
  const int rc = vs_clips_walk(clips, n, VS_IMAGES_TAIL, io_u8 ? 1 : 0, S_h, S_w, antialias ? 1 : 0, [&](const vs_images_group_t& grp) {
    total += grp.first_wg[grp.count];
    return (int)VS_OK;
  });
  return rc == VS_OK ? total : -1;
}

extern "C" int vs_psnr_scale_items(const double* energy, const double* elems, const int32_t* first_item, int n_items, int n_groups, float target_db,
                                   float max_scale, float* scale, void* stream) {
  VS_REQUIRE(energy && elems && scale && n_items > 0 && std::isfinite(target_db));
  VS_REQUIRE(!first_item || n_groups > 0);
  const double amp = std::pow(10.0, -(double)target_db / 20.0);      // (host libm, as vs_psnr_scale)
  if (first_item)
    hipLaunchKernelGGL(psnr_scale_groups_kernel, dim3(n_groups), dim3(256), 0, (hipStream_t)stream, energy, elems, first_item, n_items, amp, max_scale,
                       scale);
  else
    hipLaunchKernelGGL(psnr_scale_items_kernel, dim3((n_items + 255) / 256), dim3(256), 0, (hipStream_t)stream, energy, elems, n_items, amp, max_scale,
                       scale);
  return vs_launch_status();
}
