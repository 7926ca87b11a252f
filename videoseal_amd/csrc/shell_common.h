// What the shell kernels of shell.hip, the YUV family (yuv_surf.h) and the packed RGB family (rgb_surf.h) share: tile geometry, the resize_pre
// epilogue, the JND and blend expressions (every kernel calls the SAME functions, so its forms agree bit for bit), the tail arguments, the
// colour affines of the YUV kernels and, on the host, the launch rules: which tail form, which strip heights, and the one launcher of each
// phase for the two surface families.  (The phases of the surface tails are tail_phases.h.)
#pragma once
#include "vs_common.h"
#include "resize_taps.h"
#include "resize_stream.h"

namespace {

using namespace vs_taps;

// ---------------------------------------------------------------------------------------------------
constexpr int TTW = 256, TTH = 16, TLW = TTW + 4;   // embed tail tile: 256 columns (one per thread) x 16 rows
constexpr int DW_W = 136, DW_H = 12;      // its delta source window in LDS (covers up-resizes by >= 2x; a 3x one needs ~90 x 9)
constexpr int RS_WW = 113, RS_WH = 32;   // LDS window of resize_pre (odd row pitch); covers down-scales up to ~3.3x
constexpr int MAXT = 8;   // taps held in registers by the resize kernels (triangle filter support 2*scale + 1 <= 8 for scale <= 3.5)

// The row-streaming form lives in resize_stream.h (shared with aug.hip's Crop -> Resize -> colour kernel); this is its `resize_pre` epilogue:
// NHWC(4) rgb * mul + add and / or the key frames' Y (or rgb) mapped to [-1, 1].
struct ResizePreEpi {
  float* dst_rgb; float* dst_key; float mul, add; int key_step, key_mode; float y0c, y1c, y2c; int oh, ow;
  __device__ __forceinline__ void operator()(const int b, const int oy, const int ox, const float (&acc)[3]) const {
    const int64_t opix = ((int64_t)oy * ow + ox);
    if (dst_rgb) {
      f32x4 v = {acc[0] * mul + add, acc[1] * mul + add, acc[2] * mul + add, 0.f};
      *reinterpret_cast<f32x4*>(dst_rgb + ((int64_t)b * oh * ow + opix) * 4) = v;
    }
    if (dst_key && (b % key_step) == 0) {
      f32x4 v;
      if (key_mode == 0) {
        const float y = y0c * acc[0] + y1c * acc[1] + y2c * acc[2];
        v = f32x4{y * 2.f - 1.f, 0.f, 0.f, 0.f};
      } else {
        v = f32x4{acc[0] * 2.f - 1.f, acc[1] * 2.f - 1.f, acc[2] * 2.f - 1.f, 0.f};
      }
      *reinterpret_cast<f32x4*>(dst_key + ((int64_t)(b / key_step) * oh * ow + opix) * 4) = v;
    }
  }
};

// ---- JND (jnd.py:63-108) on a luminance tile held in LDS --------------------------------------------------
struct JndTaps { float lum[25]; float sx[9]; float sy[9]; };

// luminance of 255 * rgb (jnd.py:86-89) and the blend (blender.py:61-68, wam.py:103-113 / jnd.py:110-114) evaluated the way ATen does: separate
// multiplications and additions, no fused multiply-add.  Every kernel of the tail calls these two functions, so its forms agree bit for bit
// (hipcc's contraction of `a * b + c * d` picks either product for the fma depending on the surrounding code).
__device__ __forceinline__ float lum255(const float r, const float g, const float b) {
#pragma clang fp contract(off)
  return 0.299f * (255.f * r) + 0.587f * (255.f * g) + 0.114f * (255.f * b);
}
__device__ __forceinline__ float blend_px(const float si, const float sw, const float p, const float dw, const float hm, const bool fwd_order) {
#pragma clang fp contract(off)
  float v = si * p + sw * dw;
  if (fwd_order) v = p + hm * (v - p);
  return v;
}

__device__ __forceinline__ float jnd_at(const float* L, int stride, int x, int y, const JndTaps& k) {
  // L points at tile origin, (x,y) is the centre inside the tile with a 2-pixel halo available
  float la = 0.f;
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) la += k.lum[i * 5 + j] * L[(y + i - 2) * stride + (x + j - 2)];
  la = la / 32.f;
  la = la <= 127.f ? 17.f * (1.f - sqrtf(la / 127.f + 1e-5f)) : 3.f / 128.f * (la - 127.f) + 3.f;
  float gx = 0.f, gy = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = L[(y + i - 1) * stride + (x + j - 1)];
      gx += k.sx[i * 3 + j] * v;
      gy += k.sy[i * 3 + j] * v;
    }
  float cm = sqrtf(__builtin_fmaf(gx, gx, gy * gy));
  // cm^2.4 through the hardware log2/exp2 (1 ulp each): relative error <= ~1e-6 on a term that enters the frame scaled by
  // 1/255 * delta * scaling_w, i.e. < 1e-8 absolute -- ocml's powf costs ~10x the instructions
  cm = 16.f * (cm > 0.f ? __builtin_amdgcn_exp2f(2.4f * __builtin_amdgcn_logf(cm)) : 0.f) / (cm * cm + 676.f);
  cm = 0.117f * cm;
  const float h = la + cm - 0.3f * fminf(la, cm);
  return fmaxf(h, 0.f) / 255.f;
}

constexpr int TW = 32, TH = 8, HALO = 2, LW = TW + 2 * HALO, LH = TH + 2 * HALO;

// delta taps of one output pixel from the staged source window: d[c] = sum_jy wy * sum_jx wx * Dw[c][..] (Dw = hm*(wa*key_a+wb*key_b))
template <int NT, int DWH = DW_H>
__device__ __forceinline__ void tail_taps(float (&d)[3], const float* Dw, const int Cd, const int base, const int xn, const int yn,
                                          const float* wxp, const float* wyp) {
  int ox[NT], oy[NT];
  float wx[NT], wy[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {       // clamped offsets + zero weights past the real tap count: no branches, all reads in flight
    ox[j] = j < xn ? j : xn - 1;
    oy[j] = (j < yn ? j : yn - 1) * DW_W;
    wx[j] = wxp[j];
    wy[j] = wyp[j];
  }
  for (int c = 0; c < Cd; ++c) {
    const float* p = Dw + c * (DW_W * DWH) + base;
    float v[NT][NT];
#pragma unroll
    for (int jy = 0; jy < NT; ++jy)
#pragma unroll
      for (int jx = 0; jx < NT; ++jx) v[jy][jx] = p[oy[jy] + ox[jx]];
    // explicit fma chains: `r += wx * v` with r starting at 0 leaves hipcc an `a * b + c * d` to contract, and it fuses EITHER product depending on
    // the surrounding code -- two kernels calling this function disagreed in the last bit (round 4)
    float dc = 0.f;
#pragma unroll
    for (int jy = 0; jy < NT; ++jy) {
      float r = 0.f;
#pragma unroll
      for (int jx = 0; jx < NT; ++jx) r = __builtin_fmaf(wx[jx], v[jy][jx], r);
      dc = __builtin_fmaf(wy[jy], r, dc);
    }
    d[c] = dc;
  }
}

// STANDARD JND kernels (jnd.py:24-41: Sobel pair + the 5 x 5 luminance mask = box5 + box3 - 2 centre) evaluated separably inside
// embed_tail_kernel<T, true>: for a group of RG output rows the RG + 4 luminance rows are read once (5 LDS reads per row: x-2 .. x+2), giving per
// row H5 = box5 row sum, H3, S = L[x+1] - L[x-1] and T = L[x-1] + 2 L[x] + L[x+1]; the vertical combinations run over registers -- 10 LDS reads
// per pixel instead of 43.  The luminance mask jumps at la = 127 (jnd.py:66-68): a pixel whose separable sum lands within 0.02 of the jump is
// re-evaluated with the 25-tap order of jnd_at, so the branch taken is the one the generic path / the low-resolution heat-map kernel take.
// Measured (32 x 768^2, fp32, full JND, no preds_w): 43-tap form 227 us, this form 215 us -- the LDS taps were not the limit; what the JND costs
// over the plain tail (137 us) is the separate luminance phase (1.27 x frame read + LDS fill + barrier before the first output row).  A
// column-register form that reads the frame once and keeps the 16 centre pixels in registers needed 195 VGPRs (two waves per SIMD) and
// ran at 391 us: profiles/r03h_shell_*.log, r03i_shell_separable.log.
__device__ __forceinline__ float jnd_finish(float la_sum, float gx, float gy) {
  float la = la_sum / 32.f;
  la = la <= 127.f ? 17.f * (1.f - sqrtf(la / 127.f + 1e-5f)) : 3.f / 128.f * (la - 127.f) + 3.f;
  float cm = sqrtf(__builtin_fmaf(gx, gx, gy * gy));
  cm = 16.f * (cm > 0.f ? __builtin_amdgcn_exp2f(2.4f * __builtin_amdgcn_logf(cm)) : 0.f) / (cm * cm + 676.f);
  cm = 0.117f * cm;
  const float h = la + cm - 0.3f * fminf(la, cm);
  return fmaxf(h, 0.f) / 255.f;
}

// ---------------------------------------------------------------------------------------------------
struct TailArgs {
  const void* imgs; void* out; float* preds_w; const float* delta; const float* hmap_lowres;
  int F, H, W, Sh, Sw, Cd, step, video_mode, total_key, attenuate, clamp, antialias;
  float scaling_i, scaling_w;
};

constexpr int SG = 4, RING = 3 * SG, SUBR = 16;

__device__ __forceinline__ float jnd_at_ring(const float* Lr, const int cslot, const int lxh, const JndTaps& k) {
  // jnd_at() on the ring: rows cslot - 2 .. cslot + 2 (mod RING), columns lxh - 2 .. lxh + 2; same summation order
  float la = 0.f;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const float* row = Lr + ((cslot + i + RING - 2) % RING) * TLW + lxh;
#pragma unroll
    for (int j = 0; j < 5; ++j) la += k.lum[i * 5 + j] * row[j - 2];
  }
  la = la / 32.f;
  la = la <= 127.f ? 17.f * (1.f - sqrtf(la / 127.f + 1e-5f)) : 3.f / 128.f * (la - 127.f) + 3.f;
  float gx = 0.f, gy = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float* row = Lr + ((cslot + i + RING - 1) % RING) * TLW + lxh;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = row[j - 1];
      gx += k.sx[i * 3 + j] * v;
      gy += k.sy[i * 3 + j] * v;
    }
  }
  float cm = sqrtf(__builtin_fmaf(gx, gx, gy * gy));
  cm = 16.f * (cm > 0.f ? __builtin_amdgcn_exp2f(2.4f * __builtin_amdgcn_logf(cm)) : 0.f) / (cm * cm + 676.f);
  cm = 0.117f * cm;
  const float h = la + cm - 0.3f * fminf(la, cm);
  return fmaxf(h, 0.f) / 255.f;
}

// ---------------------------------------------------------------------------------------------------
// The colour affines of the 4:2:0 kernels (yuv420.hip).  They come from the host (videoseal_amd/yuv420.py: built and inverted in float64,
// handed over as 12 floats, row-major 3 x 4) in code units of the surface's depth: dec maps (Y, Cb, Cr, 1) to RGB, which is clamped to [0, 1]
// before anything else uses it; enc maps (R, G, B, 1) back to code units.
struct Nv12Mat { float m[12]; };

// (explicit fma chains: every 4:2:0 kernel evaluates the same expression, see tail_taps)
__device__ __forceinline__ float nv12_aff(const Nv12Mat& k, const int r, const float a, const float b, const float c) {
  return __builtin_fmaf(k.m[4 * r], a, __builtin_fmaf(k.m[4 * r + 1], b, __builtin_fmaf(k.m[4 * r + 2], c, k.m[4 * r + 3])));
}
__device__ __forceinline__ void nv12_rgb(const Nv12Mat& k, const float y, const float cb, const float cr, float (&rgb)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[c] = fminf(fmaxf(nv12_aff(k, c, y, cb, cr), 0.f), 1.f);
}

// ---------------------------------------------------------------------------------------------------
// the taps of jnd.py:24-41 (what every released card carries in its state dict)
inline bool standard_jnd_taps(const float* t) {
  static const float lum[25] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 2, 0, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1};
  static const float sx[9] = {-1, 0, 1, -2, 0, 2, -1, 0, 1}, sy[9] = {1, 2, 1, 0, 0, 0, -1, -2, -1};
  for (int i = 0; i < 25; ++i) if (t[i] != lum[i]) return false;
  for (int i = 0; i < 9; ++i) if (t[25 + i] != sx[i] || t[34 + i] != sy[i]) return false;
  return true;
}

// The launch rule of the row-streaming tail, one copy for vs_embed_tail (fp32) and the 4:2:0 tails.  The form applies to an up-scale of the
// watermark by >= 2 in both directions and, for the full-resolution heat-map, the standard JND taps.
inline bool tail_can_stream(bool full_jnd, const float* taps43, int H, int W, int Sh, int Sw) {
  return (!full_jnd || (taps43 && standard_jnd_taps(taps43))) && W >= 2 * Sw && H >= 2 * Sh;
}
// strip height, from tools/bench_tail_sweep.py (profiles/r04zz_tail_sweep.log, 768^2; us for 16 / 32 / 128 frames): without the luminance phase
// short strips win (32 rows 43 / 104 / 364, 48 rows 44 / 94 / 360, 96 rows 61 / 114 / 354); with it the strip should be tall (4 halo rows + the
// pipeline fill per strip) as long as the launch still has three workgroups per CU: 96 rows 115 / 155 / 503, 48 rows 76 / 151 / 510, 32 rows 87 / 152 / 521
inline int tail_strip(bool full_jnd, int F, int H, int W) {
  const int64_t cols = (W + TTW - 1) / TTW;
  int strip = 32;
  if (full_jnd) {
    for (int cand : {96, 48})
      if (cols * ((H + cand - 1) / cand) * F >= 768) { strip = cand; break; }
  } else if (cols * ((H + 47) / 48) * F >= 1024) {
    strip = 48;
  }
  if (const int v = vs_debug_get(VS_DBG_TAIL_STRIP); v >= 4) strip = (v + 3) / 4 * 4;     // VS_TAIL_STRIP; tests: every strip height, per call
  return strip;
}

inline JndTaps taps_from(const float* t43) {
  JndTaps k;
  for (int i = 0; i < 25; ++i) k.lum[i] = t43[i];
  for (int i = 0; i < 9; ++i) { k.sx[i] = t43[25 + i]; k.sy[i] = t43[34 + i]; }
  return k;
}


// ---- the surface families (YUV, packed RGB) on the host: one launcher per phase.  K names a family's kernels for one surface trait --
//   K::ALIGN, K::resize_stream<OW>(), K::resize_tile(), K::tail_stream<JND, CD>(), K::tail_tile()
// -- and `surf...` are the leading kernel arguments that describe the source (YUV: planes, decode affine; RGB: plane, component positions).
struct ResizeOut { float* dst_rgb; float mul, add; float* dst_key; int key_step, key_mode; float y0, y1, y2; };
inline ResizeOut resize_out(float* dst_rgb, float mul, float add, float* dst_key, int key_step, const float* ymat3) {
  return ResizeOut{dst_rgb, mul, add, dst_key, key_step < 1 ? 1 : key_step, ymat3 ? 0 : 1, ymat3 ? ymat3[0] : 0.f, ymat3 ? ymat3[1] : 0.f, ymat3 ? ymat3[2] : 0.f};
}
// strip of the surfaces' row-streaming resize: the tallest that still launches ~512 workgroups (two per CU), down to 8 rows for the 8-frame
// launches of detect: the fastest height of every batch size in `tools/bench_nv12.py --sweep` (profiles/nv12_resize_strip_sweep.json)
inline int surf_resize_strip(int cols, int oh, int B) {
  int strip = 8;
  for (int cand : {64, 48, 32, 24, 16, 12})
    if ((int64_t)cols * ((oh + cand - 1) / cand) * B >= 512) { strip = cand; break; }
  if (const int v = vs_debug_get(VS_DBG_RESIZE_STRIP); v >= 1) strip = v;
  return strip;
}
template <class K, class... SurfArgs>
int launch_resize(int B, int H, int W, int oh, int ow, int antialias, const ResizeOut& o, hipStream_t st, const SurfArgs&... surf) {
  // row-streaming form where its windows fit (the development switches of vs_resize_pre apply: form, strip height), the tile form elsewhere
  const int OWsel = vs_rs::rs_pick(H, W, oh, ow, antialias, K::ALIGN);
  if (vs_debug_get(VS_DBG_RESIZE_FORM) != 1 && OWsel) {
    const int cols = (ow + OWsel - 1) / OWsel;
    const int strip = surf_resize_strip(cols, oh, B);
    dim3 gs(cols, (oh + strip - 1) / strip, B);
    const size_t lds = OWsel == 128 ? vs_rs::rs_lds_bytes<128>() : vs_rs::rs_lds_bytes<64>();
    const ResizePreEpi epi{o.dst_rgb, o.dst_key, o.mul, o.add, o.key_step, o.key_mode, o.y0, o.y1, o.y2, oh, ow};
    if ((int64_t)lds <= vs_max_lds_bytes()) {
      if (OWsel == 128) hipLaunchKernelGGL(K::template resize_stream<128>(), gs, dim3(256), lds, st, surf..., H, W, oh, ow, antialias, epi, strip);
      else hipLaunchKernelGGL(K::template resize_stream<64>(), gs, dim3(256), lds, st, surf..., H, W, oh, ow, antialias, epi, strip);
      return vs_launch_status();
    }
  }
  dim3 grid((ow + 31) / 32, (oh + 7) / 8, B);
  hipLaunchKernelGGL(K::resize_tile(), grid, dim3(256), 0, st, surf..., B, H, W, oh, ow, antialias, o.dst_rgb, o.mul, o.add, o.dst_key, o.key_step,
                     o.key_mode, o.y0, o.y1, o.y2);
  return vs_launch_status();
}
template <class K, class Geo>
int launch_tail(const TailArgs& a, const JndTaps& k, const Geo& g, bool stream_form, bool full_jnd, hipStream_t st) {
  if (stream_form) {
    const int strip = tail_strip(full_jnd, a.F, a.H, a.W);
    dim3 gs((a.W + TTW - 1) / TTW, (a.H + strip - 1) / strip, a.F);
    const size_t lds_w = (size_t)2 * a.Cd * DW_W * DW_H * sizeof(float);
    const size_t lds_j = lds_w + RING * TLW * sizeof(float);
    if (full_jnd && a.Cd == 1) hipLaunchKernelGGL((K::template tail_stream<true, 1>()), gs, dim3(256), lds_j, st, a, k, g, strip);
    else if (full_jnd) hipLaunchKernelGGL((K::template tail_stream<true, 3>()), gs, dim3(256), lds_j, st, a, k, g, strip);
    else if (a.Cd == 1) hipLaunchKernelGGL((K::template tail_stream<false, 1>()), gs, dim3(256), lds_w, st, a, k, g, strip);
    else hipLaunchKernelGGL((K::template tail_stream<false, 3>()), gs, dim3(256), lds_w, st, a, k, g, strip);
    return vs_launch_status();
  }
  dim3 grid((a.W + TTW - 1) / TTW, (a.H + TTH - 1) / TTH, a.F);
  hipLaunchKernelGGL(K::tail_tile(), grid, dim3(256), 0, st, a, k, g);
  return vs_launch_status();
}

// The checks of a surface tail descriptor that do not depend on the surface, in the order vs_embed_tail_yuv420 has always applied them
// around its own: tail_desc_numbers first, then the family's size, format and surface checks, then tail_desc_form -- what the tail cannot do,
// the taps, the kernel arguments and the form (row-streaming by default where vs_embed_tail's applies, the 16-row tiles elsewhere and with
// variant = 1).
struct TailForm { TailArgs a; JndTaps k; bool stream_form, full_jnd; };
template <class DESC>
int tail_desc_numbers(const DESC* d) {
  VS_REQUIRE((d->Cd == 1 || d->Cd == 3) && d->step >= 1 && d->total_key >= 1);
  VS_REQUIRE(d->video_mode >= 0 && d->video_mode <= 2);
  return VS_OK;
}
template <class DESC>
int tail_desc_form(const DESC* d, TailForm& t) {
  if (d->preds_w || d->attenuate == 2 || (d->variant != 0 && d->variant != 1 && d->variant != 4)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  t.a = TailArgs{nullptr, nullptr, nullptr, d->delta, d->attenuate ? d->hmap_lowres : nullptr, d->F, d->H, d->W, d->S_h, d->S_w,
                 d->Cd, d->step, d->video_mode, d->total_key, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  t.k = JndTaps{};
  if (d->taps43) t.k = taps_from(d->taps43);
  t.full_jnd = d->attenuate && !d->hmap_lowres;
  const bool can_stream = tail_can_stream(t.full_jnd, d->taps43, d->H, d->W, d->S_h, d->S_w);
  if (d->variant == 4 && !can_stream) return VS_ERR_UNSUPPORTED;
  t.stream_form = d->variant != 1 && can_stream;
  return VS_OK;
}

}  // namespace
