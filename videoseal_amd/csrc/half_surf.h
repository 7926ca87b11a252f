// Half-precision RGB frames as a generator's decoder hands them over: float16 / bfloat16 samples in [0, 1] ("unit") or [-1, 1] ("signed"),
// planar or packed.  No kernel body of its own: the two surface families already have one body per form, and a half surface is a trait of
// theirs with a floating-point sample codec in place of the integer one.
//   trait               kernels of                 geometry
//   HalfPlanes<BF>      yuv_surf.h (4:4:4 planar)  three planes R, G, B of 16-bit samples, 8 per 16-byte piece; the codec (HalfPlaneCodec)
//                                                  replaces code -> colour matrix -> clamp on the way in and matrix -> rounding on the way out
//   HalfPixels<6, BF>   rgb_surf.h (RgbSurf<6, 0>) pixels of 3 samples, straddling pieces staged through LDS
//   HalfPixels<8, BF>   rgb_surf.h (RgbSurf<8, 0>) pixels of 4 samples; the fourth (alpha) word is copied
// BF selects bfloat16; the value range is a kernel ARGUMENT: it rides in the slot the family uses for its own decode parameters (the colour
// affines of the YUV kernels: m[0] != 0 means signed; the component positions of the packed kernels: RgbPos::r != 0 means signed -- the
// samples of a half pixel are always R, G, B in memory order).  Six traits, two value ranges each.
// Decode: v = float(word) (unit) or fma(float(word), 0.5, 0.5) (signed; the product is exact, so this is the one rounding of
// `x.float() * 0.5 + 0.5`); not clamped.  Encode: w = the kernels' clamp to [0, 1]; the word is RNE(w) or RNE(fma(w, 2, -1)).
// Conversions: fp16 <-> fp32 are the hardware converts (v_cvt_f32_f16 / v_cvt_f16_f32, round-to-nearest-even, subnormals kept: the
// default fp16 denormal mode of a HIP kernel); bf16 -> fp32 is a 16-bit shift; fp32 -> bf16 is the conversion of clang's __bf16, which
// gfx950 has as one instruction (v_cvt_pk_bf16_f32, round-to-nearest-even, ties as tensor.to(torch.bfloat16)).
// Between decode and encode everything is the families' own text: a half clip gives the bits of the fp32 path on its decoded frames.
#pragma once
#include "rgb_surf.h"
#include "yuv_surf.h"

namespace {

template <bool BF>
struct HalfWord {
  static __device__ __forceinline__ float dec(const unsigned raw) {            // the low 16 bits of `raw` -> fp32, exact
    if (BF) return __builtin_bit_cast(float, raw << 16);
    return (float)__builtin_bit_cast(_Float16, (unsigned short)raw);
  }
  static __device__ __forceinline__ unsigned enc(const float v) {              // fp32 -> the 16-bit word, round-to-nearest-even
    if (BF) return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v);
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v);
  }
  static __device__ __forceinline__ float comp(const unsigned raw, const bool sgn) {      // stored word -> component
    const float y = dec(raw);
    return sgn ? __builtin_fmaf(y, 0.5f, 0.5f) : y;
  }
  static __device__ __forceinline__ unsigned word(const float w, const bool sgn) {        // component in [0, 1] -> stored word
    return enc(sgn ? __builtin_fmaf(w, 2.f, -1.f) : w);
  }
};

// ---- planar: the codec of Surf<true, 16, false, 0, 0, .>.  A "code" is the stored VALUE (val: word -> fp32, exact); the colour affine's
// slot carries the value range (m[0]); `aff` returns the stored value of component r, which the 4:4:4 kernels hand to word() unchanged
// (their chroma sum over a 1 x 1 block is 0.f + value).
template <bool BF>
struct HalfPlaneCodec {
  static constexpr int BPS = 2;
  using S = unsigned short;
  static __device__ __forceinline__ float val(const unsigned raw) { return HalfWord<BF>::dec(raw); }
  static __device__ __forceinline__ S word(const float v) { return (S)HalfWord<BF>::enc(v); }
  static __device__ __forceinline__ void rgb(const Nv12Mat& k, const float y, const float cb, const float cr, float (&out)[3]) {
    const bool sgn = k.m[0] != 0.f;
    out[0] = sgn ? __builtin_fmaf(y, 0.5f, 0.5f) : y;
    out[1] = sgn ? __builtin_fmaf(cb, 0.5f, 0.5f) : cb;
    out[2] = sgn ? __builtin_fmaf(cr, 0.5f, 0.5f) : cr;
  }
  static __device__ __forceinline__ float aff(const Nv12Mat& k, const int r, const float a, const float b, const float c) {
    const float w = r == 0 ? a : (r == 1 ? b : c);
    return k.m[0] != 0.f ? __builtin_fmaf(w, 2.f, -1.f) : w;
  }
};
template <bool BF>
using HalfPlanes = Surf<true, 16, false, 0, 0, HalfPlaneCodec<BF>>;

// ---- packed: RgbSurf<6 | 8, 0>'s piece machinery with a float decode / encode in place of unit() and floor(v * top)
template <int BPP_, bool BF>
struct HalfPixels : RgbSurf<BPP_, false> {
  static_assert(BPP_ == 6 || BPP_ == 8, "3 or 4 samples of 16 bits");
  static __device__ __forceinline__ void decode(const Raw x, const RgbPos& pos, float (&rgb)[3]) {
    const bool sgn = pos.r != 0;
    rgb[0] = HalfWord<BF>::comp(x.w0 & 0xffffu, sgn);
    rgb[1] = HalfWord<BF>::comp(x.w0 >> 16, sgn);
    rgb[2] = HalfWord<BF>::comp(x.w1 & 0xffffu, sgn);
  }
  // the source pixel with R, G, B replaced (v already clamped to [0, 1]); the alpha word is the source's
  static __device__ __forceinline__ Raw encode(const Raw x, const RgbPos& pos, const float (&v)[3]) {
    const bool sgn = pos.r != 0;
    const unsigned r = HalfWord<BF>::word(v[0], sgn), g = HalfWord<BF>::word(v[1], sgn), b = HalfWord<BF>::word(v[2], sgn);
    return Raw{r | (g << 16), (x.w1 & 0xffff0000u) | b};
  }
};

}  // namespace
