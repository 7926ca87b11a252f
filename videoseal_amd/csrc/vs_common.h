// Internal helpers shared by the HIP translation units of libvideoseal_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "videoseal_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define VS_REQUIRE(cond)                  \
  do {                                    \
    if (!(cond)) return VS_ERR_BAD_ARG;   \
  } while (0)

static inline int vs_launch_status() { return hipGetLastError() == hipSuccess ? VS_OK : VS_ERR_LAUNCH; }

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// an NV12 clip in one buffer (uint8 [F][3H/2][W]: the chroma rows under the luma rows, one pitch, one frame stride) as a two-plane surface
static inline vs_yuv420_surface_t vs_nv12_surface(const void* base, int H, int64_t pitch, int64_t frame_stride) {
  vs_yuv420_surface_t s{};
  unsigned char* p = static_cast<unsigned char*>(const_cast<void*>(base));
  s.plane[0] = p;
  s.plane[1] = p + (int64_t)H * pitch;
  s.pitch[0] = s.pitch[1] = pitch;
  s.frame_stride[0] = s.frame_stride[1] = frame_stride;
  s.depth = 8;
  return s;
}

// Development switches of the launchers: ONE list for the key numbers (VS_DBG_<name>), the names vs_debug_key() answers to and the environment
// defaults.  A launcher asks vs_debug_get(key) and nothing else: the value vs_debug_set gave the key when that is non-zero, else the key's
// environment default, else 0 = the library's own choice.  api.hip reads the environment for the whole list once, at the first vs_debug_get /
// vs_debug_set of the process; no other file of the library reads the environment (not thread-safe against setenv).
//   X(name, variable or nullptr, words, bias, min, meaning)
//   words: "word=value,..." -- the variable's text must equal a word ("word*": start with it); nullptr: value = atoi(text) + bias
//   min:   the smallest value that counts as set; anything below is ignored (VS_DBG_ANY: every non-zero value)
// Keys 0 - 9 keep their numbers (tests and tools of earlier rounds); new keys go at the end.
#define VS_DBG_ANY (-0x7fffffff - 1)
#define VS_DBG_KEYS(X)                                                                                                                              \
  X(RESIZE_FORM, "VIDEOSEAL_RESIZE", "tile=1", 0, 1, "vs_resize_pre(_nv12): 1 = the 32 x 8 tile kernel")                                            \
  X(RESIZE_STRIP, "VS_RESIZE_STRIP", nullptr, 0, 2, "vs_resize_pre(_nv12): strip height in output rows (the variable from 2, the key from 1)")      \
  X(TAIL_STRIP, "VS_TAIL_STRIP", nullptr, 0, 4, "vs_embed_tail(_nv12): strip height in rows, rounded up to 4 (from 4)")                             \
  X(JPEG_FORM, "VIDEOSEAL_JPEG", "scalar=1", 0, 1, "JPEG round trip: 1 = the one-pixel-per-lane kernels")                                           \
  X(CROP_RESIZE_FORM, "VIDEOSEAL_CROP_RESIZE", "tile=1", 0, 1, "Crop -> Resize -> colour: 1 = the 32 x 8 tile kernel")                              \
  X(TO_PLANES_FORM, nullptr, nullptr, 0, 1, "vs_to_planes_affine: 1 = one row per wave")                                                            \
  X(DWCONV_ROWS, "VS_DWCONV_ROWS", nullptr, 0, VS_DBG_ANY, "one-row depthwise kernel: 2 = two output rows per strip, any other value = one")        \
  X(LN_FORM, "VIDEOSEAL_LN", "wave=1", 0, 1, "vs_layernorm_act: 1 = one wave per row")                                                              \
  X(SPLITK_EPI, "VS_SPLITK_EPI", "s*=1", 0, 1, "K-slice epilogue: 1 = the first kernel, one load in flight per thread (VS_SPLITK_EPI=scalar)")      \
  X(UPCONV_FORM, nullptr, nullptr, 0, 1, "vs_upconv_gather_ln and phase 3 of vs_upconv_fused: 1 = per-pixel gather instead of 2 x 2 blocks")        \
  X(TAIL_FORM, "VIDEOSEAL_TAIL", "v1=1,sep=2,keep=3", 0, 1, "vs_embed_tail: the numbers of vs_tail_desc_t::variant (which overrides it per call)")  \
  X(VIT_ATTN, "VS_VIT_ATTN", "valu=1", 0, 1, "vs_vit_attention: 1 = the vector kernel on the matrix-core shapes too")                               \
  X(WGRAD, "VS_WGRAD", "mfma=1,fma=2", 0, 1, "vs_gemm_wgrad: 1 = the fp32 matrix-core kernel, 2 = the fp32 vector kernel, everywhere")              \
  X(DWCONV, "VS_DWCONV", nullptr, 1, 1, "depthwise 7 x 7 + LayerNorm: 1 + configuration (1 = the one-row kernel, 2.. = tiled; VS_DWCONV=0 -> 1)")    \
  X(GEMM_GRID, "VS_GEMM_GRID", nullptr, 0, 1, "wave-specialised 1 x 1 GEMM: workgroups of the persistent grid instead of one per CU")               \
  X(GEMM_PL_RASTER, "VS_GEMM_PL_RASTER", "0*=1", 0, 1, "planes GEMMs: 1 = row-major tile order instead of the XCD-grouped one (the variable: 0)")    \
  X(CNX_PIPE, "VS_CNX_PIPE", nullptr, 1, 1, "fused ConvNeXt block: 1 = the serial cnx_block_kernel (VS_CNX_PIPE=0), any other value = the pipeline") \
  X(CNX_ABL, "VS_CNX_ABL", nullptr, 0, VS_DBG_ANY, "fused ConvNeXt block: ablation bits (builds with VS_CNX_ABLATION only)")                        \
  X(UPCONV_ABL, "VS_UPCONV_ABL", nullptr, 0, VS_DBG_ANY, "vs_upconv_fused: ablation bits")                                                          \
  X(STEM_FUSED, "VIDEOSEAL_STEM_FUSED", "1*=1", 0, 1, "vs_model_detect: 1 = stem conv + LayerNorm in one kernel")                                   \
  X(ARITH, "VIDEOSEAL_CONV", "f16x2=2,bf16x3=3", 0, 2, "default vs_conv_desc_t::arith of the model-level entry points")
#define VS_DBG_ENUM(name, env, words, bias, min, doc) VS_DBG_##name,
enum { VS_DBG_KEYS(VS_DBG_ENUM) VS_DBG_COUNT };
#undef VS_DBG_ENUM
static_assert(VS_DBG_RESIZE_FORM == 0 && VS_DBG_UPCONV_FORM == 9 && VS_DBG_ARITH == 20 && VS_DBG_COUNT == 21, "development switch keys keep their numbers");

// Default arithmetic of the split conv / GEMM path (vs_conv_desc_t::arith): 3 = "3 x bf16" (exact operand split, 6 products),
// 2 = "2 x f16" (round-to-nearest split with power-of-two range scaling, 3 products; conv_common.h).  VIDEOSEAL_CONV=f16x2 | bf16x3
// overrides it for the model-level entry points (the operator level takes it from the descriptor).
#define VS_DEFAULT_ARITH 2
static inline int vs_default_arith() {
  const int a = vs_debug_get(VS_DBG_ARITH);
  return a == 2 || a == 3 ? a : VS_DEFAULT_ARITH;
}

// LDS a workgroup may ask for on the current device (160 KiB on gfx950, 64 KiB on earlier CDNA parts): launchers whose kernels want more than
// 64 KiB check it and fall back to their small-LDS form instead of failing the launch
static inline int vs_max_lds_bytes() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) v = 64 * 1024;
    return v;
  }();
  return n;
}

// compute units of the current device (256 on MI355X): grid size of the persistent kernels
static inline int vs_num_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    return v;
  }();
  return n;
}

// Exact-erf GELU (nn.GELU default, convnext.py:49) in ~16 VALU instructions, branch-free (ocml's erff is two divergent
// branches, ~40 instructions, and made the pwconv1 epilogues VALU-bound):
//   gelu(v) = max(v, 0) - 0.5 |v| erfc(|v|/sqrt2),   erfc(t) = exp(-P(t)),  P(t) = t * Q8(t) fitted to -ln erfc on [0, 4]
// with the 1/sqrt2 and -log2(e) factors folded into the coefficients (tools/micro/fit_gelu.py).  Max |error| vs the exact
// function 2.4e-7 over [-9, 9] -- ATen's own fp32 GELU is off by up to 1.2e-6 there.  Beyond |v| = 5.66 the argument of the fit is clamped, so
// erfc stays at 1.5e-8: v >= 5.66 returns v exactly (the correction is below half an ulp of v), v <= -5.66 returns -7.7e-9 |v|, not 0.
// erfc(a / sqrt2) for a >= 0 (the fitted factor of vs_gelu; shared with its derivative in bwd_ops.hip)
__device__ __forceinline__ float vs_erfc_sqrt2(float a) {
  const float u = fminf(a, 5.65685424949238f);
  float q = 5.128553084e-07f;
  q = __builtin_fmaf(q, u, -9.560153558e-06f);
  q = __builtin_fmaf(q, u, 7.497344632e-05f);
  q = __builtin_fmaf(q, u, -2.843466646e-04f);
  q = __builtin_fmaf(q, u, 1.498938855e-05f);
  q = __builtin_fmaf(q, u, 6.931120995e-03f);
  q = __builtin_fmaf(q, u, -5.243476480e-02f);
  q = __builtin_fmaf(q, u, -4.592214525e-01f);
  q = __builtin_fmaf(q, u, -1.151104212e+00f);
  return __builtin_amdgcn_exp2f(q * u);
}
__device__ __forceinline__ float vs_gelu(float v) {
  const float a = fabsf(v);
  const float e = vs_erfc_sqrt2(a);
  return fmaxf(v, 0.f) - (0.5f * a) * e;
}
// vs_gelu on two values at once (round 6: the GEMM epilogues; the fused ConvNeXt block has had its own copy since round 4): polynomial and blends as
// 2-wide fp32 operations -- v_pk_fma_f32 / v_pk_mul_f32, two results per VALU slot, 23 instead of 40 instructions per pair --, only min / max / exp2
// stay scalar.  Same coefficients and operation order; every multiply-add is an explicit fma with contraction off, which is what hipcc makes of
// vs_gelu's `max - (0.5 a) e` -> the same values bit for bit (tests/test_gpu_kernels.py compares the epilogues that use it with those that do not).
typedef float vs_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ vs_f32x2 vs_gelu2(const vs_f32x2 v) {
#pragma clang fp contract(off)
  const vs_f32x2 a = {fabsf(v[0]), fabsf(v[1])};
  const vs_f32x2 u = {fminf(a[0], 5.65685424949238f), fminf(a[1], 5.65685424949238f)};
  vs_f32x2 q = {5.128553084e-07f, 5.128553084e-07f};
  q = __builtin_elementwise_fma(q, u, vs_f32x2{-9.560153558e-06f, -9.560153558e-06f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{7.497344632e-05f, 7.497344632e-05f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{-2.843466646e-04f, -2.843466646e-04f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{1.498938855e-05f, 1.498938855e-05f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{6.931120995e-03f, 6.931120995e-03f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{-5.243476480e-02f, -5.243476480e-02f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{-4.592214525e-01f, -4.592214525e-01f});
  q = __builtin_elementwise_fma(q, u, vs_f32x2{-1.151104212e+00f, -1.151104212e+00f});
  const vs_f32x2 t = q * u;
  const vs_f32x2 e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
  const vs_f32x2 m = {fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)};
  return __builtin_elementwise_fma(a * -0.5f, e, m);
}
// d gelu / dv = Phi(v) + v phi(v),  Phi(v) = 1 - erfc(v / sqrt2) / 2
__device__ __forceinline__ float vs_gelu_grad(float v) {
  const float e = vs_erfc_sqrt2(fabsf(v));
  const float Phi = v >= 0.f ? 1.f - 0.5f * e : 0.5f * e;
  return Phi + v * (0.3989422804014327f * __expf(-0.5f * v * v));
}

// ReLU that lets NaN through (fmaxf / `v > 0 ? v : 0` turn it into 0): an out-of-range operand of the 2 x f16 arithmetic must surface as
// NaN in the output, not as a silently wrong finite number
__device__ __forceinline__ float vs_relu(float v) { return v <= 0.f ? 0.f : v; }

__device__ __forceinline__ float vs_apply_act(float v, int act) {
  switch (act) {
    case VS_ACT_RELU: return vs_relu(v);
    case VS_ACT_GELU: return vs_gelu(v);
    case VS_ACT_TANH: return tanhf(v);
    case VS_ACT_SILU: return v / (1.0f + __expf(-v));       // nn.SiLU: x * sigmoid(x)
    default: return v;
  }
}

// 64-lane butterfly sum (every lane ends with the total)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
