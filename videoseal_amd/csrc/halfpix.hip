// Half-precision RGB frames: the instantiations of the two surface kernel families for the traits of half_surf.h and the entry points
// vs_resize_pre_half / vs_embed_tail_half (include/videoseal_half.h).
//   float16 / bfloat16  x  planar (three planes R, G, B) | packed with 3 or 4 samples per pixel (the fourth is alpha, copied)
//   x  value range unit (stored value = component) | signed (component = stored value * 0.5 + 0.5), a kernel argument.
// Not here: fp32 surfaces with a value range, planar alpha, big-endian words, premultiplied alpha.
#include "half_surf.h"

#include "videoseal_half.h"

namespace {

// known element type, layout, component count and value range?
bool half_format(const vs_half_surface_t& s) {
  if (s.elem != VS_HALF_FP16 && s.elem != VS_HALF_BF16) return false;
  if (s.value_range != VS_HALF_UNIT && s.value_range != VS_HALF_SIGNED) return false;
  if (s.layout == VS_HALF_PLANAR) return s.components == 3;
  if (s.layout == VS_HALF_PACKED) return s.components == 3 || s.components == 4;
  return false;
}
bool same_format(const vs_half_surface_t& a, const vs_half_surface_t& b) {
  return a.elem == b.elem && a.layout == b.layout && a.components == b.components && a.value_range == b.value_range;
}
// planes present, every pitch holds a row, frames of a plane do not overlap
bool half_surface_ok(const vs_half_surface_t& s, int F, int H, int W) {
  const int np = s.layout == VS_HALF_PLANAR ? 3 : 1;
  const int64_t rowb = (int64_t)W * 2 * (s.layout == VS_HALF_PLANAR ? 1 : s.components);
  for (int i = 0; i < np; ++i) {
    if (!s.plane[i] || s.pitch[i] < rowb) return false;
    if (F > 1 && s.frame_stride[i] < s.pitch[i] * (H - 1) + rowb) return false;
  }
  return true;
}
YuvSurf dev_planes(const vs_half_surface_t& s) {
  YuvSurf d{};
  for (int i = 0; i < 3; ++i) {
    d.p[i] = static_cast<const unsigned char*>(s.plane[i]);
    d.pitch[i] = s.pitch[i];
    d.fs[i] = s.frame_stride[i];
  }
  return d;
}
RgbPlane dev_pixels(const vs_half_surface_t& s) { return RgbPlane{static_cast<const unsigned char*>(s.plane[0]), s.pitch[0], s.frame_stride[0]}; }
// the value range in the slot of the family's decode parameters (half_surf.h)
Nv12Mat range_mat(const vs_half_surface_t& s) {
  Nv12Mat m{};
  m.m[0] = s.value_range == VS_HALF_SIGNED ? 1.f : 0.f;
  return m;
}
RgbPos range_pos(const vs_half_surface_t& s) { return RgbPos{s.value_range == VS_HALF_SIGNED ? 1 : 0, 0, 0}; }

// the kernels of one packed trait, for launch_resize / launch_tail (shell_common.h); the planar traits use YuvKernels (yuv_surf.h)
template <class SF>
struct HalfPixelKernels {
  static constexpr int ALIGN = RGB_RS_ALIGN;
  template <int OW> static auto resize_stream() { return resize_pre_rgb_stream_kernel<SF, OW>; }
  static auto resize_tile() { return resize_pre_rgb_kernel<SF>; }
  template <bool JND, int CD> static auto tail_stream() { return embed_tail_rgb_stream_kernel<SF, JND, CD>; }
  static auto tail_tile() { return embed_tail_rgb_kernel<SF>; }
};

}  // namespace

extern "C" int vs_sizeof_half_surface(void) { return (int)sizeof(vs_half_surface_t); }
extern "C" int vs_sizeof_tail_half_desc(void) { return (int)sizeof(vs_tail_half_desc_t); }

extern "C" int vs_resize_pre_half(const vs_half_surface_t* src, int B, int H, int W, int oh, int ow, int antialias, float* dst_rgb, float mul,
                                  float add, float* dst_y, int y_step, const float* ymat3, void* stream) {
  VS_REQUIRE(src && B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_y));
  VS_REQUIRE(!dst_y || y_step >= 1);
  if (!half_format(*src)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(half_surface_ok(*src, B, H, W));
  const ResizeOut o = resize_out(dst_rgb, mul, add, dst_y, y_step, ymat3);
  hipStream_t st = (hipStream_t)stream;
  const bool bf = src->elem == VS_HALF_BF16;
  if (src->layout == VS_HALF_PLANAR) {
    const YuvSurf s = dev_planes(*src);
    const Nv12Mat m = range_mat(*src);
    return bf ? launch_resize<YuvKernels<HalfPlanes<true>>>(B, H, W, oh, ow, antialias, o, st, s, m)
              : launch_resize<YuvKernels<HalfPlanes<false>>>(B, H, W, oh, ow, antialias, o, st, s, m);
  }
  const RgbPlane s = dev_pixels(*src);
  const RgbPos pos = range_pos(*src);
  if (src->components == 3)
    return bf ? launch_resize<HalfPixelKernels<HalfPixels<6, true>>>(B, H, W, oh, ow, antialias, o, st, s, pos)
              : launch_resize<HalfPixelKernels<HalfPixels<6, false>>>(B, H, W, oh, ow, antialias, o, st, s, pos);
  return bf ? launch_resize<HalfPixelKernels<HalfPixels<8, true>>>(B, H, W, oh, ow, antialias, o, st, s, pos)
            : launch_resize<HalfPixelKernels<HalfPixels<8, false>>>(B, H, W, oh, ow, antialias, o, st, s, pos);
}

extern "C" int vs_embed_tail_half(const vs_tail_half_desc_t* d, void* stream) {
  VS_REQUIRE(d && d->delta && d->F > 0 && d->H > 0 && d->W > 0 && d->S_h > 0 && d->S_w > 0);
  if (const int rc = tail_desc_numbers(d); rc != VS_OK) return rc;
  VS_REQUIRE(d->clamp == 1);                              // words are only defined for values in [0, 1]
  if (!half_format(d->src) || !half_format(d->dst) || !same_format(d->src, d->dst)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(half_surface_ok(d->src, d->F, d->H, d->W) && half_surface_ok(d->dst, d->F, d->H, d->W));
  const int np = d->src.layout == VS_HALF_PLANAR ? 3 : 1;
  for (int i = 0; i < np; ++i)
    for (int j = 0; j < np; ++j) VS_REQUIRE(d->dst.plane[i] != d->src.plane[j]);      // the JND reads a halo of the source
  TailForm t;
  if (const int rc = tail_desc_form(d, t); rc != VS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool bf = d->src.elem == VS_HALF_BF16;
  if (d->src.layout == VS_HALF_PLANAR) {
    const YuvGeo g{dev_planes(d->src), dev_planes(d->dst), range_mat(d->src), range_mat(d->src)};
    return bf ? launch_tail<YuvKernels<HalfPlanes<true>>>(t.a, t.k, g, t.stream_form, t.full_jnd, st)
              : launch_tail<YuvKernels<HalfPlanes<false>>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
  }
  const RgbGeo g{dev_pixels(d->src), dev_pixels(d->dst), range_pos(d->src)};
  if (d->src.components == 3)
    return bf ? launch_tail<HalfPixelKernels<HalfPixels<6, true>>>(t.a, t.k, g, t.stream_form, t.full_jnd, st)
              : launch_tail<HalfPixelKernels<HalfPixels<6, false>>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
  return bf ? launch_tail<HalfPixelKernels<HalfPixels<8, true>>>(t.a, t.k, g, t.stream_form, t.full_jnd, st)
            : launch_tail<HalfPixelKernels<HalfPixels<8, false>>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
}
