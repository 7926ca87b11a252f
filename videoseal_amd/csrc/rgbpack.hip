// Packed RGB frames: the instantiations of the packed-pixel kernel family (rgb_surf.h) for its five layouts and the entry points
// vs_resize_pre_rgb / vs_embed_tail_rgb.  Twelve formats (ffmpeg's pix_fmt names without the "le"; everything little-endian):
//   rgb24, bgr24                  uint8   [H][W][3]     R G B / B G R
//   rgba, bgra, argb, abgr        uint8   [H][W][4]     R G B A / B G R A / A R G B / A B G R
//   rgb48, bgr48                  uint16  [H][W][3]     words R G B / B G R
//   rgba64, bgra64                uint16  [H][W][4]     words R G B A / B G R A
//   x2rgb10, x2bgr10              uint32  [H][W]        bits 31-30 X, 29-20 R (B), 19-10 G, 9-0 B (R)
// A format is a layout (bytes per pixel, or the 10:10:10:2 word) and the positions of R, G and B inside the pixel, which travel as kernel
// arguments.  Not here: packed YUV, big-endian words, premultiplied alpha; half-float RGB is halfpix.hip.
#include "rgb_surf.h"

namespace {

using Rgb3 = RgbSurf<3, false>;
using Rgb4 = RgbSurf<4, false>;
using Rgb6 = RgbSurf<6, false>;
using Rgb8 = RgbSurf<8, false>;
using RgbX2 = RgbSurf<4, true>;

// layout 0 .. 4 (3, 4, 6, 8 bytes per pixel, the 10:10:10:2 word) and where R, G, B sit; false: not one of the twelve formats
bool rgb_format(const int fmt, int& layout, int& bpp, RgbPos& pos) {
  switch (fmt) {
    case VS_RGB_RGB24: layout = 0; bpp = 3; pos = RgbPos{0, 1, 2}; return true;
    case VS_RGB_BGR24: layout = 0; bpp = 3; pos = RgbPos{2, 1, 0}; return true;
    case VS_RGB_RGBA: layout = 1; bpp = 4; pos = RgbPos{0, 1, 2}; return true;
    case VS_RGB_BGRA: layout = 1; bpp = 4; pos = RgbPos{2, 1, 0}; return true;
    case VS_RGB_ARGB: layout = 1; bpp = 4; pos = RgbPos{1, 2, 3}; return true;
    case VS_RGB_ABGR: layout = 1; bpp = 4; pos = RgbPos{3, 2, 1}; return true;
    case VS_RGB_RGB48: layout = 2; bpp = 6; pos = RgbPos{0, 1, 2}; return true;
    case VS_RGB_BGR48: layout = 2; bpp = 6; pos = RgbPos{2, 1, 0}; return true;
    case VS_RGB_RGBA64: layout = 3; bpp = 8; pos = RgbPos{0, 1, 2}; return true;
    case VS_RGB_BGRA64: layout = 3; bpp = 8; pos = RgbPos{2, 1, 0}; return true;
    case VS_RGB_X2RGB10: layout = 4; bpp = 4; pos = RgbPos{20, 10, 0}; return true;
    case VS_RGB_X2BGR10: layout = 4; bpp = 4; pos = RgbPos{0, 10, 20}; return true;
    default: return false;
  }
}
// the pitch holds a row, frames do not overlap
bool rgb_surface_ok(const vs_rgb_surface_t& s, int bpp, int F, int H, int W) {
  const int64_t rowb = (int64_t)W * bpp;
  if (s.pitch < rowb) return false;
  return !(F > 1 && s.frame_stride < s.pitch * (H - 1) + rowb);
}
RgbPlane dev_plane(const vs_rgb_surface_t& s) { return RgbPlane{static_cast<const unsigned char*>(s.data), s.pitch, s.frame_stride}; }

// the kernels of one layout, for launch_resize / launch_tail (shell_common.h)
template <class SF>
struct RgbKernels {
  static constexpr int ALIGN = RGB_RS_ALIGN;
  template <int OW> static auto resize_stream() { return resize_pre_rgb_stream_kernel<SF, OW>; }
  static auto resize_tile() { return resize_pre_rgb_kernel<SF>; }
  template <bool JND, int CD> static auto tail_stream() { return embed_tail_rgb_stream_kernel<SF, JND, CD>; }
  static auto tail_tile() { return embed_tail_rgb_kernel<SF>; }
};

}  // namespace

extern "C" int vs_sizeof_rgb_surface(void) { return (int)sizeof(vs_rgb_surface_t); }
extern "C" int vs_sizeof_tail_rgb_desc(void) { return (int)sizeof(vs_tail_rgb_desc_t); }

extern "C" int vs_resize_pre_rgb(const vs_rgb_surface_t* src, int B, int H, int W, int oh, int ow, int antialias, float* dst_rgb, float mul,
                                 float add, float* dst_y, int y_step, const float* ymat3, void* stream) {
  VS_REQUIRE(src && src->data && B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_y));
  VS_REQUIRE(!dst_y || y_step >= 1);
  int layout, bpp;
  RgbPos pos;
  if (!rgb_format(src->format, layout, bpp, pos)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(rgb_surface_ok(*src, bpp, B, H, W));
  const RgbPlane s = dev_plane(*src);
  const ResizeOut o = resize_out(dst_rgb, mul, add, dst_y, y_step, ymat3);
  hipStream_t st = (hipStream_t)stream;
  switch (layout) {
    case 0: return launch_resize<RgbKernels<Rgb3>>(B, H, W, oh, ow, antialias, o, st, s, pos);
    case 1: return launch_resize<RgbKernels<Rgb4>>(B, H, W, oh, ow, antialias, o, st, s, pos);
    case 2: return launch_resize<RgbKernels<Rgb6>>(B, H, W, oh, ow, antialias, o, st, s, pos);
    case 3: return launch_resize<RgbKernels<Rgb8>>(B, H, W, oh, ow, antialias, o, st, s, pos);
    default: return launch_resize<RgbKernels<RgbX2>>(B, H, W, oh, ow, antialias, o, st, s, pos);
  }
}

extern "C" int vs_embed_tail_rgb(const vs_tail_rgb_desc_t* d, void* stream) {
  VS_REQUIRE(d && d->src.data && d->dst.data && d->delta && d->F > 0 && d->H > 0 && d->W > 0 && d->S_h > 0 && d->S_w > 0);
  if (const int rc = tail_desc_numbers(d); rc != VS_OK) return rc;
  VS_REQUIRE(d->clamp == 1);                              // codes are only defined for values in [0, 1]
  VS_REQUIRE(d->dst.data != d->src.data);                 // the JND reads a halo of the source
  int layout, bpp;
  RgbPos pos;
  if (!rgb_format(d->src.format, layout, bpp, pos) || d->dst.format != d->src.format) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(rgb_surface_ok(d->src, bpp, d->F, d->H, d->W) && rgb_surface_ok(d->dst, bpp, d->F, d->H, d->W));
  TailForm t;
  if (const int rc = tail_desc_form(d, t); rc != VS_OK) return rc;
  const RgbGeo g{dev_plane(d->src), dev_plane(d->dst), pos};
  hipStream_t st = (hipStream_t)stream;
  switch (layout) {
    case 0: return launch_tail<RgbKernels<Rgb3>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
    case 1: return launch_tail<RgbKernels<Rgb4>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
    case 2: return launch_tail<RgbKernels<Rgb6>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
    case 3: return launch_tail<RgbKernels<Rgb8>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
    default: return launch_tail<RgbKernels<RgbX2>>(t.a, t.k, g, t.stream_form, t.full_jnd, st);
  }
}
