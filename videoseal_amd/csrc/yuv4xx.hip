// 4:2:2 and 4:4:4 frames: the instantiations of the surface-trait kernel family (yuv_surf.h) for the six formats beside the 4:2:0 ones, in a
// translation unit of their own (the build stays parallel), and the entry points that take every format.
//   yuv422p    uint8   Y [H][W], U, V [H][W/2]                     yuv422p10  uint16  as yuv422p, code = min(word, 1023)
//   nv16       uint8   Y [H][W], interleaved CbCr [H][W]            p210       uint16  as nv16, code = word >> 6
//   yuv444p    uint8   Y, U, V [H][W]                               yuv444p10  uint16  as yuv444p, code = min(word, 1023)
// 4:2:2 needs W even, 4:4:4 takes any size.  Not here: packed formats (yuyv422, uyvy422, v210), semi-planar 4:4:4 (nv24, p410), depth 12.
// chroma = 420 goes to vs_resize_pre_yuv420 / vs_embed_tail_yuv420 (yuv420.hip): the same launches, the same bits.
#include "yuv_surf.h"

#include <cstring>

namespace {

using SurfNv16 = Surf<false, 8, false, 1, 0>;
using Surf422p = Surf<true, 8, false, 1, 0>;
using SurfP210 = Surf<false, 10, true, 1, 0>;
using Surf422p10 = Surf<true, 10, false, 1, 0>;
using Surf444p = Surf<true, 8, false, 0, 0>;
using Surf444p10 = Surf<true, 10, false, 0, 0>;

static_assert(sizeof(vs_yuv_surface_t) == sizeof(vs_yuv420_surface_t) && sizeof(vs_tail_yuv_desc_t) == sizeof(vs_tail_yuv420_desc_t),
              "a surface of any chroma format is the 4:2:0 surface with `chroma` in its reserved member");

// one of the ten formats?  sx, sy: its chroma shifts
bool format_known(const vs_yuv_surface_t& s, int& sx, int& sy) {
  if ((s.planar != 0 && s.planar != 1) || surface_format(s) < 0) return false;
  if (s.chroma == 420) { sx = 1; sy = 1; return true; }
  if (s.chroma == 422) { sx = 1; sy = 0; return true; }
  if (s.chroma == 444 && s.planar == 1) { sx = 0; sy = 0; return true; }
  return false;
}
vs_yuv420_surface_t as_yuv420(const vs_yuv_surface_t& s) {
  vs_yuv420_surface_t r;
  std::memcpy(&r, &s, sizeof(r));
  r.reserved_ = 0;
  return r;
}

}  // namespace

extern "C" int vs_sizeof_yuv_surface(void) { return (int)sizeof(vs_yuv_surface_t); }
extern "C" int vs_sizeof_tail_yuv_desc(void) { return (int)sizeof(vs_tail_yuv_desc_t); }

extern "C" int vs_resize_pre_yuv(const vs_yuv_surface_t* src, int B, int H, int W, const float* yuv2rgb12, int oh, int ow, int antialias,
                                 float* dst_rgb, float mul, float add, float* dst_y, int y_step, const float* ymat3, void* stream) {
  VS_REQUIRE(src);
  int sx, sy;
  if (!format_known(*src, sx, sy)) return VS_ERR_UNSUPPORTED;
  if (src->chroma == 420) {
    const vs_yuv420_surface_t s = as_yuv420(*src);
    return vs_resize_pre_yuv420(&s, B, H, W, yuv2rgb12, oh, ow, antialias, dst_rgb, mul, add, dst_y, y_step, ymat3, stream);
  }
  ResizeCall c;
  if (const int rc = prep_resize(src, sx, sy, B, H, W, yuv2rgb12, oh, ow, antialias, dst_rgb, mul, add, dst_y, y_step, ymat3, stream, c); rc != VS_OK)
    return rc;
  if (src->chroma == 444) return c.fmt == 1 ? run_resize<Surf444p>(c) : run_resize<Surf444p10>(c);
  switch (c.fmt) {
    case 0: return run_resize<SurfNv16>(c);
    case 1: return run_resize<Surf422p>(c);
    case 2: return run_resize<SurfP210>(c);
    default: return run_resize<Surf422p10>(c);
  }
}

extern "C" int vs_embed_tail_yuv(const vs_tail_yuv_desc_t* d, void* stream) {
  VS_REQUIRE(d);
  int sx, sy, dx, dy;
  if (!format_known(d->src, sx, sy) || !format_known(d->dst, dx, dy) || d->src.chroma != d->dst.chroma) return VS_ERR_UNSUPPORTED;
  if (d->src.chroma == 420) {
    vs_tail_yuv420_desc_t y;
    std::memcpy(&y, d, sizeof(y));
    y.src.reserved_ = y.dst.reserved_ = 0;
    return vs_embed_tail_yuv420(&y, stream);
  }
  TailCall c;
  if (const int rc = prep_tail(d, sx, sy, stream, c); rc != VS_OK) return rc;
  if (d->src.chroma == 444) return c.fmt == 1 ? run_tail<Surf444p>(c) : run_tail<Surf444p10>(c);
  switch (c.fmt) {
    case 0: return run_tail<SurfNv16>(c);
    case 1: return run_tail<Surf422p>(c);
    case 2: return run_tail<SurfP210>(c);
    default: return run_tail<Surf422p10>(c);
  }
}
