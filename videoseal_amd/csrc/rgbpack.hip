// Packed RGB frames: the instantiations of the packed-pixel kernel family (rgb_surf.h) for its five layouts and the entry points
// vs_resize_pre_rgb / vs_embed_tail_rgb.  Twelve formats (ffmpeg's pix_fmt names without the "le"; everything little-endian):
//   rgb24, bgr24                  uint8   [H][W][3]     R G B / B G R
//   rgba, bgra, argb, abgr        uint8   [H][W][4]     R G B A / B G R A / A R G B / A B G R
//   rgb48, bgr48                  uint16  [H][W][3]     words R G B / B G R
//   rgba64, bgra64                uint16  [H][W][4]     words R G B A / B G R A
//   x2rgb10, x2bgr10              uint32  [H][W]        bits 31-30 X, 29-20 R (B), 19-10 G, 9-0 B (R)
// A format is a layout (bytes per pixel, or the 10:10:10:2 word) and the positions of R, G and B inside the pixel, which travel as kernel
// arguments.  Not here: packed YUV, big-endian words, half-float RGB, premultiplied alpha.
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

template <class SF>
int launch_resize_rgb(const RgbPlane& s, const RgbPos& pos, int B, int H, int W, int oh, int ow, int antialias, float* dst_rgb, float mul,
                      float add, float* dst_y, int y_step, int key_mode, float y0, float y1, float y2, hipStream_t st) {
  // row-streaming form where its windows fit (the development switches of vs_resize_pre apply: form, strip height), the tile form elsewhere
  const int OWsel = rgb_rs_pick(H, W, oh, ow, antialias);
  if (vs_debug_get(VS_DBG_RESIZE_FORM) != 1 && OWsel) {
    const int cols = (ow + OWsel - 1) / OWsel;
    int strip = 8;          // (the strip rule of the YUV resize: ~512 workgroups, down to 8 rows for the short launches of detect)
    for (int cand : {64, 48, 32, 24, 16, 12})
      if ((int64_t)cols * ((oh + cand - 1) / cand) * B >= 512) { strip = cand; break; }
    if (const int v = vs_debug_get(VS_DBG_RESIZE_STRIP); v >= 1) strip = v;
    dim3 gs(cols, (oh + strip - 1) / strip, B);
    const size_t lds = OWsel == 128 ? vs_rs::rs_lds_bytes<128>() : vs_rs::rs_lds_bytes<64>();
    const ResizePreEpi epi{dst_rgb, dst_y, mul, add, y_step, key_mode, y0, y1, y2, oh, ow};
    if ((int64_t)lds <= vs_max_lds_bytes()) {
      if (OWsel == 128) hipLaunchKernelGGL((resize_pre_rgb_stream_kernel<SF, 128>), gs, dim3(256), lds, st, s, pos, H, W, oh, ow, antialias, epi, strip);
      else hipLaunchKernelGGL((resize_pre_rgb_stream_kernel<SF, 64>), gs, dim3(256), lds, st, s, pos, H, W, oh, ow, antialias, epi, strip);
      return vs_launch_status();
    }
  }
  dim3 grid((ow + 31) / 32, (oh + 7) / 8, B);
  hipLaunchKernelGGL(resize_pre_rgb_kernel<SF>, grid, dim3(256), 0, st, s, pos, B, H, W, oh, ow, antialias, dst_rgb, mul, add, dst_y, y_step,
                     key_mode, y0, y1, y2);
  return vs_launch_status();
}

template <class SF>
int launch_tail_rgb(const TailArgs& a, const JndTaps& k, const RgbGeo& g, bool stream_form, bool full_jnd, hipStream_t st) {
  if (stream_form) {
    const int strip = tail_strip(full_jnd, a.F, a.H, a.W);
    dim3 gs((a.W + TTW - 1) / TTW, (a.H + strip - 1) / strip, a.F);
    const size_t lds_w = (size_t)2 * a.Cd * DW_W * DW_H * sizeof(float);
    const size_t lds_j = lds_w + RING * TLW * sizeof(float);
    if (full_jnd && a.Cd == 1) hipLaunchKernelGGL((embed_tail_rgb_stream_kernel<SF, true, 1>), gs, dim3(256), lds_j, st, a, k, g, strip);
    else if (full_jnd) hipLaunchKernelGGL((embed_tail_rgb_stream_kernel<SF, true, 3>), gs, dim3(256), lds_j, st, a, k, g, strip);
    else if (a.Cd == 1) hipLaunchKernelGGL((embed_tail_rgb_stream_kernel<SF, false, 1>), gs, dim3(256), lds_w, st, a, k, g, strip);
    else hipLaunchKernelGGL((embed_tail_rgb_stream_kernel<SF, false, 3>), gs, dim3(256), lds_w, st, a, k, g, strip);
    return vs_launch_status();
  }
  dim3 grid((a.W + TTW - 1) / TTW, (a.H + TTH - 1) / TTH, a.F);
  hipLaunchKernelGGL(embed_tail_rgb_kernel<SF>, grid, dim3(256), 0, st, a, k, g);
  return vs_launch_status();
}

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
  const int ks = y_step < 1 ? 1 : y_step, km = ymat3 ? 0 : 1;
  const float y0 = ymat3 ? ymat3[0] : 0.f, y1 = ymat3 ? ymat3[1] : 0.f, y2 = ymat3 ? ymat3[2] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  switch (layout) {
    case 0: return launch_resize_rgb<Rgb3>(s, pos, B, H, W, oh, ow, antialias, dst_rgb, mul, add, dst_y, ks, km, y0, y1, y2, st);
    case 1: return launch_resize_rgb<Rgb4>(s, pos, B, H, W, oh, ow, antialias, dst_rgb, mul, add, dst_y, ks, km, y0, y1, y2, st);
    case 2: return launch_resize_rgb<Rgb6>(s, pos, B, H, W, oh, ow, antialias, dst_rgb, mul, add, dst_y, ks, km, y0, y1, y2, st);
    case 3: return launch_resize_rgb<Rgb8>(s, pos, B, H, W, oh, ow, antialias, dst_rgb, mul, add, dst_y, ks, km, y0, y1, y2, st);
    default: return launch_resize_rgb<RgbX2>(s, pos, B, H, W, oh, ow, antialias, dst_rgb, mul, add, dst_y, ks, km, y0, y1, y2, st);
  }
}

extern "C" int vs_embed_tail_rgb(const vs_tail_rgb_desc_t* d, void* stream) {
  VS_REQUIRE(d && d->src.data && d->dst.data && d->delta && d->F > 0 && d->H > 0 && d->W > 0 && d->S_h > 0 && d->S_w > 0);
  VS_REQUIRE((d->Cd == 1 || d->Cd == 3) && d->step >= 1 && d->total_key >= 1);
  VS_REQUIRE(d->video_mode >= 0 && d->video_mode <= 2);
  VS_REQUIRE(d->clamp == 1);                              // codes are only defined for values in [0, 1]
  VS_REQUIRE(d->dst.data != d->src.data);                 // the JND reads a halo of the source
  int layout, bpp;
  RgbPos pos;
  if (!rgb_format(d->src.format, layout, bpp, pos) || d->dst.format != d->src.format) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(rgb_surface_ok(d->src, bpp, d->F, d->H, d->W) && rgb_surface_ok(d->dst, bpp, d->F, d->H, d->W));
  if (d->preds_w || d->attenuate == 2 || (d->variant != 0 && d->variant != 1 && d->variant != 4)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  const TailArgs a{nullptr, nullptr, nullptr, d->delta, d->attenuate ? d->hmap_lowres : nullptr, d->F, d->H, d->W, d->S_h, d->S_w,
                   d->Cd, d->step, d->video_mode, d->total_key, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  JndTaps k{};
  if (d->taps43) k = taps_from(d->taps43);
  const RgbGeo g{dev_plane(d->src), dev_plane(d->dst), pos};
  // row-streaming form (default) where vs_embed_tail's applies, the 16-row tile form elsewhere and with variant = 1
  const bool full_jnd = d->attenuate && !d->hmap_lowres;
  const bool can_stream = tail_can_stream(full_jnd, d->taps43, d->H, d->W, d->S_h, d->S_w);
  if (d->variant == 4 && !can_stream) return VS_ERR_UNSUPPORTED;
  const bool sf = d->variant != 1 && can_stream;
  hipStream_t st = (hipStream_t)stream;
  switch (layout) {
    case 0: return launch_tail_rgb<Rgb3>(a, k, g, sf, full_jnd, st);
    case 1: return launch_tail_rgb<Rgb4>(a, k, g, sf, full_jnd, st);
    case 2: return launch_tail_rgb<Rgb6>(a, k, g, sf, full_jnd, st);
    case 3: return launch_tail_rgb<Rgb8>(a, k, g, sf, full_jnd, st);
    default: return launch_tail_rgb<RgbX2>(a, k, g, sf, full_jnd, st);
  }
}
