// 4:2:0 frames as a decoder delivers them: the instantiations of the surface-trait kernel family (yuv_surf.h: resize and tail, each as a tile
// form and a row-streaming form, one body per kernel) for the four 4:2:0 formats, and their entry points.
//   nv12       uint8   Y plane + interleaved CbCr plane           i420       uint8   Y, U, V planes
//   p010       uint16  as nv12, code = word >> 6                  yuv420p10  uint16  as i420, code = min(word, 1023)
// The 4:2:2 and 4:4:4 instantiations and the entry points that take every format (vs_resize_pre_yuv, vs_embed_tail_yuv) are yuv4xx.hip.
// The single-buffer NV12 entry points (vs_resize_pre_nv12, vs_embed_tail_nv12: uint8 [F][3H/2][W], chroma rows under the luma rows at the
// same pitch) are shims at the end of this file: they check their arguments and run the nv12 trait on a two-plane surface.
#include "yuv_surf.h"

namespace {

using SurfNv12 = Surf<false, 8, false>;
using SurfI420 = Surf<true, 8, false>;
using SurfP010 = Surf<false, 10, true>;
using SurfP10 = Surf<true, 10, false>;

}  // namespace

extern "C" int vs_sizeof_yuv420_surface(void) { return (int)sizeof(vs_yuv420_surface_t); }
extern "C" int vs_sizeof_tail_yuv420_desc(void) { return (int)sizeof(vs_tail_yuv420_desc_t); }

extern "C" int vs_resize_pre_yuv420(const vs_yuv420_surface_t* src, int B, int H, int W, const float* yuv2rgb12, int oh, int ow, int antialias,
                                    float* dst_rgb, float mul, float add, float* dst_y, int y_step, const float* ymat3, void* stream) {
  ResizeCall c;
  if (const int rc = prep_resize(src, 1, 1, B, H, W, yuv2rgb12, oh, ow, antialias, dst_rgb, mul, add, dst_y, y_step, ymat3, stream, c); rc != VS_OK)
    return rc;
  switch (c.fmt) {
    case 0: return run_resize<SurfNv12>(c);
    case 1: return run_resize<SurfI420>(c);
    case 2: return run_resize<SurfP010>(c);
    default: return run_resize<SurfP10>(c);
  }
}

extern "C" int vs_embed_tail_yuv420(const vs_tail_yuv420_desc_t* d, void* stream) {
  TailCall c;
  if (const int rc = prep_tail(d, 1, 1, stream, c); rc != VS_OK) return rc;
  switch (c.fmt) {
    case 0: return run_tail<SurfNv12>(c);
    case 1: return run_tail<SurfI420>(c);
    case 2: return run_tail<SurfP010>(c);
    default: return run_tail<SurfP10>(c);
  }
}

// ---- NV12 clips in one buffer: uint8 [F][3H/2][W], the chroma rows under the luma rows at the same pitch.  The entry points check what a
// single buffer asks beyond its two planes (a frame is pitch * (3H/2 - 1) + W bytes: the planes of consecutive frames must not interleave)
// and hand the two-plane surface (vs_nv12_surface) to the entry points above.

extern "C" int vs_sizeof_tail_nv12_desc(void) { return (int)sizeof(vs_tail_nv12_desc_t); }

extern "C" int vs_resize_pre_nv12(const unsigned char* src, int B, int H, int W, int64_t pitch, int64_t frame_stride, const float* yuv2rgb12,
                                  int oh, int ow, int antialias, float* dst_rgb, float mul, float add, float* dst_y, int y_step,
                                  const float* ymat3, void* stream) {
  VS_REQUIRE(src && yuv2rgb12 && B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_y));
  VS_REQUIRE(!(H & 1) && !(W & 1) && pitch >= W && (B == 1 || frame_stride >= pitch * (H / 2 * 3 - 1) + W));
  const vs_yuv420_surface_t s = vs_nv12_surface(src, H, pitch, frame_stride);
  return vs_resize_pre_yuv420(&s, B, H, W, yuv2rgb12, oh, ow, antialias, dst_rgb, mul, add, dst_y, y_step, ymat3, stream);
}

extern "C" int vs_embed_tail_nv12(const vs_tail_nv12_desc_t* d, void* stream) {
  VS_REQUIRE(d && d->imgs && d->out && d->H > 0 && d->W > 0 && !(d->H & 1) && !(d->W & 1));
  const int64_t rows = d->H / 2 * 3;
  VS_REQUIRE(d->src_pitch >= d->W && d->dst_pitch >= d->W);
  VS_REQUIRE(d->F == 1 || (d->src_frame_stride >= d->src_pitch * (rows - 1) + d->W && d->dst_frame_stride >= d->dst_pitch * (rows - 1) + d->W));
  vs_tail_yuv420_desc_t y{};
  y.src = vs_nv12_surface(d->imgs, d->H, d->src_pitch, d->src_frame_stride);
  y.dst = vs_nv12_surface(d->out, d->H, d->dst_pitch, d->dst_frame_stride);
  y.preds_w = d->preds_w; y.delta = d->delta; y.hmap_lowres = d->hmap_lowres; y.taps43 = d->taps43;
  y.F = d->F; y.H = d->H; y.W = d->W; y.S_h = d->S_h; y.S_w = d->S_w; y.Cd = d->Cd;
  y.step = d->step; y.video_mode = d->video_mode; y.total_key = d->total_key;
  y.attenuate = d->attenuate; y.clamp = d->clamp; y.antialias = d->antialias;
  y.scaling_i = d->scaling_i; y.scaling_w = d->scaling_w; y.variant = d->variant;
  for (int i = 0; i < 12; ++i) { y.yuv2rgb12[i] = d->yuv2rgb12[i]; y.rgb2yuv12[i] = d->rgb2yuv12[i]; }
  return vs_embed_tail_yuv420(&y, stream);       // (every remaining check, in the order this entry point has always applied them)
}
