// Geometry and launch rule of the row-streaming resize (resize_stream.h): which tile shape serves a resize.  Host code, no HIP dependency --
// the launchers of shell.hip / aug.hip and the image-list planner (images_plan.h) ask here.
#pragma once
#include <stddef.h>

namespace vs_rs {

constexpr int RS_GI = 8;                                 // input rows per group
constexpr int RS_WTAB_ROWS = 64;                         // strip rows whose vertical weights are tabulated (taller strips evaluate them per row)
template <int OW_> struct RsGeo;
template <> struct RsGeo<128> { static constexpr int INW = 448, MT = 8, RING = 16; };
template <> struct RsGeo<64> { static constexpr int INW = 288, MT = 10, RING = 32; };
template <int OW> constexpr size_t rs_lds_bytes() {
  return (size_t)(RS_GI * 3 * RsGeo<OW>::INW + RsGeo<OW>::RING * 3 * OW + RS_WTAB_ROWS * (RsGeo<OW>::MT + 2)) * sizeof(float);
}
// which tile shape serves a resize (0: none -- the caller keeps its per-pixel kernel).  margin: columns the loader's window may hold beyond
// the taps' own -- 3 for the fp32 loader (a window start rounded down to a 16-byte vector), the alignment of the window start for the surface
// loaders (16 columns, 32 for half-width planar chroma of 8-bit samples), which take whole pieces
inline int rs_pick(int H, int W, int oh, int ow, int antialias, int margin = 3) {
  const float sx = (float)W / (float)ow, sy = (float)H / (float)oh;
  const float supx = antialias ? (sx >= 1.f ? sx : 1.f) : 1.f, supy = antialias ? (sy >= 1.f ? sy : 1.f) : 1.f;
  auto fits = [&](int OW, int INW, int MT, int RING) {
    return 2.f * supx + 2.f <= (float)MT && 2.f * supy + 2.f <= (float)MT && (float)OW * sx + 2.f * supx + 4.f + (float)margin <= (float)INW &&
           2.f * supy + 2.f + (float)RS_GI <= (float)RING;
  };
  if (fits(128, RsGeo<128>::INW, RsGeo<128>::MT, RsGeo<128>::RING)) return 128;
  if (fits(64, RsGeo<64>::INW, RsGeo<64>::MT, RsGeo<64>::RING)) return 64;
  return 0;
}

}  // namespace vs_rs
