// Launch plan of the YUV clip-list shell passes (vs_resize_pre_yuv_clips, vs_embed_tail_yuv_clips): clips_plan.h for surface slots.  What
// differs: a launch holds VS_YUV_CLIPS_PER_LAUNCH slots (a slot carries two surfaces: videoseal_yuv_clips.h derives the number), and the form
// of a resize is the one launch_resize<YuvKernels<SF>> (shell_common.h) picks per clip: rs_pick with the trait's alignment margin.  The tile
// counts and the strip rule are those of images_plan.h: one copy of each.
// Host code, no HIP dependency, no allocation; vs_yuv_clips_plan (yuv_clips_plan.hip) copies the groups out, the launchers of yuv_clips.hip
// launch them.
#pragma once
#include "images_plan.h"
#include "videoseal_yuv_clips.h"

// the chroma shifts of one of the ten formats; false: no such format  (second spelling: format_known of yuv4xx.hip)
static inline bool vs_yuv_clips_format(const vs_yuv_surface_t& s, int& sx, int& sy) {
  if (s.planar != 0 && s.planar != 1) return false;
  const bool d8 = s.depth == 8 && !s.msb_aligned, d10 = s.depth == 10 && (s.planar ? !s.msb_aligned : s.msb_aligned == 1);
  if (!d8 && !d10) return false;
  if (s.chroma == 420) { sx = 1; sy = 1; return true; }
  if (s.chroma == 422) { sx = 1; sy = 0; return true; }
  if (s.chroma == 444 && s.planar == 1) { sx = 0; sy = 0; return true; }
  return false;
}
static inline bool vs_yuv_clips_same_format(const vs_yuv_surface_t& a, const vs_yuv_surface_t& b) {
  return a.planar == b.planar && a.depth == b.depth && a.msb_aligned == b.msb_aligned && a.chroma == b.chroma;
}
// window start of the row-streaming resize, in columns: max(16, Surf::CW) of yuv_surf.h (yuv_clips.hip holds the two together with a
// static_assert per trait) -- 32 for half-width planar chroma of 8-bit samples (i420, yuv422p), 16 elsewhere
constexpr int vs_yuv_clips_align_of(bool planar, int depth, int chroma) { return (planar && chroma != 444 && depth == 8) ? 32 : 16; }
static inline int vs_yuv_clips_align(const vs_yuv_surface_t& s) { return vs_yuv_clips_align_of(s.planar != 0, s.depth, s.chroma); }

static inline int vs_yuv_clips_form(int kind, int align, int H, int W, int oh, int ow, int antialias) {
  if (kind == VS_IMAGES_RESIZE) {
    const int OW = vs_rs::rs_pick(H, W, oh, ow, antialias, align);
    if (OW) return OW == 128 ? VS_IMAGES_FORM_STREAM128 : VS_IMAGES_FORM_STREAM64;
  }
  return VS_IMAGES_FORM_TILE;
}

// Walk the slots form by form, in list order inside a form, VS_YUV_CLIPS_PER_LAUNCH slots per group; emit(group) -> VS_OK to go on.
// The strip of a streaming resize follows vs_images_resize_strip with the group's FRAME count for the batch, as vs_clips_walk does.
// Arguments are the caller's to check (n >= 0, every F, H, W > 0, oh, ow > 0).  VS_ERR_UNSUPPORTED: a launch would pass 2^31 - 1 workgroups.
template <class Emit>
static inline int vs_yuv_clips_walk(const vs_yuv_clip_desc_t* clips, int n, int kind, int align, int oh, int ow, int antialias, Emit&& emit) {
  for (int form = VS_IMAGES_FORM_TILE; form <= VS_IMAGES_FORM_STREAM64; ++form) {
    int of_form = 0;
    for (int i = 0; i < n; ++i) of_form += vs_yuv_clips_form(kind, align, clips[i].H, clips[i].W, oh, ow, antialias) == form;
    int next = 0;
    while (of_form > 0) {
      vs_yuv_clips_group_t g{};
      g.form = form;
      g.count = of_form < VS_YUV_CLIPS_PER_LAUNCH ? of_form : VS_YUV_CLIPS_PER_LAUNCH;
      int64_t frames = 0;
      for (int k = 0, i = next; k < g.count; ++i) {
        if (vs_yuv_clips_form(kind, align, clips[i].H, clips[i].W, oh, ow, antialias) != form) continue;
        g.slot[k++] = i;
        frames += clips[i].F;
      }
      next = g.slot[g.count - 1] + 1;
      g.strip = (kind == VS_IMAGES_RESIZE && form != VS_IMAGES_FORM_TILE)
                    ? vs_images_resize_strip(form, (int)(frames < INT32_MAX ? frames : INT32_MAX), oh, ow) : 0;
      int64_t wg = 0;
      for (int k = 0; k < g.count; ++k) {
        const vs_yuv_clip_desc_t& c = clips[g.slot[k]];
        g.first_wg[k] = (int32_t)wg;
        wg += (int64_t)c.F * vs_images_tiles(kind, form, g.strip, c.H, c.W, oh, ow);
        if (wg > INT32_MAX) return VS_ERR_UNSUPPORTED;
      }
      for (int k = g.count; k <= VS_YUV_CLIPS_PER_LAUNCH; ++k) g.first_wg[k] = (int32_t)wg;      // [count] = the grid; the rest never matches
      of_form -= g.count;
      if (const int rc = emit(g); rc != VS_OK) return rc;
    }
  }
  return VS_OK;
}
