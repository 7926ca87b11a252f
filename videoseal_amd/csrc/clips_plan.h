// Launch plan of the clip-list shell passes (vs_resize_pre_clips, vs_embed_tail_clips): images_plan.h with a frame dimension.  A slot is a run
// of F frames of one size; its workgroups are F x tiles, frame-major (frame f of the slot owns [first_wg + f * tiles, first_wg + (f + 1) * tiles)),
// so neighbouring workgroups share a frame.  The form and the tile counts are those of images_plan.h: one copy of each rule.
// Host code, no HIP dependency, no allocation; vs_clips_plan (clips_plan.hip) copies the groups out, the launchers of shell.hip launch them.
#pragma once
#include "images_plan.h"

// Walk the slots form by form, in list order inside a form, VS_IMAGES_PER_LAUNCH slots per group; emit(group) -> VS_OK to go on.  group.image[k]
// indexes the caller's slots.  The strip of a streaming resize follows vs_images_resize_strip with the group's FRAME count for the batch.
// Arguments are the caller's to check (n >= 0, every F, H, W > 0, oh, ow > 0).  VS_ERR_UNSUPPORTED: a launch would pass 2^31 - 1 workgroups.
template <class Emit>
static inline int vs_clips_walk(const vs_clip_desc_t* clips, int n, int kind, int io_u8, int oh, int ow, int antialias, Emit&& emit) {
  for (int form = VS_IMAGES_FORM_TILE; form <= VS_IMAGES_FORM_STREAM64; ++form) {
    int of_form = 0;
    for (int i = 0; i < n; ++i) of_form += vs_images_form(kind, io_u8, clips[i].H, clips[i].W, oh, ow, antialias) == form;
    int next = 0;
    while (of_form > 0) {
      vs_images_group_t g{};
      g.form = form;
      g.count = of_form < VS_IMAGES_PER_LAUNCH ? of_form : VS_IMAGES_PER_LAUNCH;
      int64_t frames = 0;
      for (int k = 0, i = next; k < g.count; ++i) {
        if (vs_images_form(kind, io_u8, clips[i].H, clips[i].W, oh, ow, antialias) != form) continue;
        g.image[k++] = i;
        frames += clips[i].F;
      }
      next = g.image[g.count - 1] + 1;
      g.strip = (kind == VS_IMAGES_RESIZE && form != VS_IMAGES_FORM_TILE)
                    ? vs_images_resize_strip(form, (int)(frames < INT32_MAX ? frames : INT32_MAX), oh, ow) : 0;
      int64_t wg = 0;
      for (int k = 0; k < g.count; ++k) {
        const vs_clip_desc_t& c = clips[g.image[k]];
        g.first_wg[k] = (int32_t)wg;
        wg += (int64_t)c.F * vs_images_tiles(kind, form, g.strip, c.H, c.W, oh, ow);
        if (wg > INT32_MAX) return VS_ERR_UNSUPPORTED;
      }
      for (int k = g.count; k <= VS_IMAGES_PER_LAUNCH; ++k) g.first_wg[k] = (int32_t)wg;      // [count] = the grid; the rest never matches
      of_form -= g.count;
      if (const int rc = emit(g); rc != VS_OK) return rc;
    }
  }
  return VS_OK;
}
