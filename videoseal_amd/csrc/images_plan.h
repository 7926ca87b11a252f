// Launch plan of the image-list shell passes (vs_resize_pre_images, vs_embed_tail_images): which kernel form serves which image, how the
// images are grouped into launches of at most VS_IMAGES_PER_LAUNCH descriptors and where each image's workgroups start inside a launch.
// Host code, no HIP dependency, no allocation: vs_images_walk hands one finished group at a time to its callback -- vs_images_plan
// (images_plan.hip) copies it out, the launchers of shell.hip launch it.  One copy of the rule, so a test of the plan is a test of the launches.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "resize_pick.h"
#include "videoseal_hip.h"

// tiles of the per-pixel forms (shell.hip holds its kernels to these numbers with a static_assert)
constexpr int VS_IMG_RS_TW = 32, VS_IMG_RS_TH = 8;        // resize_pre tile kernel: 32 x 8 outputs
constexpr int VS_IMG_TAIL_TW = 256, VS_IMG_TAIL_TH = 16;  // embed tail tile kernel: 256 columns x 16 rows of the image

// the form an image takes.  Every form of a pass gives the same bits, so this is a performance choice only.
//   resize: the row-streaming kernel where its windows fit (fp32 planes, scales up to 4), else the 32 x 8 tile kernel (RGB24 always)
//   tail:   the 16-row tile kernel
static inline int vs_images_form(int kind, int io_u8, int H, int W, int oh, int ow, int antialias) {
  if (kind == VS_IMAGES_RESIZE && !io_u8) {
    const int OW = vs_rs::rs_pick(H, W, oh, ow, antialias);
    if (OW) return OW == 128 ? VS_IMAGES_FORM_STREAM128 : VS_IMAGES_FORM_STREAM64;
  }
  return VS_IMAGES_FORM_TILE;
}

// strip height (output rows) of a streaming resize launch over `count` images: the tallest that still gives every CU two workgroups
// (vs_resize_pre's rule with the group's image count for the batch)
static inline int vs_images_resize_strip(int form, int count, int oh, int ow) {
  const int OW = form == VS_IMAGES_FORM_STREAM128 ? 128 : 64;
  const int64_t cols = (ow + OW - 1) / OW;
  for (int cand : {64, 48, 32, 24, 16})
    if (cols * ((oh + cand - 1) / cand) * count >= 512) return cand;
  return 32;
}

// workgroups of one image in a launch of `form` (strip: streaming resize only)
static inline int64_t vs_images_tiles(int kind, int form, int strip, int H, int W, int oh, int ow) {
  if (kind == VS_IMAGES_TAIL) return (int64_t)((W + VS_IMG_TAIL_TW - 1) / VS_IMG_TAIL_TW) * ((H + VS_IMG_TAIL_TH - 1) / VS_IMG_TAIL_TH);
  if (form == VS_IMAGES_FORM_TILE) return (int64_t)((ow + VS_IMG_RS_TW - 1) / VS_IMG_RS_TW) * ((oh + VS_IMG_RS_TH - 1) / VS_IMG_RS_TH);
  const int OW = form == VS_IMAGES_FORM_STREAM128 ? 128 : 64;
  return (int64_t)((ow + OW - 1) / OW) * ((oh + strip - 1) / strip);
}

// Walk the list form by form, in list order inside a form, VS_IMAGES_PER_LAUNCH images per group; emit(group) -> VS_OK to go on.
// The number of groups depends on ceil(images of a form / VS_IMAGES_PER_LAUNCH) summed over the forms present, never on n itself.
// Arguments are the caller's to check (n >= 0, every H, W > 0, oh, ow > 0).  VS_ERR_UNSUPPORTED: a launch would pass 2^31 - 1 workgroups.
template <class Emit>
static inline int vs_images_walk(const vs_image_desc_t* imgs, int n, int kind, int io_u8, int oh, int ow, int antialias, Emit&& emit) {
  for (int form = VS_IMAGES_FORM_TILE; form <= VS_IMAGES_FORM_STREAM64; ++form) {
    int of_form = 0;
    for (int i = 0; i < n; ++i) of_form += vs_images_form(kind, io_u8, imgs[i].H, imgs[i].W, oh, ow, antialias) == form;
    int next = 0;
    while (of_form > 0) {
      vs_images_group_t g{};
      g.form = form;
      g.count = of_form < VS_IMAGES_PER_LAUNCH ? of_form : VS_IMAGES_PER_LAUNCH;
      g.strip = (kind == VS_IMAGES_RESIZE && form != VS_IMAGES_FORM_TILE) ? vs_images_resize_strip(form, g.count, oh, ow) : 0;
      int64_t wg = 0;
      for (int k = 0; k < g.count; ++next) {
        if (vs_images_form(kind, io_u8, imgs[next].H, imgs[next].W, oh, ow, antialias) != form) continue;
        g.image[k] = next;
        g.first_wg[k] = (int32_t)wg;
        wg += vs_images_tiles(kind, form, g.strip, imgs[next].H, imgs[next].W, oh, ow);
        if (wg > INT32_MAX) return VS_ERR_UNSUPPORTED;
        ++k;
      }
      for (int k = g.count; k <= VS_IMAGES_PER_LAUNCH; ++k) g.first_wg[k] = (int32_t)wg;      // [count] = the grid; the rest never matches
      of_form -= g.count;
      if (const int rc = emit(g); rc != VS_OK) return rc;
    }
  }
  return VS_OK;
}
