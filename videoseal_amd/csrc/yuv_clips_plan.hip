// vs_yuv_clips_plan: the launch plan of vs_resize_pre_yuv_clips / vs_embed_tail_yuv_clips as data (yuv_clips_plan.h holds the rule the
// launchers walk).  A pure function of the slots' F, H and W and of the format of the first slot's source -- no GPU call, no environment, no
// state, no allocation; plane pointers, pitches and strides are never read.
#include "yuv_clips_plan.h"

extern "C" int vs_sizeof_yuv_clip_desc(void) { return (int)sizeof(vs_yuv_clip_desc_t); }
extern "C" int vs_sizeof_tail_yuv_clips_desc(void) { return (int)sizeof(vs_tail_yuv_clips_desc_t); }
extern "C" int vs_sizeof_yuv_clips_group(void) { return (int)sizeof(vs_yuv_clips_group_t); }

extern "C" int vs_yuv_clips_plan(const vs_yuv_clip_desc_t* clips, int n, int kind, int oh, int ow, int antialias, vs_yuv_clips_group_t* groups,
                                 int max_groups, int* n_groups) {
  if (!n_groups || n < 0 || (n > 0 && !clips) || (kind != VS_IMAGES_RESIZE && kind != VS_IMAGES_TAIL) || oh <= 0 || ow <= 0 ||
      (groups && max_groups < 0))
    return VS_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i)
    if (clips[i].F <= 0 || clips[i].H <= 0 || clips[i].W <= 0) return VS_ERR_BAD_ARG;
  int align = 16, sx, sy;
  if (n > 0) {
    if (!vs_yuv_clips_format(clips[0].src, sx, sy)) return VS_ERR_UNSUPPORTED;
    align = vs_yuv_clips_align(clips[0].src);
  }
  int made = 0;
  const int rc = vs_yuv_clips_walk(clips, n, kind, align, oh, ow, antialias ? 1 : 0, [&](const vs_yuv_clips_group_t& g) {
    if (groups && made < max_groups) groups[made] = g;
    ++made;
    return (int)VS_OK;
  });
  *n_groups = made;              // groups == NULL or max_groups too small: the count alone (call again with room for it)
  return rc;
}
