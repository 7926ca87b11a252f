// vs_clips_plan: the launch plan of vs_resize_pre_clips / vs_embed_tail_clips as data (clips_plan.h holds the rule the launchers walk).
// A pure function of the slots' F, H and W -- no GPU call, no environment, no state, no allocation; pointers of the descriptors are never read.
#include "clips_plan.h"

extern "C" int vs_clips_plan(const vs_clip_desc_t* clips, int n, int kind, int io_u8, int oh, int ow, int antialias, vs_images_group_t* groups,
                             int max_groups, int* n_groups) {
  if (!n_groups || n < 0 || (n > 0 && !clips) || (kind != VS_IMAGES_RESIZE && kind != VS_IMAGES_TAIL) || oh <= 0 || ow <= 0 ||
      (groups && max_groups < 0))
    return VS_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i)
    if (clips[i].F <= 0 || clips[i].H <= 0 || clips[i].W <= 0) return VS_ERR_BAD_ARG;
  int made = 0;
  const int rc = vs_clips_walk(clips, n, kind, io_u8 ? 1 : 0, oh, ow, antialias ? 1 : 0, [&](const vs_images_group_t& g) {
    if (groups && made < max_groups) groups[made] = g;
    ++made;
    return VS_OK;
  });
  *n_groups = made;              // groups == NULL or max_groups too small: the count alone (call again with room for it)
  return rc;
}
