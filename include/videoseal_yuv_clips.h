/*
 * Lists of YUV clips: the clip lists of videoseal_hip.h (vs_resize_pre_clips / vs_embed_tail_clips) on decoder surfaces of the ten formats
 * of vs_yuv_surface_t.  The two full-resolution passes of MANY short clips of different sizes and lengths around ONE network pass, with
 * the colour conversion fused in each way: no RGB or fp32 frame is written, 10-bit clips keep their 10 bits.
 *
 * They live in a header of their own, beside videoseal_hip.h, for the reason include/videoseal_regions.h gives: the suite holds
 * videoseal_hip.h to an export ledger that lists every function it declares, and vs_version() stays as it is.  The functions below are held
 * to the same discipline by tests/test_yuv_clips_cpu.py (exported by the library, bound in videoseal_amd/native.py, nothing here declared
 * in videoseal_hip.h).  The conventions are those of videoseal_hip.h: device pointers unless said otherwise, `stream` a hipStream_t, VS_OK
 * or a negative VS_ERR_* code, no host synchronisation, no device allocation and no host-to-device copy inside.
 *
 * A slot is a run of F consecutive frames of one clip, as in vs_clip_desc_t; its source and (tail) destination are surfaces: up to three
 * plane pointers, pitches and frame strides in bytes, any values the per-clip entry points take.  All slots of a call share one format and
 * one pair of colour affines; sizes and lengths differ.  Descriptors are a HOST array and travel in the kernel arguments, at most
 * VS_YUV_CLIPS_PER_LAUNCH per launch.  The number follows from the 4 KiB of kernel arguments: a slot with two surfaces is 176 bytes, so
 * 16 slots + the prefix table are 2888 bytes; with the tail's arguments (96), the JND taps (172) and the two affines (96) a tail launch
 * carries 3252 bytes (844 to spare), a resize launch at most 3024.  32 slots would need 5704.  A workgroup finds its slot in the prefix table in
 * four halving steps (wave-uniform: scalar loads), then (frame, tile row, tile column) frame-major, as the fp32 clip lists do.
 */
#ifndef VIDEOSEAL_YUV_CLIPS_H
#define VIDEOSEAL_YUV_CLIPS_H

#include "videoseal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VS_YUV_CLIPS_PER_LAUNCH 16

/*   src          the slot's frames; every format rule of vs_yuv_surface_t applies (4:2:0 needs H and W even, 4:2:2 W even)
 *   dst          vs_embed_tail_yuv_clips: the watermarked frames, a surface of src's format.  Ignored by vs_resize_pre_yuv_clips.
 *   first_frame  frame 0 of the slot is frame first_frame of dst_rgb / hmap_lowres
 *   first_key    its first key frame is frame first_key of dst_key / delta */
typedef struct vs_yuv_clip_desc {
  vs_yuv_surface_t src, dst;
  int32_t F, H, W;
  int32_t first_frame;
  int32_t first_key;
} vs_yuv_clip_desc_t;

int vs_sizeof_yuv_clip_desc(void);          /* sizeof(vs_yuv_clip_desc_t) */
int vs_sizeof_tail_yuv_clips_desc(void);    /* sizeof(vs_tail_yuv_clips_desc_t) */
int vs_sizeof_yuv_clips_group(void);        /* sizeof(vs_yuv_clips_group_t) */

/* vs_resize_pre_yuv on every slot: frame f of slot s goes to dst_rgb[first_frame + f] when dst_rgb is given and, when dst_key is given and
 * f % key_step == 0, to dst_key[first_key + f / key_step]; other frames leave dst_key alone and rows no slot owns are not touched.  The
 * bits are those of the per-slot call (every form of the resize computes the same expressions in the same order).  The form is per slot,
 * by the rule of vs_resize_pre_yuv: the row-streaming kernel (128 or 64 output columns) where its windows fit with the format's alignment
 * margin, the 32 x 8 tile kernel elsewhere; slots are grouped form by form and the strip of a streaming group follows its frame count.
 * VS_ERR_BAD_ARG without a launch: a null pointer, n <= 0, oh or ow <= 0, a slot with F, H or W <= 0, a negative first_frame / first_key,
 *   a size the format's chroma rule forbids, a pitch shorter than its row, overlapping frames, both destinations NULL, dst_key with
 *   key_step < 1.
 * VS_ERR_UNSUPPORTED without a launch: a format outside the ten, slots of different formats. */
int vs_resize_pre_yuv_clips(const vs_yuv_clip_desc_t* clips, int n, const float* yuv2rgb12, int oh, int ow, int antialias, float* dst_rgb,
                            float mul, float add, float* dst_key, int key_step, const float* ymat3, void* stream);

/* vs_embed_tail_yuv with variant = 1 (the 256 x 16 tile kernel) on every slot: slot s behaves as that call with F = slot.F,
 * total_key = ceil(F / step), its delta starting at frame first_key of delta [keys][Cd][S_h][S_w] and its hmap_lowres at frame first_frame
 * of hmap_lowres [frames][S_h][S_w]; the other members mean what they mean in vs_tail_yuv_desc_t.  The bytes of dst are those of the
 * per-slot call; bytes between a row's end and its pitch, spare rows and everything outside the planes are never written; src is read only.
 * VS_ERR_BAD_ARG without a launch: what vs_resize_pre_yuv_clips lists for slots and surfaces (src and dst), a null delta, S_h or S_w <= 0,
 *   Cd other than 1 or 3, clamp = 0, step < 1, an unknown video_mode, the full-resolution heat-map (attenuate without hmap_lowres) without taps43.
 * VS_ERR_UNSUPPORTED without a launch: a format outside the ten, slots of different formats, a slot whose src and dst formats differ,
 *   attenuate = 2. */
typedef struct vs_tail_yuv_clips_desc {
  const vs_yuv_clip_desc_t* clips;     /* HOST array of n descriptors */
  const float* delta; const float* hmap_lowres; const float* taps43;   /* taps43: HOST pointer */
  int32_t n, S_h, S_w, Cd;
  int32_t attenuate, clamp, antialias;
  float scaling_i, scaling_w;
  int32_t step, video_mode;
  float yuv2rgb12[12], rgb2yuv12[12];
} vs_tail_yuv_clips_desc_t;
int vs_embed_tail_yuv_clips(const vs_tail_yuv_clips_desc_t* d, void* stream);

/* The plan both launchers walk, as data (a pure host function: no GPU, no allocation; of a descriptor only F, H, W and the format of
 * clips[0].src -- its alignment margin decides the form of a resize -- are read, never a plane pointer).  kind: VS_IMAGES_RESIZE or
 * VS_IMAGES_TAIL; (oh, ow): the processing size.  One group = one launch: slot[k] (k < count) indexes the caller's slots, in list order; the
 * workgroups of slot[k] are F x tiles, contiguous and frame-major, [first_wg[k], first_wg[k + 1]); first_wg[count] is the grid; form is
 * VS_IMAGES_FORM_*; strip: output rows per workgroup of a streaming resize, 0 otherwise.  Groups come form by form.  At most max_groups
 * groups are written (groups may be NULL); *n_groups is the number the list needs.  n = 0 is an empty plan.
 * VS_ERR_UNSUPPORTED past 2^31 - 1 workgroups in a launch, or for a format outside the ten. */
typedef struct vs_yuv_clips_group {
  int32_t form, count, strip, reserved_;
  int32_t slot[VS_YUV_CLIPS_PER_LAUNCH];
  int32_t first_wg[VS_YUV_CLIPS_PER_LAUNCH + 1];
} vs_yuv_clips_group_t;
int vs_yuv_clips_plan(const vs_yuv_clip_desc_t* clips, int n, int kind, int oh, int ow, int antialias, vs_yuv_clips_group_t* groups,
                      int max_groups, int* n_groups);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOSEAL_YUV_CLIPS_H */
