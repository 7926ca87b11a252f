/*
 * Half-precision RGB surfaces: the C entry points of libvideoseal_hip.so for float16 / bfloat16 frames, as an image or video generator
 * hands them over.  vs_resize_pre / vs_embed_tail with the decode and the encode fused in: no fp32 frame is written.
 *
 * They live in a header of their own, beside videoseal_hip.h, for the reason include/videoseal_regions.h gives: the suite holds
 * videoseal_hip.h to an export ledger that lists every function it declares.  The functions below are held to the same discipline by
 * tests/test_halfpix_cpu.py (exported by the library, bound in videoseal_amd/native.py, nothing here declared in videoseal_hip.h).  The
 * conventions are those of videoseal_hip.h: device pointers unless said otherwise, `stream` a hipStream_t, VS_OK or a negative VS_ERR_*
 * code, no host synchronisation inside.
 *
 * Layout.  Samples are 16-bit words, little-endian: IEEE binary16 (VS_HALF_FP16) or bfloat16 (VS_HALF_BF16).
 *   VS_HALF_PLANAR   three planes R, G, B of [H][W] samples: plane[i], pitch[i], frame_stride[i] in bytes, each plane on its own.
 *                    components = 3.
 *   VS_HALF_PACKED   [H][W] pixels of `components` = 3 (R G B, 6 bytes) or 4 (R G B A, 8 bytes) samples: plane[0] is the first byte,
 *                    pitch[0] / frame_stride[0] the bytes from a row / a frame to the next; the other entries are ignored.
 *   Any base address and any pitch >= the row's bytes work, odd ones included (a word may sit at an odd address).  Frame bytes move as
 *   16-byte pieces where a piece lies inside its row and its address is aligned, sample by sample elsewhere; bytes between a row's end and
 *   its pitch are neither used nor written.  Frames (and planes) must not overlap.
 * Rules (videoseal_amd/halfpix.py is the executable statement):
 *   Decode: VS_HALF_UNIT   component = float(word)
 *           VS_HALF_SIGNED component = float(word) * 0.5 + 0.5 in fp32 (the product is exact: one rounding).  Not clamped.
 *   Encode: w = clamp(v, 0, 1); the word is round-to-nearest-even of w (unit) or of the fp32 value w * 2 - 1 (signed); results below 2^-14
 *           are fp16 subnormals.  Non-finite samples are outside the contract.
 *   Alpha:  the fourth word of an output pixel is the source pixel's, bit for bit; it never enters arithmetic.
 * Between decode and encode the filter, JND, key-frame and blend expressions and their order are those of the fp32 kernels of the same form:
 * a half clip gives the bits of the fp32 path on its decoded frames.
 * Not here: fp32 surfaces with a value range, planar alpha, big-endian words, premultiplied alpha.
 */
#ifndef VIDEOSEAL_HALF_H
#define VIDEOSEAL_HALF_H

#include "videoseal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VS_HALF_FP16 0
#define VS_HALF_BF16 1
#define VS_HALF_PLANAR 0
#define VS_HALF_PACKED 1
#define VS_HALF_UNIT 0
#define VS_HALF_SIGNED 1

typedef struct vs_half_surface {
  void* plane[3];                           /* planar: R, G, B; packed: plane[0] */
  int64_t pitch[3], frame_stride[3];        /* bytes */
  int32_t elem;                             /* VS_HALF_FP16 | VS_HALF_BF16 */
  int32_t layout;                           /* VS_HALF_PLANAR | VS_HALF_PACKED */
  int32_t components;                       /* 3, or 4 (packed only) */
  int32_t value_range;                      /* VS_HALF_UNIT | VS_HALF_SIGNED */
} vs_half_surface_t;

/* two surfaces, then vs_tail_desc_t's members from preds_w on (as vs_tail_rgb_desc_t) */
typedef struct vs_tail_half_desc {
  vs_half_surface_t src, dst;
  float* preds_w;
  const float* delta; const float* hmap_lowres; const float* taps43;   /* taps43: HOST pointer */
  int32_t F, H, W, S_h, S_w, Cd;
  int32_t step, video_mode, total_key;
  int32_t attenuate, clamp, antialias;
  float scaling_i, scaling_w;
  int32_t io_u8;
  int32_t variant;
} vs_tail_half_desc_t;

int vs_sizeof_half_surface(void);           /* sizeof(vs_half_surface_t) */
int vs_sizeof_tail_half_desc(void);         /* sizeof(vs_tail_half_desc_t) */

/*
 * vs_resize_pre / vs_embed_tail on such surfaces; arguments and forms as vs_resize_pre_rgb / vs_embed_tail_rgb (variant: 0 = row-streaming
 * form where it applies and the tile form elsewhere, 1 = tile form, 4 = row-streaming form).
 * VS_ERR_UNSUPPORTED: an unknown element type, layout or value range, components other than 3 or 4, a planar surface with 4 components,
 *   source and destination of different formats, preds_w != NULL, attenuate = 2, a variant other than 0 / 1 / 4.
 * VS_ERR_BAD_ARG, without a launch: a null pointer, H or W (or any size) below 1, a pitch shorter than its row, overlapping frames,
 *   clamp != 1, a destination that is the source (the JND reads a halo of the source).
 * Development switches: keys 0 - 2, as for vs_resize_pre / vs_embed_tail.
 */
int vs_resize_pre_half(const vs_half_surface_t* src, int B, int H, int W, int oh, int ow, int antialias, float* dst_rgb, float mul, float add,
                       float* dst_y, int y_step, const float* ymat3, void* stream);
int vs_embed_tail_half(const vs_tail_half_desc_t* d, void* stream);

/*
 * The model-level calls (vs_model_embed_rgb / vs_model_detect_rgb of videoseal_hip.h) on half surfaces: `in` and `out` hold the same format
 * and are different buffers; alpha of `out` is `in`'s.  n_msgs is 1 or the number of key frames; step = 1 with n_msgs = frames is image
 * mode (a message per frame).  VS_ERR_UNSUPPORTED: in and out of different formats, and what vs_resize_pre_half / vs_embed_tail_half
 * answer for the surfaces.  VS_ERR_BAD_ARG: a null pointer, non-positive sizes, a model without clamp, out == in, an unaligned workspace.
 */
int vs_model_embed_half(vs_model_t* m, const vs_half_surface_t* in, const vs_half_surface_t* out, const int32_t* msgs, int n_msgs, int frames,
                        int H, int W, int step, int video_mode, int lowres_attenuation, int antialias, void* ws, int64_t ws_bytes, void* stream);
int vs_model_detect_half(vs_model_t* m, const vs_half_surface_t* in, int frames, int H, int W, int antialias, float* logits, void* ws,
                         int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOSEAL_HALF_H */
