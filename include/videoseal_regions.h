/*
 * Region-wise watermarks: the C entry points of libvideoseal_hip.so that tie a message to a region of a frame.
 *
 * They live in a header of their own, beside videoseal_hip.h, because the suite holds videoseal_hip.h to an export ledger
 * (tests/_ledger.py, tests/test_unet_contract_cpu.py::test_every_export_is_in_the_ledger) that lists every function it declares; the
 * functions below are held to the same discipline by tests/test_regions_cpu.py (exported by the library, bound in videoseal_amd/native.py,
 * named in tests/test_gpu_regions.py, and nothing here declared in videoseal_hip.h).  Folding both headers and both lists into one is a
 * follow-up.  The conventions are those of videoseal_hip.h: device pointers unless said otherwise, `stream` a hipStream_t, VS_OK or a
 * negative VS_ERR_* code, no host synchronisation inside.
 *
 * A label map is uint8 [F][H][W], contiguous: 0 is background, r in 1 .. R selects message r - 1, a value above R counts as background.
 * R <= VS_REGIONS_MAX.  Regions are disjoint by construction; fractional masks are not covered.
 */
#ifndef VIDEOSEAL_REGIONS_H
#define VIDEOSEAL_REGIONS_H

#include "videoseal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VS_REGIONS_MAX 8

/*
 * vs_embed_tail with a label per pixel.  d->delta is [total_key * R][Cd][S_h][S_w]: the planes of (key frame k, label r) are set
 * k * R + r - 1.  A pixel of label r > 0 receives what vs_embed_tail computes for it with the plane sets of label r as delta -- the same
 * expressions in the same order (key-frame expansion, heat-map of d->imgs, scaling_i / scaling_w, clamp), bit for bit.  A pixel of label 0
 * is d->imgs bit for bit: uint8 frames copy the byte, fp32 values outside [0, 1] are not clamped.  d->preds_w, when given, receives the
 * selected planes' up-sampled value, and 0 on background.  A 16 x 256 tile whose pixels are all background does not read delta.
 * Forms: the 16-row tiles with the 43-tap (variant 1; uint8 frames always) or the separable stencils (variant 2).  The row-streaming form is
 * not built for this entry point: variant 0 and 4 take the separable tiles, whose bits are the streaming form's.  variant 3 and
 * attenuate = 2 answer VS_ERR_UNSUPPORTED.  VS_ERR_BAD_ARG without a launch: labels == NULL, R < 1, R > VS_REGIONS_MAX and whatever
 * vs_embed_tail_scaled refuses (a null frame or delta pointer, non-positive sizes, Cd outside {1, 3}, uint8 frames without clamp, ...).
 */
int vs_embed_tail_regions(const vs_tail_desc_t* d, const uint8_t* labels, int R, void* stream);

/*
 * Pixel vote of all R regions in one pass over preds [B][K][S_h * S_w] (`batch_stride` floats between frames, as vs_pixel_vote takes it).
 * The labels stay at frame resolution, [B][H][W]: map pixel (y, x) reads labels[b][((2 y + 1) H) / (2 S_h)][((2 x + 1) W) / (2 S_w)]
 * in integer arithmetic (the centre of the map pixel; the identity when the sizes agree).  No resized label map is stored.
 *   votes int32  [B][R][K] : pixels of the region with preds > threshold
 *   nsel  int32  [B][R]    : pixels of the region
 *   sums  double [B][R][K] : sum of the logits over the region
 * Every value of preds is read once whatever R is.  No atomics: a workgroup writes its partial counts and sums (float64) into `partial`
 * (vs_pixel_vote_regions_partial_doubles(B, K, S_h * S_w, R) doubles, no need to clear them) and a second launch adds them in a fixed
 * order, so two runs give the same bits.  VS_ERR_BAD_ARG: a null pointer, non-positive sizes, R outside 1 .. VS_REGIONS_MAX,
 * S_h * S_w past 2^31 - 1.
 */
int64_t vs_pixel_vote_regions_partial_doubles(int B, int K, int64_t HW, int R);
int vs_pixel_vote_regions(const float* preds, int64_t batch_stride, const uint8_t* labels, int B, int K, int S_h, int S_w, int H, int W, int R,
                          float threshold, int32_t* votes, int32_t* nsel, double* sums, double* partial, void* stream);

/*
 * Bounding boxes of the labels: boxes int32 [F][R][4] = (y0, x0, y1, x1) with exclusive ends, (0, 0, 0, 0) for a label without a pixel.
 * VS_ERR_BAD_ARG: a null pointer, non-positive sizes, R outside 1 .. VS_REGIONS_MAX.
 */
int vs_label_boxes(const uint8_t* labels, int F, int H, int W, int R, int32_t* boxes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOSEAL_REGIONS_H */
