/*
 * Target PSNR for lists: the C entry points of libvideoseal_hip.so that choose the watermark's strength per image of an image list
 * (vs_embed_tail_images) and per frame or per clip of a clip list (vs_embed_tail_clips), on the device.
 *
 * They live in a header of their own, beside videoseal_hip.h, for the reason include/videoseal_regions.h gives -- this is the same
 * arrangement: the suite holds videoseal_hip.h to an export ledger (tests/_ledger.py, tests/test_host.py) that lists every function it
 * declares; the functions below are held to the same discipline by tests/test_lists_psnr_cpu.py (exported by the library, bound in
 * videoseal_amd/native.py as LIST_PSNR_EXPORTS, and nothing here declared in videoseal_hip.h).  The conventions are those of
 * videoseal_hip.h: device pointers unless said otherwise, `stream` a hipStream_t, VS_OK or a negative VS_ERR_* code, no allocation and no
 * host synchronisation inside -- chained on one stream the calls need none.
 *
 * The arithmetic is that of vs_embed_tail_energy / vs_psnr_scale / vs_embed_tail_scaled (videoseal_hip.h, "Embedding to a target PSNR"):
 * with d the perturbation of a pixel at strength 1 (what preds_w receives),
 *   E_i = (3 / Cd) * sum d^2 over item i, float64;   s_i = 10^(-T / 20) * sqrt(n_g / E_g);   out = clamp(scaling_i * img + s_i * d, 0, 1)
 * where an item is an image, or a frame of a clip slot.  The descriptors are those of the fixed-strength list entries, unchanged.
 */
#ifndef VIDEOSEAL_LISTS_PSNR_H
#define VIDEOSEAL_LISTS_PSNR_H

#include "videoseal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Doubles of workspace the energy entries below need for a list: one per workgroup of the VS_IMAGES_TAIL plan of the list (the sum over
 * the plan's groups of first_wg[count]).  Pure host functions: no GPU, no allocation, the pointers of the descriptors are not read.
 * n = 0 gives 0.  -1: a null list with n > 0, n < 0, a non-positive size, a list the plan refuses.
 */
int64_t vs_tail_images_energy_partial_doubles(const vs_image_desc_t* images, int n, int io_u8, int S_h, int S_w, int antialias);
int64_t vs_tail_clips_energy_partial_doubles(const vs_clip_desc_t* clips, int n, int io_u8, int S_h, int S_w, int antialias);

/*
 * energy[i] = E of image i of the list (i: the index in the caller's list), from the expressions of vs_embed_tail_images in its own kernel
 * form; d * d and every sum in float64.  No image is stored: out, preds_w, scaling_w and clamp are ignored, images[i].out may be NULL.
 * Every workgroup of a launch group writes one partial into the group's run of `partials` (sized by the function above, no need to clear
 * it: every slot that is read was written by this call), then ONE finish launch per group adds the partials of each image in a fixed
 * order: no atomics, two runs give the same bits.  Launches: two per group of the plan.
 * Refusals are those of vs_embed_tail_images, before any launch: VS_ERR_BAD_ARG for a null pointer (partials and energy among them),
 * n <= 0, an image with H or W <= 0; VS_ERR_UNSUPPORTED for attenuate other than 0 / 1; a list the plan refuses launches nothing.
 */
int vs_embed_tail_images_energy(const vs_tail_images_desc_t* d, double* partials, double* energy /* DEVICE [n] */, void* stream);

/* vs_embed_tail_images with scaling_w replaced, for image i, by image_scale[i] read from device memory: bit for bit vs_embed_tail_images
 * at scaling_w = image_scale[i] for every image.  Refusals as vs_embed_tail_images, and a null image_scale. */
int vs_embed_tail_images_scaled(const vs_tail_images_desc_t* d, const float* image_scale /* DEVICE [n] */, void* stream);

/*
 * The same for slots of clips (vs_embed_tail_clips).  energy and frame_scale are indexed like hmap_lowres: frame f of a slot is entry
 * first_frame + f; entries that no slot covers are neither read nor written.  n_frames is the length of that array: a slot with
 * first_frame + F > n_frames is VS_ERR_BAD_ARG, decided on the host before any launch.  The other refusals are those of
 * vs_embed_tail_clips (the energy entry ignores out, preds_w, scaling_w and clamp; clips[i].out may be NULL).
 */
int vs_embed_tail_clips_energy(const vs_tail_clips_desc_t* d, double* partials, double* energy /* DEVICE [n_frames] */, int n_frames,
                               void* stream);
int vs_embed_tail_clips_scaled(const vs_tail_clips_desc_t* d, const float* frame_scale /* DEVICE [n_frames] */, int n_frames, void* stream);

/*
 * Strengths of items of different pixel counts: scale[i] = 10^(-target_db / 20) * sqrt(n_g / E_g) in float64, rounded once to fp32, where
 * E_g and n_g are the sums of energy and of elems (3 H W of the item, filled by the caller; DEVICE float64 [n_items]) over the items of
 * i's group, added in index order.  Groups are contiguous runs given by first_item (DEVICE int32 [n_groups + 1], non-decreasing, inside
 * [0, n_items]); first_item == NULL: every item is a group of its own and n_groups is ignored.  E_g == 0 gives 0; max_scale > 0 is a
 * ceiling.  An empty group is legal and writes nothing; an item outside every group is left untouched.
 * VS_ERR_BAD_ARG: a null energy / elems / scale, n_items <= 0, a prefix with n_groups <= 0, a non-finite target_db.
 */
int vs_psnr_scale_items(const double* energy, const double* elems, const int32_t* first_item, int n_items, int n_groups, float target_db,
                        float max_scale /* <= 0: none */, float* scale /* DEVICE [n_items] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOSEAL_LISTS_PSNR_H */
