// Lists of YUV clips (include/videoseal_yuv_clips.h): the list instantiations of the surface-trait kernels of yuv_surf.h -- the 32 x 8 resize
// tile, the row-streaming resize (128 / 64 output columns) and the 256 x 16 tail tile, for all ten traits -- in a translation unit of their
// own (the build stays parallel), and the two launchers.  The bodies are the grid kernels'; only the prologue differs (yuv_surf.h, "Where a
// workgroup works").  The row-streaming tail has no list form, as for the fp32 lists.  The launchers walk vs_yuv_clips_walk
// (yuv_clips_plan.h): no device allocation, no copy, no synchronisation.
#include "yuv_surf.h"
#include "yuv_clips_plan.h"

namespace {

static_assert(YUV_CLIPS == VS_YUV_CLIPS_PER_LAUNCH && YUV_CLIPS == 16, "yuv_at: four halving steps");
// the 4 KiB of kernel arguments: 2888 + 96 (affines) + 96 + 172 = 3252 for the tail, 844 to spare; the resize kernels carry the descriptors, one
// affine, the epilogue (or its members) and at most 32 bytes of scalars: 3024, 1072 to spare
static_assert(sizeof(YuvClipSlot) == 176 && sizeof(YuvClipsArgs) == 2888, "a slot with two surfaces");
static_assert(sizeof(YuvClipsGeo) + sizeof(TailArgs) + sizeof(JndTaps) <= 4096 - 844, "descriptors + tail arguments + JND taps + two affines fit the kernel arguments");
static_assert(sizeof(YuvClipsArgs) + sizeof(Nv12Mat) + sizeof(ResizePreEpi) + 32 <= 4096 - 1072, "descriptors + one affine + resize epilogue fit the kernel arguments");

using SurfNv12 = Surf<false, 8, false>;
using SurfI420 = Surf<true, 8, false>;
using SurfP010 = Surf<false, 10, true>;
using SurfP10 = Surf<true, 10, false>;
using SurfNv16 = Surf<false, 8, false, 1, 0>;
using Surf422p = Surf<true, 8, false, 1, 0>;
using SurfP210 = Surf<false, 10, true, 1, 0>;
using Surf422p10 = Surf<true, 10, false, 1, 0>;
using Surf444p = Surf<true, 8, false, 0, 0>;
using Surf444p10 = Surf<true, 10, false, 0, 0>;

template <class SF> constexpr bool align_agrees() {
  return yuv_rs_align<SF>() == vs_yuv_clips_align_of(SF::PLANAR, SF::DEPTH, SF::SX ? (SF::SY ? 420 : 422) : 444);
}
static_assert(align_agrees<SurfNv12>() && align_agrees<SurfI420>() && align_agrees<SurfP010>() && align_agrees<SurfP10>() && align_agrees<SurfNv16>() &&
              align_agrees<Surf422p>() && align_agrees<SurfP210>() && align_agrees<Surf422p10>() && align_agrees<Surf444p>() && align_agrees<Surf444p10>(),
              "yuv_clips_plan.h picks the resize form with the trait's window alignment");

// f(trait) for the trait of a surface format_known accepted
template <class Fn>
int with_trait(const vs_yuv_surface_t& s, Fn&& f) {
  const int fmt = surface_format(s);
  if (s.chroma == 420) {
    switch (fmt) {
      case 0: return f(SurfNv12{});
      case 1: return f(SurfI420{});
      case 2: return f(SurfP010{});
      default: return f(SurfP10{});
    }
  }
  if (s.chroma == 444) return fmt == 1 ? f(Surf444p{}) : f(Surf444p10{});
  switch (fmt) {
    case 0: return f(SurfNv16{});
    case 1: return f(Surf422p{});
    case 2: return f(SurfP210{});
    default: return f(Surf422p10{});
  }
}

// the checks of the slots, before any launch; sx, sy: the chroma shifts of the list's format
int check_slots(const vs_yuv_clip_desc_t* clips, int n, bool with_dst, int& sx, int& sy) {
  for (int i = 0; i < n; ++i)
    VS_REQUIRE(clips[i].F > 0 && clips[i].H > 0 && clips[i].W > 0 && clips[i].first_frame >= 0 && clips[i].first_key >= 0);
  if (!vs_yuv_clips_format(clips[0].src, sx, sy)) return VS_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) {
    if (!vs_yuv_clips_same_format(clips[i].src, clips[0].src)) return VS_ERR_UNSUPPORTED;
    if (with_dst && !vs_yuv_clips_same_format(clips[i].dst, clips[i].src)) return VS_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < n; ++i) {
    const vs_yuv_clip_desc_t& c = clips[i];
    VS_REQUIRE(!(c.H & ((1 << sy) - 1)) && !(c.W & ((1 << sx) - 1)));
    VS_REQUIRE(surface_ok(c.src, sx, sy, c.F, c.H, c.W) && (!with_dst || surface_ok(c.dst, sx, sy, c.F, c.H, c.W)));
  }
  return VS_OK;
}

// kernel arguments of one group of the plan
YuvClipsArgs clips_args(const vs_yuv_clip_desc_t* clips, const vs_yuv_clips_group_t& grp, const int kind, const int oh, const int ow) {
  YuvClipsArgs g{};
  for (int k = 0; k <= YUV_CLIPS; ++k) g.first_wg[k] = grp.first_wg[k];
  for (int k = 0; k < grp.count; ++k) {
    const vs_yuv_clip_desc_t& d = clips[grp.slot[k]];
    int cols = (d.W + TTW - 1) / TTW;
    if (kind == VS_IMAGES_RESIZE) {
      const int tw = grp.form == VS_IMAGES_FORM_TILE ? VS_IMG_RS_TW : (grp.form == VS_IMAGES_FORM_STREAM128 ? 128 : 64);
      cols = (ow + tw - 1) / tw;
    }
    g.slot[k] = YuvClipSlot{dev_surface(d.src), kind == VS_IMAGES_TAIL ? dev_surface(d.dst) : YuvSurf{}, d.F, d.H, d.W, d.first_frame, d.first_key,
                            cols, (int)vs_images_tiles(kind, grp.form, grp.strip, d.H, d.W, oh, ow), 0};
  }
  return g;
}

}  // namespace

extern "C" int vs_resize_pre_yuv_clips(const vs_yuv_clip_desc_t* clips, int n, const float* yuv2rgb12, int oh, int ow, int antialias,
                                       float* dst_rgb, float mul, float add, float* dst_key, int key_step, const float* ymat3, void* stream) {
  VS_REQUIRE(clips && n > 0 && yuv2rgb12 && oh > 0 && ow > 0 && (dst_rgb || dst_key));
  VS_REQUIRE(!dst_key || key_step >= 1);
  int sx, sy;
  if (const int rc = check_slots(clips, n, false, sx, sy); rc != VS_OK) return rc;
  const int align = vs_yuv_clips_align(clips[0].src), aa = antialias ? 1 : 0;
  int n_groups = 0;      // a dry walk first: a list the plan refuses launches nothing
  if (const int rc = vs_yuv_clips_plan(clips, n, VS_IMAGES_RESIZE, oh, ow, aa, nullptr, 0, &n_groups); rc != VS_OK) return rc;
  if ((int64_t)vs_rs::rs_lds_bytes<128>() > vs_max_lds_bytes() || (int64_t)vs_rs::rs_lds_bytes<64>() > vs_max_lds_bytes()) return VS_ERR_UNSUPPORTED;
  const ResizeOut o = resize_out(dst_rgb, mul, add, dst_key, key_step, ymat3);
  const ResizePreEpi epi{o.dst_rgb, o.dst_key, o.mul, o.add, o.key_step, o.key_mode, o.y0, o.y1, o.y2, oh, ow};
  Nv12Mat dec;
  for (int i = 0; i < 12; ++i) dec.m[i] = yuv2rgb12[i];
  const hipStream_t st = (hipStream_t)stream;
  return with_trait(clips[0].src, [&](auto sf) {
    using SF = decltype(sf);
    return vs_yuv_clips_walk(clips, n, VS_IMAGES_RESIZE, align, oh, ow, aa, [&](const vs_yuv_clips_group_t& grp) {
      const YuvClipsArgs g = clips_args(clips, grp, VS_IMAGES_RESIZE, oh, ow);
      const dim3 grid((unsigned)grp.first_wg[grp.count]);
      if (grp.form == VS_IMAGES_FORM_STREAM128)
        hipLaunchKernelGGL((resize_pre_yuv_stream_kernel<SF, 128, YuvClipsArgs>), grid, dim3(256), vs_rs::rs_lds_bytes<128>(), st, g, dec, 0, 0, oh, ow, aa,
                           epi, grp.strip);
      else if (grp.form == VS_IMAGES_FORM_STREAM64)
        hipLaunchKernelGGL((resize_pre_yuv_stream_kernel<SF, 64, YuvClipsArgs>), grid, dim3(256), vs_rs::rs_lds_bytes<64>(), st, g, dec, 0, 0, oh, ow, aa,
                           epi, grp.strip);
      else
        hipLaunchKernelGGL((resize_pre_yuv_kernel<SF, YuvClipsArgs>), grid, dim3(256), 0, st, g, dec, 0, 0, 0, oh, ow, aa, o.dst_rgb, o.mul, o.add,
                           o.dst_key, o.key_step, o.key_mode, o.y0, o.y1, o.y2);
      return vs_launch_status();
    });
  });
}

extern "C" int vs_embed_tail_yuv_clips(const vs_tail_yuv_clips_desc_t* d, void* stream) {
  VS_REQUIRE(d && d->clips && d->n > 0 && d->delta && d->S_h > 0 && d->S_w > 0 && (d->Cd == 1 || d->Cd == 3));
  VS_REQUIRE(d->step >= 1 && d->video_mode >= 0 && d->video_mode <= 2 && d->clamp);        // codes are only defined for values in [0, 1]
  int sx, sy;
  if (const int rc = check_slots(d->clips, d->n, true, sx, sy); rc != VS_OK) return rc;
  if (d->attenuate != 0 && d->attenuate != 1) return VS_ERR_UNSUPPORTED;      // (2: the training forward's order, single clips only)
  VS_REQUIRE(!(d->attenuate && !d->hmap_lowres) || d->taps43);
  const int aa = d->antialias ? 1 : 0;
  int n_groups = 0;
  if (const int rc = vs_yuv_clips_plan(d->clips, d->n, VS_IMAGES_TAIL, d->S_h, d->S_w, aa, nullptr, 0, &n_groups); rc != VS_OK) return rc;
  // F, H, W, total_key and the first frames of delta / hmap_lowres are the slot's (set per workgroup)
  const TailArgs a{nullptr, nullptr, nullptr, d->delta, d->attenuate ? d->hmap_lowres : nullptr, 0, 0, 0, d->S_h, d->S_w, d->Cd, d->step,
                   d->video_mode, 0, d->attenuate, d->clamp, d->antialias, d->scaling_i, d->scaling_w};
  JndTaps k{};
  if (d->taps43) k = taps_from(d->taps43);
  const hipStream_t st = (hipStream_t)stream;
  return with_trait(d->clips[0].src, [&](auto sf) {
    using SF = decltype(sf);
    return vs_yuv_clips_walk(d->clips, d->n, VS_IMAGES_TAIL, 16, d->S_h, d->S_w, aa, [&](const vs_yuv_clips_group_t& grp) {
      YuvClipsGeo g{clips_args(d->clips, grp, VS_IMAGES_TAIL, d->S_h, d->S_w), {}, {}};
      for (int i = 0; i < 12; ++i) { g.dec.m[i] = d->yuv2rgb12[i]; g.enc.m[i] = d->rgb2yuv12[i]; }
      hipLaunchKernelGGL((embed_tail_yuv_kernel<SF, YuvClipsGeo>), dim3((unsigned)grp.first_wg[grp.count]), dim3(256), 0, st, a, k, g);
      return vs_launch_status();
    });
  });
}
