// The key-frame expansion of vs_embed_tail, written once for the four surface tails (YUV: yuv_surf.h, packed RGB: rgb_surf.h, each as a
// 16-row tile form and a row-streaming form): which two key frames a frame's watermark comes from, with which weights, and the frame's
// low-resolution heat-map.  It runs once per workgroup, ahead of every loop.
// Second spellings, to be changed together with this one: embed_tail_tile and embed_tail_stream_kernel of shell.hip (fp32 / uint8) and
// tail_key_reduce_kernel of bwd_shell.hip (which needs the indices and weights, not the plane pointers).
// The other phases of the tail (tap tables, window staging, JND accumulators, jump test, blend) stay written out in every kernel: as shared
// inlined functions they gave the same bits, but hipcc scheduled the bodies differently and kernels of every family measured slower -- the
// fp32 row-streaming tail with the full-resolution heat-map 141 -> 177 us at 32 x 768^2, the yuv422p one 248 -> 258 us, tile forms 1.4 - 3 %
// (profiles/shell_phases_ab.md).  The surface tests and tests/test_gpu_shell_digests.py hold the spellings to each other and to recorded bits.
#pragma once
#include "shell_common.h"

namespace {

// ---- key-frame expansion (videoseal.py:80-118): the watermark of frame f is wa * key[ka] + wb * key[kb]
struct KeyMix {
  const float* dka; const float* dkb;      // first plane of the two key frames' plane sets
  const float* hml;                        // frame f of the low-resolution heat-map, or null
  float wa, wb;
};
template <class Args>
__device__ __forceinline__ KeyMix key_mix(const Args& a, const int f, const int Cd) {
  int ka = 0, kb = 0;
  float wa = 1.f, wb = 0.f;
  if (a.video_mode == VS_VIDEO_REPEAT) {
    ka = f / a.step;
  } else if (a.video_mode == VS_VIDEO_ALTERNATE) {
    ka = f / a.step;
    wa = (f % a.step) == 0 ? 1.f : 0.f;
  } else {
    const int ninter = ((a.F - 1) / a.step) * a.step;
    if (f < ninter) {
      ka = f / a.step; kb = ka + 1;
      const int j = f % a.step;
      const float lin = a.step > 1 ? (float)j / (float)(a.step - 1) : 0.f;
      wa = 1.f - lin; wb = 1.f - wa;
    } else {
      ka = a.total_key - 1;
    }
  }
  if (ka >= a.total_key) ka = a.total_key - 1;
  if (kb >= a.total_key) kb = a.total_key - 1;
  const int splane = a.Sh * a.Sw;
  return KeyMix{a.delta + (int64_t)ka * Cd * splane, a.delta + (int64_t)kb * Cd * splane,
                a.hmap_lowres ? a.hmap_lowres + (int64_t)f * splane : nullptr, wa, wb};
}

}  // namespace
