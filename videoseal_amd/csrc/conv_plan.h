// Shape preconditions of the kernels behind vs_conv_gemm and the tile-code decode: conv_gemm.hip checks arguments with them,
// conv_plan.hip (vs_conv_plan / vs_cnx_stage_plan) and model_api.hip plan launches with them.  Host code, no HIP dependency.
#pragma once
#include "videoseal_hip.h"

static inline int vs_tile_code(int tile_hint) { return (tile_hint & 0xf) + ((tile_hint & VS_CONV_TILE_HI) ? 16 : 0); }
static inline bool vs_tile_is_gemm_pc(int tile) { return tile == 17 || tile == 18 || tile == 26; }

// the GRN rows of a K slice of the wave-specialised 1x1 GEMM are staged in LDS: K elements per slice
#define VS_GRN_SLICE_K 3072

// 3x3 / stride 1 / "same": the patch kernels (input patch staged once per channel chunk) ...
static inline bool vs_conv_same3x3(const vs_conv_desc_t& d) {
  return d.KH == 3 && d.KW == 3 && d.SH == 1 && d.SW == 1 && d.PH == 1 && d.PW == 1 && d.Ho == d.H && d.Wo == d.W;
}
// ... chosen unasked on tile-aligned frames only
static inline bool vs_conv_patch_frames(const vs_conv_desc_t& d) { return d.W % 16 == 0 && d.H % 8 == 0; }
// thin full-resolution layers (16 input channels, <= 32 outputs): persistent kernel with the weights in registers (tile 20)
static inline bool vs_conv_small_shape(const vs_conv_desc_t& d) {
  return d.CinP == 16 && d.N <= 32 && d.n_store <= 32 && (!d.in2 || d.Cin2P == 16) && d.split_k <= 1 && !d.sumsq_part;
}
// wave-specialised 1x1 GEMM (tiles 17 / 18 / 26): dense rows, whole 32-wide K pairs, no second phase; with the GRN transform on its A path
// a 128-row tile touches at most two frames
static inline bool vs_conv_gemm_pc_shape(const vs_conv_desc_t& d) {
  return d.KH == 1 && d.KW == 1 && d.SH == 1 && d.SW == 1 && d.PH == 0 && d.PW == 0 && d.Ho == d.H && d.Wo == d.W && !d.in2 &&
         d.Cin % 32 == 0 && d.CinP == d.Cin && d.in_sy == (int64_t)d.W * d.in_sx && d.in_sb == (int64_t)d.H * d.in_sy &&
         (!d.a_scale || d.H * d.W >= 128 || d.H * d.W == 64);
}
