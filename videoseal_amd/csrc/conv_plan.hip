// Which kernel form and how many K slices a dense layer launches with (vs_conv_plan, vs_cnx_stage_plan).  Pure functions of shapes and
// flags -- no GPU call, no environment, no state.  The Python engine and the model-level C host both ask here: whether K is split, and into
// how many slices, fixes the fp32 summation order, so the rules exist once.  Never timing-based for the same reason.
#include <initializer_list>

#include "conv_plan.h"

namespace {
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// K slices for small-M GEMMs: double while 128 x 128 tiles cannot give every CU a workgroup and a slice keeps >= 4 K pairs
// (aiming at 128 / 512 / 1024 workgroups instead of 256 measured slower: detect of 32 frames 4.17 / 3.95 / 4.24 against 3.87 ms, round 4)
int small_m_slices(int64_t rows, int n, int64_t k) {
  const int64_t blocks = cdiv(rows, 128) * cdiv(n, 128);
  const int64_t pairs = k / 32;
  int sk = 1;
  while (blocks * sk < 256 && pairs % (sk * 2) == 0 && pairs / (sk * 2) >= 4) sk *= 2;
  return sk;
}

// K slices (whole 16-channel chunks) for wide 3x3 layers with too few 128-pixel tiles to fill 256 CUs,
// e.g. the 4 key frames of a 16-frame streaming chunk: 32 tiles x 2 = 64 workgroups
int patch_slices(const vs_conv_desc_t& d) {
  if (d.N < 128 || d.CinP < 128) return 1;
  const int64_t blocks = (int64_t)d.B * (d.H / 8) * (d.W / 16) * (d.N % 192 == 0 ? (d.N + 191) / 192 : (d.N + 127) / 128);
  const int spt = d.CinP / 16;
  int sk = 1;
  for (int cand : {2, 3, 4, 6, 8}) {
    if (blocks * sk >= 192) break;
    if (spt % cand == 0 && spt / cand >= 2) sk = cand;
  }
  return sk;
}
}  // namespace

extern "C" int vs_sizeof_conv_plan(void) { return (int)sizeof(vs_conv_plan_t); }
extern "C" int vs_sizeof_cnx_stage_plan(void) { return (int)sizeof(vs_cnx_stage_plan_t); }

extern "C" int vs_conv_plan(const vs_conv_desc_t* dp, int grn_hw, int grn_c4, vs_conv_plan_t* out) {
  if (!dp || !out) return VS_ERR_BAD_ARG;
  const vs_conv_desc_t& d = *dp;
  const bool gemm_pc = d.wt_split && d.wt_blk && vs_conv_gemm_pc_shape(d);
  const bool same3 = d.wt_split && vs_conv_same3x3(d) && !d.a_scale;
  const bool patch = same3 && vs_conv_patch_frames(d);
  const bool patch_pc = patch && d.wt_blk && (!d.in2 || d.wt2_blk);
  const int routes = (gemm_pc ? VS_ROUTE_GEMM_PC : 0) | (patch ? VS_ROUTE_PATCH : 0) | (patch_pc ? VS_ROUTE_PATCH_PC : 0) |
                     (same3 && vs_conv_small_shape(d) ? VS_ROUTE_SMALL : 0);
  int sk = d.sumsq_part ? 1 : d.split_k;       // (the GRN partials of the epilogue have no K-slice form)
  if (sk == 0) {
    sk = 1;
    if (d.tile_hint == 0 && gemm_pc) {
      // the cap applies to the SLICE the rule picks (convnext_base stage 3, K = 4096, runs as two slices of 2048); a slice beyond it leaves the
      // launch unsplit for vs_conv_gemm's generic dispatch
      const int s = small_m_slices((int64_t)d.B * d.H * d.W, d.N, d.CinP);
      if (!d.a_scale || d.CinP / s <= VS_GRN_SLICE_K) sk = s;
    } else if (d.tile_hint == 0 && patch_pc) {
      sk = patch_slices(d);
    }
  }
  *out = {routes, sk, d.tile_hint, 0, 0};
  if (sk > 1) {
    // + the slice of the 1x1 second phase (told by its weights: a host that only counts workspace has no activations yet).  Counted wherever the
    // wave-specialised 3x3 kernel CAN take the launch, not only where it is chosen unasked: a caller that names tile 15 / 16 reaches it on any
    // frame size (vs_conv_gemm's patch_ok has no frame condition), and that kernel always writes slice `split_k` for a second phase.  With the
    // frame-aligned `patch_pc` route alone the count was one slice short on ragged frames and the kernel wrote M * splitk_ld floats past the
    // workspace (found by tests/test_gpu_frame_bias_envelope.py at 24 x 40, 2 K slices)
    const bool pc_named = same3 && d.wt_blk && (!d.in2 || d.wt2_blk);
    out->ws_slices = sk + (((pc_named || d.in_pl) && d.wt2) ? 1 : 0);
    if (d.tile_hint == 0)       // the kernels that implement the K-slice plan
      out->tile_hint = d.KH == 3 ? (d.N % 192 == 0 ? (VS_CONV_TILE_HI | 0) : 15) : (VS_CONV_TILE_HI | (d.N % 192 == 0 ? 2 : 1));
  }
  // GRN's finish (||h|| -> scale) INSIDE the GEMM: the launch is known to run on the wave-specialised kernel, a frame has <= 16 partial rows and
  // K is the partials' channel count.  Same scale values bit for bit as the separate vs_grn_scale_from_partials launch
  out->grn_fold = grn_hw != 0 && vs_tile_is_gemm_pc(vs_tile_code(out->tile_hint)) && grn_hw % 32 == 0 && grn_hw / 32 <= 16 &&
                  d.CinP == grn_c4 && d.a_scale_ld == grn_c4;
  return VS_OK;
}

extern "C" int vs_cnx_stage_plan(int64_t rows, int HW, int C, int h_ld, int pw1_cinp, int arith, int flags, vs_cnx_stage_plan_t* out) {
  if (!out) return VS_ERR_BAD_ARG;
  // all-DMA GEMM on operand planes (gemm_pl.hip, tile code 24): 2 x f16 arithmetic, and where its 256-row x 192-column tiles give every CU work.
  // pwconv1 reads the LayerNorm output as f16 planes written by the dwconv kernel itself; pwconv2 only for long K (K >= 2048: the GRN apply then
  // runs in a separate conversion pass, which costs more than it saves on the shorter layers -- tools/bench_gemm.py planes)
  const bool split2 = !(flags & VS_CNX_NO_SPLIT) && arith == 2, planes = split2 && !(flags & VS_CNX_NO_PLANES_GEMM);
  const int64_t tiles2 = cdiv(rows, 256) * cdiv(C, 192);
  const bool pl1 = planes && cdiv(rows, 256) * cdiv(4 * (int64_t)C, 192) >= 200 && pw1_cinp % 16 == 0;
  int pl2 = 0, sk2 = 1;
  if (planes && h_ld >= 2048 && h_ld % 16 == 0) {
    const int steps2 = h_ld / 16;
    while (tiles2 * sk2 < 200 && steps2 / (sk2 * 2) >= 24 && steps2 % (sk2 * 2) == 0) sk2 *= 2;
    pl2 = tiles2 * sk2 >= 128;
    // round 5: small-M layers (VideoSeal stage 3: 2048 rows x K = 3072) go back to the wave-specialised GEMM with the GRN transform on its A
    // path -- with the producers' lanes all busy it is 50.9 us (4 K slices) against 15.0 (conversion pass over h) + 51.5 us on planes
    // (tools/bench_gemm.py planes); ChunkySeal's wide layers (thousands of rows, K slices beyond the GRN rows' LDS budget) stay
    if (pl2 && rows <= 2048 && HW % 64 == 0 && h_ld % 32 == 0 && !(flags & VS_CNX_NO_PW2_SMALL_PC) &&
        h_ld / small_m_slices(rows, C, h_ld) <= VS_GRN_SLICE_K)
      pl2 = false;
  } else if (planes && h_ld % 16 == 0 && HW % 64 != 0 && tiles2 >= 200) {
    // round 6 (ChunkySeal stages 0 / 1: 127 x 127 and 63 x 63 frames, K = 1448 / 2896 < 2048 at stage 0): frames that do not align with the
    // wave-specialised GEMM's 64-row halves pay a full pass over h anyway (vs_grn_apply in place) and then run the slower kernel -- the planes
    // conversion IS that pass, and the all-DMA GEMM behind it is twice as fast (1.6 -> 0.85 ms per launch at 258 064 x 1448 x 362)
    pl2 = true;
  }
  // round 6: 256 x 256 tiles with one wave per SIMD (tile 27) for the GEMMs with several rounds of 256 x 192 tiles per launch -- those run at the
  // chip's LDS-DMA stream rate, and the larger tile moves 15 % fewer operand bytes per FLOP (ChunkySeal; off unless VS_CNX_GEMM_BIG)
  const bool big = flags & VS_CNX_GEMM_BIG, big1 = big && pl1 && cdiv(rows, 256) * cdiv(4 * (int64_t)C, 256) >= 3 * 256;
  const bool big2 = big && pl2 && sk2 == 1 && cdiv(rows, 256) * cdiv(C, 256) >= 3 * 256;
  // round 5: where 128-row x 128-column tiles would need K slices to occupy the CUs (stage 2: 64 x 3 tiles -> 2 slices + an epilogue launch that
  // adds 25 MB of partial sums), 128 x 96 tiles give 64 x 4 workgroups with the whole K each: one launch (tile 26 takes the whole K in one
  // workgroup: its GRN rows must fit the kernel's LDS area, whole K pairs).  Neutral while the wave-specialised GEMM's producers set its K loop's
  // pace (profiles/r05a / r05c); with their lanes all working in both half steps the kernel alone is 49.9 us against 56.3 + 13
  // (tools/bench_gemm.py ksweep2) and detect of 32 frames 3.725 -> 3.651 ms (median of five alternating runs, profiles/r05o_detect_pw2_tile26.json)
  const bool narrow = !pl2 && HW % 64 == 0 && split2 && !(flags & VS_CNX_NO_PW2_NARROW) && cdiv(rows, 128) * cdiv(C, 128) < 256 &&
                      cdiv(rows, 128) * cdiv(C, 96) >= 200 && C % 96 == 0 && HW >= 128 && h_ld <= VS_GRN_SLICE_K && h_ld % 32 == 0 && h_ld == 4 * C;
  *out = {pl1, pl2, sk2, VS_CONV_TILE_HI | (big1 ? 11 : 8), VS_CONV_TILE_HI | (big2 ? 11 : 8), narrow};
  return VS_OK;
}
