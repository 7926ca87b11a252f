// Stand-alone walker over the golden launch-plan rows (tests/golden/conv_plan.json, flattened to text by tests/test_conv_plan_cpu.py):
// links csrc/conv_plan.hip alone -- the unit has no GPU dependency -- so that it can run under -fsanitize=address,undefined on any host.
//   input:  "c" 32 descriptor inputs 5 expected outputs | "s" 7 inputs 6 expected outputs, whitespace separated (column order of the JSON)
//   exit 0: every row reproduced; 1: mismatch (printed); 2: malformed input
#include <cstdio>
#include <cstring>

#include "videoseal_hip.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  alignas(16) static float fake[4];      // pointers are flags to the rules: never dereferenced
  long long n = 0, bad = 0, v[37];
  char kind[4];
  while (std::fscanf(f, "%3s", kind) == 1) {
    const int cols = kind[0] == 'c' ? 37 : 13;
    for (int i = 0; i < cols; ++i)
      if (std::fscanf(f, "%lld", &v[i]) != 1) return 2;
    ++n;
    if (kind[0] == 'c') {
      vs_conv_desc_t d;
      std::memset(&d, 0, sizeof(d));
      d.B = (int)v[0]; d.H = (int)v[1]; d.W = (int)v[2]; d.Cin = (int)v[3]; d.KH = (int)v[4]; d.KW = (int)v[5]; d.SH = (int)v[6]; d.SW = (int)v[7];
      d.PH = (int)v[8]; d.PW = (int)v[9]; d.Ho = (int)v[10]; d.Wo = (int)v[11]; d.CinP = (int)v[12]; d.N = (int)v[13]; d.n_store = (int)v[14];
      d.Cin2P = (int)v[15]; d.in_sb = v[16]; d.in_sy = v[17]; d.in_sx = v[18]; d.a_scale_ld = v[19];
      d.a_scale = v[20] ? fake : nullptr; d.in2 = v[21] ? fake : nullptr; d.wt2 = (v[21] || v[26]) ? fake : nullptr;
      d.wt_split = v[22] ? fake : nullptr; d.wt_blk = v[23] ? fake : nullptr; d.wt2_blk = v[24] ? fake : nullptr;
      d.in_pl = v[25] ? fake : nullptr; d.in2_pl = v[26] ? fake : nullptr; d.sumsq_part = v[27] ? fake : nullptr;
      d.tile_hint = (int)v[28]; d.split_k = (int)v[29];
      vs_conv_plan_t p;
      if (vs_conv_plan(&d, (int)v[30], (int)v[31], &p) != VS_OK || p.routes != v[32] || p.split_k != v[33] || p.tile_hint != v[34] ||
          p.ws_slices != v[35] || p.grn_fold != v[36]) {
        std::printf("conv row %lld: got %d %d %d %d %d\n", n, p.routes, p.split_k, p.tile_hint, p.ws_slices, p.grn_fold);
        ++bad;
      }
    } else {
      vs_cnx_stage_plan_t p;
      if (vs_cnx_stage_plan(v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], &p) != VS_OK || p.pl1 != v[7] || p.pl2 != v[8] ||
          p.sk2 != v[9] || p.tile1 != v[10] || p.tile2 != v[11] || p.pw2_narrow != v[12]) {
        std::printf("stage row %lld: got %d %d %d %d %d %d\n", n, p.pl1, p.pl2, p.sk2, p.tile1, p.tile2, p.pw2_narrow);
        ++bad;
      }
    }
  }
  std::fclose(f);
  std::printf("%lld rows, %lld mismatches\n", n, bad);
  return bad ? 1 : (n ? 0 : 2);
}
