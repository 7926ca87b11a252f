// Stand-alone walker over slot lists for vs_yuv_clips_plan: links csrc/yuv_clips_plan.hip alone -- the unit has no GPU dependency -- so that
// it can run under -fsanitize=address,undefined on any host (tests/test_yuv_clips_cpu.py writes the lists and checks what is printed).
//   input:  one list per line: kind planar depth msb chroma oh ow antialias n  F H W  F H W ...
//   output: "list <line> groups <g>", then per group "g <form> <strip> <count> | slot ... | first_wg ... <grid>"
//   exit 0: every list planned, the count-only call agrees with the full one and nothing is written past max_groups; 1: not so; 2: malformed input
#include <cstdio>
#include <vector>

#include "videoseal_yuv_clips.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int kind, planar, depth, msb, chroma, oh, ow, aa, n, line = 0, bad = 0;
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d %d", &kind, &planar, &depth, &msb, &chroma, &oh, &ow, &aa, &n) == 9) {
    if (n < 0) return 2;
    std::vector<vs_yuv_clip_desc_t> clips((size_t)n);        // exactly n descriptors: a read past the list is a heap overflow
    for (int i = 0; i < n; ++i) {
      vs_yuv_clip_desc_t& c = clips[(size_t)i];
      c = vs_yuv_clip_desc_t{};
      c.src.planar = planar; c.src.depth = depth; c.src.msb_aligned = msb; c.src.chroma = chroma;
      if (std::fscanf(f, "%d %d %d", &c.F, &c.H, &c.W) != 3) return 2;
    }
    int need = -1, got = -1;
    if (vs_yuv_clips_plan(n ? clips.data() : nullptr, n, kind, oh, ow, aa, nullptr, 0, &need) != VS_OK || need < 0) { ++bad; continue; }
    std::vector<vs_yuv_clips_group_t> groups((size_t)need);      // exactly the groups asked for
    if (vs_yuv_clips_plan(n ? clips.data() : nullptr, n, kind, oh, ow, aa, need ? groups.data() : nullptr, need, &got) != VS_OK || got != need) ++bad;
    if (need > 1) {                                               // room for one group only: one is written, the count is still the full one
      std::vector<vs_yuv_clips_group_t> one(1);
      if (vs_yuv_clips_plan(clips.data(), n, kind, oh, ow, aa, one.data(), 1, &got) != VS_OK || got != need || one[0].count != groups[0].count) ++bad;
    }
    std::printf("list %d groups %d\n", line++, need);
    for (const vs_yuv_clips_group_t& g : groups) {
      std::printf("g %d %d %d |", g.form, g.strip, g.count);
      for (int k = 0; k < g.count; ++k) std::printf(" %d", g.slot[k]);
      std::printf(" |");
      for (int k = 0; k <= g.count; ++k) std::printf(" %d", g.first_wg[k]);
      std::printf("\n");
    }
  }
  std::fclose(f);
  std::printf("%d lists, %d failures\n", line, bad);
  return bad ? 1 : 0;
}
