// Stand-alone walker over image-size lists for vs_images_plan: links csrc/images_plan.hip alone -- the unit has no GPU dependency -- so that
// it can run under -fsanitize=address,undefined on any host (tests/test_images_cpu.py writes the lists and checks what is printed).
//   input:  one list per line: kind io_u8 oh ow antialias n  H W  H W ...
//   output: "list <line> groups <g>", then per group "g <form> <strip> <count> | image ... | first_wg ... <grid>"
//   exit 0: every list planned, the count-only call agrees with the full one and nothing is written past max_groups; 1: not so; 2: malformed input
#include <cstdio>
#include <vector>

#include "videoseal_hip.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int kind, u8, oh, ow, aa, n, line = 0, bad = 0;
  while (std::fscanf(f, "%d %d %d %d %d %d", &kind, &u8, &oh, &ow, &aa, &n) == 6) {
    if (n < 0) return 2;
    std::vector<vs_image_desc_t> imgs((size_t)n);        // exactly n descriptors: a read past the list is a heap overflow
    for (int i = 0; i < n; ++i) {
      imgs[(size_t)i] = vs_image_desc_t{};
      if (std::fscanf(f, "%d %d", &imgs[(size_t)i].H, &imgs[(size_t)i].W) != 2) return 2;
    }
    int need = -1, got = -1;
    if (vs_images_plan(n ? imgs.data() : nullptr, n, kind, u8, oh, ow, aa, nullptr, 0, &need) != VS_OK || need < 0) { ++bad; continue; }
    std::vector<vs_images_group_t> groups((size_t)need);      // exactly the groups asked for
    if (vs_images_plan(n ? imgs.data() : nullptr, n, kind, u8, oh, ow, aa, need ? groups.data() : nullptr, need, &got) != VS_OK || got != need) ++bad;
    if (need > 1) {                                            // room for one group only: one is written, the count is still the full one
      std::vector<vs_images_group_t> one(1);
      if (vs_images_plan(imgs.data(), n, kind, u8, oh, ow, aa, one.data(), 1, &got) != VS_OK || got != need || one[0].count != groups[0].count) ++bad;
    }
    std::printf("list %d groups %d\n", line++, need);
    for (const vs_images_group_t& g : groups) {
      std::printf("g %d %d %d |", g.form, g.strip, g.count);
      for (int k = 0; k < g.count; ++k) std::printf(" %d", g.image[k]);
      std::printf(" |");
      for (int k = 0; k <= g.count; ++k) std::printf(" %d", g.first_wg[k]);
      std::printf("\n");
    }
  }
  std::fclose(f);
  std::printf("%d lists, %d failures\n", line, bad);
  return bad ? 1 : 0;
}
