// model_tables_test -- csrc/model_tables.hpp (the host arithmetic of problem creation) for the comparison with the
// oracle's tables.  CPU only: includes nothing but that header and links nothing of the library
// (tests/test_model_tables_cpu.py).  Reads cases on stdin (numbers in any form strtod takes: the test sends float.hex())
// and prints one result line per case, integers in decimal and doubles with %a:
//   wt W H dx dy    ->  X[W] Y[H]
//   mw W H dx dy    ->  refusal ox oy ntaps fx w[4] len(ytab) ytab[]
//   nm src dst      ->  map[dst]
//   gk b sigma      ->  k1[b] k2[b*b]
//   mr W H s        ->  0 | 1, with the LR size and the two decimation maps derived as srmap_problem_create derives them
#include <cstdio>
#include <cstring>
#include <vector>

#include "model_tables.hpp"

using namespace srmap;

static void ints(const std::vector<int>& v) {
  for (int x : v) std::printf(" %d", x);
}

int main() {
  char what[8];
  while (std::scanf("%7s", what) == 1) {
    if (std::strcmp(what, "wt") == 0 || std::strcmp(what, "mw") == 0) {
      int W = 0, H = 0;
      double dx = 0, dy = 0;
      if (std::scanf("%d %d %lf %lf", &W, &H, &dx, &dy) != 4 || W < 1 || H < 1) return 2;
      if (what[0] == 'w') {
        std::vector<int> X, Y;
        warp_tables(W, H, dx, dy, &X, &Y);
        ints(X);
        ints(Y);
      } else {
        WarpTable t;
        const int refusal = (int)make_warp(W, H, dx, dy, &t);
        std::printf("%d %d %d %d %d %a %a %a %a %d", refusal, t.ox, t.oy, t.ntaps, t.fx, t.w[0], t.w[1], t.w[2], t.w[3], (int)t.ytab.size());
        ints(t.ytab);
      }
    } else if (std::strcmp(what, "nm") == 0) {
      int src = 0, dst = 0;
      if (std::scanf("%d %d", &src, &dst) != 2 || src < 1 || dst < 1) return 2;
      std::vector<int> map;
      nearest_map(src, dst, &map);
      ints(map);
    } else if (std::strcmp(what, "gk") == 0) {
      int b = 0;
      double sigma = 0;
      if (std::scanf("%d %lf", &b, &sigma) != 2 || b < 1) return 2;
      std::vector<double> k1, k2;
      gaussian_kernel(b, sigma, &k1, &k2);
      for (double v : k1) std::printf(" %a", v);
      for (double v : k2) std::printf(" %a", v);
    } else if (std::strcmp(what, "mr") == 0) {
      int W = 0, H = 0, s = 0;
      if (std::scanf("%d %d %d", &W, &H, &s) != 3 || W < 1 || H < 1 || s < 1) return 2;
      const double scale_factor = 1.0 / (double)s;
      const int w = (int)(W * scale_factor), h = (int)(H * scale_factor);
      if (w < 1 || h < 1) return 2;
      std::vector<int> cmap, rmap;
      nearest_map(W, w, &cmap);
      nearest_map(H, h, &rmap);
      std::printf("%d", maps_regular(W, H, w, h, s, cmap, rmap) ? 1 : 0);
    } else {
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
