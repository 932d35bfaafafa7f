// solver_host_test -- csrc/solver_host.hpp (the More'-Thuente step, the L-BFGS recursion on coefficients and the unpacking
// of the update pass's rows) for the bit-for-bit comparison with tests/lbfgs_restatement.py, and the polling decision of
// csrc/solver_mailbox.hpp on plain host memory.  CPU only: includes nothing but those headers and links nothing of the
// library (tests/test_solver_host_cpu.py).  Reads cases on stdin, numbers in any form strtod takes (the test sends
// float.hex()), and prints one result line per case with %a:
//   mt stx fx dx sty fy dy stp fp dp brackt stmin stmax     ->  stx fx dx sty fy dy stp brackt info
//   tl m k q SY[m*m] YY[m*m] gs[m] gy[m] rho[m]             ->  "none" when s_p.y_p or y_p.y_p is 0, else
//                                                               rho[p] coef[0 .. 2 (q + 1)]
//   up m p live SY[m*m] YY[m*m] gs[m] gy[m] r[lb_rows(live)]   ->  SY[m*m] YY[m*m] gs[m] gy[m] after lbfgs_unpack_rows
//   pt slot timeout_word want budget_seconds                   ->  arrived | timeout | expired
#include <cstdio>
#include <cstring>
#include <vector>

#include "solver_host.hpp"

using namespace srmap;

static bool number(double* v) { return std::scanf("%lf", v) == 1; }

static bool numbers(std::vector<double>& v) {
  for (double& x : v)
    if (!number(&x)) return false;
  return true;
}

int main() {
  char what[8];
  while (std::scanf("%7s", what) == 1) {
    if (std::strcmp(what, "mt") == 0) {
      std::vector<double> a(12);
      if (!numbers(a)) return 2;
      Bracket b = {a[0], a[1], a[2], a[3], a[4], a[5]};
      double stp = a[6];
      bool brackt = a[9] != 0.0;
      int info = -1;
      mt_step(&b, &stp, a[7], a[8], &brackt, a[10], a[11], &info);
      std::printf("%a %a %a %a %a %a %a %d %d\n", b.stx, b.fx, b.dx, b.sty, b.fy, b.dy, stp, brackt ? 1 : 0, info);
    } else if (std::strcmp(what, "tl") == 0) {
      int m = 0, k = 0, q = 0;
      if (std::scanf("%d %d %d", &m, &k, &q) != 3 || m < 1 || k < 0 || q < 0 || q >= m) return 2;
      std::vector<double> SY((size_t)m * m), YY((size_t)m * m), gs(m), gy(m), rho(m), coef(1 + 2 * m, 0.0);
      if (!numbers(SY) || !numbers(YY) || !numbers(gs) || !numbers(gy) || !numbers(rho)) return 2;
      if (!lbfgs_two_loop(SY.data(), YY.data(), gs.data(), gy.data(), rho.data(), k, q, m, coef.data())) {
        std::printf("none\n");
        continue;
      }
      std::printf("%a", rho[k % m]);
      for (int i = 0; i < 1 + 2 * (q + 1); ++i) std::printf(" %a", coef[i]);
      std::printf("\n");
    } else if (std::strcmp(what, "up") == 0) {
      int m = 0, p = 0, live = 0;
      if (std::scanf("%d %d %d", &m, &p, &live) != 3 || m < 1 || m > kLbfgsMaxM || p < 0 || p >= m || live < 1 || live > m) return 2;
      std::vector<double> SY((size_t)m * m), YY((size_t)m * m), gs(m), gy(m), r(lb_rows(live));
      if (!numbers(SY) || !numbers(YY) || !numbers(gs) || !numbers(gy) || !numbers(r)) return 2;
      lbfgs_unpack_rows(r.data(), p, live, m, SY.data(), YY.data(), gs.data(), gy.data());
      const char* sep = "";
      for (const std::vector<double>* t : {&SY, &YY, &gs, &gy})
        for (double v : *t) { std::printf("%s%a", sep, v); sep = " "; }
      std::printf("\n");
    } else if (std::strcmp(what, "pt") == 0) {
      std::vector<double> a(4);
      if (!numbers(a)) return 2;
      const double slot = a[0], timeout_word = a[1];
      const Arrival got = poll_tag(&slot, &timeout_word, a[2], a[3]);
      std::printf("%s\n", got == Arrival::kArrived ? "arrived" : got == Arrival::kDeviceTimeout ? "timeout" : "expired");
    } else {
      return 2;
    }
  }
  return 0;
}
