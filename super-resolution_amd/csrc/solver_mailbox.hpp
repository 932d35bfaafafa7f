// solver_mailbox.hpp -- the scalar mailbox of the inner solvers (solver.hip): every word the device and the host exchange
// during a run, by name, and the host's polling decision.  Plain C++ with no HIP call in it: tests/cpp/solver_host_test.cpp
// runs it without a GPU.
//
// A kernel that publishes stores its words, a system-scope fence, then the tag it was handed (tags only grow, over all
// solves of a context); the host reads a word once the arrival tag has reached that value.  One-launch scheme (un-sharded
// solves: Fin with granules, LbfgsRed, EvalReq::Publish): the pass's last workgroup writes.  Two-launch scheme (sharded
// solves): k_finish reduces the block partials into dscal, the sums are all-reduced there, k_publish copies them out.
//
//   buffer            word                 writer                                              reader                        valid under
//   ctx->h_scal       kHsPass + 0 .. 3     a reducing pass: its <= 3 rows, then the forwarded  Mailbox::finish, run_cg       the pass's tag
//   (host-mapped)                          cost (Fin::out, cost_src / k_publish)               (row 0 = g.g)
//                     kHsPubF, kHsPubGd    an evaluation's d_cost[kCostValue], [kCostGd]:      fetch_f_gd, begin_run (f)     the publisher's tag
//                     (the same words)     its finish kernel (EvalReq::Publish), k_publish,
//                                          or f alone beside a direction pass (Fin::pub_dst)
//                     kHsDir + kDirMax,    a direction pass (norms_pub, LbfgsRed::out_host);   Mailbox::wait_dir,            dir_tag
//                     kDirSs, kDirGdn      k_publish (two-launch scheme)                       begin_run (dk.dk)
//                     kHsTimeout           any finisher that gave up waiting for a workgroup   every poll of wait_tag,       at once (no tag);
//                                          (Fin::timeout_host, ZArgs::to_host)                 recover_timeout               cleared by open, recovery 
//                     kHsSideTag           the side publish of finish(with_dir) (always 0)     nobody
//                     kHsTag               every publisher, last                               wait_tag
//   dscal             kDsPass + 0 .. 3     k_finish; the copy of d_cost[kCostValue, kCostGd]   the all-reduce, k_publish     stream order
//   (device)          kDsDir + kDirMax ..  a direction pass (Fin::out, LbfgsRed::out_dev);     k_normalize, the folded       stream order
//                                          k_finish + all-reduce                               evaluation (SpFold::norms)
//                     kDsBeta              k_beta_dots' finishing thread                       the direction pass queued     stream order
//                                                                                              behind it (beta_dev)
//                     kDsTimeout           a CG pass that gave up (Fin::timeout_flag, sticky)  nobody (kHsTimeout carries it)
//   lb_host           kLbGg, kLbSs,        k_lbfgs_update's last workgroup                     lbfgs_unpack_rows             the pass's tag
//   (host-mapped)     lb_row(j, kLb*)      (LbfgsRed::out_host)                                (solver_host.hpp)             (at kHsTag)
#pragma once

#include <chrono>

namespace srmap {

// ---- ctx->h_scal ----
constexpr int kHsPass = 0, kHsPassWords = 4;  // up to 3 sums + the forwarded cost
constexpr int kHsPubF = kHsPass, kHsPubGd = kHsPass + 1;
constexpr int kHsDir = 8;
constexpr int kDirMax = 0, kDirSs = 1, kDirGdn = 2, kDirWords = 3;  // {max|dn|, dn.dn, g.dn}, in h_scal and dscal alike
constexpr int kHsTimeout = 13;
constexpr int kHsSideTag = 14;
constexpr int kHsTag = 15;
constexpr int kHsSlots = 16;
// ---- the solver's device scalars ----
constexpr int kDsPass = 0, kDsDir = 4, kDsBeta = 8, kDsTimeout = 15, kDsSlots = 16;
// ---- the rows of the L-BFGS update pass (kernels_lbfgs.hip): two of the new pair, then five per ring slot j ----
constexpr int kLbfgsMaxM = 8;  // history cap of srmap_problem_set_solver (bounds the update pass's accumulators)
constexpr int kLbGg = 0, kLbSs = 1;
constexpr int kLbSyj = 0, kLbYsj = 1, kLbYyj = 2, kLbGsj = 3, kLbGyj = 4, kLbPerSlot = 5;  // s.y_j, y.s_j, y.y_j, g.s_j, g.y_j
constexpr int lb_row(int j, int which) { return 2 + kLbPerSlot * j + which; }
constexpr int lb_rows(int live) { return lb_row(live, 0); }
constexpr int kLbRows = lb_rows(kLbfgsMaxM);

static_assert(kHsPass >= 0 && kHsPubGd < kHsPass + kHsPassWords && kHsPass + kHsPassWords <= kHsDir && kHsDir + kDirWords <= kHsTimeout &&
              kHsTimeout < kHsSideTag && kHsSideTag < kHsTag && kHsTag < kHsSlots, "h_scal: disjoint ranges inside the slot count");
static_assert(kDsPass >= 0 && kDsPass + kHsPassWords <= kDsDir && kDsDir + kDirWords <= kDsBeta && kDsBeta < kDsTimeout &&
              kDsTimeout < kDsSlots, "dscal: disjoint ranges inside the slot count");
static_assert(kLbSs < lb_row(0, 0) && lb_row(0, kLbGyj) + 1 == lb_row(1, kLbSyj) && lb_row(kLbfgsMaxM - 1, kLbGyj) < kLbRows,
              "lb_host: disjoint rows inside kLbRows");

// ---- the host's side of a wait ----
// Tags only grow and the publishing kernels of one stream finish in order, so "arrived" is slot >= want: a later kernel
// queued behind the awaited one (chained passes, run_cg) may already have stored its own tag.
inline bool tag_arrived(const volatile double* slot, double want) { return *slot >= want; }

enum class Arrival { kArrived, kDeviceTimeout, kExpired };
// Poll until the tag has arrived, the device raises the time-out word, or `budget_seconds` have passed (the clock is
// looked at every 1024 spins).
inline Arrival poll_tag(const volatile double* slot, const volatile double* timeout_word, double want, double budget_seconds) {
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (!tag_arrived(slot, want)) {
    if (*timeout_word != 0.0) return Arrival::kDeviceTimeout;
    if ((++spins & 0x3ff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > budget_seconds)
      return Arrival::kExpired;
  }
  return Arrival::kArrived;
}

}  // namespace srmap
