// solver.hip -- IRLSMapSolver::Solve on the GPU (irls_map_solver.cpp:45-157, 192-265): the IRLS outer loop
// (solve_typed) around either inner minimiser of the reference, paced by the host -- L-BFGS (run_lbfgs, minlbfgs) or
// the nonlinear CG the reference obtains from ALGLIB 3.10.0 (run_cg; mincg, default settings: DY/HS hybrid beta,
// More'-Thuente line search, libs/alglib/src/optimization.cpp:17137-17880, alglibinternal.cpp:12313-12632) --
// single-GPU or sharded over one rank per GPU, and the single-run trace entry points.
//
// This file is the control flow only.  Every n-vector lives in HBM and is touched only by the passes
// (solver_passes.hip, kernels_lbfgs.hip) and the evaluation (shard_eval.hip); DeviceCG owns the vectors, hands out the
// arrival tags and queues the passes.  Step selection and the stopping rules run on the host, in double, in ALGLIB's
// order of operations (solver_host.hpp: the More'-Thuente step, the L-BFGS recursion on coefficients), so that the
// trajectory follows the reference's up to reduction order.  Per CG iteration the host waits for the device 2 + nfev
// times: once for the direction's sums, once per trial point for (f, g.d), once for the beta dot products.
//
// Sharding.  The passes reduce over the elements a rank OWNS and DeviceCG all-reduces the sums through the
// communicator (sum, and max for the max-norm), so every rank takes the same decisions; x halos are refreshed before
// every evaluation (comm.hpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "cg_norm.hpp"
#include "comm.hpp"
#include "solver_host.hpp"
#include "solver_passes.hpp"

namespace srmap {

// ---------------------------------------------------------------------------------------------------------
template <typename T>
struct DeviceCG {
  srmap_problem* p;
  hipStream_t st;
  size_t n;
  srmap_comm* comm = nullptr;
  const srmap_shard_desc* shard = nullptr;
  Owned ow{};
  bool reduce_scalars = false;  // row / channel shards: the owned-element sums are all-reduced
  EvalReq::View view;           // channel view of every evaluation (split_channels)
  bool gd_valid = false;        // the last evaluation left g.d in d_cost[1]
  bool published = false;       // the last evaluation's finish kernel published {f, g.d} + tag (fetch_f_gd just waits)
  // chained passes (run_cg): launches whose inputs are already on the device are queued without waiting for the host.
  // srmap_irls_options::host_paced_passes turns this off (every pass then waits for the host's answer, as up to
  // round 3): same arithmetic, same results bit for bit -- tests/test_gpu_solve_parity.py compares the two.  Chaining
  // applies to un-sharded solves only: under frame sharding a speculative first-trial evaluation would queue a
  // gradient + cost all-reduce that every rank has to match before the host has decided to keep it.
  bool chain_enabled = true;
  bool chained() const { return fused() && chain_enabled && (shard == nullptr || comm == nullptr); }
  // x, g: current point and gradient; xk/dk: accepted point and direction; dn: next direction;
  // d: normalised direction (stored only where evaluations read it from memory: !foldable); gp: the gradient at xk
  // while the line search writes its trial gradients to g (the two
  // buffers swap; mincg's yk = g_{k+1} - g_k is formed on the fly).  The line-search base is xk itself.
  T *x = nullptr, *g = nullptr, *xk = nullptr, *dk = nullptr, *dn = nullptr, *d = nullptr, *gp = nullptr;
  double* part = nullptr;   // [3][kRedBlocks] block partials (two-launch reductions: sharded solves)
  unsigned long long* gran = nullptr;  // [3][kRedBlocks] granules of the one-launch reductions (armed)
  double* dscal = nullptr;  // device scalars: [0..3] reduction results, [4..6] the direction's sums {max|dn|, dn.dn, g.dn}, [8] beta, [15] time-out flag
  double* hs = nullptr;     // host-mapped pinned scalars (ctx->h_scal): pass results [0..3], the direction's sums [8..10], arrival tag [15]
  double tag = 0;           // last tag handed to a publishing kernel
  int evaluations = 0;
  double wait_seconds = 0;  // host time spent in wait_tag
  int waits = 0;
  // L-BFGS (run_lbfgs, kernels_lbfgs.hip): ring of lb_m pairs S[j] = s_j, Y[j] = y_j ([lb_m][n] each), the passes'
  // workgroup partials and ticket, and the update pass's sums (host-mapped: they are not ctx->h_scal's 16 slots)
  int lb_m = 0;
  T *S = nullptr, *Y = nullptr;
  double* lb_part = nullptr;
  unsigned* lb_ticket = nullptr;
  double* lb_host = nullptr;
  static constexpr int kLbRows = 2 + 5 * kLbfgsMaxM;
  // the owners of every device buffer above (the typed members are views: the passes swap them); freed with the solver
  std::vector<DevBuf> mem;
  PinnedBuf lb_host_mem;
  template <typename U>
  int dev_alloc(U** view, size_t bytes) {
    mem.emplace_back();
    SRMAP_HIP(p->ctx, mem.back().alloc(bytes));
    *view = mem.back().template as<U>();
    return SRMAP_OK;
  }

  // Wait until the kernel that was given tag `want` (default: the last one handed out) has published its results (see
  // k_finish): poll the host-mapped word, fall back to a stream synchronisation after ~2 s (also surfaces asynchronous
  // errors).  Tags only grow and the publishing kernels of one stream finish in order, so "arrived" is slot >= want:
  // a later kernel queued behind the awaited one (chained passes, run_cg) may already have stored its own tag.
  int wait_tag(double want = -1.0) {
    if (want < 0) want = tag;
    volatile double* slot = hs + 15;
    const auto t0 = std::chrono::steady_clock::now();
    struct Acc { DeviceCG* c; std::chrono::steady_clock::time_point t; ~Acc() {
      c->wait_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); c->waits++; } } acc{this, t0};
    unsigned spins = 0;
    volatile double* to = hs + 13;   // a device-side reduction of this solve timed out: its sums are NaN, its granules not re-armed
    while (!(*slot >= want)) {
      if (*to != 0.0) return set_error(p->ctx, SRMAP_EHIP, "solver: a device-side reduction timed out waiting for a workgroup");
      if ((++spins & 0x3ff) == 0 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) {
        SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
        if (!(*slot >= want)) return set_error(p->ctx, SRMAP_EHIP, "solver: device results did not arrive");
        break;
      }
    }
    return SRMAP_OK;
  }

  int nb() const { size_t b = (n + 255) / 256; return (int)(b < (size_t)kRedBlocks ? b : kRedBlocks); }

  int alloc() {
    T** v[] = {&x, &g, &xk, &dk, &dn, &d, &gp};
    for (T** q : v)
      if (int rc = dev_alloc(q, n * sizeof(T))) return rc;
    if (int rc = dev_alloc(&part, sizeof(double) * 3 * kRedBlocks)) return rc;
    if (int rc = dev_alloc(&dscal, sizeof(double) * 16)) return rc;
    SRMAP_HIP(p->ctx, hipMemsetAsync(dscal, 0, sizeof(double) * 16, st));
    if (int rc = dev_alloc(&gran, sizeof(double) * 3 * kRedBlocks)) return rc;
    SRMAP_HIP(p->ctx, hipMemsetD32Async((hipDeviceptr_t)gran, (int)kArm32, 2 * 3 * kRedBlocks, st));
    // sharded evaluations write only the owned part of g: the vector kernels run over all n elements, so everything
    // they combine starts defined (the halo values never enter a reduction, and x halos are re-exchanged)
    T* z[] = {g, dn, d, dk, gp};
    for (T* q : z) SRMAP_HIP(p->ctx, hipMemsetAsync(q, 0, n * sizeof(T), st));
    int rc = ensure_staging(p->ctx);
    if (rc) return rc;
    hs = p->ctx->h_scal.as<double>();
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    hs[13] = 0.0;  // time-out word of this solve (Fin::timeout_host, ZArgs::to_host)
    tag = hs[15];  // tags keep increasing across solves of one context: a stale word can never match
    return SRMAP_OK;
  }
  int alloc_lbfgs(int m) {
    lb_m = m;
    if (int rc = dev_alloc(&S, (size_t)m * n * sizeof(T))) return rc;
    if (int rc = dev_alloc(&Y, (size_t)m * n * sizeof(T))) return rc;
    SRMAP_HIP(p->ctx, hipMemsetAsync(S, 0, (size_t)m * n * sizeof(T), st));
    SRMAP_HIP(p->ctx, hipMemsetAsync(Y, 0, (size_t)m * n * sizeof(T), st));
    if (int rc = dev_alloc(&lb_part, sizeof(double) * kLbRows * kRedBlocks)) return rc;
    if (int rc = dev_alloc(&lb_ticket, sizeof(unsigned))) return rc;
    SRMAP_HIP(p->ctx, hipMemsetAsync(lb_ticket, 0, sizeof(unsigned), st));
    SRMAP_HIP(p->ctx, lb_host_mem.alloc(sizeof(double) * kLbRows, hipHostMallocMapped | hipHostMallocCoherent));
    lb_host = lb_host_mem.as<double>();
    for (int i = 0; i < kLbRows; ++i) lb_host[i] = 0.0;
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    return SRMAP_OK;
  }
  int copy(T* dst, const T* src) {
    SRMAP_HIP(p->ctx, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    return SRMAP_OK;
  }
  // One-launch reductions (struct Fin) whenever the sums need no all-reduce.
  bool fused() const { return !reduce_scalars; }
  // the pass about to be launched reduces to the host: out = hs[0 .. rows) (+ the cost at hs[rows]), then the tag
  Fin fin_host(bool with_cost, const double* pub_src = nullptr, double* pub_dst = nullptr, int pub_n = 0,
               double* out = nullptr) {
    Fin f{};
    if (fused()) {
      tag += 1.0;
      f.gran = gran; f.out = out ? out : hs; f.cost_src = with_cost ? (const double*)p->d_cost.as<double>() : nullptr;
      f.timeout_flag = dscal + 15; f.timeout_host = hs + 13;
      f.pub_src = pub_src; f.pub_dst = pub_dst; f.pub_n = pub_n;
      f.tag_slot = hs + 15; f.tag = tag;
    }
    return f;
  }
  // Bring the sums of the pass just launched to the host: out[0..rows) (+ out[rows] = cost).  One wait.  Two-launch
  // scheme: reduces the `rows` partial rows here (k_finish), all-reduces them, publishes.
  int finish(int rows, bool max0, bool with_cost, double* out, int extra_n = 0) {
    const int cnt = rows + (with_cost ? 1 : 0);
    if (!fused()) {
      tag += 1.0;
      launch_finish(part, nb(), rows, max0 ? 1 : 0, dscal, with_cost ? (const double*)p->d_cost.as<double>() : nullptr, nullptr, 0.0, st);
      int rc = SRMAP_OK;
      if (max0) {
        rc = comm_allreduce(comm, dscal, 1, SRMAP_F64, 1, st);
        if (rc) return rc;
        if (cnt > 1) rc = comm_allreduce(comm, dscal + 1, (size_t)cnt - 1, SRMAP_F64, 0, st);
      } else {
        rc = comm_allreduce(comm, dscal, (size_t)cnt, SRMAP_F64, 0, st);
      }
      if (rc) return rc;
      if (extra_n > 0)
        launch_publish(hs + 8, dscal + 4, extra_n, hs + 14, 0.0, st);
      launch_publish(hs, dscal, cnt, hs + 15, tag, st);
    }
    SRMAP_HIP(p->ctx, hipGetLastError());
    int rc = wait_tag();
    if (rc) return rc;
    for (int i = 0; i < cnt; ++i) out[i] = hs[i];
    return SRMAP_OK;
  }
  // objective at x: g <- gradient; the cost stays on the device (finish(with_cost) fetches it).  With a direction
  // the tile kernel may produce g.d in the same pass (gd_valid; not under frame sharding, where the local
  // gradient is only a partial sum).
  // the line search may hand its trial point to the evaluation as (xk, stp): un-sharded solves on the tile kernel's
  // g.d instance (ztile_can_fold); decided once per CG run
  bool foldable = false;
  bool fold_enabled = true;   // srmap_irls_options::host_paced_passes also forms every trial point by its own pass (the A/B of the fold)
  int evaluate(const T* dir = nullptr, T* at = nullptr, const T* fold_xk = nullptr, double fold_stp = 0.0) {  // at: the point (default x)
    evaluations++;
    const int mode = shard_mode(comm, shard);
    EvalReq req;
    req.view = view;
    req.dvec = (mode == SRMAP_SHARD_FRAMES || mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) ? nullptr : dir;
    // without a scalar all-reduce the evaluation's finish kernel can publish {f, g.d} and the arrival tag itself
    req.pub = {(!reduce_scalars && req.dvec != nullptr) ? hs : nullptr, hs + 15, tag + 1.0, hs + 13};
    // fold: `dir` is the UNNORMALISED direction dk; the kernel scales it by the factors it derives from the norms the
    // direction pass left at dscal[4..5] (norm_factors / norm_elem: the bits of the stored d)
    if (fold_xk != nullptr && req.dvec != nullptr) req.fold = {fold_xk, req.dvec, fold_stp, (const double*)(dscal + 4)};
    EvalOut out;
    const int rc = shard_eval(p, comm, shard, req, &out, SRMAP_TERM_ALL, at ? at : x, g, st);
    gd_valid = out.gd_valid;
    published = out.published;
    if (published) tag += 1.0;
    return rc;
  }
  // The evaluation queued ahead of the host's decision (run_cg: the first trial point behind the normalisation pass)
  // turned out not to be wanted: it is not one of the solve's evaluations and nobody fetches its sums.  Its tag, if it
  // publishes one, is simply passed over (wait_tag compares with >=).
  void discard_speculative() {
    evaluations--;
    published = false;
  }
  // End of a solve or trace: a reduction that gave up waiting for a workgroup (the tile kernel's in-kernel finish:
  // sticky word d_cost[6]; a CG pass: dscal[15]) left NaN sums behind -- the stopping rules ended the run -- and its
  // granules un-re-armed.  The evaluations of a run never look at the word (wait_tag ends the run on the host-mapped
  // word hs[13], which both kinds of finisher raise): look now, re-initialise, report.  No device copy on success.
  int recover_timeout(int rc) {
    (void)hipStreamSynchronize(st);
    if (hs == nullptr || hs[13] == 0.0) return rc;
    const int rr = recover_reduction_timeout(p, hs + 13);
    if (rc != SRMAP_OK) return rc;
    return rr ? rr : set_error(p->ctx, SRMAP_EHIP, "a device-side reduction timed out waiting for a workgroup during the solve (device fault or a wedged queue)");
  }
  // f and g.d of the evaluation just made, with one wait: out[0] = g.d, out[1] = f
  int fetch_f_gd(double* out) {
    if (!gd_valid) {
      launch_cg_dot<T>(g, d, n, ow, part, fin_host(true), nb(), st);
      return finish(1, false, true, out);
    }
    if (published) {  // the evaluation's own finish kernel carries the tag
      published = false;
      const int rcw = wait_tag();
      if (rcw) return rcw;
      out[0] = hs[1];
      out[1] = hs[0];
      return SRMAP_OK;
    }
    tag += 1.0;
    if (!reduce_scalars) {
      launch_publish(hs, p->d_cost.as<double>(), 2, hs + 15, tag, st);
    } else {
      SRMAP_HIP(p->ctx, hipMemcpyAsync(dscal, p->d_cost.as<double>(), 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
      int rc = comm_allreduce(comm, dscal, 2, SRMAP_F64, 0, st);
      if (rc) return rc;
      launch_publish(hs, dscal, 2, hs + 15, tag, st);
    }
    SRMAP_HIP(p->ctx, hipGetLastError());
    int rc = wait_tag();
    if (rc) return rc;
    out[0] = hs[1];
    out[1] = hs[0];
    return SRMAP_OK;
  }
  // dn = -g + beta dk (dk may be null); {max|dn|, dn.dn, g.dn} -> dscal[4..6] (device, all-reduced) and, under a tag of
  // the pass's own (dir_tag: wait_dir), hs[8..10].  publish_cost: the first pass of a CG run also hands f to the host
  // (one-launch scheme: hs[0] with the same tag; two-launch scheme: the caller's finish(0, ..., 3) publishes all four).
  // beta_dev: beta comes from the device scalar the k_beta_dots queued just before left there (one-launch scheme only)
  double dir_tag = 0;
  int direction(const T* dk_or_null, double beta, bool publish_cost = false, const double* beta_dev = nullptr) {
    Fin f{};
    if (fused()) {
      tag += 1.0;
      dir_tag = tag;
      f.gran = gran; f.out = dscal + 4; f.timeout_flag = dscal + 15; f.timeout_host = hs + 13;
      if (publish_cost) { f.pub_src = (const double*)p->d_cost.as<double>(); f.pub_dst = hs; f.pub_n = 1; }  // hs[0] = f
      f.tag_slot = hs + 15; f.tag = tag;
    }
    double* npub = fused() ? hs + 8 : (double*)nullptr;
    const int keep = foldable ? 1 : 0;
    launch_cg_direction<T>(dn, g, dk_or_null, (T)beta, n, ow, part, f, beta_dev, npub, keep, nb(), st);
    if (!fused()) {
      launch_finish(part, nb(), 3, 1, dscal + 4, nullptr, nullptr, 0.0, st);
      int rc = comm_allreduce(comm, dscal + 4, 1, SRMAP_F64, 1, st);
      if (rc) return rc;
      rc = comm_allreduce(comm, dscal + 5, 2, SRMAP_F64, 0, st);
      if (rc) return rc;
      if (!publish_cost) {
        tag += 1.0;
        dir_tag = tag;
        launch_publish(hs + 8, dscal + 4, 3, hs + 15, tag, st);
      }
    }
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // L-BFGS: ring slot p <- (x - xk, g - gk) and the Gram rows of the new pair (launch_lbfgs_update) -> lb_host, one wait
  int lbfgs_update(const T* gk, int p_slot, int live) {
    tag += 1.0;
    const LbfgsRed red{lb_part, lb_ticket, nullptr, lb_host, hs + 15, tag};
    int rc = launch_lbfgs_update<T>(x, xk, g, gk, S, Y, p_slot, live, n, nb(), red, st);
    if (rc) return set_error(p->ctx, rc, "lbfgs: bad history length");
    SRMAP_HIP(p->ctx, hipGetLastError());
    return wait_tag();
  }
  // L-BFGS: dn from the coefficients over {g, S[0..live), Y[0..live)}; its sums where `direction` leaves them
  // (dscal[4..6], hs[8..10] under dir_tag)
  int lbfgs_direction(const LbfgsCoef& c, int live) {
    tag += 1.0;
    dir_tag = tag;
    const LbfgsRed red{lb_part, lb_ticket, dscal + 4, hs + 8, hs + 15, tag};
    int rc = launch_lbfgs_direction<T>(dn, g, S, Y, live, c, n, nb(), foldable ? 1 : 0, red, st);
    if (rc) return set_error(p->ctx, rc, "lbfgs: bad history length");
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // the sums of the last direction pass on the host: {max|dn|, dn.dn, g.dn}
  int wait_dir(double* mx, double* ss, double* gdn) {
    const int rc = wait_tag(dir_tag);
    if (rc) return rc;
    *mx = hs[8]; *ss = hs[9]; *gdn = hs[10];
    return SRMAP_OK;
  }
  // d = dk s1 s2 stored as a vector (+ the first trial point x = xk + stp1 d when stp1 != 0): the paths whose evaluations
  // read the normalised direction from memory
  int normalize(double stp1) {
    launch_cg_normalize<T>(d, dk, dscal + 4, n, xk, stp1 != 0.0 ? x : (T*)nullptr, (T)stp1, nb(), st);
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // The opening of a run (run_cg, run_lbfgs): evaluate at the start point, dk = -g with its sums, and f and g.g = dk.dk
  // on the host after one wait.  *small_g: the epsg rule already holds (the caller ends the run with x = xk).
  int begin_run(double epsg, double* f, double* gg, bool* small_g, std::vector<double>* trace) {
    // the start point becomes the base point xk by exchanging the two buffers (no copy); x is trial scratch from here on:
    // every path of a run writes it before reading it (the trial points) or copies xk back into it (the early exits)
    std::swap(xk, x);
    foldable = shard_mode(comm, shard) == SRMAP_SHARD_NONE && fold_enabled && ztile_can_fold(p, view.C > 0 ? view.C : p->geo.C);
    int rc = evaluate(nullptr, xk);
    if (rc) return rc;
    // dk = -g (written as dn, swapped below), norms of dk
    rc = direction(nullptr, 0.0, true);
    if (rc) return rc;
    if (fused()) {  // the direction pass published {f -> hs[0]; max|dk|, dk.dk, g.dk -> hs[8..10]} itself
      rc = wait_tag();
      if (rc) return rc;
      *f = hs[0];
    } else {
      // fetch f and the direction's sums (already reduced on the device) with one wait
      double h[1];
      rc = finish(0, false, true, h, 3);
      if (rc) return rc;
      dir_tag = tag;
      *f = h[0];
    }
    *gg = hs[9];  // g.g = dk.dk
    if (trace) trace->push_back(*f);
    std::swap(dk, dn);
    *small_g = std::sqrt(*gg) <= epsg;
    return SRMAP_OK;
  }
};

// mcsrch with the device evaluation inlined (constants alglibinternal.cpp:156-160;
// trimfunction after each evaluation as mincgiteration does, optimization.cpp:17594).
template <typename T>
static int line_search(DeviceCG<T>& cg, double* f, double dginit, double* stp, double gtol,
                       int* info, int* nfev, double trim, std::vector<double>* trace, double stp_in_x = 0.0,
                       bool pre_launched = false, double* dg_last = nullptr) {
  const double ftol = 0.001, xtol = 100 * 5E-16, stpmin = 1.0e-50, stpmax = 1.0e+50, p5 = 0.5,
               p66 = 0.66, xtrapf = 4.0;
  const int maxfev = 20;
  if (*stp < stpmin) *stp = stpmin;
  if (*stp > stpmax) *stp = stpmax;
  int infoc = 1;
  *info = 0;
  *nfev = 0;
  // On entry the base point is cg.xk; cg.x is scratch for the trial points.  The paths that try nothing
  // still leave x = base, as mcsrch does.
  // pre_launched: the evaluation at xk + stp_in_x * d is already queued (behind the pass that wrote that point)
  if (*stp <= 0 || dginit >= 0) {  // (dginit >= 0: not a descent direction)
    if (pre_launched) cg.discard_speculative();
    return cg.copy(cg.x, cg.xk);
  }
  bool brackt = false, stage1 = true;
  const double finit = *f, dgtest = ftol * dginit;
  double width = stpmax - stpmin, width1 = width / p5;
  int rc = SRMAP_OK;
  Bracket b = {0, finit, dginit, 0, finit, dginit};
  double stmin = 0, stmax = 0;
  for (;;) {
    if (brackt) { stmin = dmin(b.stx, b.sty); stmax = dmax(b.stx, b.sty); }
    else { stmin = b.stx; stmax = *stp + xtrapf * (*stp - b.stx); }
    if (*stp > stpmax) *stp = stpmax;
    if (*stp < stpmin) *stp = stpmin;
    if ((brackt && (*stp <= stmin || *stp >= stmax)) || *nfev >= maxfev - 1 || infoc == 0 ||
        (brackt && stmax - stmin <= xtol * stmax))
      *stp = b.stx;
    // stp_in_x: cg.x already holds xk + stp_in_x * d (written by the scaling pass) or the evaluation that forms it is
    // already queued (pre_launched); any other step is formed here
    const bool first_in_x = *nfev == 0 && stp_in_x != 0.0 && *stp == stp_in_x;
    if (*nfev == 0 && pre_launched && !first_in_x) { cg.discard_speculative(); pre_launched = false; }
    // the trial point x = xk + stp * d: formed by the evaluation itself as it loads its window where that is possible
    // (one n-vector pass less per trial point; x holds the point afterwards all the same), else by its own pass
    const bool fold_here = !first_in_x && cg.foldable;
    if (!first_in_x && !fold_here) launch_axpy_out<T>(cg.x, cg.xk, cg.d, (T)*stp, cg.n, cg.st);
    if (!(first_in_x && pre_launched)) {
      rc = fold_here ? cg.evaluate(cg.dk, nullptr, cg.xk, *stp) : cg.evaluate(cg.d);
      if (rc) return rc;
    }
    double h[2];
    rc = cg.fetch_f_gd(h);  // h[0] = g.d, h[1] = f
    if (rc) return rc;
    double dg = h[0];
    *f = h[1];
    if (trace) trace->push_back(*f);
    if (*f >= trim) {  // trimfunction: F = threshold, G = 0
      *f = trim;
      launch_fill<T>(cg.g, T(0), cg.n, cg.st);
      dg = 0;
    }
    *info = 0;
    *nfev += 1;
    if (dg_last) *dg_last = dg;
    const double ftest1 = finit + *stp * dgtest;
    if ((brackt && (*stp <= stmin || *stp >= stmax)) || infoc == 0) *info = 6;
    if (*stp == stpmax && *f < finit && *f <= ftest1 && dg <= dgtest) *info = 5;
    if (*stp == stpmin && (*f >= finit || *f > ftest1 || dg >= dgtest)) *info = 4;
    if (*nfev >= maxfev) *info = 3;
    if (brackt && stmax - stmin <= xtol * stmax) *info = 2;
    if (*f < finit && *f <= ftest1 && std::fabs(dg) <= -gtol * dginit) *info = 1;
    if (*info != 0) {
      if (*info == 1 || *info == 5) {
        // ALGLIB additionally demotes to 6 when the point did not move
        // (sum (wa-x)^2 == 0); with stp > 0 and a unit d this cannot be 0
        // unless stp*d underflows against x, which we test through stp.
        if (*f >= finit || *stp == 0.0) *info = 6;
      }
      return SRMAP_OK;
    }
    if (stage1 && *f <= ftest1 && dg >= dmin(ftol, gtol) * dginit) stage1 = false;
    if (stage1 && *f <= b.fx && *f > ftest1) {
      const double fm = *f - *stp * dgtest;
      Bracket m = {b.stx, b.fx - b.stx * dgtest, b.dx - dgtest, b.sty, b.fy - b.sty * dgtest, b.dy - dgtest};
      mt_step(&m, stp, fm, dg - dgtest, &brackt, stmin, stmax, &infoc);
      b.stx = m.stx; b.sty = m.sty;
      b.fx = m.fx + m.stx * dgtest; b.fy = m.fy + m.sty * dgtest;
      b.dx = m.dx + dgtest; b.dy = m.dy + dgtest;
    } else {
      mt_step(&b, stp, *f, dg, &brackt, stmin, stmax, &infoc);
    }
    if (brackt) {
      if (std::fabs(b.sty - b.stx) >= p66 * width1) *stp = b.stx + p5 * (b.sty - b.stx);
      width1 = width;
      width = std::fabs(b.sty - b.stx);
    }
  }
}

struct CgResult { int type = 0, its = 0, nfev = 0; double f = 0; };

// mincgiteration (optimization.cpp:17137-17880), default configuration: no
// preconditioner, unit scales, cgtype = 1, no stpmax.  On return cg.x holds
// the accepted point XN.  trace (optional): f of every evaluation, in order.
template <typename T>
static int run_cg(DeviceCG<T>& cg, double epsg, double epsf, double epsx, int maxits, CgResult* out,
                  std::vector<double>* trace) {
  const double gtol = 0.3;
  const int rscountdownlen = 10;
  if (epsg == 0 && epsf == 0 && epsx == 0 && maxits == 0) epsx = 1.0E-6;
  const size_t n = cg.n;
  CgResult res;
  double f = 0, gg = 0;
  bool small_g = false;
  int rc = cg.begin_run(epsg, &f, &gg, &small_g, trace);
  if (rc) return rc;
  const double trim = 10 * (std::fabs(f) + 1);
  if (small_g) { res.type = 4; res.f = f; *out = res; return cg.copy(cg.x, cg.xk); }
  res.nfev = 1;
  double fold = f, lastgoodstep = 1.0;
  int rstimer = rscountdownlen;
  for (;;) {
    // d = dk s1 s2 (linminnormalized); g.d and d.d follow from the sums of the pass that produced dk.  x = xk is not
    // materialised: every trial point x = xk + stp * d is written by the line search -- by the evaluation itself, from dk
    // and the norms on the device, where the tile kernel can (foldable), else from the d a scaling pass stores.
    double stp = 1.0, dginit = 0, dd = 0;
    double gdk = 0, ns1 = 1, ns2 = 1;  // g.dk at xk and the two scale factors, for the beta denominator below
    bool pre_launched = false, g_swapped = false;
    // the first step is lastgoodstep unless that is 0 (then it comes from the direction's norms)
    const double stp_pre = (lastgoodstep != 0 && lastgoodstep >= 1.0e-50 && lastgoodstep <= 1.0e+50) ? lastgoodstep : 0.0;
    double stp_ready = 0.0;  // the step whose trial point is already in cg.x and / or whose evaluation is already queued
    {
      if (!cg.foldable) {
        rc = cg.normalize(stp_pre);
        if (rc) return rc;
        stp_ready = stp_pre;
      }
      // The line search's first trial evaluation is queued NOW, behind the passes above, and runs while the host waits
      // for the direction's sums and decides (mcsrch tries stp first whenever g.d < 0; otherwise line_search discards the
      // evaluation): no host round trip in front of it.
      if (stp_pre != 0.0 && cg.chained()) {
        std::swap(cg.g, cg.gp);  // gp = gradient at xk
        g_swapped = true;
        rc = cg.foldable ? cg.evaluate(cg.dk, nullptr, cg.xk, stp_pre) : cg.evaluate(cg.d);
        if (rc) return rc;
        pre_launched = true;
        stp_ready = stp_pre;
      }
      double mx = 0, ss = 0, gdn = 0;
      rc = cg.wait_dir(&mx, &ss, &gdn);
      if (rc) return rc;
      double s1, s2;
      norm_factors(mx, ss, s1, s2);
      dginit = (gdn * s1) * s2;
      dd = ((ss * s1) * s1) * (s2 * s2);
      gdk = gdn; ns1 = s1; ns2 = s2;
      if (mx != 0) { stp = stp / s1; stp = stp / s2; }
    }
    if (lastgoodstep != 0) stp = lastgoodstep;
    int mcinfo = 0, nfev = 0;
    if (!g_swapped) std::swap(cg.g, cg.gp);  // gp = gradient at xk; the trial evaluations write g
    double dg_acc = 0;  // g.d at the last trial point
    rc = line_search(cg, &f, dginit, &stp, gtol, &mcinfo, &nfev, trim, trace, stp_ready, pre_launched, &dg_acc);
    if (rc) return rc;
    if (nfev == 0) std::swap(cg.g, cg.gp);  // nothing was evaluated: g stays the gradient at xk, as in mcsrch
    double betak = 0;
    // One-launch scheme: the direction pass is queued right behind the pass that reduces the beta sums -- beta itself is
    // formed by that pass's finishing thread (k_beta_dots) -- and runs while the host waits for the sums it needs for
    // the stopping rules.  (mincg's periodic restart is known beforehand; `direction` was always launched before the
    // rules are looked at.)
    const bool chain = cg.chained();
    const int restart = (res.its > 0 && res.its % (3 + (long long)n) == 0) ? 1 : 0;
    if (mcinfo == 1) {
      // yk = g - gp ; vv = yk.dk ; betady = g.g/vv ; betahs = g.yk/vv.  vv = g.dk - gp.dk from sums already on the
      // host: gp.dk is the direction pass's g.dn, g.dk = (g.d) / (s2 s1) with the accepted evaluation's g.d (k_beta_dots)
      const double vv = (dg_acc / ns2) / ns1 - gdk;
      double* beta_dst = chain ? cg.dscal + 8 : (double*)nullptr;
      // host-paced passes: the pass also sums y.dk directly (one more vector read) and the deviation of the derived
      // denominator from it is recorded (srmap_problem_selfcheck; tests/test_gpu_solve_parity.py)
      const T* dk_chk = chain ? (const T*)nullptr : (const T*)cg.dk;
      launch_cg_beta_dots<T>(cg.gp, cg.g, n, cg.ow, cg.part, cg.fin_host(false), beta_dst, restart, vv, dk_chk, cg.nb(), cg.st);
      if (chain) {
        const double tag_beta = cg.tag;
        rc = cg.direction(cg.dk, 0.0, false, cg.dscal + 8);  // dn, sums of dn (device)
        if (rc) return rc;
        rc = cg.wait_tag(tag_beta);
        if (rc) return rc;
        gg = cg.hs[0];
      } else {
        double h[3];
        rc = cg.finish(3, false, false, h);
        if (rc) return rc;
        betak = dmax(0.0, dmin(h[0] / vv, h[1] / vv));
        gg = h[0];
        if (h[2] != 0.0 && std::isfinite(h[2]) && std::isfinite(vv))
          cg.p->selfcheck_beta_den = dmax(cg.p->selfcheck_beta_den, std::fabs(vv - h[2]) / std::fabs(h[2]));
      }
    } else {
      launch_cg_dot<T>(cg.g, cg.g, n, cg.ow, cg.part, cg.fin_host(false), cg.nb(), cg.st);
      if (chain) {
        const double tag_gg = cg.tag;
        rc = cg.direction(cg.dk, 0.0);  // beta = 0
        if (rc) return rc;
        rc = cg.wait_tag(tag_gg);
        if (rc) return rc;
        gg = cg.hs[0];
      } else {
        double h[1];
        rc = cg.finish(1, false, false, h);
        if (rc) return rc;
        gg = h[0];
      }
    }
    if (restart) betak = 0;
    if (mcinfo == 1 || mcinfo == 5) rstimer = rscountdownlen; else rstimer -= 1;
    if (!chain) {
      rc = cg.direction(cg.dk, betak);  // dn, norms of dn (device)
      if (rc) return rc;
    }
    const double lastscaledstep = stp * std::sqrt(dd);
    if (mcinfo == 1) lastgoodstep = stp * std::sqrt(dd);
    if (!std::isfinite(gg) || !std::isfinite(f)) { res.type = -8; break; }
    res.nfev += nfev;
    res.its += 1;
    if (res.its >= maxits && maxits > 0) { res.type = 5; break; }
    if (std::sqrt(gg) <= epsg) { res.type = 4; break; }
    if (fold - f <= epsf * dmax(std::fabs(fold), dmax(std::fabs(f), 1.0))) { res.type = 1; break; }
    if (lastscaledstep <= epsx) { res.type = 2; break; }
    if (rstimer <= 0) { res.type = 7; break; }
    std::swap(cg.xk, cg.x);    // xk <- accepted point; the old xk becomes trial scratch
    std::swap(cg.dk, cg.dn);   // dk <- new direction
    fold = f;
  }
  res.f = f;
  *out = res;
  return SRMAP_OK;
}

// minlbfgsiteration (optimization.cpp:21640 ff.), default configuration: no preconditioner (prectype 0), unit scales,
// no stpmax, analytic gradient.  Same device vectors and line search as run_cg; the history lives in the ring
// cg.S / cg.Y.  ALGLIB's two-loop recursion runs on the host on the coefficients of the direction over
// {g, s_j, y_j}, each dot product taken from the Gram rows the update pass reduced (kernels_lbfgs.hip): per iteration
// one update pass, one direction pass, and a wait for each.  On return cg.x holds the accepted point.  trace
// (optional): f of every evaluation, in order.
template <typename T>
static int run_lbfgs(DeviceCG<T>& cg, double epsg, double epsf, double epsx, int maxits, CgResult* out,
                     std::vector<double>* trace) {
  const double gtol = 0.4;  // minlbfgs_gtol, optimization.cpp:8941
  const int m = cg.lb_m;
  if (epsg == 0 && epsf == 0 && epsx == 0 && maxits == 0) epsx = 1.0E-6;  // minlbfgssetcond
  CgResult res;
  double f = 0, gg = 0;
  bool small_g = false;
  int rc = cg.begin_run(epsg, &f, &gg, &small_g, trace);
  if (rc) return rc;
  const double trim = 10 * (std::fabs(f) + 1);  // trimprepare
  if (small_g) { res.type = 4; res.f = f; *out = res; return cg.copy(cg.x, cg.xk); }
  res.nfev = 1;
  double fold = f;
  double stp = dmin(1.0 / std::sqrt(gg), 1.0);  // prectype 0, stpmax 0
  // Gram tables over the ring slots: SY[a * m + b] = s_a.y_b, YY[a * m + b] = y_a.y_b, gs[j] = g.s_j, gy[j] = g.y_j (g
  // the current gradient).  The update pass recomputes every entry of the slot it writes.
  std::vector<double> SY((size_t)m * m, 0.0), YY((size_t)m * m, 0.0), gs(m, 0.0), gy(m, 0.0), rho(m, 0.0);
  int k = 0, nfev_state = 0;  // ALGLIB's state->nfev: a line search that returns before its first trial leaves it as it was
  for (;;) {
    const int p = k % m, q = k < m - 1 ? k : m - 1, live = q + 1;
    if (k != 0) stp = 1.0;
    // linminnormalized from the direction's sums (cg_norm.hpp); the paths whose evaluations read d from memory store it
    if (!cg.foldable) {
      rc = cg.normalize(0.0);
      if (rc) return rc;
    }
    double mx = 0, ss = 0, gdn = 0;
    rc = cg.wait_dir(&mx, &ss, &gdn);
    if (rc) return rc;
    double s1, s2;
    norm_factors(mx, ss, s1, s2);
    const double dginit = (gdn * s1) * s2;
    if (mx != 0) { stp = stp / s1; stp = stp / s2; }
    int mcinfo = 0, nfev = 0;
    std::swap(cg.g, cg.gp);  // gp = gradient at xk; the trial evaluations write g
    rc = line_search(cg, &f, dginit, &stp, gtol, &mcinfo, &nfev, trim, trace);
    if (rc) return rc;
    if (nfev == 0) std::swap(cg.g, cg.gp);  // nothing evaluated: x = xk, g the gradient there (s = y = 0)
    if (nfev != 0) nfev_state = nfev;
    res.nfev += nfev_state;
    res.its += 1;
    // sk = x - xk, yk = g - g_k into slot p (ALGLIB writes them whatever mcinfo is) and the Gram rows of the new pair
    rc = cg.lbfgs_update(nfev == 0 ? (const T*)cg.g : (const T*)cg.gp, p, live);
    if (rc) return rc;
    const double* r = cg.lb_host;
    gg = r[0];
    const double sks = r[1];
    for (int j = 0; j < live; ++j) {
      SY[(size_t)p * m + j] = r[2 + 5 * j];
      SY[(size_t)j * m + p] = r[3 + 5 * j];
      YY[(size_t)p * m + j] = r[4 + 5 * j];
      YY[(size_t)j * m + p] = r[4 + 5 * j];
      gs[j] = r[5 + 5 * j];
      gy[j] = r[6 + 5 * j];
    }
    if (!std::isfinite(gg) || !std::isfinite(f)) { res.type = -8; break; }
    if (res.its >= maxits && maxits > 0) { res.type = 5; break; }
    if (std::sqrt(gg) <= epsg) { res.type = 4; break; }
    if (fold - f <= epsf * dmax(std::fabs(fold), dmax(std::fabs(f), 1.0))) { res.type = 1; break; }
    if (std::sqrt(sks) <= epsx) { res.type = 2; break; }
    if (mcinfo != 1) {
      // restart from the steepest descent; k is not advanced (slot p is written again), and while k == 0 the next
      // line search starts from the step this one ended on
      fold = f;
      rc = cg.direction(nullptr, 0.0);
      if (rc) return rc;
    } else {
      LbfgsCoef c{};
      if (!lbfgs_two_loop(SY.data(), YY.data(), gs.data(), gy.data(), rho.data(), k, q, m, c.c)) { res.type = -2; break; }
      rc = cg.lbfgs_direction(c, live);  // d = -work
      if (rc) return rc;
      fold = f;
      k += 1;
    }
    std::swap(cg.xk, cg.x);   // xk <- accepted point; the old xk becomes trial scratch
    std::swap(cg.dk, cg.dn);  // dk <- new direction
  }
  res.f = f;
  *out = res;
  return SRMAP_OK;
}

template <typename T>
static int solve_typed(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard, const srmap_irls_options* opt,
                       const double* x0, double* x_out, srmap_solve_report* report, const void* x0_dev = nullptr,
                       void* x_out_dev = nullptr) {
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "cannot super-resolve with 0 low-res images");
  const Geometry& geo = p->geo;
  const size_t N = (size_t)geo.W * geo.H;
  const int C = geo.C;
  const int mode = shard_mode(comm, shard);
  const bool lbfgs = p->solver == SRMAP_SOLVER_LBFGS;
  if (lbfgs && mode != SRMAP_SHARD_NONE)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "L-BFGS solves are not sharded over a communicator (its Gram rows would need an all-reduce): run them unsharded, or per channel with split_channels");
  const bool huber = p->dw.loss() == SRMAP_DATA_LOSS_HUBER;
  if (int rc = refuse_sharded(p, mode, "solve")) return rc;
  if (mode != SRMAP_SHARD_NONE && opt->split_channels)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "split_channels solves are independent per channel: run them unsharded");
  if (mode == SRMAP_SHARD_ROWS &&
      (shard->own_row0 < 0 || shard->own_row1 > geo.H || shard->own_row0 >= shard->own_row1 ||
       shard->own_row0 != geo.cr0 || shard->own_row1 != geo.cr1))
    return set_error(p->ctx, SRMAP_EINVAL, "row shard: owned rows must equal the problem's cost rows");
  if ((mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) &&
      (shard->own_ch0 < 0 || shard->own_ch1 > C || shard->own_ch0 >= shard->own_ch1))
    return set_error(p->ctx, SRMAP_EINVAL, "channel shard: bad owned channel range");
  if (mode == SRMAP_SHARD_GRID && (shard->frame_groups < 1 || comm_world(comm) % shard->frame_groups != 0 ||
                                   (shard->frame_groups > 1 && !shard->frame_comm)))
    return set_error(p->ctx, SRMAP_EINVAL, "grid shard: frame_groups must divide the world size and frame_comm must be given");
  // GRID: the unknowns of a channel block are replicated over its frame groups; group 0 counts them in the reductions
  const bool grid_replica = mode == SRMAP_SHARD_GRID && shard->frame_groups > 1 && (comm_rank(comm) % shard->frame_groups) != 0;
  const int per_split = opt->split_channels ? 1 : C;
  const int rounds = C / per_split;
  const size_t npts = (size_t)per_split * N;
  srmap_irls_options o = *opt;
  double lambda_sum = 0.0;
  for (int r = 0; r < p->nreg; ++r) lambda_sum += p->reg[r].lambda;
  {  // AdjustThresholdsAdaptively (map_solver.cpp:16-26, irls_map_solver.cpp:161-171) on the JOINT problem size
    double params = (double)(int)npts;
    if (mode == SRMAP_SHARD_ROWS || mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) {
      double own = mode == SRMAP_SHARD_ROWS ? (double)C * geo.W * (shard->own_row1 - shard->own_row0)
                                            : (grid_replica ? 0.0 : (double)(shard->own_ch1 - shard->own_ch0) * N);
      // every rank must derive the same thresholds: total parameter count = sum of the owned counts
      DevBuf tmp;
      SRMAP_HIP(p->ctx, tmp.alloc(sizeof(double)));
      SRMAP_HIP(p->ctx, hipMemcpy(tmp.as(), &own, sizeof(double), hipMemcpyHostToDevice));
      if (int rc0 = comm_allreduce(comm, tmp.as(), 1, SRMAP_F64, 0, p->ctx->stream)) return rc0;
      SRMAP_HIP(p->ctx, hipStreamSynchronize(p->ctx->stream));
      SRMAP_HIP(p->ctx, hipMemcpy(&own, tmp.as(), sizeof(double), hipMemcpyDeviceToHost));
      params = (double)(int)own;
    }
    const double scale = params * lambda_sum;
    if (!(scale < 1.0)) {
      o.gradient_norm_threshold *= scale;
      o.cost_decrease_threshold *= scale;
      o.parameter_variation_threshold *= scale;
      o.irls_cost_difference_threshold *= scale;
    }
  }
  srmap_solve_report rep = {0, 0, 0, 0, 0.0, 0.0, 0.0, 0};
  hipStream_t st = p->ctx->stream;
  DeviceCG<T> cg;
  cg.p = p; cg.st = st; cg.n = npts; cg.comm = comm; cg.shard = shard;
  cg.chain_enabled = o.host_paced_passes == 0;
  cg.fold_enabled = o.host_paced_passes == 0;
  cg.ow.on = 0; cg.ow.e0 = 0; cg.ow.e1 = npts; cg.ow.W = geo.W; cg.ow.H = geo.H; cg.ow.r0 = 0; cg.ow.r1 = geo.H;
  if (mode == SRMAP_SHARD_ROWS) { cg.ow.on = 1; cg.ow.r0 = shard->own_row0; cg.ow.r1 = shard->own_row1; cg.reduce_scalars = true; }
  if (mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) {
    cg.ow.on = 1; cg.ow.e0 = (size_t)shard->own_ch0 * N; cg.ow.e1 = grid_replica ? cg.ow.e0 : (size_t)shard->own_ch1 * N;
    cg.reduce_scalars = true;
  }
  int rc = cg.alloc();
  if (rc == SRMAP_OK && lbfgs) rc = cg.alloc_lbfgs(p->lbfgs_m);
  if (rc == SRMAP_OK && huber && !p->dw.effective<T>()) rc = set_error(p->ctx, SRMAP_EINVAL, "internal: a Huber loss without its weight buffer");
  // IRLS weights live in the problem's RegSpec (full [C][H][W]); make sure they exist.
  for (int r = 0; r < p->nreg && rc == SRMAP_OK; ++r) {
    if (!p->reg[r].weights && p->reg[r].weights.alloc(p->hr_count() * sizeof(T)) != hipSuccess)
      rc = set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed");
  }
  for (int round = 0; round < rounds && rc == SRMAP_OK; ++round) {
    const int c0 = round * per_split;
    if (opt->split_channels) { cg.view.c0 = c0; cg.view.C = per_split; }
    Geometry vg = geo;
    vg.C = per_split;
    // the start: the caller's host doubles rounded to the dtype, or (solve_device) an image that already holds them so
    if (!x0_dev) rc = convert_upload(p, x0 + (size_t)c0 * N, cg.x, npts, st);
    else if (hipMemcpyAsync(cg.x, (const T*)x0_dev + (size_t)c0 * N, npts * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess)
      rc = set_error(p->ctx, SRMAP_EHIP, "solve: the copy of the start failed: %s", hipGetErrorString(hipGetLastError()));
    if (rc) break;
    // w <- 1  (irls_map_solver.cpp:66-74)
    for (int r = 0; r < p->nreg; ++r)
      launch_fill<T>(p->reg[r].weights.as<T>() + (size_t)c0 * N, T(1), npts, st);
    if (huber) {  // the data weights of this round's channels likewise, or to their prior
      rc = p->dw.reset(p, c0, per_split, st);
      if (rc) break;
    }
    double previous_cost = INFINITY;
    double cost_difference = o.irls_cost_difference_threshold + 1.0;
    int ran = 0;
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    const auto t_loop0 = std::chrono::steady_clock::now();
    while (std::fabs(cost_difference) >= o.irls_cost_difference_threshold) {
      CgResult cr;
      rc = lbfgs ? run_lbfgs(cg, o.gradient_norm_threshold, o.cost_decrease_threshold, o.parameter_variation_threshold,
                             o.max_num_solver_iterations, &cr, nullptr)
                 : run_cg(cg, o.gradient_norm_threshold, o.cost_decrease_threshold, o.parameter_variation_threshold,
                          o.max_num_solver_iterations, &cr, nullptr);
      if (rc) break;
      rep.cg_iterations += cr.its;
      rep.last_termination = cr.type;
      rep.final_cost = cr.f;
      if (p->nreg == 0 && !huber) { ran++; break; }
      // w = 1/max(1e-5, reg(x)), :128-143 -- on fresh halos (the weights of a halo plane / halo rows feed the
      // owned gradient through the neighbour terms)
      rc = shard_exchange_x(p, comm, mode == SRMAP_SHARD_NONE ? nullptr : shard, cg.x, st);
      if (rc) break;
      for (int r = 0; r < p->nreg; ++r) {
        rc = launch_reg_weights<T>(p, vg, p->reg[r], (const T*)cg.x, p->reg[r].weights.as<T>() + (size_t)c0 * N, st);
        if (rc) break;
      }
      if (rc) break;
      // Huber: the data weights from the residuals at the same iterate
      if (huber) rc = p->dw.huber_step(p, c0, per_split, cg.x, st);
      if (rc) break;
      cost_difference = previous_cost - cr.f;
      previous_cost = cr.f;
      ran++;
      if (o.max_num_irls_iterations > 0 && ran >= o.max_num_irls_iterations) break;
    }
    if (rc) break;
    (void)hipStreamSynchronize(st);
    rep.loop_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop0).count();
    rep.irls_rounds += ran;
    rc = shard_exchange_x(p, comm, mode == SRMAP_SHARD_NONE ? nullptr : shard, cg.x, st);  // x_out carries valid halos
    if (rc) break;
    if (x_out_dev) {
      if (hipMemcpyAsync((T*)x_out_dev + (size_t)c0 * N, cg.x, npts * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        rc = set_error(p->ctx, SRMAP_EHIP, "solve: the copy of the result failed: %s", hipGetErrorString(hipGetLastError()));
    } else {
      rc = convert_download(p, cg.x, x_out + (size_t)c0 * N, npts, st);
    }
  }
  rep.evaluations = cg.evaluations;
  rep.wait_seconds = cg.wait_seconds;
  rep.waits = cg.waits;
  rc = cg.recover_timeout(rc);
  if (report) *report = rep;
  return rc;
}

// One nonlinear-CG run (no IRLS re-weighting) with the f of every evaluation recorded: the trajectory the tests
// compare with ALGLIB's mincg on the same objective (tests/test_gpu_parity.py).  lbfgs_m > 0: one L-BFGS run with that
// history instead (minlbfgs; tests/test_gpu_lbfgs.py).
template <typename T>
static int cg_trace_typed(srmap_problem* p, int lbfgs_m, double epsg, double epsf, double epsx, int maxits, const double* x0,
                          double* x_out, int* iterations, int* nfev, int* termination, double* f_trace, int trace_cap,
                          int* trace_len) {
  const size_t npts = p->hr_count();
  DeviceCG<T> cg;
  cg.p = p; cg.st = p->ctx->stream; cg.n = npts;
  cg.ow.on = 0; cg.ow.e0 = 0; cg.ow.e1 = npts; cg.ow.W = p->geo.W; cg.ow.H = p->geo.H; cg.ow.r0 = 0; cg.ow.r1 = p->geo.H;
  int rc = cg.alloc();
  if (rc == SRMAP_OK && lbfgs_m > 0) rc = cg.alloc_lbfgs(lbfgs_m);
  if (rc == SRMAP_OK) rc = convert_upload(p, x0, cg.x, npts, cg.st);
  CgResult cr;
  std::vector<double> tr;
  if (rc == SRMAP_OK) rc = lbfgs_m > 0 ? run_lbfgs(cg, epsg, epsf, epsx, maxits, &cr, &tr) : run_cg(cg, epsg, epsf, epsx, maxits, &cr, &tr);
  if (rc == SRMAP_OK) rc = convert_download(p, cg.x, x_out, npts, cg.st);
  rc = cg.recover_timeout(rc);
  if (rc) return rc;
  if (iterations) *iterations = cr.its;
  if (nfev) *nfev = cr.nfev;
  if (termination) *termination = cr.type;
  const int m = (int)tr.size() < trace_cap ? (int)tr.size() : trace_cap;
  for (int i = 0; i < m; ++i) f_trace[i] = tr[i];
  if (trace_len) *trace_len = (int)tr.size();
  return SRMAP_OK;
}

}  // namespace srmap

using namespace srmap;

extern "C" {

int srmap_cg_trace(srmap_problem* p, double epsg, double epsf, double epsx, int maxits, const double* x0, double* x_out,
                   int* iterations, int* nfev, int* termination, double* f_trace, int trace_cap, int* trace_len) {
  if (!p || !x0 || !x_out || (trace_cap > 0 && !f_trace)) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  return dispatch_dtype(p->dtype, [&](auto t) {
    return cg_trace_typed<decltype(t)>(p, 0, epsg, epsf, epsx, maxits, x0, x_out, iterations, nfev, termination, f_trace, trace_cap, trace_len);
  });
}

int srmap_lbfgs_trace(srmap_problem* p, int m, double epsg, double epsf, double epsx, int maxits, const double* x0,
                      double* x_out, int* iterations, int* nfev, int* termination, double* f_trace, int trace_cap,
                      int* trace_len) {
  if (!p || !x0 || !x_out || (trace_cap > 0 && !f_trace)) return SRMAP_EINVAL;
  if (m < 1) return set_error(p->ctx, SRMAP_EINVAL, "num_lbfgs_hessian_corrections must be >= 1 (got %d)", m);
  if (m > kLbfgsMaxM) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "num_lbfgs_hessian_corrections %d: at most %d are supported", m, kLbfgsMaxM);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  return dispatch_dtype(p->dtype, [&](auto t) {
    return cg_trace_typed<decltype(t)>(p, m, epsg, epsf, epsx, maxits, x0, x_out, iterations, nfev, termination, f_trace, trace_cap, trace_len);
  });
}

void srmap_irls_options_default(srmap_irls_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_irls_options);
  o->max_num_solver_iterations = 50;
  o->gradient_norm_threshold = 1.0e-6;
  o->cost_decrease_threshold = 1.0e-6;
  o->parameter_variation_threshold = 1.0e-6;
  o->split_channels = 0;
  o->max_num_irls_iterations = 20;
  o->irls_cost_difference_threshold = 1.0e-5;
  o->host_paced_passes = 0;
}

}  // extern "C"

namespace srmap {

int irls_options_in_force(srmap_problem* p, const srmap_irls_options* options, srmap_irls_options* out) {
  srmap_irls_options& o = *out;
  if (options) {
    // the first member is the size of the struct the caller was compiled with: another layout is refused, not guessed at
    if (options->struct_size != (int)sizeof(srmap_irls_options))
      return set_error(p->ctx, SRMAP_EINVAL, "srmap_irls_options: struct_size %d, this library expects %d (fill the struct with "
                       "srmap_irls_options_default() of the matching include/srmap.h)", options->struct_size, (int)sizeof(srmap_irls_options));
    o = *options;
  } else {
    srmap_irls_options_default(&o);
  }
  return SRMAP_OK;
}

int solve_device(srmap_problem* p, const srmap_irls_options* opt, const void* x0_dev, void* x_out_dev, srmap_solve_report* report) {
  return dispatch_dtype(p->dtype, [&](auto t) {
    return solve_typed<decltype(t)>(p, nullptr, nullptr, opt, nullptr, nullptr, report, x0_dev, x_out_dev);
  });
}

}  // namespace srmap

extern "C" {

int srmap_solve_sharded(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard,
                        const srmap_irls_options* options, const double* x0, double* x_out,
                        srmap_solve_report* report) {
  if (!p || !x0 || !x_out) return SRMAP_EINVAL;
  srmap_irls_options o;
  if (int rc = irls_options_in_force(p, options, &o)) return rc;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return dispatch_dtype(p->dtype, [&](auto t) { return solve_typed<decltype(t)>(p, comm, shard, &o, x0, x_out, report); });
}

int srmap_problem_selfcheck(const srmap_problem* p, double* beta_denominator_rel_dev) {
  if (!p || !beta_denominator_rel_dev) return SRMAP_EINVAL;
  *beta_denominator_rel_dev = p->selfcheck_beta_den;
  return SRMAP_OK;
}

int srmap_solve(srmap_problem* p, const srmap_irls_options* options, const double* x0, double* x_out,
                srmap_solve_report* report) {
  return srmap_solve_sharded(p, nullptr, nullptr, options, x0, x_out, report);
}

}  // extern "C"
