// solver.hip -- IRLSMapSolver::Solve on the GPU (irls_map_solver.cpp:45-157, 192-265): the IRLS outer loop
// (solve_typed) around either inner minimiser of the reference, paced by the host -- L-BFGS (run_lbfgs, minlbfgs) or
// the nonlinear CG the reference obtains from ALGLIB 3.10.0 (run_cg; mincg, default settings: DY/HS hybrid beta,
// More'-Thuente line search, libs/alglib/src/optimization.cpp:17137-17880, alglibinternal.cpp:12313-12632) --
// single-GPU or sharded over one rank per GPU, and the single-run trace entry points.
//
// This file is the control flow only.  Every n-vector lives in HBM and is touched only by the passes
// (solver_passes.hip, kernels_lbfgs.hip) and the evaluation (shard_eval.hip); DeviceCG owns the vectors and queues the
// passes, its Mailbox owns the scalars the device and the host exchange (the slot map: solver_mailbox.hpp), hands out the
// arrival tags and waits on them.  Step selection and the stopping rules run on the host, in double, in ALGLIB's
// order of operations (solver_host.hpp: the More'-Thuente step, the L-BFGS recursion on coefficients), so that the
// trajectory follows the reference's up to reduction order.  Per CG iteration the host waits for the device 2 + nfev
// times: once for the direction's sums, once per trial point for (f, g.d), once for the beta dot products.
//
// Sharding.  The passes reduce over the elements a rank OWNS and the Mailbox all-reduces the sums through the
// communicator (sum, and max for the max-norm), so every rank takes the same decisions; x halos are refreshed before
// every evaluation (comm.hpp).
#include <chrono>
#include <cmath>
#include <utility>
#include <vector>

#include "cg_norm.hpp"
#include "comm.hpp"
#include "solver_host.hpp"
#include "solver_passes.hpp"

namespace srmap {

static_assert(kHsPubF - kHsPass == kCostValue && kHsPubGd - kHsPass == kCostGd, "a published {f, g.d} pair is d_cost's head");

// GRID: the unknowns of a channel block are replicated over its frame groups; group 0 counts them in the reductions
static bool grid_replica(const srmap_comm* comm, const srmap_shard_desc* shard) {
  return shard_mode(comm, shard) == SRMAP_SHARD_GRID && shard->frame_groups > 1 && (comm_rank(comm) % shard->frame_groups) != 0;
}

// ---------------------------------------------------------------------------------------------------------
// The host's one owner of the scalar protocol of solver_mailbox.hpp (the table there: who writes which word under which
// tag).  One-launch scheme (fused(): the sums need no all-reduce): a pass's last workgroup publishes (struct Fin).
// Two-launch scheme: finish / finish_dir reduce the block partials, all-reduce and publish.
struct Mailbox {
  srmap_problem* p = nullptr;
  hipStream_t st = nullptr;
  srmap_comm* comm = nullptr;          // the scalar all-reduces of the two-launch scheme
  bool reduce_scalars = false;         // row / channel shards: the owned-element sums are all-reduced
  double* hs = nullptr;                // ctx->h_scal, host-mapped [kHsSlots]
  double* dscal = nullptr;             // device scalars [kDsSlots]
  double* part = nullptr;              // [3][kRedBlocks] block partials (two-launch scheme)
  unsigned long long* gran = nullptr;  // [3][kRedBlocks] granules of the one-launch reductions (armed)
  DevBuf dscal_mem, part_mem, gran_mem;
  double tag = 0, dir_tag = 0;         // the last tag handed to a publishing kernel; the last direction pass's
  double wait_seconds = 0;             // host time spent in wait_tag
  int waits = 0;

  bool fused() const { return !reduce_scalars; }
  double next_tag() { return tag += 1.0; }
  const double* cost() const { return p->d_cost.as<double>(); }

  int alloc() {
    constexpr size_t kGranules = 3 * (size_t)kRedBlocks, kArmWords = sizeof(*gran) / sizeof(kArm32);
    SRMAP_HIP(p->ctx, part_mem.alloc(sizeof(*part) * 3 * kRedBlocks));
    SRMAP_HIP(p->ctx, dscal_mem.alloc(sizeof(*dscal) * kDsSlots));
    SRMAP_HIP(p->ctx, gran_mem.alloc(sizeof(*gran) * kGranules));
    part = part_mem.as<double>(); dscal = dscal_mem.as<double>(); gran = gran_mem.as<unsigned long long>();
    SRMAP_HIP(p->ctx, hipMemsetAsync(dscal, 0, sizeof(*dscal) * kDsSlots, st));
    SRMAP_HIP(p->ctx, hipMemsetD32Async((hipDeviceptr_t)gran, (int)kArm32, kGranules * kArmWords, st));
    if (int rc = ensure_staging(p->ctx)) return rc;
    hs = p->ctx->h_scal.as<double>();
    return SRMAP_OK;
  }
  // behind alloc and a stream synchronisation: this solve's time-out word (Fin::timeout_host, ZArgs::to_host) starts clear,
  // its tags go on from the context's last -- they keep increasing across solves, so a stale word can never match
  void open() { hs[kHsTimeout] = 0.0; tag = hs[kHsTag]; }

  // Wait until the kernel that was given tag `want` (default: the last one handed out) has published its results:
  // poll_tag on the host-mapped words, and after ~2 s a stream synchronisation (also surfaces asynchronous errors).
  int wait_tag(double want = -1.0) {
    if (want < 0) want = tag;
    const volatile double* slot = hs + kHsTag;
    using Clock = std::chrono::steady_clock;
    struct Acc { Mailbox* c; Clock::time_point t; ~Acc() {
      c->wait_seconds += std::chrono::duration<double>(Clock::now() - t).count(); c->waits++; } } acc{this, Clock::now()};
    switch (poll_tag(slot, hs + kHsTimeout, want, 2.0)) {
      case Arrival::kArrived: break;
      case Arrival::kDeviceTimeout:  // its sums are NaN, its granules not re-armed
        return set_error(p->ctx, SRMAP_EHIP, "solver: a device-side reduction timed out waiting for a workgroup");
      case Arrival::kExpired:
        SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
        if (!tag_arrived(slot, want)) return set_error(p->ctx, SRMAP_EHIP, "solver: device results did not arrive");
    }
    return SRMAP_OK;
  }
  // the sums of the last direction pass on the host: {max|dn|, dn.dn, g.dn}
  int wait_dir(double* mx, double* ss, double* gdn) {
    const int rc = wait_tag(dir_tag);
    if (rc) return rc;
    *mx = hs[kHsDir + kDirMax]; *ss = hs[kHsDir + kDirSs]; *gdn = hs[kHsDir + kDirGdn];
    return SRMAP_OK;
  }

  // Where the pass about to be launched leaves its sums.  One-launch scheme: under the next tag, in h_scal's pass words
  // (+ the cost behind them) or, a direction pass (dir), in dscal's direction words under dir_tag, f published beside them
  // (publish_f).  Two-launch scheme: empty -- block partials; finish / finish_dir follows.
  Fin fin(bool with_cost, bool dir = false, bool publish_f = false) {
    Fin f{};
    if (!fused()) return f;
    f.gran = gran; f.out = dir ? dscal + kDsDir : hs + kHsPass; f.cost_src = with_cost ? cost() : nullptr;
    if (publish_f) { f.pub_src = cost() + kCostValue; f.pub_dst = hs + kHsPubF; f.pub_n = 1; }
    f.timeout_flag = dscal + kDsTimeout; f.timeout_host = hs + kHsTimeout;
    f.tag_slot = hs + kHsTag; f.tag = next_tag();
    if (dir) dir_tag = tag;
    return f;
  }
  // What an evaluation's finish kernel may publish itself: {f, g.d} (with_gd, and no scalar all-reduce) and the next
  // tag.  The tag is taken (next_tag) only when the evaluation reports that it published.
  EvalReq::Publish offer(bool with_gd) const {
    return {(fused() && with_gd) ? hs + kHsPubF : nullptr, hs + kHsTag, tag + 1.0, hs + kHsTimeout};
  }
  // Behind a reducing pass of nb workgroups, what brings its `rows` sums (+ the cost behind them) to h_scal's pass words.
  // One-launch scheme: nothing, the pass does.  Two-launch scheme: k_finish over the partial rows, the all-reduce, the
  // publish under the next tag; with_dir: the direction's sums (already reduced in dscal) ride along under that tag.
  int queue_finish(int nb, int rows, bool with_cost, bool with_dir = false) {
    const int cnt = rows + (with_cost ? 1 : 0);
    if (!fused()) {
      next_tag();
      launch_finish(part, nb, rows, 0, dscal + kDsPass, with_cost ? cost() : nullptr, nullptr, 0.0, st);
      if (int rc = comm_allreduce(comm, dscal + kDsPass, (size_t)cnt, SRMAP_F64, 0, st)) return rc;
      if (with_dir) launch_publish(hs + kHsDir, dscal + kDsDir, kDirWords, hs + kHsSideTag, 0.0, st);
      launch_publish(hs + kHsPass, dscal + kDsPass, cnt, hs + kHsTag, tag, st);
      if (with_dir) dir_tag = tag;
    }
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // queue_finish, one wait, and the sums on the host: out[0..rows) (+ out[rows] = cost)
  int finish(int nb, int rows, bool with_cost, double* out, bool with_dir = false) {
    int rc = queue_finish(nb, rows, with_cost, with_dir);
    if (rc == SRMAP_OK) rc = wait_tag();
    if (rc) return rc;
    for (int i = 0; i < rows + (with_cost ? 1 : 0); ++i) out[i] = hs[kHsPass + i];
    return SRMAP_OK;
  }
  // Two-launch scheme, behind a direction pass: its three partial rows -> dscal's direction words, all-reduced;
  // publish: to the host under a tag of their own (else the caller's finish(with_dir) carries them)
  int finish_dir(int nb, bool publish) {
    double* d = dscal + kDsDir;
    launch_finish(part, nb, kDirWords, 1, d, nullptr, nullptr, 0.0, st);
    int rc = comm_allreduce(comm, d + kDirMax, 1, SRMAP_F64, 1, st);
    if (rc) return rc;
    rc = comm_allreduce(comm, d + kDirSs, 2, SRMAP_F64, 0, st);
    if (rc) return rc;
    if (publish) {
      dir_tag = next_tag();
      launch_publish(hs + kHsDir, d, kDirWords, hs + kHsTag, tag, st);
    }
    return SRMAP_OK;
  }
  // The {f, g.d} an evaluation left in d_cost, to the host under the next tag (all-reduced first where sums are)
  int publish_f_gd() {
    next_tag();
    const double* src = cost();
    if (reduce_scalars) {
      SRMAP_HIP(p->ctx, hipMemcpyAsync(dscal + kDsPass, src, 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
      int rc = comm_allreduce(comm, dscal + kDsPass, 2, SRMAP_F64, 0, st);
      if (rc) return rc;
      src = dscal + kDsPass;
    }
    launch_publish(hs + kHsPubF, src, 2, hs + kHsTag, tag, st);
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // End of a solve or trace: a reduction that gave up waiting for a workgroup (the tile kernel's in-kernel finish:
  // sticky word d_cost[kCostTimeout]; a CG pass: dscal[kDsTimeout]) left NaN sums behind -- the stopping rules ended the
  // run -- and its granules un-re-armed.  wait_tag ends the run on hs[kHsTimeout], which both kinds of finisher raise:
  // look now, re-initialise, report.  No device copy on success.
  int recover_timeout(int rc) {
    (void)hipStreamSynchronize(st);
    if (hs == nullptr || hs[kHsTimeout] == 0.0) return rc;
    const int rr = recover_reduction_timeout(p, hs + kHsTimeout);
    if (rc != SRMAP_OK) return rc;
    return rr ? rr : set_error(p->ctx, SRMAP_EHIP, "a device-side reduction timed out waiting for a workgroup during the solve (device fault or a wedged queue)");
  }
};

// What both runs need of the direction's sums at the opening of an iteration (DeviceCG::begin_step)
struct StepNorms { double dginit, dd, gdn, s1, s2; };

template <typename T>
struct DeviceCG {
  srmap_problem* p = nullptr;
  hipStream_t st = nullptr;
  size_t n = 0;
  const srmap_shard_desc* shard = nullptr;
  Mailbox mb;
  Owned ow{};
  EvalReq::View view;           // channel view of every evaluation (split_channels)
  bool gd_valid = false;        // the last evaluation left g.d in d_cost[kCostGd]
  bool published = false;       // the last evaluation's finish kernel published {f, g.d} + tag (fetch_f_gd just waits)
  // chained passes (run_cg): launches whose inputs are already on the device are queued without waiting for the host.
  // srmap_irls_options::host_paced_passes turns this off (every pass then waits for the host's answer, as up to
  // round 3): same arithmetic, same results bit for bit -- tests/test_gpu_solve_parity.py compares the two.  Chaining
  // applies to un-sharded solves only: under frame sharding a speculative first-trial evaluation would queue a
  // gradient + cost all-reduce that every rank has to match before the host has decided to keep it.
  bool chain_enabled = true;
  bool chained() const { return mb.fused() && chain_enabled && (shard == nullptr || mb.comm == nullptr); }
  // the line search may hand its trial point to the evaluation as (xk, stp): un-sharded solves on the tile kernel's
  // g.d instance (ztile_can_fold); decided once per run (begin_run).  fold_enabled: srmap_irls_options::host_paced_passes
  // also forms every trial point by its own pass (the A/B of the fold)
  bool foldable = false, fold_enabled = true;
  // x, g: current point and gradient; xk/dk: accepted point and direction; dn: next direction; d: normalised direction
  // (stored only where evaluations read it from memory: !foldable); gp: the gradient at xk while the line search writes its
  // trial gradients to g (the two buffers swap; mincg's yk = g_{k+1} - g_k is formed on the fly).  The line-search base is xk.
  T *x = nullptr, *g = nullptr, *xk = nullptr, *dk = nullptr, *dn = nullptr, *d = nullptr, *gp = nullptr;
  int evaluations = 0;
  // L-BFGS (run_lbfgs, kernels_lbfgs.hip): ring of lb_m pairs S[j] = s_j, Y[j] = y_j ([lb_m][n] each), the passes'
  // workgroup partials and ticket, and the update pass's kLbRows sums (host-mapped, a buffer of their own)
  int lb_m = 0;
  T *S = nullptr, *Y = nullptr;
  double* lb_part = nullptr;
  unsigned* lb_ticket = nullptr;
  double* lb_host = nullptr;
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

  int nb() const { size_t b = (n + 255) / 256; return (int)(b < (size_t)kRedBlocks ? b : kRedBlocks); }

  // The solver of problem p_ over n_ unknowns, this rank's shard of them: the owned elements, the reduction scheme, every
  // buffer (lbfgs_m > 0: the ring too).  opt == nullptr (the traces): chained and folded.
  int init(srmap_problem* p_, srmap_comm* comm, const srmap_shard_desc* shard_, size_t n_, const srmap_irls_options* opt,
           int lbfgs_m) {
    p = p_; st = p->ctx->stream; n = n_; shard = shard_;
    mb.p = p; mb.st = st; mb.comm = comm;
    if (opt) chain_enabled = fold_enabled = opt->host_paced_passes == 0;
    const Geometry& geo = p->geo;
    const size_t N = (size_t)geo.W * geo.H;
    const int mode = shard_mode(comm, shard);
    ow.on = 0; ow.e0 = 0; ow.e1 = n; ow.W = geo.W; ow.H = geo.H; ow.r0 = 0; ow.r1 = geo.H;
    if (mode == SRMAP_SHARD_ROWS) { ow.on = 1; ow.r0 = shard->own_row0; ow.r1 = shard->own_row1; }
    if (mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) {
      ow.on = 1; ow.e0 = (size_t)shard->own_ch0 * N; ow.e1 = grid_replica(comm, shard) ? ow.e0 : (size_t)shard->own_ch1 * N;
    }
    mb.reduce_scalars = ow.on != 0;
    T** v[] = {&x, &g, &xk, &dk, &dn, &d, &gp};
    for (T** q : v)
      if (int rc = dev_alloc(q, n * sizeof(T))) return rc;
    if (int rc = mb.alloc()) return rc;
    // sharded evaluations write only the owned part of g: the vector kernels run over all n elements, so everything
    // they combine starts defined (the halo values never enter a reduction, and x halos are re-exchanged)
    T* z[] = {g, dn, d, dk, gp};
    for (T* q : z) SRMAP_HIP(p->ctx, hipMemsetAsync(q, 0, n * sizeof(T), st));
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    mb.open();
    return lbfgs_m > 0 ? alloc_lbfgs(lbfgs_m) : SRMAP_OK;
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
  // objective at x: g <- gradient; the cost stays on the device (Mailbox::finish(with_cost) fetches it).  With a direction
  // the tile kernel may produce g.d in the same pass (gd_valid; not under frame sharding: the local gradient is a partial sum).
  int evaluate(const T* dir = nullptr, T* at = nullptr, const T* fold_xk = nullptr, double fold_stp = 0.0) {  // at: the point (default x)
    evaluations++;
    const int mode = shard_mode(mb.comm, shard);
    EvalReq req;
    req.view = view;
    req.dvec = (mode == SRMAP_SHARD_FRAMES || mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) ? nullptr : dir;
    // without a scalar all-reduce the evaluation's finish kernel can publish {f, g.d} and the arrival tag itself
    req.pub = mb.offer(req.dvec != nullptr);
    // fold: `dir` is the UNNORMALISED direction dk; the kernel scales it by the factors it derives from the norms the
    // direction pass left in dscal's direction words (norm_factors / norm_elem: the bits of the stored d)
    if (fold_xk != nullptr && req.dvec != nullptr) req.fold = {fold_xk, req.dvec, fold_stp, (const double*)(mb.dscal + kDsDir)};
    EvalOut out;
    const int rc = shard_eval(p, mb.comm, shard, req, &out, SRMAP_TERM_ALL, at ? at : x, g, st);
    gd_valid = out.gd_valid;
    published = out.published;
    if (published) mb.next_tag();
    return rc;
  }
  // The evaluation queued ahead of the host's decision (run_cg: the first trial point behind the normalisation pass)
  // turned out not to be wanted: it is not one of the solve's evaluations and nobody fetches its sums.  Its tag, if it
  // publishes one, is simply passed over (wait_tag compares with >=).
  void discard_speculative() {
    evaluations--;
    published = false;
  }
  // f and g.d of the evaluation just made, with one wait: out[0] = g.d, out[1] = f
  int fetch_f_gd(double* out) {
    int i_gd = kHsPubGd, i_f = kHsPubF, rc = SRMAP_OK;
    if (!gd_valid) {  // g.d by a pass of its own: its one row, the cost forwarded behind it
      launch_cg_dot<T>(g, d, n, ow, mb.part, mb.fin(true), nb(), st);
      rc = mb.queue_finish(nb(), 1, true);
      i_gd = kHsPass; i_f = kHsPass + 1;
    } else if (published) {
      published = false;  // the evaluation's own finish kernel carries the tag
    } else {
      rc = mb.publish_f_gd();
    }
    if (rc == SRMAP_OK) rc = mb.wait_tag();
    if (rc) return rc;
    out[0] = mb.hs[i_gd];
    out[1] = mb.hs[i_f];
    return SRMAP_OK;
  }
  // dn = -g + beta dk (dk may be null); {max|dn|, dn.dn, g.dn} -> dscal's direction words (device, all-reduced) and, under
  // dir_tag (Mailbox::wait_dir), h_scal's.  publish_cost: the first pass of a run also hands f to the host (one-launch
  // scheme: with the same tag; two-launch scheme: the caller's finish(with_dir) publishes all four).
  // beta_dev: beta comes from the device scalar the k_beta_dots queued just before left there (one-launch scheme only)
  int direction(const T* dk_or_null, double beta, bool publish_cost = false, const double* beta_dev = nullptr) {
    const Fin f = mb.fin(false, true, publish_cost);
    double* npub = mb.fused() ? mb.hs + kHsDir : (double*)nullptr;
    launch_cg_direction<T>(dn, g, dk_or_null, (T)beta, n, ow, mb.part, f, beta_dev, npub, foldable ? 1 : 0, nb(), st);
    if (!mb.fused())
      if (int rc = mb.finish_dir(nb(), !publish_cost)) return rc;
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // L-BFGS: ring slot p <- (x - xk, g - gk) and the Gram rows of the new pair (launch_lbfgs_update) -> lb_host, one wait
  int lbfgs_update(const T* gk, int p_slot, int live) {
    const LbfgsRed red{lb_part, lb_ticket, nullptr, lb_host, mb.hs + kHsTag, mb.next_tag()};
    int rc = launch_lbfgs_update<T>(x, xk, g, gk, S, Y, p_slot, live, n, nb(), red, st);
    if (rc) return set_error(p->ctx, rc, "lbfgs: bad history length");
    SRMAP_HIP(p->ctx, hipGetLastError());
    return mb.wait_tag();
  }
  // L-BFGS: dn from the coefficients over {g, S[0..live), Y[0..live)}; its sums where `direction` leaves them, under dir_tag
  int lbfgs_direction(const LbfgsCoef& c, int live) {
    mb.dir_tag = mb.next_tag();
    const LbfgsRed red{lb_part, lb_ticket, mb.dscal + kDsDir, mb.hs + kHsDir, mb.hs + kHsTag, mb.tag};
    int rc = launch_lbfgs_direction<T>(dn, g, S, Y, live, c, n, nb(), foldable ? 1 : 0, red, st);
    if (rc) return set_error(p->ctx, rc, "lbfgs: bad history length");
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // d = dk s1 s2 stored as a vector (+ the first trial point x = xk + stp1 d when stp1 != 0): the paths whose evaluations
  // read the normalised direction from memory
  int normalize(double stp1) {
    launch_cg_normalize<T>(d, dk, mb.dscal + kDsDir, n, xk, stp1 != 0.0 ? x : (T*)nullptr, (T)stp1, nb(), st);
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // The opening of a run (run_cg, run_lbfgs): evaluate at the start point, dk = -g with its sums, and f and g.g = dk.dk
  // on the host after one wait.  *small_g: the epsg rule already holds (the caller ends the run with x = xk).
  int begin_run(double epsg, double* f, double* gg, bool* small_g, std::vector<double>* trace) {
    // the start point becomes the base point xk by exchanging the two buffers (no copy); x is trial scratch from here on:
    // every path of a run writes it before reading it (the trial points) or copies xk back into it (the early exits)
    std::swap(xk, x);
    foldable = shard_mode(mb.comm, shard) == SRMAP_SHARD_NONE && fold_enabled && ztile_can_fold(p, view.C > 0 ? view.C : p->geo.C);
    int rc = evaluate(nullptr, xk);
    if (rc) return rc;
    // dk = -g (written as dn, swapped below), norms of dk
    rc = direction(nullptr, 0.0, true);
    if (rc) return rc;
    if (mb.fused()) {  // the direction pass published f and {max|dk|, dk.dk, g.dk} itself
      rc = mb.wait_tag();
      if (rc) return rc;
      *f = mb.hs[kHsPubF];
    } else {  // fetch f and the direction's sums (already reduced on the device) with one wait
      rc = mb.finish(nb(), 0, true, f, true);
      if (rc) return rc;
    }
    *gg = mb.hs[kHsDir + kDirSs];  // g.g = dk.dk
    if (trace) trace->push_back(*f);
    std::swap(dk, dn);
    *small_g = std::sqrt(*gg) <= epsg;
    return SRMAP_OK;
  }
  // The opening of an iteration, behind the pass that stores d where one is needed (normalize): wait for the direction's
  // sums; linminnormalized's factors (cg_norm.hpp), g.d and d.d of the normalised direction; *stp rescaled as mincg /
  // minlbfgs rescale it.
  int begin_step(double* stp, StepNorms* o) {
    double mx = 0, ss = 0;
    const int rc = mb.wait_dir(&mx, &ss, &o->gdn);
    if (rc) return rc;
    norm_factors(mx, ss, o->s1, o->s2);
    o->dginit = (o->gdn * o->s1) * o->s2;
    o->dd = ((ss * o->s1) * o->s1) * (o->s2 * o->s2);
    if (mx != 0) { *stp = *stp / o->s1; *stp = *stp / o->s2; }
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
  Mailbox& mb = cg.mb;
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
    double stp = 1.0;
    bool pre_launched = false, g_swapped = false;
    // the first step is lastgoodstep unless that is 0 (then it comes from the direction's norms)
    const double stp_pre = (lastgoodstep != 0 && lastgoodstep >= 1.0e-50 && lastgoodstep <= 1.0e+50) ? lastgoodstep : 0.0;
    double stp_ready = 0.0;  // the step whose trial point is already in cg.x and / or whose evaluation is already queued
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
    StepNorms sn;  // g.dk at xk (sn.gdn) and the two scale factors also serve the beta denominator below
    rc = cg.begin_step(&stp, &sn);
    if (rc) return rc;
    if (lastgoodstep != 0) stp = lastgoodstep;
    int mcinfo = 0, nfev = 0;
    if (!g_swapped) std::swap(cg.g, cg.gp);  // gp = gradient at xk; the trial evaluations write g
    double dg_acc = 0;  // g.d at the last trial point
    rc = line_search(cg, &f, sn.dginit, &stp, gtol, &mcinfo, &nfev, trim, trace, stp_ready, pre_launched, &dg_acc);
    if (rc) return rc;
    if (nfev == 0) std::swap(cg.g, cg.gp);  // nothing was evaluated: g stays the gradient at xk, as in mcsrch
    double betak = 0;
    // One-launch scheme: the direction pass is queued right behind the pass that reduces the beta sums -- beta itself is
    // formed by that pass's finishing thread (k_beta_dots) -- and runs while the host waits for the sums it needs for
    // the stopping rules.  (mincg's periodic restart is known beforehand; `direction` was always launched before the
    // rules are looked at.)
    const bool chain = cg.chained();
    const int restart = (res.its > 0 && res.its % (3 + (long long)n) == 0) ? 1 : 0;
    // yk = g - gp ; vv = yk.dk ; betady = g.g/vv ; betahs = g.yk/vv.  vv = g.dk - gp.dk from sums already on the
    // host: gp.dk is the direction pass's g.dn, g.dk = (g.d) / (s2 s1) with the accepted evaluation's g.d (k_beta_dots)
    const double vv = (dg_acc / sn.s2) / sn.s1 - sn.gdn;
    double* beta_dev = (chain && mcinfo == 1) ? mb.dscal + kDsBeta : (double*)nullptr;
    if (mcinfo == 1) {
      // host-paced passes: the pass also sums y.dk directly (one more vector read) and the deviation of the derived
      // denominator from it is recorded (srmap_problem_selfcheck; tests/test_gpu_solve_parity.py)
      const T* dk_chk = chain ? (const T*)nullptr : (const T*)cg.dk;
      launch_cg_beta_dots<T>(cg.gp, cg.g, n, cg.ow, mb.part, mb.fin(false), beta_dev, restart, vv, dk_chk, cg.nb(), cg.st);
    } else {
      launch_cg_dot<T>(cg.g, cg.g, n, cg.ow, mb.part, mb.fin(false), cg.nb(), cg.st);
    }
    double h[3] = {0, 0, 0};  // g.g [, g.y, y.dk summed directly]
    if (chain) {
      const double tag_sums = mb.tag;
      rc = cg.direction(cg.dk, 0.0, false, beta_dev);  // dn (beta from the device, or 0), sums of dn (device)
      if (rc) return rc;
      rc = mb.wait_tag(tag_sums);
      if (rc) return rc;
      h[0] = mb.hs[kHsPass];
    } else {
      rc = mb.finish(cg.nb(), mcinfo == 1 ? 3 : 1, false, h);
      if (rc) return rc;
      if (mcinfo == 1) {
        betak = dmax(0.0, dmin(h[0] / vv, h[1] / vv));
        if (h[2] != 0.0 && std::isfinite(h[2]) && std::isfinite(vv))
          cg.p->selfcheck_beta_den = dmax(cg.p->selfcheck_beta_den, std::fabs(vv - h[2]) / std::fabs(h[2]));
      }
    }
    gg = h[0];
    if (restart) betak = 0;
    if (mcinfo == 1 || mcinfo == 5) rstimer = rscountdownlen; else rstimer -= 1;
    if (!chain) {
      rc = cg.direction(cg.dk, betak);  // dn, norms of dn (device)
      if (rc) return rc;
    }
    const double lastscaledstep = stp * std::sqrt(sn.dd);
    if (mcinfo == 1) lastgoodstep = stp * std::sqrt(sn.dd);
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
    StepNorms sn;
    rc = cg.begin_step(&stp, &sn);
    if (rc) return rc;
    int mcinfo = 0, nfev = 0;
    std::swap(cg.g, cg.gp);  // gp = gradient at xk; the trial evaluations write g
    rc = line_search(cg, &f, sn.dginit, &stp, gtol, &mcinfo, &nfev, trim, trace);
    if (rc) return rc;
    if (nfev == 0) std::swap(cg.g, cg.gp);  // nothing evaluated: x = xk, g the gradient there (s = y = 0)
    if (nfev != 0) nfev_state = nfev;
    res.nfev += nfev_state;
    res.its += 1;
    // sk = x - xk, yk = g - g_k into slot p (ALGLIB writes them whatever mcinfo is) and the Gram rows of the new pair
    rc = cg.lbfgs_update(nfev == 0 ? (const T*)cg.g : (const T*)cg.gp, p, live);
    if (rc) return rc;
    gg = cg.lb_host[kLbGg];
    const double sks = cg.lb_host[kLbSs];
    lbfgs_unpack_rows(cg.lb_host, p, live, m, SY.data(), YY.data(), gs.data(), gy.data());
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

// What a solve over `mode` shards refuses, before any collective
static int check_solve_shard(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard, const srmap_irls_options* opt,
                             int mode) {
  const Geometry& geo = p->geo;
  if (p->solver == SRMAP_SOLVER_LBFGS && mode != SRMAP_SHARD_NONE)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "L-BFGS solves are not sharded over a communicator (its Gram rows would need an all-reduce): run them unsharded, or per channel with split_channels");
  if (int rc = refuse_sharded(p, mode, "solve")) return rc;
  if (mode != SRMAP_SHARD_NONE && opt->split_channels)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "split_channels solves are independent per channel: run them unsharded");
  if (mode == SRMAP_SHARD_ROWS &&
      (shard->own_row0 < 0 || shard->own_row1 > geo.H || shard->own_row0 >= shard->own_row1 ||
       shard->own_row0 != geo.cr0 || shard->own_row1 != geo.cr1))
    return set_error(p->ctx, SRMAP_EINVAL, "row shard: owned rows must equal the problem's cost rows");
  if ((mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) &&
      (shard->own_ch0 < 0 || shard->own_ch1 > geo.C || shard->own_ch0 >= shard->own_ch1))
    return set_error(p->ctx, SRMAP_EINVAL, "channel shard: bad owned channel range");
  if (mode == SRMAP_SHARD_GRID && (shard->frame_groups < 1 || comm_world(comm) % shard->frame_groups != 0 ||
                                   (shard->frame_groups > 1 && !shard->frame_comm)))
    return set_error(p->ctx, SRMAP_EINVAL, "grid shard: frame_groups must divide the world size and frame_comm must be given");
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
  const bool huber = p->dw.loss() == SRMAP_DATA_LOSS_HUBER;
  if (int rc = check_solve_shard(p, comm, shard, opt, mode)) return rc;
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
                                            : (grid_replica(comm, shard) ? 0.0 : (double)(shard->own_ch1 - shard->own_ch0) * N);
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
  DeviceCG<T> cg;
  int rc = cg.init(p, comm, shard, npts, &o, lbfgs ? p->lbfgs_m : 0);
  hipStream_t st = cg.st;
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
  rep.wait_seconds = cg.mb.wait_seconds;
  rep.waits = cg.mb.waits;
  rc = cg.mb.recover_timeout(rc);
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
  int rc = cg.init(p, nullptr, nullptr, npts, nullptr, lbfgs_m);
  if (rc == SRMAP_OK) rc = convert_upload(p, x0, cg.x, npts, cg.st);
  CgResult cr;
  std::vector<double> tr;
  if (rc == SRMAP_OK) rc = lbfgs_m > 0 ? run_lbfgs(cg, epsg, epsf, epsx, maxits, &cr, &tr) : run_cg(cg, epsg, epsf, epsx, maxits, &cr, &tr);
  if (rc == SRMAP_OK) rc = convert_download(p, cg.x, x_out, npts, cg.st);
  rc = cg.mb.recover_timeout(rc);
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
