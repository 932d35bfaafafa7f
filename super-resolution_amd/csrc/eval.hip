// eval.hip -- the dispatch of one cost+gradient evaluation onto the HIP kernels (the sequence of a direct evaluation and
// that of a tile evaluation), the stream ordering of the device state an evaluation reads (observations, weights), and
// the entry points that run kernels on host buffers.  No CPU compute path exists here: every numeric entry point launches
// gfx950 kernels or fails.
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "srmap_internal.hpp"
#include "ztile_plan.hpp"

using namespace srmap;

namespace srmap {

static size_t partials_needed(const srmap_problem* p) {
  const Geometry& g = p->geo;
  const size_t fwd = (size_t)((g.w * g.h + 255) / 256) * g.C * g.K;
  const size_t reg_blocks = std::max((size_t)((g.W * g.H + 255) / 256), (size_t)((g.W + 63) / 64) * ((g.H + 3) / 4));
  const size_t reg = reg_blocks * g.C * kMaxRegularizers;
  const size_t n = fwd + reg + ztile_est_partials(p->zplan.get(), g.w, g.H, g.C) + 16;
  return n + (size_t)reduce_scratch_slots(n) + 16;  // + the second-stage scratch of launch_reduce_partials
}

int ensure_eval_partials(srmap_problem* p) {
  const size_t n = 2 * partials_needed(p);  // second half: partials of g.d (EvalReq::dvec; gd_partials)
  if (p->partials_cap >= n) return SRMAP_OK;
  p->partials_cap = 0;
  SRMAP_HIP(p->ctx, p->d_partials.alloc(n * sizeof(double)));
  p->partials_cap = n;
  return SRMAP_OK;
}

// The regularisers through the direct kernels, accumulating into g (nullptr: cost only -- the gradient kernel still
// produces the lambda*w*r^2 partials), every active one but `skip` (the one fused into the tiles; -1: none).  Their cost
// partials go behind the *nparts that are already at `partials`, and *nparts counts them in.
template <typename T>
static int launch_regs_direct(srmap_problem* p, const Geometry& geo, int c0, int skip, const T* x, T* g, double* partials,
                              int* nparts, hipStream_t st) {
  const size_t N = (size_t)geo.W * geo.H;
  for (int r = 0; r < p->nreg; ++r) {
    const RegSpec& rs = p->reg[r];
    if (r == skip || rs.lambda <= 0.0) continue;  // objective_irls_regularization_term.cpp:16-18
    const bool onfly = rs.kind != SRMAP_REG_BTV;  // TV kinds: values recomputed in the gradient kernel
    if (!onfly) {
      if (int rc = ensure(p, &p->d_regvals, p->hr_count() * sizeof(T))) return rc;
      if (int rc = launch_reg_values<T>(p, geo, rs, x, p->d_regvals.as<T>(), st)) return rc;
    }
    int nb = 0;
    const T* wts = rs.weights ? rs.weights.as<const T>() + (size_t)c0 * N : nullptr;
    if (int rc = launch_reg_gradient_direct<T>(p, geo, rs, x, wts, rs.lambda, onfly ? nullptr : p->d_regvals.as<const T>(), g,
                                               true, partials + *nparts, &nb, st))
      return rc;
    *nparts += nb;
  }
  return SRMAP_OK;
}

// d_resid <- A_k x - y_k (dw: .* the data weights) of the channel view, with the data-cost partials, by the forward kernel
// the problem's evaluations use: the forward tile kernel where the plan has one, else the direct kernel
template <typename T>
static int forward_residuals(srmap_problem* p, const ZPlan* z, const Geometry& geo, int obs_c0, const T* x, double* partials,
                             int* nfwd, hipStream_t st, const SpFold& fold, const T* dw) {
  if (int rc = ensure(p, &p->d_resid, p->lr_count() * sizeof(T))) return rc;
  if (z != nullptr && z->subpix && z->spf.ok)
    return launch_forward_sp<T>(p, geo, z->spf, x, p->d_obs.as<const T>(), p->geo.C, obs_c0, p->d_resid.as<T>(), partials, nfwd, st, fold, dw);
  return launch_forward_direct<T>(p, geo, x, p->d_obs.as<const T>(), p->geo.C, obs_c0, p->d_resid.as<T>(), 0, geo.K, partials, nfwd, st, dw);
}
template <typename T>
int launch_forward_residual(srmap_problem* p, const Geometry& geo, int obs_c0, const T* x, double* partials, hipStream_t st) {
  int nfwd = 0;
  return forward_residuals<T>(p, ztile_active(p), geo, obs_c0, x, partials, &nfwd, st, SpFold(), nullptr);
}
template int launch_forward_residual<float>(srmap_problem*, const Geometry&, int, const float*, double*, hipStream_t);
template int launch_forward_residual<double>(srmap_problem*, const Geometry&, int, const double*, double*, hipStream_t);

// The sequence of an evaluation on the tile path: (sub-pixel plans: forward kernel, ring pass,) tile launch, the remaining
// regularisers, finish.  *nblocks: the partials left at `partials` for the caller's reduction; 0: the cost is in d_cost
template <typename T>
static int eval_ztile(srmap_problem* p, const ZPlan& z, const EvalReq& req, EvalOut* out, const Geometry& geo, int obs_c0,
                      unsigned terms, const T* x, T* g, double* partials, int* nblocks, hipStream_t st) {
  const bool want_reg = (terms & SRMAP_TERM_REG) != 0;
  // the regulariser fused into the tiles takes part when the evaluation asks for the regularisers
  const int regk = want_reg ? z.regk : 0, regr = want_reg ? z.regr : 0;
  const T* wts = regk && p->reg[z.reg_index].weights ? p->reg[z.reg_index].weights.as<const T>() + (size_t)obs_c0 * geo.W * geo.H : nullptr;
  const unsigned zterms = (terms & SRMAP_TERM_DATA) | (regk ? SRMAP_TERM_REG : 0u);
  int rc = SRMAP_OK, nb = 0;
  // g.d with the gradient (solver line search): only when this launch produces the WHOLE gradient and the single
  // finish launch reduces it -- no further regulariser kernels, few enough partials
  const bool more_regs = want_reg && ztile_more_regs(p, z);
  const size_t est_parts = ztile_est_partials(&z, geo.w, geo.H, geo.C);
  const bool sp_data = z.subpix && (terms & SRMAP_TERM_DATA);
  const bool with_d = req.dvec != nullptr && g != nullptr && ztile_gd_instance_ok(p, z, geo.w, geo.H, geo.C, terms);
  int nfwd = 0;
  // the exact ring pass AHEAD of the tile kernel (k_gather_ring into the plan's buffer; the edge tiles add the values as
  // they store g, so g.d and the cost finish inside the tile launch) wherever the ring kernel applies; else behind it,
  // adding to g (then no g.d from the launch: ztile_gd_instance_ok).  Ring blocks at the front of the tile launch's own
  // grid (one launch less) were built and measured: every ring workgroup holds a tile slot (73 KB of LDS) for its 6 - 9 us of
  // latency, 450 of the 512 slots of the first generation -- 82.9 us against 82.5 us, and slower inside a solve.
  const bool ring_ahead = sp_data && g != nullptr && z.d_ringbuf;
  if (sp_data) {
    // sub-pixel shifts: exact residuals (and the data cost) from the direct forward kernel, then the tile kernel
    // gathers them with the 4-tap tables; the pixels within Dr of the edge are evaluated exactly by the ring pass
    if (req.fold.xk != nullptr && !(with_d && z.spf.ok && z.spf.can_fold))
      return set_error(p->ctx, SRMAP_EINVAL, "internal: a folded trial point needs the forward tile kernel and the g.d instance (ztile_can_fold)");
    // data weights: the WEIGHTED forward instances leave w .* r for the gathers
    rc = forward_residuals<T>(p, &z, geo, obs_c0, x, partials, &nfwd, st, req.fold, p->dw.effective<T>());
    if (rc) return rc;
    partials += nfwd;
    if (ring_ahead) {
      rc = launch_gather_direct<T>(p, geo, p->d_resid.as<const T>(), g, 0, geo.K, 2.0 * geo.s * geo.s, true, st, z.Dr, z.d_ringbuf.as<T>());
      if (rc) return rc;
    }
  }
  if (req.fold.xk != nullptr && !(with_d && req.overlap.fn == nullptr))
    return set_error(p->ctx, SRMAP_EINVAL, "internal: a folded trial point needs the tile kernel's g.d instance (ztile_can_fold)");
  const T* dv = with_d ? (const T*)req.dvec : nullptr;
  double* pgd = with_d ? gd_partials(p) : nullptr;
  // tiles: the cost reduction inside the kernel (no finish launch) when no in-image pixel of the border frame needs a
  // correction, no further regulariser kernel follows and the granules suffice
  // Sub-pixel plan: the forward kernel's data-cost partials (plain doubles, complete before the tile kernel starts) are
  // added by the same in-kernel finish; the ring pass touches g only.
  MFin mfin;
  mfin.on = !more_regs && req.overlap.fn == nullptr && z.d_mpart && est_parts <= z.mpart_cap &&
            (z.n_ring == 0 || (z.ring.rg[0] == 0 && z.ring.rg[1] == 0)) && (size_t)nfwd <= kMaxFusedPartials;
  mfin.publish = mfin.on && with_d && req.pub.out != nullptr;
  mfin.xpart = (mfin.on && sp_data) ? partials - nfwd : nullptr;
  mfin.n_xpart = (mfin.on && sp_data) ? nfwd : 0;
  rc = launch_ztiles<T>(p, req, geo, obs_c0, zterms, regk, regr, x, g, wts, z, partials, &nb, st, dv, pgd, mfin, ring_ahead);
  if (rc) return rc;
  if (sp_data) {
    partials -= nfwd;
    nb += nfwd;
    if (g != nullptr && !ring_ahead) {
      rc = launch_gather_direct<T>(p, geo, p->d_resid.as<const T>(), g, 0, geo.K, 2.0 * geo.s * geo.s, true, st, z.Dr);
      if (rc) return rc;
    }
  }
  int total = nb;
  // remaining regularisers (3-D TV, a second regulariser, BTV range > 3): direct kernels, accumulating into g
  if (want_reg) {
    rc = launch_regs_direct<T>(p, geo, obs_c0, z.reg_index, x, g, partials, &total, st);
    if (rc) return rc;
  }
  const bool corr_on = (terms & SRMAP_TERM_DATA) && z.n_ring > 0 && g != nullptr;
  if (!mfin.on && (size_t)total > kMaxFusedPartials) {
    // many partials (multi-channel problems): corrections here, two-stage reduction by the caller.  The launch reduces
    // nothing: the zero it stores goes to the g.d slot, which this evaluation leaves invalid (gd_valid stays false)
    *nblocks = total;
    return corr_on ? launch_zfinish<T>(p, z, geo, g, partials, 0, p->d_cost.as<double>() + kCostGd, nullptr, nullptr, nullptr, 0.0, st) : SRMAP_OK;
  }
  // the cost (and with_d: g.d in d_cost[kCostGd], published when asked) is reduced by the last workgroup of the tile
  // kernel, or by the finish launch: border corrections of g + the fixed-order cost reduction, one launch
  if (!mfin.on) {
    rc = launch_zfinish<T>(p, z, geo, corr_on ? g : (T*)nullptr, partials, total, p->d_cost.as<double>(), pgd,
                           with_d ? req.pub.out : (double*)nullptr, req.pub.tag_slot, req.pub.tag, st);
    if (rc) return rc;
  }
  out->gd_valid = with_d;
  out->published = with_d && req.pub.out != nullptr;
  *nblocks = 0;  // total already in d_cost[kCostValue]
  return SRMAP_OK;
}

// One ObjectiveFunction::ComputeAllTerms on device buffers.
template <typename T>
static int eval_typed(srmap_problem* p, EvalReq req, EvalOut* out, unsigned terms, const T* x, T* g, hipStream_t st) {
  Geometry geo = p->geo;
  const int c0 = req.view.C > 0 ? req.view.c0 : 0;
  if (req.view.C > 0) geo.C = req.view.C;
  geo.zlo = (req.view.coupled && c0 > 0) ? 1 : 0;
  geo.zhi = (req.view.coupled && c0 + geo.C < p->geo.C) ? 1 : 0;
  geo.rr0 = std::min(req.rr0, geo.H);
  geo.rr1 = std::min(req.rr1, geo.H);
  const size_t N = (size_t)geo.W * geo.H;
  int rc = ensure_eval_partials(p);
  if (rc) return rc;
  if ((terms & SRMAP_TERM_DATA) && !p->have_obs)
    return set_error(p->ctx, SRMAP_EINVAL, "data term requested but no observations set");
  const ZPlan* ztile = ztile_active(p);
  if (req.overlap.fn != nullptr && !(ztile && ztile_overlaps_halo(p))) {
    // row shard on a path that cannot run under the halo exchange: exchange first
    rc = req.overlap.fn(req.overlap.arg);
    if (rc) return rc;
    SRMAP_HIP(p->ctx, hipStreamWaitEvent(st, req.overlap.event, 0));
    req.overlap.fn = nullptr;
  }
  if (p->impl == SRMAP_IMPL_TILED && !ztile) {
    if (p->motion.kind() == kMotionLattice) return p->motion.refuse(p->ctx, SRMAP_EUNSUPPORTED, "tiled kernels do not cover %s (%s)");
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "tiled kernels do not cover this geometry");
  }
  int nparts = 0;
  if (ztile) {
    rc = eval_ztile<T>(p, *ztile, req, out, geo, c0, terms, x, g, p->d_partials.as<double>(), &nparts, st);
    if (rc) return rc;
  } else {
    if (terms & SRMAP_TERM_DATA) {
      rc = forward_residuals<T>(p, nullptr, geo, c0, x, p->d_partials.as<double>(), &nparts, st, SpFold(), p->dw.effective<T>());
      if (rc) return rc;
      if (g) {
        rc = launch_gather_direct<T>(p, geo, p->d_resid.as<const T>(), g, 0, geo.K,
                                     2.0 * geo.s * geo.s, false, st, 0, nullptr, c0);
        if (rc) return rc;
      }
    } else if (g) {
      SRMAP_HIP(p->ctx, hipMemsetAsync(g, 0, N * geo.C * sizeof(T), st));
    }
    if (terms & SRMAP_TERM_REG) {
      rc = launch_regs_direct<T>(p, geo, c0, -1, x, g, p->d_partials.as<double>(), &nparts, st);
      if (rc) return rc;
    }
  }
  if (ztile && nparts == 0) return SRMAP_OK;  // reduced inside the last kernel of the evaluation
  return launch_reduce_partials(p, p->d_partials.as<double>(), nparts, p->d_cost.as<double>(), st);
}

// ---- stream ordering of the problem's device state (include/srmap.h, "Streams"; srmap_internal.hpp) ----
int state_begin_write(srmap_problem* p, hipStream_t st) {
  if (p->use_stream && p->use_stream != st) SRMAP_HIP(p->ctx, hipStreamSynchronize(p->use_stream));
  return SRMAP_OK;
}
int state_end_write(srmap_problem* p, hipStream_t st) {
  if (!p->state_ev) SRMAP_HIP(p->ctx, hipEventCreateWithFlags(&p->state_ev, hipEventDisableTiming));
  SRMAP_HIP(p->ctx, hipEventRecord(p->state_ev, st));
  p->state_stream = st;
  p->state_seen = nullptr;
  return SRMAP_OK;
}
// an evaluation on st: ordered after the last asynchronous state write (nothing to do on the same stream)
static inline int state_read(srmap_problem* p, hipStream_t st) {
  if (p->state_stream && p->state_stream != st && p->state_seen != st) {
    SRMAP_HIP(p->ctx, hipStreamWaitEvent(st, p->state_ev, 0));
    p->state_seen = st;
  }
  p->use_stream = st;
  return SRMAP_OK;
}

int problem_state_read(srmap_problem* p, hipStream_t st) { return state_read(p, st); }

int eval_dispatch(srmap_problem* p, const EvalReq& req, EvalOut* out, unsigned terms, const void* x, void* g,
                  hipStream_t st) {
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (int rc = state_read(p, st)) return rc;
  return dispatch_dtype(p->dtype, [&](auto t) { return eval_typed<decltype(t)>(p, req, out, terms, (const decltype(t)*)x, (decltype(t)*)g, st); });
}

int recover_reduction_timeout(srmap_problem* p, double* host_word) {
  // a late workgroup may still publish into the granules: re-initialise them only behind everything in flight
  SRMAP_HIP(p->ctx, hipDeviceSynchronize());
  ztile_rearm(p);
  if (p->d_cost.as<double>()) SRMAP_HIP(p->ctx, hipMemset(p->d_cost.as<double>() + kCostTimeout, 0, sizeof(double)));
  if (host_word) *host_word = 0.0;
  return SRMAP_OK;
}

// One staging buffer of the problem and the caller's array of n doubles that goes into it or comes out of it.
struct HostBuf { DevBuf* dev; const double* in; double* out; size_t n; };
// The frame the four operators share: the buffers allocated on first use (HR-sized), the inputs up, launch(T()), the
// outputs back; all on the context's stream
template <typename F>
static int host_operator(srmap_problem* p, std::initializer_list<HostBuf> bufs, F&& launch) {
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  for (const HostBuf& b : bufs)
    if (int rc = ensure(p, b.dev, p->hr_count() * p->elem())) return rc;
  for (const HostBuf& b : bufs)
    if (b.in)
      if (int rc = convert_upload(p, b.in, b.dev->as(), b.n, st)) return rc;
  if (int rc = dispatch_dtype(p->dtype, launch)) return rc;
  for (const HostBuf& b : bufs)
    if (b.out)
      if (int rc = convert_download(p, b.dev->as(), b.out, b.n, st)) return rc;
  return SRMAP_OK;
}

}  // namespace srmap

extern "C" {

static int need_solver_geometry(srmap_problem* p) {
  if (!p->maps_regular)
    return set_error(p->ctx, SRMAP_EINVAL,
                     "HR size %dx%d is not LR size * scale (%d); MapSolver requires it (map_solver.cpp:72-76)",
                     p->geo.W, p->geo.H, p->geo.s);
  return SRMAP_OK;
}

// the frames from host doubles or from a device array of the dtype (one of the two), complete on return: the source may
// be reused, any stream may evaluate
static int set_observations(srmap_problem* p, const double* lr_host, const void* lr_dev, hipStream_t st) {
  int rc = need_solver_geometry(p);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  rc = state_begin_write(p, st);
  if (rc) return rc;
  DevBuf* raw = p->photometric ? &p->d_obs_raw : &p->d_obs;  // photometric parameters persist: the new frames are normalised
  rc = ensure(p, raw, p->lr_count() * p->elem());
  if (rc) return rc;
  if (lr_host) rc = convert_upload(p, lr_host, raw->as(), p->lr_count(), st);  // waits for st itself
  else SRMAP_HIP(p->ctx, hipMemcpyAsync(raw->as(), lr_dev, p->lr_count() * p->elem(), hipMemcpyDeviceToDevice, st));
  if (rc == SRMAP_OK && p->photometric) rc = photometric_normalise(p, st);
  if (rc) return rc;
  if (lr_dev || p->photometric) SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  p->have_obs = true;
  return SRMAP_OK;
}

int srmap_set_observations(srmap_problem* p, const double* lr_host) {
  if (!p || !lr_host) return SRMAP_EINVAL;
  return set_observations(p, lr_host, nullptr, p->ctx->stream);
}

int srmap_set_observations_device(srmap_problem* p, const void* lr_dev, void* hip_stream) {
  if (!p || !lr_dev) return SRMAP_EINVAL;
  return set_observations(p, nullptr, lr_dev, stream_of(p->ctx, hip_stream));
}

int srmap_set_irls_weights(srmap_problem* p, int reg, const double* w_host) {
  if (!p || reg < 0 || reg >= p->nreg) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  RegSpec& rs = p->reg[reg];
  int rc = state_begin_write(p, p->ctx->stream);
  if (rc) return rc;
  if (!w_host) {
    rs.weights.reset();
    return SRMAP_OK;
  }
  rc = ensure(p, &rs.weights, p->hr_count() * p->elem());
  if (rc) return rc;
  return convert_upload(p, w_host, rs.weights.as(), p->hr_count(), p->ctx->stream);
}

int srmap_update_irls_weights_device(srmap_problem* p, int reg, const void* x_dev, void* hip_stream) {
  if (!p || reg < 0 || reg >= p->nreg || !x_dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  RegSpec& rs = p->reg[reg];
  hipStream_t st = stream_of(p->ctx, hip_stream);
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  rc = ensure(p, &rs.weights, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = dispatch_dtype(p->dtype, [&](auto t) { return launch_reg_weights<decltype(t)>(p, p->geo, rs, (const decltype(t)*)x_dev, rs.weights.as<decltype(t)>(), st); });
  if (rc) return rc;
  return state_end_write(p, st);  // asynchronous: evaluations on other streams wait for this event
}

// ---- operators on host buffers ----
int srmap_apply(srmap_problem* p, int frame, const double* hr, double* lr) {
  if (!p || !hr || !lr) return SRMAP_EINVAL;
  if (frame < 0 || frame >= p->geo.K) return set_error(p->ctx, SRMAP_EINVAL, "frame index %d out of range", frame);  // motion_shift.cpp:48-50
  const Geometry& g = p->geo;
  return host_operator(p, {{&p->d_x, hr, nullptr, p->hr_count()}, {&p->d_tmp, nullptr, lr, (size_t)g.C * g.w * g.h}}, [&](auto t) {
    using T = decltype(t);
    return launch_forward_direct<T>(p, g, p->d_x.as<const T>(), nullptr, g.C, 0, p->d_tmp.as<T>(), frame, 1, nullptr, nullptr, p->ctx->stream);
  });
}

int srmap_apply_transpose(srmap_problem* p, int frame, const double* lr, double* hr) {
  if (!p || !lr || !hr) return SRMAP_EINVAL;
  if (frame < 0 || frame >= p->geo.K) return set_error(p->ctx, SRMAP_EINVAL, "frame index %d out of range", frame);
  const Geometry& g = p->geo;
  if (g.W != g.w * g.s || g.H != g.h * g.s) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "transpose needs HR size == LR size * scale");
  return host_operator(p, {{&p->d_g, nullptr, hr, p->hr_count()}, {&p->d_tmp, lr, nullptr, (size_t)g.C * g.w * g.h}}, [&](auto t) {
    using T = decltype(t);
    return launch_gather_direct<T>(p, g, p->d_tmp.as<const T>(), p->d_g.as<T>(), frame, 1, 1.0, false, p->ctx->stream);
  });
}

int srmap_reg_values(srmap_problem* p, int reg, const double* x, double* values) {
  if (!p || !x || !values || reg < 0 || reg >= p->nreg) return SRMAP_EINVAL;
  const size_t n = p->hr_count();
  return host_operator(p, {{&p->d_x, x, nullptr, n}, {&p->d_regvals, nullptr, values, n}}, [&](auto t) {
    using T = decltype(t);
    return launch_reg_values<T>(p, p->geo, p->reg[reg], p->d_x.as<const T>(), p->d_regvals.as<T>(), p->ctx->stream);
  });
}

int srmap_reg_values_and_gradient(srmap_problem* p, int reg, const double* x, const double* gc,
                                  double* values, double* gradient) {
  if (!p || !x || !gc || !values || !gradient || reg < 0 || reg >= p->nreg) return SRMAP_EINVAL;
  const size_t n = p->hr_count();
  const RegSpec& rs = p->reg[reg];
  return host_operator(p, {{&p->d_x, x, nullptr, n}, {&p->d_regvals, nullptr, values, n}, {&p->d_tmp, gc, nullptr, n}, {&p->d_g, nullptr, gradient, n}}, [&](auto t) {
    using T = decltype(t);
    hipStream_t st = p->ctx->stream;
    if (int r = launch_reg_values<T>(p, p->geo, rs, p->d_x.as<const T>(), p->d_regvals.as<T>(), st)) return r;
    return launch_reg_gradient_direct<T>(p, p->geo, rs, p->d_x.as<const T>(), p->d_tmp.as<const T>(), 1.0,
                                         p->d_regvals.as<const T>(), p->d_g.as<T>(), false, nullptr, nullptr, st);
  });
}

// ---- objective ----
int srmap_eval_device(srmap_problem* p, unsigned terms, const void* x_dev, void* g_dev, double* cost,
                      void* hip_stream) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  hipStream_t st = stream_of(p->ctx, hip_stream);
  EvalOut out;
  int rc = eval_dispatch(p, EvalReq(), &out, terms, x_dev, g_dev, st);
  if (rc) return rc;
  if (cost) {
    SRMAP_HIP(p->ctx, hipMemcpyAsync(cost, p->d_cost.as<double>(), sizeof(double), hipMemcpyDeviceToHost, st));
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    if (*cost != *cost) {  // NaN: the input's, or the in-kernel reduction gave up waiting for a workgroup (sticky word)
      double flag = 0.0;
      SRMAP_HIP(p->ctx, hipMemcpy(&flag, p->d_cost.as<double>() + kCostTimeout, sizeof(double), hipMemcpyDeviceToHost));
      if (flag != 0.0) {  // re-arm and report: the evaluation's gradient is not trustworthy
        rc = recover_reduction_timeout(p, nullptr);
        if (rc) return rc;
        return set_error(p->ctx, SRMAP_EHIP, "in-kernel cost reduction timed out waiting for a workgroup (device fault or a wedged queue)");
      }
    }
  }
  return SRMAP_OK;
}

int srmap_last_cost(srmap_problem* p, double* cost) {
  if (!p || !cost) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  SRMAP_HIP(p->ctx, hipDeviceSynchronize());
  SRMAP_HIP(p->ctx, hipMemcpy(cost, p->d_cost.as<double>(), sizeof(double), hipMemcpyDeviceToHost));
  return SRMAP_OK;
}

int srmap_eval(srmap_problem* p, unsigned terms, const double* x, double* cost, double* grad) {
  if (!p || !x) return SRMAP_EINVAL;  // CHECK_NOTNULL(estimated_image_data)
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const size_t n = p->hr_count();
  int rc = ensure(p, &p->d_x, n * p->elem()); if (rc) return rc;
  if (grad) { rc = ensure(p, &p->d_g, n * p->elem()); if (rc) return rc; }
  rc = convert_upload(p, x, p->d_x.as(), n, st); if (rc) return rc;
  double c = 0;
  rc = srmap_eval_device(p, terms, p->d_x.as(), grad ? p->d_g.as() : nullptr, &c, st); if (rc) return rc;
  if (cost) *cost = c;
  if (grad) return convert_download(p, p->d_g.as(), grad, n, st);
  return SRMAP_OK;
}

}  // extern "C"
