// eval.hip -- the dispatch of one cost+gradient evaluation onto the HIP kernels, the stream ordering of the device state
// an evaluation reads (observations, weights), and the entry points that run kernels on host buffers.  No CPU compute
// path exists here: every numeric entry point launches gfx950 kernels or fails.
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

static int ensure_partials(srmap_problem* p, size_t n) {
  n *= 2;  // second half: partials of g.d (EvalReq::dvec)
  if (p->partials_cap >= n) return SRMAP_OK;
  p->partials_cap = 0;
  SRMAP_HIP(p->ctx, p->d_partials.alloc(n * sizeof(double)));
  p->partials_cap = n;
  return SRMAP_OK;
}

static size_t partials_needed(const srmap_problem* p) {
  const Geometry& g = p->geo;
  const size_t fwd = (size_t)((g.w * g.h + 255) / 256) * g.C * g.K;
  const size_t reg_blocks = std::max((size_t)((g.W * g.H + 255) / 256), (size_t)((g.W + 63) / 64) * ((g.H + 3) / 4));
  const size_t reg = reg_blocks * g.C * kMaxRegularizers;
  const size_t n = fwd + reg + ztile_partials_needed(p) + 16;
  return n + (size_t)reduce_scratch_slots(n) + 16;  // + the second-stage scratch of launch_reduce_partials
}

int ensure_eval_partials(srmap_problem* p) { return ensure_partials(p, partials_needed(p)); }

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
  const bool ztile = p->impl != SRMAP_IMPL_DIRECT && p->zplan != nullptr;
  if (req.overlap.fn != nullptr && !(ztile && ztile_overlaps_halo(p))) {
    // row shard on a path that cannot run under the halo exchange: exchange first
    rc = req.overlap.fn(req.overlap.arg);
    if (rc) return rc;
    SRMAP_HIP(p->ctx, hipStreamWaitEvent(st, req.overlap.event, 0));
    req.overlap.fn = nullptr;
  }
  if (p->impl == SRMAP_IMPL_TILED && !ztile) {
    if (p->lat_step)
      return set_error(p->ctx, SRMAP_EUNSUPPORTED, "tiled kernels do not cover %s (%s)", field_motion_name(p), field_motion_setter(p));
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "tiled kernels do not cover this geometry");
  }
  int nparts = 0;
  if (ztile) {
    rc = launch_eval_ztile<T>(p, req, out, geo, c0, terms, x, g, p->d_partials.as<double>(), &nparts, st);
    if (rc) return rc;
  } else {
    bool g_written = false;
    if (terms & SRMAP_TERM_DATA) {
      rc = ensure(p, &p->d_resid, p->lr_count() * sizeof(T));
      if (rc) return rc;
      int nb = 0;
      rc = launch_forward_direct<T>(p, geo, x, p->d_obs.as<const T>(), p->geo.C, c0,
                                    p->d_resid.as<T>(), 0, geo.K, p->d_partials.as<double>() + nparts, &nb, st, p->dw.effective<T>());
      if (rc) return rc;
      nparts += nb;
      if (g) {
        rc = launch_gather_direct<T>(p, geo, p->d_resid.as<const T>(), g, 0, geo.K,
                                     2.0 * geo.s * geo.s, false, st, 0, nullptr, c0);
        if (rc) return rc;
        g_written = true;
      }
    }
    if (g && !g_written) SRMAP_HIP(p->ctx, hipMemsetAsync(g, 0, N * geo.C * sizeof(T), st));
    if (terms & SRMAP_TERM_REG) {
      for (int r = 0; r < p->nreg; ++r) {
        const RegSpec& rs = p->reg[r];
        if (rs.lambda <= 0.0) continue;  // objective_irls_regularization_term.cpp:16-18
        // (cost only, g == nullptr: the gradient kernel still produces the lambda*w*r^2 partials)
        const bool onfly = rs.kind != SRMAP_REG_BTV;  // TV kinds: values recomputed in the gradient kernel
        if (!onfly) {
          rc = ensure(p, &p->d_regvals, p->hr_count() * sizeof(T));
          if (rc) return rc;
          rc = launch_reg_values<T>(p, geo, rs, x, p->d_regvals.as<T>(), st);
          if (rc) return rc;
        }
        int nb = 0;
        const T* wts = rs.weights ? rs.weights.as<const T>() + (size_t)c0 * N : nullptr;
        rc = launch_reg_gradient_direct<T>(p, geo, rs, x, wts, rs.lambda,
                                           onfly ? nullptr : p->d_regvals.as<const T>(), g, true,
                                           p->d_partials.as<double>() + nparts, &nb, st);
        if (rc) return rc;
        nparts += nb;
      }
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
  if (p->d_cost.as<double>()) SRMAP_HIP(p->ctx, hipMemset(p->d_cost.as<double>() + 6, 0, sizeof(double)));
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
      SRMAP_HIP(p->ctx, hipMemcpy(&flag, p->d_cost.as<double>() + 6, sizeof(double), hipMemcpyDeviceToHost));
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
