// data_weights.hip -- DataWeights (data_weights.hpp: the legal states and what each buffer holds in them) and the C
// entry points of the robust data term (no reference counterpart).  The only code that moves the
// data-weight buffers.
#include <cmath>
#include <utility>

#include "solver_passes.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

// Weights or the loss changed whether the problem is robust(): the tile plan has another form then (ztile_plan)
static void replan_if(srmap_problem* p, bool was_robust) {
  if (p->dw.robust() != was_robust) model_replan(p);
}

// *dst (allocated if it is not) <- the source, on src.st: waited for from the host, enqueued from the device
static int write_factor(srmap_problem* p, DevBuf* dst, const WeightSource& src) {
  const size_t n = p->lr_count();
  if (int rc = ensure(p, dst, n * p->elem())) return rc;
  if (src.host) return convert_upload(p, src.host, dst->as(), n, src.st);
  SRMAP_HIP(p->ctx, hipMemcpyAsync(dst->as(), src.dev, n * p->elem(), hipMemcpyDeviceToDevice, src.st));
  return SRMAP_OK;
}

// allocate eff (all ones) if there is none
int DataWeights::ensure_ones(srmap_problem* p, hipStream_t st) {
  if (eff_) return SRMAP_OK;
  const size_t n = p->lr_count();
  SRMAP_HIP(p->ctx, eff_.alloc(n * p->elem()));
  dispatch_dtype(p->dtype, [&](auto t) { launch_fill(eff_.as<decltype(t)>(), decltype(t)(1), n, st); });
  SRMAP_HIP(p->ctx, hipGetLastError());
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

// eff <- prior .* user (ones where the caller gave none) on st, waited for: a problem with a prior only
int DataWeights::rebuild(srmap_problem* p, hipStream_t st) {
  const int rc = dispatch_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    return launch_weight_product<T>(p, prior_.as<const T>(), user_.as<const T>(), eff_.as<T>(), p->lr_count(), st);
  });
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

int DataWeights::set_user(srmap_problem* p, const WeightSource& src) {
  const hipStream_t st = src.st;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  const bool was = robust();
  DevBuf* dst = prior_ ? &user_ : &eff_;  // beside a prior the caller's weights go to the second buffer
  if (src.none()) {
    if (*dst) { SRMAP_HIP(p->ctx, hipStreamSynchronize(st)); dst->reset(); }
  } else {
    rc = write_factor(p, dst, src);
  }
  if (prior_) return rc ? rc : rebuild(p, st);
  // no weights: the unweighted kernels again -- except under a Huber loss, which keeps (and owns) the buffer
  if (src.none() && loss_ == SRMAP_DATA_LOSS_HUBER) rc = ensure_ones(p, st);
  if (src.dev && rc == SRMAP_OK) SRMAP_HIP(p->ctx, hipStreamSynchronize(st));  // complete on return, as srmap_set_observations_device
  replan_if(p, was);
  return rc;
}

int DataWeights::set_prior(srmap_problem* p, const WeightSource& src) {
  const hipStream_t st = src.st;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  const bool was = robust();
  if (src.none()) {
    if (!prior_) return SRMAP_OK;
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    prior_.reset();
    eff_ = std::move(user_);  // the product is freed; the caller's weights as given, or none: the unweighted kernels again
    if (loss_ == SRMAP_DATA_LOSS_HUBER) rc = ensure_ones(p, st);
    replan_if(p, was);
    return rc;
  }
  if (!prior_) {  // the first prior: the weights in force become the caller's factor, eff the product's buffer
    const size_t bytes = p->lr_count() * p->elem();
    DevBuf m, product;
    if (m.alloc(bytes) != hipSuccess || product.alloc(bytes) != hipSuccess)
      return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (data prior: 2 x %zu bytes)", bytes);
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
    prior_ = std::move(m);
    user_ = std::move(eff_);  // possibly none (ones)
    eff_ = std::move(product);
  }
  rc = write_factor(p, &prior_, src);
  if (rc) return rc;
  rc = rebuild(p, st);  // complete on return
  replan_if(p, was);
  return rc;
}

int DataWeights::set_loss(srmap_problem* p, int loss, double huber_delta) {
  const bool was = robust();
  loss_ = loss;
  delta_ = loss == SRMAP_DATA_LOSS_HUBER ? huber_delta : 0.0;
  int rc = SRMAP_OK;
  if (loss == SRMAP_DATA_LOSS_HUBER) {
    rc = state_begin_write(p, p->ctx->stream);
    if (rc == SRMAP_OK) rc = ensure_ones(p, p->ctx->stream);
  }
  replan_if(p, was);
  return rc;
}

int DataWeights::reset(srmap_problem* p, int c0, int C, hipStream_t st) {
  const Geometry& g = p->geo;
  if (C <= 0) { c0 = 0; C = g.C; }
  if (!eff_) return set_error(p->ctx, SRMAP_EINVAL, "internal: a Huber loss without its weight buffer");
  const size_t nl = (size_t)g.w * g.h, run = (size_t)C * nl, e = p->elem();
  for (int k = 0; k < g.K; ++k) {  // [K][C][h][w]: one run per frame
    const size_t off = ((size_t)k * g.C + c0) * nl;
    if (prior_)
      SRMAP_HIP(p->ctx, hipMemcpyAsync(eff_.as<char>() + off * e, prior_.as<const char>() + off * e, run * e, hipMemcpyDeviceToDevice, st));
    else
      dispatch_dtype(p->dtype, [&](auto t) { launch_fill(eff_.as<decltype(t)>() + off, decltype(t)(1), run, st); });
  }
  return SRMAP_OK;
}

int DataWeights::huber_step(srmap_problem* p, int c0, int C, const void* x, hipStream_t st) {
  if (loss_ != SRMAP_DATA_LOSS_HUBER)
    return set_error(p->ctx, SRMAP_EINVAL, "the data weights are re-derived for a Huber loss only (srmap_problem_set_data_loss)");
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  rc = ensure_ones(p, st);
  if (rc) return rc;
  Geometry geo = p->geo;
  if (C > 0) geo.C = C; else c0 = 0;
  rc = ensure_eval_partials(p);
  if (rc) return rc;
  rc = dispatch_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    // d_resid: [K][geo.C][h][w], unweighted
    if (int r = launch_forward_residual<T>(p, geo, c0, (const T*)x, p->d_partials.as<double>(), st)) return r;
    const size_t nl = (size_t)geo.w * geo.h;
    return launch_huber_weights<T>(p, p->d_resid.as<const T>(), eff_.as<T>() + (size_t)c0 * nl, (size_t)geo.K, (size_t)geo.C * nl,
                                   (size_t)geo.C * nl, (size_t)p->geo.C * nl, delta_, st,
                                   prior_ ? prior_.as<const T>() + (size_t)c0 * nl : nullptr);
  });
  if (rc) return rc;
  return state_end_write(p, st);  // asynchronous: evaluations on other streams wait for this event
}

}  // namespace srmap

extern "C" {

static int finite_and_not_negative(srmap_problem* p, const double* v, const char* fmt) {
  if (v)
    for (size_t i = 0, n = p->lr_count(); i < n; ++i)
      if (!(v[i] >= 0.0) || !std::isfinite(v[i])) return set_error(p->ctx, SRMAP_EINVAL, fmt, i, v[i]);
  return SRMAP_OK;
}

int srmap_set_data_weights(srmap_problem* p, const double* w_host) {
  if (!p) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (int rc = finite_and_not_negative(p, w_host, "data weight %zu is %g: weights must be finite and >= 0")) return rc;
  return p->dw.set_user(p, {w_host, nullptr, p->ctx->stream});
}

int srmap_set_data_weights_device(srmap_problem* p, const void* w_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  if (!w_dev) return srmap_set_data_weights(p, nullptr);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return p->dw.set_user(p, {nullptr, w_dev, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream});
}

int srmap_set_data_prior(srmap_problem* p, const double* m_host) {
  if (!p) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (int rc = finite_and_not_negative(p, m_host, "data prior %zu is %g: the prior must be finite and >= 0")) return rc;
  return p->dw.set_prior(p, {m_host, nullptr, p->ctx->stream});
}

int srmap_set_data_prior_device(srmap_problem* p, const void* m_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  if (!m_dev) return srmap_set_data_prior(p, nullptr);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return p->dw.set_prior(p, {nullptr, m_dev, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream});
}

// a factor for the caller: ones where there is none
static int download_or_ones(srmap_problem* p, const void* dev, double* host) {
  const size_t n = p->lr_count();
  if (dev) return convert_download(p, dev, host, n, p->ctx->stream);
  for (size_t i = 0; i < n; ++i) host[i] = 1.0;
  return SRMAP_OK;
}

int srmap_get_data_prior(srmap_problem* p, double* m_host, int* is_set) {
  if (!p) return SRMAP_EINVAL;
  const void* m = p->dw.prior<void>();
  if (is_set) *is_set = m ? 1 : 0;
  if (!m_host) return SRMAP_OK;
  if (m) SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return download_or_ones(p, m, m_host);
}

int srmap_get_data_weights(srmap_problem* p, double* w_host) {
  if (!p || !w_host) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const void* w = p->dw.effective<void>();
  // the weights may have been written asynchronously on another stream (srmap_update_data_weights_device)
  if (w && p->state_stream && p->state_stream != p->ctx->stream) SRMAP_HIP(p->ctx, hipStreamSynchronize(p->state_stream));
  return download_or_ones(p, w, w_host);
}

int srmap_problem_set_data_loss(srmap_problem* p, int loss, double huber_delta) {
  if (!p) return SRMAP_EINVAL;
  if (loss != SRMAP_DATA_LOSS_L2 && loss != SRMAP_DATA_LOSS_HUBER)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown data loss %d", loss);
  if (loss == SRMAP_DATA_LOSS_HUBER && !(huber_delta > 0.0 && std::isfinite(huber_delta)))
    return set_error(p->ctx, SRMAP_EINVAL, "huber_delta must be finite and > 0 (got %g)", huber_delta);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return p->dw.set_loss(p, loss, huber_delta);
}

int srmap_update_data_weights_device(srmap_problem* p, const void* x_dev, void* hip_stream) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return p->dw.huber_step(p, 0, 0, x_dev, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

}  // extern "C"
