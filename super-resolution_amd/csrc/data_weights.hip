// data_weights.hip -- DataWeights (data_weights.hpp: the legal states and what each buffer holds in them) and the C
// entry points of the robust data term (no reference counterpart).  The only code that moves the
// data-weight buffers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>

#include "solver_passes.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

namespace {  // the kernels of the data weights: only this file launches them

// ---------------------------------------------------------------------------
// Huber IRLS weights of the data term from the UNWEIGHTED residuals: w = 1 where |r| <= delta, delta / |r| elsewhere
// (continuous at |r| = delta), arithmetic in T.  Elementwise and HBM-bound: one read and one write stream.  `rows` runs of
// `rowlen` elements (blockIdx.y = run; a channel view of [K][C][h][w] is K runs, the whole stack one).  VEC: every run
// starts on a 16-byte boundary in both buffers -- 16-byte accesses in a grid-stride loop, the run's last elements one by one.
template <typename T>
__device__ __forceinline__ T huber_weight(T r, T delta) {
  const T a = r < T(0) ? -r : r;
  return a <= delta ? T(1) : delta / a;
}

// PRIOR: a third stream m, indexed like w (the persistent prior of srmap_set_data_prior): w = m .* huber(r), the product
// rounded once in T.  The instance without it reads nothing of m.
// DELTA_DEV: delta_arg is a device double -- the record of the step's residual scale (residual_scale.hip), written earlier
// on the same stream -- rounded to T as the host's (T)delta is; the instances without it take the value itself.
template <typename T, bool VEC, bool PRIOR = false, bool DELTA_DEV = false>
__global__ __launch_bounds__(256) void k_huber_weights(const T* __restrict__ r, T* __restrict__ w, size_t rowlen,
                                                      size_t r_stride, size_t w_stride,
                                                      std::conditional_t<DELTA_DEV, const double*, T> delta_arg,
                                                      const T* __restrict__ m = nullptr) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(16 / sizeof(T))));
  T delta;
  if constexpr (DELTA_DEV) delta = (T)*delta_arg;
  else delta = delta_arg;
  const T* rr = r + (size_t)blockIdx.y * r_stride;
  T* ww = w + (size_t)blockIdx.y * w_stride;
  const T* mm = PRIOR ? m + (size_t)blockIdx.y * w_stride : nullptr;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
  size_t done = 0;
  if (VEC) {
    const size_t nv = rowlen / V;
    for (size_t i = tid; i < nv; i += nth) {
      const VT v = reinterpret_cast<const VT*>(rr)[i];
      VT o;
#pragma unroll
      for (int q = 0; q < V; ++q) o[q] = huber_weight<T>(v[q], delta);
      if constexpr (PRIOR) {
        const VT pv = reinterpret_cast<const VT*>(mm)[i];
#pragma unroll
        for (int q = 0; q < V; ++q) o[q] = pv[q] * o[q];
      }
      reinterpret_cast<VT*>(ww)[i] = o;
    }
    done = nv * V;
  }
  for (size_t i = done + tid; i < rowlen; i += nth) {
    const T hw = huber_weight<T>(rr[i], delta);
    if constexpr (PRIOR) ww[i] = mm[i] * hw;
    else ww[i] = hw;
  }
}

// r: `rows` runs of `rowlen` elements, r_stride apart; w likewise, w_stride apart, starting at w (a channel view of
// [K][C][h][w]).  prior != nullptr (indexed like w): the instance with the prior as a third stream.  delta_dev != nullptr:
// the instances that read delta from there (a device double), `delta` unused
template <typename T>
int launch_huber_weights(srmap_problem* p, const T* r, T* w, size_t rows, size_t rowlen, size_t r_stride, size_t w_stride,
                         double delta, hipStream_t st, const T* prior, const double* delta_dev = nullptr) {
  constexpr size_t V = 16 / sizeof(T);
  if (rows == 0 || rowlen == 0) return SRMAP_OK;
  if (rows > 1 && r_stride == rowlen && w_stride == rowlen) { rowlen *= rows; rows = 1; }  // one contiguous run
  const bool vec = (reinterpret_cast<uintptr_t>(r) % 16 == 0) && (reinterpret_cast<uintptr_t>(w) % 16 == 0) &&
                   (reinterpret_cast<uintptr_t>(prior) % 16 == 0) && (rows == 1 || (r_stride % V == 0 && w_stride % V == 0));
  // grid-stride: enough workgroups to fill the device several times over, no more than the run has 16-byte groups
  const size_t groups = (rowlen + V * 256 - 1) / (V * 256);
  const size_t cap = (size_t)std::max(1, p->ctx->num_cus) * 8;
  dim3 grid((unsigned)std::max<size_t>(1, std::min(groups, (cap + rows - 1) / rows)), (unsigned)rows);
  if (delta_dev) {  // the MAD scale mode: delta is on the device
    if (prior) {
      if (vec) hipLaunchKernelGGL((k_huber_weights<T, true, true, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, delta_dev, prior);
      else hipLaunchKernelGGL((k_huber_weights<T, false, true, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, delta_dev, prior);
    } else if (vec) {
      hipLaunchKernelGGL((k_huber_weights<T, true, false, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, delta_dev, (const T*)nullptr);
    } else {
      hipLaunchKernelGGL((k_huber_weights<T, false, false, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, delta_dev, (const T*)nullptr);
    }
  } else if (prior) {
    if (vec) hipLaunchKernelGGL((k_huber_weights<T, true, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, (T)delta, prior);
    else hipLaunchKernelGGL((k_huber_weights<T, false, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, (T)delta, prior);
  } else if (vec) {
    hipLaunchKernelGGL((k_huber_weights<T, true>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, (T)delta, (const T*)nullptr);
  } else {
    hipLaunchKernelGGL((k_huber_weights<T, false>), grid, dim3(256), 0, st, r, w, rowlen, r_stride, w_stride, (T)delta, (const T*)nullptr);
  }
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// out = a .* b (b == nullptr: out = a), one rounding in T: the effective data weights m .* w of a problem with a prior,
// rebuilt whenever either factor changes.  Elementwise, grid-stride.
template <typename T>
__global__ __launch_bounds__(256) void k_weight_product(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = b ? a[i] * b[i] : a[i];
}

template <typename T>
int launch_weight_product(srmap_problem* p, const T* a, const T* b, T* out, size_t n, hipStream_t st) {
  if (n == 0) return SRMAP_OK;
  const size_t cap = (size_t)std::max(1, p->ctx->num_cus) * 8;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min((n + 255) / 256, cap));
  hipLaunchKernelGGL(k_weight_product<T>, dim3(blocks), dim3(256), 0, st, a, b, out, n);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

}  // namespace

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

// The first prior of a problem: the weights in force become the caller's factor, eff the product's buffer.  Allocates
// prior_ (contents for the caller to write) and the product; a failure leaves the problem as it was
int DataWeights::enter_prior(srmap_problem* p, hipStream_t st) {
  const size_t bytes = p->lr_count() * p->elem();
  DevBuf m, product;
  if (m.alloc(bytes) != hipSuccess || product.alloc(bytes) != hipSuccess)
    return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (data prior: 2 x %zu bytes)", bytes);
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  prior_ = std::move(m);
  user_ = std::move(eff_);  // possibly none (ones)
  eff_ = std::move(product);
  return SRMAP_OK;
}

// Removing the prior: the product is freed; the caller's weights as given, or none: the unweighted kernels again
int DataWeights::leave_prior(srmap_problem* p, hipStream_t st) {
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  prior_.reset();
  eff_ = std::move(user_);
  return loss_ == SRMAP_DATA_LOSS_HUBER ? ensure_ones(p, st) : SRMAP_OK;
}

// prior <- caller's m (ones without one) .* (1 - h) on st: a problem with a hold-out only
int DataWeights::form_held_prior(srmap_problem* p, hipStream_t st) {
  return dispatch_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    return launch_holdout_prior<T>(p, caller_.as<const T>(), prior_.as<T>(), p->lr_count(), hold_.seed, hold_.lo, hold_.threshold, st);
  });
}

int DataWeights::set_holdout(srmap_problem* p, const Holdout& h) {
  const hipStream_t st = p->ctx->stream;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  const bool was = robust();
  if (h.threshold == 0) {  // lift it
    if (!hold_.threshold) return SRMAP_OK;
    holdout_pass_release(p);  // a score is complete on return: nothing of it is in flight
    p->holdout_counts.clear();
    if (caller_) {  // the caller's prior again, as it was given
      SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
      prior_ = std::move(caller_);
      hold_ = Holdout();
      rc = rebuild(p, st);
    } else {
      hold_ = Holdout();
      rc = leave_prior(p, st);
    }
    replan_if(p, was);
    return rc;
  }
  if (!hold_.threshold) {
    if (prior_) {  // the caller's prior moves aside, the product takes its place
      DevBuf product;
      if (product.alloc(p->lr_count() * p->elem()) != hipSuccess)
        return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (hold-out: %zu bytes)", p->lr_count() * p->elem());
      SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
      caller_ = std::move(prior_);
      prior_ = std::move(product);
    } else {
      rc = enter_prior(p, st);
      if (rc) return rc;
    }
  }
  const Holdout before = hold_;
  hold_ = h;
  p->holdout_counts.clear();
  rc = form_held_prior(p, st);
  if (rc == SRMAP_OK) rc = rebuild(p, st);  // complete on return
  if (rc != SRMAP_OK && before.threshold) {  // the factor in force again (a failed launch: best effort, the first error stands)
    hold_ = before;
    if (form_held_prior(p, st) == SRMAP_OK) (void)rebuild(p, st);
  }
  replan_if(p, was);
  return rc;
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
  if (hold_.threshold) {  // beside a hold-out the caller's m is kept apart; what the kernels read is its product with 1 - h
    if (src.none()) {
      if (!caller_) return SRMAP_OK;
      SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
      caller_.reset();
    } else {
      rc = write_factor(p, &caller_, src);
      if (rc) return rc;
    }
    rc = form_held_prior(p, st);
    return rc ? rc : rebuild(p, st);
  }
  if (src.none()) {
    if (!prior_) return SRMAP_OK;
    rc = leave_prior(p, st);
    replan_if(p, was);
    return rc;
  }
  if (!prior_) {
    rc = enter_prior(p, st);
    if (rc) return rc;
  }
  rc = write_factor(p, &prior_, src);
  if (rc) return rc;
  rc = rebuild(p, st);  // complete on return
  replan_if(p, was);
  return rc;
}

int DataWeights::set_loss(srmap_problem* p, int loss, double huber_delta) {
  const bool was = robust();
  if (loss != loss_) mad_recorded_ = false;  // the record of a step belongs to the loss it ran under
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
    const T* prior = prior_ ? prior_.as<const T>() + (size_t)c0 * nl : nullptr;
    const double* delta_dev = nullptr;
    if (scale_mode_ == SRMAP_HUBER_DELTA_MAD) {  // delta from the scale of these residuals; what counts is the prior's support
      if (int r = launch_residual_scale<T>(p, p->d_resid.as<const T>(), prior, (size_t)geo.C * nl, (size_t)p->geo.C * nl, 0, true,
                                           tuning_, min_delta_, st))
        return r;
      delta_dev = residual_scale_record(p, 0);
      mad_recorded_ = true;
    }
    return launch_huber_weights<T>(p, p->d_resid.as<const T>(), eff_.as<T>() + (size_t)c0 * nl, (size_t)geo.K, (size_t)geo.C * nl,
                                   (size_t)geo.C * nl, (size_t)p->geo.C * nl, delta_, st, prior, delta_dev);
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
  return p->dw.set_user(p, {nullptr, w_dev, stream_of(p->ctx, hip_stream)});
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
  return p->dw.set_prior(p, {nullptr, m_dev, stream_of(p->ctx, hip_stream)});
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
  const void* m = p->dw.caller_prior<void>();  // under a hold-out still what the caller set
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
  return p->dw.huber_step(p, 0, 0, x_dev, stream_of(p->ctx, hip_stream));
}

}  // extern "C"
