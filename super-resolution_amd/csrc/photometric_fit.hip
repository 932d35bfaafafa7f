// photometric_fit.hip -- the photometric frame model (srmap_problem_set_photometric, srmap_fit_photometric):
// frame k is y_k = a_k (D B M_k x) + b_k + noise, and the problem solves against the NORMALISED frames
// (y_k - b_k) / a_k.  Only the observation buffer changes: every kernel that reads observations reads p->d_obs, which is
// the normalised copy while parameters are set (the raw frames stay in p->d_obs_raw).  No reference counterpart; the
// checker is tests/photometric_restatement.py.
//   normalise k_photometric_normalise: per element, in double on the stored value, the subtraction, a true division, one
//             rounding to the problem's dtype (no reciprocal, no contraction: a numpy restatement is bit-identical);
//   pass      ONE launch of k_photometric_sums over every frame: per LR pixel and channel s = (D B M_k x)(c, u), M_k
//             sampled as the problem's forward kernel samples it (MotionSampler of sample_dev.hpp; the
//             identity without motion), the blur in force; six f64 sums per
//             workgroup {w, w s, w y, w s^2, w s y, w y^2} held in registers in both dtypes, folded by a wave shuffle and
//             LDS in a fixed order, no atomics (fold_sums_256); k_fit_reduce adds the chunk records in index order;
//   pacing    one launch, one reduce, one copy of K x 6 doubles, one stream wait (FitPass without a table, motion_fit.hip);
//   solve     on the host in double, per frame: the 2 x 2 (or 1 x 1) system of photometric_host.hpp.
#include <algorithm>
#include <cmath>
#include <vector>

#include "motion_fit_dev.hpp"
#include "photometric_host.hpp"
#include "sample_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kMaxChunks = 256;

// out[i] = (raw[i] - bias_k) / gain_k rounded once to T, k the frame of element i; gb[k] = {gain, bias}
template <typename T>
__global__ __launch_bounds__(256) void k_photometric_normalise(const T* __restrict__ raw, T* __restrict__ out,
                                                               const double* __restrict__ gb, size_t per_frame,
                                                               size_t total) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t k = i / per_frame;
  const double d = (double)raw[i] - gb[2 * k + 1];
  out[i] = (T)(d / gb[2 * k]);
}

// The six sums of every frame: grid = (chunks of LR pixels, frames), 256 threads; a workgroup covers the LR pixels
// [chunk * 256 * ppt, (chunk + 1) * 256 * ppt) of its frame, thread t the pixels t, t + 256, ..., every channel of each.
// partial[(k * chunks + chunk)][6].
template <typename T, int MOTION, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_photometric_sums(const T* __restrict__ x, const T* __restrict__ y,
                                                          const T* __restrict__ dw, Geometry g,
                                                          MotionArgs<T> ma, const T* __restrict__ blur,
                                                          const int* __restrict__ col_map, const int* __restrict__ row_map,
                                                          int ppt, double* __restrict__ partial, BlurStride bs) {
  __shared__ double red[kPhotoSums][4];
  const int k = blockIdx.y;
  const int n = g.w * g.h;
  const MotionSampler<T, MOTION> ms(ma, g, k);  // uniform
  double acc[kPhotoSums];
#pragma unroll
  for (int q = 0; q < kPhotoSums; ++q) acc[q] = 0.0;
  const size_t base = (size_t)blockIdx.x * 256 * ppt + threadIdx.x;
  for (int t = 0; t < ppt; ++t) {
    const size_t lp = base + (size_t)t * 256;
    if (lp >= (size_t)n) break;
    const int i = (int)(lp / g.w), j = (int)(lp - (size_t)i * g.w);
    const int R0 = row_map[i], C0 = col_map[j];
    for (int c = 0; c < g.C; ++c) {
      const T* __restrict__ plane = x + (size_t)c * g.W * g.H;
      const T* __restrict__ blur_kc = blur + ((size_t)k * bs.frame + (size_t)c * bs.channel);  // a bank's entry; strides 0 without one
      const size_t oi = ((size_t)k * g.C + c) * n + lp;
      const double yv = (double)y[oi];
      const double wv = WEIGHTED ? (double)dw[oi] : 1.0;
      double s = 0.0;
      for (int a = 0; a < g.b; ++a) {
        const int rr = R0 + a - g.hb;
        if (rr < 0 || rr >= g.H) continue;  // the forward kernels' taps: the blur's zero border on the warped image
        for (int e = 0; e < g.b; ++e) {
          const int cc = C0 + e - g.hb;
          if (cc < 0 || cc >= g.W) continue;
          const double v = ms.template at<double>(plane, g.W, g.H, rr, cc);
          s += (double)blur_kc[a * g.b + e] * v;
        }
      }
      const double ws = wv * s, wy = wv * yv;
      acc[kPhotoW] += wv;
      acc[kPhotoS] += ws;
      acc[kPhotoY] += wy;
      acc[kPhotoSS] += ws * s;
      acc[kPhotoSY] += ws * yv;
      acc[kPhotoYY] += wy * yv;
    }
  }
  fold_sums_256(acc, red, partial + ((size_t)k * gridDim.x + blockIdx.x) * kPhotoSums);
}

// the instance of the problem's motion kind; false: the kind has none (a displacement field, which the entry point refuses)
template <typename T>
bool launch_sums(srmap_problem* p, const T* x, int chunks, int ppt, double* d_part, hipStream_t st) {
  const Geometry& g = p->geo;
  dim3 grid(chunks, g.K);
  const T* y = (p->d_obs_raw ? p->d_obs_raw : p->d_obs).as<const T>();  // always the RAW frames: the fit is absolute
  const MotionArgs<T> ma = p->motion.args<T>();
  const BlurStride bs = p->blur.stride();
  const T* dw = p->dw.effective<T>();
  return dispatch_value<kMotionNone, kMotionTable, kMotionAffine>(p->motion.kind(), [&](auto motion) {
    constexpr int MOTION = decltype(motion)::value;
    dispatch_value<0, 1>(dw != nullptr, [&](auto weighted) {
      hipLaunchKernelGGL((k_photometric_sums<T, MOTION, decltype(weighted)::value != 0>), grid, dim3(256), 0, st, x, y, dw, g, ma,
                         p->blur.table<T>(), p->d_col_map.as<int>(), p->d_row_map.as<int>(), ppt, d_part, bs);
    });
  });
}

}  // namespace

// p->d_obs <- the raw frames (p->d_obs_raw) normalised by the parameters in force (p->d_photo), enqueued on st
int photometric_normalise(srmap_problem* p, hipStream_t st) {
  const size_t total = p->lr_count(), per_frame = total / p->geo.K;
  if (!p->d_obs) SRMAP_HIP(p->ctx, p->d_obs.alloc(total * p->elem()));
  const dim3 grid((unsigned)((total + 255) / 256));
  dispatch_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_photometric_normalise<T>, grid, dim3(256), 0, st, p->d_obs_raw.as<const T>(), p->d_obs.as<T>(),
                       p->d_photo.as<double>(), per_frame, total);
  });
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

}  // namespace srmap

using namespace srmap;

extern "C" int srmap_problem_set_photometric(srmap_problem* p, const double* gain_bias) {
  if (!p) return SRMAP_EINVAL;
  srmap_ctx* ctx = p->ctx;
  const int K = p->geo.K;
  if (gain_bias)
    for (int k = 0; k < K; ++k) {
      const double a = gain_bias[2 * k], b = gain_bias[2 * k + 1];
      if (!std::isfinite(a) || !std::isfinite(b) || !(a > 0.0))
        return set_error(ctx, SRMAP_EINVAL, "photometric: frame %d has gain %g, bias %g: finite numbers and a gain > 0 are needed", k, a, b);
    }
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  // what the call needs first: a failed allocation leaves the problem as it was
  DevBuf photo, norm;
  const bool move_raw = gain_bias && !p->d_obs_raw && p->d_obs;  // the first parameters of a problem that holds frames
  if (gain_bias && ((!p->d_photo && photo.alloc((size_t)K * 2 * sizeof(double)) != hipSuccess) ||
                    (move_raw && norm.alloc(p->lr_count() * p->elem()) != hipSuccess)))
    return set_error(ctx, SRMAP_ENOMEM, "photometric: allocation failed");
  // evaluations in flight read the observations: drain them before the buffer changes
  if (int rc = model_drain(p)) return rc;
  if (!gain_bias) {
    // d_obs_raw -> d_obs: the raw buffer again, bit for bit (the normalised copy is freed); setting parameters moves it back
    if (p->d_obs_raw) p->d_obs = std::move(p->d_obs_raw);
    p->d_photo.reset();
    p->photometric = false;
    p->photo.clear();
    return SRMAP_OK;
  }
  if (photo) p->d_photo = std::move(photo);
  SRMAP_HIP(ctx, hipMemcpy(p->d_photo.as<double>(), gain_bias, (size_t)K * 2 * sizeof(double), hipMemcpyHostToDevice));
  p->photo.assign(gain_bias, gain_bias + (size_t)K * 2);
  p->photometric = true;
  if (move_raw) {
    p->d_obs_raw = std::move(p->d_obs);
    p->d_obs = std::move(norm);
  }
  if (p->d_obs_raw && p->have_obs) {
    int rc = photometric_normalise(p, ctx->stream);
    if (rc) return rc;
    SRMAP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // complete on return: any stream may evaluate
  }
  return SRMAP_OK;
}

extern "C" int srmap_problem_get_photometric(const srmap_problem* p, double* gain_bias_out, int* is_set) {
  if (!p) return SRMAP_EINVAL;
  if (is_set) *is_set = p->photometric ? 1 : 0;
  if (gain_bias_out)
    for (int k = 0; k < p->geo.K; ++k) {
      gain_bias_out[2 * k] = p->photometric ? p->photo[2 * (size_t)k] : 1.0;
      gain_bias_out[2 * k + 1] = p->photometric ? p->photo[2 * (size_t)k + 1] : 0.0;
    }
  return SRMAP_OK;
}

extern "C" void srmap_photometric_fit_options_default(srmap_photometric_fit_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_photometric_fit_options);
  o->model = 0;
  o->gauge_frame = 0;
  o->min_gain = 0.25;
  o->max_gain = 4.0;
  o->apply = 1;
}

// the checks of the options' values (they need no device)
static int photometric_option_values(srmap_problem* p, const srmap_photometric_fit_options& opt) {
  srmap_ctx* ctx = p->ctx;
  if (opt.model < kPhotoGainBias || opt.model > kPhotoBiasOnly)
    return set_error(ctx, SRMAP_EINVAL, "photometric fit: model must be 0, 1 or 2 (got %d)", opt.model);
  if (opt.gauge_frame < -1 || opt.gauge_frame >= p->geo.K)
    return set_error(ctx, SRMAP_EINVAL, "photometric fit: gauge_frame %d is no frame of the problem (and not -1)", opt.gauge_frame);
  if (!std::isfinite(opt.min_gain) || !std::isfinite(opt.max_gain) || !(opt.min_gain > 0.0) || !(opt.max_gain >= opt.min_gain))
    return set_error(ctx, SRMAP_EINVAL, "photometric fit: the gain bounds must be finite with 0 < min_gain <= max_gain");
  return SRMAP_OK;
}

extern "C" int srmap_fit_photometric_device(srmap_problem* p, const void* x_dev, void* hip_stream,
                                            const srmap_photometric_fit_options* options, double* gain_bias_out,
                                            double* quality_out, double* sums_out) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  srmap_ctx* ctx = p->ctx;
  if (p->motion.is_field())
    return p->motion.refuse(ctx, SRMAP_EUNSUPPORTED, "the photometric fit has no sampling leg for %s: not available while one is set (%s)");
  srmap_photometric_fit_options opt;
  int rc = options_in_force(ctx, options, srmap_photometric_fit_options_default, "srmap_photometric_fit_options", &opt);
  if (!rc) rc = photometric_option_values(p, opt);
  if (rc) return rc;
  if (!p->have_obs) return set_error(ctx, SRMAP_EINVAL, "no observations set");
  const Geometry& g = p->geo;
  const int K = g.K;

  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream_of(ctx, hip_stream);
  rc = problem_state_read(p, st);
  if (rc) return rc;

  const PixelChunks plan = plan_pixel_chunks(g.w * g.h, kMaxChunks);
  const int ppt = plan.ppt, chunks = plan.chunks;
  FitPass fit;  // no table: every frame is fitted in the one pass
  if (!fit.alloc(K, kPhotoSums, (size_t)K * chunks * kPhotoSums, false)) return set_error(ctx, SRMAP_ENOMEM, "photometric fit: allocation failed");
  if (!dispatch_dtype(p->dtype, [&](auto t) { return launch_sums<decltype(t)>(p, (const decltype(t)*)x_dev, chunks, ppt, fit.d_part.as<double>(), st); }))
    return set_error(ctx, SRMAP_EINVAL, "internal: the photometric fit has no kernel for motion kind %d", (int)p->motion.kind());
  if (!fit.reduce_and_fetch(chunks, st)) return set_error(ctx, SRMAP_EHIP, "photometric fit: pass failed");

  // ---- the host solve, frame by frame ----
  std::vector<double> gb((size_t)K * 2);
  for (int k = 0; k < K; ++k) {
    const double a_cur = p->photometric ? p->photo[2 * (size_t)k] : 1.0;
    const double b_cur = p->photometric ? p->photo[2 * (size_t)k + 1] : 0.0;
    PhotometricFit f = photometric_solve(fit.sums(k), opt.model, a_cur, b_cur, opt.min_gain, opt.max_gain);
    if (k == opt.gauge_frame) {  // the gauge keeps its parameters
      f.gain = a_cur; f.bias = b_cur; f.e1 = f.e0; f.status = 0;
    }
    gb[2 * (size_t)k] = f.gain;
    gb[2 * (size_t)k + 1] = f.bias;
    if (quality_out) {
      double* q = quality_out + 4 * (size_t)k;
      q[0] = f.e0; q[1] = f.e1; q[2] = fit.sums(k)[kPhotoW]; q[3] = f.status;
    }
    if (sums_out) std::copy(fit.sums(k), fit.sums(k) + kPhotoSums, sums_out + (size_t)kPhotoSums * k);
  }
  if (opt.apply) {
    rc = srmap_problem_set_photometric(p, gb.data());
    if (rc) return rc;
  }
  if (gain_bias_out) std::copy(gb.begin(), gb.end(), gain_bias_out);
  return SRMAP_OK;
}

extern "C" int srmap_fit_photometric(srmap_problem* p, const double* x_host, const srmap_photometric_fit_options* options,
                                     double* gain_bias_out, double* quality_out, double* sums_out) {
  if (!p || !x_host) return SRMAP_EINVAL;
  if (int rc = host_fit_prologue(p, x_host, options, srmap_photometric_fit_options_default, "srmap_photometric_fit_options",
                                 photometric_option_values))
    return rc;
  return srmap_fit_photometric_device(p, p->d_x.as(), p->ctx->stream, options, gain_bias_out, quality_out, sums_out);
}
