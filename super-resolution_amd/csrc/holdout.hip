// holdout.hip -- hold-out validation of the data term (no reference counterpart): the kernel that forms
// the prior's factor 1 - h, the score of the held-out observations at an image x, and the C entry points
// srmap_problem_set_holdout / _get_holdout and srmap_holdout_score*.  Which observation is held out is a function of its
// index (holdout_host.hpp; the device copy is holdout_dev.hpp's): no mask is stored anywhere.  Where the factor lives and
// what reads it: data_weights.hpp.
#include <cmath>
#include <cstdint>
#include <vector>

#include "holdout_dev.hpp"
#include "holdout_host.hpp"
#include "motion_fit_dev.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

namespace {

// out[i] = 0 where observation i is held out, else m[i] (HAS_M) or 1: the product m .* (1 - h), exact because h is 0 or 1.
// Elementwise over the whole [K][C][h][w], i its flat index: 16-byte accesses in a grid-stride loop (both buffers are
// whole allocations), the last elements one by one.  The instance without m reads nothing.
template <typename T, bool HAS_M>
__global__ __launch_bounds__(256) void k_holdout_prior(const T* __restrict__ m, T* __restrict__ out, size_t n,
                                                      unsigned long long seed, unsigned lo, unsigned hi) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(16 / sizeof(T))));
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
  const size_t nv = n / V;
  for (size_t g = tid; g < nv; g += nth) {
    VT o;
    if constexpr (HAS_M) o = reinterpret_cast<const VT*>(m)[g];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const T keep = HAS_M ? o[q] : T(1);
      o[q] = holdout_held_dev((uint64_t)(g * V + q), seed, lo, hi) ? T(0) : keep;
    }
    reinterpret_cast<VT*>(out)[g] = o;
  }
  for (size_t i = nv * V + tid; i < n; i += nth) {
    const T keep = HAS_M ? m[i] : T(1);
    out[i] = holdout_held_dev((uint64_t)i, seed, lo, hi) ? T(0) : keep;
  }
}

constexpr int kHoldSums = 4;  // S1 = sum u rho, S2 = sum u rho^2, S0 = sum u, n = #{u > 0}, over the held-out observations

// The sums of the score over the residuals r, [K] runs of rowlen elements (blockIdx.y = frame k; element j of the run is
// observation k * rowlen + j of the whole problem, from which h is recomputed: there is no mask stream).  BASE streams of
// base weights, indexed like r: 0 -- u = 1; 1 -- u = a; 2 -- u = a * b, the product rounded once in T as the effective
// weights are.  rho(r) = r^2 where delta == 0 or |r| <= delta, (2 delta) |r| - delta^2 beyond; delta is *delta_dev when that
// is given (the record of the last Huber step, residual_scale.hip), else the argument.  A thread adds its elements to four
// doubles in the order it meets them -- the run's unaligned head, its 16-byte groups (elements in index order), its tail,
// each in a grid-stride loop -- every operation rounded on its own; the workgroup's sums go to its record (fold_sums_256).
// No atomics: for a given launch shape the result is the same bits every time.  16-byte loads over the part of the run
// that is 16-byte aligned in every stream, as k_select_hist does.
template <typename T, int BASE>
__global__ __launch_bounds__(256) void k_holdout_sums(const T* __restrict__ r, const T* __restrict__ a, const T* __restrict__ b,
                                                     size_t rowlen, unsigned long long seed, unsigned lo, unsigned hi, double delta,
                                                     const double* __restrict__ delta_dev, double* __restrict__ part) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(16 / sizeof(T))));
  __shared__ double red[kHoldSums][4];
  const int k = blockIdx.y;
  const double dl = delta_dev ? *delta_dev : delta;
  const T* rr = r + (size_t)k * rowlen;
  const T* aa = BASE >= 1 ? a + (size_t)k * rowlen : nullptr;
  const T* bb = BASE >= 2 ? b + (size_t)k * rowlen : nullptr;
  const uint64_t i0 = (uint64_t)k * rowlen;
  double acc[kHoldSums] = {0.0, 0.0, 0.0, 0.0};
  auto take = [&](size_t j, T rv, T uv) {
#pragma clang fp contract(off)
    if (!holdout_held_dev(i0 + j, seed, lo, hi)) return;
    const double u = (double)uv, rd = (double)rv, ar = fabs(rd);
    double rho = rd * rd;
    if (dl > 0.0 && ar > dl) {
      const double lin = (2.0 * dl) * ar, sq = dl * dl;
      rho = lin - sq;
    }
    const double t = u * rho;
    acc[0] += t;
    acc[1] += t * rho;
    acc[2] += u;
    acc[3] += u > 0.0 ? 1.0 : 0.0;
  };
  auto base = [&](T av, T bv) { return BASE == 0 ? T(1) : BASE == 1 ? av : (T)(av * bv); };
  size_t head = ((16 - reinterpret_cast<uintptr_t>(rr) % 16) % 16) / sizeof(T);
  if (head > rowlen) head = rowlen;
  if (BASE >= 1 && (reinterpret_cast<uintptr_t>(aa) - reinterpret_cast<uintptr_t>(rr)) % 16 != 0) head = rowlen;  // no common alignment
  if (BASE >= 2 && (reinterpret_cast<uintptr_t>(bb) - reinterpret_cast<uintptr_t>(rr)) % 16 != 0) head = rowlen;
  const size_t nv = (rowlen - head) / V;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
  for (size_t j = tid; j < head; j += nth) take(j, rr[j], base(BASE >= 1 ? aa[j] : T(1), BASE >= 2 ? bb[j] : T(1)));
  for (size_t g = tid; g < nv; g += nth) {
    const VT v = reinterpret_cast<const VT*>(rr + head)[g];
    VT av, bv;
    if constexpr (BASE >= 1) av = reinterpret_cast<const VT*>(aa + head)[g];
    if constexpr (BASE >= 2) bv = reinterpret_cast<const VT*>(bb + head)[g];
#pragma unroll
    for (int q = 0; q < V; ++q) take(head + g * V + q, v[q], base(BASE >= 1 ? av[q] : T(1), BASE >= 2 ? bv[q] : T(1)));
  }
  for (size_t j = head + nv * V + tid; j < rowlen; j += nth) take(j, rr[j], base(BASE >= 1 ? aa[j] : T(1), BASE >= 2 ? bb[j] : T(1)));
  fold_sums_256(acc, red, part + ((size_t)k * gridDim.x + blockIdx.x) * kHoldSums);
}

// workgroups per frame of the score: the device a few times over in all, no more than the run has 16-byte groups
template <typename T>
int holdout_sums_groups(const srmap_problem* p, size_t rowlen) {
  constexpr size_t V = 16 / sizeof(T);
  const size_t gmax = (size_t)std::max(1, std::max(1, p->ctx->num_cus) * 4 / p->geo.K);
  return (int)std::max<size_t>(1, std::min(gmax, (rowlen + V * 256 - 1) / (V * 256)));
}

}  // namespace

template <typename T>
int launch_holdout_prior(srmap_problem* p, const T* m, T* out, size_t n, unsigned long long seed, unsigned lo, unsigned hi, hipStream_t st) {
  constexpr size_t V = 16 / sizeof(T);
  if (n == 0) return SRMAP_OK;
  const size_t cap = (size_t)std::max(1, p->ctx->num_cus) * 8;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min((n + V * 256 - 1) / (V * 256), cap));
  if (m) hipLaunchKernelGGL((k_holdout_prior<T, true>), dim3(blocks), dim3(256), 0, st, m, out, n, seed, lo, hi);
  else hipLaunchKernelGGL((k_holdout_prior<T, false>), dim3(blocks), dim3(256), 0, st, m, out, n, seed, lo, hi);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}
template int launch_holdout_prior<float>(srmap_problem*, const float*, float*, size_t, unsigned long long, unsigned, unsigned, hipStream_t);
template int launch_holdout_prior<double>(srmap_problem*, const double*, double*, size_t, unsigned long long, unsigned, unsigned, hipStream_t);

void holdout_pass_release(srmap_problem* p) {
  delete p->holdout_pass;
  p->holdout_pass = nullptr;
}

// The residual pass at x, then the sums: h_sums of the problem's pass holds S1, S2, S0, n of every frame on return
template <typename T>
static int holdout_sums(srmap_problem* p, const T* x, double delta, const double* delta_dev, hipStream_t st) {
  const Geometry& g = p->geo;
  const size_t run = (size_t)g.C * g.w * g.h;
  const int G = holdout_sums_groups<T>(p, run);
  if (!p->holdout_pass) {
    FitPass* fp = new FitPass();
    if (!fp->alloc(g.K, kHoldSums, (size_t)g.K * G * kHoldSums, false)) {
      delete fp;
      return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (hold-out score: %d x %d records)", g.K, G);
    }
    p->holdout_pass = fp;
  }
  if (int rc = launch_forward_residual<T>(p, g, 0, x, p->d_partials.as<double>(), st)) return rc;
  // the base weight: what the observation would weigh were it not held out, before any Huber factor -- under L2 the
  // caller's prior times the caller's weights, under Huber the caller's prior
  const T* a = p->dw.caller_prior<T>();
  const T* b = p->dw.loss() == SRMAP_DATA_LOSS_HUBER ? nullptr : p->dw.user<T>();
  if (!a) { a = b; b = nullptr; }
  const T* r = p->d_resid.as<const T>();
  const DataWeights::Holdout& h = p->dw.holdout();
  double* part = p->holdout_pass->d_part.as<double>();
  const dim3 grid(G, g.K);
  if (a && b) hipLaunchKernelGGL((k_holdout_sums<T, 2>), grid, dim3(256), 0, st, r, a, b, run, h.seed, h.lo, h.threshold, delta, delta_dev, part);
  else if (a) hipLaunchKernelGGL((k_holdout_sums<T, 1>), grid, dim3(256), 0, st, r, a, b, run, h.seed, h.lo, h.threshold, delta, delta_dev, part);
  else hipLaunchKernelGGL((k_holdout_sums<T, 0>), grid, dim3(256), 0, st, r, a, b, run, h.seed, h.lo, h.threshold, delta, delta_dev, part);
  SRMAP_HIP(p->ctx, hipGetLastError());
  if (!p->holdout_pass->reduce_and_fetch(G, st))
    return set_error(p->ctx, SRMAP_EHIP, "hold-out score: the reduction of the sums failed: %s", hipGetErrorString(hipGetLastError()));
  return SRMAP_OK;
}

}  // namespace srmap

extern "C" {

int srmap_problem_set_holdout(srmap_problem* p, double fraction, unsigned long long seed) {
  if (!p) return SRMAP_EINVAL;
  DataWeights::Holdout h;
  if (fraction != 0.0) {
    h.threshold = holdout_threshold(fraction);
    if (!h.threshold)
      return set_error(p->ctx, SRMAP_EINVAL, "the hold-out fraction must be in (0, 0.5] and at least 2^-%d, or 0 to lift the hold-out (got %g)",
                       kHoldoutBits, fraction);
    h.seed = seed;
    h.fraction = fraction;
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return p->dw.set_holdout(p, h);
}

int srmap_problem_set_holdout_fold(srmap_problem* p, int folds, int fold, unsigned long long seed) {
  if (!p) return SRMAP_EINVAL;
  DataWeights::Holdout h;
  if (folds != 0) {
    if (!holdout_fold_band(folds, fold, &h.lo, &h.threshold))
      return set_error(p->ctx, SRMAP_EINVAL, "srmap_problem_set_holdout_fold: folds must be in %d...%d and 0 <= fold < folds, or folds 0 to lift the hold-out (got folds %d, fold %d)",
                       kHoldoutMinFolds, kHoldoutMaxFolds, folds, fold);
    h.seed = seed;
    h.fraction = std::ldexp((double)(h.threshold - h.lo), -kHoldoutBits);
    h.folds = folds;
    h.fold = fold;
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return p->dw.set_holdout(p, h);
}

int srmap_problem_get_holdout_fold(srmap_problem* p, int* folds, int* fold, unsigned long long* seed) {
  if (!p) return SRMAP_EINVAL;
  const DataWeights::Holdout& h = p->dw.holdout();
  if (folds) *folds = h.folds;
  if (fold) *fold = h.fold;
  if (seed) *seed = h.seed;
  return SRMAP_OK;
}

int srmap_problem_get_holdout(srmap_problem* p, double* fraction, unsigned long long* seed, double* mask_out, double* counts) {
  if (!p) return SRMAP_EINVAL;
  const DataWeights::Holdout& h = p->dw.holdout();
  if (fraction) *fraction = h.fraction;
  if (seed) *seed = h.seed;
  if (!mask_out && !counts) return SRMAP_OK;
  const Geometry& g = p->geo;
  const size_t n = p->lr_count(), run = (size_t)g.C * g.w * g.h;
  if (!mask_out) {  // the counts alone: no device work -- kept from an earlier call, or counted once with the plain-C++ twin
    if (p->holdout_counts.empty()) {
      p->holdout_counts.assign(1 + (size_t)g.K, 0.0);
      for (int k = 0; k < g.K && h.threshold; ++k) {
        double c = 0.0;
        for (size_t j = 0; j < run; ++j) c += holdout_held_band((uint64_t)k * run + j, h.seed, h.lo, h.threshold) ? 1.0 : 0.0;
        p->holdout_counts[1 + k] = c;
        p->holdout_counts[0] += c;
      }
    }
    for (int s = 0; s <= g.K; ++s) counts[s] = p->holdout_counts[s];
    return SRMAP_OK;
  }
  double* mask = mask_out;
  if (!h.threshold) {
    for (size_t i = 0; i < n; ++i) mask[i] = 0.0;
  } else {  // from the device's copy of the hash: 1 - h as the prior's kernel forms it, read back
    SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
    DevBuf keep;
    if (keep.alloc(n * p->elem()) != hipSuccess) return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (hold-out mask: %zu bytes)", n * p->elem());
    const hipStream_t st = p->ctx->stream;
    int rc = dispatch_dtype(p->dtype, [&](auto t) {
      using T = decltype(t);
      return launch_holdout_prior<T>(p, (const T*)nullptr, keep.as<T>(), n, h.seed, h.lo, h.threshold, st);
    });
    if (rc == SRMAP_OK) rc = convert_download(p, keep.as(), mask, n, st);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) mask[i] = 1.0 - mask[i];
  }
  if (counts) {
    counts[0] = 0.0;
    for (int k = 0; k < g.K; ++k) {
      double c = 0.0;
      for (size_t j = 0; j < run; ++j) c += mask[(size_t)k * run + j];
      counts[1 + k] = c;
      counts[0] += c;
    }
    p->holdout_counts.assign(counts, counts + 1 + g.K);
  }
  return SRMAP_OK;
}

int srmap_holdout_score_device(srmap_problem* p, const void* x_dev, void* hip_stream, double delta, double* score, double* sums) {
  if (!p || !x_dev || !score) return SRMAP_EINVAL;
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  if (!p->dw.holdout().threshold) return set_error(p->ctx, SRMAP_EINVAL, "no hold-out set (srmap_problem_set_holdout)");
  if (!(delta == delta) || std::isinf(delta)) return set_error(p->ctx, SRMAP_EINVAL, "the score's delta must be finite (got %g)", delta);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const double* delta_dev = nullptr;
  if (delta < 0.0) {  // the problem's
    delta = 0.0;
    if (p->dw.loss() == SRMAP_DATA_LOSS_HUBER) {
      if (p->dw.scale_mode() == SRMAP_HUBER_DELTA_MAD) {
        if (!p->dw.mad_delta_recorded())
          return set_error(p->ctx, SRMAP_EINVAL, "the problem's delta is the last Huber step's (SRMAP_HUBER_DELTA_MAD) and no step has run: solve first, or pass a delta");
        delta_dev = residual_scale_record(p, 0);
      } else {
        delta = p->dw.delta();
      }
    }
  }
  const hipStream_t st = stream_of(p->ctx, hip_stream);
  // d_resid and the pass's buffers are written: ordered like a state write, and complete on return
  int rc = state_begin_write(p, st);
  if (rc == SRMAP_OK) rc = problem_state_read(p, st);
  if (rc == SRMAP_OK) rc = ensure_eval_partials(p);
  if (rc) return rc;
  rc = dispatch_dtype(p->dtype, [&](auto t) { return holdout_sums<decltype(t)>(p, (const decltype(t)*)x_dev, delta, delta_dev, st); });
  if (rc) return rc;
  const int K = p->geo.K;
  double tot[kHoldSums] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < K; ++k) {  // the frames in index order
    const double* s = p->holdout_pass->sums(k);
    for (int q = 0; q < kHoldSums; ++q) {
      tot[q] += s[q];
      if (sums) sums[(size_t)(1 + k) * kHoldSums + q] = s[q];
    }
    score[1 + k] = s[2] != 0.0 ? s[0] / s[2] : 0.0;
  }
  for (int q = 0; q < kHoldSums && sums; ++q) sums[q] = tot[q];
  if (!(tot[3] > 0.0)) {
    score[0] = 0.0;
    return set_error(p->ctx, SRMAP_EINVAL, "nothing is held out: no held-out observation has a base weight above 0");
  }
  score[0] = tot[0] / tot[2];
  return SRMAP_OK;
}

int srmap_holdout_score(srmap_problem* p, const double* x_host, double delta, double* score, double* sums) {
  if (!p || !x_host || !score) return SRMAP_EINVAL;
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  if (!p->dw.holdout().threshold) return set_error(p->ctx, SRMAP_EINVAL, "no hold-out set (srmap_problem_set_holdout)");
  if (int rc = stage_host_x(p, x_host)) return rc;
  return srmap_holdout_score_device(p, p->d_x.as(), p->ctx->stream, delta, score, sums);
}

}  // extern "C"
