// srmap_api.hip -- C ABI (include/srmap.h) of the MI355X MAP gradient path:
// problem set-up (what the reference's ImageModel / MapSolver constructors do
// on the host), buffer management, and the dispatch of one cost+gradient
// evaluation onto the HIP kernels.  No CPU compute path exists here: every
// numeric entry point launches gfx950 kernels or fails.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <new>

#include "affine_map.hpp"
#include "solver_passes.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

int set_error(srmap_ctx* ctx, int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->error = buf;
  return status;
}

// ---- host restatement of the OpenCV 3.x parameter arithmetic the reference
// relies on (the per-pixel work itself happens in the kernels) ----

static inline int cv_round(double v) { return (int)std::lrint(v); }

// cv::warpAffine fixed-point coordinate tables for M = [1 0 dx; 0 1 dy]
// (motion_module.cpp:18-25): AB_BITS = 10, INTER_BITS = 5.
static void warp_tables(int W, int H, double dx, double dy, std::vector<int>* X,
                        std::vector<int>* Y) {
  double M[6] = {1.0, 0.0, dx, 0.0, 1.0, dy};
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1.0 / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
  X->resize(W);
  Y->resize(H);
  for (int x = 0; x < W; ++x)
    (*X)[x] = (cv_round((M[1] * 0 + M[2]) * 1024) + 16 + cv_round(M[0] * x * 1024)) >> 5;
  for (int y = 0; y < H; ++y)
    (*Y)[y] = (cv_round((M[4] * y + M[5]) * 1024) + 16 + cv_round(M[3] * 0 * 1024)) >> 5;
}

static int make_warp(srmap_ctx* ctx, int W, int H, double dx, double dy,
                     WarpTaps<double>* out, std::vector<int>* ytab) {
  if (!(std::fabs(dx) < 16000.0) || !(std::fabs(dy) < 16000.0))
    return set_error(ctx, SRMAP_EUNSUPPORTED, "motion shift (%g, %g) too large", dx, dy);
  std::vector<int> X, Y;
  warp_tables(W, H, dx, dy, &X, &Y);
  for (int x = 0; x < W; ++x)
    if (X[x] != X[0] + 32 * x)  // adelta[x] + a constant: cannot happen for a pure translation
      return set_error(ctx, SRMAP_EUNSUPPORTED, "non-uniform warpAffine x table");
  bool uniform_y = true;
  for (int y = 0; y < H; ++y)
    if (Y[y] != Y[0] + 32 * y) uniform_y = false;
  out->ox = X[0] >> 5;
  out->oy = Y[0] >> 5;
  const int fx = X[0] & 31, fy = Y[0] & 31;
  // BilinearTab_f: float32 table; the products are exact multiples of 1/1024.
  const float tx1 = (float)fx * (1.f / 32), tx0 = 1.f - tx1;
  const float ty1 = (float)fy * (1.f / 32), ty0 = 1.f - ty1;
  out->w[0] = ty0 * tx0; out->w[1] = ty0 * tx1; out->w[2] = ty1 * tx0; out->w[3] = ty1 * tx1;
  out->ntaps = (fx == 0 && fy == 0) ? 1 : 4;
  out->fx = fx;
  out->ytab = nullptr;
  ytab->clear();
  if (!uniform_y) {
    // dy within floating-point rounding of a 1/32-px quantisation tie: warpAffine's per-row y coordinate
    // (cvRound((y + b) * 1024) evaluated in double) lands on either side of the tie depending on the row.  The
    // kernels then read the source row and fraction of every destination row from a table.
    ytab->resize(H);
    for (int y = 0; y < H; ++y) (*ytab)[y] = Y[y];  // absolute: source row << 5 | fraction
    out->ntaps = 4;
  }
  return SRMAP_OK;
}

// cv::resize(INTER_NEAREST) source index per destination index
// (image_data.cpp:338-350).
static void nearest_map(int src_len, int dst_len, std::vector<int>* map) {
  const double inv_scale = (double)dst_len / src_len;
  const double ifx = 1.0 / inv_scale;
  map->resize(dst_len);
  for (int x = 0; x < dst_len; ++x) {
    const int sx = (int)std::floor(x * ifx);
    (*map)[x] = sx < src_len - 1 ? sx : src_len - 1;
  }
}

template <typename T>
static int upload_warps(srmap_problem* p, const std::vector<WarpTaps<double>>& src, DevBuf* dst) {
  std::vector<WarpTaps<T>> tmp(src.size());
  for (size_t i = 0; i < src.size(); ++i) {
    tmp[i].ox = src[i].ox; tmp[i].oy = src[i].oy; tmp[i].ntaps = src[i].ntaps; tmp[i].fx = src[i].fx;
    tmp[i].ytab = src[i].ytab;
    for (int t = 0; t < 4; ++t) tmp[i].w[t] = (T)src[i].w[t];
  }
  SRMAP_HIP(p->ctx, dst->alloc(sizeof(WarpTaps<T>) * tmp.size()));
  SRMAP_HIP(p->ctx, hipMemcpy(dst->as(), tmp.data(), sizeof(WarpTaps<T>) * tmp.size(), hipMemcpyHostToDevice));
  return SRMAP_OK;
}

template <typename T>
static int upload_array(srmap_problem* p, const std::vector<double>& src, DevBuf* dst) {
  std::vector<T> tmp(src.begin(), src.end());
  SRMAP_HIP(p->ctx, dst->alloc(sizeof(T) * tmp.size()));
  SRMAP_HIP(p->ctx, hipMemcpy(dst->as(), tmp.data(), sizeof(T) * tmp.size(), hipMemcpyHostToDevice));
  return SRMAP_OK;
}

template <typename T>
__global__ void k_from_double(const double* __restrict__ src, T* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (T)src[i];
}
template <typename T>
__global__ void k_to_double(const T* __restrict__ src, double* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (double)src[i];
}

// Caller buffers are pageable.  A plain hipMemcpy of them runs at 2-6 GB/s; two
// pinned chunks pipeline the PCIe transfer against the host-side memcpy.
constexpr size_t kStageBytes = 4u << 20;

int ensure_staging(srmap_ctx* ctx) {
  for (int i = 0; i < 2; ++i) {
    if (!ctx->h_stage[i]) SRMAP_HIP(ctx, ctx->h_stage[i].alloc(kStageBytes, hipHostMallocDefault));
    if (!ctx->h_event[i]) SRMAP_HIP(ctx, hipEventCreateWithFlags(&ctx->h_event[i], hipEventDisableTiming));
  }
  if (!ctx->h_scal) {
    SRMAP_HIP(ctx, ctx->h_scal.alloc(16 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    for (int i = 0; i < 16; ++i) ctx->h_scal.as<double>()[i] = 0.0;
  }
  return SRMAP_OK;
}

static int staged_h2d(srmap_ctx* ctx, void* dev, const void* host, size_t bytes, hipStream_t st) {
  int rc = ensure_staging(ctx);
  if (rc) return rc;
  size_t off = 0;
  for (int i = 0; off < bytes; ++i, off += kStageBytes) {
    const size_t nb = bytes - off < kStageBytes ? bytes - off : kStageBytes;
    const int b = i & 1;
    if (i >= 2) SRMAP_HIP(ctx, hipEventSynchronize(ctx->h_event[b]));  // chunk i-2 has left the buffer
    std::memcpy(ctx->h_stage[b].as(), (const char*)host + off, nb);
    SRMAP_HIP(ctx, hipMemcpyAsync((char*)dev + off, ctx->h_stage[b].as(), nb, hipMemcpyHostToDevice, st));
    SRMAP_HIP(ctx, hipEventRecord(ctx->h_event[b], st));
  }
  SRMAP_HIP(ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

static int staged_d2h(srmap_ctx* ctx, void* host, const void* dev, size_t bytes, hipStream_t st) {
  int rc = ensure_staging(ctx);
  if (rc) return rc;
  const size_t nchunks = (bytes + kStageBytes - 1) / kStageBytes;
  for (size_t i = 0; i <= nchunks; ++i) {
    if (i < nchunks) {  // chunk i -> pinned buffer (its previous content, chunk i-2, was copied out below)
      const size_t off = i * kStageBytes, nb = bytes - off < kStageBytes ? bytes - off : kStageBytes;
      SRMAP_HIP(ctx, hipMemcpyAsync(ctx->h_stage[i & 1].as(), (const char*)dev + off, nb, hipMemcpyDeviceToHost, st));
      SRMAP_HIP(ctx, hipEventRecord(ctx->h_event[i & 1], st));
    }
    if (i >= 1) {  // chunk i-1 -> caller, while chunk i is on the wire
      const size_t off = (i - 1) * kStageBytes, nb = bytes - off < kStageBytes ? bytes - off : kStageBytes;
      SRMAP_HIP(ctx, hipEventSynchronize(ctx->h_event[(i - 1) & 1]));
      std::memcpy((char*)host + off, ctx->h_stage[(i - 1) & 1].as(), nb);
    }
  }
  return SRMAP_OK;
}

int convert_upload(srmap_problem* p, const double* host, void* dev, size_t n, hipStream_t st) {
  if (p->dtype == SRMAP_F64) return staged_h2d(p->ctx, dev, host, n * 8, st);
  DevBuf tmp;  // read by the conversion kernel: the stream is waited for before it goes
  SRMAP_HIP(p->ctx, tmp.alloc(n * 8));
  if (int rc = staged_h2d(p->ctx, tmp.as(), host, n * 8, st)) return rc;
  hipLaunchKernelGGL(k_from_double<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     tmp.as<const double>(), (float*)dev, n);
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

int convert_download(srmap_problem* p, const void* dev, double* host, size_t n, hipStream_t st) {
  if (p->dtype == SRMAP_F64) return staged_d2h(p->ctx, host, dev, n * 8, st);
  DevBuf tmp;
  SRMAP_HIP(p->ctx, tmp.alloc(n * 8));
  hipLaunchKernelGGL(k_to_double<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     (const float*)dev, tmp.as<double>(), n);
  return staged_d2h(p->ctx, host, tmp.as(), n * 8, st);
}

static int ensure(srmap_problem* p, DevBuf* buf, size_t bytes) {
  if (!*buf) SRMAP_HIP(p->ctx, buf->alloc(bytes));
  return SRMAP_OK;
}

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
  int rc = ensure_partials(p, partials_needed(p));
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
  if (p->impl == SRMAP_IMPL_TILED && !ztile)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "tiled kernels do not cover this geometry");
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
                                    p->d_resid.as<T>(), 0, geo.K, p->d_partials.as<double>() + nparts, &nb, st, p->d_dw.as<const T>());
      if (rc) return rc;
      nparts += nb;
      if (g) {
        rc = launch_gather_direct<T>(p, geo, p->d_resid.as<const T>(), g, 0, geo.K,
                                     2.0 * geo.s * geo.s, false, st);
        if (rc) return rc;
        g_written = true;
      }
    }
    if (g && !g_written) SRMAP_HIP(p->ctx, hipMemsetAsync(g, 0, N * geo.C * sizeof(T), st));
    if (terms & SRMAP_TERM_REG) {
      for (int r = 0; r < p->nreg; ++r) {
        const RegSpec& rs = p->reg[r];
        if (rs.lambda <= 0.0) continue;  // objective_irls_regularization_term.cpp:16-18
        if (!g) {
          // cost only: the gradient kernel still produces the lambda*w*r^2 partials
        }
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

// ---- stream ordering of the problem's device state (include/srmap.h, "Streams") ----
// before overwriting observations / weights: the last evaluation may still be reading them on another stream
static int state_begin_write(srmap_problem* p, hipStream_t st) {
  if (p->use_stream && p->use_stream != st) SRMAP_HIP(p->ctx, hipStreamSynchronize(p->use_stream));
  return SRMAP_OK;
}
// after an ASYNCHRONOUS write on st: later evaluations on other streams wait for this event
static int state_end_write(srmap_problem* p, hipStream_t st) {
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
  if (p->dtype == SRMAP_F32) return eval_typed<float>(p, req, out, terms, (const float*)x, (float*)g, st);
  return eval_typed<double>(p, req, out, terms, (const double*)x, (double*)g, st);
}

int model_drain(srmap_problem* p) {
  if (p->use_stream) SRMAP_HIP(p->ctx, hipStreamSynchronize(p->use_stream));
  SRMAP_HIP(p->ctx, hipStreamSynchronize(p->ctx->stream));
  return SRMAP_OK;
}

void model_replan(srmap_problem* p) {
  p->plan_gen++;
  if (ztile_plan(p)) ztile_preload(p);
}

// Weights or the loss changed whether the problem is robust(): the tile plan has another form then (ztile_plan)
static void replan_if(srmap_problem* p, bool was_robust) {
  if (p->robust() != was_robust) model_replan(p);
}

// allocate the data weights (all ones) if there are none
static int ensure_data_weights(srmap_problem* p, hipStream_t st) {
  if (p->d_dw) return SRMAP_OK;
  const size_t n = p->lr_count();
  SRMAP_HIP(p->ctx, p->d_dw.alloc(n * p->elem()));
  if (p->dtype == SRMAP_F32) launch_fill<float>(p->d_dw.as<float>(), 1.f, n, st);
  else launch_fill<double>(p->d_dw.as<double>(), 1.0, n, st);
  SRMAP_HIP(p->ctx, hipGetLastError());
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

template <typename T>
static int update_data_weights_typed(srmap_problem* p, int c0, int C, const T* x, hipStream_t st) {
  Geometry geo = p->geo;
  if (C > 0) geo.C = C; else c0 = 0;
  int rc = ensure_partials(p, partials_needed(p));
  if (rc) return rc;
  rc = launch_forward_residual<T>(p, geo, c0, x, p->d_partials.as<double>(), st);  // d_resid: [K][geo.C][h][w], unweighted
  if (rc) return rc;
  const size_t nl = (size_t)geo.w * geo.h;
  return launch_huber_weights<T>(p, p->d_resid.as<const T>(), p->d_dw.as<T>() + (size_t)c0 * nl, (size_t)geo.K, (size_t)geo.C * nl,
                                 (size_t)geo.C * nl, (size_t)p->geo.C * nl, p->huber_delta, st,
                                 p->d_prior ? p->d_prior.as<const T>() + (size_t)c0 * nl : nullptr);
}

int update_data_weights(srmap_problem* p, int c0, int C, const void* x, hipStream_t st) {
  if (p->data_loss != SRMAP_DATA_LOSS_HUBER)
    return set_error(p->ctx, SRMAP_EINVAL, "the data weights are re-derived for a Huber loss only (srmap_problem_set_data_loss)");
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  rc = ensure_data_weights(p, st);
  if (rc) return rc;
  rc = p->dtype == SRMAP_F32 ? update_data_weights_typed<float>(p, c0, C, (const float*)x, st)
                             : update_data_weights_typed<double>(p, c0, C, (const double*)x, st);
  if (rc) return rc;
  return state_end_write(p, st);  // asynchronous: evaluations on other streams wait for this event
}

int reset_data_weights(srmap_problem* p, int c0, int C, hipStream_t st) {
  const Geometry& g = p->geo;
  if (C <= 0) { c0 = 0; C = g.C; }
  if (!p->d_dw) return set_error(p->ctx, SRMAP_EINVAL, "internal: a Huber loss without its weight buffer");
  const size_t nl = (size_t)g.w * g.h, run = (size_t)C * nl, e = p->elem();
  for (int k = 0; k < g.K; ++k) {  // [K][C][h][w]: one run per frame
    const size_t off = ((size_t)k * g.C + c0) * nl;
    if (p->d_prior)
      SRMAP_HIP(p->ctx, hipMemcpyAsync(p->d_dw.as<char>() + off * e, p->d_prior.as<const char>() + off * e, run * e, hipMemcpyDeviceToDevice, st));
    else if (p->dtype == SRMAP_F32) launch_fill<float>(p->d_dw.as<float>() + off, 1.f, run, st);
    else launch_fill<double>(p->d_dw.as<double>() + off, 1.0, run, st);
  }
  return SRMAP_OK;
}

int recover_reduction_timeout(srmap_problem* p, double* host_word) {
  // a late workgroup may still publish into the granules: re-initialise them only behind everything in flight
  SRMAP_HIP(p->ctx, hipDeviceSynchronize());
  ztile_rearm(p);
  if (p->d_cost.as<double>()) SRMAP_HIP(p->ctx, hipMemset(p->d_cost.as<double>() + 6, 0, sizeof(double)));
  if (host_word) *host_word = 0.0;
  return SRMAP_OK;
}

// srmap_problem_set_affine_motion (below) and the motion refinement: validate K 2x3 matrices and fill the per-frame
// records (inverse in double, formed once here).
int affine_records(srmap_ctx* ctx, int K, const double* a23, std::vector<double>* recs) {
  for (int i = 0; i < 6 * K; ++i)
    if (!std::isfinite(a23[i]))
      return set_error(ctx, SRMAP_EINVAL, "affine motion: entry %d of frame %d is not finite", i % 6, i / 6);
  recs->assign((size_t)K * kAffineRec, 0.0);
  for (int k = 0; k < K; ++k) {
    AffineMap F;
    std::copy(a23 + 6 * k, a23 + 6 * (k + 1), F.m);
    const double a = F.m[0], b = F.m[1], tx = F.m[2], c = F.m[3], d = F.m[4], ty = F.m[5];
    const double dev = deviation(F);
    if (!(dev <= kAffineMaxDeviation))
      return set_error(ctx, SRMAP_EUNSUPPORTED,
                       "affine motion of frame %d: max(|a-1|+|b|, |c|+|d-1|) = %g exceeds %g (the transpose gathers 3 x 3 candidates)",
                       k, dev, kAffineMaxDeviation);
    if (!(std::fabs(tx) < 1.0e9) || !(std::fabs(ty) < 1.0e9))
      return set_error(ctx, SRMAP_EUNSUPPORTED, "affine motion of frame %d: translation (%g, %g) too large", k, tx, ty);
    double* m = recs->data() + (size_t)k * kAffineRec;
    const AffineMap G = inverse(F);
    std::copy(G.m, G.m + 6, m);
    std::copy(F.m, F.m + 6, m + 6);
    // candidate radii, widened so that rounding of F(p) can drop no candidate (2 * (1.25 + 1e-9) < 3: still three integers)
    m[12] = std::fabs(a) + std::fabs(b) + 1.0e-9;
    m[13] = std::fabs(c) + std::fabs(d) + 1.0e-9;
  }
  return SRMAP_OK;
}

int stage_host_x(srmap_problem* p, const double* x_host) {
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const size_t n = p->hr_count();
  if (int rc = ensure(p, &p->d_x, n * p->elem())) return rc;
  return convert_upload(p, x_host, p->d_x.as(), n, p->ctx->stream);
}

}  // namespace srmap

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char* srmap_version(void) { return "srmap 0.1 (HIP, gfx950)"; }

long long srmap_live_allocations(void) { return g_live_allocations.load(); }

int srmap_ctx_create(int device_id, srmap_ctx** out) {
  if (!out) return SRMAP_EINVAL;
  *out = nullptr;
  srmap_ctx* ctx = new (std::nothrow) srmap_ctx();
  if (!ctx) return SRMAP_ENOMEM;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
    fprintf(stderr, "srmap: no usable HIP device %d (%s); this library has no CPU path\n",
            device_id, e != hipSuccess ? hipGetErrorString(e) : "device index out of range");
    delete ctx;
    return SRMAP_EHIP;
  }
  ctx->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return SRMAP_EHIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
  *out = ctx;
  return SRMAP_OK;
}

void srmap_ctx_destroy(srmap_ctx* ctx) {
  if (!ctx) return;
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  for (int i = 0; i < 2; ++i)
    if (ctx->h_event[i]) (void)hipEventDestroy(ctx->h_event[i]);
  blas_release(ctx);
  delete ctx;  // and its pinned staging
}

const char* srmap_last_error(const srmap_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

int srmap_problem_create(srmap_ctx* ctx, const srmap_problem_desc* d, srmap_problem** out) {
  if (!ctx || !d || !out) return SRMAP_EINVAL;
  *out = nullptr;
  if (d->hr_width <= 0 || d->hr_height <= 0 || d->channels <= 0)
    return set_error(ctx, SRMAP_EINVAL, "image size and channel count must be positive");
  if (d->scale < 1) return set_error(ctx, SRMAP_EINVAL, "downsampling scale must be >= 1");  // image_model.cpp:66
  if (d->frames < 1) return set_error(ctx, SRMAP_EINVAL, "at least one frame is required");
  if (d->dtype != SRMAP_F64 && d->dtype != SRMAP_F32) return set_error(ctx, SRMAP_EINVAL, "bad dtype");
  if (d->hr_width > 32000 || d->hr_height > 32000)
    return set_error(ctx, SRMAP_EUNSUPPORTED, "image larger than warpAffine's 16-bit coordinates");
  const bool blur = d->blur_ksize > 0 && d->blur_sigma > 0.0;  // image_model.cpp:42
  if (blur && (d->blur_ksize % 2 != 1))
    return set_error(ctx, SRMAP_EINVAL, "blur radius must be an odd number");  // blur_module.cpp:18
  if (blur && d->blur_ksize * d->blur_ksize > kMaxBlurTaps)
    return set_error(ctx, SRMAP_EUNSUPPORTED, "blur kernel larger than %d taps", kMaxBlurTaps);
  if ((size_t)d->channels * d->hr_width * d->hr_height > (size_t)2147483647)
    return set_error(ctx, SRMAP_EINVAL, "number of data points exceeds INT_MAX");  // map_solver.cpp:96-101
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));

  srmap_problem* p = new (std::nothrow) srmap_problem();
  if (!p) return SRMAP_ENOMEM;
  p->ctx = ctx;
  p->dtype = d->dtype;
  Geometry& g = p->geo;
  g.W = d->hr_width; g.H = d->hr_height; g.C = d->channels; g.K = d->frames; g.s = d->scale;
  const double scale_factor = 1.0 / (double)g.s;  // downsampling_module.cpp:24
  g.w = (int)(g.W * scale_factor);
  g.h = (int)(g.H * scale_factor);
  if (g.w <= 0 || g.h <= 0) { delete p; return set_error(ctx, SRMAP_EINVAL, "image smaller than the scale"); }
  g.b = blur ? d->blur_ksize : 1;
  g.hb = (g.b - 1) / 2;
  g.cr0 = 0; g.cr1 = g.H;
  g.rr0 = 0; g.rr1 = g.H;
  g.zlo = 0; g.zhi = 0;
  // Gaussian kernel: cv::getGaussianKernel (sigma > 0) and k * k^T, blur_module.cpp:20-22
  p->blur2d.assign((size_t)g.b * g.b, 1.0);
  p->blur1d.assign((size_t)g.b, 1.0);
  if (blur) {
    std::vector<double> k1(g.b);
    const double scale2x = -0.5 / (d->blur_sigma * d->blur_sigma);
    double sum = 0;
    for (int i = 0; i < g.b; ++i) {
      const double xx = i - (g.b - 1) * 0.5;
      k1[i] = std::exp(scale2x * xx * xx);
      sum += k1[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < g.b; ++i) k1[i] *= sum;
    p->blur1d = k1;
    for (int a = 0; a < g.b; ++a)
      for (int e = 0; e < g.b; ++e) p->blur2d[(size_t)a * g.b + e] = k1[a] * k1[e];
  }
  p->blur2d_t.resize(p->blur2d.size());
  for (int a = 0; a < g.b; ++a)
    for (int e = 0; e < g.b; ++e) p->blur2d_t[(size_t)a * g.b + e] = p->blur2d[(size_t)e * g.b + a];

  p->created_b = g.b;
  p->created_blur2d = p->blur2d;
  p->created_blur2d_t = p->blur2d_t;
  p->created_blur1d = p->blur1d;

  int rc = SRMAP_OK;
  p->has_motion = d->shifts_xy != nullptr;
  if (p->has_motion) {
    p->shifts.assign(d->shifts_xy, d->shifts_xy + 2 * (size_t)g.K);
    p->fwd_warps.resize(g.K);
    p->bwd_warps.resize(g.K);
    auto upload_ytab = [&](const std::vector<int>& t, WarpTaps<double>* wt) -> int {
      if (t.empty()) return SRMAP_OK;
      DevBuf d;
      if (d.alloc(sizeof(int) * t.size()) != hipSuccess ||
          hipMemcpy(d.as(), t.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice) != hipSuccess)
        return set_error(ctx, SRMAP_ENOMEM, "hipMalloc failed");
      wt->ytab = d.as<const int>();
      p->d_ytabs.push_back(std::move(d));
      return SRMAP_OK;
    };
    std::vector<int> ytab;
    for (int k = 0; k < g.K && rc == SRMAP_OK; ++k) {
      rc = make_warp(ctx, g.W, g.H, p->shifts[2 * k], p->shifts[2 * k + 1], &p->fwd_warps[k], &ytab);
      if (rc == SRMAP_OK) rc = upload_ytab(ytab, &p->fwd_warps[k]);
      // the transpose warps an image of size (w*s, h*s)
      if (rc == SRMAP_OK)
        rc = make_warp(ctx, g.w * g.s, g.h * g.s, -p->shifts[2 * k], -p->shifts[2 * k + 1], &p->bwd_warps[k], &ytab);
      if (rc == SRMAP_OK) rc = upload_ytab(ytab, &p->bwd_warps[k]);
    }
  }
  std::vector<int> cmap, rmap;
  nearest_map(g.W, g.w, &cmap);
  nearest_map(g.H, g.h, &rmap);
  p->maps_regular = (g.W == g.w * g.s) && (g.H == g.h * g.s);
  for (int j = 0; j < g.w && p->maps_regular; ++j) p->maps_regular = cmap[j] == j * g.s;
  for (int i = 0; i < g.h && p->maps_regular; ++i) p->maps_regular = rmap[i] == i * g.s;
  if (p->maps_regular) {
    // NN upsampling used by the HR-resolution residual must replicate each LR
    // pixel exactly s*s times (objective_data_term.cpp:29, map_solver.cpp:80-85).
    std::vector<int> up;
    nearest_map(g.w, g.W, &up);
    for (int x = 0; x < g.W && p->maps_regular; ++x) p->maps_regular = up[x] == x / g.s;
    nearest_map(g.h, g.H, &up);
    for (int y = 0; y < g.H && p->maps_regular; ++y) p->maps_regular = up[y] == y / g.s;
  }
  auto fail = [&](int code) { srmap_problem_destroy(p); return code; };
  if (rc) return fail(rc);
  if (p->dtype == SRMAP_F32) {
    if (p->has_motion) { rc = upload_warps<float>(p, p->fwd_warps, &p->d_fwd_warps); if (rc) return fail(rc);
                         rc = upload_warps<float>(p, p->bwd_warps, &p->d_bwd_warps); if (rc) return fail(rc); }
    rc = upload_array<float>(p, p->blur2d, &p->d_blur); if (rc) return fail(rc);
    rc = upload_array<float>(p, p->blur2d_t, &p->d_blur_t); if (rc) return fail(rc);
  } else {
    if (p->has_motion) { rc = upload_warps<double>(p, p->fwd_warps, &p->d_fwd_warps); if (rc) return fail(rc);
                         rc = upload_warps<double>(p, p->bwd_warps, &p->d_bwd_warps); if (rc) return fail(rc); }
    rc = upload_array<double>(p, p->blur2d, &p->d_blur); if (rc) return fail(rc);
    rc = upload_array<double>(p, p->blur2d_t, &p->d_blur_t); if (rc) return fail(rc);
  }
  if (p->d_col_map.alloc(sizeof(int) * g.w) != hipSuccess || p->d_row_map.alloc(sizeof(int) * g.h) != hipSuccess ||
      p->d_cost.alloc(sizeof(double) * 8) != hipSuccess)
    return fail(set_error(ctx, SRMAP_ENOMEM, "hipMalloc failed"));
  (void)hipMemcpy(p->d_col_map.as<int>(), cmap.data(), sizeof(int) * g.w, hipMemcpyHostToDevice);
  (void)hipMemcpy(p->d_row_map.as<int>(), rmap.data(), sizeof(int) * g.h, hipMemcpyHostToDevice);
  // everything above used blocking copies; d_cost is first touched by kernels on caller streams: clear it on the
  // context's (non-blocking) stream and wait, so no legacy-stream work is left behind the creation
  if (hipMemsetAsync(p->d_cost.as<double>(), 0, sizeof(double) * 8, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
    return fail(set_error(ctx, SRMAP_EHIP, "clearing the cost scalars failed"));
  model_replan(p);
  *out = p;
  return SRMAP_OK;
}

void srmap_problem_destroy(srmap_problem* p) {
  if (!p) return;
  ztile_release(p);
  if (p->state_ev) (void)hipEventDestroy(p->state_ev);
  delete p;  // and every device buffer it owns
}

int srmap_problem_set_impl(srmap_problem* p, int impl) {
  if (!p) return SRMAP_EINVAL;
  if (impl < SRMAP_IMPL_AUTO || impl > SRMAP_IMPL_TILED) return set_error(p->ctx, SRMAP_EINVAL, "bad impl");
  p->impl = impl;
  p->plan_gen++;
  return SRMAP_OK;
}

// ---- affine per-frame motion model (no reference counterpart; generalises motion_module.cpp:18-51) ----
int srmap_problem_set_affine_motion(srmap_problem* p, const double* affine_2x3) {
  if (!p) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  std::vector<double> recs;
  if (affine_2x3) {
    int rc = affine_records(p->ctx, p->geo.K, affine_2x3, &recs);
    if (rc) return rc;  // the problem keeps the motion it had
  }
  // evaluations in flight read the records: drain them before the buffer changes
  if (int rc = model_drain(p)) return rc;
  if (affine_2x3) {
    if (int rc = ensure(p, &p->d_affine, recs.size() * sizeof(double))) return rc;
    SRMAP_HIP(p->ctx, hipMemcpy(p->d_affine.as<double>(), recs.data(), recs.size() * sizeof(double), hipMemcpyHostToDevice));
    p->affine_recs.swap(recs);
    p->affine = true;
  } else {
    p->affine = false;
    p->affine_recs.clear();
    p->d_affine.reset();
  }
  // alternatives: an affine motion replaces a displacement field, and NULL restores the created motion
  p->d_flow.reset();
  p->d_flow_seed.reset();
  p->flow = false;
  model_replan(p);  // "not covered" while an affine motion is set
  return SRMAP_OK;
}

// ---- free-form blur kernel (no reference counterpart; BlurModule builds a Gaussian only, blur_module.cpp:13-22) ----
int srmap_problem_set_blur_kernel(srmap_problem* p, int ksize, const double* taps) {
  if (!p) return SRMAP_EINVAL;
  if (taps) {
    if (ksize < 1 || ksize % 2 != 1) return set_error(p->ctx, SRMAP_EINVAL, "blur kernel size must be odd and >= 1 (got %d)", ksize);
    if (ksize > kMaxCustomBlur)
      return set_error(p->ctx, SRMAP_EUNSUPPORTED, "blur kernel size %d: a free-form kernel has at most %d x %d taps", ksize, kMaxCustomBlur, kMaxCustomBlur);
    for (int i = 0; i < ksize * ksize; ++i)
      if (!std::isfinite(taps[i])) return set_error(p->ctx, SRMAP_EINVAL, "blur kernel: tap %d is not finite", i);
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const int b = taps ? ksize : p->created_b;
  std::vector<double> k2, k2t;
  if (taps) {
    k2.assign(taps, taps + (size_t)b * b);
    k2t.resize(k2.size());
    // the adjoint of a correlation is the correlation with the kernel flipped in BOTH axes (kernel.t(), the reference's
    // form, is that only for a kernel symmetric under both)
    for (int a = 0; a < b; ++a)
      for (int e = 0; e < b; ++e) k2t[(size_t)a * b + e] = k2[(size_t)(b - 1 - a) * b + (b - 1 - e)];
  } else {
    k2 = p->created_blur2d;
    k2t = p->created_blur2d_t;
  }
  // the new tables first: a failed allocation leaves the problem as it was
  DevBuf nb, nbt;
  int rc = p->dtype == SRMAP_F32 ? upload_array<float>(p, k2, &nb) : upload_array<double>(p, k2, &nb);
  if (rc == SRMAP_OK) rc = p->dtype == SRMAP_F32 ? upload_array<float>(p, k2t, &nbt) : upload_array<double>(p, k2t, &nbt);
  if (rc) return rc;
  // evaluations in flight read the old tables: drain them before the buffers change
  rc = model_drain(p);
  if (rc) return rc;
  p->d_blur = std::move(nb);  // the new tables move in; the old ones are freed
  p->d_blur_t = std::move(nbt);
  p->blur2d.swap(k2);
  p->blur2d_t.swap(k2t);
  p->blur1d = taps ? std::vector<double>((size_t)b, 0.0) : p->created_blur1d;  // a free-form kernel has no separable factor
  p->geo.b = b;
  p->geo.hb = (b - 1) / 2;
  p->custom_blur = taps != nullptr;
  model_replan(p);  // "not covered" while a free-form kernel is set
  return SRMAP_OK;
}

int srmap_problem_get_blur_kernel(const srmap_problem* p, int* ksize, double* taps_out) {
  if (!p) return SRMAP_EINVAL;
  if (ksize) *ksize = p->geo.b;
  if (taps_out) std::copy(p->blur2d.begin(), p->blur2d.end(), taps_out);
  return SRMAP_OK;
}

int srmap_problem_set_solver(srmap_problem* p, int least_squares_solver, int num_lbfgs_hessian_corrections) {
  if (!p) return SRMAP_EINVAL;
  if (least_squares_solver != SRMAP_SOLVER_CG && least_squares_solver != SRMAP_SOLVER_LBFGS)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown least-squares solver %d", least_squares_solver);
  if (num_lbfgs_hessian_corrections < 1)
    return set_error(p->ctx, SRMAP_EINVAL, "num_lbfgs_hessian_corrections must be >= 1 (got %d)", num_lbfgs_hessian_corrections);
  if (num_lbfgs_hessian_corrections > kLbfgsMaxM)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "num_lbfgs_hessian_corrections %d: at most %d are supported",
                     num_lbfgs_hessian_corrections, kLbfgsMaxM);
  p->solver = least_squares_solver;
  p->lbfgs_m = num_lbfgs_hessian_corrections;
  return SRMAP_OK;
}

int srmap_problem_active_impl(const srmap_problem* p, int* impl) {
  if (!p || !impl) return SRMAP_EINVAL;
  const bool ztile = p->impl != SRMAP_IMPL_DIRECT && p->zplan != nullptr;
  *impl = ztile ? SRMAP_IMPL_TILED : SRMAP_IMPL_DIRECT;
  return SRMAP_OK;
}

int srmap_problem_set_cost_rows(srmap_problem* p, int hr_row0, int hr_row1) {
  if (!p) return SRMAP_EINVAL;
  const Geometry& g = p->geo;
  if (hr_row0 < 0 || hr_row1 > g.H || hr_row0 >= hr_row1)
    return set_error(p->ctx, SRMAP_EINVAL, "cost rows [%d, %d) outside the image", hr_row0, hr_row1);
  if (hr_row0 % g.s != 0 || (hr_row1 % g.s != 0 && hr_row1 != g.H))
    return set_error(p->ctx, SRMAP_EINVAL, "cost rows must be multiples of the scale %d", g.s);
  p->geo.cr0 = hr_row0;
  p->geo.cr1 = hr_row1;
  return SRMAP_OK;
}

int srmap_problem_lr_size(const srmap_problem* p, int* lw, int* lh) {
  if (!p) return SRMAP_EINVAL;
  if (lw) *lw = p->geo.w;
  if (lh) *lh = p->geo.h;
  return SRMAP_OK;
}

static int need_solver_geometry(srmap_problem* p) {
  if (!p->maps_regular)
    return set_error(p->ctx, SRMAP_EINVAL,
                     "HR size %dx%d is not LR size * scale (%d); MapSolver requires it (map_solver.cpp:72-76)",
                     p->geo.W, p->geo.H, p->geo.s);
  return SRMAP_OK;
}

int srmap_set_observations(srmap_problem* p, const double* lr_host) {
  if (!p || !lr_host) return SRMAP_EINVAL;
  int rc = need_solver_geometry(p);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  rc = state_begin_write(p, p->ctx->stream);
  if (rc) return rc;
  DevBuf* raw = p->photometric ? &p->d_obs_raw : &p->d_obs;  // photometric parameters persist: the new frames are normalised
  rc = ensure(p, raw, p->lr_count() * p->elem());
  if (rc) return rc;
  rc = convert_upload(p, lr_host, raw->as(), p->lr_count(), p->ctx->stream);
  if (rc) return rc;
  if (p->photometric) {
    rc = photometric_normalise(p, p->ctx->stream);
    if (rc) return rc;
    SRMAP_HIP(p->ctx, hipStreamSynchronize(p->ctx->stream));
  }
  p->have_obs = true;
  return SRMAP_OK;
}

int srmap_set_observations_device(srmap_problem* p, const void* lr_dev, void* hip_stream) {
  if (!p || !lr_dev) return SRMAP_EINVAL;
  int rc = need_solver_geometry(p);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->ctx->stream;
  rc = state_begin_write(p, st);
  if (rc) return rc;
  DevBuf* raw = p->photometric ? &p->d_obs_raw : &p->d_obs;
  rc = ensure(p, raw, p->lr_count() * p->elem());
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipMemcpyAsync(raw->as(), lr_dev, p->lr_count() * p->elem(), hipMemcpyDeviceToDevice, st));
  if (p->photometric) {
    rc = photometric_normalise(p, st);
    if (rc) return rc;
  }
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));  // complete on return: lr_dev may be reused, any stream may evaluate
  p->have_obs = true;
  return SRMAP_OK;
}

int srmap_add_regularizer(srmap_problem* p, int kind, double lambda, int btv_range, double btv_decay,
                          int* reg_index) {
  if (!p) return SRMAP_EINVAL;
  if (kind != SRMAP_REG_TV && kind != SRMAP_REG_TV3D && kind != SRMAP_REG_BTV)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown regularizer kind %d", kind);
  if (p->nreg >= kMaxRegularizers) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "too many regularizers");
  RegSpec& rs = p->reg[p->nreg];
  rs = RegSpec{};
  rs.kind = kind;
  rs.lambda = lambda;
  if (kind == SRMAP_REG_BTV) {
    if (btv_range < 1) return set_error(p->ctx, SRMAP_EINVAL, "BTV range must be at least 1");  // btv_regularizer.cpp:58
    if (!(0 < btv_decay && btv_decay <= 1)) return set_error(p->ctx, SRMAP_EINVAL, "BTV decay must be in (0, 1]");
    if (btv_range > kMaxBtvRange) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "BTV range > %d", kMaxBtvRange);
    rs.range = btv_range;
    rs.decay = btv_decay;
    for (int i = 0; i < 2 * kMaxBtvRange + 1; ++i) rs.pow_table[i] = std::pow(btv_decay, i);
  }
  if (reg_index) *reg_index = p->nreg;
  p->nreg++;
  model_replan(p);
  return SRMAP_OK;
}

int srmap_clear_regularizers(srmap_problem* p) {
  if (!p) return SRMAP_EINVAL;
  for (int r = 0; r < p->nreg; ++r) p->reg[r].weights.reset();
  p->nreg = 0;
  model_replan(p);
  return SRMAP_OK;
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
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->ctx->stream;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  rc = ensure(p, &rs.weights, p->hr_count() * p->elem());
  if (rc) return rc;
  if (p->dtype == SRMAP_F32) rc = launch_reg_weights<float>(p, p->geo, rs, (const float*)x_dev, rs.weights.as<float>(), st);
  else rc = launch_reg_weights<double>(p, p->geo, rs, (const double*)x_dev, rs.weights.as<double>(), st);
  if (rc) return rc;
  return state_end_write(p, st);  // asynchronous: evaluations on other streams wait for this event
}

// ---- robust data term: per-observation weights, Huber loss (no reference counterpart) ----
// d_dw <- d_prior .* d_dw_user (ones where the caller gave none) on st, waited for: a problem with a prior only
static int rebuild_effective_weights(srmap_problem* p, hipStream_t st) {
  const size_t n = p->lr_count();
  int rc = p->dtype == SRMAP_F32
               ? launch_weight_product<float>(p, p->d_prior.as<const float>(), p->d_dw_user.as<const float>(), p->d_dw.as<float>(), n, st)
               : launch_weight_product<double>(p, p->d_prior.as<const double>(), p->d_dw_user.as<const double>(), p->d_dw.as<double>(), n, st);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

int srmap_set_data_weights(srmap_problem* p, const double* w_host) {
  if (!p) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const size_t n = p->lr_count();
  if (w_host)
    for (size_t i = 0; i < n; ++i)
      if (!(w_host[i] >= 0.0) || !std::isfinite(w_host[i]))
        return set_error(p->ctx, SRMAP_EINVAL, "data weight %zu is %g: weights must be finite and >= 0", i, w_host[i]);
  hipStream_t st = p->ctx->stream;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  const bool was = p->robust();
  if (p->d_prior) {  // the caller's weights go to the second buffer; d_dw is the product with the prior
    if (!w_host) {
      if (p->d_dw_user) { SRMAP_HIP(p->ctx, hipStreamSynchronize(st)); p->d_dw_user.reset(); }
    } else {
      rc = ensure(p, &p->d_dw_user, n * p->elem());
      if (rc == SRMAP_OK) rc = convert_upload(p, w_host, p->d_dw_user.as(), n, st);
    }
    return rc ? rc : rebuild_effective_weights(p, st);
  }
  if (!w_host) {
    // all ones: the unweighted kernels again -- except under a Huber loss, which keeps (and owns) the buffer
    if (p->d_dw) { SRMAP_HIP(p->ctx, hipStreamSynchronize(st)); p->d_dw.reset(); }
    if (p->data_loss == SRMAP_DATA_LOSS_HUBER) rc = ensure_data_weights(p, st);
  } else {
    rc = ensure(p, &p->d_dw, n * p->elem());
    if (rc == SRMAP_OK) rc = convert_upload(p, w_host, p->d_dw.as(), n, st);
  }
  replan_if(p, was);
  return rc;
}

int srmap_set_data_weights_device(srmap_problem* p, const void* w_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  if (!w_dev) return srmap_set_data_weights(p, nullptr);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->ctx->stream;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  const bool was = p->robust();
  DevBuf* dst = p->d_prior ? &p->d_dw_user : &p->d_dw;
  rc = ensure(p, dst, p->lr_count() * p->elem());
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipMemcpyAsync(dst->as(), w_dev, p->lr_count() * p->elem(), hipMemcpyDeviceToDevice, st));
  if (p->d_prior) return rebuild_effective_weights(p, st);
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));  // complete on return, as srmap_set_observations_device
  replan_if(p, was);
  return SRMAP_OK;
}

// ---- persistent prior on the data weights (no reference counterpart) ----
// The first prior of a problem: the weights in force become the caller's factor w (d_dw_user), d_dw the product's buffer.
static int data_prior_begin(srmap_problem* p, hipStream_t st) {
  const size_t bytes = p->lr_count() * p->elem();
  if (p->d_prior) return SRMAP_OK;
  DevBuf m, eff;
  if (m.alloc(bytes) != hipSuccess || eff.alloc(bytes) != hipSuccess)
    return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (data prior: 2 x %zu bytes)", bytes);
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  p->d_prior = std::move(m);
  p->d_dw_user = std::move(p->d_dw);  // d_dw -> d_dw_user (empty: ones); data_prior_remove moves it back
  p->d_dw = std::move(eff);
  return SRMAP_OK;
}

// after d_prior was written on st: the product, the plan of a problem that has become robust(); complete on return
static int data_prior_end(srmap_problem* p, bool was_robust, hipStream_t st) {
  int rc = rebuild_effective_weights(p, st);
  replan_if(p, was_robust);
  return rc;
}

static int data_prior_remove(srmap_problem* p, hipStream_t st) {
  if (!p->d_prior) return SRMAP_OK;
  const bool was = p->robust();
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  p->d_prior.reset();
  p->d_dw = std::move(p->d_dw_user);  // the product is freed; the caller's weights as given, or empty: the unweighted kernels again
  int rc = SRMAP_OK;
  if (p->data_loss == SRMAP_DATA_LOSS_HUBER) rc = ensure_data_weights(p, st);
  replan_if(p, was);
  return rc;
}

int srmap_set_data_prior(srmap_problem* p, const double* m_host) {
  if (!p) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const size_t n = p->lr_count();
  if (m_host)
    for (size_t i = 0; i < n; ++i)
      if (!(m_host[i] >= 0.0) || !std::isfinite(m_host[i]))
        return set_error(p->ctx, SRMAP_EINVAL, "data prior %zu is %g: the prior must be finite and >= 0", i, m_host[i]);
  hipStream_t st = p->ctx->stream;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  if (!m_host) return data_prior_remove(p, st);
  const bool was = p->robust();
  rc = data_prior_begin(p, st);
  if (rc) return rc;
  rc = convert_upload(p, m_host, p->d_prior.as(), n, st);
  if (rc) return rc;
  return data_prior_end(p, was, st);
}

int srmap_set_data_prior_device(srmap_problem* p, const void* m_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  if (!m_dev) return srmap_set_data_prior(p, nullptr);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->ctx->stream;
  int rc = state_begin_write(p, st);
  if (rc) return rc;
  const bool was = p->robust();
  rc = data_prior_begin(p, st);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, hipMemcpyAsync(p->d_prior.as(), m_dev, p->lr_count() * p->elem(), hipMemcpyDeviceToDevice, st));
  return data_prior_end(p, was, st);
}

int srmap_get_data_prior(srmap_problem* p, double* m_host, int* is_set) {
  if (!p) return SRMAP_EINVAL;
  if (is_set) *is_set = p->d_prior ? 1 : 0;
  if (!m_host) return SRMAP_OK;
  const size_t n = p->lr_count();
  if (!p->d_prior) {
    for (size_t i = 0; i < n; ++i) m_host[i] = 1.0;
    return SRMAP_OK;
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_download(p, p->d_prior.as(), m_host, n, p->ctx->stream);
}

int srmap_get_data_weights(srmap_problem* p, double* w_host) {
  if (!p || !w_host) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const size_t n = p->lr_count();
  if (!p->d_dw) {
    for (size_t i = 0; i < n; ++i) w_host[i] = 1.0;
    return SRMAP_OK;
  }
  // the weights may have been written asynchronously on another stream (srmap_update_data_weights_device)
  if (p->state_stream && p->state_stream != p->ctx->stream) SRMAP_HIP(p->ctx, hipStreamSynchronize(p->state_stream));
  return convert_download(p, p->d_dw.as(), w_host, n, p->ctx->stream);
}

int srmap_problem_set_data_loss(srmap_problem* p, int loss, double huber_delta) {
  if (!p) return SRMAP_EINVAL;
  if (loss != SRMAP_DATA_LOSS_L2 && loss != SRMAP_DATA_LOSS_HUBER)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown data loss %d", loss);
  if (loss == SRMAP_DATA_LOSS_HUBER && !(huber_delta > 0.0 && std::isfinite(huber_delta)))
    return set_error(p->ctx, SRMAP_EINVAL, "huber_delta must be finite and > 0 (got %g)", huber_delta);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const bool was = p->robust();
  p->data_loss = loss;
  p->huber_delta = loss == SRMAP_DATA_LOSS_HUBER ? huber_delta : 0.0;
  int rc = SRMAP_OK;
  if (loss == SRMAP_DATA_LOSS_HUBER) {
    rc = state_begin_write(p, p->ctx->stream);
    if (rc == SRMAP_OK) rc = ensure_data_weights(p, p->ctx->stream);
  }
  replan_if(p, was);
  return rc;
}

int srmap_update_data_weights_device(srmap_problem* p, const void* x_dev, void* hip_stream) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return update_data_weights(p, 0, 0, x_dev, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

// ---- operators on host buffers ----
int srmap_apply(srmap_problem* p, int frame, const double* hr, double* lr) {
  if (!p || !hr || !lr) return SRMAP_EINVAL;
  if (frame < 0 || frame >= p->geo.K) return set_error(p->ctx, SRMAP_EINVAL, "frame index %d out of range", frame);  // motion_shift.cpp:48-50
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const Geometry& g = p->geo;
  const size_t nlr = (size_t)g.C * g.w * g.h;
  int rc = ensure(p, &p->d_x, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = ensure(p, &p->d_tmp, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = convert_upload(p, hr, p->d_x.as(), p->hr_count(), st);
  if (rc) return rc;
  if (p->dtype == SRMAP_F32)
    rc = launch_forward_direct<float>(p, p->geo, p->d_x.as<const float>(), nullptr, p->geo.C, 0, p->d_tmp.as<float>(), frame, 1, nullptr, nullptr, st);
  else
    rc = launch_forward_direct<double>(p, p->geo, p->d_x.as<const double>(), nullptr, p->geo.C, 0, p->d_tmp.as<double>(), frame, 1, nullptr, nullptr, st);
  if (rc) return rc;
  return convert_download(p, p->d_tmp.as(), lr, nlr, st);
}

int srmap_apply_transpose(srmap_problem* p, int frame, const double* lr, double* hr) {
  if (!p || !lr || !hr) return SRMAP_EINVAL;
  if (frame < 0 || frame >= p->geo.K) return set_error(p->ctx, SRMAP_EINVAL, "frame index %d out of range", frame);
  if (p->geo.W != p->geo.w * p->geo.s || p->geo.H != p->geo.h * p->geo.s)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "transpose needs HR size == LR size * scale");
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const Geometry& g = p->geo;
  const size_t nlr = (size_t)g.C * g.w * g.h;
  int rc = ensure(p, &p->d_g, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = ensure(p, &p->d_tmp, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = convert_upload(p, lr, p->d_tmp.as(), nlr, st);
  if (rc) return rc;
  if (p->dtype == SRMAP_F32)
    rc = launch_gather_direct<float>(p, p->geo, p->d_tmp.as<const float>(), p->d_g.as<float>(), frame, 1, 1.0, false, st);
  else
    rc = launch_gather_direct<double>(p, p->geo, p->d_tmp.as<const double>(), p->d_g.as<double>(), frame, 1, 1.0, false, st);
  if (rc) return rc;
  return convert_download(p, p->d_g.as(), hr, p->hr_count(), st);
}

int srmap_reg_values(srmap_problem* p, int reg, const double* x, double* values) {
  if (!p || !x || !values || reg < 0 || reg >= p->nreg) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  int rc = ensure(p, &p->d_x, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = ensure(p, &p->d_regvals, p->hr_count() * p->elem());
  if (rc) return rc;
  rc = convert_upload(p, x, p->d_x.as(), p->hr_count(), st);
  if (rc) return rc;
  if (p->dtype == SRMAP_F32)
    rc = launch_reg_values<float>(p, p->geo, p->reg[reg], p->d_x.as<const float>(), p->d_regvals.as<float>(), st);
  else
    rc = launch_reg_values<double>(p, p->geo, p->reg[reg], p->d_x.as<const double>(), p->d_regvals.as<double>(), st);
  if (rc) return rc;
  return convert_download(p, p->d_regvals.as(), values, p->hr_count(), st);
}

int srmap_reg_values_and_gradient(srmap_problem* p, int reg, const double* x, const double* gc,
                                  double* values, double* gradient) {
  if (!p || !x || !gc || !values || !gradient || reg < 0 || reg >= p->nreg) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const size_t n = p->hr_count();
  int rc = ensure(p, &p->d_x, n * p->elem()); if (rc) return rc;
  rc = ensure(p, &p->d_g, n * p->elem()); if (rc) return rc;
  rc = ensure(p, &p->d_tmp, n * p->elem()); if (rc) return rc;
  rc = ensure(p, &p->d_regvals, n * p->elem()); if (rc) return rc;
  rc = convert_upload(p, x, p->d_x.as(), n, st); if (rc) return rc;
  rc = convert_upload(p, gc, p->d_tmp.as(), n, st); if (rc) return rc;
  const RegSpec& rs = p->reg[reg];
  if (p->dtype == SRMAP_F32) {
    rc = launch_reg_values<float>(p, p->geo, rs, p->d_x.as<const float>(), p->d_regvals.as<float>(), st); if (rc) return rc;
    rc = launch_reg_gradient_direct<float>(p, p->geo, rs, p->d_x.as<const float>(), p->d_tmp.as<const float>(), 1.0,
                                           p->d_regvals.as<const float>(), p->d_g.as<float>(), false, nullptr, nullptr, st);
  } else {
    rc = launch_reg_values<double>(p, p->geo, rs, p->d_x.as<const double>(), p->d_regvals.as<double>(), st); if (rc) return rc;
    rc = launch_reg_gradient_direct<double>(p, p->geo, rs, p->d_x.as<const double>(), p->d_tmp.as<const double>(), 1.0,
                                            p->d_regvals.as<const double>(), p->d_g.as<double>(), false, nullptr, nullptr, st);
  }
  if (rc) return rc;
  rc = convert_download(p, p->d_regvals.as(), values, n, st); if (rc) return rc;
  return convert_download(p, p->d_g.as(), gradient, n, st);
}

// ---- objective ----
int srmap_eval_device(srmap_problem* p, unsigned terms, const void* x_dev, void* g_dev, double* cost,
                      void* hip_stream) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->ctx->stream;
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

int srmap_device_alloc(srmap_ctx* ctx, size_t bytes, void** dev) {
  if (!ctx || !dev) return SRMAP_EINVAL;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf b;  // handed to the caller, who returns it through srmap_device_free
  SRMAP_HIP(ctx, b.alloc(bytes));
  *dev = b.release();
  return SRMAP_OK;
}
int srmap_device_free(srmap_ctx* ctx, void* dev) {
  if (!ctx) return SRMAP_EINVAL;
  if (dev) SRMAP_HIP(ctx, hipFree(dev));
  return SRMAP_OK;
}
int srmap_upload(srmap_problem* p, const double* host, void* dev, size_t count) {
  if (!p || !host || !dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_upload(p, host, dev, count, p->ctx->stream);
}
int srmap_download(srmap_problem* p, const void* dev, double* host, size_t count) {
  if (!p || !host || !dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_download(p, dev, host, count, p->ctx->stream);
}
int srmap_synchronize(srmap_ctx* ctx) {
  if (!ctx) return SRMAP_EINVAL;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  SRMAP_HIP(ctx, hipDeviceSynchronize());
  return SRMAP_OK;
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

int srmap_solve_sharded(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard,
                        const srmap_irls_options* options, const double* x0, double* x_out,
                        srmap_solve_report* report) {
  if (!p || !x0 || !x_out) return SRMAP_EINVAL;
  srmap_irls_options o;
  if (options) {
    // the first member is the size of the struct the caller was compiled with: another layout is refused, not guessed at
    if (options->struct_size != (int)sizeof(srmap_irls_options))
      return set_error(p->ctx, SRMAP_EINVAL, "srmap_irls_options: struct_size %d, this library expects %d (fill the struct with "
                       "srmap_irls_options_default() of the matching include/srmap.h)", options->struct_size, (int)sizeof(srmap_irls_options));
    o = *options;
  } else {
    srmap_irls_options_default(&o);
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return solve_impl(p, comm, shard, &o, x0, x_out, report);
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
