// blur_fit.hip -- calibration fit of the blur kernel, one (srmap_fit_blur) or a bank of them
// (srmap_fit_blur_bank; one body, fit_device): with the HR image x KNOWN (a chart, a
// calibration pair) the ksize x ksize taps h of B in A_k = D B M_k are a linear least-squares problem,
//   E(h) = sum_k sum_c sum_u w (sum_t h_t s_t - y)^2,  s_t = (M_k x)(R0 + a - hb, C0 + e - hb), t = (a, e), 0 outside the image,
// (R0, C0) the decimation source of LR pixel u, M_k sampled exactly as the forward kernel of the problem's motion samples it
// (MotionSampler of sample_dev.hpp; the identity without motion), over
// every LR pixel of every channel and frame (the cost-row restriction is ignored, as in 3.8).  No reference counterpart
// (blur_module.cpp:13-22 builds a Gaussian from (radius, sigma)); the checker is tests/blur_kernel_restatement.py.
//   pass      ONE launch of k_blur_fit_sums: with n = ksize^2 the record is the upper triangle (row-major) of the
//             (n + 1) x (n + 1) Gram of the columns [s_0 ... s_{n-1}, y] under w: P = (n + 1)(n + 2) / 2 sums (3 / 55 / 351 /
//             1275).  grid (chunks, frames), 256 threads; the workgroup walks its chunk in tiles of 128 observations
//             (pixel, channel); phase 1 forms the tile's n + 1 columns once, in double after the loads, in LDS (row stride
//             129 doubles: odd, so the rows a wave reads in phase 2 spread over the banks and lanes that share a row
//             broadcast); phase 2 gives every thread its own <= 5 pairs (i <= j) and adds (w u_i) u_j over the tile in
//             index order in f64 registers.  No cross-thread reduction, no atomics, a fixed order: bit-identical run to run;
//             A bank entry is the same quadratic over the entry's observations alone: the PER_CHANNEL instances keep a
//             record per (frame, channel, chunk);
//   reduce    k_fit_reduce (motion_fit.hip) adds the records of every entry in index order -- all of them for the single kernel;
//   pacing    one launch, one reduce, one copy of entries x P doubles, one stream wait (FitPass, motion_fit.hip);
//   solve     on the host in double, per entry: (G + mu I) h = b + mu h_current, mu = ridge trace(G) / n, by Cholesky
//             (cholesky_factor_n, affine_map.hpp); sum_to_one: the KKT system of the constraint 1^T h = 1 by block
//             elimination over the same factor, h = u - lambda v, u = A^-1 rhs, v = A^-1 1, lambda = (1^T u - 1) / (1^T v).
#include <algorithm>
#include <cmath>
#include <vector>

#include "affine_map.hpp"
#include "motion_fit_dev.hpp"
#include "sample_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kTile = 128;       // observations per tile
constexpr int kStride = 129;     // LDS row stride in doubles (odd)
constexpr int kMaxChunks = 128;  // chunks per frame at most
constexpr int kMinTilesPerChunk = 2;

// PER_CHANNEL (compile time; the bank fit): grid (chunks, frames, channels), the workgroup's observations are the LR pixels
// of channel blockIdx.z alone, so that a record belongs to one (frame, channel): partial[((k * C + c) * chunks + chunk)][P].
// Otherwise the grid is (chunks, frames) and the chunk walks (channel, pixel) together: partial[(k * chunks + chunk)][P].
// (A run-time switch cost the existing instances 20 to 45 VGPRs and with them waves per SIMD: profiles/r17_blur_bank_resources.txt.)
template <typename T, int B, int MOTION, bool WEIGHTED, bool PER_CHANNEL = false>
__global__ __launch_bounds__(256) void k_blur_fit_sums(const T* __restrict__ x, const T* __restrict__ y,
                                                       const T* __restrict__ dw, Geometry g,
                                                       MotionArgs<T> ma, const int* __restrict__ col_map,
                                                       const int* __restrict__ row_map, int tiles_per_chunk,
                                                       double* __restrict__ partial) {
  constexpr int N = B * B, N1 = N + 1, P = N1 * (N1 + 1) / 2, PP = (P + 255) / 256, HB = (B - 1) / 2;
  __shared__ double u[N1 * kStride];  // column t of the tile: u[t * kStride + observation]; column N is y
  __shared__ double wl[kTile];
  const int k = blockIdx.y;
  const int n = g.w * g.h;
  const long long nobs = PER_CHANNEL ? (long long)n : (long long)n * g.C;
  // this thread's pairs (i <= j) of the upper triangle, row-major: q = threadIdx.x + 256 m
  int pi[PP], pj[PP];
  double acc[PP];
#pragma unroll
  for (int m = 0; m < PP; ++m) {
    const int q = (int)threadIdx.x + 256 * m;
    int i = 0, rem = q < P ? q : 0;
    while (rem >= N1 - i) { rem -= N1 - i; ++i; }
    pi[m] = i * kStride;
    pj[m] = (i + rem) * kStride;
    acc[m] = 0.0;
  }
  const MotionSampler<T, MOTION> ms(ma, g, k);  // uniform
  const int ob = threadIdx.x & (kTile - 1), half = threadIdx.x >> 7;
  for (int tile = 0; tile < tiles_per_chunk; ++tile) {
    const long long o0 = ((long long)blockIdx.x * tiles_per_chunk + tile) * kTile;
    if (o0 >= nobs && tile > 0) break;  // uniform
    const long long o = o0 + ob;
    const bool live = o < nobs;
    __syncthreads();  // the previous tile's phase 2 has read the columns
    // ---- phase 1: the tile's columns ----
    int c = 0, lp = 0, R0 = 0, C0 = 0;
    if (live) {
      if constexpr (PER_CHANNEL) {
        c = (int)blockIdx.z;
        lp = (int)o;
      } else {
        c = (int)(o / n);
        lp = (int)(o - (long long)c * n);
      }
      const int i = lp / g.w, j = lp - i * g.w;
      R0 = row_map[i];
      C0 = col_map[j];
    }
    const T* __restrict__ plane = x + (size_t)c * g.W * g.H;
    for (int t = half; t < N; t += 2) {
      const int a = t / B, e = t - a * B;
      const int rr = R0 + a - HB, cc = C0 + e - HB;
      double s = 0.0;
      if (live && rr >= 0 && rr < g.H && cc >= 0 && cc < g.W)  // the blur's zero border on the warped image
        s = ms.template at<double>(plane, g.W, g.H, rr, cc);
      u[t * kStride + ob] = s;
    }
    {
      const size_t oi = ((size_t)k * g.C + c) * n + lp;
      if (half == 0) u[N * kStride + ob] = live ? (double)y[oi] : 0.0;
      else wl[ob] = live ? (WEIGHTED ? (double)dw[oi] : 1.0) : 0.0;
    }
    __syncthreads();
    // ---- phase 2: this thread's pairs over the tile, in index order ----
    for (int q = 0; q < kTile; ++q) {
      const double wv = wl[q];
#pragma unroll
      for (int m = 0; m < PP; ++m) acc[m] += (wv * u[pi[m] + q]) * u[pj[m] + q];
    }
  }
  const size_t row = PER_CHANNEL ? (size_t)k * gridDim.z + blockIdx.z : (size_t)k;
  double* __restrict__ rec = partial + (row * gridDim.x + blockIdx.x) * P;
#pragma unroll
  for (int m = 0; m < PP; ++m) {
    const int q = (int)threadIdx.x + 256 * m;
    if (q < P) rec[q] = acc[m];
  }
}

// the instance of the problem's motion kind; false: the kind has none (a displacement field, which the entry point refuses).
// per_channel: the bank fit's grid, a record per (frame, channel, chunk)
template <typename T, int B, bool PER_CHANNEL>
bool launch_sums_m(srmap_problem* p, const T* x, int chunks, int tpc, double* d_part, hipStream_t st) {
  const Geometry& g = p->geo;
  dim3 grid(chunks, g.K, PER_CHANNEL ? g.C : 1);
  const MotionArgs<T> ma = p->motion.args<T>();
  const T* dw = p->dw.effective<T>();
  return dispatch_value<kMotionNone, kMotionTable, kMotionAffine>(p->motion.kind(), [&](auto motion) {
    constexpr int MOTION = decltype(motion)::value;
    dispatch_value<0, 1>(dw != nullptr, [&](auto weighted) {
      hipLaunchKernelGGL((k_blur_fit_sums<T, B, MOTION, decltype(weighted)::value != 0, PER_CHANNEL>), grid, dim3(256), 0, st, x,
                         p->d_obs.as<const T>(), dw, g, ma, p->d_col_map.as<int>(), p->d_row_map.as<int>(), tpc, d_part);
    });
  });
}

template <typename T, bool PER_CHANNEL>
bool launch_sums(srmap_problem* p, int ksize, const T* x, int chunks, int tpc, double* d_part, hipStream_t st) {
  if (ksize == 1) return launch_sums_m<T, 1, PER_CHANNEL>(p, x, chunks, tpc, d_part, st);
  if (ksize == 3) return launch_sums_m<T, 3, PER_CHANNEL>(p, x, chunks, tpc, d_part, st);
  if (ksize == 5) return launch_sums_m<T, 5, PER_CHANNEL>(p, x, chunks, tpc, d_part, st);
  return launch_sums_m<T, 7, PER_CHANNEL>(p, x, chunks, tpc, d_part, st);
}

// The kernel `cur` (b x b) zero-padded or centre-cropped to ksize
std::vector<double> resized_kernel(const double* cur, int b, int ksize) {
  std::vector<double> hcur((size_t)ksize * ksize, 0.0);
  const int off = (ksize - b) / 2;  // both odd: exact, negative when cropping
  for (int a = 0; a < ksize; ++a)
    for (int e = 0; e < ksize; ++e) {
      const int sa = a - off, se = e - off;
      if (sa >= 0 && sa < b && se >= 0 && se < b) hcur[(size_t)a * ksize + e] = cur[(size_t)sa * b + se];
    }
  return hcur;
}

// E(h) = [h; -1]^T M [h; -1], M the (n + 1) x (n + 1) Gram (full, row-major)
double energy(const std::vector<double>& M, int n, const double* h) {
  const int n1 = n + 1;
  double e = 0.0;
  for (int i = 0; i < n1; ++i) {
    const double vi = i < n ? h[i] : -1.0;
    double row = 0.0;
    for (int j = 0; j < n1; ++j) row += M[(size_t)i * n1 + j] * (j < n ? h[j] : -1.0);
    e += vi * row;
  }
  return e;
}

// The host solve of one Gram: sums = the packed upper triangle of the (n + 1) x (n + 1) Gram, hcur the kernel in force at the
// fit's size.  h (n taps; hcur for status 3) and quality[5] = {E(hcur), E(h), smallest / largest pivot, status}.
void solve_taps(const double* sums, int n, const std::vector<double>& hcur, const srmap_blur_fit_options& opt,
                std::vector<double>* h_out, double* quality) {
  const int n1 = n + 1;
  std::vector<double> M((size_t)n1 * n1);
  for (int i = 0, q = 0; i < n1; ++i)
    for (int j = i; j < n1; ++j, ++q) M[(size_t)i * n1 + j] = M[(size_t)j * n1 + i] = sums[q];
  const double e0 = energy(M, n, hcur.data());
  double trace = 0.0;
  for (int i = 0; i < n; ++i) trace += M[(size_t)i * n1 + i];
  const double mu = opt.ridge * trace / n;
  std::vector<double> A((size_t)n * n), Lc((size_t)n * n, 0.0), rhs((size_t)n), h((size_t)n), ones((size_t)n, 1.0), v((size_t)n);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = M[(size_t)i * n1 + j];
    A[(size_t)i * n + i] += mu;
    rhs[i] = M[(size_t)i * n1 + n] + mu * hcur[i];
  }
  double pmin = 0.0, pmax = 0.0, e1 = e0;
  int status = 0;
  if (!cholesky_factor_n(A.data(), n, Lc.data(), &pmin, &pmax)) {
    status = 3;  // no texture, or every weight 0: the kernel stays
    h = hcur;
  } else {
    cholesky_apply_n(Lc.data(), n, rhs.data(), h.data());
    if (opt.sum_to_one) {
      cholesky_apply_n(Lc.data(), n, ones.data(), v.data());
      double su = 0.0, sv = 0.0;
      for (int i = 0; i < n; ++i) { su += h[i]; sv += v[i]; }
      const double lambda = (su - 1.0) / sv;
      for (int i = 0; i < n; ++i) h[i] -= lambda * v[i];
      // one more step along v for the rounding the first left in the constraint (|sum h - 1| <= 1e-14 is promised)
      su = 0.0;
      for (int i = 0; i < n; ++i) su += h[i];
      const double rest = (su - 1.0) / sv;
      for (int i = 0; i < n; ++i) h[i] -= rest * v[i];
    }
    for (int i = 0; i < n; ++i)
      if (!std::isfinite(h[i])) status = 3;
    if (status == 3) h = hcur;
    else e1 = energy(M, n, h.data());
  }
  quality[0] = e0; quality[1] = e1; quality[2] = pmin; quality[3] = pmax; quality[4] = status;
  h_out->swap(h);
}

const char kOptionsName[] = "srmap_blur_fit_options";

// srmap_fit_blur refuses while a bank is set (the host form after its other checks, the device form first)
int refuse_bank(srmap_problem* p) {
  if (!p->blur.is_bank()) return SRMAP_OK;
  return set_error(p->ctx, SRMAP_EUNSUPPORTED, "a blur bank is set: the ridge and the energy at the kernel in force have no single kernel to refer to (srmap_fit_blur_bank fits a bank)");
}

// The one body of the two fits' device forms: a kernel per entry of `mode`, mode 0 the single kernel -- one entry over every
// observation, by the instances that walk (channel, pixel) together; a bank mode by the PER_CHANNEL instances.  The outputs
// hold one entry after the other.
int fit_device(srmap_problem* p, const void* x_dev, void* hip_stream, int mode, const srmap_blur_fit_options* options,
               double* taps_out, double* quality_out, double* normal_equations_out) {
  srmap_ctx* ctx = p->ctx;
  const Geometry& g = p->geo;
  const char* const what = mode ? "blur bank fit" : "blur fit";
  if (p->motion.is_field())
    return p->motion.refuse(ctx, SRMAP_EUNSUPPORTED, "the blur fit has no sampling leg for %s: not available while one is set (%s)");
  srmap_blur_fit_options opt;
  if (int rc = options_in_force(ctx, options, srmap_blur_fit_options_default, kOptionsName, &opt)) return rc;
  const int ksize = opt.ksize == 0 ? g.b : opt.ksize;
  if (ksize < 1 || ksize % 2 != 1) return set_error(ctx, SRMAP_EINVAL, "blur fit: ksize must be odd and >= 1 (got %d)", ksize);
  if (ksize > kMaxCustomBlur)
    return set_error(ctx, SRMAP_EUNSUPPORTED, "blur fit: ksize %d: at most %d x %d taps are fitted", ksize, kMaxCustomBlur, kMaxCustomBlur);
  if (!(opt.ridge >= 0.0) || !std::isfinite(opt.ridge)) return set_error(ctx, SRMAP_EINVAL, "blur fit: ridge must be finite and >= 0");
  if (!p->have_obs) return set_error(ctx, SRMAP_EINVAL, "no observations set");

  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream_of(ctx, hip_stream);
  if (int rc = problem_state_read(p, st)) return rc;

  // a chunk holds tpc tiles of the observations of a frame (mode 0) or of one of its channels; the records lie
  // [frame][chunk] or [frame][channel][chunk]
  const int n = ksize * ksize, n1 = n + 1, P = n1 * (n1 + 1) / 2;
  const long long nobs = (long long)g.w * g.h * (mode ? 1 : g.C);
  const long long tiles = (nobs + kTile - 1) / kTile;
  const int tpc = (int)std::max<long long>(kMinTilesPerChunk, (tiles + kMaxChunks - 1) / kMaxChunks);
  const int chunks = (int)((tiles + tpc - 1) / tpc);
  const int per_frame = mode ? g.C * chunks : chunks;
  const int entries = BlurModel::entries(mode, g.K, g.C);
  FitPass fit;  // a row per entry, no table
  if (!fit.alloc(entries, P, (size_t)g.K * per_frame * P, false)) return set_error(ctx, SRMAP_ENOMEM, "%s: allocation failed", what);
  if (!dispatch_dtype(p->dtype, [&](auto t) {
        using T = decltype(t);
        return mode ? launch_sums<T, true>(p, ksize, (const T*)x_dev, chunks, tpc, fit.d_part.as<double>(), st)
                    : launch_sums<T, false>(p, ksize, (const T*)x_dev, chunks, tpc, fit.d_part.as<double>(), st);
      }))
    return set_error(ctx, SRMAP_EINVAL, "internal: the blur fit has no kernel for motion kind %d", (int)p->motion.kind());
  SRMAP_HIP(ctx, hipGetLastError());
  // the records of an entry, in (frame, channel, chunk) order: all of them, a frame's, a channel's chunks of every frame, or
  // the chunks of one (frame, channel)
  const int row_stride = mode == SRMAP_BLUR_PER_FRAME ? per_frame : chunks;  // (mode 0 has the one row)
  const int outer = mode == SRMAP_BLUR_PER_CHANNEL ? g.K : 1;
  const int inner = mode == 0 ? g.K * per_frame : mode == SRMAP_BLUR_PER_FRAME ? per_frame : chunks;
  if (!fit.reduce_and_fetch(row_stride, outer, per_frame, inner, st)) return set_error(ctx, SRMAP_EHIP, "%s: pass failed", what);

  // ---- the host solve, entry by entry ----
  std::vector<double> taps((size_t)entries * n), quality((size_t)entries * 5);
  bool any = false;
  for (int q = 0; q < entries; ++q) {
    // the (frame, channel) that stands for entry q, and the kernel in force for it, zero-padded or centre-cropped to ksize
    const int k = mode == SRMAP_BLUR_PER_FRAME ? q : mode == SRMAP_BLUR_PER_FRAME_CHANNEL ? q / g.C : 0;
    const int c = mode == SRMAP_BLUR_PER_CHANNEL ? q : mode == SRMAP_BLUR_PER_FRAME_CHANNEL ? q % g.C : 0;
    std::vector<double> h;
    solve_taps(fit.sums(q), n, resized_kernel(p->blur.entry_taps(k, c), g.b, ksize), opt, &h, quality.data() + (size_t)q * 5);
    std::copy(h.begin(), h.end(), taps.begin() + (size_t)q * n);
    any = any || quality[(size_t)q * 5 + 4] == 0.0;
  }
  if (any && opt.apply) {
    const int rc = mode ? srmap_problem_set_blur_bank(p, mode, ksize, taps.data()) : srmap_problem_set_blur_kernel(p, ksize, taps.data());
    if (rc) return rc;
  }
  if (taps_out) std::copy(taps.begin(), taps.end(), taps_out);
  if (quality_out) std::copy(quality.begin(), quality.end(), quality_out);
  if (normal_equations_out) std::copy(fit.sums(0), fit.sums(0) + (size_t)entries * P, normal_equations_out);
  return SRMAP_OK;
}

}  // namespace

}  // namespace srmap

using namespace srmap;

extern "C" void srmap_blur_fit_options_default(srmap_blur_fit_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_blur_fit_options);
  o->ksize = 0;
  o->sum_to_one = 1;
  o->ridge = 0.0;
  o->apply = 1;
}

extern "C" int srmap_fit_blur_device(srmap_problem* p, const void* x_dev, void* hip_stream,
                                     const srmap_blur_fit_options* options, double* taps_out, double* quality_out,
                                     double* normal_equations_out) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  if (int rc = refuse_bank(p)) return rc;
  return fit_device(p, x_dev, hip_stream, 0, options, taps_out, quality_out, normal_equations_out);
}

extern "C" int srmap_fit_blur_bank_device(srmap_problem* p, const void* x_dev, void* hip_stream, int mode,
                                          const srmap_blur_fit_options* options, double* taps_out, double* quality_out,
                                          double* normal_equations_out) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  if (int rc = BlurModel::check_bank_mode(p->ctx, mode)) return rc;
  return fit_device(p, x_dev, hip_stream, mode, options, taps_out, quality_out, normal_equations_out);
}

extern "C" int srmap_fit_blur_bank(srmap_problem* p, const double* x_host, int mode, const srmap_blur_fit_options* options,
                                   double* taps_out, double* quality_out, double* normal_equations_out) {
  if (!p || !x_host) return SRMAP_EINVAL;
  if (int rc = BlurModel::check_bank_mode(p->ctx, mode)) return rc;
  if (int rc = host_fit_prologue(p, x_host, options, srmap_blur_fit_options_default, kOptionsName)) return rc;
  return fit_device(p, p->d_x.as(), p->ctx->stream, mode, options, taps_out, quality_out, normal_equations_out);
}

extern "C" int srmap_fit_blur(srmap_problem* p, const double* x_host, const srmap_blur_fit_options* options,
                              double* taps_out, double* quality_out, double* normal_equations_out) {
  if (!p || !x_host) return SRMAP_EINVAL;
  if (int rc = host_fit_prologue(p, x_host, options, srmap_blur_fit_options_default, kOptionsName, NoFitCheck(),
                                 [](srmap_problem* q, const srmap_blur_fit_options&) { return refuse_bank(q); }))
    return rc;
  return fit_device(p, p->d_x.as(), p->ctx->stream, 0, options, taps_out, quality_out, normal_equations_out);
}
