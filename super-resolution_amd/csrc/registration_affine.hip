// registration_affine.hip -- affine registration of a frame stack on the GPU (srmap_register_affine).
//
// For every frame k >= 1: F_k(p) = L_k p + t_k with I_k(F_k(p)) ~= I_0(p), the convention of the affine motion model
// (srmap_problem_set_affine_motion) and of MotionShift.  No reference counterpart (registration.cpp keeps the translation of a
// feature-based fit); the checker is tests/affine_registration_restatement.py.
//   1. box pyramid of the whole stack, built once (k_down2_stack, motion_fit.hip), halved while the shorter side is >= 64;
//   2. seed at the coarsest level: integer search over [-R, R]^2, mean squared difference over the FIXED template window
//      [R, w-R) x [R, h-R) (k_ssd_window).  The overlap window of the translational search moves with the candidate and
//      lets the zero wedges of a rotated frame vote for far-away shifts; a fixed window compares every candidate on the
//      same pixels;
//   3. inverse-compositional Gauss-Newton, coarse to fine: per pass ONE launch of k_affine_gn_sums for all frames
//      (26 sums per workgroup, fixed-order reduction), one k_fit_reduce, one 26 x (K-1) double copy and one stream wait
//      (FitPass, motion_fit.hip); the 6 x 6 Cholesky solve and the composition F <- F o W^-1 run on the host in double
//      (affine_map.hpp).
// Sample positions are the affine sampler's (sample_dev.hpp; affine_coord of motion_fit_dev.hpp: every operation rounded on its own).
#include <algorithm>
#include <cmath>
#include <vector>

#include "affine_map.hpp"
#include "motion_fit_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kGnSums = 26;       // 18 of H, 6 of g, sum e^2, pixel count
constexpr int kMaxRowChunks = 128;
constexpr int kMaxSeedChunks = 8;

// partial[((f * ncand + cand) * gridDim.y + chunk)] = sum of (I_{f+1}(p + u) - I_0(p))^2 over the rows of this chunk of
// the window [R, w-R) x [R, h-R), u = (cand % n1 - R, cand / n1 - R), n1 = 2R + 1.  grid = (ncand, chunks, frames - 1).
__global__ __launch_bounds__(256) void k_ssd_window(const double* __restrict__ stack, int w, int h, int R,
                                                    int rows_per_chunk, double* __restrict__ partial) {
  __shared__ double red[4];
  const int n1 = 2 * R + 1, cand = blockIdx.x, ux = cand % n1 - R, uy = cand / n1 - R;
  const double* a = stack;
  const double* b = stack + (size_t)(blockIdx.z + 1) * w * h;
  const int r0 = R + blockIdx.y * rows_per_chunk, r1 = min(h - R, r0 + rows_per_chunk);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) {
    for (int c = R + (int)threadIdx.x; c < w - R; c += 256) {
      const double d = b[(size_t)(r + uy) * w + c + ux] - a[(size_t)r * w + c];
      s += d * d;
    }
  }
  s = wave_sum(s);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[((size_t)blockIdx.z * gridDim.x + cand) * gridDim.y + blockIdx.y] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Gauss-Newton sums of one inverse-compositional pass for every frame: grid = (row chunks, frames - 1).
// table[f][kFitTabRec]: F of frame f + 1 at this level and its "active" flag.  Over the template pixels p of this chunk's
// rows (1 px from the border) whose four taps of I_{f+1} at s = F(p) are inside:
//   e = I(s) - I_0(p), (gx, gy) central differences of I_0, (u, v) = p - centre,
//   partial[(f * chunks + chunk)][26] = {gx^2, gx gy, gy^2} x {u^2, uv, u, v^2, v, 1} (index 6 a + m),
//                                       {gx e, gy e} x {u, v, 1} (18 + 3 a + m), e^2 (24), count (25).
__global__ __launch_bounds__(256) void k_affine_gn_sums(const double* __restrict__ stack, int w, int h, int rows_per_chunk,
                                                        const double* __restrict__ table, double* __restrict__ partial) {
  __shared__ double red[kGnSums][4];
  const int f = blockIdx.y;
  const double* m = table + (size_t)f * kFitTabRec;
  if (m[6] == 0.0) return;  // converged frame: uniform
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  const double* a = stack;
  const double* b = stack + (size_t)(f + 1) * w * h;
  const double cx = 0.5 * (double)(w - 1), cy = 0.5 * (double)(h - 1);
  const double xmax = (double)(w - 1), ymax = (double)(h - 1);
  const int r0 = 1 + blockIdx.x * rows_per_chunk, r1 = min(h - 1, r0 + rows_per_chunk);
  double acc[kGnSums];
#pragma unroll
  for (int q = 0; q < kGnSums; ++q) acc[q] = 0.0;
  for (int r = r0; r < r1; ++r) {
    const double v = (double)r - cy;
    for (int c = 1 + (int)threadIdx.x; c < w - 1; c += 256) {
      const double sx = affine_coord(m0, m1, m2, (double)c, (double)r);
      const double sy = affine_coord(m3, m4, m5, (double)c, (double)r);
      if (!(sx >= 0.0 && sx < xmax && sy >= 0.0 && sy < ymax)) continue;  // a tap outside (NaN included): left out
      const double x0 = __builtin_floor(sx), y0 = __builtin_floor(sy);
      const double fx = sx - x0, fy = sy - y0;
      const double* pb = b + (size_t)(int)y0 * w + (int)x0;  // x0 in [0, w-2], y0 in [0, h-2]
      const double val = (1.0 - fy) * ((1.0 - fx) * pb[0] + fx * pb[1]) + fy * ((1.0 - fx) * pb[w] + fx * pb[w + 1]);
      const double* pa = a + (size_t)r * w + c;
      const double e = val - pa[0];
      const double gx = 0.5 * (pa[1] - pa[-1]), gy = 0.5 * (pa[w] - pa[-w]);
      const double u = (double)c - cx;
      const double gg[3] = {gx * gx, gx * gy, gy * gy};
      const double mm[5] = {u * u, u * v, u, v * v, v};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[6 * i + j] += gg[i] * mm[j];
        acc[6 * i + 5] += gg[i];
      }
      const double ge[2] = {gx * e, gy * e};
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        acc[18 + 3 * i] += ge[i] * u;
        acc[19 + 3 * i] += ge[i] * v;
        acc[20 + 3 * i] += ge[i];
      }
      acc[24] += e * e;
      acc[25] += 1.0;
    }
  }
  fold_sums_256(acc, red, partial + ((size_t)f * gridDim.x + blockIdx.x) * kGnSums);
}

// H (6 x 6, from the 18 sums) D = g by Cholesky; false: no texture
bool solve_step(const double* S, double* delta) {
  // J_i = g_{i / 3} * m_{i % 3}, m = (u, v, 1); product index of (m_i, m_j) in {u^2, uv, u, v^2, v, 1}
  static const int mprod[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  double H[6][6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) H[i][j] = S[6 * (i / 3 + j / 3) + mprod[i % 3][j % 3]];
  return cholesky_solve(H, S + 18, 6, delta);
}

}  // namespace

}  // namespace srmap

using namespace srmap;

extern "C" void srmap_affine_registration_options_default(srmap_affine_registration_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_affine_registration_options);
  o->hr_scale = 1;
  o->max_iterations = 30;
  o->step_tolerance = 1e-4;
  o->max_levels = 0;
  o->initial_affine_2x3 = nullptr;
}

extern "C" int srmap_register_affine(srmap_ctx* ctx, int num_images, int width, int height, const double* images_host,
                                     const srmap_affine_registration_options* options, double* affine_2x3_out,
                                     double* quality_out) {
  if (!ctx || !affine_2x3_out || num_images < 0) return SRMAP_EINVAL;
  srmap_affine_registration_options opt;
  if (int rc = options_in_force(ctx, options, srmap_affine_registration_options_default, "srmap_affine_registration_options", &opt)) return rc;
  if (opt.hr_scale < 1 || opt.max_iterations < 1 || opt.max_levels < 0 || !(opt.step_tolerance >= 0.0))
    return set_error(ctx, SRMAP_EINVAL, "affine registration: bad options");
  if (num_images == 0) return SRMAP_OK;
  if (!images_host || width < 8 || height < 8)
    return set_error(ctx, SRMAP_EINVAL, "registration needs images of at least 8 x 8");
  // a NaN sum fails every comparison: the seed would keep candidate 0 and the Cholesky refusal would keep the matrix
  for (size_t i = 0, n = (size_t)width * height; i < (size_t)num_images * n; ++i)
    if (!std::isfinite(images_host[i])) return set_error(ctx, SRMAP_EINVAL, "affine registration: image %d is not finite", (int)(i / n));
  const int K = num_images, nf = K - 1;
  const double ident[6] = {1, 0, 0, 0, 1, 0};
  std::copy(ident, ident + 6, affine_2x3_out);
  if (quality_out) { quality_out[0] = 1.0; quality_out[1] = 0.0; quality_out[2] = 1.0; quality_out[3] = 0.0; }
  if (K == 1) return SRMAP_OK;

  std::vector<AffineMap> F(nf);
  std::vector<double> sep(nf, 1.0);
  if (opt.initial_affine_2x3) {
    for (int f = 0; f < nf; ++f) {
      std::copy(opt.initial_affine_2x3 + 6 * (f + 1), opt.initial_affine_2x3 + 6 * (f + 2), F[f].m);
      if (!all_finite(F[f]) || deviation(F[f]) > kAffineMaxDeviation)
        return set_error(ctx, SRMAP_EINVAL, "affine registration: initial matrix %d is not finite or outside the model's domain", f + 1);
    }
  }

  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<int> lw, lh;
  pyramid_levels(width, height, 64, opt.max_levels, &lw, &lh);
  const int L = (int)lw.size();
  std::vector<size_t> off(L + 1, 0);
  for (int l = 0; l < L; ++l) off[l + 1] = off[l] + (size_t)K * lw[l] * lh[l];
  auto chunks_of = [](int h) { return std::min(kMaxRowChunks, std::max(1, (h - 2 + 7) / 8)); };
  const int cw = lw.back(), ch = lh.back();
  const int R = std::max(4, std::min(16, std::min(cw, ch) / 4)), n1 = 2 * R + 1, ncand = n1 * n1;
  const bool seed = !opt.initial_affine_2x3, seed_window = cw - 2 * R > 0 && ch - 2 * R > 0;
  const int seed_chunks = seed_window ? std::min(kMaxSeedChunks, ch - 2 * R) : 0;
  const size_t part_elems = std::max((size_t)nf * chunks_of(height) * kGnSums, seed ? (size_t)nf * ncand * seed_chunks : 0);

  DevBuf pyr;
  FitPass fit;  // its d_part also takes the seed search's partials
  auto fail = [&](int code, const char* what) { return set_error(ctx, code, "affine registration: %s", what); };
  if (pyr.alloc(off[L] * sizeof(double)) != hipSuccess || !fit.alloc(nf, kGnSums, part_elems, true)) return fail(SRMAP_ENOMEM, "allocation failed");
  double* const d_pyr = pyr.as<double>();

  // ---- pyramids of the whole stack, once ----
  if (hipMemcpyAsync(d_pyr, images_host, (size_t)K * width * height * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
    return fail(SRMAP_EHIP, "upload failed");
  for (int l = 1; l < L; ++l) launch_down2_stack(d_pyr + off[l - 1], d_pyr + off[l], lw[l - 1], lh[l - 1], K, st);
  if (hipGetLastError() != hipSuccess) return fail(SRMAP_EHIP, "pyramid failed");

  // ---- seed: integer translation at the coarsest level, or the caller's matrices taken down the pyramid ----
  if (!seed) {
    for (int f = 0; f < nf; ++f)
      for (int l = 1; l < L; ++l) F[f] = to_coarser(F[f]);
  } else {
    for (int f = 0; f < nf; ++f) { std::copy(ident, ident + 6, F[f].m); sep[f] = 0.0; }
    if (seed_window) {
      const int rows = ch - 2 * R, rpc = (rows + seed_chunks - 1) / seed_chunks;
      const size_t n = (size_t)nf * ncand * seed_chunks;
      std::vector<double> h_part(n);
      hipLaunchKernelGGL(k_ssd_window, dim3(ncand, seed_chunks, nf), dim3(256), 0, st, d_pyr + off[L - 1], cw, ch, R, rpc, fit.d_part.as<double>());
      if (hipGetLastError() != hipSuccess ||
          hipMemcpyAsync(h_part.data(), fit.d_part.as<double>(), n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return fail(SRMAP_EHIP, "coarse search failed");
      const double count = (double)rows * (cw - 2 * R);
      std::vector<double> msd(ncand);
      for (int f = 0; f < nf; ++f) {
        int bi = 0;
        for (int c = 0; c < ncand; ++c) {
          double s = 0.0;
          for (int k = 0; k < seed_chunks; ++k) s += h_part[((size_t)f * ncand + c) * seed_chunks + k];
          msd[c] = s / count;
          if (msd[c] < msd[bi]) bi = c;  // the first minimum in row-major order wins
        }
        sep[f] = search_separation(msd.data(), n1, bi);
        F[f].m[2] = bi % n1 - R;
        F[f].m[5] = bi / n1 - R;
      }
    }
  }

  // one pass over every frame flagged active: sums land in fit.sums(f)
  std::vector<char> active(nf, 1);
  auto pass = [&](int l) -> bool {
    for (int f = 0; f < nf; ++f) fit.set(f, F[f], active[f] != 0);
    const int chunks = chunks_of(lh[l]), rpc = (lh[l] - 2 + chunks - 1) / chunks;
    if (!fit.upload(st)) return false;
    hipLaunchKernelGGL(k_affine_gn_sums, dim3(chunks, nf), dim3(256), 0, st, d_pyr + off[l], lw[l], lh[l], rpc, fit.d_tab.as<double>(), fit.d_part.as<double>());
    return fit.reduce_and_fetch(chunks, st);
  };

  // ---- Gauss-Newton, coarse to fine ----
  std::vector<int> iters(nf, 0);
  for (int l = L - 1; l >= 0; --l) {
    std::fill(active.begin(), active.end(), 1);
    for (int it = 0; it < opt.max_iterations; ++it) {
      if (std::find(active.begin(), active.end(), 1) == active.end()) break;
      if (!pass(l)) return fail(SRMAP_EHIP, "Gauss-Newton pass failed");
      for (int f = 0; f < nf; ++f) {
        if (!active[f]) continue;
        const double* S = fit.sums(f);
        ++iters[f];
        if (S[25] < 0.25 * lw[l] * lh[l]) return fail(SRMAP_EINVAL, "Could not determine motion between images.");
        double delta[6];
        if (!solve_step(S, delta)) { active[f] = 0; continue; }  // no texture: this level keeps F
        const AffineMap Fn = compose_with_inverse(F[f], delta, lw[l], lh[l]);
        if (!all_finite(Fn) || deviation(Fn) > kAffineMaxDeviation) return fail(SRMAP_EINVAL, "Could not determine motion between images.");
        const double step = corner_displacement(Fn, F[f], lw[l], lh[l]);
        F[f] = Fn;
        if (step < opt.step_tolerance) active[f] = 0;
      }
    }
    if (l > 0)
      for (int f = 0; f < nf; ++f) F[f] = to_finer(F[f]);
  }

  // ---- residual at the result (full resolution), output ----
  if (quality_out) {
    std::fill(active.begin(), active.end(), 1);
    if (!pass(0)) return fail(SRMAP_EHIP, "residual pass failed");
  }
  for (int f = 0; f < nf; ++f) {
    double* o = affine_2x3_out + 6 * (f + 1);
    std::copy(F[f].m, F[f].m + 6, o);
    o[2] *= opt.hr_scale;
    o[5] *= opt.hr_scale;
    if (quality_out) {
      const double* S = fit.sums(f);
      double* q = quality_out + 4 * (f + 1);
      q[0] = sep[f];
      q[1] = S[25] > 0 ? std::sqrt(S[24] / S[25]) : 0.0;
      q[2] = S[25] / ((double)width * height);
      q[3] = iters[f];
    }
  }
  return SRMAP_OK;
}
