// motion_refinement.hip -- joint motion refinement (srmap_refine_motion): re-fit every frame's 2 x 3 matrix
// to an HR estimate x THROUGH the forward model, minimising E_k(G) = sum_c sum_u w_k(c,u) r^2, r = (D B M(G) x)(c,u) - y_k(c,u),
// over G = F_k^-1 by Levenberg-Marquardt.  The model holds the aliasing, the blur and the zero border that bias a
// frame-to-frame registration (registration_affine.hip).  No reference counterpart; the checker is
// tests/motion_refinement_restatement.py.
//   pass      ONE launch of k_refine_sums for every still-active frame: per LR pixel and channel the residual r and
//             J_i = sum over k_forward_direct's blur taps of blur * g * {q_x - c0x, q_y - c0y, 1}, g the exact derivative of
//             the four-tap sample in s_x (i = 0..2) or s_y (i = 3..5), from the four tap values the sample itself uses;
//             28 f64 sums per workgroup (21 of H = sum w J J^T, upper triangle row-major; 6 of g = sum w J r; E), folded by a
//             wave shuffle and LDS in a fixed order, no atomics (fold_sums_256); k_fit_reduce adds the chunk records in
//             index order;
//   pacing    per pass one upload of the frame table, one copy of K x 28 doubles, one stream wait (section 3.7's; FitPass,
//             motion_fit.hip);
//   LM        on the host in double, per frame, in lockstep: (H + lambda diag H) d = -g by the Cholesky of affine_map.hpp
//             (dof = 2: the 2 x 2 sub-system of (tx, ty)), G' = G + dL (q - c0) + dt.
// Everything after the loads is double in both dtypes.  Sample positions are the affine sampler's (sample_dev.hpp; affine_coord of
// motion_fit_dev.hpp).
#include <algorithm>
#include <cmath>
#include <vector>

#include "affine_map.hpp"
#include "motion_fit_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kSums = 28;       // 21 of H, 6 of g, E
constexpr int kMaxChunks = 256;
constexpr double kMinDamping = 1e-9, kMaxDamping = 1e6;

// Sums of one pass for every active frame: grid = (chunks of LR pixels, frames), 256 threads; a workgroup covers the LR
// pixels [chunk * 256 * ppt, (chunk + 1) * 256 * ppt) of its frame, thread t the pixels t, t + 256, ...
// table[k][kFitTabRec] (G = [ia ib itx ic id ity], active, pad) is indexed by the frame alone (scalar loads).
// partial[(k * chunks + chunk)][28].
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_refine_sums(const T* __restrict__ x, const T* __restrict__ y,
                                                     const T* __restrict__ dw, Geometry g, const T* __restrict__ blur,
                                                     const int* __restrict__ col_map, const int* __restrict__ row_map,
                                                     const double* __restrict__ table, int ppt,
                                                     double* __restrict__ partial, BlurStride bs) {
  __shared__ double red[kSums][4];
  const int k = blockIdx.y;
  const double* __restrict__ m = table + (size_t)k * kFitTabRec;  // uniform: scalar loads
  if (m[6] == 0.0) return;                                     // stopped frame: uniform
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  const int n = g.w * g.h;
  const double c0x = 0.5 * (double)(g.W - 1), c0y = 0.5 * (double)(g.H - 1);
  double acc[kSums];
#pragma unroll
  for (int q = 0; q < kSums; ++q) acc[q] = 0.0;
  const size_t base = (size_t)blockIdx.x * 256 * ppt + threadIdx.x;
  for (int t = 0; t < ppt; ++t) {
    const size_t lp = base + (size_t)t * 256;
    if (lp >= (size_t)n) break;
    const int i = (int)(lp / g.w), j = (int)(lp - (size_t)i * g.w);
    const int R0 = row_map[i], C0 = col_map[j];
    for (int c = 0; c < g.C; ++c) {
      const T* __restrict__ plane = x + (size_t)c * g.W * g.H;
      const T* __restrict__ blur_kc = blur + ((size_t)k * bs.frame + (size_t)c * bs.channel);  // a bank's entry; strides 0 without one
      double val = 0.0, J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int a = 0; a < g.b; ++a) {
        const int rr = R0 + a - g.hb;
        if (rr < 0 || rr >= g.H) continue;  // k_forward_direct's taps: the blur's zero border
        for (int e = 0; e < g.b; ++e) {
          const int cc = C0 + e - g.hb;
          if (cc < 0 || cc >= g.W) continue;
          const double sx = affine_coord(m0, m1, m2, (double)cc, (double)rr);
          const double sy = affine_coord(m3, m4, m5, (double)cc, (double)rr);
          if (!(sx > -1.0 && sx < (double)g.W && sy > -1.0 && sy < (double)g.H)) continue;  // no tap inside (NaN included)
          const double x0d = __builtin_floor(sx), y0d = __builtin_floor(sy);
          const double fx = sx - x0d, fy = sy - y0d;
          const int sc = (int)x0d, sr = (int)y0d;  // sr in [-1, H-1], sc in [-1, W-1]
          const bool r0 = sr >= 0, r1 = sr + 1 < g.H, q0 = sc >= 0, q1 = sc + 1 < g.W;
          const double v00 = (r0 && q0) ? (double)plane[(size_t)sr * g.W + sc] : 0.0;
          const double v01 = (r0 && q1) ? (double)plane[(size_t)sr * g.W + sc + 1] : 0.0;
          const double v10 = (r1 && q0) ? (double)plane[(size_t)(sr + 1) * g.W + sc] : 0.0;
          const double v11 = (r1 && q1) ? (double)plane[(size_t)(sr + 1) * g.W + sc + 1] : 0.0;
          const double bw = (double)blur_kc[a * g.b + e];
          const double s = (1.0 - fy) * ((1.0 - fx) * v00 + fx * v01) + fy * ((1.0 - fx) * v10 + fx * v11);
          const double gx = bw * ((1.0 - fy) * (v01 - v00) + fy * (v11 - v10));
          const double gy = bw * ((1.0 - fx) * (v10 - v00) + fx * (v11 - v01));
          const double u = (double)cc - c0x, v = (double)rr - c0y;
          val += bw * s;
          J[0] += gx * u; J[1] += gx * v; J[2] += gx;
          J[3] += gy * u; J[4] += gy * v; J[5] += gy;
        }
      }
      const size_t oi = ((size_t)k * g.C + c) * n + lp;
      const double r = val - (double)y[oi];
      const double wv = WEIGHTED ? (double)dw[oi] : 1.0;
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double wj = wv * J[a];
#pragma unroll
        for (int e = a; e < 6; ++e) acc[q++] += wj * J[e];
        acc[21 + a] += wj * r;
      }
      acc[27] += (wv * r) * r;
    }
  }
  fold_sums_256(acc, red, partial + ((size_t)k * gridDim.x + blockIdx.x) * kSums);
}

// ---- host side ----
// (H + lambda diag H) d = -g over the parameters idx[0..n) by Cholesky; the other entries of d are 0.  S: the 28 sums.
// false: no texture
bool lm_step(const double* S, double lambda, const int* idx, int n, double* d) {
  double Hf[6][6], A[6][6], ng[6], sol[6];
  for (int i = 0, q = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++q) Hf[i][j] = Hf[j][i] = S[q];
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) A[i][j] = Hf[idx[i]][idx[j]];
    A[i][i] = A[i][i] + lambda * A[i][i];
    ng[i] = -S[21 + idx[i]];
  }
  if (!cholesky_solve(A, ng, n, sol)) return false;
  for (int i = 0; i < 6; ++i) d[i] = 0.0;
  for (int i = 0; i < n; ++i) d[idx[i]] = sol[i];
  return true;
}

struct FrameState {
  AffineMap F, G, Gt, Ft;  // current matrix and its inverse; the trial and its inverse
  double S[kSums];     // sums at G
  double lambda = 0.0, e0 = 0.0;
  int passes = 0, status = 1;
  bool active = false;
};

template <typename T>
void launch_sums(srmap_problem* p, const T* x, const double* d_tab, int chunks, int ppt, double* d_part, hipStream_t st) {
  const Geometry& g = p->geo;
  dim3 grid(chunks, g.K);
  const BlurStride bs = p->blur.stride();
  const T* dw = p->dw.effective<T>();
  dispatch_value<0, 1>(dw != nullptr, [&](auto weighted) {
    hipLaunchKernelGGL((k_refine_sums<T, decltype(weighted)::value != 0>), grid, dim3(256), 0, st, x, p->d_obs.as<const T>(), dw, g,
                       p->blur.table<T>(), p->d_col_map.as<int>(), p->d_row_map.as<int>(), d_tab, ppt, d_part, bs);
  });
}

}  // namespace

}  // namespace srmap

using namespace srmap;

extern "C" void srmap_motion_refinement_options_default(srmap_motion_refinement_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_motion_refinement_options);
  o->dof = 6;
  o->max_iterations = 30;
  o->step_tolerance = 1e-4;
  o->initial_damping = 1e-3;
  o->apply = 1;
  o->initial_affine_2x3 = nullptr;
}

extern "C" int srmap_refine_motion_device(srmap_problem* p, const void* x_dev, void* hip_stream,
                                          const srmap_motion_refinement_options* options, double* affine_2x3_out,
                                          double* quality_out, double* normal_equations_out) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  srmap_ctx* ctx = p->ctx;
  if (p->motion.is_field())
    return p->motion.refuse(ctx, SRMAP_EUNSUPPORTED, "motion refinement fits affine matrices: not available while %s is set (%s)");
  srmap_motion_refinement_options opt;
  if (int rc = options_in_force(ctx, options, srmap_motion_refinement_options_default, "srmap_motion_refinement_options", &opt)) return rc;
  if (opt.dof != 2 && opt.dof != 6) return set_error(ctx, SRMAP_EINVAL, "motion refinement: dof must be 2 or 6 (got %d)", opt.dof);
  if (opt.max_iterations < 0 || !(opt.step_tolerance >= 0.0) || !(opt.initial_damping >= 0.0) ||
      !std::isfinite(opt.step_tolerance) || !std::isfinite(opt.initial_damping))
    return set_error(ctx, SRMAP_EINVAL, "motion refinement: bad options");
  if (!p->have_obs) return set_error(ctx, SRMAP_EINVAL, "no observations set");
  const Geometry& g = p->geo;
  const int K = g.K;

  // starting matrices: the caller's, else the problem's affine motion, else its shifts, else the identity
  std::vector<double> start((size_t)K * 6, 0.0);
  const std::vector<double>& set = p->motion.replacement().recs;  // the records of an affine motion in force
  for (int k = 0; k < K; ++k) {
    double* s = start.data() + 6 * (size_t)k;
    if (opt.initial_affine_2x3) std::copy(opt.initial_affine_2x3 + 6 * (size_t)k, opt.initial_affine_2x3 + 6 * (size_t)(k + 1), s);
    else if (p->motion.kind() == kMotionAffine) std::copy(&set[(size_t)k * kAffineRec + 6], &set[(size_t)k * kAffineRec + 12], s);
    else {
      s[0] = 1.0; s[4] = 1.0;
      if (p->motion.has_table()) { s[2] = p->motion.shifts()[2 * (size_t)k]; s[5] = p->motion.shifts()[2 * (size_t)k + 1]; }
    }
  }
  std::vector<double> recs;
  int rc = affine_records(ctx, K, start.data(), &recs);  // EINVAL: not finite; EUNSUPPORTED: outside the domain
  if (rc) return rc;

  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream_of(ctx, hip_stream);
  rc = problem_state_read(p, st);
  if (rc) return rc;

  const PixelChunks plan = plan_pixel_chunks(g.w * g.h, kMaxChunks);
  const int ppt = plan.ppt, chunks = plan.chunks;
  FitPass fit;
  auto fail = [&](int code, const char* what) { return set_error(ctx, code, "motion refinement: %s", what); };
  if (!fit.alloc(K, kSums, (size_t)K * chunks * kSums, true)) return fail(SRMAP_ENOMEM, "allocation failed");

  std::vector<FrameState> fs(K);
  for (int k = 0; k < K; ++k) {
    std::copy(start.data() + 6 * (size_t)k, start.data() + 6 * (size_t)(k + 1), fs[k].F.m);
    std::copy(recs.data() + (size_t)k * kAffineRec, recs.data() + (size_t)k * kAffineRec + 6, fs[k].G.m);
    fs[k].Gt = fs[k].G;
    fs[k].Ft = fs[k].F;
    fs[k].lambda = opt.initial_damping;
    fs[k].active = true;
  }

  // one pass over the trial matrices of every active frame: sums land in fit.sums(k)
  auto pass = [&]() -> bool {
    for (int k = 0; k < K; ++k) fit.set(k, fs[k].Gt, fs[k].active);
    if (!fit.upload(st)) return false;
    dispatch_dtype(p->dtype, [&](auto t) { launch_sums<decltype(t)>(p, (const decltype(t)*)x_dev, fit.d_tab.as<double>(), chunks, ppt, fit.d_part.as<double>(), st); });
    return fit.reduce_and_fetch(chunks, st);
  };

  const double c0x = 0.5 * (double)(g.W - 1), c0y = 0.5 * (double)(g.H - 1);
  static const int idx6[6] = {0, 1, 2, 3, 4, 5}, idx2[2] = {2, 5};
  const int* idx = opt.dof == 2 ? idx2 : idx6;
  // the next trial of frame k from its current sums, or its stop; rejections that need no pass are taken here
  auto propose = [&](FrameState& f) {
    while (f.active) {
      if (f.passes - 1 >= opt.max_iterations) { f.status = 1; f.active = false; break; }
      double d[6];
      if (!lm_step(f.S, f.lambda, idx, opt.dof, d)) { f.status = 3; f.active = false; break; }
      f.Gt = increment(f.G, d, c0x, c0y);
      f.Ft = inverse(f.Gt);
      if (opt.dof == 2) { f.Ft.m[0] = f.F.m[0]; f.Ft.m[1] = f.F.m[1]; f.Ft.m[3] = f.F.m[3]; f.Ft.m[4] = f.F.m[4]; }
      if (all_finite(f.Gt) && all_finite(f.Ft) && deviation(f.Ft) <= kAffineMaxDeviation) break;  // a trial for the next pass
      f.lambda *= 10.0;
      if (f.lambda > kMaxDamping) { f.status = 2; f.active = false; }
    }
  };

  if (!pass()) return fail(SRMAP_EHIP, "pass failed");
  for (int k = 0; k < K; ++k) {
    FrameState& f = fs[k];
    std::copy(fit.sums(k), fit.sums(k) + kSums, f.S);
    f.e0 = f.S[27];
    f.passes = 1;
    if (k == 0) { f.active = false; f.passes = 0; f.status = 0; continue; }  // the gauge
    propose(f);
  }
  for (;;) {
    bool any = false;
    for (int k = 0; k < K; ++k) any = any || fs[k].active;
    if (!any) break;
    if (!pass()) return fail(SRMAP_EHIP, "pass failed");
    for (int k = 0; k < K; ++k) {
      FrameState& f = fs[k];
      if (!f.active) continue;
      const double* S = fit.sums(k);
      ++f.passes;
      if (S[27] < f.S[27]) {  // accepted: the trial's sums become the current ones
        const double step = corner_displacement(f.F, f.Ft, g.W, g.H);
        f.G = f.Gt;
        f.F = f.Ft;
        std::copy(S, S + kSums, f.S);
        f.lambda = std::max(f.lambda / 10.0, kMinDamping);
        if (step < opt.step_tolerance) { f.status = 0; f.active = false; continue; }
      } else {
        f.lambda *= 10.0;
        if (f.lambda > kMaxDamping) { f.status = 2; f.active = false; continue; }
      }
      propose(f);
    }
  }

  std::vector<double> result((size_t)K * 6);
  for (int k = 0; k < K; ++k) std::copy(fs[k].F.m, fs[k].F.m + 6, result.data() + 6 * (size_t)k);
  if (opt.apply) {
    rc = srmap_problem_set_affine_motion(p, result.data());
    if (rc) return rc;
  }
  for (int k = 0; k < K; ++k) {
    const FrameState& f = fs[k];
    if (affine_2x3_out) std::copy(f.F.m, f.F.m + 6, affine_2x3_out + 6 * (size_t)k);
    if (quality_out) {
      double* q = quality_out + 4 * (size_t)k;
      q[0] = f.e0; q[1] = f.S[27]; q[2] = f.passes; q[3] = f.status;
    }
    if (normal_equations_out) std::copy(f.S, f.S + kSums, normal_equations_out + (size_t)kSums * k);
  }
  return SRMAP_OK;
}

extern "C" int srmap_refine_motion(srmap_problem* p, const double* x_host, const srmap_motion_refinement_options* options,
                                   double* affine_2x3_out, double* quality_out, double* normal_equations_out) {
  if (!p || !x_host) return SRMAP_EINVAL;
  if (int rc = host_fit_prologue(p, x_host, options, srmap_motion_refinement_options_default, "srmap_motion_refinement_options")) return rc;
  return srmap_refine_motion_device(p, p->d_x.as(), p->ctx->stream, options, affine_2x3_out, quality_out, normal_equations_out);
}
