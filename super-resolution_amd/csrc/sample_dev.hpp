// sample_dev.hpp -- the sample functions of the forward model's warp M_k, shared by the kernels that evaluate it
// (k_forward_direct of kernels_direct.hip, k_forward_affine of kernels_affine.hip, k_forward_flow of kernels_flow.hip),
// their transposes in gather form (k_gather_affine, k_gather_flow) and the kernel that fits the blur to it
// (k_blur_fit_sums of blur_fit.hip): ONE copy of each expression, so that a fit sees exactly the warped image an
// evaluation blurs and a transpose recomputes exactly the weights its forward kernel multiplied by.  A is the type the four products are formed and added in: the storage type T in the evaluation
// kernels, double in the fit (the taps and the weights are the same T values either way).
#pragma once

#include <hip/hip_runtime.h>

#include "srmap_internal.hpp"

namespace srmap {

template <typename T>
__device__ __forceinline__ WarpTaps<T> identity_warp() {
  WarpTaps<T> w;
  w.ox = 0; w.oy = 0; w.ntaps = 1; w.fx = 0; w.ytab = nullptr;
  w.w[0] = T(1); w.w[1] = T(0); w.w[2] = T(0); w.w[3] = T(0);
  return w;
}

// warped_k(rr, cc) for (rr, cc) already known to be inside the image:
// cv::warpAffine bilinear gather with zero border (motion_module.cpp:18-38).
template <typename T, typename A = T>
__device__ __forceinline__ A warp_sample(const T* __restrict__ plane, int W, int H,
                                         const WarpTaps<T>& wt, int rr, int cc) {
  int sr = rr + wt.oy;
  const int sc = cc + wt.ox;
  T w0 = wt.w[0], w1 = wt.w[1], w2 = wt.w[2], w3 = wt.w[3];
  if (wt.ytab != nullptr) {
    // per-row y table (rounding-tie shifts): BilinearTab_f's float32 products for this row's fraction index
    const int Y = wt.ytab[rr];
    sr = Y >> 5;
    const float tx1 = (float)wt.fx * (1.f / 32), tx0 = 1.f - tx1;
    const float ty1 = (float)(Y & 31) * (1.f / 32), ty0 = 1.f - ty1;
    w0 = (T)(ty0 * tx0); w1 = (T)(ty0 * tx1); w2 = (T)(ty1 * tx0); w3 = (T)(ty1 * tx1);
  } else if (wt.ntaps == 1) {
    return (sr >= 0 && sr < H && sc >= 0 && sc < W) ? (A)plane[(size_t)sr * W + sc] : A(0);
  }
  const bool r0 = sr >= 0 && sr < H, r1 = sr + 1 >= 0 && sr + 1 < H;
  const bool c0 = sc >= 0 && sc < W, c1 = sc + 1 >= 0 && sc + 1 < W;
  const A v0 = (r0 && c0) ? (A)plane[(size_t)sr * W + sc] : A(0);
  const A v1 = (r0 && c1) ? (A)plane[(size_t)sr * W + sc + 1] : A(0);
  const A v2 = (r1 && c0) ? (A)plane[(size_t)(sr + 1) * W + sc] : A(0);
  const A v3 = (r1 && c1) ? (A)plane[(size_t)(sr + 1) * W + sc + 1] : A(0);
  return ((v0 * (A)w0 + v1 * (A)w1) + v2 * (A)w2) + v3 * (A)w3;
}

// (M_k x)(q) of the affine model: four-tap bilinear sample of `plane` at (sx, sy), zero outside the image; the weights
// are the double products rounded to T
template <typename T, typename A = T>
__device__ __forceinline__ A affine_sample(const T* __restrict__ plane, int W, int H, double sx, double sy) {
  if (!(sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H)) return A(0);  // no tap inside (NaN included)
  const double x0d = __builtin_floor(sx), y0d = __builtin_floor(sy);
  const double fx = sx - x0d, fy = sy - y0d;
  const int sc = (int)x0d, sr = (int)y0d;
  const T w0 = (T)((1.0 - fy) * (1.0 - fx)), w1 = (T)((1.0 - fy) * fx), w2 = (T)(fy * (1.0 - fx)), w3 = (T)(fy * fx);
  const bool r0 = sr >= 0, r1 = sr + 1 < H;  // sr in [-1, H-1], sc in [-1, W-1]
  const bool c0 = sc >= 0, c1 = sc + 1 < W;
  const A v0 = (r0 && c0) ? (A)plane[(size_t)sr * W + sc] : A(0);
  const A v1 = (r0 && c1) ? (A)plane[(size_t)sr * W + sc + 1] : A(0);
  const A v2 = (r1 && c0) ? (A)plane[(size_t)(sr + 1) * W + sc] : A(0);
  const A v3 = (r1 && c1) ? (A)plane[(size_t)(sr + 1) * W + sc + 1] : A(0);
  return ((v0 * (A)w0 + v1 * (A)w1) + v2 * (A)w2) + v3 * (A)w3;
}

// s = q + u(q) along one axis, the sample position of the displacement-field model (kernels_flow.hip): both conversions
// and the one addition are exact in double for |u| <= 2^20, in both dtypes
template <typename T>
__device__ __forceinline__ double flow_source(int q, T u) {
  return (double)q + (double)u;
}

// weight of tap `p` along one axis for a sample at coordinate s: the forward kernel's (1 - f) / f, 0 for any other p
__device__ __forceinline__ double affine_axis_weight(double s, int p) {
  const double s0 = __builtin_floor(s), f = s - s0, pd = (double)p;
  return s0 == pd ? 1.0 - f : (s0 + 1.0 == pd ? f : 0.0);
}

// (B^T D^T r)(q) at the HR pixel q = (pc, pr) inside the image: k_gather_direct's inner expression (zero-insertion
// upsample, correlation with kernel.t(), each stage clipped to the domain; only the taps that land on the LR grid)
template <typename T>
__device__ __forceinline__ T blur_t_upsampled_at(const T* __restrict__ rk, const T* __restrict__ blur_t, const Geometry& g,
                                                 int gs, int pr, int pc) {
  T v = T(0);
  int a0 = (g.hb - pr) % gs, e0 = (g.hb - pc) % gs;
  if (a0 < 0) a0 += gs;
  if (e0 < 0) e0 += gs;
  for (int a = a0; a < g.b; a += gs) {
    const int R = pr + a - g.hb;
    if (R < 0 || R >= g.H) continue;
    const int li = R / gs;
    if (li >= g.h) continue;
    for (int e = e0; e < g.b; e += gs) {
      const int Cc = pc + e - g.hb;
      if (Cc < 0 || Cc >= g.W) continue;
      const int lj = Cc / gs;
      if (lj >= g.w) continue;
      v += blur_t[a * g.b + e] * rk[(size_t)li * g.w + lj];
    }
  }
  return v;
}

}  // namespace srmap
