// sample_dev.hpp -- the sample functions of the forward model's warp M_k, shared by the kernels that evaluate it
// (k_forward_direct of kernels_direct.hip, k_forward_affine of kernels_affine.hip) and the kernel that fits the blur to it
// (k_blur_fit_sums of blur_fit.hip): ONE copy of each expression, so that a fit sees exactly the warped image an
// evaluation blurs.  A is the type the four products are formed and added in: the storage type T in the evaluation
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

}  // namespace srmap
