// sample_dev.hpp -- the forward model's warp M_k on the device, shared by the kernels that evaluate it (k_forward_direct
// of kernels_data_direct.hip, every motion kind), the transposes in gather form of the per-pixel kinds (k_gather_sampled) and
// the kernels that fit to it (k_blur_fit_sums of blur_fit.hip, k_photometric_sums of photometric_fit.hip): ONE copy of
// each expression AND of the choice between them (MotionSampler), so that a fit sees exactly the warped image an
// evaluation blurs and a transpose recomputes exactly the weights its forward kernel multiplied by.  A is the type the
// four products are formed and added in: the storage type T in the evaluation kernels, double in the fits (the taps and
// the weights are the same T values either way).  MotionKind and the kernel argument block MotionArgs<T> are declared in
// srmap_internal.hpp, next to the host helpers that name the kind, fill the block and dispatch on it.  The table kind
// tests its table for null in every kernel (a uniform branch): only the forward kernel is ever given none.
#pragma once

#include <hip/hip_runtime.h>

#include "motion_fit_dev.hpp"
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

// s = q + u(q) along one axis, the sample position of the displacement-field model: both conversions
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

// (B^T D^T r)(q) at the HR pixel q = (pc, pr) inside the image, the inner expression of k_gather_direct and k_gather_sampled (zero-insertion
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

// The transpose of the displacement-field model finds its candidates around a seed stored per (frame, HR pixel) when the
// field is set (kernels_flow.hip): seed (sx, sy), each clamped to [-kFlowPad, size - 1 + kFlowPad], as one int
constexpr int kFlowPad = kFlowRadius;
__device__ __forceinline__ int flow_pack_seed(int sx, int sy, int W) { return (sy + kFlowPad) * (W + 2 * kFlowPad) + (sx + kFlowPad); }
__device__ __forceinline__ void flow_unpack_seed(int v, int W, int* sx, int* sy) {
  const int SW = W + 2 * kFlowPad;
  const int y = v / SW;
  *sy = y - kFlowPad;
  *sx = v - y * SW - kFlowPad;
}

// The displacement field of one frame kept on a control lattice (LatticeDesc, srmap_internal.hpp): u at the HR pixel
// (x, y) is the bilinear interpolant of the frame's nodes at (x, y) / step, clamped to the lattice (constant beyond the
// last node), in double, in k_flow_resample's order (registration_flow.hip with sub = 0, div = step, gain = 1) and
// without contraction, then rounded ONCE to T: the value a dense field holds after srmap_problem_set_flow rounded the
// same interpolant.  The one copy of that expression: the evaluation kernels (MotionSampler's lattice kind) and the
// set-time kernels (kernels_flow.hip) read u through it.  The node bases are wave-uniform.
template <typename T>
struct LatticeField {
  const double* __restrict__ nx;
  const double* __restrict__ ny;
  int step, lw, lh;
  __device__ __forceinline__ LatticeField(const LatticeDesc& a, int k)
      : nx(a.nodes + (size_t)k * 2 * (a.lw * a.lh)), ny(nx + a.lw * a.lh), step(a.step), lw(a.lw), lh(a.lh) {}
  __device__ __forceinline__ double value(const double* __restrict__ plane, int x, int y) const {
#pragma clang fp contract(off)
    const double cx = fmin(fmax((double)x / (double)step, 0.0), (double)(lw - 1));
    const double cy = fmin(fmax((double)y / (double)step, 0.0), (double)(lh - 1));
    const int xi = min((int)__builtin_floor(cx), lw - 2), yi = min((int)__builtin_floor(cy), lh - 2);
    const double fx = cx - (double)xi, fy = cy - (double)yi;
    const double* __restrict__ p = plane + (size_t)yi * lw + xi;
    return (1.0 - fy) * ((1.0 - fx) * p[0] + fx * p[1]) + fy * ((1.0 - fx) * p[lw] + fx * p[lw + 1]);
  }
  // the reader's form of the set-time kernels: (flat pixel index, x, y)
  __device__ __forceinline__ T ux(size_t, int x, int y) const { return (T)value(nx, x, y); }
  __device__ __forceinline__ T uy(size_t, int x, int y) const { return (T)value(ny, x, y); }
};

// M_k of frame k for one motion kind (MotionKind, srmap_internal.hpp), built from the kernel's argument block, the
// geometry and the WAVE-UNIFORM frame index alone: the affine record then comes through scalar loads, and the plane bases
// of the field and of the seeds are uniform.
//   at<A>(plane, W, H, rr, cc)   (M_k x)(rr, cc) for (rr, cc) inside the W x H image: what every forward and fit kernel
//                             multiplies a blur tap by.  The size comes by value, as the sample functions take it: read
//                             through a reference to the geometry inside at(), the table kind's forward instance needed
//                             three more registers and ran 2 % slower.
// The per-pixel kinds also describe the exact transpose in gather form (k_gather_sampled): the pixels q whose footprint
// can contain the HR pixel p = (col, r) are a kWindow x kWindow block,
//   window(g, hp, r, col, &qx0, &qy0)   its first candidate, or false when p has none;
//   weight_x(qi, qx, qy, col), weight_y(qi, qx, qy, r)   the two factors of the weight of (q, p), qi = qy * W + qx formed
//                                       once by the gather, each recomputed from q's sample position along that axis by
//                                       at()'s expressions (0.0: p is no tap of q); the gather asks for the y factor only
//                                       where the x factor is not zero.
template <typename T, int MOTION>
struct MotionSampler;

template <typename T>
struct MotionSampler<T, kMotionNone> {
  __device__ __forceinline__ MotionSampler(const MotionArgs<T>&, const Geometry&, int) {}
  template <typename A>
  __device__ __forceinline__ A at(const T* __restrict__ plane, int W, int H, int rr, int cc) const {
    return (A)plane[(size_t)rr * W + cc];
  }
};

// translation: the frame's tap table; a problem without motion has no table (warps == nullptr) and takes the identity
template <typename T>
struct MotionSampler<T, kMotionTable> {
  WarpTaps<T> wt;
  __device__ __forceinline__ MotionSampler(const MotionArgs<T>& a, const Geometry&, int k)
      : wt(a.warps ? a.warps[k] : identity_warp<T>()) {}
  template <typename A>
  __device__ __forceinline__ A at(const T* __restrict__ plane, int W, int H, int rr, int cc) const {
    return warp_sample<T, A>(plane, W, H, wt, rr, cc);
  }
};

// affine: s = F_k^-1(q) by the frame's record (kAffineRec doubles: inverse map, forward map, candidate radii).  The
// candidates of p are the integers inside F_k(p) +- (|a|+|b|, |c|+|d|), at most 3 x 3 under the entry point's bound.
template <typename T>
struct MotionSampler<T, kMotionAffine> {
  static constexpr int kWindow = 3;
  const double* __restrict__ m;
  __device__ __forceinline__ MotionSampler(const MotionArgs<T>& a, const Geometry&, int k)
      : m(a.recs + (size_t)k * kAffineRec) {}
  template <typename A>
  __device__ __forceinline__ A at(const T* __restrict__ plane, int W, int H, int rr, int cc) const {
    const double sx = affine_coord(m[0], m[1], m[2], (double)cc, (double)rr);
    const double sy = affine_coord(m[3], m[4], m[5], (double)cc, (double)rr);
    return affine_sample<T, A>(plane, W, H, sx, sy);
  }
  __device__ __forceinline__ bool window(const Geometry& g, int, int r, int col, int* qx0, int* qy0) const {
    // F_k(p) and the first candidate of each axis; clamped ahead of the conversion (a far translation: no candidate)
    const double cx = affine_coord(m[6], m[7], m[8], (double)col, (double)r);
    const double cy = affine_coord(m[9], m[10], m[11], (double)col, (double)r);
    const double lx = __builtin_ceil(cx - m[12]), ly = __builtin_ceil(cy - m[13]);
    if (!(lx > -4.0 && lx < (double)g.W && ly > -4.0 && ly < (double)g.H)) return false;
    *qx0 = (int)lx;
    *qy0 = (int)ly;
    return true;
  }
  __device__ __forceinline__ double weight_x(size_t, int qx, int qy, int col) const {
    return affine_axis_weight(affine_coord(m[0], m[1], m[2], (double)qx, (double)qy), col);
  }
  __device__ __forceinline__ double weight_y(size_t, int qx, int qy, int r) const {
    return affine_axis_weight(affine_coord(m[3], m[4], m[5], (double)qx, (double)qy), r);
  }
};

// displacement field: s = q + u_k(q), the (ux, uy) planes of frame k.  The candidates of p are the (2 kFlowRadius + 1)^2
// pixels around p's seed (verified when the field was set).
template <typename T>
struct MotionSampler<T, kMotionFlow> {
  static constexpr int kWindow = 2 * kFlowRadius + 1;
  const T* __restrict__ fux;
  const T* __restrict__ fuy;
  const int* __restrict__ seeds;
  __device__ __forceinline__ MotionSampler(const MotionArgs<T>& a, const Geometry& g, int k)
      : fux(a.flow + (size_t)k * 2 * (g.W * g.H)), fuy(fux + g.W * g.H), seeds(a.seeds + (size_t)k * (g.W * g.H)) {}
  template <typename A>
  __device__ __forceinline__ A at(const T* __restrict__ plane, int W, int H, int rr, int cc) const {
    const size_t qi = (size_t)rr * W + cc;
    const double sx = flow_source(cc, fux[qi]), sy = flow_source(rr, fuy[qi]);
    return affine_sample<T, A>(plane, W, H, sx, sy);
  }
  __device__ __forceinline__ bool window(const Geometry& g, int hp, int, int, int* qx0, int* qy0) const {
    flow_unpack_seed(seeds[hp], g.W, qx0, qy0);
    *qx0 -= kFlowRadius;
    *qy0 -= kFlowRadius;
    return true;
  }
  __device__ __forceinline__ double weight_x(size_t qi, int qx, int, int col) const {
    return affine_axis_weight(flow_source(qx, fux[qi]), col);
  }
  __device__ __forceinline__ double weight_y(size_t qi, int, int qy, int r) const {
    return affine_axis_weight(flow_source(qy, fuy[qi]), r);
  }
};

// displacement field on a control lattice: the flow kind with u_k(q) interpolated from the frame's nodes (LatticeField)
// where that kind loads it; seeds, window and weights are the flow kind's.  The nodes come through the caches per
// sample: 4 doubles per component, shared by the step x step pixels of a cell.  The gather was also measured with the
// 3 x 3 ux nodes of a window held in registers (loaded once per frame, picked by selects): 88-92 VGPRs against 52-56 and
// 1.23 x the time of this form (profiles/r24_flow_lattice.txt), so the per-candidate form stays.  The compiler already
// forms cy / yi / fy once per window row; one double division per candidate (cx) is left.
template <typename T>
struct MotionSampler<T, kMotionLattice> {
  static constexpr int kWindow = 2 * kFlowRadius + 1;
  const LatticeField<T> f;
  const int* __restrict__ seeds;
  __device__ __forceinline__ MotionSampler(const MotionArgs<T>& a, const Geometry& g, int k)
      : f(a.lat, k), seeds(a.seeds + (size_t)k * (g.W * g.H)) {}
  template <typename A>
  __device__ __forceinline__ A at(const T* __restrict__ plane, int W, int H, int rr, int cc) const {
    const double sx = flow_source(cc, f.ux(0, cc, rr)), sy = flow_source(rr, f.uy(0, cc, rr));
    return affine_sample<T, A>(plane, W, H, sx, sy);
  }
  __device__ __forceinline__ bool window(const Geometry& g, int hp, int, int, int* qx0, int* qy0) const {
    flow_unpack_seed(seeds[hp], g.W, qx0, qy0);
    *qx0 -= kFlowRadius;
    *qy0 -= kFlowRadius;
    return true;
  }
  __device__ __forceinline__ double weight_x(size_t, int qx, int qy, int col) const {
    return affine_axis_weight(flow_source(qx, f.ux(0, qx, qy)), col);
  }
  __device__ __forceinline__ double weight_y(size_t, int qx, int qy, int r) const {
    return affine_axis_weight(flow_source(qy, f.uy(0, qx, qy)), r);
  }
};

}  // namespace srmap
