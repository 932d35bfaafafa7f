// kernels_affine.hip -- the direct family's data-term kernels for an AFFINE per-frame motion model
// (srmap_problem_set_affine_motion; no reference counterpart: motion_module.cpp:18-51 warps by a translation only).
//
// Frame k maps HR content at p to F_k(p) = L_k p + t_k in its HR-grid image.  The forward warp samples x bilinearly at
// s = F_k^-1(q) for every pixel q of the warped image (taps outside the image contribute 0); blur and decimation are the
// translational path's (k_forward_direct).  The transpose is the EXACT transpose of that matrix in gather form: for an HR
// pixel p the pixels q whose footprint contains p are the integers inside F_k(p) +- (|a|+|b|, |c|+|d|), at most 3 x 3
// under the domain bound of the entry point; the weight of (q, p) is recomputed from s = F_k^-1(q) by the expressions the
// forward kernel uses, so the two kernels hold the same matrix bit for bit and no atomics are needed.
//
// Source coordinates are double in both dtypes (an f32 coordinate at 2048 px carries 1e-4 px of error) and are formed by
// the same uncontracted expression in both kernels (affine_coord); the weights are the double products rounded to T.
//
// Both kernels read their sources through the caches (per LR pixel b^2 x 4 taps of x; per HR pixel and frame <= 9
// candidates, each the taps of B^T D^T that land on the LR grid).  The frame's record (kAffineRec doubles: inverse map,
// forward map, candidate radii) is indexed by wave-uniform values only, so it comes through scalar loads.
#include <algorithm>
#include <cmath>

#include "affine_map.hpp"
#include "motion_fit_dev.hpp"
#include "sample_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

// s = F^-1(q) for the warped-image pixel q = (qx, qy): THE expression of both kernels (affine_coord, motion_fit_dev.hpp)
__device__ __forceinline__ void affine_source(const double* __restrict__ m, int qx, int qy, double* sx, double* sy) {
  *sx = affine_coord(m[0], m[1], m[2], (double)qx, (double)qy);
  *sy = affine_coord(m[3], m[4], m[5], (double)qx, (double)qy);
}

// (M_k x)(q), the four-tap sample at (sx, sy): affine_sample of sample_dev.hpp (shared with the blur fit)

// affine_axis_weight and blur_t_upsampled_at: sample_dev.hpp (shared with kernels_flow.hip)

}  // namespace

// ---------------------------------------------------------------------------
// A_k = D B M_k at every LR pixel of frames [k0, k0 + gridDim.z): k_forward_direct's contract (residual or weighted
// residual into `out`, cost partial with the cost-row test, one partial per workgroup in the same order).
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_forward_affine(
    const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out, double* __restrict__ partials, Geometry g,
    const double* __restrict__ recs, const T* __restrict__ blur, const int* __restrict__ col_map,
    const int* __restrict__ row_map, int k0, double cost_scale, int obs_C, int obs_c0, const T* __restrict__ dw) {
  __shared__ double red[4];
  const int lp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, kk = blockIdx.z, k = k0 + kk;
  const int n = g.w * g.h;
  const double* __restrict__ m = recs + (size_t)k * kAffineRec;  // uniform: scalar loads
  double sq = 0.0;
  if (lp < n) {
    const int i = lp / g.w, j = lp - i * g.w;
    const int R0 = row_map[i], C0 = col_map[j];
    const T* plane = x + (size_t)c * g.W * g.H;
    T acc = T(0);
    for (int a = 0; a < g.b; ++a) {
      const int rr = R0 + a - g.hb;
      if (rr < 0 || rr >= g.H) continue;  // filter2D BORDER_CONSTANT on the warped image
      for (int e = 0; e < g.b; ++e) {
        const int cc = C0 + e - g.hb;
        if (cc < 0 || cc >= g.W) continue;
        double sx, sy;
        affine_source(m, cc, rr, &sx, &sy);
        acc += blur[a * g.b + e] * affine_sample(plane, g.W, g.H, sx, sy);
      }
    }
    T res = acc;
    if (WEIGHTED) {
      const size_t oi = ((size_t)k * obs_C + c + obs_c0) * n + lp;
      const T yv = y[oi], wv = dw[oi];
      res -= yv;
      const T wr = wv * res;
      out[((size_t)kk * g.C + c) * n + lp] = wr;
      sq = (i * g.s >= g.cr0 && i * g.s < g.cr1) ? (double)wr * (double)res : 0.0;
    } else {
      if (y) res -= y[((size_t)k * obs_C + c + obs_c0) * n + lp];
      out[((size_t)kk * g.C + c) * n + lp] = res;
      sq = (i * g.s >= g.cr0 && i * g.s < g.cr1) ? (double)res * (double)res : 0.0;
    }
  }
  if (partials) {
    const double s = block_sum_256(sq, red);
    if (threadIdx.x == 0)
      partials[(size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = cost_scale * s;
  }
}

template <typename T>
int launch_forward_affine(srmap_problem* p, const Geometry& g, const T* x, const T* y, int obs_C, int obs_c0, T* out,
                          int k0, int nk, double* partials, int* nblocks, hipStream_t st, const T* dw) {
  if (!p->affine || !p->d_affine) return set_error(p->ctx, SRMAP_EINVAL, "internal: no affine motion set");
  if (dw != nullptr && y == nullptr) return set_error(p->ctx, SRMAP_EINVAL, "internal: data weights without observations");
  dim3 grid((g.w * g.h + 255) / 256, g.C, nk);
  const double cost_scale = (double)g.s * (double)g.s;
  if (dw != nullptr)
    hipLaunchKernelGGL((k_forward_affine<T, true>), grid, dim3(256), 0, st, x, y, out, partials, g, p->d_affine,
                       (const T*)p->d_blur, p->d_col_map, p->d_row_map, k0, cost_scale, obs_C, obs_c0, dw);
  else
    hipLaunchKernelGGL((k_forward_affine<T, false>), grid, dim3(256), 0, st, x, y, out, partials, g, p->d_affine,
                       (const T*)p->d_blur, p->d_col_map, p->d_row_map, k0, cost_scale, obs_C, obs_c0, dw);
  if (nblocks) *nblocks = (int)(grid.x * grid.y * grid.z);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// ---------------------------------------------------------------------------
// g = (accumulate ? g : 0) + out_scale * sum_k M_k^T B^T D^T r_k at every HR pixel: frames in increasing order, per frame
// the <= 3 x 3 candidates q in row-major order.  SC: the scale at compile time (2, 3, 4; 0 = run time), as k_gather_direct.
template <typename T, int SC>
__global__ __launch_bounds__(256) void k_gather_affine(const T* __restrict__ resid, T* __restrict__ gout, Geometry g,
                                                      const double* __restrict__ recs, const T* __restrict__ blur_t,
                                                      int k0, int nk, T out_scale, int accumulate) {
  const int gs = SC ? SC : g.s;
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const int N = g.W * g.H, n = g.w * g.h;
  if (hp >= N) return;
  const int r = hp / g.W, col = hp - r * g.W;
  T acc = T(0);
  for (int kk = 0; kk < nk; ++kk) {
    const double* __restrict__ m = recs + (size_t)(k0 + kk) * kAffineRec;  // uniform: scalar loads
    const T* rk = resid + ((size_t)kk * g.C + c) * n;
    // F_k(p) and the first candidate of each axis; clamped ahead of the conversion (a far translation: no candidate)
    const double cx = affine_coord(m[6], m[7], m[8], (double)col, (double)r);
    const double cy = affine_coord(m[9], m[10], m[11], (double)col, (double)r);
    const double lx = __builtin_ceil(cx - m[12]), ly = __builtin_ceil(cy - m[13]);
    if (!(lx > -4.0 && lx < (double)g.W && ly > -4.0 && ly < (double)g.H)) continue;
    const int qx0 = (int)lx, qy0 = (int)ly;
    T tk = T(0);
    for (int dy = 0; dy < 3; ++dy) {
      const int qy = qy0 + dy;
      if (qy < 0 || qy >= g.H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int qx = qx0 + dx;
        if (qx < 0 || qx >= g.W) continue;
        double sx, sy;
        affine_source(m, qx, qy, &sx, &sy);
        const double wd = affine_axis_weight(sy, r) * affine_axis_weight(sx, col);
        if (wd == 0.0) continue;  // p is no tap of q
        tk += (T)wd * blur_t_upsampled_at(rk, blur_t, g, gs, qy, qx);
      }
    }
    acc += tk;
  }
  const size_t o = (size_t)c * N + hp;
  const T base = accumulate ? gout[o] : T(0);
  gout[o] = base + out_scale * acc;
}

template <typename T>
int launch_gather_affine(srmap_problem* p, const Geometry& geo, const T* resid, T* g, int k0, int nk, double out_scale,
                         bool accumulate, hipStream_t st) {
  if (!p->affine || !p->d_affine) return set_error(p->ctx, SRMAP_EINVAL, "internal: no affine motion set");
  dim3 grid((unsigned)(((size_t)geo.W * geo.H + 255) / 256), geo.C);
  const T* bt = (const T*)p->d_blur_t;
  const int acc1 = accumulate ? 1 : 0;
#define SRMAP_GATHER_AFFINE(SS) \
  hipLaunchKernelGGL((k_gather_affine<T, SS>), grid, dim3(256), 0, st, resid, g, geo, p->d_affine, bt, k0, nk, (T)out_scale, acc1)
  if (geo.s == 2) SRMAP_GATHER_AFFINE(2);
  else if (geo.s == 3) SRMAP_GATHER_AFFINE(3);
  else if (geo.s == 4) SRMAP_GATHER_AFFINE(4);
  else SRMAP_GATHER_AFFINE(0);
#undef SRMAP_GATHER_AFFINE
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// Validate K 2x3 matrices and fill the per-frame records (inverse in double, formed once here).
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

#define INSTANTIATE_AFFINE(T)                                                                                            \
  template int launch_forward_affine<T>(srmap_problem*, const Geometry&, const T*, const T*, int, int, T*, int, int,    \
                                        double*, int*, hipStream_t, const T*);                                           \
  template int launch_gather_affine<T>(srmap_problem*, const Geometry&, const T*, T*, int, int, double, bool, hipStream_t);
INSTANTIATE_AFFINE(float)
INSTANTIATE_AFFINE(double)

}  // namespace srmap
