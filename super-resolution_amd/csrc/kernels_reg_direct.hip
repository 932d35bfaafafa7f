// kernels_reg_direct.hip -- the regularisers' straightforward gfx950 kernels (TV, 3-D TV, BTV): values, IRLS weights and
// the gradient given the values or, for the TV kinds, in one pass.  They serve
//   (a) the operator entry points (srmap_reg_values, srmap_reg_values_and_gradient), the IRLS weight pass of the solve, and
//   (b) the fallback of srmap_eval when the tile kernels (kernels_ztile.hip) do not cover the geometry, and their
//       cross-check.
// tests/reg_matrix.py mirrors the launchers' dispatch rules.
//
// Math: SURVEY.md section 8(a'); reference lines are cited per kernel.
#include <climits>
#include <cstdint>

#include "reduce_dev.hpp"
#include "reg_gradient_host.hpp"
#include "srmap_internal.hpp"

namespace srmap {

// ---------------------------------------------------------------------------
// Regularizer values: TotalVariationRegularizer::ApplyToImage
// (tv_regularizer.cpp:110-132, helpers :21-106) and
// BilateralTotalVariationRegularizer::ApplyToImage (btv_regularizer.cpp:19-46,
// :67-90).
struct PowTable {
  double v[2 * kMaxBtvRange + 1];
};
static_assert(std::is_trivially_copyable_v<PowTable>, "a kernel argument: no owner inside");

template <typename T>
__device__ __forceinline__ T absval(T v) { return v < T(0) ? -v : v; }

// the IRLS weight of a residual value: 1 / max(1e-5, v) (irls_map_solver.cpp:128-143, kMinResidualValue :35)
template <typename T>
__device__ __forceinline__ T irls_weight(T v) {
  const T m = v > (T)0.00001 ? v : (T)0.00001;
  return T(1) / m;
}

template <typename T>
__device__ __forceinline__ T reg_value_at(const T* __restrict__ x, int W, int H, int C,
                                          int c, int r, int col, int kind, int range,
                                          const PowTable& pw, int zhi = 0) {
  const size_t N = (size_t)W * H;
  const T* plane = x + (size_t)c * N;
  const T x0 = plane[(size_t)r * W + col];
  if (kind == SRMAP_REG_BTV) {
    T tv = T(0);
    for (int i = 0; i <= range; ++i) {
      const int rr = r + i;
      if (rr >= H) continue;
      for (int j = 0; j <= range; ++j) {
        const int cc = col + j;
        if (cc >= W) continue;
        tv += (T)pw.v[i + j] * absval(x0 - plane[(size_t)rr * W + cc]);
      }
    }
    return tv;
  }
  const T yv = (r + 1 < H) ? absval(plane[(size_t)(r + 1) * W + col] - x0) : T(0);
  const T xv = (col + 1 < W) ? absval(plane[(size_t)r * W + col + 1] - x0) : T(0);
  T tv = yv + xv;
  if (kind == SRMAP_REG_TV3D && (c + 1 < C || zhi)) tv += absval(plane[N + (size_t)r * W + col] - x0);
  return tv;
}

template <typename T>
__global__ __launch_bounds__(256) void k_reg_values(const T* __restrict__ x,
                                                   T* __restrict__ values, int W, int H,
                                                   int C, int kind, int range,
                                                   PowTable pw, int zhi, int as_weights) {
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (hp >= W * H) return;
  const int r = hp / W, col = hp - r * W;
  T v = reg_value_at(x, W, H, C, c, r, col, kind, range, pw, zhi);
  if (as_weights) v = irls_weight(v);  // in the same pass
  values[(size_t)c * W * H + hp] = v;
}

// BTV values (and IRLS weights) with FOUR consecutive pixels per thread: the (R + 1) x (R + 4) window of a thread comes as
// two 4-element vectors per row instead of (R + 1)^2 scalar loads per pixel (k_reg_values: 50 us per 2048^2 plane, 3 x per
// cfg2 solve).  Same taps in the same (i outer, j inner) order per pixel, skipped taps as exact zeros: bit-identical.
// Requires W % 4 == 0 and range R <= 3.
template <typename T, int R>
__global__ __launch_bounds__(256) void k_btv_values4(const T* __restrict__ x, T* __restrict__ values, int W, int H,
                                                    PowTable pw, int as_weights) {
  const int W4 = W >> 2;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (cell >= W4 * H) return;
  const int r = cell / W4, c0 = (cell - r * W4) * 4;
  const T* plane = x + (size_t)c * W * H;
  const bool nin = c0 + 4 < W;  // the next cell of the row exists
  T tv[4] = {T(0), T(0), T(0), T(0)}, x0[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
  for (int i = 0; i <= R; ++i) {
    const int rr = r + i;
    const bool rin = rr < H;
    const T* row = plane + (size_t)(rin ? rr : r) * W + c0;
    T a[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = row[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[4 + q] = row[nin ? 4 + q : q];
    if (i == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) x0[q] = a[q];
    }
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
#pragma unroll
      for (int j = 0; j <= R; ++j) {
        const bool in = rin && (pc + j < 4 || nin);
        const T d = in ? x0[pc] - a[pc + j] : T(0);
        tv[pc] += (T)pw.v[i + j] * absval(d);
      }
    }
  }
  T* out = values + (size_t)c * W * H + (size_t)r * W + c0;
#pragma unroll
  for (int pc = 0; pc < 4; ++pc) {
    T v = tv[pc];
    if (as_weights) v = irls_weight(v);
    out[pc] = v;
  }
}

// The same with a thread walking DOWN a strip of RS rows: the window's R + 1 rows stay in registers and every output
// row requests ONE new row (two 4-element vectors) instead of R + 1 -- (RS + R) / RS rows read per row written instead
// of R + 1, a quarter of the memory instructions at R = 3.  Per pixel the same taps in the same order with the same
// zeros for the skipped ones as k_btv_values4: bit-identical (tests/test_gpu_reg_kernels.py asserts it).
constexpr int kBtvStripRows = 4;  // RS of the solve's pass (tests/reg_matrix.py mirrors it as STRIP_ROWS)
__device__ __forceinline__ float fabs_mod(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double fabs_mod(double v) { return __builtin_fabs(v); }
// BORDER = false: the strip's windows stay inside the image (no per-tap masks: two f64 issues per tap instead of four).
template <typename T, int R, int RS, bool BORDER>
__device__ __forceinline__ void btv_strip_rows(const T* __restrict__ plane, T* __restrict__ oplane, int W, int H, int r0,
                                               int c0, bool nin, const PowTable& pw, int as_weights) {
  T win[R + 1][8];  // window rows r .. r + R of the row being written (rotating: row q lives in win[q % (R + 1)])
#pragma unroll
  for (int q = 0; q < RS + R; ++q) {
    // row r0 + q enters the window (rows below the image: a valid address, never used -- see `rin` below)
    {
      const int rr = r0 + q;
      const T* row = plane + (size_t)((!BORDER || rr < H) ? rr : r0) * W + c0;
#pragma unroll
      for (int e = 0; e < 4; ++e) win[q % (R + 1)][e] = row[e];
#pragma unroll
      for (int e = 0; e < 4; ++e) win[q % (R + 1)][4 + e] = row[(!BORDER || nin) ? 4 + e : e];
    }
    if (q < R) continue;
    const int o = q - R, r = r0 + o;  // the output row whose window is complete now
    if (BORDER && r >= H) continue;
    T tv[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int i = 0; i <= R; ++i) {
      const bool rin = r + i < H;
#pragma unroll
      for (int pc = 0; pc < 4; ++pc) {
#pragma unroll
        for (int j = 0; j <= R; ++j) {
          T d = win[o % (R + 1)][pc] - win[(o + i) % (R + 1)][pc + j];
          if (BORDER) d = (rin && (pc + j < 4 || nin)) ? d : T(0);
          // |d| as the FMA's source modifier (absval's compare + select cost three more issues per tap).  The two differ
          // for d = -0 only, and a -0 product leaves the sum -- which starts at +0 -- unchanged just like a +0 one.
          tv[pc] += (T)pw.v[i + j] * fabs_mod(d);
        }
      }
    }
    T* out = oplane + (size_t)r * W + c0;
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
      T v = tv[pc];
      if (as_weights) v = irls_weight(v);
      out[pc] = v;
    }
  }
}

template <typename T, int R, int RS>
__global__ __launch_bounds__(256) void k_btv_values_strip(const T* __restrict__ x, T* __restrict__ values, int W, int H,
                                                         PowTable pw, int as_weights) {
  const int W4 = W >> 2;
  const int nstrips = (H + RS - 1) / RS;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (cell >= W4 * nstrips) return;
  const int sidx = cell / W4, c0 = (cell - sidx * W4) * 4;
  const int r0 = sidx * RS;
  const T* plane = x + (size_t)c * W * H;
  T* oplane = values + (size_t)c * W * H;
  const bool nin = c0 + 4 < W;  // the next cell of the row exists
  // one path per wave: only the waves that hold a row's last cell or the image's last strips take the masked one
  if (__all(nin && r0 + RS + R <= H)) btv_strip_rows<T, R, RS, false>(plane, oplane, W, H, r0, c0, nin, pw, as_weights);
  else btv_strip_rows<T, R, RS, true>(plane, oplane, W, H, r0, c0, nin, pw, as_weights);
}

template <typename T>
static bool launch_btv_values4(const Geometry& g, const RegSpec& rs, const T* x, T* out, int as_weights, const PowTable& pw,
                               hipStream_t st) {
  if (rs.kind != SRMAP_REG_BTV || rs.range < 1 || rs.range > 3 || (g.W & 3) != 0) return false;
  if ((long long)g.W * g.H / 4 >= (long long)INT_MAX) return false;
  if (rs.range == 3 && g.H >= 4 * kBtvStripRows) {  // the solve's pass at cfg2
    constexpr int RS = kBtvStripRows;
    const long long cells = (long long)(g.W >> 2) * ((g.H + RS - 1) / RS);
    dim3 sgrid((unsigned)((cells + 255) / 256), g.C);
    hipLaunchKernelGGL((k_btv_values_strip<T, 3, RS>), sgrid, dim3(256), 0, st, x, out, g.W, g.H, pw, as_weights);
    return true;
  }
  dim3 grid((unsigned)(((long long)(g.W >> 2) * g.H + 255) / 256), g.C);
  if (rs.range == 1) hipLaunchKernelGGL((k_btv_values4<T, 1>), grid, dim3(256), 0, st, x, out, g.W, g.H, pw, as_weights);
  else if (rs.range == 2) hipLaunchKernelGGL((k_btv_values4<T, 2>), grid, dim3(256), 0, st, x, out, g.W, g.H, pw, as_weights);
  else hipLaunchKernelGGL((k_btv_values4<T, 3>), grid, dim3(256), 0, st, x, out, g.W, g.H, pw, as_weights);
  return true;
}

static PowTable make_pow(const RegSpec& rs) {
  PowTable t;
  for (int i = 0; i < 2 * kMaxBtvRange + 1; ++i) t.v[i] = rs.pow_table[i];
  return t;
}

// the values (as_weights = 0) or, in the same single pass over x, the IRLS weights of irls_map_solver.cpp:128-143
template <typename T>
static int launch_reg_values_as(srmap_problem* p, const Geometry& g, const RegSpec& rs, const T* x, T* out, int as_weights,
                                hipStream_t st) {
  dim3 grid((g.W * g.H + 255) / 256, g.C);
  if (!launch_btv_values4<T>(g, rs, x, out, as_weights, make_pow(rs), st))
    hipLaunchKernelGGL(k_reg_values<T>, grid, dim3(256), 0, st, x, out, g.W, g.H, g.C,
                       rs.kind, rs.range, make_pow(rs), g.zhi, as_weights);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

template <typename T>
int launch_reg_values(srmap_problem* p, const Geometry& g, const RegSpec& rs, const T* x, T* values, hipStream_t st) {
  return launch_reg_values_as<T>(p, g, rs, x, values, 0, st);
}

template <typename T>
int launch_reg_weights(srmap_problem* p, const Geometry& g, const RegSpec& rs, const T* x, T* weights, hipStream_t st) {
  return launch_reg_values_as<T>(p, g, rs, x, weights, 1, st);
}

// ---------------------------------------------------------------------------
// Regularizer gradient given the values (tv_regularizer.cpp:143-224,
// btv_regularizer.cpp:105-166), bug-compatible: 3-D TV has no z self term; BTV
// uses the exclusive window and skips the absolute pixel (0,0) as a source.
// Constants c[q] = gc_scale * gc[q] (gc == nullptr means 1).
// Exact (srmap_problem_set_regularizer_gradient): the gradient of the cost with c held fixed instead -- BTV over the
// inclusive window with every pixel a source, 3-D TV with its -sgn dz self term.  A compile-time leg: the reference
// instances are the code they were (profiles/r31_reg_exact_resources.txt).
template <typename T>
__device__ __forceinline__ T sgn(T d) { return d > T(0) ? T(1) : (d < T(0) ? T(-1) : T(0)); }

template <typename T, bool Exact = false>
__global__ __launch_bounds__(256) void k_reg_gradient_direct(
    const T* __restrict__ x, const T* __restrict__ gc, T gc_scale,
    const T* __restrict__ values, T* __restrict__ gout, int accumulate,
    double* __restrict__ partials, int W, int H, int C, int kind, int range,
    PowTable pw, int cr0, int cr1) {
  __shared__ double red[4];
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const size_t N = (size_t)W * H;
  double cost = 0.0;
  if (hp < W * H) {
    const int r = hp / W, col = hp - r * W;
    const T* plane = x + (size_t)c * N;
    const T* vals = values + (size_t)c * N;
    const T* gcp = gc ? gc + (size_t)c * N : nullptr;
    const size_t idx = (size_t)r * W + col;
    const T x0 = plane[idx];
    const T wt0 = gcp ? gcp[idx] : T(1);
    const T c0 = gc_scale * wt0;
    // values == nullptr (TV kinds only): the residual values are recomputed where they are needed -- the
    // k_reg_values pass and its C*N array round trip disappear (TV is 2-3 differences per value)
    const bool onfly = values == nullptr;
    const T r0 = onfly ? reg_value_at(x, W, H, C, c, r, col, kind, range, pw) : vals[idx];
    T grad = T(0);
    if (kind == SRMAP_REG_BTV) {
      const int wend = Exact ? range + 1 : range;  // the window differentiated: [0, R] or the reference's [0, R - 1]
      T didi = T(0);
      for (int i = 0; i < wend; ++i) {
        const int rr = r + i;
        if (rr >= H) continue;
        for (int j = 0; j < wend; ++j) {
          const int cc = col + j;
          if (cc >= W) continue;
          didi += (T)pw.v[i + j] * sgn(x0 - plane[(size_t)rr * W + cc]);
        }
      }
      grad += T(2) * c0 * r0 * didi;
      for (int i = 0; i < wend; ++i) {
        const int rr = r - i;
        if (rr < 0) continue;
        for (int j = 0; j < wend; ++j) {
          const int cc = col - j;
          if (cc < 0 || (Exact ? (i == 0 && j == 0) : (rr == 0 && cc == 0))) continue;
          const size_t q = (size_t)rr * W + cc;
          const T cq = gc_scale * (gcp ? gcp[q] : T(1));
          const T didj = -sgn(plane[q] - x0) * (T)pw.v[i + j];
          grad += T(2) * cq * vals[q] * didj;
        }
      }
    } else {
      T didi = T(0);
      if (col + 1 < W) didi -= sgn(plane[idx + 1] - x0);
      if (r + 1 < H) didi -= sgn(plane[idx + W] - x0);
      if (Exact && kind == SRMAP_REG_TV3D && c + 1 < C) didi -= sgn(plane[idx + N] - x0);
      grad += T(2) * c0 * r0 * didi;
      if (col - 1 >= 0) {
        const size_t q = idx - 1;
        const T cq = gc_scale * (gcp ? gcp[q] : T(1));
        grad += T(2) * cq * (onfly ? reg_value_at(x, W, H, C, c, r, col - 1, kind, range, pw) : vals[q]) * sgn(x0 - plane[q]);
      }
      if (r - 1 >= 0) {
        const size_t q = idx - W;
        const T cq = gc_scale * (gcp ? gcp[q] : T(1));
        grad += T(2) * cq * (onfly ? reg_value_at(x, W, H, C, c, r - 1, col, kind, range, pw) : vals[q]) * sgn(x0 - plane[q]);
      }
      if (kind == SRMAP_REG_TV3D && c > 0) {
        const T xb = plane[idx - N];
        const T cq = gc_scale * (gcp ? gcp[idx - N] : T(1));
        grad += T(2) * cq * (onfly ? reg_value_at(x, W, H, C, c - 1, r, col, kind, range, pw) : vals[idx - N]) * sgn(x0 - xb);
      }
    }
    const size_t o = (size_t)c * N + idx;
    if (gout) gout[o] = (accumulate ? gout[o] : T(0)) + grad;
    // lambda * w * r^2  (objective_irls_regularization_term.cpp:45-50)
    cost = (r >= cr0 && r < cr1) ? (double)c0 * (double)r0 * (double)r0 : 0.0;
  }
  if (partials) {
    const double s = block_sum_256(cost, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// The arithmetic of one pixel of TV / 3-D TV, once for the two kernels below (tests/test_gpu_reg_kernels.py asserts that
// they agree bit for bit): the same expressions, in the same order, as reg_value_at + the TV branch of
// k_reg_gradient_direct.  tv_value: the residual value of a pixel v from its down, right and next-channel neighbours.
template <typename T>
__device__ __forceinline__ T tv_value(const T& v, const T& d, const T& r, const T& n, bool down, bool right, bool has_next) {
  const T yv = down ? absval(d - v) : T(0);
  const T xv = right ? absval(r - v) : T(0);
  T tv = yv + xv;
  if (has_next) tv += absval(n - v);
  return tv;
}

// tv_pixel: the gradient at the pixel x0 (returned) and its value (*r0).  x0 comes with its right, down and next-channel
// neighbours and its constant c0 = gc_scale * weight; the left (l), upper (u) and previous-channel (p) neighbours each with
// the down / right / next-channel neighbours of THEIR value that are not x0 itself, and their weight; then which of the six
// neighbours exist.  What does not exist is not read (the arguments are references).  ExactZ: the self term has its
// -sgn dz (the exact 3-D TV gradient); without it the reference's.
template <typename T, bool ExactZ = false>
__device__ __forceinline__ T tv_pixel(const T& x0, const T& xr, const T& xd, const T& xn, T c0, T gc_scale,
                                      const T& l, const T& ld, const T& ln, const T& wl,
                                      const T& u, const T& ur, const T& un, const T& wu,
                                      const T& p, const T& pd, const T& pr, const T& wp,
                                      bool right, bool down, bool has_next, bool left, bool up, bool has_prev, T* r0) {
  const T val = tv_value(x0, xd, xr, xn, down, right, has_next);
  *r0 = val;
  T grad = T(0);
  T didi = T(0);
  if (right) didi -= sgn(xr - x0);
  if (down) didi -= sgn(xd - x0);
  if (ExactZ && has_next) didi -= sgn(xn - x0);
  grad += T(2) * c0 * val * didi;  // reference: 3-D TV has no z self term (tv_regularizer.cpp:154-170)
  // the neighbour's own value has x0 as its right / down / next-channel neighbour, which always exists
  if (left) grad += T(2) * (gc_scale * wl) * tv_value(l, ld, x0, ln, down, true, has_next) * sgn(x0 - l);
  if (up) grad += T(2) * (gc_scale * wu) * tv_value(u, x0, ur, un, true, right, has_next) * sgn(x0 - u);
  if (has_prev) grad += T(2) * (gc_scale * wp) * tv_value(p, pd, pr, x0, down, right, true) * sgn(x0 - p);
  return grad;
}

// TV / 3-D TV in ONE pass (tv_regularizer.cpp:110-227): value, gradient and cost per pixel with the values of
// the left / upper / previous-channel neighbours recomputed on the spot (2-3 differences each) -- no values
// array, no integer division.  A thread owns 4 consecutive pixels of a row (block = 256 columns x 4 rows) and
// loads the row segments it needs once: rows r-1, r, r+1 of its plane, and for 3-D TV rows of the next and the
// previous channel; the arithmetic is tv_pixel.
template <typename T, bool D3, bool ExactZ = false>
__global__ __launch_bounds__(256) void k_tv_onepass(const T* __restrict__ x, const T* __restrict__ gc, T gc_scale,
                                                    T* __restrict__ gout, int accumulate,
                                                    double* __restrict__ partials, int W, int H, int C, int cr0,
                                                    int cr1, int zlo, int zhi) {
  __shared__ double red[4];
  constexpr int P = 4;
  const int c0 = (blockIdx.x * 64 + threadIdx.x) * P, r = blockIdx.y * 4 + threadIdx.y, c = blockIdx.z;
  const size_t N = (size_t)W * H;
  double cost = 0.0;
  if (c0 < W && r < H) {
    const T* plane = x + (size_t)c * N;
    const T* gcp = gc ? gc + (size_t)c * N : nullptr;
    // n values of row rr starting at column cs; positions outside the image read as 0 (never used unmasked)
    auto row = [&](const T* pl, int rr, int cs, int n, T* dst, T fill) {
      const bool rin = (unsigned)rr < (unsigned)H;
      const T* src = pl + (rin ? (size_t)rr * W : (size_t)0);
#pragma unroll
      for (int k = 0; k < P + 2; ++k)
        if (k < n) { const int cc = cs + k; dst[k] = (rin && (unsigned)cc < (unsigned)W) ? src[cc] : fill; }
    };
    T xc[P + 2], xd[P + 2], xu[P + 2], xn[P + 2], xnu[P + 2], xp[P + 2], xpd[P + 2], wc[P + 2], wu[P + 2], wp[P + 2];
    T gold[P];
#pragma unroll
    for (int i = 0; i < P; ++i) gold[i] = T(0);
    const bool has_next = D3 && (c + 1 < C || zhi), has_prev = D3 && (c > 0 || zlo);
    T* gdst = gout ? gout + (size_t)c * N + (size_t)r * W + c0 : nullptr;
    // rows r-1 .. r+1 inside the image and whole 4-pixel cells: every segment is one unconditional 4-vector plus
    // at most one clamped neighbour element, all requested before the first use (wave-uniform branch; the masked
    // element-wise form below made every load wait for the one before it)
    const bool fast = (W & 3) == 0 && r >= 1 && r + 1 < H;
    if (fast) {
      const int cl = c0 > 0 ? c0 - 1 : 0, cr = c0 + P < W ? c0 + P : W - 1;
      const size_t o0 = (size_t)r * W, od = o0 + W, ou = o0 - W;
      auto vec = [&](const T* src, T* dst) {
#pragma unroll
        for (int k = 0; k < P; ++k) dst[k] = src[k];
      };
      vec(plane + o0 + c0, xc + 1); xc[0] = plane[o0 + cl]; xc[P + 1] = plane[o0 + cr];
      vec(plane + od + c0, xd + 1); xd[0] = plane[od + cl];
      vec(plane + ou + c0, xu); xu[P] = plane[ou + cr];
      if (has_next) { vec(plane + N + o0 + c0, xn + 1); xn[0] = plane[N + o0 + cl]; vec(plane + N + ou + c0, xnu); }
      if (has_prev) { vec(plane - N + o0 + c0, xp); xp[P] = plane[o0 + cr - N]; vec(plane - N + od + c0, xpd); }
      if (gcp) {
        vec(gcp + o0 + c0, wc + 1); wc[0] = gcp[o0 + cl];
        vec(gcp + ou + c0, wu);
        if (has_prev) vec(gcp - N + o0 + c0, wp);
      }
      if (gdst && accumulate) vec(gdst, gold);
    } else {
      row(plane, r, c0 - 1, P + 2, xc, T(0));      // columns c0-1 .. c0+4
      row(plane, r + 1, c0 - 1, P + 1, xd, T(0));  // c0-1 .. c0+3
      row(plane, r - 1, c0, P + 1, xu, T(0));      // c0 .. c0+4
      if (has_next) { row(plane + N, r, c0 - 1, P + 1, xn, T(0)); row(plane + N, r - 1, c0, P, xnu, T(0)); }
      if (has_prev) { row(plane - N, r, c0, P + 1, xp, T(0)); row(plane - N, r + 1, c0, P, xpd, T(0)); }
      if (gcp) {
        row(gcp, r, c0 - 1, P + 1, wc, T(1));
        row(gcp, r - 1, c0, P, wu, T(1));
        if (has_prev) row(gcp - N, r, c0, P, wp, T(1));
      }
      if (gdst && accumulate) {
#pragma unroll
        for (int i = 0; i < P; ++i) if (c0 + i < W) gold[i] = gdst[i];
      }
    }
    const bool down = r + 1 < H;
    const T one = T(1);  // the weight where there are none
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int col = c0 + i;
      if (col < W) {
        const T cc0 = gc_scale * (gcp ? wc[i + 1] : one);
        T r0;
        const T grad = tv_pixel<T, ExactZ>(xc[i + 1], xc[i + 2], xd[i + 1], xn[i + 1], cc0, gc_scale,
                                   xc[i], xd[i], xn[i], gcp ? wc[i] : one,
                                   xu[i], xu[i + 1], xnu[i], gcp ? wu[i] : one,
                                   xp[i], xpd[i], xp[i + 1], gcp ? wp[i] : one,
                                   col + 1 < W, down, has_next, col - 1 >= 0, r - 1 >= 0, has_prev, &r0);
        if (gdst) gdst[i] = gold[i] + grad;
        // lambda * w * r^2  (objective_irls_regularization_term.cpp:45-50)
        cost += (r >= cr0 && r < cr1) ? (double)cc0 * (double)r0 * (double)r0 : 0.0;
      }
    }
  }
  if (partials) {  // (64, 4) block: wave = threadIdx.y
    const double ws = wave_sum(cost);
    if (threadIdx.x == 0) red[threadIdx.y] = ws;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
      partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// 3-D TV marching along the CHANNEL axis (tv_regularizer.cpp:110-227, the z terms :154-170 and :205-222).
// k_tv_onepass gives every (pixel, channel) its own thread, so each plane is fetched three times (as the current,
// the next and the previous channel) one whole plane of blocks apart -- from the Infinity Cache at best.  Here a
// thread keeps its 4 pixels and walks a chunk of channels with the planes c-1, c, c+1 (rows r-1, r, r+1 of each)
// in registers: per step it requests plane c+1, the weights and the old gradient of c -- all unconditional
// (out-of-range planes are clamped to a valid one and never used), one wait, then the arithmetic; other waves
// cover the wait.  Every plane, weight and gradient element crosses the fabric once per chunk.  The three plane
// sets rotate with compile-time indices (loop unrolled by 3).  The arithmetic is tv_pixel, as in k_tv_onepass.
template <typename T> struct TvPlane { T m[6], d[5], u[5]; };  // row r: c0-1..c0+4, row r+1: c0-1..c0+3, row r-1: c0..c0+4

template <typename T>
__device__ __forceinline__ void tv_load4(const T* __restrict__ src, T* dst) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  const V4 v = *reinterpret_cast<const V4*>(src);
  dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
}

template <typename T>
__device__ __forceinline__ void tv_load_plane(const T* __restrict__ pl, size_t o0, size_t od, size_t ou, int c0, int cl,
                                              int cr, TvPlane<T>& R) {
  tv_load4(pl + o0 + c0, R.m + 1); R.m[0] = pl[o0 + cl]; R.m[5] = pl[o0 + cr];
  tv_load4(pl + od + c0, R.d + 1); R.d[0] = pl[od + cl];
  tv_load4(pl + ou + c0, R.u); R.u[4] = pl[ou + cr];
}

template <typename T, bool ExactZ = false>
__global__ __launch_bounds__(256) void k_tv3d_march(const T* __restrict__ x, const T* __restrict__ gc, T gc_scale,
                                                    T* __restrict__ gout, int accumulate,
                                                    double* __restrict__ partials, int W, int H, int C, int cr0,
                                                    int cr1, int zlo, int zhi, int chunk) {
  __shared__ double red[4];
  constexpr int P = 4;
  const int c0 = (blockIdx.x * 64 + threadIdx.x) * P, r = blockIdx.y * 4 + threadIdx.y;
  const int cbeg = blockIdx.z * chunk, cend = (cbeg + chunk < C) ? cbeg + chunk : C;
  const ptrdiff_t N = (ptrdiff_t)W * H;
  double cost = 0.0;
  if (c0 < W && r < H) {  // W % 4 == 0: whole cells
    const bool up = r >= 1, down = r + 1 < H;
    const int cl = c0 >= 1 ? c0 - 1 : 0, cr = c0 + P < W ? c0 + P : W - 1;
    const size_t o0 = (size_t)r * W, od = o0 + (down ? W : 0), ou = o0 - (up ? W : 0);
    const bool cost_row = r >= cr0 && r < cr1;
    const int plo = zlo ? -1 : 0, phi = zhi ? C : C - 1;  // planes that exist
    auto clampc = [&](int c) { return c < plo ? plo : (c > phi ? phi : c); };
    TvPlane<T> R[3];
    T wprev[P];
    tv_load_plane(x + clampc(cbeg - 1) * N, o0, od, ou, c0, cl, cr, R[2]);
    tv_load_plane(x + cbeg * N, o0, od, ou, c0, cl, cr, R[0]);
#pragma unroll
    for (int i = 0; i < P; ++i) wprev[i] = T(1);
    if (gc) tv_load4(gc + clampc(cbeg - 1) * N + o0 + c0, wprev);
    for (int cb = cbeg; cb < cend; cb += 3) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int c = cb + k;
        if (c < cend) {  // uniform
          const TvPlane<T>& Rc = R[k];
          TvPlane<T>& Rn = R[(k + 1) % 3];
          const TvPlane<T>& Rp = R[(k + 2) % 3];
          tv_load_plane(x + clampc(c + 1) * N, o0, od, ou, c0, cl, cr, Rn);
          T wc[P + 1], wu[P], gold[P];
#pragma unroll
          for (int i = 0; i < P; ++i) { wc[i] = T(1); wu[i] = T(1); gold[i] = T(0); }
          wc[P] = T(1);
          if (gc) {
            const T* g0 = gc + c * N;
            tv_load4(g0 + o0 + c0, wc + 1); wc[0] = g0[o0 + cl];
            tv_load4(g0 + ou + c0, wu);
          }
          if (gout && accumulate) tv_load4(gout + c * N + o0 + c0, gold);
          const bool has_next = (c + 1 < C || zhi), has_prev = (c > 0 || zlo);
          T gnew[P];
#pragma unroll
          for (int i = 0; i < P; ++i) {
            const int col = c0 + i;
            const T cc0 = gc_scale * wc[i + 1];
            T r0;
            const T grad = tv_pixel<T, ExactZ>(Rc.m[i + 1], Rc.m[i + 2], Rc.d[i + 1], Rn.m[i + 1], cc0, gc_scale,
                                       Rc.m[i], Rc.d[i], Rn.m[i], wc[i],
                                       Rc.u[i], Rc.u[i + 1], Rn.u[i], wu[i],
                                       Rp.m[i + 1], Rp.d[i + 1], Rp.m[i + 2], wprev[i],
                                       col + 1 < W, down, has_next, col - 1 >= 0, up, has_prev, &r0);
            gnew[i] = gold[i] + grad;
            cost += cost_row ? (double)cc0 * (double)r0 * (double)r0 : 0.0;
          }
          if (gout) {
            typedef T V4 __attribute__((ext_vector_type(4)));
            V4 v; v.x = gnew[0]; v.y = gnew[1]; v.z = gnew[2]; v.w = gnew[3];
            *reinterpret_cast<V4*>(gout + c * N + o0 + c0) = v;
          }
#pragma unroll
          for (int i = 0; i < P; ++i) wprev[i] = wc[i + 1];
        }
      }
    }
  }
  if (partials) {  // (64, 4) block: wave = threadIdx.y
    const double ws = wave_sum(cost);
    if (threadIdx.x == 0) red[threadIdx.y] = ws;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
      partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// The EXACT BTV gradient given the values, FOUR consecutive pixels per thread in gather form (the Exact leg of
// k_reg_gradient_direct asks for 2 (R + 1)^2 scalar x loads, (R + 1)^2 value and weight loads and an integer division per
// pixel).  A pixel p gathers
//   its own term      2 c[p] r[p] sum_{i,j in [0,R]} a^(i+j) sgn(x[p] - x[p + (i,j)])          rows r .. r + R, this cell and the next
//   its sources' terms  - sum_{(i,j) != (0,0)} 2 c[q] r[q] a^(i+j) sgn(x[q] - x[p]), q = p - (i,j)   rows r - R .. r, the previous cell and this
// so a thread requests every row of its window as two 4-element vectors (row r: three) of x, and for the source rows two
// each of the values and the weights, and forms m[q] = 2 c[q] r[q] once per element loaded -- the values come from the
// evaluation's values pass, never recomputed: a pixel has (R + 1)^2 - 1 sources of (R + 1)^2 taps each.  Per pixel the
// same terms in the same (i outer, j inner) order as the generic leg, masked taps as exact zeros.  No atomics, no LDS but
// the cost reduction's four words: results are bit-identical run to run.  Requires W % 4 == 0, R <= 3 and arrays aligned
// to four elements.  BORDER = false: the whole window lies inside the image and both neighbour cells exist (no masks, no
// clamped addresses).
template <typename T, int R, bool BORDER>
__device__ __forceinline__ double btv_exact_cell(const T* __restrict__ plane, const T* __restrict__ vals,
                                                 const T* __restrict__ gcp, T gc_scale, int W, int H, int r, int c0,
                                                 const PowTable& pw, T (&grad)[4]) {
  const bool pin = !BORDER || c0 >= 4, nin = !BORDER || c0 + 4 < W;  // the previous / next cell of the row exists
  const size_t o0 = (size_t)r * W + c0;
  const int dp = pin ? 4 : 0, dn = nin ? 4 : 0;  // a missing cell: a valid address, never used unmasked
  T pwt[2 * R + 1];
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) pwt[k] = (T)pw.v[k];
  T xr[12];  // row r: the previous cell, this one, the next
  tv_load4(plane + o0 - dp, xr);
  tv_load4(plane + o0, xr + 4);
  tv_load4(plane + o0 + dn, xr + 8);
  T didi[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
  for (int i = 0; i <= R; ++i) {  // the own term: rows r .. r + R
    const bool rin = !BORDER || r + i < H;
    T a[8];
    if (i == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = xr[4 + e];
    } else {
      const T* row = plane + o0 + (rin ? (size_t)i * W : (size_t)0);
      tv_load4(row, a);
      tv_load4(row + dn, a + 4);
    }
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
#pragma unroll
      for (int j = 0; j <= R; ++j) {
        T s = sgn(xr[4 + pc] - a[pc + j]);
        if (BORDER) s = (rin && (pc + j < 4 || nin)) ? s : T(0);
        didi[pc] += pwt[i + j] * s;
      }
    }
  }
  double cost = 0.0;
#pragma unroll
  for (int i = 0; i <= R; ++i) {  // the sources' terms: rows r .. r - R
    const bool rin = !BORDER || r - i >= 0;
    const size_t o = o0 - (rin ? (size_t)i * W : (size_t)0);
    T b[8], v[8], w[8];
    if (i == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = xr[e];
    } else {
      tv_load4(plane + o - dp, b);
      tv_load4(plane + o, b + 4);
    }
    tv_load4(vals + o - dp, v);
    tv_load4(vals + o, v + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = T(1);
    if (gcp) {
      tv_load4(gcp + o - dp, w);
      tv_load4(gcp + o, w + 4);
    }
    T m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = T(2) * (gc_scale * w[e]) * v[e];
    if (i == 0) {
#pragma unroll
      for (int pc = 0; pc < 4; ++pc) {
        grad[pc] = m[4 + pc] * didi[pc];
        // lambda * w * r^2  (objective_irls_regularization_term.cpp:45-50)
        cost += (double)(gc_scale * w[4 + pc]) * (double)v[4 + pc] * (double)v[4 + pc];
      }
    }
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
#pragma unroll
      for (int j = 0; j <= R; ++j) {
        if (i == 0 && j == 0) continue;
        const int e = 4 + pc - j;
        T t = -sgn(b[e] - xr[4 + pc]) * pwt[i + j];
        if (BORDER) t = (rin && (e >= 4 || pin)) ? t : T(0);
        grad[pc] += m[e] * t;
      }
    }
  }
  return cost;
}

template <typename T, int R>
__global__ __launch_bounds__(256) void k_btv_gradient_exact4(const T* __restrict__ x, const T* __restrict__ gc, T gc_scale,
                                                            const T* __restrict__ values, T* __restrict__ gout,
                                                            int accumulate, double* __restrict__ partials, int W, int H,
                                                            PowTable pw, int cr0, int cr1) {
  __shared__ double red[4];
  const int W4 = W >> 2;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const size_t N = (size_t)W * H;
  double cost = 0.0;
  if (cell < W4 * H) {
    const int r = cell / W4, c0 = (cell - r * W4) * 4;
    const T* plane = x + (size_t)c * N;
    const T* vals = values + (size_t)c * N;
    const T* gcp = gc ? gc + (size_t)c * N : nullptr;
    T grad[4];
    double cst;
    // one path per wave: only the waves that hold a row's first or last cell or one of the image's first / last R rows
    // take the masked one
    if (__all(c0 >= 4 && c0 + 4 < W && r >= R && r + R < H)) cst = btv_exact_cell<T, R, false>(plane, vals, gcp, gc_scale, W, H, r, c0, pw, grad);
    else cst = btv_exact_cell<T, R, true>(plane, vals, gcp, gc_scale, W, H, r, c0, pw, grad);
    if (gout) {
      T* gdst = gout + (size_t)c * N + (size_t)r * W + c0;
      T gold[4] = {T(0), T(0), T(0), T(0)};
      if (accumulate) tv_load4(gdst, gold);
      typedef T V4 __attribute__((ext_vector_type(4)));
      V4 o; o.x = gold[0] + grad[0]; o.y = gold[1] + grad[1]; o.z = gold[2] + grad[2]; o.w = gold[3] + grad[3];
      *reinterpret_cast<V4*>(gdst) = o;
    }
    cost = (r >= cr0 && r < cr1) ? cst : 0.0;
  }
  if (partials) {
    const double s = block_sum_256(cost, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// the launch where k_btv_gradient_exact4 serves the call (the rule: reg_gradient_host.hpp)
template <typename T>
static bool launch_btv_gradient_exact4(const Geometry& geo, const RegSpec& rs, const T* x, const T* gc, T gc_scale,
                                       const T* values, T* g, int accumulate, double* partials, int* nblocks,
                                       hipStream_t st) {
  if (!btv_exact4_serves(rs.range, geo.W, geo.H, sizeof(T), (uintptr_t)x, (uintptr_t)values, (uintptr_t)gc, (uintptr_t)g)) return false;
  dim3 grid((unsigned)(((long long)(geo.W >> 2) * geo.H + 255) / 256), geo.C);
  const PowTable pw = make_pow(rs);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, x, gc, gc_scale, values, g, accumulate, partials, geo.W, geo.H, pw,
                       geo.cr0, geo.cr1);
  };
  if (rs.range == 1) go(k_btv_gradient_exact4<T, 1>);
  else if (rs.range == 2) go(k_btv_gradient_exact4<T, 2>);
  else go(k_btv_gradient_exact4<T, 3>);
  if (nblocks) *nblocks = (int)(grid.x * grid.y);
  return true;
}

template <typename T>
int launch_reg_gradient_direct(srmap_problem* p, const Geometry& geo, const RegSpec& rs,
                               const T* x, const T* gc, double gc_scale, const T* values,
                               T* g, bool accumulate, double* partials, int* nblocks,
                               hipStream_t st) {
  const bool exact = rs.exact();
  if (values == nullptr && rs.kind != SRMAP_REG_BTV) {  // TV kinds, one pass
    dim3 grid2((geo.W + 255) / 256, (geo.H + 3) / 4, geo.C);
    const size_t valign = 4 * sizeof(T);
    if (rs.kind == SRMAP_REG_TV3D && geo.C >= 2 && (geo.W & 3) == 0 && ((uintptr_t)x % valign) == 0 &&
        (!gc || ((uintptr_t)gc % valign) == 0) && (!g || ((uintptr_t)g % valign) == 0)) {
      // channel march: chunks of channels per thread; enough chunks to fill the GPU at a few planes of overlap each
      const long long per_plane = (long long)grid2.x * grid2.y;
      int chunk = geo.C;
      while (chunk > 16 && per_plane * ((geo.C + chunk - 1) / chunk) < 4096) chunk = (chunk + 1) / 2;
      dim3 grid3(grid2.x, grid2.y, (geo.C + chunk - 1) / chunk);
      if (exact)
        hipLaunchKernelGGL((k_tv3d_march<T, true>), grid3, dim3(64, 4), 0, st, x, gc, (T)gc_scale, g, accumulate ? 1 : 0, partials,
                           geo.W, geo.H, geo.C, geo.cr0, geo.cr1, geo.zlo, geo.zhi, chunk);
      else
        hipLaunchKernelGGL(k_tv3d_march<T>, grid3, dim3(64, 4), 0, st, x, gc, (T)gc_scale, g, accumulate ? 1 : 0, partials,
                           geo.W, geo.H, geo.C, geo.cr0, geo.cr1, geo.zlo, geo.zhi, chunk);
      if (nblocks) *nblocks = (int)(grid3.x * grid3.y * grid3.z);
      SRMAP_HIP(p->ctx, hipGetLastError());
      return SRMAP_OK;
    }
    if (rs.kind == SRMAP_REG_TV3D && exact)
      hipLaunchKernelGGL((k_tv_onepass<T, true, true>), grid2, dim3(64, 4), 0, st, x, gc, (T)gc_scale, g, accumulate ? 1 : 0,
                         partials, geo.W, geo.H, geo.C, geo.cr0, geo.cr1, geo.zlo, geo.zhi);
    else if (rs.kind == SRMAP_REG_TV3D)
      hipLaunchKernelGGL((k_tv_onepass<T, true>), grid2, dim3(64, 4), 0, st, x, gc, (T)gc_scale, g, accumulate ? 1 : 0,
                         partials, geo.W, geo.H, geo.C, geo.cr0, geo.cr1, geo.zlo, geo.zhi);
    else
      hipLaunchKernelGGL((k_tv_onepass<T, false>), grid2, dim3(64, 4), 0, st, x, gc, (T)gc_scale, g, accumulate ? 1 : 0,
                         partials, geo.W, geo.H, geo.C, geo.cr0, geo.cr1, 0, 0);
    if (nblocks) *nblocks = (int)(grid2.x * grid2.y * grid2.z);
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // given the values (every BTV call; the TV kinds from srmap_reg_values_and_gradient, whose view has no halo channel:
  // the Exact leg's dz self term asks c + 1 < C)
  if (exact && rs.kind == SRMAP_REG_BTV &&
      launch_btv_gradient_exact4<T>(geo, rs, x, gc, (T)gc_scale, values, g, accumulate ? 1 : 0, partials, nblocks, st)) {
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  dim3 grid((geo.W * geo.H + 255) / 256, geo.C);
  if (exact)
    hipLaunchKernelGGL((k_reg_gradient_direct<T, true>), grid, dim3(256), 0, st, x, gc, (T)gc_scale,
                       values, g, accumulate ? 1 : 0, partials, geo.W, geo.H, geo.C, rs.kind,
                       rs.range, make_pow(rs), geo.cr0, geo.cr1);
  else
    hipLaunchKernelGGL(k_reg_gradient_direct<T>, grid, dim3(256), 0, st, x, gc, (T)gc_scale,
                       values, g, accumulate ? 1 : 0, partials, geo.W, geo.H, geo.C, rs.kind,
                       rs.range, make_pow(rs), geo.cr0, geo.cr1);
  if (nblocks) *nblocks = (int)(grid.x * grid.y);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

#define INSTANTIATE(T)                                                                      \
  template int launch_reg_values<T>(srmap_problem*, const Geometry&, const RegSpec&,       \
                                    const T*, T*, hipStream_t);                             \
  template int launch_reg_gradient_direct<T>(srmap_problem*, const Geometry&,              \
                                             const RegSpec&, const T*, const T*, double,   \
                                             const T*, T*, bool, double*, int*,            \
                                             hipStream_t);                                  \
  template int launch_reg_weights<T>(srmap_problem*, const Geometry&, const RegSpec&, const T*, T*, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)

}  // namespace srmap
