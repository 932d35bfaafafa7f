// registration_flow.hip -- dense flow registration of a frame stack on the GPU (srmap_register_flow).
//
// For every frame k >= 1 a field u_k on frame k's grid with I_0(q + u_k(q)) ~= I_k(q): the convention of the
// displacement-field motion model (kernels_flow.hip), frame 0 playing x.  No reference counterpart; the checker is
// tests/flow_registration_restatement.py.
//   1. box pyramid of the whole stack, built once (k_down2_stack, motion_fit.hip), halved while the shorter side is >= 32,
//      and the two gradient planes of frame 0 at every level (k_flow_gradients);
//   2. start at the coarsest level: u = 0, or u(q) = F^-1(q) - q of the caller's matrices taken down the pyramid;
//   3. per level a FIXED number of warp passes, each two launches for all frames (k_flow_lk_pass, k_flow_smooth), then
//      k_flow_resample to the next level;
//   4. k_flow_resample to the HR grid, k_flow_finish (validity mask, residual sums) and k_flow_maxdiff (the neighbour
//      differences of the returned field), their per-workgroup records added on the host in index order.
// Nothing comes back to the host between the upload and the final copies: one stream wait per call.
// Three entry points share the one body: srmap_register_flow (host doubles in, host results out), srmap_register_flow_device
// (device doubles in, device results out, the non-finite scan a device count in the records that come back anyway) and
// srmap_problem_register_flow (the plane from the problem's observation buffer, the field and the masks installed as the
// problem's motion and data prior without leaving the device).
// Every kernel here keeps fp contraction OFF: each operation is rounded on its own and the sums run in the order the
// restatement states, so the result does not depend on the tile decomposition and the restatement forms the same numbers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "affine_map.hpp"
#include "motion_fit_dev.hpp"
#include "solver_passes.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kMinSize = 16;
constexpr int kMaxWindowRadius = 8;
constexpr int kMaxSmoothRadius = 8;
constexpr int kMaxRecordBlocks = 1024;

// the four-tap sample at p = &plane[y0][x0] with fractions (fx, fy); x0 <= w - 2, y0 <= h - 2
__device__ __forceinline__ double bilinear4(const double* __restrict__ p, int w, double fx, double fy) {
#pragma clang fp contract(off)
  return (1.0 - fy) * ((1.0 - fx) * p[0] + fx * p[1]) + fy * ((1.0 - fx) * p[w] + fx * p[w + 1]);
}

// the four taps at (sx, sy) are inside a w x h image (a NaN position is outside)
__device__ __forceinline__ bool taps_inside(double sx, double sy, int w, int h) {
  return sx >= 0.0 && sx < (double)(w - 1) && sy >= 0.0 && sy < (double)(h - 1);
}

// gx, gy [h][w]: central differences of img, one-sided at the border.  w, h >= 2.
__global__ __launch_bounds__(256) void k_flow_gradients(const double* __restrict__ img, int w, int h, double* __restrict__ gx,
                                                        double* __restrict__ gy) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w * h) return;
  const int y = i / w, x = i - y * w;
  const double* p = img + i;
  gx[i] = x == 0 ? p[1] - p[0] : x == w - 1 ? p[0] - p[-1] : 0.5 * (p[1] - p[-1]);
  gy[i] = y == 0 ? p[w] - p[0] : y == h - 1 ? p[0] - p[-w] : 0.5 * (p[w] - p[-w]);
}

// u[f][2][h][w] = G_f(q) - q, G_f = table[f][6] (the inverse of frame f + 1's matrix at this level).  grid = (pixels, frames)
__global__ __launch_bounds__(256) void k_flow_affine_start(const double* __restrict__ table, int w, int h, double* __restrict__ u) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w * h) return;
  const int y = i / w, x = i - y * w;
  const double* m = table + (size_t)blockIdx.y * 6;
  double* o = u + (size_t)blockIdx.y * 2 * w * h;
  o[i] = affine_coord(m[0], m[1], m[2], (double)x, (double)y) - (double)x;
  o[(size_t)w * h + i] = affine_coord(m[3], m[4], m[5], (double)x, (double)y) - (double)y;
}

// One warp pass for every frame, before the smoothing: v = u + du.  grid = (tiles_x * tiles_y, frames - 1), 256 threads,
// an output tile of TX x TY pixels, window radius r <= RMAX.
//   1. the tile with its 2 r halo: Tx, Ty, e at q + u(q) into LDS (0 outside the image or where a tap is outside);
//   2. per product (Tx Tx, Tx Ty, Ty Ty, Tx e, Ty e): the triangular sums along x of the halo rows into LDS, d ascending,
//      then along y into a register, d ascending -- every window sum is formed from the same numbers in the same order
//      whichever tile holds it;
//   3. the damped 2 x 2 solve, the step clipped to +-1 px.
template <int TX, int TY, int RMAX>
__global__ __launch_bounds__(256) void k_flow_lk_pass(const double* __restrict__ i0, const double* __restrict__ gx,
                                                      const double* __restrict__ gy, const double* __restrict__ frames,
                                                      const double* __restrict__ u, double* __restrict__ v, int w, int h,
                                                      int tiles_x, int r, double damping) {
#pragma clang fp contract(off)
  constexpr int kNpt = TX * TY / 256;
  static_assert(TX * TY % 256 == 0, "whole outputs per thread");
  constexpr int kPlane = (TX + 4 * RMAX) * (TY + 4 * RMAX);
  __shared__ double s_t[3][kPlane];              // Tx, Ty, e
  __shared__ double s_h[(TY + 4 * RMAX) * TX];   // the sums along x of one product
  const int f = blockIdx.y, tid = threadIdx.x;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int x0 = tile_x * TX, y0 = tile_y * TY, halo = 2 * r;
  const int pw = TX + 2 * halo, ph = TY + 2 * halo;
  const size_t n = (size_t)w * h;
  const double* ik = frames + (size_t)(f + 1) * n;
  const double* uf = u + (size_t)f * 2 * n;
  double* vf = v + (size_t)f * 2 * n;

  for (int idx = tid; idx < pw * ph; idx += 256) {
    const int ly = idx / pw, lx = idx - ly * pw;
    const int y = y0 - halo + ly, x = x0 - halo + lx;
    double tx = 0.0, ty = 0.0, e = 0.0;
    if (x >= 0 && x < w && y >= 0 && y < h) {
      const size_t q = (size_t)y * w + x;
      const double sx = (double)x + uf[q], sy = (double)y + uf[n + q];
      if (taps_inside(sx, sy, w, h)) {
        const double fx0 = __builtin_floor(sx), fy0 = __builtin_floor(sy);
        const double fx = sx - fx0, fy = sy - fy0;
        const size_t o = (size_t)(int)fy0 * w + (int)fx0;  // x in [0, w - 2], y in [0, h - 2]
        tx = bilinear4(gx + o, w, fx, fy);
        ty = bilinear4(gy + o, w, fx, fy);
        e = bilinear4(i0 + o, w, fx, fy) - ik[q];
      }
    }
    s_t[0][idx] = tx;
    s_t[1][idx] = ty;
    s_t[2][idx] = e;
  }
  __syncthreads();

  double acc[kNpt][5];
  constexpr int kFirst[5] = {0, 0, 1, 0, 1}, kSecond[5] = {0, 1, 1, 2, 2};
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    const double* a = s_t[kFirst[p]];
    const double* b = s_t[kSecond[p]];
    for (int idx = tid; idx < ph * TX; idx += 256) {
      const int ly = idx / TX, lx = idx - ly * TX;
      const double* pa = a + ly * pw + lx;  // lx + halo + d, d = -halo ... halo
      const double* pb = b + ly * pw + lx;
      double s = 0.0;
      for (int j = 0; j <= 2 * halo; ++j) {
        const int d = j - halo;
        s = s + (double)(halo + 1 - (d < 0 ? -d : d)) * (pa[j] * pb[j]);
      }
      s_h[idx] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kNpt; ++i) {
      const int o = tid + i * 256, oy = o / TX, ox = o - oy * TX;
      const double* ps = s_h + oy * TX + ox;  // row oy + halo + d
      double s = 0.0;
      for (int j = 0; j <= 2 * halo; ++j) {
        const int d = j - halo;
        s = s + (double)(halo + 1 - (d < 0 ? -d : d)) * ps[j * TX];
      }
      acc[i][p] = s;
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < kNpt; ++i) {
    const int o = tid + i * 256, oy = o / TX, ox = o - oy * TX;
    const int x = x0 + ox, y = y0 + oy;
    if (x >= w || y >= h) continue;
    const double a = acc[i][0], b = acc[i][1], c = acc[i][2], p = acc[i][3], q = acc[i][4];
    const double lam = damping * (0.5 * (a + c));
    const double a1 = a + lam, c1 = c + lam;
    const double det = a1 * c1 - b * b;
    double dux = 0.0, duy = 0.0;
    if (det > 0.0) {
      dux = -((c1 * p - b * q) / det);
      duy = -((a1 * q - b * p) / det);
      dux = fmin(fmax(dux, -1.0), 1.0);
      duy = fmin(fmax(duy, -1.0), 1.0);
    }
    const size_t qi = (size_t)y * w + x;
    vf[qi] = uf[qi] + dux;
    vf[n + qi] = uf[n + qi] + duy;
  }
}

// u[plane] = the box mean of v[plane] over radius R, rows then columns ascending, divided by the number of in-image pixels.
// grid = (pixels, 2 * (frames - 1))
__global__ __launch_bounds__(256) void k_flow_smooth(const double* __restrict__ v, double* __restrict__ u, int w, int h, int R) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w * h) return;
  const int y = i / w, x = i - y * w;
  const double* p = v + (size_t)blockIdx.y * w * h;
  const int ya = max(0, y - R), yb = min(h - 1, y + R), xa = max(0, x - R), xb = min(w - 1, x + R);
  double s = 0.0;
  for (int yy = ya; yy <= yb; ++yy)
    for (int xx = xa; xx <= xb; ++xx) s = s + p[(size_t)yy * w + xx];
  u[(size_t)blockIdx.y * w * h + i] = s / (double)((yb - ya + 1) * (xb - xa + 1));
}

// out[plane][oh][ow] = gain * bilinear(u[plane] at (Q - sub) / div), coordinates clamped to u's w x h image (w, h >= 2).
// grid = (output pixels, planes)
__global__ __launch_bounds__(256) void k_flow_resample(const double* __restrict__ u, int w, int h, double* __restrict__ out, int ow,
                                                       int oh, double sub, double div, double gain) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)ow * oh) return;
  const int y = (int)(i / ow), x = (int)(i - (size_t)y * ow);
  const double cx = fmin(fmax(((double)x - sub) / div, 0.0), (double)(w - 1));
  const double cy = fmin(fmax(((double)y - sub) / div, 0.0), (double)(h - 1));
  const int xi = min((int)__builtin_floor(cx), w - 2), yi = min((int)__builtin_floor(cy), h - 2);
  const double* p = u + (size_t)blockIdx.y * w * h + (size_t)yi * w + xi;
  out[(size_t)blockIdx.y * ow * oh + i] = gain * bilinear4(p, w, cx - (double)xi, cy - (double)yi);
}

// valid[f][h][w] (1 / 0) at the result and record[(f * blocks + block)][2] = {sum of e^2, count} over the valid pixels this
// workgroup visits, e = I_0(q + u) - I_{f+1}(q).  grid = (blocks, frames - 1)
__global__ __launch_bounds__(256) void k_flow_finish(const double* __restrict__ i0, const double* __restrict__ frames,
                                                     const double* __restrict__ u, int w, int h, int margin,
                                                     double* __restrict__ valid, double* __restrict__ record) {
#pragma clang fp contract(off)
  __shared__ double red[2][4];
  const int f = blockIdx.y;
  const size_t n = (size_t)w * h;
  const double* ik = frames + (size_t)(f + 1) * n;
  const double* uf = u + (size_t)f * 2 * n;
  double see = 0.0, cnt = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int y = (int)(i / w), x = (int)(i - (size_t)y * w);
    const double sx = (double)x + uf[i], sy = (double)y + uf[n + i];
    const bool ok = taps_inside(sx, sy, w, h) && x >= margin && x <= w - 1 - margin && y >= margin && y <= h - 1 - margin;
    if (ok) {
      const double fx0 = __builtin_floor(sx), fy0 = __builtin_floor(sy);
      const double e = bilinear4(i0 + (size_t)(int)fy0 * w + (int)fx0, w, sx - fx0, sy - fy0) - ik[i];
      see = see + e * e;
      cnt = cnt + 1.0;
    }
    valid[(size_t)f * n + i] = ok ? 1.0 : 0.0;
  }
  const double a = block_sum_256(see, red[0]), b = block_sum_256(cnt, red[1]);
  if (threadIdx.x == 0) {
    double* o = record + ((size_t)f * gridDim.x + blockIdx.x) * 2;
    o[0] = a;
    o[1] = b;
  }
}

// record[(f * blocks + block)][2] = the largest |difference| between horizontal / vertical neighbours over both components
// of field[f][2][H][W], over the pixels this workgroup visits.  grid = (blocks, frames - 1)
__global__ __launch_bounds__(256) void k_flow_maxdiff(const double* __restrict__ field, int W, int H, double* __restrict__ record) {
  __shared__ double red[2][4];
  const size_t n = (size_t)W * H;
  const double* uf = field + (size_t)blockIdx.y * 2 * n;
  double mx = 0.0, my = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    for (int c = 0; c < 2; ++c) {
      const double* p = uf + (size_t)c * n + i;
      if (x + 1 < W) mx = fmax(mx, fabs(p[1] - p[0]));
      if (y + 1 < H) my = fmax(my, fabs(p[W] - p[0]));
    }
  }
  mx = wave_max(mx);
  my = wave_max(my);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[0][wv] = mx; red[1][wv] = my; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = record + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = combine4(red[0], true);
    o[1] = combine4(red[1], true);
  }
}

void launch_lk_pass(const double* i0, const double* gx, const double* gy, const double* frames, const double* u, double* v, int w,
                    int h, int nf, int r, double damping, hipStream_t st) {
  if (r <= 4) {
    const int tx = (w + 31) / 32, ty = (h + 15) / 16;
    hipLaunchKernelGGL((k_flow_lk_pass<32, 16, 4>), dim3(tx * ty, nf), dim3(256), 0, st, i0, gx, gy, frames, u, v, w, h, tx, r, damping);
  } else {
    const int tx = (w + 15) / 16, ty = (h + 15) / 16;
    hipLaunchKernelGGL((k_flow_lk_pass<16, 16, kMaxWindowRadius>), dim3(tx * ty, nf), dim3(256), 0, st, i0, gx, gy, frames, u, v, w,
                       h, tx, r, damping);
  }
}

int blocks_of(size_t n) { return (int)((n + 255) / 256); }

// ---- the device-resident forms (srmap_register_flow_device, srmap_problem_register_flow) ----
// record[k * blocks + block] = the number of non-finite pixels of images[k][n] this workgroup visits.  grid = (blocks, K)
__global__ __launch_bounds__(256) void k_flow_count_nonfinite(const double* __restrict__ images, size_t n, double* __restrict__ record) {
  __shared__ double red[4];
  const double* p = images + (size_t)blockIdx.y * n;
  double c = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    if (!(fabs(p[i]) < INFINITY)) c = c + 1.0;
  const double t = block_sum_256(c, red);
  if (threadIdx.x == 0) record[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// plane[k][n] (double) of obs[k][C][n]: channel >= 0 that channel; else the mean, the sum in ascending channel order and
// one division by C.  T -> double is exact.  grid = (pixels, K)
template <typename T>
__global__ __launch_bounds__(256) void k_flow_plane(const T* __restrict__ obs, int C, int channel, size_t n, double* __restrict__ plane) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T* o = obs + (size_t)blockIdx.y * C * n + i;
  double v;
  if (channel >= 0) {
    v = (double)o[(size_t)channel * n];
  } else {
    double t = 0.0;
    for (int c = 0; c < C; ++c) t = t + (double)o[(size_t)c * n];
    v = t / (double)C;
  }
  plane[(size_t)blockIdx.y * n + i] = v;
}

// out[K][2][N] (T) = the double field hr[K - 1][2][N] of the frames 1..., rounded once; frame 0 is zero
template <typename T>
__global__ __launch_bounds__(256) void k_flow_round(const double* __restrict__ hr, size_t frame_elems, size_t total, T* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
    out[i] = i < frame_elems ? T(0) : (T)hr[i - frame_elems];
}

// nodes[frames][2][n] = gain * u[frames][2][n]: the input-level field in HR pixels, the control lattice of step `gain`
// (srmap_problem_register_flow_lattice; the product commutes with k_flow_resample's rounding for a power of two)
__global__ __launch_bounds__(256) void k_flow_nodes(const double* __restrict__ u, size_t total, double gain, double* __restrict__ nodes) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) nodes[i] = gain * u[i];
}

// prior[K][C][n] (T) = valid[K - 1][n] of the frames 1... broadcast over the channels; frame 0 is one.  grid = (pixels, C, K)
template <typename T>
__global__ __launch_bounds__(256) void k_flow_prior(const double* __restrict__ valid, size_t n, T* __restrict__ prior) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = blockIdx.z;
  prior[((size_t)k * gridDim.y + blockIdx.y) * n + i] = k == 0 ? T(1) : (T)valid[(size_t)(k - 1) * n + i];
}

// the device buffers of one call
struct FlowBuffers {
  DevBuf pyr, grad, u, v, hr, valid, rec, tab;  // doubles
  DevBuf field, prior;  // srmap_problem_register_flow: the field and the prior in the problem's dtype
  DevBuf nodes;         // srmap_problem_register_flow_lattice: [K][2][h][w] doubles, s * u of the input level (image 0: zero)
  static bool get(DevBuf* b, size_t elems) { return b->alloc(elems * sizeof(double)) == hipSuccess; }
};

// Where the stack of one call comes from and where its results go.  Exactly one source: images_host (pageable doubles,
// scanned on the host), images_dev (device doubles) or problem (its observation buffer; k_flow_plane).  Host results
// (flow_host, valid_host) are copied back; device results are written where they are wanted: flow_dev / valid_dev when
// given, else the call's own buffers b.hr / b.valid ([frames - 1] planes, image 0 left to the caller).  lattice (with
// problem): the call stops at the input level -- b.nodes instead of b.hr, no output-sized buffer, and quality [3i+2] from
// the nodes: (largest node difference along x + along y) / step, which the expanded field's equals to rounding.
struct FlowIo {
  const double* images_host = nullptr;
  const double* images_dev = nullptr;
  srmap_problem* problem = nullptr;
  int channel = -1;
  bool lattice = false;
  double *flow_host = nullptr, *valid_host = nullptr;
  double *flow_dev = nullptr, *valid_dev = nullptr;
  bool on_device() const { return images_host == nullptr; }
};

int check_options(srmap_ctx* ctx, const srmap_flow_registration_options* options, srmap_flow_registration_options* opt) {
  if (int rc = options_in_force(ctx, options, srmap_flow_registration_options_default, "srmap_flow_registration_options", opt)) return rc;
  if (opt->hr_scale < 1 || opt->warps < 1 || opt->window_radius < 1 || opt->window_radius > kMaxWindowRadius ||
      !(opt->damping >= 0.0) || !std::isfinite(opt->damping) || opt->smooth_radius < 0 || opt->smooth_radius > kMaxSmoothRadius ||
      opt->valid_margin < 0 || opt->max_levels < 0)
    return set_error(ctx, SRMAP_EINVAL, "flow registration: bad options");
  return SRMAP_OK;
}

// The registration of K >= 1 images of width x height by the checked options `opt`, on st: the one body of the host form
// and the device forms.  One stream wait; everything is complete on return.
int register_flow_body(srmap_ctx* ctx, int K, int width, int height, const srmap_flow_registration_options& opt, const FlowIo& io,
                       FlowBuffers& b, hipStream_t st, double* quality_out) {
  if (width < kMinSize || height < kMinSize)
    return set_error(ctx, SRMAP_EINVAL, "flow registration needs images of at least 16 x 16");
  const int nf = K - 1, s = opt.hr_scale;
  const size_t n = (size_t)width * height;
  if ((size_t)s * width > (size_t)1 << 20 || (size_t)s * height > (size_t)1 << 20 || n * s * s > (size_t)1 << 30)
    return set_error(ctx, SRMAP_EINVAL, "flow registration: the output grid is too large");
  if (io.images_host)
    for (size_t i = 0; i < (size_t)K * n; ++i)
      if (!std::isfinite(io.images_host[i]))
        return set_error(ctx, SRMAP_EINVAL, "flow registration: image %d is not finite", (int)(i / n));

  std::vector<int> lw, lh;
  pyramid_levels(width, height, 2 * kMinSize, opt.max_levels, &lw, &lh);
  const int L = (int)lw.size();

  std::vector<double> h_tab;
  if (opt.initial_affine_2x3 && nf > 0) {
    h_tab.resize((size_t)nf * 6);
    for (int f = 0; f < nf; ++f) {
      AffineMap F;
      std::copy(opt.initial_affine_2x3 + 6 * (f + 1), opt.initial_affine_2x3 + 6 * (f + 2), F.m);
      if (!all_finite(F) || deviation(F) > kAffineMaxDeviation)
        return set_error(ctx, SRMAP_EINVAL, "flow registration: initial matrix %d is not finite or outside the model's domain", f + 1);
      for (int l = 1; l < L; ++l) F = to_coarser(F);
      const AffineMap G = inverse(F);
      std::copy(G.m, G.m + 6, h_tab.begin() + 6 * f);
    }
  }

  const size_t N = n * s * s;
  if (io.flow_host) std::memset(io.flow_host, 0, 2 * N * sizeof(double));
  if (io.valid_host) std::fill(io.valid_host, io.valid_host + n, 1.0);
  if (quality_out) { quality_out[0] = 0.0; quality_out[1] = 1.0; quality_out[2] = 0.0; }
  if (K == 1 && !io.on_device()) return SRMAP_OK;

  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  // image 0's planes of the device results
  if (io.flow_dev) SRMAP_HIP(ctx, hipMemsetAsync(io.flow_dev, 0, 2 * N * sizeof(double), st));
  if (io.valid_dev) launch_fill<double>(io.valid_dev, 1.0, n, st);

  std::vector<size_t> off(L + 1, 0), goff(L + 1, 0);
  for (int l = 0; l < L; ++l) {
    off[l + 1] = off[l] + (size_t)K * lw[l] * lh[l];
    goff[l + 1] = goff[l] + (size_t)2 * lw[l] * lh[l];
  }
  const int fin_blocks = std::min(kMaxRecordBlocks, blocks_of(n)), max_blocks = std::min(kMaxRecordBlocks, blocks_of(io.lattice ? n : N));
  const int cnt_blocks = io.on_device() ? fin_blocks : 0;  // the device count of the non-finite pixels, per image
  const size_t rec_quality = (size_t)nf * 2 * (fin_blocks + max_blocks), rec_elems = rec_quality + (size_t)K * cnt_blocks;
  const bool own_hr = !io.flow_dev && !io.lattice, own_valid = !io.valid_dev;

  if (!FlowBuffers::get(&b.pyr, off[L]) || !FlowBuffers::get(&b.grad, goff[L]) || !FlowBuffers::get(&b.u, (size_t)nf * 2 * n) ||
      !FlowBuffers::get(&b.v, (size_t)nf * 2 * n) || (own_hr && !FlowBuffers::get(&b.hr, (size_t)nf * 2 * N)) ||
      (own_valid && !FlowBuffers::get(&b.valid, (size_t)nf * n)) || !FlowBuffers::get(&b.rec, rec_elems) ||
      (io.lattice && !FlowBuffers::get(&b.nodes, (size_t)K * 2 * n)) ||
      !FlowBuffers::get(&b.tab, h_tab.size()))
    return set_error(ctx, SRMAP_ENOMEM, "flow registration: allocation failed");
  double *const pyr = b.pyr.as<double>(), *const grad = b.grad.as<double>(), *const rec = b.rec.as<double>(), *const tab = b.tab.as<double>();
  double* hr = io.lattice ? nullptr : own_hr ? b.hr.as<double>() : io.flow_dev + 2 * N;
  if (io.lattice) SRMAP_HIP(ctx, hipMemsetAsync(b.nodes.as(), 0, 2 * n * sizeof(double), st));  // image 0
  double* valid = own_valid ? b.valid.as<double>() : io.valid_dev + n;

  // ---- pyramids of the whole stack and the gradient planes of frame 0, once ----
  if (io.images_host) {
    SRMAP_HIP(ctx, hipMemcpyAsync(pyr, io.images_host, (size_t)K * n * sizeof(double), hipMemcpyHostToDevice, st));
  } else if (io.images_dev) {
    SRMAP_HIP(ctx, hipMemcpyAsync(pyr, io.images_dev, (size_t)K * n * sizeof(double), hipMemcpyDeviceToDevice, st));
  } else {
    const srmap_problem* p = io.problem;
    dispatch_dtype(p->dtype, [&](auto t) {
      hipLaunchKernelGGL(k_flow_plane<decltype(t)>, dim3(blocks_of(n), K), dim3(256), 0, st, p->d_obs.as<const decltype(t)>(), p->geo.C, io.channel, n, pyr);
    });
  }
  if (cnt_blocks > 0)
    hipLaunchKernelGGL(k_flow_count_nonfinite, dim3(cnt_blocks, K), dim3(256), 0, st, (const double*)pyr, n, rec + rec_quality);
  if (nf > 0) {
    for (int l = 1; l < L; ++l) launch_down2_stack(pyr + off[l - 1], pyr + off[l], lw[l - 1], lh[l - 1], K, st);
    for (int l = 0; l < L; ++l) {
      const size_t nl = (size_t)lw[l] * lh[l];
      hipLaunchKernelGGL(k_flow_gradients, dim3(blocks_of(nl)), dim3(256), 0, st, pyr + off[l], lw[l], lh[l], grad + goff[l],
                         grad + goff[l] + nl);
    }

    // ---- start at the coarsest level ----
    double *u = b.u.as<double>(), *v = b.v.as<double>();
    {
      const int cw = lw[L - 1], ch = lh[L - 1];
      if (h_tab.empty()) {
        SRMAP_HIP(ctx, hipMemsetAsync(u, 0, (size_t)nf * 2 * cw * ch * sizeof(double), st));
      } else {
        SRMAP_HIP(ctx, hipMemcpyAsync(tab, h_tab.data(), h_tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_flow_affine_start, dim3(blocks_of((size_t)cw * ch), nf), dim3(256), 0, st, tab, cw, ch, u);
      }
    }

    // ---- the warp passes, coarse to fine ----
    for (int l = L - 1; l >= 0; --l) {
      const int w = lw[l], h = lh[l];
      const size_t nl = (size_t)w * h;
      for (int it = 0; it < opt.warps; ++it) {
        launch_lk_pass(pyr + off[l], grad + goff[l], grad + goff[l] + nl, pyr + off[l], u, v, w, h, nf, opt.window_radius,
                       opt.damping, st);
        hipLaunchKernelGGL(k_flow_smooth, dim3(blocks_of(nl), 2 * nf), dim3(256), 0, st, v, u, w, h, opt.smooth_radius);
      }
      if (l > 0) {
        const int fw = lw[l - 1], fh = lh[l - 1];
        hipLaunchKernelGGL(k_flow_resample, dim3(blocks_of((size_t)fw * fh), 2 * nf), dim3(256), 0, st, u, w, h, v, fw, fh, 0.5, 2.0, 2.0);
        std::swap(u, v);
      }
    }

    // ---- the HR field, the mask and the quality records ----
    double* rec_fin = rec;
    double* rec_max = rec + (size_t)nf * 2 * fin_blocks;
    if (io.lattice) {
      const size_t total = (size_t)nf * 2 * n;
      hipLaunchKernelGGL(k_flow_nodes, dim3(std::min(blocks_of(total), 4096)), dim3(256), 0, st, (const double*)u, total, (double)s,
                         b.nodes.as<double>() + 2 * n);
    } else {
      hipLaunchKernelGGL(k_flow_resample, dim3(blocks_of(N), 2 * nf), dim3(256), 0, st, u, width, height, hr, s * width, s * height, 0.0,
                         (double)s, (double)s);
    }
    hipLaunchKernelGGL(k_flow_finish, dim3(fin_blocks, nf), dim3(256), 0, st, pyr, pyr, u, width, height, opt.valid_margin, valid,
                       rec_fin);
    if (io.lattice)
      hipLaunchKernelGGL(k_flow_maxdiff, dim3(max_blocks, nf), dim3(256), 0, st, b.nodes.as<const double>() + 2 * n, width, height, rec_max);
    else
      hipLaunchKernelGGL(k_flow_maxdiff, dim3(max_blocks, nf), dim3(256), 0, st, hr, s * width, s * height, rec_max);
  }
  SRMAP_HIP(ctx, hipGetLastError());
  // ---- the one wait ----
  std::vector<double> h_rec(rec_elems);
  if (io.flow_host) SRMAP_HIP(ctx, hipMemcpyAsync(io.flow_host + 2 * N, hr, (size_t)nf * 2 * N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (io.valid_host) SRMAP_HIP(ctx, hipMemcpyAsync(io.valid_host + n, valid, (size_t)nf * n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (rec_elems > 0) SRMAP_HIP(ctx, hipMemcpyAsync(h_rec.data(), rec, rec_elems * sizeof(double), hipMemcpyDeviceToHost, st));
  SRMAP_HIP(ctx, hipStreamSynchronize(st));

  for (int k = 0; k < K && cnt_blocks > 0; ++k) {
    double bad = 0.0;
    for (int j = 0; j < cnt_blocks; ++j) bad += h_rec[rec_quality + (size_t)k * cnt_blocks + j];
    if (bad != 0.0) return set_error(ctx, SRMAP_EINVAL, "flow registration: image %d is not finite", k);
  }
  if (quality_out) {
    for (int f = 0; f < nf; ++f) {
      double see = 0.0, cnt = 0.0, mx = 0.0, my = 0.0;
      for (int k = 0; k < fin_blocks; ++k) {
        see += h_rec[((size_t)f * fin_blocks + k) * 2];
        cnt += h_rec[((size_t)f * fin_blocks + k) * 2 + 1];
      }
      const double* rm = h_rec.data() + (size_t)nf * 2 * fin_blocks;
      for (int k = 0; k < max_blocks; ++k) {
        mx = std::max(mx, rm[((size_t)f * max_blocks + k) * 2]);
        my = std::max(my, rm[((size_t)f * max_blocks + k) * 2 + 1]);
      }
      double* q = quality_out + 3 * (f + 1);
      q[0] = cnt > 0 ? std::sqrt(see / cnt) : 0.0;
      q[1] = cnt / (double)n;
      q[2] = io.lattice ? (mx + my) / (double)s : mx + my;
    }
  }
  return SRMAP_OK;
}

// (want_field) the field and (want_prior) the prior of a problem in its dtype from the body's buffers, enqueued on st
template <typename T>
int problem_stage(srmap_problem* p, FlowBuffers& b, bool want_field, bool want_prior, hipStream_t st) {
  const Geometry& g = p->geo;
  const size_t n = (size_t)g.w * g.h, N = (size_t)g.W * g.H, total = (size_t)g.K * 2 * N;
  if ((want_field && b.field.alloc(total * sizeof(T)) != hipSuccess) || (want_prior && b.prior.alloc(p->lr_count() * sizeof(T)) != hipSuccess))
    return set_error(p->ctx, SRMAP_ENOMEM, "flow registration: allocation failed");
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)std::max(1, p->ctx->num_cus) * 16);
  if (want_field)
    hipLaunchKernelGGL(k_flow_round<T>, dim3(std::max(1u, blocks)), dim3(256), 0, st, b.hr.as<const double>(), 2 * N, total, b.field.as<T>());
  if (want_prior)
    hipLaunchKernelGGL(k_flow_prior<T>, dim3(blocks_of(n), g.C, g.K), dim3(256), 0, st, b.valid.as<const double>(), n, b.prior.as<T>());
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// srmap_problem_register_flow (lattice = false) and srmap_problem_register_flow_lattice: the plane rule, the options and
// the errors are one; the lattice form stops at the input level and installs nodes = s * u with step s on the LR grid
int problem_register(srmap_problem* p, int channel, const srmap_flow_registration_options* options, int install_prior,
                     double* quality_out, bool lattice) {
  srmap_ctx* ctx = p->ctx;
  const Geometry& g = p->geo;
  srmap_flow_registration_options opt;
  if (int rc = check_options(ctx, options, &opt)) return rc;
  if (!p->have_obs || !p->d_obs) return set_error(ctx, SRMAP_EINVAL, "flow registration: no observations set");
  if (channel < -1 || channel >= g.C) return set_error(ctx, SRMAP_EINVAL, "flow registration: channel %d of %d", channel, g.C);
  if (g.W != g.w * g.s || g.H != g.h * g.s)
    return set_error(ctx, SRMAP_EINVAL, "flow registration: HR size %dx%d is not LR size * scale (%d)", g.W, g.H, g.s);
  if (opt.hr_scale != 1 && opt.hr_scale != g.s)
    return set_error(ctx, SRMAP_EINVAL, "flow registration: hr_scale %d is neither 1 nor the problem's scale %d", opt.hr_scale, g.s);
  opt.hr_scale = g.s;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = problem_state_read(p, st)) return rc;
  FlowIo io;
  io.problem = p;
  io.channel = channel;
  io.lattice = lattice;
  FlowBuffers b;
  if (int rc = register_flow_body(ctx, g.K, g.w, g.h, opt, io, b, st, quality_out)) return rc;
  const bool prior = install_prior != 0;
  if (int rc = dispatch_dtype(p->dtype, [&](auto t) { return problem_stage<decltype(t)>(p, b, !lattice, prior, st); })) return rc;
  // a refused field leaves the motion -- and the prior -- the problem had
  if (int rc = lattice ? srmap_problem_set_flow_lattice_device(p, g.s, g.w, g.h, b.nodes.as<const double>(), st)
                       : srmap_problem_set_flow_device(p, b.field.as(), st))
    return rc;
  return prior ? srmap_set_data_prior_device(p, b.prior.as(), st) : SRMAP_OK;
}

}  // namespace

}  // namespace srmap

using namespace srmap;

extern "C" void srmap_flow_registration_options_default(srmap_flow_registration_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_flow_registration_options);
  o->hr_scale = 1;
  o->warps = 8;
  o->window_radius = 4;
  o->damping = 0.05;
  o->smooth_radius = 2;
  o->valid_margin = 3;
  o->max_levels = 0;
  o->initial_affine_2x3 = nullptr;
}

extern "C" int srmap_register_flow(srmap_ctx* ctx, int num_images, int width, int height, const double* images_host,
                                   const srmap_flow_registration_options* options, double* flow_out, double* valid_out,
                                   double* quality_out) {
  if (!ctx || !flow_out || num_images < 0) return SRMAP_EINVAL;
  srmap_flow_registration_options opt;
  if (int rc = check_options(ctx, options, &opt)) return rc;
  if (num_images == 0) return SRMAP_OK;
  if (!images_host) return set_error(ctx, SRMAP_EINVAL, "flow registration needs images of at least 16 x 16");
  FlowIo io;
  io.images_host = images_host;
  io.flow_host = flow_out;
  io.valid_host = valid_out;
  FlowBuffers b;
  return register_flow_body(ctx, num_images, width, height, opt, io, b, ctx->stream, quality_out);
}

extern "C" int srmap_register_flow_device(srmap_ctx* ctx, int num_images, int width, int height, const double* images_dev,
                                          void* hip_stream, const srmap_flow_registration_options* options, double* flow_dev_out,
                                          double* valid_dev_out, double* quality_out) {
  if (!ctx || !flow_dev_out || num_images < 0) return SRMAP_EINVAL;
  srmap_flow_registration_options opt;
  if (int rc = check_options(ctx, options, &opt)) return rc;
  if (num_images == 0) return SRMAP_OK;
  if (!images_dev) return set_error(ctx, SRMAP_EINVAL, "flow registration needs images of at least 16 x 16");
  FlowIo io;
  io.images_dev = images_dev;
  io.flow_dev = flow_dev_out;
  io.valid_dev = valid_dev_out;
  FlowBuffers b;
  return register_flow_body(ctx, num_images, width, height, opt, io, b, stream_of(ctx, hip_stream), quality_out);
}

extern "C" int srmap_problem_register_flow(srmap_problem* p, int channel, const srmap_flow_registration_options* options,
                                           int install_prior, double* quality_out) {
  if (!p) return SRMAP_EINVAL;
  return problem_register(p, channel, options, install_prior, quality_out, false);
}

extern "C" int srmap_problem_register_flow_lattice(srmap_problem* p, int channel, const srmap_flow_registration_options* options,
                                                   int install_prior, double* quality_out) {
  if (!p) return SRMAP_EINVAL;
  return problem_register(p, channel, options, install_prior, quality_out, true);
}
