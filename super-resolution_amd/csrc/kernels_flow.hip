// kernels_flow.hip -- the direct family's data-term kernels for a DENSE per-frame displacement field
// (srmap_problem_set_flow; no reference counterpart: motion_module.cpp:18-51 warps by a translation only).  DESIGN.md 3.11.
//
// Frame k carries a field u_k = (ux, uy) on its HR-grid image, stored in the problem's dtype as [K][2][H][W].  The forward
// warp samples x bilinearly at s = q + u_k(q) for every pixel q of the warped image (taps outside the image contribute 0:
// affine_sample); blur and decimation are the translational path's.  s = (double)q + (double)u is exact in double for
// both dtypes (|u| <= 2^20), and the weights are the double products rounded to T, as in the affine model.
//
// The transpose is the EXACT transpose of that matrix in gather form.  For an HR pixel p the contributing q are those with
// q + u(q) strictly inside p +- 1 per axis.  They are found through a SEED stored per (k, p) when the field is set
// (k_flow_seed: the fixed-point iteration q <- round(p - u(clamp(q)))): the gather scans the 5 x 5 window around the seed
// and recomputes each candidate's weight from s by the forward kernel's expressions (flow_source, affine_axis_weight), so
// the two kernels hold the same matrix bit for bit and no atomics are needed.  That every (q, p) pair of the matrix lies
// inside p's window is VERIFIED when the field is set (k_flow_check walks the forward direction), not assumed: a field
// that folds or shears beyond the window is refused and never reaches these kernels.
//
// Both kernels read their sources through the caches (per LR pixel b^2 x (2 field values + 4 taps of x); per HR pixel and
// frame one seed and <= 25 candidates' field values, the x component first and the y component only where the x weight is
// not zero).  The plane bases of the field and of the seeds are formed from wave-uniform values (blockIdx, the frame loop).
#include <algorithm>
#include <cmath>

#include "reduce_dev.hpp"
#include "sample_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kFlowSeedSteps = 16;         // fixed-point steps of k_flow_seed (it stops early at a fixed point)
constexpr int kFlowPad = kFlowRadius;      // seeds are clamped to [-kFlowPad, W - 1 + kFlowPad] per axis before packing
constexpr double kFlowMaxDisp = 1048576.0; // 2^20

// seed (sx, sy), each clamped to [-kFlowPad, size - 1 + kFlowPad], as one int
__device__ __forceinline__ int flow_pack_seed(int sx, int sy, int W) { return (sy + kFlowPad) * (W + 2 * kFlowPad) + (sx + kFlowPad); }
__device__ __forceinline__ void flow_unpack_seed(int v, int W, int* sx, int* sy) {
  const int SW = W + 2 * kFlowPad;
  const int y = v / SW;
  *sy = y - kFlowPad;
  *sx = v - y * SW - kFlowPad;
}

}  // namespace

// ---------------------------------------------------------------------------
// A_k = D B M_k at every LR pixel of frames [k0, k0 + gridDim.z): k_forward_affine's contract (residual or weighted
// residual into `out`, cost partial with the cost-row test, one partial per workgroup in the same order).
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_forward_flow(
    const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out, double* __restrict__ partials, Geometry g,
    const T* __restrict__ flow, const T* __restrict__ blur, const int* __restrict__ col_map,
    const int* __restrict__ row_map, int k0, double cost_scale, int obs_C, int obs_c0, const T* __restrict__ dw) {
  __shared__ double red[4];
  const int lp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, kk = blockIdx.z, k = k0 + kk;
  const int n = g.w * g.h;
  const size_t N = (size_t)g.W * g.H;
  const T* __restrict__ fux = flow + (size_t)k * 2 * N;  // uniform bases
  const T* __restrict__ fuy = fux + N;
  double sq = 0.0;
  if (lp < n) {
    const int i = lp / g.w, j = lp - i * g.w;
    const int R0 = row_map[i], C0 = col_map[j];
    const T* plane = x + (size_t)c * N;
    T acc = T(0);
    for (int a = 0; a < g.b; ++a) {
      const int rr = R0 + a - g.hb;
      if (rr < 0 || rr >= g.H) continue;  // filter2D BORDER_CONSTANT on the warped image
      for (int e = 0; e < g.b; ++e) {
        const int cc = C0 + e - g.hb;
        if (cc < 0 || cc >= g.W) continue;
        const size_t qi = (size_t)rr * g.W + cc;
        const double sx = flow_source(cc, fux[qi]), sy = flow_source(rr, fuy[qi]);
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
int launch_forward_flow(srmap_problem* p, const Geometry& g, const T* x, const T* y, int obs_C, int obs_c0, T* out,
                        int k0, int nk, double* partials, int* nblocks, hipStream_t st, const T* dw) {
  if (!p->flow || !p->d_flow) return set_error(p->ctx, SRMAP_EINVAL, "internal: no displacement field set");
  if (dw != nullptr && y == nullptr) return set_error(p->ctx, SRMAP_EINVAL, "internal: data weights without observations");
  dim3 grid((g.w * g.h + 255) / 256, g.C, nk);
  const double cost_scale = (double)g.s * (double)g.s;
  if (dw != nullptr)
    hipLaunchKernelGGL((k_forward_flow<T, true>), grid, dim3(256), 0, st, x, y, out, partials, g, (const T*)p->d_flow,
                       (const T*)p->d_blur, p->d_col_map, p->d_row_map, k0, cost_scale, obs_C, obs_c0, dw);
  else
    hipLaunchKernelGGL((k_forward_flow<T, false>), grid, dim3(256), 0, st, x, y, out, partials, g, (const T*)p->d_flow,
                       (const T*)p->d_blur, p->d_col_map, p->d_row_map, k0, cost_scale, obs_C, obs_c0, dw);
  if (nblocks) *nblocks = (int)(grid.x * grid.y * grid.z);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// ---------------------------------------------------------------------------
// g = (accumulate ? g : 0) + out_scale * sum_k M_k^T B^T D^T r_k at every HR pixel: frames in increasing order, per frame
// the 5 x 5 candidates q around the seed in row-major order.  SC: the scale at compile time (2, 3, 4; 0 = run time).
template <typename T, int SC>
__global__ __launch_bounds__(256) void k_gather_flow(const T* __restrict__ resid, T* __restrict__ gout, Geometry g,
                                                    const T* __restrict__ flow, const int* __restrict__ seeds,
                                                    const T* __restrict__ blur_t, int k0, int nk, T out_scale,
                                                    int accumulate) {
  const int gs = SC ? SC : g.s;
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const int N = g.W * g.H, n = g.w * g.h;
  if (hp >= N) return;
  const int r = hp / g.W, col = hp - r * g.W;
  T acc = T(0);
  for (int kk = 0; kk < nk; ++kk) {
    const size_t kb = (size_t)(k0 + kk);  // uniform bases
    const T* __restrict__ fux = flow + kb * 2 * N;
    const T* __restrict__ fuy = fux + N;
    const T* rk = resid + ((size_t)kk * g.C + c) * n;
    int qxs, qys;
    flow_unpack_seed(seeds[kb * N + hp], g.W, &qxs, &qys);
    T tk = T(0);
    for (int dy = -kFlowRadius; dy <= kFlowRadius; ++dy) {
      const int qy = qys + dy;
      if (qy < 0 || qy >= g.H) continue;
      for (int dx = -kFlowRadius; dx <= kFlowRadius; ++dx) {
        const int qx = qxs + dx;
        if (qx < 0 || qx >= g.W) continue;
        const size_t qi = (size_t)qy * g.W + qx;
        const double wx = affine_axis_weight(flow_source(qx, fux[qi]), col);
        if (wx == 0.0) continue;
        const double wd = affine_axis_weight(flow_source(qy, fuy[qi]), r) * wx;
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
int launch_gather_flow(srmap_problem* p, const Geometry& geo, const T* resid, T* g, int k0, int nk, double out_scale,
                       bool accumulate, hipStream_t st) {
  if (!p->flow || !p->d_flow || !p->d_flow_seed) return set_error(p->ctx, SRMAP_EINVAL, "internal: no displacement field set");
  dim3 grid((unsigned)(((size_t)geo.W * geo.H + 255) / 256), geo.C);
  const T* bt = (const T*)p->d_blur_t;
  const int acc1 = accumulate ? 1 : 0;
#define SRMAP_GATHER_FLOW(SS)                                                                                      \
  hipLaunchKernelGGL((k_gather_flow<T, SS>), grid, dim3(256), 0, st, resid, g, geo, (const T*)p->d_flow, p->d_flow_seed, \
                     bt, k0, nk, (T)out_scale, acc1)
  if (geo.s == 2) SRMAP_GATHER_FLOW(2);
  else if (geo.s == 3) SRMAP_GATHER_FLOW(3);
  else if (geo.s == 4) SRMAP_GATHER_FLOW(4);
  else SRMAP_GATHER_FLOW(0);
#undef SRMAP_GATHER_FLOW
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// ---------------------------------------------------------------------------
// Set time.  seeds[k][p] = the fixed point (or the kFlowSeedSteps-th iterate) of q <- round(p - u_k(clamp(q))) from q = p,
// clamped to the image widened by kFlowPad and packed.  A value that is not finite or beyond 2^20 ends the iteration (the
// check kernel reports it; the seed only has to be a valid int).
template <typename T>
__global__ __launch_bounds__(256) void k_flow_seed(const T* __restrict__ flow, int* __restrict__ seeds, int W, int H) {
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  const int N = W * H;
  if (hp >= N) return;
  const T* __restrict__ fux = flow + (size_t)k * 2 * N;  // uniform bases
  const T* __restrict__ fuy = fux + N;
  const int r = hp / W, col = hp - r * W;
  int qx = col, qy = r;
  for (int it = 0; it < kFlowSeedSteps; ++it) {
    const int cx = min(max(qx, 0), W - 1), cy = min(max(qy, 0), H - 1);
    const size_t qi = (size_t)cy * W + cx;
    const double ux = (double)fux[qi], uy = (double)fuy[qi];
    if (!(__builtin_fabs(ux) <= kFlowMaxDisp && __builtin_fabs(uy) <= kFlowMaxDisp)) break;
    const int nx = (int)__builtin_rint((double)col - ux), ny = (int)__builtin_rint((double)r - uy);
    if (nx == qx && ny == qy) break;
    qx = nx;
    qy = ny;
  }
  qx = min(max(qx, -kFlowPad), W - 1 + kFlowPad);
  qy = min(max(qy, -kFlowPad), H - 1 + kFlowPad);
  seeds[(size_t)k * N + hp] = flow_pack_seed(qx, qy, W);
}

// The forward direction, per pixel q of frame k: counts {entries that are not finite, entries beyond 2^20, taps p of q
// (inside the image, weight not zero: the pairs the forward kernel multiplies) whose gather window does not contain q};
// one record of three partials per workgroup, part[j * nblk + block].
template <typename T>
__global__ __launch_bounds__(256) void k_flow_check(const T* __restrict__ flow, const int* __restrict__ seeds, int W, int H,
                                                   double* __restrict__ part, int part_stride) {
  __shared__ double red[3][4];
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  const int N = W * H;
  double bad_nan = 0.0, bad_big = 0.0, bad_win = 0.0;
  if (hp < N) {
    const T* __restrict__ fux = flow + (size_t)k * 2 * N;  // uniform bases
    const T* __restrict__ fuy = fux + N;
    const int* __restrict__ sk = seeds + (size_t)k * N;
    const int qy = hp / W, qx = hp - qy * W;
    const T ux = fux[hp], uy = fuy[hp];
    const double ax = __builtin_fabs((double)ux), ay = __builtin_fabs((double)uy);
    if (!(ax < __builtin_inf() && ay < __builtin_inf())) bad_nan = 1.0;
    else if (ax > kFlowMaxDisp || ay > kFlowMaxDisp) bad_big = 1.0;
    else {
      const double sx = flow_source(qx, ux), sy = flow_source(qy, uy);
      if (sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H) {  // affine_sample's test: some tap inside
        const int x0 = (int)__builtin_floor(sx), y0 = (int)__builtin_floor(sy);
        for (int ty = 0; ty < 2; ++ty) {
          const int py = y0 + ty;
          if (py < 0 || py >= H) continue;
          const double wy = affine_axis_weight(sy, py);
          for (int tx = 0; tx < 2; ++tx) {
            const int px = x0 + tx;
            if (px < 0 || px >= W) continue;
            if (wy * affine_axis_weight(sx, px) == 0.0) continue;
            int qxs, qys;
            flow_unpack_seed(sk[(size_t)py * W + px], W, &qxs, &qys);
            if (abs(qx - qxs) > kFlowRadius || abs(qy - qys) > kFlowRadius) bad_win += 1.0;
          }
        }
      }
    }
  }
  const double s0 = block_sum_256(bad_nan, red[0]);
  const double s1 = block_sum_256(bad_big, red[1]);
  const double s2 = block_sum_256(bad_win, red[2]);
  if (threadIdx.x == 0) {
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[b] = s0;
    part[(size_t)part_stride + b] = s1;
    part[2 * (size_t)part_stride + b] = s2;
  }
}

// Seeds for the field `flow` ([K][2][H][W] of T, device) into `seeds`, and the three counts of k_flow_check into
// counts_host: enqueued on st and waited for.
template <typename T>
static int flow_seed_and_check(srmap_problem* p, const T* flow, int* seeds, double counts_host[3], hipStream_t st) {
  const Geometry& g = p->geo;
  const int N = g.W * g.H;
  dim3 grid((unsigned)((N + 255) / 256), g.K);
  const int nblk = (int)(grid.x * grid.y);
  const int stride = nblk + reduce_scratch_slots((size_t)nblk) + 8;  // partials + launch_reduce_partials' second stage
  double* d_part = nullptr;
  SRMAP_HIP(p->ctx, hipMalloc((void**)&d_part, ((size_t)3 * stride + 3) * sizeof(double)));
  double* d_counts = d_part + (size_t)3 * stride;
  hipLaunchKernelGGL(k_flow_seed<T>, grid, dim3(256), 0, st, flow, seeds, g.W, g.H);
  hipLaunchKernelGGL(k_flow_check<T>, grid, dim3(256), 0, st, flow, (const int*)seeds, g.W, g.H, d_part, stride);
  int rc = SRMAP_OK;
  for (int j = 0; j < 3 && rc == SRMAP_OK; ++j)
    rc = launch_reduce_partials(p, d_part + (size_t)j * stride, nblk, d_counts + j, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(counts_host, d_counts, 3 * sizeof(double), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  (void)hipFree(d_part);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, e);
  SRMAP_HIP(p->ctx, e2);
  return SRMAP_OK;
}

// flow_dev != nullptr: the field in the problem's dtype on the device (read on st); else flow_host (doubles, rounded once)
static int flow_set(srmap_problem* p, const double* flow_host, const void* flow_dev, hipStream_t st) {
  srmap_ctx* ctx = p->ctx;
  const Geometry& g = p->geo;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)g.W * g.H, n = (size_t)g.K * 2 * N;
  void* nf = nullptr;
  int* ns = nullptr;
  const bool set = flow_host != nullptr || flow_dev != nullptr;
  if (set) {
    if (((size_t)g.W + 2 * kFlowPad) * ((size_t)g.H + 2 * kFlowPad) >= ((size_t)1 << 31))
      return set_error(ctx, SRMAP_EUNSUPPORTED, "displacement field: an image of %d x %d is beyond the packed seed's range", g.W, g.H);
    if (hipMalloc(&nf, n * p->elem()) != hipSuccess || hipMalloc((void**)&ns, (size_t)g.K * N * sizeof(int)) != hipSuccess) {
      if (nf) (void)hipFree(nf);
      (void)hipGetLastError();
      return set_error(ctx, SRMAP_ENOMEM, "hipMalloc failed (displacement field: %zu bytes, seeds: %zu bytes)", n * p->elem(),
                       (size_t)g.K * N * sizeof(int));
    }
    auto fail = [&](int code) { (void)hipFree(nf); (void)hipFree(ns); return code; };
    int rc = SRMAP_OK;
    if (flow_dev) {
      if (hipMemcpyAsync(nf, flow_dev, n * p->elem(), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(set_error(ctx, SRMAP_EHIP, "copying the displacement field failed"));
    } else {
      rc = convert_upload(p, flow_host, nf, n, st);
      if (rc) return fail(rc);
    }
    double counts[3] = {0.0, 0.0, 0.0};
    rc = p->dtype == SRMAP_F32 ? flow_seed_and_check<float>(p, (const float*)nf, ns, counts, st)
                               : flow_seed_and_check<double>(p, (const double*)nf, ns, counts, st);
    if (rc) return fail(rc);
    // the problem keeps the motion it had
    if (counts[0] != 0.0)
      return fail(set_error(ctx, SRMAP_EINVAL, "displacement field: %.0f entries are not finite in the problem's dtype", counts[0]));
    if (counts[1] != 0.0)
      return fail(set_error(ctx, SRMAP_EUNSUPPORTED, "displacement field: %.0f entries exceed 2^20 pixels", counts[1]));
    if (counts[2] != 0.0)
      return fail(set_error(ctx, SRMAP_EUNSUPPORTED,
                            "displacement field: %.0f (pixel, tap) pairs lie outside the transpose's %d x %d gather window (the field "
                            "folds, or its neighbour differences exceed the documented bound)",
                            counts[2], 2 * kFlowRadius + 1, 2 * kFlowRadius + 1));
  }
  // evaluations in flight read the field: drain them before the buffers change
  if (p->use_stream) SRMAP_HIP(ctx, hipStreamSynchronize(p->use_stream));
  SRMAP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (p->d_flow) (void)hipFree(p->d_flow);
  if (p->d_flow_seed) (void)hipFree(p->d_flow_seed);
  p->d_flow = nf;
  p->d_flow_seed = ns;
  p->flow = set;
  p->affine = false;  // alternatives: a flow replaces an affine motion, and NULL restores the created motion
  p->affine_recs.clear();
  p->plan_gen++;
  if (ztile_plan(p)) ztile_preload(p);  // "not covered" while a flow is set
  return SRMAP_OK;
}

#define INSTANTIATE_FLOW(T)                                                                                            \
  template int launch_forward_flow<T>(srmap_problem*, const Geometry&, const T*, const T*, int, int, T*, int, int,    \
                                      double*, int*, hipStream_t, const T*);                                           \
  template int launch_gather_flow<T>(srmap_problem*, const Geometry&, const T*, T*, int, int, double, bool, hipStream_t);
INSTANTIATE_FLOW(float)
INSTANTIATE_FLOW(double)

}  // namespace srmap

using namespace srmap;

extern "C" int srmap_problem_set_flow(srmap_problem* p, const double* flow_host) {
  if (!p) return SRMAP_EINVAL;
  return flow_set(p, flow_host, nullptr, p->ctx->stream);
}

extern "C" int srmap_problem_set_flow_device(srmap_problem* p, const void* flow_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  return flow_set(p, nullptr, flow_dev, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

extern "C" int srmap_problem_get_flow(srmap_problem* p, double* flow_out, int* is_set) {
  if (!p) return SRMAP_EINVAL;
  if (is_set) *is_set = p->flow ? 1 : 0;
  if (!flow_out || !p->flow) return SRMAP_OK;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_download(p, p->d_flow, flow_out, (size_t)p->geo.K * 2 * p->geo.W * p->geo.H, p->ctx->stream);
}
