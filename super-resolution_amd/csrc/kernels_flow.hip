// kernels_flow.hip -- the set-time side of the per-frame displacement field, DENSE (srmap_problem_set_flow) or on a
// CONTROL LATTICE (srmap_problem_set_flow_lattice); no reference counterpart: motion_module.cpp:18-51 warps by a
// translation only.  DESIGN.md 3.11, 3.16.
//
// Frame k carries a field u_k = (ux, uy) on its HR-grid image, stored in the problem's dtype as [K][2][H][W].  The forward
// warp samples x bilinearly at s = q + u_k(q) for every pixel q of the warped image (taps outside the image contribute 0:
// affine_sample); blur and decimation are the translational path's.  s = (double)q + (double)u is exact in double for
// both dtypes (|u| <= 2^20), and the weights are the double products rounded to T, as in the affine model.  The kernels
// that evaluate it are k_forward_direct and k_gather_sampled (kernels_data_direct.hip) through MotionSampler's flow kind
// (sample_dev.hpp).
//
// The transpose is the EXACT transpose of that matrix in gather form.  For an HR pixel p the contributing q are those with
// q + u(q) strictly inside p +- 1 per axis.  They are found through a SEED stored per (k, p) when the field is set
// (k_flow_seed: the fixed-point iteration q <- round(p - u(clamp(q)))): the gather scans the 5 x 5 window around the seed
// and recomputes each candidate's weight from s by the forward kernel's expressions (flow_source, affine_axis_weight), so
// the two kernels hold the same matrix bit for bit and no atomics are needed.  That every (q, p) pair of the matrix lies
// inside p's window is VERIFIED when the field is set (k_flow_check walks the forward direction), not assumed: a field
// that folds or shears beyond the window is refused and never reaches those kernels.
//
// A lattice keeps lw x lh nodes per component and frame, step HR pixels apart, as doubles in both dtypes; u_k(q) is their
// bilinear interpolant rounded once to the dtype (LatticeField, sample_dev.hpp).  From u_k(q) on everything above is
// unchanged: the seed and check kernels below are templates over the READER of u (DenseField / LatticeField), the seeds
// stay a [K][H][W] table, and a lattice problem evaluates bit for bit as a dense one given the expanded nodes.
#include <algorithm>
#include <cmath>

#include "reduce_dev.hpp"
#include "sample_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

constexpr int kFlowSeedSteps = 16;         // fixed-point steps of k_flow_seed (it stops early at a fixed point)
constexpr double kFlowMaxDisp = 1048576.0; // 2^20

// flow_pack_seed / flow_unpack_seed, kFlowPad: sample_dev.hpp (shared with the gather)

// The reader of a dense field: frame k's planes of flow[K][2][H][W]; (flat pixel index, x, y) as LatticeField
template <typename T>
struct DenseField {
  const T* __restrict__ fux;
  const T* __restrict__ fuy;
  __device__ __forceinline__ T ux(size_t qi, int, int) const { return fux[qi]; }
  __device__ __forceinline__ T uy(size_t qi, int, int) const { return fuy[qi]; }
};
// reader of frame k (uniform bases) from the kernel argument of its form: the dense field, or the lattice
template <typename T>
__device__ __forceinline__ DenseField<T> field_of(const T* __restrict__ flow, int k, int N) {
  const T* fux = flow + (size_t)k * 2 * N;
  return {fux, fux + N};
}
template <typename T>
__device__ __forceinline__ LatticeField<T> field_of(const LatticeDesc& lat, int k, int) {
  return LatticeField<T>(lat, k);
}

}  // namespace

// ---------------------------------------------------------------------------
// Set time.  seeds[k][p] = the fixed point (or the kFlowSeedSteps-th iterate) of q <- round(p - u_k(clamp(q))) from q = p,
// clamped to the image widened by kFlowPad and packed.  A value that is not finite or beyond 2^20 ends the iteration (the
// check kernel reports it; the seed only has to be a valid int).
// FIELD: the kernel argument u is read from -- const T* (dense) or LatticeDesc.
template <typename T, typename FIELD>
__global__ __launch_bounds__(256) void k_flow_seed(FIELD flow, int* __restrict__ seeds, int W, int H) {
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  const int N = W * H;
  if (hp >= N) return;
  const auto f = field_of<T>(flow, k, N);
  const int r = hp / W, col = hp - r * W;
  int qx = col, qy = r;
  for (int it = 0; it < kFlowSeedSteps; ++it) {
    const int cx = min(max(qx, 0), W - 1), cy = min(max(qy, 0), H - 1);
    const size_t qi = (size_t)cy * W + cx;
    const double ux = (double)f.ux(qi, cx, cy), uy = (double)f.uy(qi, cx, cy);
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
template <typename T, typename FIELD>
__global__ __launch_bounds__(256) void k_flow_check(FIELD flow, const int* __restrict__ seeds, int W, int H,
                                                   double* __restrict__ part, int part_stride) {
  __shared__ double red[3][4];
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  const int N = W * H;
  double bad_nan = 0.0, bad_big = 0.0, bad_win = 0.0;
  if (hp < N) {
    const auto f = field_of<T>(flow, k, N);
    const int* __restrict__ sk = seeds + (size_t)k * N;
    const int qy = hp / W, qx = hp - qy * W;
    const T ux = f.ux((size_t)hp, qx, qy), uy = f.uy((size_t)hp, qx, qy);
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

// Seeds for the field `flow` ([K][2][H][W] of T on the device, or a lattice's description) into `seeds`, and the three
// counts of k_flow_check into counts_host: enqueued on st and waited for.
template <typename T, typename FIELD>
static int flow_seed_and_check(srmap_problem* p, FIELD flow, int* seeds, double counts_host[3], hipStream_t st) {
  const Geometry& g = p->geo;
  const int N = g.W * g.H;
  dim3 grid((unsigned)((N + 255) / 256), g.K);
  const int nblk = (int)(grid.x * grid.y);
  const int stride = nblk + reduce_scratch_slots((size_t)nblk) + 8;  // partials + launch_reduce_partials' second stage
  DevBuf part;  // the kernels below write it: the stream is waited for on every path before it goes out of scope
  SRMAP_HIP(p->ctx, part.alloc(((size_t)3 * stride + 3) * sizeof(double)));
  double* d_part = part.as<double>();
  double* d_counts = d_part + (size_t)3 * stride;
  hipLaunchKernelGGL((k_flow_seed<T, FIELD>), grid, dim3(256), 0, st, flow, seeds, g.W, g.H);
  hipLaunchKernelGGL((k_flow_check<T, FIELD>), grid, dim3(256), 0, st, flow, (const int*)seeds, g.W, g.H, d_part, stride);
  int rc = SRMAP_OK;
  for (int j = 0; j < 3 && rc == SRMAP_OK; ++j)
    rc = launch_reduce_partials(p, d_part + (size_t)j * stride, nblk, d_counts + j, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(counts_host, d_counts, 3 * sizeof(double), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  if (rc) return rc;
  SRMAP_HIP(p->ctx, e);
  SRMAP_HIP(p->ctx, e2);
  return SRMAP_OK;
}

// The answer to the three counts of k_flow_check for a field called `what`; the problem keeps the motion it had
static int flow_counts_answer(srmap_ctx* ctx, const char* what, const double counts[3]) {
  if (counts[0] != 0.0)
    return set_error(ctx, SRMAP_EINVAL, "%s: %.0f entries are not finite in the problem's dtype", what, counts[0]);
  if (counts[1] != 0.0)
    return set_error(ctx, SRMAP_EUNSUPPORTED, "%s: %.0f entries exceed 2^20 pixels", what, counts[1]);
  if (counts[2] != 0.0)
    return set_error(ctx, SRMAP_EUNSUPPORTED,
                     "%s: %.0f (pixel, tap) pairs lie outside the transpose's %d x %d gather window (the field "
                     "folds, or its neighbour differences exceed the documented bound)",
                     what, counts[2], 2 * kFlowRadius + 1, 2 * kFlowRadius + 1);
  return SRMAP_OK;
}

static int flow_seed_range(srmap_problem* p) {
  const Geometry& g = p->geo;
  if (((size_t)g.W + 2 * kFlowPad) * ((size_t)g.H + 2 * kFlowPad) >= ((size_t)1 << 31))
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "displacement field: an image of %d x %d is beyond the packed seed's range", g.W, g.H);
  return SRMAP_OK;
}

// flow_dev != nullptr: the field in the problem's dtype on the device (read on st); else flow_host (doubles, rounded once)
static int flow_set(srmap_problem* p, const double* flow_host, const void* flow_dev, hipStream_t st) {
  srmap_ctx* ctx = p->ctx;
  const Geometry& g = p->geo;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)g.W * g.H, n = (size_t)g.K * 2 * N;
  MotionModel::Replacement r;  // the new field and its seeds: built here, installed once they are valid
  if (flow_host != nullptr || flow_dev != nullptr) {
    if (int rc = flow_seed_range(p)) return rc;
    if (r.d_flow.alloc(n * p->elem()) != hipSuccess || r.d_seeds.alloc((size_t)g.K * N * sizeof(int)) != hipSuccess)
      return set_error(ctx, SRMAP_ENOMEM, "hipMalloc failed (displacement field: %zu bytes, seeds: %zu bytes)", n * p->elem(),
                       (size_t)g.K * N * sizeof(int));
    int rc = SRMAP_OK;
    if (flow_dev) {
      if (hipMemcpyAsync(r.d_flow.as(), flow_dev, n * p->elem(), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return set_error(ctx, SRMAP_EHIP, "copying the displacement field failed");
    } else {
      rc = convert_upload(p, flow_host, r.d_flow.as(), n, st);
      if (rc) return rc;
    }
    double counts[3] = {0.0, 0.0, 0.0};
    rc = dispatch_dtype(p->dtype, [&](auto t) {
      using T = decltype(t);
      return flow_seed_and_check<T, const T*>(p, r.d_flow.as<const T>(), r.d_seeds.as<int>(), counts, st);
    });
    if (rc) return rc;
    if (int rc2 = flow_counts_answer(ctx, "displacement field", counts)) return rc2;
    r.kind = kMotionFlow;
  }
  return p->motion.install(p, std::move(r));  // empty when the call clears the flow
}

// The lattice form: nodes [K][2][lh][lw] doubles, on the device (read on st) or on the host; both NULL restores the created
// motion.  The nodes are kept as doubles in both dtypes; u is read through LatticeField by the kernels above
static int lattice_set(srmap_problem* p, int step, int lw, int lh, const double* nodes_host, const double* nodes_dev, hipStream_t st) {
  srmap_ctx* ctx = p->ctx;
  const Geometry& g = p->geo;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  MotionModel::Replacement r;
  if (nodes_host != nullptr || nodes_dev != nullptr) {
    if (step < 1 || step > kLatticeMaxStep) return set_error(ctx, SRMAP_EINVAL, "flow lattice: step %d is outside 1 ... %d", step, kLatticeMaxStep);
    if (lw < 2 || lh < 2) return set_error(ctx, SRMAP_EINVAL, "flow lattice: %d x %d nodes (at least 2 x 2)", lw, lh);
    if ((long long)(lw - 1) * step >= (long long)g.W + step || (long long)(lh - 1) * step >= (long long)g.H + step)
      return set_error(ctx, SRMAP_EINVAL, "flow lattice: %d x %d nodes at step %d reach more than a cell beyond the %d x %d image", lw, lh, step, g.W, g.H);
    if (int rc = flow_seed_range(p)) return rc;
    const size_t N = (size_t)g.W * g.H, bytes = (size_t)g.K * 2 * lw * lh * sizeof(double);
    if (r.d_lattice.alloc(bytes) != hipSuccess || r.d_seeds.alloc((size_t)g.K * N * sizeof(int)) != hipSuccess)
      return set_error(ctx, SRMAP_ENOMEM, "hipMalloc failed (flow lattice: %zu bytes, seeds: %zu bytes)", bytes, (size_t)g.K * N * sizeof(int));
    if (hipMemcpyAsync(r.d_lattice.as(), nodes_dev ? nodes_dev : nodes_host, bytes, nodes_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st) != hipSuccess)
      return set_error(ctx, SRMAP_EHIP, "copying the flow lattice failed");
    const LatticeDesc lat = {r.d_lattice.as<const double>(), step, lw, lh};
    double counts[3] = {0.0, 0.0, 0.0};
    int rc = dispatch_dtype(p->dtype, [&](auto t) { return flow_seed_and_check<decltype(t), LatticeDesc>(p, lat, r.d_seeds.as<int>(), counts, st); });
    if (rc) return rc;
    if (int rc2 = flow_counts_answer(ctx, "flow lattice (the interpolated field)", counts)) return rc2;
    r.kind = kMotionLattice; r.step = step; r.lw = lw; r.lh = lh;
  }
  return p->motion.install(p, std::move(r));
}

}  // namespace srmap

using namespace srmap;

extern "C" int srmap_problem_set_flow(srmap_problem* p, const double* flow_host) {
  if (!p) return SRMAP_EINVAL;
  return flow_set(p, flow_host, nullptr, p->ctx->stream);
}

extern "C" int srmap_problem_set_flow_device(srmap_problem* p, const void* flow_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  return flow_set(p, nullptr, flow_dev, stream_of(p->ctx, hip_stream));
}

extern "C" int srmap_problem_get_flow(srmap_problem* p, double* flow_out, int* is_set) {
  if (!p) return SRMAP_EINVAL;
  if (is_set) *is_set = p->motion.kind() == kMotionFlow ? 1 : 0;
  if (!flow_out || p->motion.kind() != kMotionFlow) return SRMAP_OK;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_download(p, p->motion.replacement().d_flow.as(), flow_out, (size_t)p->geo.K * 2 * p->geo.W * p->geo.H, p->ctx->stream);
}

extern "C" int srmap_problem_set_flow_lattice(srmap_problem* p, int step, int lw, int lh, const double* nodes_host) {
  if (!p) return SRMAP_EINVAL;
  return lattice_set(p, step, lw, lh, nodes_host, nullptr, p->ctx->stream);
}

extern "C" int srmap_problem_set_flow_lattice_device(srmap_problem* p, int step, int lw, int lh, const double* nodes_dev, void* hip_stream) {
  if (!p) return SRMAP_EINVAL;
  return lattice_set(p, step, lw, lh, nullptr, nodes_dev, stream_of(p->ctx, hip_stream));
}

extern "C" int srmap_problem_get_flow_lattice(srmap_problem* p, int* step, int* lw, int* lh, double* nodes_out) {
  if (!p) return SRMAP_EINVAL;
  const MotionModel::Replacement& r = p->motion.replacement();
  if (step) *step = r.step;
  if (lw) *lw = r.lw;
  if (lh) *lh = r.lh;
  if (!nodes_out || !r.step) return SRMAP_OK;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  SRMAP_HIP(p->ctx, hipMemcpyAsync(nodes_out, r.d_lattice.as(), (size_t)p->geo.K * 2 * r.lw * r.lh * sizeof(double),
                                   hipMemcpyDeviceToHost, p->ctx->stream));
  SRMAP_HIP(p->ctx, hipStreamSynchronize(p->ctx->stream));
  return SRMAP_OK;
}
