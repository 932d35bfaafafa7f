// motion_fit.hip -- what the motion fits share on the device side (registration.hip, registration_affine.hip,
// motion_refinement.hip): the box-pyramid kernel, the chunk reduction of the per-workgroup sums and the owner of the
// per-pass buffers (FitPass, srmap_internal.hpp).  The sums kernels stay with their fit.
#include <algorithm>

#include "affine_map.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

// dst[k][h2][w2] = mean of the 2 x 2 blocks of src[k][h][w] (w2 = w / 2, h2 = h / 2), blockIdx.y = k
__global__ __launch_bounds__(256) void k_down2_stack(const double* __restrict__ src, double* __restrict__ dst, int w, int h,
                                                     int w2, int h2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w2 * h2) return;
  const int r = i / w2, c = i - r * w2;
  const double* s = src + (size_t)blockIdx.y * w * h + (size_t)(2 * r) * w + 2 * c;
  dst[(size_t)blockIdx.y * w2 * h2 + i] = 0.25 * ((s[0] + s[1]) + (s[w] + s[w + 1]));
}

// sums[f][nsums] = the chunk records partial[(f * chunks + k)][nsums] of frame f added in index order; a frame whose
// active flag is 0 keeps its sums.  grid = frames, 64 threads (nsums <= 64).
__global__ __launch_bounds__(64) void k_fit_reduce(const double* __restrict__ partial, int chunks, int nsums,
                                                   const double* __restrict__ table, double* __restrict__ sums) {
  const int f = blockIdx.x, q = threadIdx.x;
  if (table[(size_t)f * kFitTabRec + 6] == 0.0 || q >= nsums) return;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += partial[((size_t)f * chunks + k) * nsums + q];
  sums[(size_t)f * nsums + q] = s;
}

}  // namespace

void launch_down2_stack(const double* src, double* dst, int w, int h, int frames, hipStream_t st) {
  const int w2 = w / 2, h2 = h / 2, n = w2 * h2;
  hipLaunchKernelGGL(k_down2_stack, dim3((n + 255) / 256, frames), dim3(256), 0, st, src, dst, w, h, w2, h2);
}

bool FitPass::alloc(int frames_, int nsums_, size_t part_elems) {
  frames = frames_;
  nsums = nsums_;
  return nsums <= 64 &&
         d_part.alloc(part_elems * sizeof(double)) == hipSuccess &&
         d_tab.alloc((size_t)frames * kFitTabRec * sizeof(double)) == hipSuccess &&
         d_sums.alloc((size_t)frames * nsums * sizeof(double)) == hipSuccess &&
         h_tab.alloc((size_t)frames * kFitTabRec * sizeof(double)) == hipSuccess &&
         h_sums.alloc((size_t)frames * nsums * sizeof(double)) == hipSuccess;
}

void FitPass::set(int frame, const AffineMap& M, bool active) {
  double* rec = h_tab.as<double>() + (size_t)frame * kFitTabRec;
  std::copy(M.m, M.m + 6, rec);
  rec[6] = active ? 1.0 : 0.0;
  rec[7] = 0.0;
}

bool FitPass::upload(hipStream_t st) {
  return hipMemcpyAsync(d_tab.as(), h_tab.as(), (size_t)frames * kFitTabRec * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
}

bool FitPass::reduce_and_fetch(int chunks, hipStream_t st) {
  hipLaunchKernelGGL(k_fit_reduce, dim3(frames), dim3(64), 0, st, d_part.as<double>(), chunks, nsums, d_tab.as<double>(), d_sums.as<double>());
  return hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(h_sums.as(), d_sums.as(), (size_t)frames * nsums * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
}

}  // namespace srmap
