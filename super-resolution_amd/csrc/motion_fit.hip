// motion_fit.hip -- what the fits share on the device side (registration_affine.hip, registration_flow.hip,
// motion_refinement.hip, photometric_fit.hip, blur_fit.hip): the box-pyramid kernel and its level sizes, the ONE reduction of
// the per-workgroup records (k_fit_reduce) and the owner of the per-pass buffers (FitPass, srmap_internal.hpp).  The sums
// kernels stay with their fit.
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

// sums[e][nsums] = the records partial[r][nsums] of row e = blockIdx.y added in index order: `outer` groups outer_stride
// records apart, `inner` consecutive records each, from record e * row_stride on.  One thread per sum adds its records one
// after another from 0.0, which is all the result depends on.  table (may be null): a row whose active flag is 0 keeps
// its sums.  grid = (blocks of 256 sums, rows).
__global__ __launch_bounds__(256) void k_fit_reduce(const double* __restrict__ partial, int nsums, int row_stride, int outer,
                                                    int outer_stride, int inner, const double* __restrict__ table,
                                                    double* __restrict__ sums) {
  const int q = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
  if (q >= nsums || (table && table[(size_t)e * kFitTabRec + 6] == 0.0)) return;
  double s = 0.0;
  for (int o = 0; o < outer; ++o) {
    const double* __restrict__ rec = partial + ((size_t)e * row_stride + (size_t)o * outer_stride) * nsums + q;
    for (int r = 0; r < inner; ++r) s += rec[(size_t)r * nsums];
  }
  sums[(size_t)e * nsums + q] = s;
}

}  // namespace

void launch_down2_stack(const double* src, double* dst, int w, int h, int frames, hipStream_t st) {
  const int w2 = w / 2, h2 = h / 2, n = w2 * h2;
  hipLaunchKernelGGL(k_down2_stack, dim3((n + 255) / 256, frames), dim3(256), 0, st, src, dst, w, h, w2, h2);
}

void pyramid_levels(int width, int height, int min_side, int max_levels, std::vector<int>* lw, std::vector<int>* lh) {
  constexpr int kMaxLevels = 12;
  lw->assign(1, width);
  lh->assign(1, height);
  while (std::min(lw->back(), lh->back()) >= min_side && (int)lw->size() < kMaxLevels &&
         (max_levels == 0 || (int)lw->size() < max_levels)) {
    lw->push_back(lw->back() / 2);
    lh->push_back(lh->back() / 2);
  }
}

bool FitPass::alloc(int rows_, int nsums_, size_t part_elems, bool table) {
  rows = rows_;
  nsums = nsums_;
  const size_t tab_bytes = table ? (size_t)rows * kFitTabRec * sizeof(double) : 0;
  return d_part.alloc(part_elems * sizeof(double)) == hipSuccess &&
         d_sums.alloc((size_t)rows * nsums * sizeof(double)) == hipSuccess &&
         h_sums.alloc((size_t)rows * nsums * sizeof(double)) == hipSuccess &&
         (!table || (d_tab.alloc(tab_bytes) == hipSuccess && h_tab.alloc(tab_bytes) == hipSuccess));
}

void FitPass::set(int row, const AffineMap& M, bool active) {
  double* rec = h_tab.as<double>() + (size_t)row * kFitTabRec;
  std::copy(M.m, M.m + 6, rec);
  rec[6] = active ? 1.0 : 0.0;
  rec[7] = 0.0;
}

bool FitPass::upload(hipStream_t st) {
  return hipMemcpyAsync(d_tab.as(), h_tab.as(), (size_t)rows * kFitTabRec * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
}

bool FitPass::reduce_and_fetch(int row_stride, int outer, int outer_stride, int inner, hipStream_t st) {
  hipLaunchKernelGGL(k_fit_reduce, dim3((nsums + 255) / 256, rows), dim3(256), 0, st, d_part.as<double>(), nsums, row_stride, outer,
                     outer_stride, inner, d_tab.as<double>(), d_sums.as<double>());
  return hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(h_sums.as(), d_sums.as(), (size_t)rows * nsums * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
}

}  // namespace srmap
