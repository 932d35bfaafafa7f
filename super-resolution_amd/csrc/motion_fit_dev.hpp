// motion_fit_dev.hpp -- device inlines shared by sample_dev.hpp, registration.hip, registration_affine.hip and
// motion_refinement.hip: the sample-position expression of the affine model and the fixed-order reductions of the fits.
#pragma once

#include <hip/hip_runtime.h>

#include "reduce_dev.hpp"

namespace srmap {

// m0 * x + (m1 * y + m2) with every operation rounded on its own: no contraction into fused multiply-adds, so that a host
// restatement in plain double arithmetic (tests/affine_restatement.py) forms bit-identical coordinates and weights --
// one ulp of a coordinate at 260 px is 6e-14 of a weight, which a gradient element of size 60 shows as 3e-12.
// THE sample position of every kernel of the affine model: the warp, its transpose, the registration and the refinement.
__device__ __forceinline__ double affine_coord(double m0, double m1, double m2, double x, double y) {
#pragma clang fp contract(off)
  const double t = m1 * y + m2;
  return m0 * x + t;
}

// record[q] = sum of acc[q] over the 256 threads of the workgroup, q < N <= 256: a wave shuffle, then the four wave sums
// through `red` (LDS) in the fixed order (w0 + w1) + (w2 + w3).  Every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ void fold_sums_256(const double (&acc)[N], double (&red)[N][4], double* __restrict__ record) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const double s = wave_sum(acc[q]);
    if (lane == 0) red[q][wv] = s;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int q = threadIdx.x;
    record[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

}  // namespace srmap
