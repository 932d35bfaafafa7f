// kernels_reduce.hip -- the final reduction of the per-block cost partials that the evaluation kernels leave (eval.hip,
// kernels_flow.hip).
#include "reduce_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

// Deterministic final reduction of per-block partials, fixed order.  out[0] = sum.
// Up to kReduceChunk partials: one 256-thread block.  More (multi-channel images: one partial per tile and
// channel -- cfg5 has half a million): first one block per chunk of kReduceChunk partials into a scratch tail
// behind the partials, then one block over the chunk sums.  A single block over 73 K partials took 36 us.
constexpr int kReduceChunk = 4096;

__global__ __launch_bounds__(256) void k_reduce_partials(const double* __restrict__ partials,
                                                        int n, double* __restrict__ out) {
  __shared__ double red[4];
  const int i0 = blockIdx.x * kReduceChunk;
  const int i1 = (gridDim.x == 1) ? n : (i0 + kReduceChunk < n ? i0 + kReduceChunk : n);
  double v = 0.0;
  for (int i = i0 + threadIdx.x; i < i1; i += 256) v += partials[i];
  const double s = block_sum_256(v, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

int reduce_scratch_slots(size_t n) { return (int)((n + kReduceChunk - 1) / kReduceChunk); }

// `partials` must have room for n + reduce_scratch_slots(n) doubles.
int launch_reduce_partials(srmap_problem* p, const double* partials, int n, double* out,
                           hipStream_t st) {
  if (n <= kReduceChunk) {
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, partials, n, out);
  } else {
    const int nb = reduce_scratch_slots((size_t)n);
    double* scratch = const_cast<double*>(partials) + n;
    hipLaunchKernelGGL(k_reduce_partials, dim3(nb), dim3(256), 0, st, partials, n, scratch);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, (const double*)scratch, nb, out);
  }
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

}  // namespace srmap
