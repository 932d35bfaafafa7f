// reduce_dev.hpp -- the device inlines every kernel file shares: the 64-lane wave reductions, the fixed-order
// combination of a 256-thread workgroup's four wave results, and the 16-byte vector load / store of the n-vector passes.
// One copy: the order of the additions is part of what the tests pin bit for bit.  (The tile kernel's finisher keeps its
// own DPP reduction, ztile_dev.hpp.)
#pragma once

#include <hip/hip_runtime.h>

namespace srmap {

// sum / max over the 64 lanes of a wave; valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}

// the four wave results of a 256-thread workgroup in THE fixed order (w0 + w1) + (w2 + w3), or their max
__device__ __forceinline__ double combine4(const double (&r)[4], bool mx) {
  return mx ? fmax(fmax(r[0], r[1]), fmax(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
}

// Sum over a 256-thread block; result valid in thread 0.
__device__ __forceinline__ double block_sum_256(double v, double* smem4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) smem4[wid] = v;
  __syncthreads();
  double r = 0;
  if (threadIdx.x == 0) r = (smem4[0] + smem4[1]) + (smem4[2] + smem4[3]);
  return r;
}

// Cache policy of the n-vector passes.  What an EVALUATION touches -- x, the observations, the IRLS weights, the
// direction d (its g.d), g -- and the line search's base point xk (read for every trial point) should survive in the
// 256 MiB Infinity Cache from one evaluation to the next: 201 MB at cfg2.  The vectors only the solver's update itself
// streams (dn / dk, the previous gradient gp, the L-BFGS history) are read and written NON-TEMPORAL so that they do not
// displace that set (profiles/r03_solve_trace.txt: the evaluation ran 51.7 us inside the solve against 39.9 us alone).
// V consecutive elements as one request (V * sizeof(T) <= 16 bytes, p aligned to it); STREAM = non-temporal
template <typename T, int V, bool STREAM>
__device__ __forceinline__ void ldv(const T* __restrict__ p, T (&out)[V]) {
  typedef T __attribute__((ext_vector_type(V))) VT;
  if constexpr (V == 1) {
    out[0] = STREAM ? __builtin_nontemporal_load(p) : *p;
  } else {
    const VT v = STREAM ? __builtin_nontemporal_load(reinterpret_cast<const VT*>(p)) : *reinterpret_cast<const VT*>(p);
#pragma unroll
    for (int q = 0; q < V; ++q) out[q] = v[q];
  }
}
template <typename T, int V, bool STREAM>
__device__ __forceinline__ void stv(T* __restrict__ p, const T (&in)[V]) {
  typedef T __attribute__((ext_vector_type(V))) VT;
  if constexpr (V == 1) {
    if (STREAM) __builtin_nontemporal_store(in[0], p); else *p = in[0];
  } else {
    VT v;
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = in[q];
    if (STREAM) __builtin_nontemporal_store(v, reinterpret_cast<VT*>(p)); else *reinterpret_cast<VT*>(p) = v;
  }
}

}  // namespace srmap
