// solver_passes.hip -- the n-vector passes of the inner solvers' control flow (solver.hip): the nonlinear CG's direction
// and beta passes, the stored normalised direction and trial points of the paths that need them, and the reduction every
// pass ends with.  (The L-BFGS update and direction passes are in kernels_lbfgs.hip.)
//
// Every n-vector (iterate, gradient, directions, line-search base point) lives in HBM and is touched only by these
// kernels and the evaluation.  Per CG iteration the n-vector work is two fused passes:
//   k_direction      dn = -g + beta dk, max|dn|, dn.dn and g.dn -- from which the
//                    host derives linminnormalized's two scale factors, g.d and
//                    d.d (cg_norm.hpp): the normalised direction d = dn s1 s2 is
//                    not re-summed, and on the tile path not even stored
//   k_beta_dots      y = g - g_prev on the fly (the gradient buffers ping-pong,
//                    mincg's yk vector is never stored), g.g, g.y; their
//                    denominator y.dk = g.dk - g_prev.dk from sums already known
// plus the trial points x = xk + stp d: formed by the evaluation itself as it
// loads its window, from dk and the device-resident norms (tile kernel, un-sharded
// solves: no n-vector pass per trial point); elsewhere k_normalize stores d (and
// the first trial point) and k_axpy_out the later ones.  Each pass reduces its sums
// in the SAME launch: every block publishes its partials as write-through
// granules, the last block of the grid adds them in index order and hands the
// results (and the arrival tag) to the host -- no one-block second kernel.
//
// Sharding.  Reductions run over the elements a rank OWNS (row band or channel
// block; everything for frame shards: struct Owned) and are all-reduced through the
// communicator by the caller (two-launch scheme: block partials, k_finish, all-reduce, k_publish).
#include "solver_passes.hpp"

#include "cg_norm.hpp"
#include "reduce_dev.hpp"

namespace srmap {

// ---- one-launch reductions -------------------------------------------------------------------------------
// an unpublished granule: kArm32 in both halves
constexpr unsigned long long kArm = ((unsigned long long)kArm32 << 32) | kArm32;
__device__ __forceinline__ unsigned long long ld_dev(const unsigned long long* q) {
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_dev(unsigned long long* q, unsigned long long v) {
  __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Block partials of up to 3 sums (row 0 a max when max0).  Two-launch scheme: part[k * gridDim.x + blockIdx.x].
// One-launch scheme: granules, and the grid's last block adds all of them -- per thread i = tid, tid + 256, ... in
// ascending order, then the wave and the four-wave combination of k_finish: the same additions in the same order as
// the two-launch scheme.  Returns true in the one thread that wrote out[] (it still owes fin_tag()).
__device__ __forceinline__ bool block_partials3(double s0, double s1, double s2, double* __restrict__ part, bool max0,
                                                int rows, const Fin& fin, double* tot = nullptr) {
  __shared__ double red[3][4];
  s0 = max0 ? wave_max(s0) : wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[0][wid] = s0; red[1][wid] = s1; red[2][wid] = s2; }
  __syncthreads();
  const int nbk = gridDim.x;
  if (threadIdx.x < 3) {
    const double v = combine4(red[threadIdx.x], threadIdx.x == 0 && max0);
    if (fin.gran == nullptr) part[(size_t)threadIdx.x * nbk + blockIdx.x] = v;
    else if ((int)threadIdx.x < rows) st_dev(fin.gran + (size_t)threadIdx.x * nbk + blockIdx.x, (unsigned long long)__double_as_longlong(v));
  }
  if (fin.gran == nullptr || (int)blockIdx.x != nbk - 1) return false;
  __syncthreads();  // red[] is reused below
  double v0 = 0, v1 = 0, v2 = 0;
  bool timed_out = false;
  for (int i = threadIdx.x; i < nbk; i += 256) {
    unsigned long long a0 = 0, a1 = 0, a2 = 0;  // +0.0 for absent rows
    // bounded like the tile kernel's finisher (~2 s): a block that never publishes ends the pass with NaN sums (the
    // host's stopping rules then end the solve) instead of hanging the stream
    for (unsigned spins = 0;; ++spins) {
      if (rows > 0) a0 = ld_dev(fin.gran + i);
      if (rows > 1) a1 = ld_dev(fin.gran + (size_t)nbk + i);
      if (rows > 2) a2 = ld_dev(fin.gran + (size_t)2 * nbk + i);
      if (a0 != kArm && a1 != kArm && a2 != kArm) break;
      if (spins > (1u << 22)) { timed_out = true; break; }
      if (spins < 64) __builtin_amdgcn_s_sleep(1); else __builtin_amdgcn_s_sleep(16);
    }
    if (timed_out) continue;   // NOT re-armed: a block that arrives late must not publish into a fresh slot
    if (rows > 0) st_dev(fin.gran + i, kArm);  // re-armed for the next pass
    if (rows > 1) st_dev(fin.gran + (size_t)nbk + i, kArm);
    if (rows > 2) st_dev(fin.gran + (size_t)2 * nbk + i, kArm);
    const double d0 = __longlong_as_double((long long)a0), d1 = __longlong_as_double((long long)a1), d2 = __longlong_as_double((long long)a2);
    v0 = max0 ? fmax(v0, d0) : v0 + d0;
    v1 += d1;
    v2 += d2;
  }
  v0 = max0 ? wave_max(v0) : wave_sum(v0);
  v1 = wave_sum(v1);
  v2 = wave_sum(v2);
  // a time-out anywhere in the block makes EVERY row NaN (fmax would drop a NaN partial of the max row): the host's
  // stopping rules end the solve, srmap_solve reports SRMAP_EHIP (sticky word fin.timeout_flag) and re-initialises the granules
  const bool any_to = __syncthreads_or(timed_out ? 1 : 0) != 0;
  if (lane == 0) { red[0][wid] = v0; red[1][wid] = v1; red[2][wid] = v2; }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  if (any_to) {
    const double qn = __builtin_nan("");
    red[0][0] = qn; red[1][0] = qn; red[2][0] = qn;
    if (fin.timeout_flag != nullptr) fin.timeout_flag[0] = 1.0;
    if (fin.timeout_host != nullptr) *(volatile double*)fin.timeout_host = 1.0;
  }
  const double t0 = combine4(red[0], max0), t1 = combine4(red[1], false), t2 = combine4(red[2], false);
  if (rows > 0) fin.out[0] = t0;
  if (rows > 1) fin.out[1] = t1;
  if (rows > 2) fin.out[2] = t2;
  if (tot != nullptr) { tot[0] = t0; tot[1] = t1; tot[2] = t2; }  // the same sums for the finishing thread's own use
  if (fin.cost_src != nullptr) fin.out[rows] = fin.cost_src[0];
  for (int i = 0; i < fin.pub_n; ++i) fin.pub_dst[i] = fin.pub_src[i];
  return true;
}
__device__ __forceinline__ void fin_tag(const Fin& fin) {
  if (fin.tag_slot != nullptr) {
    __threadfence_system();
    *(volatile double*)fin.tag_slot = fin.tag;
  }
}

// dn = -g + beta * dk ; sums: [0] max |dn| (owned), [1] dn.dn (owned), [2] g.dn (owned).  From these the host (and the
// kernels that need the normalised direction d = dn s1 s2) derive s1, s2, g.d = (g.dn s1) s2 and d.d = dn.dn s1^2 s2^2:
// the normalisation pass of rounds 1-4 (k_normalize_dots: five n-vector streams and a reduction per CG iteration, only
// to re-sum g.d and d.d over the stored d) is gone from every path; where d is needed as a vector a plain scaling pass
// (k_normalize) stores it.  norms_pub (host-mapped), when given, receives the three sums from the finishing thread
// ahead of the tag.  keep_dn: dn is read again by the evaluations (trial points formed from dn): stored with the
// default cache policy instead of non-temporal.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_direction(T* __restrict__ dn, const T* __restrict__ g,
                                                  const T* __restrict__ dk, T beta, size_t n, Owned ow,
                                                  double* __restrict__ part, Fin fin, const double* __restrict__ beta_dev,
                                                  double* norms_pub, int keep_dn) {
  // beta_dev: the beta the preceding k_beta_dots left on the device (the host queues this pass without waiting for it)
  if (beta_dev != nullptr) beta = (T)beta_dev[0];
  double mx = 0, ss = 0, gd = 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (size_t)gridDim.x * 256 * V) {
    T gi[V], di[V], v[V];
    ldv<T, V, false>(g + i, gi);
    if (dk != nullptr) ldv<T, V, true>(dk + i, di);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      v[q] = -gi[q];
      if (dk != nullptr) v[q] += beta * di[q];
    }
    if (keep_dn) stv<T, V, false>(dn + i, v); else stv<T, V, true>(dn + i, v);
#pragma unroll
    for (int q = 0; q < V; ++q)
      if (ow.has(i + q)) {
        mx = fmax(mx, fabs((double)v[q])); ss += (double)v[q] * (double)v[q]; gd += (double)gi[q] * (double)v[q];
      }
  }
  if (block_partials3(mx, ss, gd, part, true, 3, fin)) {
    if (norms_pub != nullptr) { norms_pub[0] = fin.out[0]; norms_pub[1] = fin.out[1]; norms_pub[2] = fin.out[2]; }
    fin_tag(fin);
  }
}

// Second stage: rows (<= 3) x nb partials -> out[rows] in fixed order; row 0 is a max when max0.  extra_src, when
// given, is one more device scalar (the cost of the evaluation) forwarded to out[rows].  When `tag_slot` is given
// (host-mapped memory) the kernel finally stores `tag` there behind a system-scope fence: the host polls that word
// instead of paying a stream synchronisation (tens of microseconds per wait on this runtime).
__global__ __launch_bounds__(256) void k_finish(const double* __restrict__ part, int nb, int rows, int max0,
                                               double* __restrict__ out, const double* __restrict__ extra_src,
                                               double* tag_slot, double tag) {
  __shared__ double red[3][4];
  double v0 = 0, v1 = 0, v2 = 0;
  // four partials per row and thread requested together (nb <= 1024: one round trip instead of four), added in the
  // same order as before
  constexpr int U = 4;
  for (int base = threadIdx.x; base < nb; base += 256 * U) {
    double a0[U], a1[U], a2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * 256;
      const bool in = i < nb;
      a0[u] = (in && rows > 0) ? part[i] : 0.0;
      a1[u] = (in && rows > 1) ? part[(size_t)nb + i] : 0.0;
      a2[u] = (in && rows > 2) ? part[(size_t)2 * nb + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v0 = max0 ? fmax(v0, a0[u]) : v0 + a0[u];
      v1 += a1[u];
      v2 += a2[u];
    }
  }
  v0 = max0 ? wave_max(v0) : wave_sum(v0);
  v1 = wave_sum(v1);
  v2 = wave_sum(v2);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[0][wid] = v0; red[1][wid] = v1; red[2][wid] = v2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (rows > 0) out[0] = max0 ? fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]))
                                : (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    if (rows > 1) out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    if (rows > 2) out[2] = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    if (extra_src != nullptr) out[rows] = extra_src[0];
    if (tag_slot != nullptr) {
      __threadfence_system();
      *(volatile double*)tag_slot = tag;
    }
  }
}

// dst[0..n) = src[0..n) (device scalars -> host-mapped memory), then the tag (see k_finish)
__global__ void k_publish(double* __restrict__ dst, const double* __restrict__ src, int n, double* tag_slot, double tag) {
  if (threadIdx.x == 0) {
    for (int i = 0; i < n; ++i) dst[i] = src[i];
    __threadfence_system();
    *(volatile double*)tag_slot = tag;
  }
}

// d = (dn * s1) * s2 stored as a vector, for the paths whose evaluations read the normalised direction from memory
// (sharded solves, the direct kernels, host-paced passes).  norms = device {max|dn|, dn.dn} (already all-reduced); every
// thread derives the same two factors.  When the first step of the line search is known before this pass (ALGLIB's
// lastgoodstep), its trial point x1 = xk + stp1 * d is written here as well: one pass over xk / x less per CG iteration
// than a separate k_axpy_out (same expression, same rounding).
template <typename T, int V>
__global__ __launch_bounds__(256) void k_normalize(T* __restrict__ d, const T* __restrict__ dn, const double* __restrict__ norms,
                                                  size_t n, const T* __restrict__ xk, T* __restrict__ x1, T stp1) {
  const double mx = norms[0], ss = norms[1];
  double s1, s2;
  norm_factors(mx, ss, s1, s2);
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (size_t)gridDim.x * 256 * V) {
    T dv[V], xv[V], v[V];
    ldv<T, V, true>(dn + i, dv);
    if (x1 != nullptr) ldv<T, V, false>(xk + i, xv);
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = norm_elem<T>(dv[q], mx, s1, s2);
    stv<T, V, false>(d + i, v);
    if (x1 != nullptr) {  // the line search's first trial point (k_axpy_out's expression)
      T xn[V];
#pragma unroll
      for (int q = 0; q < V; ++q) xn[q] = xv[q] + stp1 * v[q];
      stv<T, V, false>(x1 + i, xn);
    }
  }
}

// y = g - gp (mincg: yk = -g_k, then yk += g_{k+1}: the same rounding) ; sums: [0] g.g, [1] g.y   (the DY / HS betas,
// optimization.cpp:17700-17760).  Their denominator vv = y.dk is not summed here: y.dk = g.dk - gp.dk, and both terms are
// already known -- gp.dk is the g.dn the direction pass reduced, g.dk = (g.d) / (s1 s2) from the accepted trial
// evaluation's g.d (the line search bounds |g.d| by 0.3 |gp.d|: no cancellation) -- so the pass reads two vectors
// instead of three (dk is not touched).  vv comes as an argument.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_beta_dots(const T* __restrict__ gp, const T* __restrict__ g,
                                                  size_t n, Owned ow, double* __restrict__ part, Fin fin,
                                                  double* __restrict__ beta_dst, int restart, double vv,
                                                  const T* __restrict__ dk_check) {
  // dk_check (host-paced passes only): the denominator y.dk summed directly as well, row [2] -- the self-check of the
  // derived vv (srmap_problem_selfcheck); the betas still use the derived one, so both pacing modes stay bit-equal
  double b = 0, c = 0, e = 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (size_t)gridDim.x * 256 * V) {
    T gv[V], pv[V], kv[V];
    ldv<T, V, false>(g + i, gv);
    ldv<T, V, true>(gp + i, pv);
    if (dk_check != nullptr) ldv<T, V, true>(dk_check + i, kv);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (!ow.has(i + q)) continue;
      const T y = -pv[q] + gv[q];
      b += (double)gv[q] * (double)gv[q]; c += (double)gv[q] * (double)y;
      if (dk_check != nullptr) e += (double)y * (double)kv[q];
    }
  }
  double tot[3];
  if (block_partials3(b, c, e, part, false, dk_check != nullptr ? 3 : 2, fin, tot)) {
    if (beta_dst != nullptr) {
      // betak = max(0, min(betady, betahs)) exactly as run_cg forms it on the host (same IEEE divisions and compares):
      // the direction pass queued behind this one reads it, the host never has to answer in between
      const double bdy = tot[0] / vv, bhs = tot[1] / vv;
      const double bm = bdy < bhs ? bdy : bhs;
      double bk = 0.0 > bm ? 0.0 : bm;
      if (restart) bk = 0.0;
      beta_dst[0] = bk;
    }
    fin_tag(fin);
  }
}

// partial of a.b over the owned elements: [0]
template <typename T, int V>
__global__ __launch_bounds__(256) void k_dot(const T* __restrict__ a, const T* __restrict__ b, size_t n, Owned ow,
                                            double* __restrict__ part, Fin fin) {
  double s = 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (size_t)gridDim.x * 256 * V) {
    T av[V], bv[V];
    ldv<T, V, false>(a + i, av);
    ldv<T, V, false>(b + i, bv);
#pragma unroll
    for (int q = 0; q < V; ++q)
      if (ow.has(i + q)) s += (double)av[q] * (double)bv[q];
  }
  if (block_partials3(s, 0.0, 0.0, part, false, 1, fin)) fin_tag(fin);
}

// dst = a + alpha * b
template <typename T>
__global__ void k_axpy_out(T* __restrict__ dst, const T* __restrict__ a, const T* __restrict__ b, T alpha, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = a[i] + alpha * b[i];
}
// the same, four elements per thread (16 / 32-byte requests; device allocations are aligned): element by element the
// same expression, so the same bits
template <typename T>
__global__ __launch_bounds__(256) void k_axpy_out4(T* __restrict__ dst, const T* __restrict__ a, const T* __restrict__ b, T alpha,
                                                  size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  T va[4], vb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { va[q] = a[4 * i + q]; vb[q] = b[4 * i + q]; }
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[4 * i + q] = va[q] + alpha * vb[q];
}
template <typename T>
__global__ void k_fill(T* __restrict__ d, T v, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[i] = v;
}

// ---- host launchers (solver_passes.hpp) ------------------------------------------------------------------
template <typename T>
void launch_cg_direction(T* dn, const T* g, const T* dk, T beta, size_t n, const Owned& ow, double* part, const Fin& fin,
                         const double* beta_dev, double* norms_pub, int keep_dn, int nb, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (n % V == 0) hipLaunchKernelGGL((k_direction<T, V>), dim3(nb), dim3(256), 0, st, dn, g, dk, beta, n, ow, part, fin, beta_dev, norms_pub, keep_dn);
  else hipLaunchKernelGGL((k_direction<T, 1>), dim3(nb), dim3(256), 0, st, dn, g, dk, beta, n, ow, part, fin, beta_dev, norms_pub, keep_dn);
}
template <typename T>
void launch_cg_beta_dots(const T* gp, const T* g, size_t n, const Owned& ow, double* part, const Fin& fin, double* beta_dst,
                         int restart, double vv, const T* dk_check, int nb, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (n % V == 0) hipLaunchKernelGGL((k_beta_dots<T, V>), dim3(nb), dim3(256), 0, st, gp, g, n, ow, part, fin, beta_dst, restart, vv, dk_check);
  else hipLaunchKernelGGL((k_beta_dots<T, 1>), dim3(nb), dim3(256), 0, st, gp, g, n, ow, part, fin, beta_dst, restart, vv, dk_check);
}
template <typename T>
void launch_cg_dot(const T* a, const T* b, size_t n, const Owned& ow, double* part, const Fin& fin, int nb, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (n % V == 0) hipLaunchKernelGGL((k_dot<T, V>), dim3(nb), dim3(256), 0, st, a, b, n, ow, part, fin);
  else hipLaunchKernelGGL((k_dot<T, 1>), dim3(nb), dim3(256), 0, st, a, b, n, ow, part, fin);
}
template <typename T>
void launch_cg_normalize(T* d, const T* dn, const double* norms, size_t n, const T* xk, T* x1, T stp1, int nb,
                         hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (n % V == 0) hipLaunchKernelGGL((k_normalize<T, V>), dim3(nb), dim3(256), 0, st, d, dn, norms, n, xk, x1, stp1);
  else hipLaunchKernelGGL((k_normalize<T, 1>), dim3(nb), dim3(256), 0, st, d, dn, norms, n, xk, x1, stp1);
}
template <typename T>
void launch_axpy_out(T* dst, const T* a, const T* b, T alpha, size_t n, hipStream_t st) {
  if ((n & 3) == 0) hipLaunchKernelGGL(k_axpy_out4<T>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, dst, a, b, alpha, n / 4);
  else hipLaunchKernelGGL(k_axpy_out<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, a, b, alpha, n);
}
template <typename T>
void launch_fill(T* d, T v, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_fill<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, v, n);
}
void launch_finish(const double* part, int nb, int rows, int max0, double* out, const double* extra_src, double* tag_slot,
                   double tag, hipStream_t st) {
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(256), 0, st, part, nb, rows, max0, out, extra_src, tag_slot, tag);
}
void launch_publish(double* dst, const double* src, int n, double* tag_slot, double tag, hipStream_t st) {
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, dst, src, n, tag_slot, tag);
}

#define SRMAP_PASSES(T)                                                                                                      \
  template void launch_cg_direction<T>(T*, const T*, const T*, T, size_t, const Owned&, double*, const Fin&, const double*, \
                                       double*, int, int, hipStream_t);                                                     \
  template void launch_cg_beta_dots<T>(const T*, const T*, size_t, const Owned&, double*, const Fin&, double*, int, double, \
                                       const T*, int, hipStream_t);                                                         \
  template void launch_cg_dot<T>(const T*, const T*, size_t, const Owned&, double*, const Fin&, int, hipStream_t);          \
  template void launch_cg_normalize<T>(T*, const T*, const double*, size_t, const T*, T*, T, int, hipStream_t);             \
  template void launch_axpy_out<T>(T*, const T*, const T*, T, size_t, hipStream_t);                                         \
  template void launch_fill<T>(T*, T, size_t, hipStream_t);
SRMAP_PASSES(float)
SRMAP_PASSES(double)
#undef SRMAP_PASSES

}  // namespace srmap
