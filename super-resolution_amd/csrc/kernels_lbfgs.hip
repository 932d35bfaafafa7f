// kernels_lbfgs.hip -- the two n-vector passes of the L-BFGS inner solver (solver.hip run_lbfgs; ALGLIB 3.10.0
// minlbfgsiteration, libs/alglib/src/optimization.cpp:21640 ff., as the reference selects it with
// LBFGS_SOLVER, irls_map_solver.cpp:97-113).
//
// ALGLIB forms the direction by the two-loop recursion: 2 (q + 1) dependent dot + axpy passes over the history.  Here
// the direction is formed in compact form instead.  Every vector of the recursion is a linear combination of the basis
// {g, s_0 .. s_q, y_0 .. y_q}; the host runs ALGLIB's two loops on the coefficient vector, taking each dot product
// from a Gram table, and the device does two streaming passes per iteration:
//   k_lbfgs_update     s_p = x - x_k and y_p = g - g_k into ring slot p (by subtraction, as ALGLIB forms sk / yk),
//                      and every dot product the next direction needs that involves a new vector:
//                      g.g (epsg), s_p.s_p (epsx), then per live slot j: s_p.y_j, y_p.s_j, y_p.y_j, g.s_j, g.y_j -- the rows
//                      kLbGg, kLbSs, lb_row(j, .) of solver_mailbox.hpp
//                      (the older pairs' entries do not change: the host keeps them)
//   k_lbfgs_direction  dn = -(c_g g + sum_j (c_sj s_j + c_yj y_j)) and {max|dn|, dn.dn, g.dn}: the sums k_direction
//                      leaves, in the same device and host-mapped slots, so the normalisation factors, the fold of the
//                      trial point into the evaluation and its g.d consume the L-BFGS direction unchanged.
// Each pass reduces in the same launch: every workgroup publishes its partials, the last one to arrive (ticket) adds
// them in workgroup order and hands the sums and the arrival tag to the host.  The result does not depend on which
// workgroup is last.  f32 vectors accumulate in f64.
#include <hip/hip_runtime.h>

#include "reduce_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

namespace {

// R sums (row 0 a max when MAX0) of the whole grid: workgroup partials to red.part[r * gridDim.x + block], then the
// last workgroup to take a ticket adds them per row in workgroup order (thread i: i, i + 256, ...; then the wave and
// the four waves), writes red.out_dev / red.out_host and finally the tag behind a system-scope fence.
template <int R, bool MAX0>
__device__ __forceinline__ void ticket_reduce(double (&acc)[R], const LbfgsRed& red) {
  __shared__ double sm[R][4];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned nb = gridDim.x;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double v = (MAX0 && r == 0) ? wave_max(acc[r]) : wave_sum(acc[r]);
    if (lane == 0) sm[r][wid] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < R) red.part[(size_t)threadIdx.x * nb + blockIdx.x] = combine4(sm[threadIdx.x], MAX0 && threadIdx.x == 0);
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(red.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = old == nb - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!is_last) return;
  __shared__ double tot[R][4];
  // every row's loads issued together (independent rows), each row still added in workgroup order
  double v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = 0.0;
  for (unsigned i = threadIdx.x; i < nb; i += 256) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned long long b = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(red.part) + (size_t)r * nb + i,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double a = __longlong_as_double((long long)b);
      v[r] = (MAX0 && r == 0) ? fmax(v[r], a) : v[r] + a;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double t = (MAX0 && r == 0) ? wave_max(v[r]) : wave_sum(v[r]);
    if (lane == 0) tot[r][wid] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int r = 0; r < R; ++r) {
      const double t = combine4(tot[r], MAX0 && r == 0);
      if (red.out_dev != nullptr) red.out_dev[r] = t;
      red.out_host[r] = t;
    }
    *red.ticket = 0u;  // armed for the next pass (the kernel boundary orders it)
    __threadfence_system();
    *(volatile double*)red.tag_slot = red.tag;
  }
}

template <typename T, int V, int L>
__global__ __launch_bounds__(256) void k_lbfgs_update(const T* __restrict__ x, const T* __restrict__ xk,
                                                     const T* __restrict__ g, const T* __restrict__ gk, T* S, T* Y,
                                                     int p, size_t n, LbfgsRed red) {
  constexpr int R = lb_rows(L);
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  T* sp = S + (size_t)p * n;
  T* yp = Y + (size_t)p * n;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (size_t)gridDim.x * 256 * V) {
    T xv[V], xkv[V], gv[V], gkv[V], s[V], y[V];
    ldv<T, V, false>(x + i, xv);
    ldv<T, V, false>(xk + i, xkv);
    ldv<T, V, false>(g + i, gv);
    ldv<T, V, true>(gk + i, gkv);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      s[q] = -xkv[q] + xv[q];  // sk = -x_k; sk += x_{k+1}
      y[q] = -gkv[q] + gv[q];  // yk = -g_k; yk += g_{k+1}
    }
    stv<T, V, true>(sp + i, s);
    stv<T, V, true>(yp + i, y);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      acc[kLbGg] += (double)gv[q] * (double)gv[q];
      acc[kLbSs] += (double)s[q] * (double)s[q];
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
      T sj[V], yj[V];
      if (j == p) {
#pragma unroll
        for (int q = 0; q < V; ++q) { sj[q] = s[q]; yj[q] = y[q]; }
      } else {
        ldv<T, V, true>(S + (size_t)j * n + i, sj);
        ldv<T, V, true>(Y + (size_t)j * n + i, yj);
      }
#pragma unroll
      for (int q = 0; q < V; ++q) {
        acc[lb_row(j, kLbSyj)] += (double)s[q] * (double)yj[q];
        acc[lb_row(j, kLbYsj)] += (double)y[q] * (double)sj[q];
        acc[lb_row(j, kLbYyj)] += (double)y[q] * (double)yj[q];
        acc[lb_row(j, kLbGsj)] += (double)gv[q] * (double)sj[q];
        acc[lb_row(j, kLbGyj)] += (double)gv[q] * (double)yj[q];
      }
    }
  }
  ticket_reduce<R, false>(acc, red);
}

// keep_dn: the evaluations read dn again (trial points formed from it): stored with the default cache policy
template <typename T, int V, int L>
__global__ __launch_bounds__(256) void k_lbfgs_direction(T* __restrict__ dn, const T* __restrict__ g, const T* S,
                                                        const T* Y, LbfgsCoef c, size_t n, int keep_dn, LbfgsRed red) {
  double acc[3] = {0.0, 0.0, 0.0};  // max|dn|, dn.dn, g.dn
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (size_t)gridDim.x * 256 * V) {
    T gv[V], v[V];
    double w[V];
    ldv<T, V, false>(g + i, gv);
#pragma unroll
    for (int q = 0; q < V; ++q) w[q] = c.c[0] * (double)gv[q];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      T sj[V], yj[V];
      ldv<T, V, true>(S + (size_t)j * n + i, sj);
      ldv<T, V, true>(Y + (size_t)j * n + i, yj);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        w[q] += c.c[1 + 2 * j] * (double)sj[q];
        w[q] += c.c[2 + 2 * j] * (double)yj[q];
      }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = (T)(-w[q]);
    if (keep_dn) stv<T, V, false>(dn + i, v); else stv<T, V, true>(dn + i, v);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const double d = (double)v[q];
      acc[0] = fmax(acc[0], fabs(d));
      acc[1] += d * d;
      acc[2] += (double)gv[q] * d;
    }
  }
  ticket_reduce<3, true>(acc, red);
}

template <typename T, int V, int L>
void launch_update_v(const T* x, const T* xk, const T* g, const T* gk, T* S, T* Y, int p, size_t n, int nb,
                     const LbfgsRed& red, hipStream_t st) {
  hipLaunchKernelGGL((k_lbfgs_update<T, V, L>), dim3(nb), dim3(256), 0, st, x, xk, g, gk, S, Y, p, n, red);
}
template <typename T, int V, int L>
void launch_direction_v(T* dn, const T* g, const T* S, const T* Y, const LbfgsCoef& c, size_t n, int nb, int keep,
                        const LbfgsRed& red, hipStream_t st) {
  hipLaunchKernelGGL((k_lbfgs_direction<T, V, L>), dim3(nb), dim3(256), 0, st, dn, g, S, Y, c, n, keep, red);
}

template <typename T, int V>
int update_v(const T* x, const T* xk, const T* g, const T* gk, T* S, T* Y, int p, int live, size_t n, int nb,
             const LbfgsRed& red, hipStream_t st) {
  switch (live) {
    case 1: launch_update_v<T, V, 1>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 2: launch_update_v<T, V, 2>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 3: launch_update_v<T, V, 3>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 4: launch_update_v<T, V, 4>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 5: launch_update_v<T, V, 5>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 6: launch_update_v<T, V, 6>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 7: launch_update_v<T, V, 7>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    case 8: launch_update_v<T, V, 8>(x, xk, g, gk, S, Y, p, n, nb, red, st); break;
    default: return SRMAP_EINVAL;
  }
  return SRMAP_OK;
}
template <typename T, int V>
int direction_v(T* dn, const T* g, const T* S, const T* Y, int live, const LbfgsCoef& c, size_t n, int nb, int keep,
                const LbfgsRed& red, hipStream_t st) {
  switch (live) {
    case 1: launch_direction_v<T, V, 1>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 2: launch_direction_v<T, V, 2>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 3: launch_direction_v<T, V, 3>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 4: launch_direction_v<T, V, 4>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 5: launch_direction_v<T, V, 5>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 6: launch_direction_v<T, V, 6>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 7: launch_direction_v<T, V, 7>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    case 8: launch_direction_v<T, V, 8>(dn, g, S, Y, c, n, nb, keep, red, st); break;
    default: return SRMAP_EINVAL;
  }
  return SRMAP_OK;
}

}  // namespace

template <typename T>
int launch_lbfgs_update(const T* x, const T* xk, const T* g, const T* gk, T* S, T* Y, int p, int live, size_t n, int nb,
                        const LbfgsRed& red, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (n % V == 0) return update_v<T, V>(x, xk, g, gk, S, Y, p, live, n, nb, red, st);
  return update_v<T, 1>(x, xk, g, gk, S, Y, p, live, n, nb, red, st);
}
template <typename T>
int launch_lbfgs_direction(T* dn, const T* g, const T* S, const T* Y, int live, const LbfgsCoef& c, size_t n, int nb,
                           int keep_dn, const LbfgsRed& red, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (n % V == 0) return direction_v<T, V>(dn, g, S, Y, live, c, n, nb, keep_dn, red, st);
  return direction_v<T, 1>(dn, g, S, Y, live, c, n, nb, keep_dn, red, st);
}

template int launch_lbfgs_update<float>(const float*, const float*, const float*, const float*, float*, float*, int, int,
                                        size_t, int, const LbfgsRed&, hipStream_t);
template int launch_lbfgs_update<double>(const double*, const double*, const double*, const double*, double*, double*,
                                         int, int, size_t, int, const LbfgsRed&, hipStream_t);
template int launch_lbfgs_direction<float>(float*, const float*, const float*, const float*, int, const LbfgsCoef&,
                                           size_t, int, int, const LbfgsRed&, hipStream_t);
template int launch_lbfgs_direction<double>(double*, const double*, const double*, const double*, int, const LbfgsCoef&,
                                            size_t, int, int, const LbfgsRed&, hipStream_t);

}  // namespace srmap
