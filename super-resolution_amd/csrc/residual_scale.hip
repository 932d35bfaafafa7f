// residual_scale.hip -- the residual scale 1.4826 median|r| of the data term (no reference counterpart):
// an exact radix select of the K + 1 lower medians of |r| -- one per frame, one over all frames -- on the device, the
// record a Huber step in the scale mode SRMAP_HUBER_DELTA_MAD takes its delta from, and the C entry points
// srmap_residual_scale*, srmap_problem_set_huber_scale and srmap_problem_get_huber_delta.  The arithmetic of the select
// (key, digit schedule, bin pick) is select_host.hpp's; nothing returns to the host between the passes.
#include <cmath>
#include <cstdint>
#include <vector>

#include "select_host.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

namespace {

// One selection, on the device: the digits fixed so far, the rank that remains within them, the counted elements.
// [0] the selection over all frames, [1 + k] frame k's
struct SelState {
  unsigned long long prefix, rank, n;
};

constexpr int kSlabWords = 2 * kSelectMaxBins;  // a workgroup's slab: its frame histogram, then its global one

// One digit pass over the residuals r, [K] runs of rowlen elements (blockIdx.y = frame).  An element counts where its
// mask m (MASK; indexed like the data weights, runs m_stride apart) is > 0; a counted element whose higher digits equal
// its frame's prefix adds to the workgroup's frame histogram, one whose higher digits equal the global prefix to its
// global histogram (LDS integer adds).  The workgroup stores both as its slab: no global atomics, and integer counts
// make the sums independent of any order.  16-byte loads over the part of the run that is 16-byte aligned in both
// streams, its first and last elements one by one.
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_select_hist(const T* __restrict__ r, const T* __restrict__ m, size_t rowlen,
                                                    size_t m_stride, const SelState* __restrict__ state, int pass,
                                                    unsigned* __restrict__ slabs) {
  typedef typename SelectKey<T>::type K;
  constexpr int V = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(16 / sizeof(T))));
  __shared__ unsigned hist[kSlabWords];
  const int k = blockIdx.y;
  const SelectDigit d = select_digit<T>(pass);
  const int nb = 1 << d.bits;
  for (int i = threadIdx.x; i < kSlabWords; i += 256) hist[i] = 0u;
  const K pf = pass ? (K)state[1 + k].prefix : (K)0, pg = pass ? (K)state[0].prefix : (K)0;
  __syncthreads();
  const T* rr = r + (size_t)k * rowlen;
  const T* mm = MASK ? m + (size_t)k * m_stride : nullptr;
  auto count = [&](T v) {
    const K key = select_key(v);
    const unsigned bin = select_bin(key, d);
    if (select_matches(key, pf, d)) atomicAdd(&hist[bin], 1u);
    if (select_matches(key, pg, d)) atomicAdd(&hist[kSelectMaxBins + bin], 1u);
  };
  size_t head = ((16 - reinterpret_cast<uintptr_t>(rr) % 16) % 16) / sizeof(T);
  if (head > rowlen) head = rowlen;
  if (MASK && (reinterpret_cast<uintptr_t>(mm) - reinterpret_cast<uintptr_t>(rr)) % 16 != 0) head = rowlen;  // no common alignment
  const size_t nv = (rowlen - head) / V;
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
  for (size_t i = tid; i < head; i += nth)
    if (!MASK || mm[i] > T(0)) count(rr[i]);
  for (size_t i = tid; i < nv; i += nth) {
    const VT v = reinterpret_cast<const VT*>(rr + head)[i];
    if constexpr (MASK) {
      const VT mv = reinterpret_cast<const VT*>(mm + head)[i];
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (mv[q] > T(0)) count(v[q]);
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q) count(v[q]);
    }
  }
  for (size_t i = head + nv * V + tid; i < rowlen; i += nth)
    if (!MASK || mm[i] > T(0)) count(rr[i]);
  __syncthreads();
  unsigned* out = slabs + ((size_t)k * gridDim.x + blockIdx.x) * kSlabWords;
  for (int i = threadIdx.x; i < 2 * nb; i += 256) {
    const int at = (i >> d.bits) * kSelectMaxBins + (i & (nb - 1));
    out[at] = hist[at];
  }
}

// Once per selection and pass (blockIdx.x = selection): add the slabs of the selection's workgroups -- G per frame, K G
// for the global one --, scan the bins, pick the bin that holds the remaining rank (select_pick) and extend the prefix by
// it.  The first pass also learns n, the counted elements, and from it the median's rank.  A thread owns 8 consecutive bins.
template <typename T>
__global__ __launch_bounds__(256) void k_select_pick(const unsigned* __restrict__ slabs, int G, int K, SelState* state, int pass) {
  typedef typename SelectKey<T>::type KeyT;
  constexpr int B = kSelectMaxBins / 256;
  static_assert(B == 8, "two 16-byte loads per thread and slab");
  __shared__ unsigned long long sc[256];
  const int s = blockIdx.x, t = threadIdx.x;
  const SelectDigit d = select_digit<T>(pass);
  const int nb = 1 << d.bits;
  const SelState was = state[s];
  const int first = s == 0 ? 0 : (s - 1) * G, cnt = s == 0 ? K * G : G;
  unsigned long long c[B];
#pragma unroll
  for (int q = 0; q < B; ++q) c[q] = 0ull;
  if (B * t < nb) {
    const unsigned* h = slabs + (size_t)first * kSlabWords + (s == 0 ? kSelectMaxBins : 0) + B * t;
#pragma unroll 8  // independent loads in flight: the global selection folds K G slabs in one workgroup
    for (int j = 0; j < cnt; ++j, h += kSlabWords) {
      const uint4 a = reinterpret_cast<const uint4*>(h)[0], b = reinterpret_cast<const uint4*>(h)[1];
      c[0] += a.x; c[1] += a.y; c[2] += a.z; c[3] += a.w;
      c[4] += b.x; c[5] += b.y; c[6] += b.z; c[7] += b.w;
    }
  }
  unsigned long long tsum = 0ull;
#pragma unroll
  for (int q = 0; q < B; ++q) tsum += c[q];
  sc[t] = tsum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive scan over the threads
    const unsigned long long v = t >= off ? sc[t - off] : 0ull;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  const unsigned long long total = sc[255], excl = sc[t] - tsum;
  const unsigned long long n = pass == 0 ? total : was.n;
  if (n == 0ull || total == 0ull) {  // nothing counted: scale 0, count 0
    if (t == 0) state[s] = {0ull, 0ull, 0ull};
    return;
  }
  const unsigned long long rank = pass == 0 ? select_median_rank(n) : was.rank;
  if (rank >= excl && rank < excl + tsum) {
    uint64_t left = rank - excl;
    const int bin = select_pick(c, B, &left);  // over the thread's own bins
    const KeyT prefix = pass == 0 ? (KeyT)0 : (KeyT)was.prefix;
    state[s] = {(unsigned long long)select_extend<KeyT>(prefix, d, B * t + bin), (unsigned long long)left, n};
  }
}

// One thread: the scales 1.4826 median and the counts of the K + 1 selections into the record rec = {delta, scales[1 + K],
// counts[1 + K]}; mad: delta = max(tuning * scales[0], min_delta) (select_mad_delta), else 0
template <typename T>
__global__ void k_select_finish(const SelState* __restrict__ state, int K, int mad, double tuning, double min_delta,
                                double* __restrict__ rec) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int s = 0; s <= K; ++s) {
    const SelState st = state[s];
    rec[1 + s] = st.n ? kMadToSigma * select_value<T>(st.prefix) : 0.0;
    rec[2 + K + s] = (double)st.n;
  }
  rec[0] = mad ? select_mad_delta(rec[1], tuning, min_delta) : 0.0;
}

}  // namespace

size_t residual_scale_record_doubles(int K) { return 3 + 2 * (size_t)K; }

// the slabs, the states and the two records (slot 0: the last Huber step's, slot 1: srmap_residual_scale's) of the problem
static int ensure_select_buffers(srmap_problem* p, int gmax, hipStream_t st) {
  const int K = p->geo.K;
  if (int rc = ensure(p, &p->d_sel_slabs, (size_t)K * gmax * kSlabWords * sizeof(unsigned))) return rc;
  if (int rc = ensure(p, &p->d_sel_state, (size_t)(K + 1) * sizeof(SelState))) return rc;
  if (!p->d_sel_rec) {
    const size_t bytes = 2 * residual_scale_record_doubles(K) * sizeof(double);
    SRMAP_HIP(p->ctx, p->d_sel_rec.alloc(bytes));
    SRMAP_HIP(p->ctx, hipMemsetAsync(p->d_sel_rec.as(), 0, bytes, st));
  }
  return SRMAP_OK;
}

template <typename T>
int launch_residual_scale(srmap_problem* p, const T* r, const T* mask, size_t rowlen, size_t m_stride, int slot, bool mad,
                          double tuning, double min_delta, hipStream_t st) {
  constexpr size_t V = 16 / sizeof(T);
  const int K = p->geo.K;
  // workgroups per frame: about two per compute unit in all (each stores a 16 KB slab per pass), no more than the run
  // has 16-byte groups
  const int gmax = std::max(1, std::max(1, p->ctx->num_cus) * 2 / K);
  if (int rc = ensure_select_buffers(p, gmax, st)) return rc;
  const int G = (int)std::max<size_t>(1, std::min<size_t>((size_t)gmax, (rowlen + V * 256 - 1) / (V * 256)));
  SelState* state = p->d_sel_state.as<SelState>();
  unsigned* slabs = p->d_sel_slabs.as<unsigned>();
  for (int pass = 0; pass < SelectKey<T>::passes; ++pass) {
    if (mask) hipLaunchKernelGGL((k_select_hist<T, true>), dim3(G, K), dim3(256), 0, st, r, mask, rowlen, m_stride, state, pass, slabs);
    else hipLaunchKernelGGL((k_select_hist<T, false>), dim3(G, K), dim3(256), 0, st, r, mask, rowlen, m_stride, state, pass, slabs);
    hipLaunchKernelGGL(k_select_pick<T>, dim3(K + 1), dim3(256), 0, st, slabs, G, K, state, pass);
  }
  hipLaunchKernelGGL(k_select_finish<T>, dim3(1), dim3(64), 0, st, state, K, mad ? 1 : 0, tuning, min_delta,
                     residual_scale_record(p, slot));
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}
template int launch_residual_scale<float>(srmap_problem*, const float*, const float*, size_t, size_t, int, bool, double, double, hipStream_t);
template int launch_residual_scale<double>(srmap_problem*, const double*, const double*, size_t, size_t, int, bool, double, double, hipStream_t);

double* residual_scale_record(srmap_problem* p, int slot) {
  return p->d_sel_rec ? p->d_sel_rec.as<double>() + (size_t)slot * residual_scale_record_doubles(p->geo.K) : nullptr;
}

// record `slot` for the caller, behind everything enqueued on st; zeros while the problem has none
static int fetch_record(srmap_problem* p, int slot, hipStream_t st, double* delta, double* scales, double* counts) {
  const int K = p->geo.K;
  std::vector<double> rec(residual_scale_record_doubles(K), 0.0);
  if (p->d_sel_rec) {
    SRMAP_HIP(p->ctx, hipMemcpyAsync(rec.data(), residual_scale_record(p, slot), rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  }
  if (delta) *delta = rec[0];
  for (int s = 0; s <= K; ++s) {
    if (scales) scales[s] = rec[1 + s];
    if (counts) counts[s] = rec[2 + K + s];
  }
  return SRMAP_OK;
}

}  // namespace srmap

extern "C" {

int srmap_problem_set_huber_scale(srmap_problem* p, int mode, double tuning, double min_delta) {
  if (!p) return SRMAP_EINVAL;
  if (mode != SRMAP_HUBER_DELTA_FIXED && mode != SRMAP_HUBER_DELTA_MAD)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown Huber scale mode %d", mode);
  if (mode == SRMAP_HUBER_DELTA_MAD) {
    if (!(tuning > 0.0 && std::isfinite(tuning))) return set_error(p->ctx, SRMAP_EINVAL, "tuning must be finite and > 0 (got %g)", tuning);
    if (!(min_delta > 0.0 && std::isfinite(min_delta)))
      return set_error(p->ctx, SRMAP_EINVAL, "min_delta must be finite and > 0 (got %g)", min_delta);
  }
  p->dw.set_scale(mode, tuning, min_delta);
  return SRMAP_OK;
}

int srmap_problem_get_huber_delta(srmap_problem* p, int* mode, double* delta, double* scales, double* counts) {
  if (!p) return SRMAP_EINVAL;
  if (mode) *mode = p->dw.scale_mode();
  if (p->dw.scale_mode() != SRMAP_HUBER_DELTA_MAD) {
    if (delta) *delta = p->dw.delta();
    for (int s = 0; s <= p->geo.K; ++s) {
      if (scales) scales[s] = 0.0;
      if (counts) counts[s] = 0.0;
    }
    return SRMAP_OK;
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  // the step recorded the problem's state event behind its weight kernel (state_end_write): waiting for the event, not for
  // the step's stream, asks nothing of a stream the caller may have destroyed since
  if (p->state_ev) SRMAP_HIP(p->ctx, hipEventSynchronize(p->state_ev));
  return fetch_record(p, 0, p->ctx->stream, delta, scales, counts);
}

int srmap_residual_scale_device(srmap_problem* p, const void* x_dev, void* hip_stream, double* scales, double* counts) {
  if (!p || !x_dev || !scales) return SRMAP_EINVAL;
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const hipStream_t st = stream_of(p->ctx, hip_stream);
  // d_resid and the select's buffers are written: ordered like a state write, and complete on return
  int rc = state_begin_write(p, st);
  if (rc == SRMAP_OK) rc = problem_state_read(p, st);
  if (rc == SRMAP_OK) rc = ensure_eval_partials(p);
  if (rc) return rc;
  rc = dispatch_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    const Geometry& g = p->geo;
    if (int r = launch_forward_residual<T>(p, g, 0, (const T*)x_dev, p->d_partials.as<double>(), st)) return r;
    const size_t run = (size_t)g.C * g.w * g.h;
    // what counts: under L2 the effective weights, under Huber (whose weights are never zero by design) the prior
    const T* mask = p->dw.loss() == SRMAP_DATA_LOSS_HUBER ? p->dw.prior<T>() : p->dw.effective<T>();
    return launch_residual_scale<T>(p, p->d_resid.as<const T>(), mask, run, run, 1, false, 0.0, 0.0, st);
  });
  if (rc) return rc;
  return fetch_record(p, 1, st, nullptr, scales, counts);
}

int srmap_residual_scale(srmap_problem* p, const double* x_host, double* scales, double* counts) {
  if (!p || !x_host || !scales) return SRMAP_EINVAL;
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  if (int rc = stage_host_x(p, x_host)) return rc;
  return srmap_residual_scale_device(p, p->d_x.as(), p->ctx->stream, scales, counts);
}

}  // extern "C"
