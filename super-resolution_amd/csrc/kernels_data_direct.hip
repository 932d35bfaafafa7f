// kernels_data_direct.hip -- the data term's straightforward gfx950 kernels: one thread per output element, inputs read
// through L1/L2.  They accept every geometry the reference accepts (arbitrary shifts, blur sizes, non-divisible HR sizes
// for ImageModel::ApplyToImage) and serve
//   (a) the operator entry points (srmap_apply, srmap_apply_transpose), and
//   (b) the fallback of srmap_eval when the tile kernels (kernels_ztile.hip) do not cover the geometry, and their
//       cross-check.
// They serve every motion kind (none, translation table, affine matrices, displacement field, dense or on a lattice): the
// forward kernel is one template over the kind's sampler, the transpose k_gather_direct for a translation and
// k_gather_sampled for the kinds that warp per pixel (MotionSampler, sample_dev.hpp).  Source coordinates of those are
// double in both dtypes (an f32 coordinate at 2048 px carries 1e-4 px of error); the weights are the double products
// rounded to T.
//
// Math: SURVEY.md section 8(a'); reference lines are cited per kernel.
#include "reduce_dev.hpp"
#include "sample_dev.hpp"
#include "srmap_internal.hpp"

namespace srmap {

// identity_warp / warp_sample / MotionSampler: sample_dev.hpp (shared with the fits)

// ---------------------------------------------------------------------------
// Forward model A_k = D B M_k (image_model.cpp:86-91) at every LR pixel of
// frames [k0, k0+gridDim.z), optionally minus the observation, optionally with
// the data-term cost partial s^2 * sum(res^2) (objective_data_term.cpp:29-50).
// MOTION (compile time): how M_k is sampled (MotionSampler) -- kMotionTable (also a problem without motion: the identity
// table), kMotionAffine, kMotionFlow, kMotionLattice.  The per-pixel kinds read their sources through the caches: per LR
// pixel b^2 x 4 taps of x, and per blur tap two field values for a flow, two times four nodes for a lattice.
// WEIGHTED (compile time; needs y): per-observation weights dw indexed like y -- out = w * res, partial s^2 * sum(w res^2).
// blur_bank: the table of the block's (frame, absolute channel) -- block-uniform; the strides are 0 without a bank.
template <typename T, int MOTION, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_forward_direct(
    const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out,
    double* __restrict__ partials, Geometry g,
    MotionArgs<T> ma, const T* __restrict__ blur_bank,
    const int* __restrict__ col_map, const int* __restrict__ row_map, int k0,
    double cost_scale, int obs_C, int obs_c0, const T* __restrict__ dw, BlurStride bs) {
  __shared__ double red[4];
  __shared__ T comb[36];  // table kind: blur (x) bilinear taps of this block's frame and channel, (b+1) x (b+1), b <= 5
  const int lp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, kk = blockIdx.z, k = k0 + kk;
  const T* __restrict__ blur = blur_bank + ((size_t)k * bs.frame + (size_t)(c + obs_c0) * bs.channel);
  const int n = g.w * g.h;
  const MotionSampler<T, MOTION> ms(ma, g, k);
  // table kind, interior fast path for bilinear warps: one (b+1)^2 stencil on x instead of b^2 four-tap samples (a
  // per-pixel kind has no such stencil: its fractions vary from pixel to pixel)
  bool use_comb = false;
  const int nb1 = g.b + 1;
  if constexpr (MOTION == kMotionTable) {
    const WarpTaps<T>& wt = ms.wt;
    use_comb = wt.ntaps == 4 && wt.ytab == nullptr && g.b <= 5;
    if (use_comb) {
      if ((int)threadIdx.x < nb1 * nb1) {
        const int a1 = threadIdx.x / nb1, e1 = threadIdx.x - a1 * nb1;
        T s = T(0);
        for (int t = 0; t < 4; ++t) {
          const int a = a1 - (t >> 1), e = e1 - (t & 1);
          if (a >= 0 && a < g.b && e >= 0 && e < g.b) s += blur[a * g.b + e] * wt.w[t];
        }
        comb[threadIdx.x] = s;
      }
      __syncthreads();
    }
  }
  double sq = 0.0;
  if (lp < n) {
    const int i = lp / g.w, j = lp - i * g.w;
    const int R0 = row_map[i], C0 = col_map[j];
    const T* plane = x + (size_t)c * g.W * g.H;
    T acc = T(0);
    int sr0 = 0, sc0 = 0;  // the stencil's first source pixel
    if constexpr (MOTION == kMotionTable) {
      sr0 = R0 - g.hb + ms.wt.oy;
      sc0 = C0 - g.hb + ms.wt.ox;
    }
    if (use_comb && R0 - g.hb >= 0 && R0 + g.hb < g.H && C0 - g.hb >= 0 && C0 + g.hb < g.W && sr0 >= 0 &&
        sr0 + g.b < g.H && sc0 >= 0 && sc0 + g.b < g.W) {
      const T* src = plane + (size_t)sr0 * g.W + sc0;
      for (int a1 = 0; a1 < nb1; ++a1)
        for (int e1 = 0; e1 < nb1; ++e1) acc += comb[a1 * nb1 + e1] * src[(size_t)a1 * g.W + e1];
    } else {
      for (int a = 0; a < g.b; ++a) {
        const int rr = R0 + a - g.hb;
        if (rr < 0 || rr >= g.H) continue;  // filter2D BORDER_CONSTANT on the warped image
        for (int e = 0; e < g.b; ++e) {
          const int cc = C0 + e - g.hb;
          if (cc < 0 || cc >= g.W) continue;
          acc += blur[a * g.b + e] * ms.template at<T>(plane, g.W, g.H, rr, cc);
        }
      }
    }
    T res = acc;
    if (WEIGHTED) {
      const size_t oi = ((size_t)k * obs_C + c + obs_c0) * n + lp;
      const T yv = y[oi], wv = dw[oi];  // requested together
      res -= yv;
      const T wr = wv * res;
      out[((size_t)kk * g.C + c) * n + lp] = wr;
      sq = (i * g.s >= g.cr0 && i * g.s < g.cr1) ? (double)wr * (double)res : 0.0;
    } else {
      if (y) res -= y[((size_t)k * obs_C + c + obs_c0) * n + lp];
      out[((size_t)kk * g.C + c) * n + lp] = res;
      // cost rows (row-band sharding): LR row i counts when its first HR row is in [cr0, cr1)
      sq = (i * g.s >= g.cr0 && i * g.s < g.cr1) ? (double)res * (double)res : 0.0;
    }
  }
  if (partials) {
    const double s = block_sum_256(sq, red);
    if (threadIdx.x == 0)
      partials[(size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
          cost_scale * s;
  }
}

template <typename T>
int launch_forward_direct(srmap_problem* p, const Geometry& g, const T* x, const T* y,
                          int obs_C, int obs_c0, T* out, int k0, int nk,
                          double* partials, int* nblocks, hipStream_t st, const T* dw) {
  const int kind = p->motion.kind() == kMotionNone ? kMotionTable : p->motion.kind();  // no table: the sampler takes the identity
  if (dw != nullptr && y == nullptr) return set_error(p->ctx, SRMAP_EINVAL, "internal: data weights without observations");
  dim3 grid((g.w * g.h + 255) / 256, g.C, nk);
  const double cost_scale = (double)g.s * (double)g.s;
  const MotionArgs<T> ma = p->motion.args<T>();
  const BlurStride bs = p->blur.stride();
  const bool launched = dispatch_value<kMotionTable, kMotionAffine, kMotionFlow, kMotionLattice>(kind, [&](auto motion) {
    constexpr int MOTION = decltype(motion)::value;
    if (dw != nullptr)
      hipLaunchKernelGGL((k_forward_direct<T, MOTION, true>), grid, dim3(256), 0, st, x, y, out, partials, g, ma,
                         p->blur.table<T>(), p->d_col_map.as<int>(), p->d_row_map.as<int>(), k0, cost_scale, obs_C, obs_c0, dw, bs);
    else
      hipLaunchKernelGGL((k_forward_direct<T, MOTION, false>), grid, dim3(256), 0, st, x, y, out, partials, g, ma,
                         p->blur.table<T>(), p->d_col_map.as<int>(), p->d_row_map.as<int>(), k0, cost_scale, obs_C, obs_c0, dw, bs);
  });
  if (!launched) return set_error(p->ctx, SRMAP_EINVAL, "internal: no forward kernel for motion kind %d", kind);
  if (nblocks) *nblocks = (int)(grid.x * grid.y * grid.z);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}


// ---------------------------------------------------------------------------
// The border ring of width `ring` (the exact border of the sub-pixel tile path): its pixels are numbered along the top
// band, the bottom band, then row by row through the left / right strips.  ring_pixel: pixel number t -> (row, column);
// false, and pixel (0, 0), for a t past the ring's last pixel.
__device__ __forceinline__ int ring_pixels(const Geometry& g, int ring) { return 2 * ring * g.W + 2 * ring * (g.H - 2 * ring); }
__device__ __forceinline__ bool ring_pixel(const Geometry& g, int ring, int t, int* rr, int* cc) {
  const int band = ring * g.W;
  const bool live = t < ring_pixels(g, ring);
  *rr = 0; *cc = 0;
  if (t < band) { *rr = t / g.W; *cc = t % g.W; }
  else if (t < 2 * band) { *rr = g.H - ring + (t - band) / g.W; *cc = (t - band) % g.W; }
  else if (live) { const int u = t - 2 * band, m = u % (2 * ring); *rr = ring + u / (2 * ring); *cc = m < ring ? m : g.W - 2 * ring + m; }
  return live;
}

// Transpose model sum_k M_k^T B^T D^T r_k (image_model.cpp:93-101) in gather
// form at every HR pixel: zero-insertion upsample (image_data.cpp:99-115),
// correlation with kernel.t() (blur_module.cpp:30-36), warpAffine(-dx,-dy)
// (motion_module.cpp:40-51); each stage clipped to the H x W domain.
// SC: the scale at compile time (2, 3, 4; 0 = run time): the divisions / remainders by it in the tap loops are
// shifts and multiplies instead of ~40-instruction sequences (the ring mode was bound by them).
template <typename T, int SC>
__global__ __launch_bounds__(256) void k_gather_direct(
    const T* __restrict__ resid, T* __restrict__ gout, Geometry g,
    const WarpTaps<T>* __restrict__ warps, const T* __restrict__ blur_t, int k0,
    int nk, T out_scale, int accumulate, int ring, int ring_groups, BlurStride bs, int obs_c0) {
  // blur_t: the flipped table; with a bank the entry of (frame, absolute channel), which changes inside the frame loop
  // (both strides are 0 without a bank)
  // ring mode: 256 / nfg pixels per block, the frames split over nfg thread groups (nfg = 16 for 16 frames and more:
  // one or a few frames per thread -- every frame costs two dependent memory round trips, its warp record and its
  // residuals, and with 4 groups a thread walked through 8 of them), combined through LDS in fixed order;
  // full mode: one pixel per thread, all frames
  const int gs = SC ? SC : g.s;
  __shared__ T part[256];
  const int nfg = ring > 0 ? ring_groups : 1, ppb = 256 / nfg;
  int hp = ring > 0 ? blockIdx.x * ppb + ((int)threadIdx.x % ppb) : blockIdx.x * 256 + threadIdx.x;
  const int fg = ring > 0 ? (int)threadIdx.x / ppb : 0;
  const int c = blockIdx.y;
  const int N = g.W * g.H, n = g.w * g.h;
  bool live = true;
  if (ring > 0) {
    int rr, cc;
    live = ring_pixel(g, ring, hp, &rr, &cc);
    hp = rr * g.W + cc;
  } else if (hp >= N) {
    return;
  }
  const int r = hp / g.W, col = hp - r * g.W;
  const T* __restrict__ blur_c = blur_t + (size_t)(c + obs_c0) * bs.channel;
  T acc = T(0);
  for (int kk = fg; kk < nk && live; kk += nfg) {
    const WarpTaps<T> wt = warps ? warps[k0 + kk] : identity_warp<T>();
    const T* rk = resid + ((size_t)kk * g.C + c) * n;
    const T* __restrict__ blur_k = blur_c + (size_t)(k0 + kk) * bs.frame;
    T tk = T(0);
    int oy = wt.oy;
    T wloc[4] = {wt.w[0], wt.w[1], wt.w[2], wt.w[3]};
    if (wt.ytab != nullptr) {  // per-row y table of the transpose warp (rounding-tie shifts)
      const int Y = wt.ytab[r];
      oy = (Y >> 5) - r;
      const float tx1 = (float)wt.fx * (1.f / 32), tx0 = 1.f - tx1;
      const float ty1 = (float)(Y & 31) * (1.f / 32), ty0 = 1.f - ty1;
      wloc[0] = (T)(ty0 * tx0); wloc[1] = (T)(ty0 * tx1); wloc[2] = (T)(ty1 * tx0); wloc[3] = (T)(ty1 * tx1);
    }
    for (int t = 0; t < wt.ntaps; ++t) {
      const int pr = r + oy + (t >> 1), pc = col + wt.ox + (t & 1);
      if (pr < 0 || pr >= g.H || pc < 0 || pc >= g.W) continue;
      // only the taps that land on the LR grid (every s-th), visited in the same increasing (a, e) order
      tk += wloc[t] * blur_t_upsampled_at(rk, blur_k, g, gs, pr, pc);
    }
    acc += tk;
  }
  if (ring > 0) {
    part[threadIdx.x] = acc;
    __syncthreads();
    if (fg != 0 || !live) return;
    acc = part[threadIdx.x];
    for (int q = 1; q < nfg; ++q) acc += part[threadIdx.x + q * ppb];
  }
  const size_t o = (size_t)c * N + hp;
  const T base = accumulate ? gout[o] : T(0);
  gout[o] = base + out_scale * acc;
}

// The ring mode of the sub-pixel tile path as its own kernel: the pixels within `ring` of the image edge, the exact
// per-stage-clipped transpose (the expression of k_gather_direct), for blur sizes <= scale (at most one blur tap per
// dimension lands on the LR grid) and frames without per-row tables.  64 pixels x 4 frame groups per block: a WAVE is one
// frame group, so a frame's warp record comes through scalar loads; a thread owns up to FP frames and issues the requests
// of ALL of them (residual + blur coefficient per warp tap, at clamped addresses, the coefficient masked) before the first
// multiply-add -- in k_gather_direct every frame was two dependent round trips inside a branchy loop (12.8 us for 57 K
// pixels at cfg2 geometry).
template <typename T, int SC, int FP>
__global__ __launch_bounds__(256) void k_gather_ring(const T* __restrict__ resid, T* __restrict__ gout, Geometry g,
                                                    const WarpTaps<T>* __restrict__ warps, const T* __restrict__ blur_t,
                                                    int nk, T out_scale, int ring, T* __restrict__ ringbuf) {
  // ringbuf != nullptr: the ring's data gradient goes to ringbuf[c][t] (t = the ring pixel's number below) instead of
  // being added to gout -- the pass then runs AHEAD of the tile kernel, which adds the value as it stores g (and can
  // produce g.d with the gradient: kernels_ztile.hip, sub-pixel WD instances)
  constexpr int gs = SC;
  __shared__ T part[256];
  const int lane = threadIdx.x & 63;
  const int fg = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int c = blockIdx.y;
  const int N = g.W * g.H, n = g.w * g.h;
  const int t = blockIdx.x * 64 + lane;
  int rr, cc;
  const bool live = ring_pixel(g, ring, t, &rr, &cc);
  const int hp = rr * g.W + cc;
  typedef const WarpTaps<T> __attribute__((address_space(4))) * WP;
  const size_t o = (size_t)c * N + hp;
  const T gold = (fg == 0 && live && ringbuf == nullptr) ? gout[o] : T(0);  // requested with everything else (the launch adds to g)
  T rv[FP][4], cf[FP][4], wq[FP][4];
  // ---- every request of this thread's frames ----
#pragma unroll
  for (int f = 0; f < FP; ++f) {
    const int kk = fg + 4 * f;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) { rv[f][tp] = T(0); cf[f][tp] = T(0); wq[f][tp] = T(0); }
    if (kk >= nk) continue;  // uniform
    WP wt = (WP)(unsigned long long)(warps + kk);
    const int oy = wt->oy, ox = wt->ox, nt = wt->ntaps;
    const T* rk = resid + ((size_t)kk * g.C + c) * n;
    // row / column part of a tap's index, once per tap row / column: the warped pixel, the blur tap that lands on the LR
    // grid ((p + a - hb) a multiple of the scale; at most one since b <= scale), the LR index, and whether all of it exists
    int ia[2], ie[2], li[2], lj[2];
    bool okr[2], okc[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int pr = rr + oy + d, pc = cc + ox + d;
      int a = (g.hb - pr) % gs, e = (g.hb - pc) % gs;
      if (a < 0) a += gs;
      if (e < 0) e += gs;
      const int R = pr + a - g.hb, Cc = pc + e - g.hb;
      ia[d] = a; ie[d] = e; li[d] = R / gs; lj[d] = Cc / gs;
      okr[d] = pr >= 0 && pr < g.H && a < g.b && R >= 0 && R < g.H && li[d] < g.h;
      okc[d] = pc >= 0 && pc < g.W && e < g.b && Cc >= 0 && Cc < g.W && lj[d] < g.w;
    }
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      if (tp >= nt) continue;  // uniform
      wq[f][tp] = wt->w[tp];
      const int dy = tp >> 1, dx = tp & 1;
      const bool ok = live && okr[dy] && okc[dx];
      const T bt = blur_t[ok ? ia[dy] * g.b + ie[dx] : 0];
      rv[f][tp] = rk[ok ? li[dy] * g.w + lj[dx] : 0];
      cf[f][tp] = ok ? bt : T(0);
    }
  }
  // ---- the sums, frame by frame, tap by tap (k_gather_direct's order within a frame) ----
  T acc = T(0);
#pragma unroll
  for (int f = 0; f < FP; ++f) {
    T tk = T(0);
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      T v = T(0);
      v += cf[f][tp] * rv[f][tp];
      tk += wq[f][tp] * v;
    }
    acc += tk;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (fg != 0 || !live) return;
  acc = part[lane];
#pragma unroll
  for (int q = 1; q < 4; ++q) acc += part[lane + q * 64];
  if (ringbuf != nullptr) ringbuf[(size_t)c * (size_t)ring_pixels(g, ring) + t] = out_scale * acc;
  else gout[o] = gold + out_scale * acc;
}

// ---------------------------------------------------------------------------
// The same transpose for a motion kind that warps per pixel (kMotionAffine, kMotionFlow, kMotionLattice), as the EXACT transpose of the
// forward kernel's matrix in gather form: g = (accumulate ? g : 0) + out_scale * sum_k M_k^T B^T D^T r_k at every HR pixel,
// frames in increasing order, per frame the kWindow x kWindow candidates q of the kind in row-major order, each weight
// recomputed by the forward kernel's expressions (MotionSampler::window / weight) -- the two kernels hold the same matrix
// bit for bit and no atomics are needed.  Per HR pixel, frame and candidate the taps of B^T D^T that land on the LR grid
// come through the caches.  SC: the scale at compile time (2, 3, 4; 0 = run time), as k_gather_direct.
template <typename T, int MOTION, int SC>
__global__ __launch_bounds__(256) void k_gather_sampled(const T* __restrict__ resid, T* __restrict__ gout, Geometry g,
                                                       MotionArgs<T> ma, const T* __restrict__ blur_t, int k0, int nk,
                                                       T out_scale, int accumulate, BlurStride bs, int obs_c0) {
  constexpr int WIN = MotionSampler<T, MOTION>::kWindow;
  const int gs = SC ? SC : g.s;
  const int hp = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const int N = g.W * g.H, n = g.w * g.h;
  if (hp >= N) return;
  const int r = hp / g.W, col = hp - r * g.W;
  const T* __restrict__ blur_c = blur_t + (size_t)(c + obs_c0) * bs.channel;  // a bank's entries: k_gather_direct
  T acc = T(0);
  for (int kk = 0; kk < nk; ++kk) {
    const MotionSampler<T, MOTION> ms(ma, g, k0 + kk);  // uniform
    const T* rk = resid + ((size_t)kk * g.C + c) * n;
    const T* __restrict__ blur_k = blur_c + (size_t)(k0 + kk) * bs.frame;  // uniform
    int qx0, qy0;
    if (!ms.window(g, hp, r, col, &qx0, &qy0)) continue;
    T tk = T(0);
    for (int dy = 0; dy < WIN; ++dy) {
      const int qy = qy0 + dy;
      if (qy < 0 || qy >= g.H) continue;
      for (int dx = 0; dx < WIN; ++dx) {
        const int qx = qx0 + dx;
        if (qx < 0 || qx >= g.W) continue;
        const size_t qi = (size_t)qy * g.W + qx;
        const double wx = ms.weight_x(qi, qx, qy, col);
        if (wx == 0.0) continue;  // a flow reads the y component only where the x weight is not zero
        const double wd = ms.weight_y(qi, qx, qy, r) * wx;
        if (wd == 0.0) continue;  // p is no tap of q
        tk += (T)wd * blur_t_upsampled_at(rk, blur_k, g, gs, qy, qx);
      }
    }
    acc += tk;
  }
  const size_t o = (size_t)c * N + hp;
  const T base = accumulate ? gout[o] : T(0);
  gout[o] = base + out_scale * acc;
}

template <typename T, int MOTION>
static void launch_gather_sampled(srmap_problem* p, const Geometry& geo, const T* resid, T* g, int k0, int nk,
                                  double out_scale, bool accumulate, hipStream_t st, int obs_c0) {
  dim3 grid((unsigned)(((size_t)geo.W * geo.H + 255) / 256), geo.C);
  const MotionArgs<T> ma = p->motion.args<T>();
  const T* bt = p->blur.table_t<T>();
  const int acc1 = accumulate ? 1 : 0;
  const BlurStride bs = p->blur.stride();
  dispatch_scale(geo.s, [&](auto sc) {
    hipLaunchKernelGGL((k_gather_sampled<T, MOTION, decltype(sc)::value>), grid, dim3(256), 0, st, resid, g, geo, ma, bt, k0, nk,
                       (T)out_scale, acc1, bs, obs_c0);
  });
}

bool gather_ring_kernel_ok(const srmap_problem* p, const Geometry& geo, int nk, int ring) {
  return ring > 0 && 2 * ring < geo.H && 2 * ring < geo.W && p->motion.has_table() && geo.b <= geo.s && geo.s >= 2 &&
         geo.s <= 4 && nk <= 16 && !p->motion.has_ytabs();
}

template <typename T>
int launch_gather_direct(srmap_problem* p, const Geometry& geo, const T* resid, T* g,
                         int k0, int nk, double out_scale, bool accumulate,
                         hipStream_t st, int ring, T* ringbuf, int obs_c0) {
  const int kind = p->motion.kind();
  if (p->blur.is_bank() && (ring > 0 || ringbuf != nullptr))
    return set_error(p->ctx, SRMAP_EINVAL, "internal: the ring pass belongs to the tile plan, which a blur bank has none of");
  if (!p->motion.is_created()) {
    if (ring > 0 || ringbuf != nullptr)
      return p->motion.refuse(p->ctx, SRMAP_EINVAL, "internal: the ring pass belongs to the tile plan, which %s has none of");
    if (!dispatch_value<kMotionAffine, kMotionFlow, kMotionLattice>(kind, [&](auto motion) {
          launch_gather_sampled<T, decltype(motion)::value>(p, geo, resid, g, k0, nk, out_scale, accumulate, st, obs_c0);
        }))
      return set_error(p->ctx, SRMAP_EINVAL, "internal: no sampled gather for motion kind %d", kind);
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  // ring > 0: only the pixels within `ring` of the image edge (the exact border of the sub-pixel tile path)
  size_t npix = (size_t)geo.W * geo.H;
  if (ring > 0) {
    if (2 * ring >= geo.H || 2 * ring >= geo.W) ring = 0;
    else npix = 2 * (size_t)ring * geo.W + 2 * (size_t)ring * (geo.H - 2 * ring);
  }
  const WarpTaps<T>* wp = p->motion.bwd_dev<T>();
  const T* bt = p->blur.table_t<T>();
  if (ringbuf != nullptr && !(accumulate && k0 == 0 && gather_ring_kernel_ok(p, geo, nk, ring)))
    return set_error(p->ctx, SRMAP_EINVAL, "internal: the ring buffer needs the ring kernel");
  if (ring > 0 && accumulate && k0 == 0 && gather_ring_kernel_ok(p, geo, nk, ring)) {
    dim3 grid((unsigned)((npix + 63) / 64), geo.C);
    // the scale, and the frames per thread of the block's four frame groups: 1, 2 or 4 (nk <= 16)
    dispatch_value<2, 3, 4>(geo.s, [&](auto sc) {
      dispatch_value<1, 2, 4>(nk <= 4 ? 1 : nk <= 8 ? 2 : 4, [&](auto fp) {
        hipLaunchKernelGGL((k_gather_ring<T, decltype(sc)::value, decltype(fp)::value>), grid, dim3(256), 0, st, resid, g, geo, wp, bt,
                           nk, (T)out_scale, ring, ringbuf);
      });
    });
    SRMAP_HIP(p->ctx, hipGetLastError());
    return SRMAP_OK;
  }
  int groups = 1;
  while (groups < 16 && groups < nk) groups *= 2;  // thread groups of the ring mode: a power of two, at most 16
  const unsigned ppb = 256u / (unsigned)groups;
  dim3 grid((unsigned)(ring > 0 ? (npix + ppb - 1) / ppb : (npix + 255) / 256), geo.C);
  dispatch_scale(geo.s, [&](auto sc) {
    hipLaunchKernelGGL((k_gather_direct<T, decltype(sc)::value>), grid, dim3(256), 0, st, resid, g, geo, wp, bt, k0, nk, (T)out_scale,
                       accumulate ? 1 : 0, ring, groups, p->blur.stride(), obs_c0);
  });
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

#define INSTANTIATE(T)                                                                      \
  template int launch_forward_direct<T>(srmap_problem*, const Geometry&, const T*,         \
                                        const T*, int, int, T*, int, int, double*, int*,   \
                                        hipStream_t, const T*);                             \
  template int launch_gather_direct<T>(srmap_problem*, const Geometry&, const T*, T*, int, \
                                       int, double, bool, hipStream_t, int, T*, int);
INSTANTIATE(float)
INSTANTIATE(double)

}  // namespace srmap
