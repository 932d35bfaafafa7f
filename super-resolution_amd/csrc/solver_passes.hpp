// solver_passes.hpp -- the n-vector passes of the inner solvers (solver_passes.hip): where a pass reduces over (Owned),
// where it leaves its sums (Fin), and one host launcher per pass.
//
// Every launcher picks the kernel instance itself: V = 16 / sizeof(T) consecutive elements per thread and step when n is
// a multiple of V (one 16-byte request; the vectors are device allocations: aligned), else V = 1.  The element-wise results are
// the same bits either way, the dot-product partials are summed in a different order (tests/test_gpu_parity.py: the PSNR
// bar of the ill-conditioned small cases follows the CPU reference path's own sensitivity to a last-bit perturbation,
// DESIGN.md section 4).  The reducing passes take their grid (nb <= kRedBlocks workgroups of 256) from the caller: it
// fixes the order of the additions.  The element-wise ones (axpy_out, fill) cover n with ceil(n / 256) workgroups.
#pragma once

#include "srmap_internal.hpp"

namespace srmap {

constexpr int kRedBlocks = 1024;

// A granule of the one-launch reductions that has not been published yet holds this NaN pattern in both halves
// (hipMemsetD32 arms the [3][kRedBlocks] granules with it).
constexpr unsigned kArm32 = 0x7FF9ABCDu;

// Which elements of an n-vector a rank owns: element range [e0, e1) (channel block) and, inside each H x W plane,
// rows [r0, r1) (row band).  on == 0: everything.
struct Owned {
  size_t e0, e1;
  int W, H, r0, r1;
  int on;
  __device__ __forceinline__ bool has(size_t i) const {
    if (!on) return true;
    if (i < e0 || i >= e1) return false;
    const int row = (int)((i / (size_t)W) % (size_t)H);
    return row >= r0 && row < r1;
  }
};
static_assert(std::is_trivially_copyable_v<Owned>, "a kernel argument: no owner inside");

// Where a pass leaves its reduced sums.  gran == nullptr: the two-launch scheme (block partials in `part`, k_finish
// follows; sharded solves, whose sums go through an all-reduce first).  Otherwise the last block of the grid reduces:
// out[0 .. rows) (device or host-mapped), the evaluation's cost forwarded from cost_src to out[rows], pub_n further
// device scalars copied to pub_dst (host-mapped), then the arrival tag behind a system-scope fence.
struct Fin {
  unsigned long long* gran;
  double* out;
  const double* cost_src;
  const double* pub_src;
  double* pub_dst;
  int pub_n;
  double* tag_slot;
  double tag;
  double* timeout_flag;   // sticky device word: a reduction gave up waiting for a block (srmap_solve reports it)
  double* timeout_host;   // the same event for the host at once (host-mapped word: wait_tag ends the solve on it)
};
static_assert(std::is_trivially_copyable_v<Fin>, "a kernel argument: no owner inside");

// dn = -g + beta dk (dk may be null; beta_dev, when given, overrides beta); sums {max|dn|, dn.dn, g.dn}
template <typename T>
void launch_cg_direction(T* dn, const T* g, const T* dk, T beta, size_t n, const Owned& ow, double* part, const Fin& fin,
                         const double* beta_dev, double* norms_pub, int keep_dn, int nb, hipStream_t st);
// sums {g.g, g.y [, y.dk_check]} with y = g - gp; beta_dst, when given, receives max(0, min(g.g, g.y) / vv)
template <typename T>
void launch_cg_beta_dots(const T* gp, const T* g, size_t n, const Owned& ow, double* part, const Fin& fin, double* beta_dst,
                         int restart, double vv, const T* dk_check, int nb, hipStream_t st);
// sum {a.b}
template <typename T>
void launch_cg_dot(const T* a, const T* b, size_t n, const Owned& ow, double* part, const Fin& fin, int nb, hipStream_t st);
// d = (dn s1) s2 from norms = {max|dn|, dn.dn}; x1 (may be null) = xk + stp1 d
template <typename T>
void launch_cg_normalize(T* d, const T* dn, const double* norms, size_t n, const T* xk, T* x1, T stp1, int nb,
                         hipStream_t st);
// dst = a + alpha b
template <typename T>
void launch_axpy_out(T* dst, const T* a, const T* b, T alpha, size_t n, hipStream_t st);
// d[0 .. n) = v
template <typename T>
void launch_fill(T* d, T v, size_t n, hipStream_t st);
// second stage of the two-launch scheme: rows (<= 3) x nb partials -> out[0 .. rows) (+ extra_src -> out[rows]), then the tag
void launch_finish(const double* part, int nb, int rows, int max0, double* out, const double* extra_src, double* tag_slot,
                   double tag, hipStream_t st);
// dst[0 .. n) = src[0 .. n) (device scalars -> host-mapped memory), then the tag
void launch_publish(double* dst, const double* src, int n, double* tag_slot, double tag, hipStream_t st);

}  // namespace srmap
