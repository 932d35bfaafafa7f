// srmap_internal.hpp -- shared declarations of libsrmap.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "blur_model.hpp"
#include "data_weights.hpp"
#include "dev_mem.hpp"
#include "motion_model.hpp"
#include "solver_mailbox.hpp"
#include "srmap.h"

namespace srmap {

constexpr int kMaxRegularizers = 4;
constexpr int kMaxBtvRange = 8;        // alpha^(i+j) table holds 2*range+1 entries

struct Geometry {
  int W, H, C, K;  // HR size, channels, frames
  int w, h;        // LR size
  int s;           // scale
  int b, hb;       // blur kernel size (1 = none) and (b-1)/2; written by BlurModel alone (blur_model.hpp)
  int rr0, rr1;    // HR rows [rr0, rr1) whose regulariser terms (gradient AND cost) this evaluation produces
                   // (EvalReq::rr0/rr1, multiples of 8, the tile height; default 0, H)
  int cr0, cr1;    // HR rows [cr0, cr1) whose cost terms are counted (row-band sharding; default 0, H):
                   // regulariser pixels of those rows, data residuals of LR rows [cr0/s, cr1/s)
  int zlo, zhi;    // channel sharding: a halo plane exists before channel 0 / after channel C-1 of this view
                   // (3-D TV couples across it, tv_regularizer.cpp:205-222); 0 otherwise
};
static_assert(std::is_trivially_copyable_v<Geometry>, "a kernel argument: no owner inside");

struct RegSpec {
  int kind;
  int range;
  double decay;
  double lambda;
  DevBuf weights;  // device [C][H][W] dtype; empty = all ones
  double pow_table[2 * kMaxBtvRange + 1];  // std::pow(decay, k), host libm
  int gradient = SRMAP_REG_GRADIENT_REFERENCE;  // srmap_problem_set_regularizer_gradient
  // EXACT changes what the kernels compute: BTV and 3-D TV (the reference's TV gradient is the true one already)
  bool exact() const { return gradient == SRMAP_REG_GRADIENT_EXACT && kind != SRMAP_REG_TV; }
};

// solver line search: the evaluation's point is xk + stp * d (d = dvec, scaled by the factors of `norms` when given:
// cg_norm.hpp); the forward kernel forms it as it loads its window and writes it to the evaluation's x.  xk == nullptr: none
struct SpFold { const void* xk = nullptr; const void* dvec = nullptr; double stp = 0.0; const double* norms = nullptr; };

// What one evaluation is asked for beyond (terms, x, g), set by its caller for that call alone.  A default request
// evaluates the whole problem and returns nothing but the cost in d_cost[kCostValue] (srmap_eval_device).
struct EvalReq {
  // channels [c0, c0 + C) (split_channels solves one channel at a time, irls_map_solver.cpp:200-262; C = 0: all);
  // coupled: the view's neighbour planes are halo channels of a channel shard (3-D TV reads them)
  struct View { int c0 = 0, C = 0; bool coupled = false; } view;
  // HR rows [rr0, rr1) (clamped to H) whose regulariser terms this evaluation produces: frame sharding splits the
  // regulariser over the ranks by row band (tile kernels only)
  int rr0 = 0, rr1 = 1 << 30;
  // row sharding: fn(arg) posts the halo exchange of x (on another stream) and records `event` when the halo rows
  // [0, top) and [H - bot, H) are in place.  The tile kernels run the tiles that read no halo row first, then the hook,
  // then -- behind the event -- the remaining tile rows; every other path calls the hook and waits before it starts.
  struct Overlap { int (*fn)(void*) = nullptr; void* arg = nullptr; hipEvent_t event = nullptr; int top = 0, bot = 0; } overlap;
  // solver: direction d (device, dtype); the tile kernel then produces g.d with the gradient (one pass and two launches
  // fewer).  fold.xk != nullptr (fold.dvec == dvec): the tile kernel forms the point to evaluate and writes it to the x
  // the evaluation was given (no separate n-vector pass per trial point); only where ztile_can_fold() says so
  const void* dvec = nullptr;
  SpFold fold;
  // solver: host-mapped words the evaluation's finish kernel publishes {cost, g.d} to, followed by the arrival tag
  // (saves the separate publish launch); timeout_host: raised when the in-kernel finish gives up waiting
  struct Publish { double* out = nullptr; double* tag_slot = nullptr; double tag = 0.0; double* timeout_host = nullptr; } pub;
};
struct EvalOut {
  bool gd_valid = false;   // the evaluation left g.d in d_cost[kCostGd]
  bool published = false;  // its finish kernel published {cost, g.d} and the tag (EvalReq::pub)
};

struct FitPass;  // below

// the plan of the tile kernels (ztile_plan.hpp), owned by its problem
struct ZPlan;
struct ZPlanDelete { void operator()(ZPlan* z) const; };  // ztile_plan.hip

// The scalars of srmap_problem::d_cost, host and device code alike
constexpr int kCostValue = 0;    // the cost of the last evaluation
constexpr int kCostGd = 1;       // its g.d (EvalOut::gd_valid)
constexpr int kCostTimeout = 6;  // sticky: an in-kernel cost reduction gave up waiting for a workgroup (recover_reduction_timeout)
constexpr int kCostBand = 7;     // scratch of the frame shards' row-band agreement (shard_eval.hip)
constexpr int kCostSlots = 8;
// A granule of the in-kernel cost reduction that has not been published yet holds this NaN pattern (both 32-bit halves
// equal: hipMemsetD32 writes it).
constexpr unsigned kSentinel32 = 0x7FF9ABCDu;
constexpr unsigned long long kSentinel = ((unsigned long long)kSentinel32 << 32) | kSentinel32;

}  // namespace srmap

struct srmap_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string error;
  int num_cus = 0;
  // pinned host staging: two chunks for pipelined host<->device copies of caller (pageable) buffers,
  // and a small scalar block the reduction kernels write directly (no copy kernels, one sync)
  srmap::PinnedBuf h_stage[2];
  hipEvent_t h_event[2] = {nullptr, nullptr};
  srmap::PinnedBuf h_scal;   // double[kHsSlots], host-mapped: the solver's mailbox (solver_mailbox.hpp)
  void* blas = nullptr;      // rocblas_handle of this context (channel_map.hip), created on first use
};

struct srmap_problem {
  srmap_ctx* ctx = nullptr;
  srmap::Geometry geo{};
  int dtype = SRMAP_F64;
  int impl = SRMAP_IMPL_AUTO;
  bool maps_regular = true;       // decimation map == s*j on both axes
  // the forward model A_k = D B M_k: the motion and the blur in force, each with one owner -- the states, what NULL
  // restores and who re-plans: motion_model.hpp, blur_model.hpp
  srmap::MotionModel motion;
  srmap::BlurModel blur;
  srmap::DevBuf d_col_map;        // int[w]  decimation source column
  srmap::DevBuf d_row_map;        // int[h]
  // state
  srmap::DevBuf d_obs;            // [K][C][h][w] dtype
  bool have_obs = false;
  // photometric frame model (srmap_problem_set_photometric, photometric_fit.hip): while parameters are set, d_obs_raw holds
  // the frames as given and d_obs -- what every kernel reads -- their normalised copy (y - bias_k) / gain_k; d_obs_raw is
  // nullptr otherwise (and until a problem with parameters receives its first frames)
  bool photometric = false;
  std::vector<double> photo;      // K x 2 {gain, bias} (host mirror of d_photo)
  srmap::DevBuf d_photo;          // double[K][2]
  srmap::DevBuf d_obs_raw;        // [K][C][h][w] dtype
  srmap::DevBuf d_resid;          // [K][C][h][w] dtype scratch
  // per-observation weights of the data term, their prior and the loss: the states and who re-plans, data_weights.hpp
  srmap::DataWeights dw;
  // the residual scale's select (residual_scale.hip), allocated on first use: the workgroups' histogram slabs, the K + 1
  // selection states, and two records {delta, scales[1 + K], counts[1 + K]} (doubles): the last Huber step's, the diagnostic's
  srmap::DevBuf d_sel_slabs, d_sel_state, d_sel_rec;
  // the hold-out score's pass (holdout.hip), allocated by the first score and freed when the hold-out is lifted: the
  // records of its workgroups and the K rows of four sums
  srmap::FitPass* holdout_pass = nullptr;
  // the 1 + K counts of held-out observations, formed by the first srmap_problem_get_holdout that asks for them and kept
  // until the hold-out changes (empty: not formed)
  std::vector<double> holdout_counts;
  srmap::DevBuf d_regvals;        // [C][H][W] dtype scratch
  srmap::DevBuf d_x;              // [C][H][W] staging for host-buffer entry points
  srmap::DevBuf d_g;
  srmap::DevBuf d_tmp;            // [C][H][W] staging (gradient constants, values)
  srmap::DevBuf d_partials;       // per-block cost partials; the second half: those of g.d (gd_partials)
  size_t partials_cap = 0;
  srmap::DevBuf d_cost;           // [kCostSlots] reduced scalars: kCostValue, kCostGd, kCostTimeout, kCostBand
  int solver = SRMAP_SOLVER_CG;     // srmap_problem_set_solver: the inner minimiser of srmap_solve
  int lbfgs_m = 5;                  // L-BFGS history length (num_lbfgs_hessian_corrections)
  double selfcheck_beta_den = 0.0;   // largest relative deviation of the derived beta denominator from the directly summed one
  // stream ordering of the device STATE an evaluation reads (observations, IRLS weights): state_ev is recorded on the
  // stream that last wrote it asynchronously (state_stream); an evaluation on another stream waits for it once
  // (state_seen); a writer on another stream than the last evaluation's (use_stream) drains that stream first
  hipEvent_t state_ev = nullptr;
  hipStream_t state_stream = nullptr, state_seen = nullptr, use_stream = nullptr;
  // frame sharding: whether EVERY rank of the communicator can evaluate the regulariser of a row band (agreed once by an
  // all-reduce, shard_eval.hip); the key it was agreed for
  const void* band_comm = nullptr;
  unsigned long long plan_gen = 1;   // bumped whenever the tile plan or the implementation choice changes (a freed and
                                     // re-allocated plan can come back at the same address: pointer identity is no key)
  unsigned long long band_gen = 0;   // generation the agreement below was reached for
  unsigned band_terms = 0;
  bool band_all = false;
  int nreg = 0;
  srmap::RegSpec reg[srmap::kMaxRegularizers];
  std::unique_ptr<srmap::ZPlan, srmap::ZPlanDelete> zplan;  // plan of the tile kernels (ztile_plan.hip); empty = not covered
  size_t elem() const { return dtype == SRMAP_F32 ? 4 : 8; }
  size_t hr_count() const { return (size_t)geo.C * geo.H * geo.W; }
  size_t lr_count() const { return (size_t)geo.K * geo.C * geo.h * geo.w; }
};

namespace srmap {

// ---- the error text (srmap_api.hip); the context's rocBLAS handle (channel_map.hip) ----
int set_error(srmap_ctx* ctx, int status, const char* fmt, ...);
void blas_release(srmap_ctx* ctx);

#define SRMAP_HIP(ctx, call)                                                     \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess)                                                        \
      return ::srmap::set_error((ctx), SRMAP_EHIP, "%s failed: %s (%s:%d)", #call, \
                                hipGetErrorString(e_), __FILE__, __LINE__);      \
  } while (0)

// the stream of an entry point that takes one: the caller's hip_stream, or the context's when that is NULL
inline hipStream_t stream_of(const srmap_ctx* ctx, void* hip_stream) {
  return hip_stream ? (hipStream_t)hip_stream : ctx->stream;
}

// The options in force of an entry point that takes an options struct O (`name`, for the message): the library's defaults
// (set_default, the struct's srmap_*_options_default), or the caller's when given -- refused when their struct_size is not
// this library's
template <typename O>
int options_in_force(srmap_ctx* ctx, const O* options, void (*set_default)(O*), const char* name, O* opt) {
  set_default(opt);
  if (!options) return SRMAP_OK;
  if (options->struct_size != (int)sizeof(O)) return set_error(ctx, SRMAP_EINVAL, "%s.struct_size is not this library's", name);
  *opt = *options;
  return SRMAP_OK;
}

// f(T()) with T the element type of `dtype`, float or double; what f returns.  The one switch from the run-time dtype to
// the template instances: f is a generic lambda that names T as decltype of its argument
template <typename F>
auto dispatch_dtype(int dtype, F&& f) {
  if (dtype == SRMAP_F32) return f(float());
  return f(double());
}

// allocate a lazily created buffer of the problem if it is not there yet
inline int ensure(srmap_problem* p, DevBuf* buf, size_t bytes) {
  if (!*buf) SRMAP_HIP(p->ctx, buf->alloc(bytes));
  return SRMAP_OK;
}
// *dst <- a new block holding v (blocking copy)
template <typename E>
int upload_vector(srmap_problem* p, const std::vector<E>& v, DevBuf* dst) {
  SRMAP_HIP(p->ctx, dst->alloc(sizeof(E) * v.size()));
  SRMAP_HIP(p->ctx, hipMemcpy(dst->as(), v.data(), sizeof(E) * v.size(), hipMemcpyHostToDevice));
  return SRMAP_OK;
}
// where an evaluation's partials of g.d go: the second half of d_partials (ensure_eval_partials sizes both halves)
inline double* gd_partials(const srmap_problem* p) { return p->d_partials.as<double>() + p->partials_cap / 2; }

// ---- the data term's direct kernels (kernels_data_direct.hip) ----
// out = A_k x (y == nullptr) or A_k x - y_k for frames [k0, k0+nk); optional
// cost partials (s^2 * sum of squares, double) appended at partials[0..nblocks).
// `g` is the geometry of this evaluation (g.C may be a channel sub-range of the
// problem: y is indexed with the problem's channel count obs_C and offset obs_c0).
// dw != nullptr (needs y; indexed like y): the WEIGHTED instance -- out = w .* r, partials s^2 * sum(w r^2).
template <typename T>
int launch_forward_direct(srmap_problem* p, const Geometry& g, const T* x, const T* y,
                          int obs_C, int obs_c0, T* out, int k0, int nk,
                          double* partials, int* nblocks, hipStream_t st, const T* dw = nullptr);
// g = (accumulate ? g : 0) + 2 s^2 sum_k A_k^T r_k   (r: [K][C][h][w])
template <typename T>
int launch_gather_direct(srmap_problem* p, const Geometry& geo, const T* resid, T* g,
                         int k0, int nk, double out_scale, bool accumulate,
                         hipStream_t st, int ring = 0, T* ringbuf = nullptr, int obs_c0 = 0);
// (obs_c0: the problem's channel of the view's channel 0, which selects the entries of a per-channel blur bank)
// whether the ring mode (ring > 0) runs as k_gather_ring (which can also write the ring's values to a side buffer)
bool gather_ring_kernel_ok(const srmap_problem* p, const Geometry& geo, int nk, int ring);
// The one switch from a run-time int to the template instances: f(std::integral_constant<int, V>) for the one of
// VALUES... that `v` is -- a motion kind: the kinds the caller has kernel instances of; false (and no call) for any other,
// which the caller answers as an internal error
template <int... VALUES, typename F>
bool dispatch_value(int v, F&& f) {
  return ((v == VALUES && (f(std::integral_constant<int, VALUES>()), true)) || ...);
}
// the scale of the transpose kernels at compile time: f(SC) with SC = 2, 3, 4, and 0 (the kernel reads it at run time) otherwise
template <typename F>
void dispatch_scale(int s, F&& f) {
  if (!dispatch_value<2, 3, 4>(s, f)) f(std::integral_constant<int, 0>());
}
// the (scale, blur size) pairs the tile kernels (kernels_ztile.hip, kernels_spfwd.hip) are instantiated for: f(S, B) as
// integral constants; false (and no call) for any other pair
template <typename F>
bool dispatch_scale_blur(int s, int b, F&& f) {
  bool hit = false;
  dispatch_value<2, 3, 4>(s, [&](auto S) { hit = dispatch_value<1, 3>(b, [&](auto B) { f(S, B); }); });
  return hit;
}
// K matrices [a b tx; c d ty] -> records; SRMAP_EINVAL (not finite) / SRMAP_EUNSUPPORTED (outside the domain) (problem.hip)
int affine_records(srmap_ctx* ctx, int K, const double* affine_2x3, std::vector<double>* recs);
// ---- the fits' shared kernels, planning and per-pass buffers (motion_fit.hip) ----
struct AffineMap;  // affine_map.hpp
// dst[k][h/2][w/2] = mean of the 2 x 2 blocks of src[k][h][w], k < frames: one level of a box pyramid
void launch_down2_stack(const double* src, double* dst, int w, int h, int frames, hipStream_t st);
// the level sizes of that pyramid, finest first: halved while the shorter side is >= min_side, max_levels at most (0: no
// limit but the pyramid's own)
void pyramid_levels(int width, int height, int min_side, int max_levels, std::vector<int>* lw, std::vector<int>* lh);
// A pass with a thread per LR pixel (every channel of it) over the n pixels of a frame: grid (chunks, frames), 256 threads,
// a workgroup covers 256 * ppt pixels; ppt grows so that max_chunks chunks suffice
struct PixelChunks { int ppt, chunks; };
inline PixelChunks plan_pixel_chunks(int n, int max_chunks) {
  const int ppt = std::max(1, (n + 256 * max_chunks - 1) / (256 * max_chunks));
  return {ppt, (n + 256 * ppt - 1) / (256 * ppt)};
}
// One pass of a fit, and the owner of its buffers.  The fit's sums kernel writes one record of nsums doubles per workgroup
// to d_part; reduce_and_fetch() adds the records of every ROW -- a frame, an entry of a blur bank, or the one row of a fit
// over everything -- in index order (k_fit_reduce), copies rows x nsums doubles and waits for the stream once; then
// sums(row) holds the row's sums.  With a table (the fits of matrices: registration_affine.hip, motion_refinement.hip) the
// sums kernel also reads d_tab[row][kFitTabRec] = {six matrix entries, active flag, pad} and returns at once for a row
// whose flag is 0, and such a row keeps the sums of its last active pass; per pass: set() every row, upload(), the sums
// kernel, reduce_and_fetch().  Without one (photometric_fit.hip, blur_fit.hip) nothing is uploaded and every row counts.
constexpr int kFitTabRec = 8;
struct FitPass {
  int rows = 0, nsums = 0;
  DevBuf d_part, d_tab, d_sums;  // doubles; d_tab empty without a table
  PinnedBuf h_tab, h_sums;       // doubles
  // part_elems: doubles of d_part (every record of a pass; a caller may ask for more and share it).  false: an
  // allocation failed
  bool alloc(int rows_, int nsums_, size_t part_elems, bool table);
  void set(int row, const AffineMap& M, bool active);
  bool upload(hipStream_t st);
  // Row e adds `outer` groups of `inner` consecutive records, the groups outer_stride records apart, from record
  // e * row_stride on.  Also reports a failed launch of the caller's sums kernel
  bool reduce_and_fetch(int row_stride, int outer, int outer_stride, int inner, hipStream_t st);
  // the records [row][chunk] of a sums kernel with grid (chunks, rows)
  bool reduce_and_fetch(int chunks, hipStream_t st) { return reduce_and_fetch(chunks, 1, 0, chunks, st); }
  const double* sums(int row) const { return h_sums.as<const double>() + (size_t)row * nsums; }
};
// ---- residual scale (residual_scale.hip) ----
// The K + 1 lower medians of |r| over r = [K] runs of rowlen residuals (a channel view of d_resid), enqueued on st: an
// element counts where mask (nullptr: everywhere; indexed like the data weights, frames m_stride apart) is > 0.  Leaves
// {delta, 1.4826 median over all frames and per frame, the counts} in the problem's record `slot` (0: the Huber step's,
// 1: the diagnostic's); mad: delta = max(tuning * scales[0], min_delta), else 0.  Nothing returns to the host
template <typename T>
int launch_residual_scale(srmap_problem* p, const T* r, const T* mask, size_t rowlen, size_t m_stride, int slot, bool mad,
                          double tuning, double min_delta, hipStream_t st);
size_t residual_scale_record_doubles(int K);
double* residual_scale_record(srmap_problem* p, int slot);  // device; nullptr before the first select
// ---- hold-out validation (holdout.hip) ----
// out[i] = (m ? m[i] : 1) where observation i is kept, 0 where it is held out (holdout_dev.hpp), i < n the flat index into
// [K][C][h][w]; enqueued on st
template <typename T>
int launch_holdout_prior(srmap_problem* p, const T* m, T* out, size_t n, unsigned long long seed, unsigned lo, unsigned hi, hipStream_t st);
void holdout_pass_release(srmap_problem* p);  // frees the score's pass; the stream that ran it has been waited for
// ---- photometric frame model (photometric_fit.hip) ----
// d_obs <- (d_obs_raw - bias_k) / gain_k by the parameters in force, enqueued on st (allocates d_obs when it is missing)
int photometric_normalise(srmap_problem* p, hipStream_t st);
// ---- the regularisers' direct kernels (kernels_reg_direct.hip) ----
// values[c][H][W] = the regulariser's residual value at every pixel
template <typename T>
int launch_reg_values(srmap_problem* p, const Geometry& geo, const RegSpec& rs,
                      const T* x, T* values, hipStream_t st);
// the IRLS weights 1 / max(1e-5, value) in the same pass
template <typename T>
int launch_reg_weights(srmap_problem* p, const Geometry& geo, const RegSpec& rs,
                       const T* x, T* weights, hipStream_t st);
// g += d(reg)/dx with constants c = lambda_or_1 * gc[p]; optional cost partials
// lambda * w * r^2 (only meaningful when gc are the IRLS weights).
template <typename T>
int launch_reg_gradient_direct(srmap_problem* p, const Geometry& geo, const RegSpec& rs,
                               const T* x, const T* gc, double gc_scale, const T* values,
                               T* g, bool accumulate, double* partials, int* nblocks,
                               hipStream_t st);
// ---- the final reduction of per-block cost partials, fixed order (kernels_reduce.hip) ----
// `partials` must have room for n + reduce_scratch_slots(n) doubles; out[0] = sum
int reduce_scratch_slots(size_t n);
int launch_reduce_partials(srmap_problem* p, const double* partials, int n,
                           double* out, hipStream_t st);

// ---- the tile path: its plan and what reads it (ztile_plan.hip; ztile_plan.hpp for the plan itself), the kernels and
// their launch (kernels_ztile.hip), the sequence of a tile evaluation (eval.hip) ----
bool ztile_plan(srmap_problem* p);
void ztile_preload(const srmap_problem* p);
void ztile_rearm(srmap_problem* p);  // re-initialise the granules of the in-kernel cost reduction (after its time-out)
// the plan when the tile path is in force for the problem's evaluations, else nullptr
inline const ZPlan* ztile_active(const srmap_problem* p) { return p->impl != SRMAP_IMPL_DIRECT ? p->zplan.get() : nullptr; }
bool ztile_overlaps_halo(const srmap_problem* p);  // the next tile evaluation can run interior tiles under the halo exchange
bool ztile_reg_band_ok(const srmap_problem* p, unsigned terms);  // the tile kernel alone produces the regulariser part
// a TERM_ALL evaluation over C channels with a direction can form its point from xk + stp * d itself (EvalReq::fold)
bool ztile_can_fold(const srmap_problem* p, int C);
// d_resid <- A_k x - y_k (UNWEIGHTED) of the channel view geo / obs_c0, by the forward kernel the problem's evaluations use
// (the forward tile kernel where the plan has one, else the direct kernel); the cost partials it leaves are scratch
template <typename T>
int launch_forward_residual(srmap_problem* p, const Geometry& geo, int obs_c0, const T* x, double* partials, hipStream_t st);

// ---- forward tile kernel for sub-pixel shifts (kernels_spfwd.hip) ----
struct SpForwardPlan {
  DevBuf d_frames;  // per frame: integer offsets + blur (x) bilinear stencil
  int RLO = 0, CLO = 0, XR = 0, XC = 0;  // LDS window of a workgroup relative to its first LR row / cell
  bool ok = false;
  int RF0 = 0, NRF = 0, CF0 = 0, NCF = 0;  // union of the window and the workgroup's own HR block (rows / cells FOLD instances walk)
  bool can_fold = false;     // that union fits the kernel's load loop: the trial point can be formed (folded) here
};
bool spfwd_plan(srmap_problem* p, SpForwardPlan* sp);
// out[k][c][h][w] = A_k x - y_k for all frames + cost partials (one per workgroup); dw != nullptr (indexed like y): the
// WEIGHTED instances, out = w .* r and partials of w r^2
template <typename T>
int launch_forward_sp(srmap_problem* p, const Geometry& geo, const SpForwardPlan& sp, const T* x, const T* y,
                      int obs_C, int obs_c0, T* out, double* partials, int* nblocks, hipStream_t st,
                      const SpFold& fold = SpFold(), const T* dw = nullptr);

// ---- a change of the model (problem.hip): every setter checks its arguments, builds the new buffers in locals (a
// failure leaves the problem as it was), then model_drain, swap, model_replan -- for the motion and the blur inside their
// owners' install (motion_model.hip, blur_model.hip) ----
int model_drain(srmap_problem* p);    // wait for the evaluations in flight: they read the buffers about to change
void model_replan(srmap_problem* p);  // a new plan generation, the tile plan for the model now in force and its preload

// ---- evaluation (eval.hip) ----
// One ObjectiveFunction::ComputeAllTerms on device buffers, on the stream st (srmap_eval_device with a request).
int eval_dispatch(srmap_problem* p, const EvalReq& req, EvalOut* out, unsigned terms, const void* x, void* g,
                  hipStream_t st);
// d_partials sized for any evaluation of the problem (and for the forward residual of a Huber step)
int ensure_eval_partials(srmap_problem* p);
// After a device-side reduction gave up waiting for a workgroup (sticky word d_cost[kCostTimeout]; the host-mapped word
// host_word when given): re-initialise the granules behind everything in flight and clear both words.
int recover_reduction_timeout(srmap_problem* p, double* host_word);
// Stream ordering of the problem's device state (include/srmap.h, "Streams").  Before overwriting observations or
// weights on st: the last evaluation may still be reading them on another stream
int state_begin_write(srmap_problem* p, hipStream_t st);
// after an ASYNCHRONOUS write on st: later evaluations on other streams wait for this event
int state_end_write(srmap_problem* p, hipStream_t st);
// A reader of the problem's device state (observations, weights) on st that is not an evaluation (motion_refinement.hip):
// ordered after the last asynchronous state write, and recorded as the stream a later writer drains
int problem_state_read(srmap_problem* p, hipStream_t st);

// ---- the solve on device images (solver.hip; lambda_path.hip runs its rows through it) ----
// the options srmap_solve would run with: the caller's, their struct_size checked, or the defaults
int irls_options_in_force(srmap_problem* p, const srmap_irls_options* options, srmap_irls_options* out);
// srmap_solve's loop, unsharded, from x0_dev to x_out_dev ([C][H][W] of the problem dtype; distinct from each other) on
// the context's stream, complete on return.  A start that holds the caller's doubles rounded to the dtype gives srmap_solve's bits
int solve_device(srmap_problem* p, const srmap_irls_options* opt, const void* x0_dev, void* x_out_dev, srmap_solve_report* report);

// ---- L-BFGS passes (kernels_lbfgs.hip; kLbfgsMaxM and the update pass's rows: solver_mailbox.hpp) ----
// Where a pass leaves its sums: workgroup partials part[rows][gridDim.x], ticket (0 between passes), the reduced sums in
// out_dev (device, may be null) and out_host (host-mapped), then `tag` at tag_slot behind a system-scope fence.
struct LbfgsRed {
  double* part;
  unsigned* ticket;
  double* out_dev;
  double* out_host;
  double* tag_slot;
  double tag;
};
static_assert(std::is_trivially_copyable_v<LbfgsRed>, "a kernel argument: no owner inside");
// coefficients of the direction over the basis: c[0] for g, c[1 + 2j] for s_j, c[2 + 2j] for y_j
struct LbfgsCoef {
  double c[1 + 2 * kLbfgsMaxM];
};
static_assert(std::is_trivially_copyable_v<LbfgsCoef>, "a kernel argument: no owner inside");
// ring slot p <- (s, y) = (x - xk, g - gk); sums [kLbGg] g.g, [kLbSs] s.s, then per slot j < live [lb_row(j, .)]: s.y_j,
// y.s_j, y.y_j, g.s_j, g.y_j (lb_rows(live) rows)
template <typename T>
int launch_lbfgs_update(const T* x, const T* xk, const T* g, const T* gk, T* S, T* Y, int p, int live, size_t n, int nb,
                        const LbfgsRed& red, hipStream_t st);
// dn = -(c_g g + sum_{j < live} c_sj s_j + c_yj y_j); sums {max|dn|, dn.dn, g.dn}
template <typename T>
int launch_lbfgs_direction(T* dn, const T* g, const T* S, const T* Y, int live, const LbfgsCoef& c, size_t n, int nb,
                           int keep_dn, const LbfgsRed& red, hipStream_t st);

// ---- conversions / staging (transfer.hip) ----
int ensure_staging(srmap_ctx* ctx);
int convert_upload(srmap_problem* p, const double* host, void* dev, size_t n,
                   hipStream_t st);
int convert_download(srmap_problem* p, const void* dev, double* host, size_t n,
                     hipStream_t st);
// The HR image of a host-buffer fit entry point into p->d_x (allocated on first use), enqueued on the context's stream.
// The caller has made every check that needs no device: an error there leaves the problem, this buffer included, untouched
int stage_host_x(srmap_problem* p, const double* x_host);
// The prologue of the host form of a fit that takes the HR image (blur_fit.hip, photometric_fit.hip,
// motion_refinement.hip).  The checks that need no device come first, so that an error leaves the problem (its staging
// buffer included) untouched: the options' struct_size, before_obs(p, opt) (opt: the options in force), observations
// present, after_obs(p, opt); then stage_host_x.  The caller goes on to the device form with p->d_x on the context's stream
struct NoFitCheck {
  template <typename O>
  int operator()(srmap_problem*, const O&) const { return SRMAP_OK; }
};
template <typename O, typename BeforeObs = NoFitCheck, typename AfterObs = NoFitCheck>
int host_fit_prologue(srmap_problem* p, const double* x_host, const O* options, void (*set_default)(O*), const char* name,
                      BeforeObs before_obs = BeforeObs(), AfterObs after_obs = AfterObs()) {
  O opt;
  if (int rc = options_in_force(p->ctx, options, set_default, name, &opt)) return rc;
  if (int rc = before_obs(p, opt)) return rc;
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "no observations set");
  if (int rc = after_obs(p, opt)) return rc;
  return stage_host_x(p, x_host);
}

}  // namespace srmap
