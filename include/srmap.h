/*
 * srmap.h -- C ABI of libsrmap.so: the MI355X-native (HIP, gfx950) MAP
 * super-resolution gradient path.
 *
 * This is the drop-in boundary for ONE path of rteammco/super-resolution: the
 * per-iteration MAP cost + gradient (ObjectiveFunction::ComputeAllTerms) and
 * the operators and solver loop around it.  The reference has no FFI of its
 * own -- the path sits behind plain C++ virtual interfaces -- so every entry
 * point below names the reference interface it replaces (file:line relative to
 * the reference repository), and super-resolution_amd/host/ holds C++ classes
 * with the reference's names that forward here.
 *
 * Conventions
 *   - every function returns an srmap_status (0 = ok); nothing aborts or throws
 *     across the ABI; srmap_last_error() gives the message.  The reference's
 *     CHECK-class violations (glog abort) map to SRMAP_EINVAL.
 *   - images are planar [C][H][W], index c*W*H + row*W + col (util.cpp:81-89);
 *     LR stacks are [K][C][h][w].  Host buffers are IEEE double, owned by the
 *     caller.  Device buffers passed to *_device entry points hold the
 *     problem's dtype (double or float) and are owned by the caller.
 *   - one context = one GPU (one process per GPU); a problem is used from one
 *     host thread at a time.
 *   - there is no CPU fallback: without a usable HIP device every entry point
 *     that computes fails with SRMAP_EHIP.
 *
 * Streams (the ordering contract of every entry point that takes a DEVICE pointer)
 *   - a context owns one NON-BLOCKING HIP stream: it is not ordered against the
 *     legacy default stream or any other stream.  Every *_device entry point
 *     takes `hip_stream` (a hipStream_t; NULL = the context's stream) and
 *     enqueues ALL its work there, so a device buffer the caller produced on
 *     stream S is ordered by passing S -- or by completing S first.  Nothing the
 *     library enqueues runs on the legacy stream.
 *   - entry points that take HOST pointers (srmap_eval, srmap_solve*,
 *     srmap_cg_trace, srmap_apply*, srmap_reg_values*, srmap_set_observations,
 *     srmap_set_irls_weights, srmap_set_data_weights, srmap_get_data_weights, srmap_channel_map, srmap_channel_pca,
 *     srmap_register_translational, srmap_register_affine, srmap_refine_motion, srmap_fit_blur, srmap_upload / srmap_download) run on the
 *     context's stream and are complete when they return.
 *   - the problem's device state (observations, IRLS weights, data weights) is ordered by the
 *     library itself: a write through srmap_update_irls_weights_device / srmap_update_data_weights_device on one
 *     stream is waited for (an event) by evaluations on another, and a writer
 *     first drains the stream of the LAST evaluation when it is a different one.
 *     Only that one: a problem may have evaluations in flight on ONE stream at a
 *     time (it owns one set of cost partials and scratch buffers anyway) -- finish
 *     the evaluations on stream A (or order B after A) before evaluating the same
 *     problem on stream B.  srmap_set_observations_device is complete when it returns.
 *   - srmap_eval_device / srmap_eval_sharded_device with cost == NULL return
 *     right after enqueueing; x_dev / g_dev must stay alive and untouched by
 *     other streams until the stream reaches that point.
 *
 * Input domain
 *   - pixel values, observations and weights are finite IEEE numbers.  The tile
 *     kernels stage x multiplied by 2^512 (f64) / 2^64 (f32) (an exact scaling
 *     that turns the regulariser's sign() into a clamp):
 *     results equal the reference's for |x| < 2^508 (f64) / 2^60 (f32) and for
 *     pixel differences that are 0 or >= 2^-512 (f64) / 2^-64 (f32) in
 *     magnitude.  (Beyond 2^511 the reference's own cost, a sum of squared
 *     residuals, overflows.)  Inputs outside that range: force
 *     SRMAP_IMPL_DIRECT, which has no such scaling.
 */
#ifndef SRMAP_H_
#define SRMAP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srmap_ctx srmap_ctx;
typedef struct srmap_problem srmap_problem;

typedef enum {
  SRMAP_OK = 0,
  SRMAP_EINVAL = 1,       /* a reference CHECK would have fired */
  SRMAP_ENOMEM = 2,
  SRMAP_EHIP = 3,         /* HIP runtime / device error */
  SRMAP_EUNSUPPORTED = 4  /* valid for the reference, not representable here */
} srmap_status;

typedef enum { SRMAP_F64 = 0, SRMAP_F32 = 1 } srmap_dtype;

/* Regularizer kinds: TotalVariationRegularizer (tv_regularizer.h),
 * the same with SetUse3dTotalVariation(true), and
 * BilateralTotalVariationRegularizer (btv_regularizer.h). */
typedef enum { SRMAP_REG_TV = 0, SRMAP_REG_TV3D = 1, SRMAP_REG_BTV = 2 } srmap_reg_kind;

/* Which ObjectiveTerms an evaluation includes (objective_function.h:18-26). */
enum {
  SRMAP_TERM_DATA = 1u,  /* ObjectiveDataTerm */
  SRMAP_TERM_REG = 2u,   /* every ObjectiveIRLSRegularizationTerm */
  SRMAP_TERM_ALL = 3u
};

/* Kernel family selection (for tests and A/B measurements).  AUTO picks the
 * workgroup-tile kernels whenever the problem geometry admits them (scale
 * 2..4, blur size 1 or 3, integer or sub-pixel shifts), else the direct
 * kernels.  TILED forces that family and fails with SRMAP_EUNSUPPORTED when it
 * does not cover the problem.  (Value 3 was round 5's marching evaluation
 * kernel: bit-equal to the tiles, not faster on gfx950 -- profiles/r05_march.txt
 * -- and removed from the library in round 6; srmap_problem_set_impl answers
 * SRMAP_EINVAL for it.) */
typedef enum { SRMAP_IMPL_AUTO = 0, SRMAP_IMPL_DIRECT = 1, SRMAP_IMPL_TILED = 2 } srmap_impl;

/* ---------------------------------------------------------------- context */
/* Binds HIP device `device_id`.  Replaces nothing in the reference (it has no
 * device notion); it is what a maintainer creates once per process. */
int srmap_ctx_create(int device_id, srmap_ctx** out);
void srmap_ctx_destroy(srmap_ctx* ctx);
const char* srmap_last_error(const srmap_ctx* ctx);
/* Library/version string, e.g. "srmap 0.1 (gfx950)". */
const char* srmap_version(void);
/* Diagnostic: the device and pinned-host blocks the library holds in this process (memory handed out by
 * srmap_device_alloc is the caller's and not counted).  0 once every problem, context and communicator is destroyed;
 * unchanged by any call that keeps no new state -- a leak test that free-memory queries on a shared GPU cannot give. */
long long srmap_live_allocations(void);

/* ---------------------------------------------------------------- problem */
/* ImageModelParameters + MapSolver geometry: image_model.h:26-44,
 * ImageModel::CreateImageModel image_model.cpp:17-61, MapSolver::MapSolver
 * map_solver.cpp:52-86. */
typedef struct {
  int hr_width, hr_height;  /* HR image size (= LR size * scale when solving) */
  int channels;             /* C */
  int frames;               /* K observations / motion shifts */
  int scale;                /* DownsamplingModule scale >= 1 */
  const double* shifts_xy;  /* K x (dx, dy) MotionShift; NULL = no MotionModule */
  int blur_ksize;           /* BlurModule "blur_radius" = kernel size (odd);
                               0 (or sigma <= 0) = no BlurModule */
  double blur_sigma;
  int dtype;                /* srmap_dtype: arithmetic/storage type on device */
} srmap_problem_desc;

int srmap_problem_create(srmap_ctx* ctx, const srmap_problem_desc* desc,
                         srmap_problem** out);
void srmap_problem_destroy(srmap_problem* p);
/* Under frame sharding (srmap_eval_sharded_device / srmap_solve_sharded with SRMAP_SHARD_FRAMES) this call and the
 * regulariser calls (add / clear) are COLLECTIVE: every rank makes them in the same order between the same
 * evaluations -- the ranks agree by an all-reduce on how the regulariser is split whenever one of them changes. */
int srmap_problem_set_impl(srmap_problem* p, int impl /* srmap_impl */);
/* The family the next evaluation will run (SRMAP_IMPL_DIRECT / TILED): how a caller learns that AUTO fell
 * back to the direct kernels (geometry outside the tile kernels' coverage, or a sub-pixel shift on a 1/32-px
 * rounding tie, whose per-row table only the direct kernels read). */
int srmap_problem_active_impl(const srmap_problem* p, int* impl);

/* Affine per-frame motion model (no reference counterpart: MotionModule warps by a translation only,
 * motion_module.cpp:18-51, and registration.cpp keeps nothing but the translation of what it fits).
 * affine_2x3: K x 6 doubles, row-major [a b tx; c d ty] per frame, in HR pixel coordinates, (x, y) order.  With
 * F_k(p) = L_k p + t_k, content at p in the HR image sits at F_k(p) in frame k's HR-grid image (MotionShift's
 * convention: L = I, t = (dx, dy) is the shift (dx, dy)).
 *   forward   (M_k x)(q) = four-tap bilinear sample of x at s = F_k^-1(q); a tap outside the image contributes 0.  Then
 *             the blur and the decimation of the translational model apply unchanged: A_k = D B M_k.
 *   coords    s is computed in double for both dtypes and is exact (no 1/32-px quantisation: a set of pure translations
 *             is a DIFFERENT definition from shifts_xy unless the shifts are multiples of 1/32 px off the rounding ties,
 *             where the two agree).  F_k^-1 is formed once on the host in double.  The weights are rounded to the dtype.
 *   adjoint   M_k^T is the exact transpose of that matrix (not a warp by the inverse map), so the gradient
 *             2 s^2 sum_k M_k^T B^T D^T (w_k .* r_k) is the true gradient of the cost; it is gathered without atomics:
 *             two evaluations of one input give bit-identical gradients.
 *   domain    all numbers finite, else SRMAP_EINVAL; max(|a-1|+|b|, |c|+|d-1|) <= 0.25 (about +-7 degrees of rotation
 *             with a few percent of scale or shear), else SRMAP_EUNSUPPORTED; on an error the problem keeps its motion.
 * NULL restores the motion the problem was created with (shifts_xy or none).  The call works on problems created with or
 * without shifts_xy and persists across srmap_set_observations and the data-weight calls.  While an affine motion is
 * set, the direct kernel family runs (srmap_problem_active_impl answers SRMAP_IMPL_DIRECT; SRMAP_IMPL_TILED answers
 * SRMAP_EUNSUPPORTED at evaluation) -- also when every L_k is exactly I.  srmap_eval*, srmap_apply, srmap_apply_transpose
 * (the exact adjoint), srmap_solve (CG, L-BFGS, split_channels), the traces, srmap_problem_set_cost_rows and the robust
 * data term honour it.  Evaluations and solves sharded over a communicator of more than one rank answer
 * SRMAP_EUNSUPPORTED.  Not thread-safe against evaluations of the same problem; evaluations already enqueued are waited
 * for.  srmap_register_affine estimates the matrices from the frames (srmap_register_translational finds translations
 * only); its output goes straight into this call. */
int srmap_problem_set_affine_motion(srmap_problem* p, const double* affine_2x3);

/* Dense per-frame displacement-field motion model (no reference counterpart; csrc/kernels_flow.hip): the
 * general motion, of which a translation and an affine map are special cases.
 * flow: K x 2 x H x W, the (ux, uy) planes of every frame on its HR-grid image, in HR pixels.
 *   forward   (M_k x)(q) = four-tap bilinear sample of x at s = q + u_k(q), q an integer pixel of frame k's HR-grid image;
 *             a tap outside the image contributes 0 (the affine model's sample).  The blur in force (Gaussian or
 *             free-form) and the decimation apply unchanged: A_k = D B M_k.  MotionShift (dx, dy) corresponds to
 *             u = (-dx, -dy), an affine F_k to u(q) = F_k^-1(q) - q.
 *   storage   the field is kept in the problem's dtype (host doubles are rounded once; the _device form takes that dtype).
 *             s = (double)q + (double)u is exact for both dtypes; the weights are the double products rounded to the
 *             dtype, as in the affine model.  Device memory: K*2*H*W*sizeof(dtype) for the field plus K*H*W*4 bytes of
 *             gather seeds (and the same again, transiently, while a new field is validated).
 *   adjoint   M_k^T is the exact transpose of that matrix, gathered per HR pixel without atomics: two evaluations of one
 *             input give bit-identical gradients.  For an HR pixel p the contributing q (those with q + u(q) strictly
 *             inside p +- 1 per axis) are looked for in the 5 x 5 window around a seed stored per (k, p) when the field is
 *             set: the fixed point of q <- round(p - u(clamp(q))) from q = p, at most 16 steps.
 *   domain    VERIFIED when the field is set, by walking the forward direction: every (q, p) pair the forward kernel
 *             multiplies must lie inside p's window.  Any violation (a fold, shear beyond the window) answers
 *             SRMAP_EUNSUPPORTED; an entry that is not finite (in the problem's dtype) SRMAP_EINVAL; |u| > 2^20
 *             SRMAP_EUNSUPPORTED; on an error the problem keeps the motion it had.  Sufficient for acceptance: with
 *             dx = max_q |u(q + e_x) - u(q)|_inf and dy likewise along y, dx + dy <= 0.4 (then u is 0.4-Lipschitz in the
 *             max norm, the seed ends within 1.5 / (1 - 0.4) + 0.4^16 * 2^20 < 3 of every contributing q).
 *             Every affine map of srmap_problem_set_affine_motion's domain with |t| <= 2^20 is accepted (its field is
 *             1/3-Lipschitz).
 * A flow and an affine motion are alternatives: setting one replaces the other, and NULL (to either call) restores the
 * motion the problem was created with (shifts_xy or none).  The flow persists across srmap_set_observations, the
 * data-weight calls, srmap_problem_set_blur_kernel and srmap_problem_set_photometric.  While a flow is set the direct
 * kernel family runs (srmap_problem_active_impl answers SRMAP_IMPL_DIRECT; SRMAP_IMPL_TILED answers SRMAP_EUNSUPPORTED at
 * evaluation).  srmap_eval*, srmap_apply, srmap_apply_transpose (the exact adjoint), srmap_solve (CG, L-BFGS,
 * split_channels), the traces, srmap_problem_set_cost_rows, the robust data term, a free-form blur and the photometric
 * parameters honour it.  srmap_refine_motion (it fits matrices), srmap_fit_blur and srmap_fit_photometric (they have no
 * sampling leg for a field) answer SRMAP_EUNSUPPORTED while a flow is set, as do evaluations and solves sharded over a
 * communicator of more than one rank.  Not thread-safe against evaluations of the same problem; evaluations already
 * enqueued are waited for.  The _device form reads flow_dev on hip_stream (NULL = the context's) and returns when the
 * field is validated and installed.  srmap_problem_get_flow: *is_set, and the field in force as doubles when flow_out is
 * not NULL and a flow is set. */
int srmap_problem_set_flow(srmap_problem* p, const double* flow_host /* K x 2 x H x W doubles; NULL restores */);
int srmap_problem_set_flow_device(srmap_problem* p, const void* flow_dev /* problem dtype */, void* hip_stream);
int srmap_problem_get_flow(srmap_problem* p, double* flow_out /* K x 2 x H x W, optional */, int* is_set);

/* The displacement-field model with the field kept on a CONTROL LATTICE and interpolated in the kernels (no reference
 * counterpart; csrc/kernels_flow.hip, csrc/sample_dev.hpp): the compact form of srmap_problem_set_flow,
 * s^2 to step^2 times smaller, and exactly what srmap_register_flow's input-level estimate is.
 *   lattice   step >= 1 HR pixels between nodes, lw x lh nodes per component; node (i, j) sits at HR pixel (i step, j step).
 *             nodes: K x 2 x lh x lw doubles (x then y component), kept on the device as DOUBLES in both dtypes.
 *   field     for the HR pixel Q = (x, y), in double, in this order, without fused operations:
 *               cx = min(max((double)x / (double)step, 0), lw - 1);  xi = min(floor(cx), lw - 2);  fx = cx - xi  (cy, yi, fy likewise)
 *               v  = (1 - fy) ((1 - fx) n[yi][xi] + fx n[yi][xi+1]) + fy ((1 - fx) n[yi+1][xi] + fx n[yi+1][xi+1])
 *               u(Q) = (dtype) v
 *             -- srmap_register_flow's output rule with the gain folded into the nodes.  Beyond the last node the field is
 *             constant.  From u(Q) on everything is srmap_problem_set_flow's: the sample, the weights, the seed rule, the
 *             5 x 5 window and the verified domain (checked on the interpolated values, with the same codes).  A lattice
 *             problem evaluates BIT FOR BIT as a dense-flow problem given the expanded nodes, in both dtypes.
 *   domain    1 <= step <= 1024; lw, lh >= 2; (lw - 1) step < W + step and (lh - 1) step < H + step; else SRMAP_EINVAL.
 *             The registration's form is lw = w, lh = h, step = scale; the covering form lw = ceil((W - 1) / step) + 1.
 *   memory    K*2*lw*lh*8 bytes of nodes plus the K*H*W*4 bytes of gather seeds (a dense field: K*2*H*W*sizeof(dtype)).
 * Lattice, dense flow and affine motion are alternatives: setting one replaces the others, NULL (to any of the calls)
 * restores the created motion, and on a refused lattice the problem keeps its motion.  While a lattice is set
 * srmap_problem_get_flow reports is_set = 0.  The lattice persists across the calls a dense flow persists across, every
 * call that honours a dense flow honours it, and every call that answers SRMAP_EUNSUPPORTED under a dense flow
 * (SRMAP_IMPL_TILED, sharding over more than one rank, srmap_refine_motion, srmap_fit_blur, srmap_fit_blur_bank,
 * srmap_fit_photometric) answers it under a lattice.  The _device form reads nodes_dev (doubles) on hip_stream (NULL = the
 * context's) and returns when the lattice is validated and installed.  srmap_problem_get_flow_lattice: *step (0 = none),
 * *lw, *lh, and the nodes in force when nodes_out is not NULL and a lattice is set. */
int srmap_problem_set_flow_lattice(srmap_problem* p, int step, int lw, int lh,
                                   const double* nodes_host /* K x 2 x lh x lw doubles; NULL restores */);
int srmap_problem_set_flow_lattice_device(srmap_problem* p, int step, int lw, int lh, const double* nodes_dev, void* hip_stream);
int srmap_problem_get_flow_lattice(srmap_problem* p, int* step, int* lw, int* lh, double* nodes_out /* optional */);

/* Free-form blur kernel (no reference counterpart: BlurModule builds an isotropic Gaussian from (blur_radius, sigma) only,
 * blur_module.cpp:13-22).  taps: ksize x ksize doubles, row-major, the layout of the Gaussian the problem
 * builds itself.  The forward model CORRELATES with them, as filter2D does (blur_module.cpp:24-28):
 *   (B z)(R, C) = sum_{a,e} taps[a][e] z(R + a - hb, C + e - hb),  hb = (ksize - 1) / 2,  z = 0 outside the image.
 *   domain    ksize odd, 1 ... 7; it may differ from the blur_ksize the problem was created with.  Taps finite; no sign and
 *             no sum is imposed and the call does not normalise.  A tap that is not finite, an even ksize or ksize < 1:
 *             SRMAP_EINVAL; ksize > 7: SRMAP_EUNSUPPORTED; on an error the problem keeps its blur.
 *   adjoint   B^T is the exact transpose: the correlation with the kernel FLIPPED IN BOTH AXES, taps[ksize-1-a][ksize-1-e]
 *             (the reference correlates with kernel.t(), blur_module.cpp:30-36, which is the same thing only for a kernel
 *             that is symmetric under both flips, as its Gaussian is).  The gradient is the true gradient of the cost.
 *   NULL      restores the blur the problem was created with (the Gaussian, or none) and its size, bit for bit: evaluations
 *             before and after a set / restore pair are bit-identical.
 * While a free-form kernel is set the direct kernel family runs (srmap_problem_active_impl answers SRMAP_IMPL_DIRECT;
 * SRMAP_IMPL_TILED answers SRMAP_EUNSUPPORTED at evaluation) -- also when the taps equal the Gaussian's; evaluations and
 * solves sharded over a communicator of more than one rank answer SRMAP_EUNSUPPORTED.  It works with no motion, shifts_xy
 * and an affine motion, with data weights and the Huber loss; srmap_eval*, srmap_apply, srmap_apply_transpose, srmap_solve
 * (CG, L-BFGS, split_channels), the traces, srmap_problem_set_cost_rows and srmap_refine_motion honour it.  It persists
 * across srmap_set_observations, the data-weight calls and srmap_problem_set_affine_motion.  Not thread-safe against
 * evaluations of the same problem; evaluations already enqueued are waited for.  srmap_fit_blur estimates the taps from a
 * known HR image. */
int srmap_problem_set_blur_kernel(srmap_problem* p, int ksize, const double* taps);
/* The blur in force (no reference counterpart; blur_module.cpp keeps its kernel private): *ksize (1 = no blur) and, when
 * taps_out is not NULL, its ksize x ksize taps (at most 15 x 15 doubles for a created Gaussian, 7 x 7 for a free-form one). */
int srmap_problem_get_blur_kernel(const srmap_problem* p, int* ksize, double* taps_out);

/* Blur-kernel bank: a point-spread function per frame, per channel or per (frame, channel) (no reference counterpart;
 * DESIGN.md 3.14).  The forward model becomes y_k,c = D B_{k,c} M_k x_c: a burst whose frames carry different streaks or
 * lenses, a cube whose PSF differs from band to band.
 *   taps      entries x ksize x ksize doubles, each entry row-major; entries = K (PER_FRAME), C (PER_CHANNEL) or K * C
 *             (PER_FRAME_CHANNEL, stored [k][c]).  The bank has ONE ksize: the caller zero-pads a smaller kernel.
 *   meaning   every entry means what srmap_problem_set_blur_kernel says of its kernel: the forward model CORRELATES with
 *             it, taps outside the image contribute 0, nothing is normalised, negative taps are allowed; the adjoint is
 *             the exact transpose (entry (k, c) flipped in both axes) and the gradient is the cost's gradient.
 *   domain    the single kernel's: an even ksize, ksize < 1, a tap that is not finite or an unknown mode: SRMAP_EINVAL;
 *             ksize > 7: SRMAP_EUNSUPPORTED; on an error the problem keeps the blur it had.
 *   NULL      restores the blur the problem was created with, bit for bit (as srmap_problem_set_blur_kernel(p, 0, NULL)).
 * A bank and the single free-form kernel are alternatives: setting one replaces the other.  While a bank is set
 * srmap_problem_get_blur_kernel returns the bank's ksize and, asked for taps, answers SRMAP_EUNSUPPORTED
 * (srmap_problem_get_blur_bank returns them); srmap_fit_blur answers SRMAP_EUNSUPPORTED (its ridge and its energy at the
 * kernel in force have no single kernel to refer to: srmap_fit_blur_bank is the call).  The direct kernel family runs
 * (srmap_problem_active_impl answers SRMAP_IMPL_DIRECT, SRMAP_IMPL_TILED answers SRMAP_EUNSUPPORTED at evaluation) and
 * calls sharded over more than one rank answer SRMAP_EUNSUPPORTED.  Every motion kind (none, shifts_xy, affine, flow), data
 * weights, the prior, the Huber loss, the photometric parameters, srmap_eval*, srmap_apply, srmap_apply_transpose,
 * srmap_solve (CG, L-BFGS, split_channels -- a per-channel entry goes by the problem's channel), the traces,
 * srmap_problem_set_cost_rows, srmap_refine_motion and srmap_fit_photometric honour the bank; it persists across the
 * observation, weight, prior, loss, motion, flow and photometric calls.  A bank whose entries are all equal evaluates bit
 * for bit as srmap_problem_set_blur_kernel with those taps does. */
typedef enum { SRMAP_BLUR_PER_FRAME = 1, SRMAP_BLUR_PER_CHANNEL = 2, SRMAP_BLUR_PER_FRAME_CHANNEL = 3 } srmap_blur_bank_mode;
int srmap_problem_set_blur_bank(srmap_problem* p, int mode, int ksize, const double* taps /* entries x ksize x ksize; NULL restores */);
/* The bank in force: *mode (0 = none set), *ksize and, when taps_out is not NULL and a bank is set, its entries x ksize x ksize taps. */
int srmap_problem_get_blur_bank(const srmap_problem* p, int* mode /* 0 = none */, int* ksize, double* taps_out /* optional */);

/* Inner minimiser of srmap_solve: MapSolverOptions::least_squares_solver and num_lbfgs_hessian_corrections
 * (enum LeastSquaresSolver { CG_SOLVER, LBFGS_SOLVER }, map_solver.h:20-51; the choice irls_map_solver.cpp:97-113;
 * the CLI's --solver=cg|lbfgs, super_resolution.cpp:98-99, 134-141).  SRMAP_SOLVER_CG (mincg, alglib_objective.cpp:47-75)
 * is the default of every problem.  SRMAP_SOLVER_LBFGS runs ALGLIB's minlbfgs with m = num_lbfgs_hessian_corrections
 * history pairs and mincg's stopping conditions (alglib_objective.cpp:111-140), default preconditioner.  The history is
 * kept on the device (2 m vectors of the problem's size).  An unknown solver or m < 1 (ALGLIB asserts m >= 1):
 * SRMAP_EINVAL; m > 8: SRMAP_EUNSUPPORTED (ALGLIB recommends 3 <= m <= 7, map_solver.h:47-50).  For CG, m is checked
 * the same way and kept for a later switch to L-BFGS.  L-BFGS solves sharded over a communicator of more than one rank
 * answer SRMAP_EUNSUPPORTED; unsharded and split_channels solves are supported. */
typedef enum { SRMAP_SOLVER_CG = 0, SRMAP_SOLVER_LBFGS = 1 } srmap_solver;
int srmap_problem_set_solver(srmap_problem* p, int least_squares_solver /* srmap_solver */,
                             int num_lbfgs_hessian_corrections);

/* Row-band sharding (no reference counterpart: the reference is single-process).
 * A rank that owns HR rows [r0, r1) of a larger image creates its problem on the
 * band extended by halo rows and restricts the COST to the rows it owns:
 * regulariser pixels of HR rows [hr_row0, hr_row1) and data residuals of LR rows
 * [hr_row0/scale, hr_row1/scale) (rows relative to this problem; multiples of the
 * scale).  The gradient is always produced for every row; the caller keeps the
 * owned ones.  Default: the whole image. */
int srmap_problem_set_cost_rows(srmap_problem* p, int hr_row0, int hr_row1);

/* LR size the model produces: (int)(len * (1.0/scale)),
 * DownsamplingModule::ApplyToImage downsampling_module.cpp:19-27. */
int srmap_problem_lr_size(const srmap_problem* p, int* lr_width, int* lr_height);

/* MapSolver's low_res_images (map_solver.cpp:52-86): [K][C][h][w] doubles at LR
 * resolution.  (The reference stores them NN-upsampled to HR; this library
 * keeps LR and accounts for the s*s replication arithmetically.)  Requires
 * hr size == lr size * scale. */
int srmap_set_observations(srmap_problem* p, const double* lr_host);
/* Same from a device buffer holding the problem dtype, copied on hip_stream
 * (NULL = the context's stream); complete on return. */
int srmap_set_observations_device(srmap_problem* p, const void* lr_dev, void* hip_stream);

/* MapSolver::AddRegularizer(regularizer, regularization_parameter)
 * map_solver.cpp:88-94; constructors tv_regularizer.h / btv_regularizer.cpp
 * :50-65 (range >= 1, 0 < decay <= 1).  Gradients are bug-compatible with the
 * reference.  In that reference mode the gradient of BTV with btv_range = 1 is identically
 * zero (the differentiated window [0, R-1] holds the pixel itself only): such a regulariser adds to the cost and leaves
 * the minimiser alone; srmap_problem_set_regularizer_gradient(.., SRMAP_REG_GRADIENT_EXACT) gives it its true gradient.
 * *reg_index receives the handle. */
int srmap_add_regularizer(srmap_problem* p, int kind, double lambda,
                          int btv_range, double btv_decay, int* reg_index);
int srmap_clear_regularizers(srmap_problem* p);
/* The gradient regulariser `reg` contributes (no reference counterpart).  The cost lambda sum w r^2, the
 * values r and the IRLS weights 1 / max(1e-5, r) are the same in both modes; with c[q] = lambda w[q] held fixed:
 *   REFERENCE (default)  the reference's gradients, bug for bug: BTV differentiates the window i, j in [0, R-1] although
 *             r sums [0, R] and never takes the absolute pixel (0, 0) as a source; 3-D TV has no -sgn dz in the self term.
 *   EXACT     the gradient of the cost.  BTV:
 *               g[p] += 2 c[p] r[p] sum_{i,j in [0,R], p+(i,j) inside} a^(i+j) sgn(x[p] - x[p+(i,j)])
 *                     - sum_{i,j in [0,R], (i,j) != (0,0), q = p-(i,j) inside} 2 c[q] r[q] a^(i+j) sgn(x[q] - x[p])
 *             with sgn(0) = 0.  3-D TV: the self term is -sgn dx - sgn dy - sgn dz, the last where the next channel
 *             exists.  2-D TV: the reference's gradient is the true one; EXACT runs the same kernels, bit for bit.
 * srmap_eval*, srmap_reg_values_and_gradient, srmap_solve (CG, L-BFGS, split_channels), the traces, the lambda paths and
 * srmap_problem_set_cost_rows honour the mode.  A BTV regulariser in EXACT mode is not fused into the tile kernels: the
 * tiles keep the data term and the direct kernels add the regulariser.  While a BTV or 3-D TV regulariser is EXACT,
 * evaluations and solves sharded over a communicator of more than one rank answer SRMAP_EUNSUPPORTED (the exact BTV
 * gradient reaches one halo row further than the shard description promises).  An unknown mode or handle:
 * SRMAP_EINVAL.  Waits for the evaluations in flight and re-plans as srmap_problem_set_regularizer_lambda does; the mode
 * persists across every other setter. */
typedef enum { SRMAP_REG_GRADIENT_REFERENCE = 0, SRMAP_REG_GRADIENT_EXACT = 1 } srmap_reg_gradient;
int srmap_problem_set_regularizer_gradient(srmap_problem* p, int reg, int mode);
int srmap_problem_get_regularizer_gradient(const srmap_problem* p, int reg, int* mode);
/* The regularization_parameter of regulariser `reg` (the handle srmap_add_regularizer gave), changed in place: the kind,
 * the BTV constants and the IRLS weights stay as they are.  No reference counterpart (the reference fixes it at
 * AddRegularizer).  lambda must be finite and >= 0, the handle must exist: SRMAP_EINVAL otherwise.  Waits for the
 * evaluations in flight and re-plans as srmap_add_regularizer does. */
int srmap_problem_set_regularizer_lambda(srmap_problem* p, int reg, double lambda);
int srmap_problem_get_regularizer_lambda(const srmap_problem* p, int reg, double* lambda);
/* The irls_weights_ vector an ObjectiveIRLSRegularizationTerm holds
 * (objective_irls_regularization_term.h:40); NULL = all ones. */
int srmap_set_irls_weights(srmap_problem* p, int reg, const double* w_host);
/* w = 1 / max(1e-5, regularizer(x)) on device, irls_map_solver.cpp:128-143.
 * Enqueued on hip_stream (NULL = the context's stream) and NOT waited for:
 * later evaluations on any stream are ordered after it by the library. */
int srmap_update_irls_weights_device(srmap_problem* p, int reg, const void* x_dev, void* hip_stream);

/* ------------------------------------------- robust data term (weights, Huber) */
/* Per-observation weights of the data term (no reference counterpart: the reference's data term is plain least
 * squares, objective_data_term.cpp:29-50).  With weights w, shaped and indexed exactly like the observations
 * ([K][C][h][w]; the channel views of split_channels and the rows of srmap_problem_set_cost_rows apply to them as to
 * the observations), the data cost is s^2 sum_k sum_i w[k][i] r[k][i]^2 and its gradient 2 s^2 sum_k A_k^T (w[k] .* r[k]),
 * r[k] = A_k x - y_k.  A weight of 0 removes a pixel ("ignore these pixels": dead pixels, a frame that failed to
 * register).  NULL = all ones: the unweighted kernels, today's behaviour.  Weights must be finite and >= 0
 * (SRMAP_EINVAL otherwise; the device form trusts the caller).  They persist across srmap_set_observations.
 * A problem with weights (or a Huber loss) evaluates through weighted instances of the forward kernels; the tile
 * family then takes its forward-residual plan for integer shifts too (forward kernel, ring pass, tile gather: DESIGN.md
 * section 3.5), and a problem without a MotionModule (shifts_xy == NULL) runs the direct family.  Solves and evaluations
 * sharded over a communicator of more than one rank answer SRMAP_EUNSUPPORTED for such a problem. */
int srmap_set_data_weights(srmap_problem* p, const double* w_host);
/* The same from a device buffer holding the problem dtype, copied on hip_stream (NULL = the context's stream);
 * complete on return.  No reference counterpart. */
int srmap_set_data_weights_device(srmap_problem* p, const void* w_dev, void* hip_stream);
/* The current EFFECTIVE weights ([K][C][h][w] host doubles; ones if none are set; with a data prior, srmap_set_data_prior,
 * the product with it): after a Huber solve, the outlier map -- the pixels the solve down-weighted.
 * No reference counterpart. */
int srmap_get_data_weights(srmap_problem* p, double* w_host);
/* Loss of the data term (no reference counterpart).  SRMAP_DATA_LOSS_L2: the quadratic above with the caller's
 * weights, which a solve leaves untouched.  SRMAP_DATA_LOSS_HUBER: srmap_solve minimises
 * s^2 sum rho(r), rho(r) = r^2 for |r| <= huber_delta and huber_delta (2 |r| - huber_delta) beyond, by IRLS: the data
 * weights are reset to 1 where the regulariser's are, and re-derived from the iterate after every inner run
 * (srmap_update_data_weights_device) together with the regulariser's; the loop runs its rounds even without a
 * regulariser; the reported cost is the weighted quadratic cost of the last inner run.  Huber OWNS the weight buffer:
 * weights the caller set are overwritten by the solve (a mask that must hold under Huber is a data prior:
 * srmap_set_data_prior below), and srmap_get_data_weights afterwards returns the final Huber weights.  huber_delta is in the units of the observations;
 * it must be finite and > 0 for HUBER (ignored for L2).  An unknown loss or a bad delta: SRMAP_EINVAL. */
typedef enum { SRMAP_DATA_LOSS_L2 = 0, SRMAP_DATA_LOSS_HUBER = 1 } srmap_data_loss;
int srmap_problem_set_data_loss(srmap_problem* p, int loss /* srmap_data_loss */, double huber_delta);
/* One Huber re-weighting step (no reference counterpart): w = 1 where |r| <= huber_delta, huber_delta / |r| elsewhere,
 * r = A x - y at x_dev (UNWEIGHTED residuals: one forward pass plus one elementwise pass over [K][C][h][w]).  Needs a
 * HUBER loss.  Enqueued on hip_stream and not waited for, ordered like srmap_update_irls_weights_device. */
int srmap_update_data_weights_device(srmap_problem* p, const void* x_dev, void* hip_stream);
/* A persistent prior m on the data weights (no reference counterpart): [K][C][h][w] host doubles, finite
 * and >= 0 (SRMAP_EINVAL otherwise; the device form takes the problem dtype and trusts the caller); NULL removes it and
 * restores the weights as they would be without it.  While a prior is set the weights every kernel reads are
 * w_eff = m .* w, the product formed in the problem's dtype with one rounding, w being what the rules above give: under L2
 * the caller's weights (kept in a second buffer while a prior is set) or ones; under HUBER the Huber weights -- the reset at
 * the start of a solve gives w_eff = m, every re-weighting (the solver's and srmap_update_data_weights_device) gives
 * m .* huber(r) of the UNWEIGHTED residual.  A validity mask therefore holds under a Huber loss.  srmap_get_data_weights
 * returns the EFFECTIVE weights.  The prior persists across srmap_set_observations and the weight, loss, motion, blur and
 * photometric calls.  A problem with a prior is weighted in every respect stated at srmap_set_data_weights (weighted
 * forward instances, SRMAP_EUNSUPPORTED for sharded solves and evaluations); srmap_refine_motion, srmap_fit_blur and
 * srmap_fit_photometric read the effective weights. */
int srmap_set_data_prior(srmap_problem* p, const double* m_host);
int srmap_set_data_prior_device(srmap_problem* p, const void* m_dev, void* hip_stream);
/* is_set: 1 while a prior is set; m_host (optional, [K][C][h][w] doubles) receives it (ones if none is set). */
int srmap_get_data_prior(srmap_problem* p, double* m_host, int* is_set);
/* The residual scale and the automatic Huber delta (no reference counterpart).  The scale of a set of
 * residuals is 1.4826 * the LOWER MEDIAN of |r|: the order statistic of 0-based rank (n - 1) / 2 among the n counted
 * observations -- an element of the input, never an average, found by an exact radix select on the device, so it does
 * not depend on any order of summation or arrival.  An observation counts, under an L2 loss, when its effective weight is
 * > 0 (all count when no weights are set) and, under a HUBER loss, when its prior is > 0 (all count without a prior: the
 * Huber weights themselves are never zero).  A selection with n = 0 has scale 0 and count 0.  A NaN residual orders above
 * +inf by its bits; that is not an error.
 *
 * srmap_problem_set_huber_scale: where a Huber step takes its delta from.  SRMAP_HUBER_DELTA_FIXED, the default of every
 * problem: srmap_problem_set_data_loss's huber_delta, today's behaviour bit for bit.  SRMAP_HUBER_DELTA_MAD: every
 * re-weighting (the solver's and srmap_update_data_weights_device) uses
 * delta = max(tuning * 1.4826 * median|r|, min_delta), the median over ALL counted observations of the step's own
 * unweighted residuals (of the step's channel under split_channels), formed on the device between the residual pass and
 * the weight pass; srmap_problem_set_data_loss's huber_delta is still checked and is unused.  tuning must be finite and
 * > 0 (1.345 is the usual value: 95 % efficiency on normal residuals), min_delta finite and > 0: the floor keeps a perfect
 * fit from producing delta = 0 (1e-4 suits observations in 0...1).  An unknown mode or a bad value: SRMAP_EINVAL (values
 * are not checked for FIXED).  The mode persists across the loss, weight, prior, motion, blur and photometric calls and
 * is read under a HUBER loss only.  One scale over all frames drives delta on purpose: a scale per frame would grant a
 * misregistered frame a large delta of its own (README, "Residual scale"). */
typedef enum { SRMAP_HUBER_DELTA_FIXED = 0, SRMAP_HUBER_DELTA_MAD = 1 } srmap_huber_delta_mode;
int srmap_problem_set_huber_scale(srmap_problem* p, int mode /* srmap_huber_delta_mode */, double tuning, double min_delta);
/* The delta, the scales ([0] over all frames, [1 + k] of frame k) and the counts of the last Huber step in the MAD mode
 * (zeros before the first); waits for that step through an event recorded behind it, so the step's stream need not
 * exist any more.  In the FIXED mode: the fixed delta and zeros.  Every output is optional. */
int srmap_problem_get_huber_delta(srmap_problem* p, int* mode, double* delta, double* scales /* 1 + K, optional */,
                                  double* counts /* 1 + K, optional */);
/* The diagnostic on its own, under any loss and any model state: scales[0] = 1.4826 * median|A x - y~| over all counted
 * observations, scales[1 + k] the same of frame k (a frame that fits worse than the others -- misregistered, wrongly
 * exposed -- stands out), counts the numbers of counted observations.  y~: what every kernel reads, the normalised frames
 * under the photometric model.  x_host: [C][H][W] doubles; the device form takes the problem dtype, read on hip_stream
 * (NULL = the context's).  Complete on return.  Without observations: SRMAP_EINVAL. */
int srmap_residual_scale(srmap_problem* p, const double* x_host, double* scales /* 1 + K */, double* counts /* 1 + K, optional */);
int srmap_residual_scale_device(srmap_problem* p, const void* x_dev, void* hip_stream, double* scales, double* counts);

/* ------------------------------------------- hold-out validation (mask, score) */
/* A hold-out keeps a pseudo-random share of the observations out of the data term, so that how well A x predicts them
 * measures a solve without the ground truth (no reference counterpart).  Observation i -- the flat index
 * into the whole problem's [K][C][h][w], as a 64-bit unsigned integer, the same under a split_channels view -- is held out
 * iff (z >> 40) < T, T = floor(fraction * 2^24) formed in double, and (mod 2^64)
 *     z = i + seed * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *     z ^= z >> 31.
 * fraction must be in (0, 0.5] with T >= 1; 0 lifts the hold-out; anything else: SRMAP_EINVAL.  The hold-out is a factor
 * of the data prior: while it is set, everything that reads the prior -- the evaluation kernels through the effective
 * weights, a Huber step, the count rule of the residual scale, the fits -- sees m .* (1 - h) (m = ones without a prior),
 * formed once by an elementwise kernel; srmap_get_data_prior still returns the caller's m, srmap_get_data_weights the
 * effective weights (0 where held out).  A problem with a hold-out evaluates and solves bit for bit as one whose caller set
 * the prior m .* (1 - h) itself, and is weighted in every respect stated at srmap_set_data_weights.  It persists across
 * srmap_set_observations and the weight, prior, loss, motion, blur and photometric calls; lifting it restores the weights
 * as they would be without it and frees what it allocated.  Solves and evaluations sharded over a communicator of more
 * than one rank answer SRMAP_EUNSUPPORTED.  As under a prior, the caller's weights are kept in a second buffer while a hold-out
 * is set; a HUBER loss owns the weight buffer (srmap_problem_set_data_loss), so when a hold-out is set under HUBER, or the
 * loss returns from HUBER to L2, that buffer holds the last Huber weights: set the weights again (NULL for none) after
 * leaving HUBER -- the effective weights and the L2 base weight of srmap_holdout_score are formed from it. */
int srmap_problem_set_holdout(srmap_problem* p, double fraction, unsigned long long seed);
/* A hold-out given as a FOLD of a partition.  Both forms are one band test on v = z >> 40, the top 24 bits of the mix:
 * observation i is held out iff lo <= v < hi.  srmap_problem_set_holdout is the band [0, T); fold `fold` of `folds` is
 *     lo = floor(fold * 2^24 / folds),  hi = floor((fold + 1) * 2^24 / folds)       (integer arithmetic)
 * so the bands of folds 0 ... folds - 1 meet end to start, the first begins at 0 and the last ends at exactly 2^24: every
 * observation is in exactly one fold.  folds must be in 2...32 and 0 <= fold < folds; folds == 0 lifts the hold-out;
 * anything else: SRMAP_EINVAL, the message naming this call.  In every other respect it IS the hold-out above -- a factor
 * of the prior, persistent across the setters, refused when sharded --; a fold and a fraction replace each other, and 0 in
 * either call lifts whichever is set.  srmap_problem_get_holdout then reports fraction = (hi - lo) / 2^24, and the mask
 * and the counts of the band. */
int srmap_problem_set_holdout_fold(srmap_problem* p, int folds, int fold, unsigned long long seed);
/* The fold in force: *folds (0: none, or a fraction is set), *fold, *seed.  Every output is optional. */
int srmap_problem_get_holdout_fold(srmap_problem* p, int* folds, int* fold, unsigned long long* seed);
/* The hold-out in force: *fraction (0: none) and *seed; mask_out ([K][C][h][w] doubles, 1 = held out) as the device
 * computes it; counts[0] the held-out observations, counts[1 + k] those of frame k.  Every output is optional. */
int srmap_problem_get_holdout(srmap_problem* p, double* fraction, unsigned long long* seed, double* mask_out /* optional */,
                              double* counts /* 1 + K, optional */);
/* The score of the held-out observations at x: one forward-residual pass (as srmap_residual_scale's: every model state)
 * and ONE streaming launch that recomputes h from the index and accumulates, per frame and in a fixed order without
 * atomics (bit-identical from run to run), over the held-out observations
 *     S1 = sum u rho(r),  S2 = sum u rho(r)^2,  S0 = sum u,  n = #{u > 0},        r = A x - y~
 * (y~ as at srmap_residual_scale).  u is the BASE weight: what the observation would weigh were it not held out, before
 * any Huber factor -- under L2 the caller's prior times the caller's weights (each 1 when absent, the product rounded once
 * in the problem's dtype), under HUBER the caller's prior.  rho: delta == 0: r^2;  delta > 0: the Huber function, r^2 for
 * |r| <= delta and 2 delta |r| - delta^2 beyond (under outliers the mean squared residual is dominated by the corrupted
 * held-out pixels and says nothing);  delta < 0: "the problem's" -- 0 under L2, the fixed delta under HUBER / FIXED, the
 * last Huber step's delta under MAD, read on the device from that step's record (SRMAP_EINVAL if no step has run since the
 * loss and the scale rule in force were set).
 * score[0] = sum_k S1_k / sum_k S0_k with the frames added in index order, score[1 + k] = S1_k / S0_k (0 where S0_k = 0);
 * sums (optional): (1 + K) x 4 doubles {S1, S2, S0, n}, row 0 the totals -- S2 and n let a caller form a standard error.
 * The rows of srmap_problem_set_cost_rows do not apply: the score covers the whole frames.  Without observations, without
 * a hold-out, or when no held-out observation has a base weight above 0: SRMAP_EINVAL.  x_host: [C][H][W] doubles; the
 * device form takes the problem dtype, read on hip_stream (NULL = the context's).  Complete on return. */
int srmap_holdout_score(srmap_problem* p, const double* x_host, double delta, double* score /* 1 + K */, double* sums /* (1 + K) x 4, optional */);
int srmap_holdout_score_device(srmap_problem* p, const void* x_dev, void* hip_stream, double delta, double* score, double* sums);

/* ------------------------------------------------------- operators (host) */
/* ImageModel::ApplyToImage(ImageData*, index) image_model.cpp:86-91:
 * hr [C][H][W] -> lr [C][h][w]. */
int srmap_apply(srmap_problem* p, int frame, const double* hr, double* lr);
/* ImageModel::ApplyTransposeToImage image_model.cpp:93-101:
 * lr [C][h][w] -> hr [C][h*s][w*s]. */
int srmap_apply_transpose(srmap_problem* p, int frame, const double* lr, double* hr);
/* Regularizer::ApplyToImage regularizer.h:13-30 (values only). */
int srmap_reg_values(srmap_problem* p, int reg, const double* x, double* values);
/* Regularizer::ApplyToImageWithDifferentiation regularizer.h:32-45: values and
 * the gradient for the given per-pixel gradient_constants. */
int srmap_reg_values_and_gradient(srmap_problem* p, int reg, const double* x,
                                  const double* gradient_constants,
                                  double* values, double* gradient);

/* ---------------------------------------------------------- objective */
/* ObjectiveFunction::ComputeAllTerms(x, gradient) objective_function.cpp:5-20
 * restricted to `terms`: zeroes the gradient, then adds the selected terms.
 * grad may be NULL (cost only, objective_function.h:23). */
int srmap_eval(srmap_problem* p, unsigned terms, const double* x, double* cost,
               double* grad);
/* Device-resident form: x_dev / g_dev hold the problem dtype ([C][H][W]).
 * Work is enqueued on `hip_stream` (NULL = the context's stream, which is a
 * NON-BLOCKING stream: it does not order itself against the legacy default
 * stream, so buffers produced by other streams must be complete -- or pass the
 * producing stream here).  When
 * cost != NULL the call synchronises the stream and returns the cost; when
 * cost == NULL it returns right after enqueueing (the cost stays on device
 * until srmap_last_cost()). */
int srmap_eval_device(srmap_problem* p, unsigned terms, const void* x_dev,
                      void* g_dev, double* cost, void* hip_stream);
int srmap_last_cost(srmap_problem* p, double* cost);

/* Device memory helpers for C/C++ hosts that do not bring their own allocator
 * (element = the problem dtype). */
int srmap_device_alloc(srmap_ctx* ctx, size_t bytes, void** dev);
int srmap_device_free(srmap_ctx* ctx, void* dev);
int srmap_upload(srmap_problem* p, const double* host, void* dev, size_t count);
int srmap_download(srmap_problem* p, const void* dev, double* host, size_t count);
int srmap_synchronize(srmap_ctx* ctx);

/* ---------------------------------------------- spectral (channel) maps */
/* out[r][p] = sum_c M[r][c] * (in[c][p] - offset_in[c]) + offset_out[r] on planar
 * images in[rows_in][n], out[rows_out][n] (host, double): the per-pixel
 * projection of SpectralPCA::GetPCAImage / ReconstructImage
 * (spectral_pca.cpp:94-161: cv::PCA::project / backProject pixel by pixel),
 * done as one dense contraction on the GPU (rocBLAS DGEMM: this is the one place
 * on the path where the matrix cores apply).  M is rows_out x rows_in, row
 * major; the offsets may be NULL (zero). */
int srmap_channel_map(srmap_ctx* ctx, int rows_out, int rows_in, size_t n,
                      const double* M, const double* offset_in,
                      const double* offset_out, const double* in_host,
                      double* out_host);

/* The same on device-resident planar f64 cubes (in_dev [rows_in][n], out_dev [rows_out][n]); M and the offsets
 * are host arrays.  Enqueued on hip_stream (NULL = the context's stream); returns when the result is complete. */
int srmap_channel_map_device(srmap_ctx* ctx, int rows_out, int rows_in, size_t n,
                             const double* M, const double* offset_in,
                             const double* offset_out, const double* in_dev,
                             double* out_dev, void* hip_stream);
/* SpectralPCA training (spectral_pca.cpp:30-88 over cv::PCA): mean, covariance / count and its
 * eigen-decomposition of `count` spectral samples, on the GPU (row means, centred samples, the covariance as one
 * DGEMM, rocSOLVER dsyevd).  samples_host is planar [rows][count].  Outputs (host): mean[rows],
 * eigenvalues[rows] in descending order, basis[rows][rows] with row k = k-th eigenvector, its
 * largest-magnitude component positive. */
int srmap_channel_pca(srmap_ctx* ctx, int rows, size_t count, const double* samples_host,
                      double* mean_out, double* eigenvalues_out, double* basis_out);
/* The same on a device-resident planar f64 cube in_dev [rows][n]: the samples are the pixels
 * first + j * stride, j < count.  Enqueued on hip_stream (NULL = the context's stream); returns when the
 * (host) results are complete. */
int srmap_channel_pca_device(srmap_ctx* ctx, int rows, size_t n, const double* in_dev,
                             size_t first, size_t stride, size_t count, double* mean_out,
                             double* eigenvalues_out, double* basis_out, void* hip_stream);

/* ------------------------------------------------------- registration */
/* registration::TranslationalRegistration (src/motion/registration.h:19-22, registration.cpp:161-201): the
 * shift (dx, dy) of every image relative to the first one -- content at p in image 0 sits at p + (dx, dy) in
 * image i, the convention of MotionModule / MotionShift -- estimated on the GPU (box pyramid, exhaustive
 * integer search coarse to fine, Gauss-Newton sub-pixel refinement; see csrc/registration.hip for why this is
 * not the reference's OpenCV feature pipeline).  images_host: num_images planes [height][width] (the reference
 * registers on channel 0, registration.cpp:41-46).  shifts_xy_out: 2 * num_images doubles, image 0 -> (0, 0).
 * num_images == 0 returns SRMAP_OK and writes nothing (registration.cpp:165-168).  SRMAP_EINVAL when no shift
 * can be determined (the reference CHECK-fails, registration.cpp:193-194): width or height < 8, and a pixel of any
 * image that is not finite ("registration: image %d is not finite"; nothing is written), and a refinement step that
 * is not finite (finite pixels whose products overflow; the images before that one are answered).
 *   pyramid   2 x 2 box means (an odd last row / column is dropped); a level is added while min(w, h) > 64 -- 64 x 64 is
 *             one level, 65 x 65 is two (the other fits halve while min(w, h) >= 64) --, at most 12 levels;
 *   search    R0 = max(4, min(16, min side of the coarsest level / 4)) around 0 there, +-1 around twice the coarser answer
 *             on every finer level; mean squared difference over the overlap; the FIRST minimum in row-major candidate
 *             order wins, so a textureless pair, where every candidate ties, answers (-R0, -R0) 2^(levels - 1) with
 *             separation 0 and is not an error;
 *   refine    at most 20 Gauss-Newton passes over the pixels ceil(max(|dx|, |dy|)) + 2 from every edge, none when fewer than
 *             4 rows or columns remain (the integer shift stands); clamped to the integer shift +-1. */
int srmap_register_translational(srmap_ctx* ctx, int num_images, int width, int height,
                                 const double* images_host, double* shifts_xy_out);
/* What this estimator is NOT: the reference finds features (BRISK), fits a RANSAC homography / rigid transform and
 * keeps its translation, so it tolerates some rotation, scale and outliers.  This one assumes a PURE TRANSLATION
 * of at most a quarter of the frame (16 pixels of the coarsest pyramid level), has no outlier rejection, and its
 * sub-pixel step stays within +-1 px of the integer search.  On periodic texture it can lock onto a wrong period;
 * rotation / scale between frames bias the result.  The _ex form reports how trustworthy each shift is --
 * quality_out (optional, 2 doubles per image): [2i] separation = 1 - best / runner-up mean squared difference of
 * the coarsest search (runner-up at least 2 coarse pixels away; near 1 = one clear minimum, near 0 = ambiguous),
 * [2i + 1] the root mean squared residual at the returned shift (of the last refinement pass evaluated), -1 when the
 * frame is too small for a refinement pass at the integer shift.  Callers with real (non-synthetic) stacks
 * should check both, or supply shifts from their own registration (MotionShiftSequence accepts any). */
int srmap_register_translational_ex(srmap_ctx* ctx, int num_images, int width, int height,
                                    const double* images_host, double* shifts_xy_out, double* quality_out);

/* Affine registration (no reference counterpart; csrc/registration_affine.hip): for every image
 * k >= 1 the 2 x 3 matrix [a b tx; c d ty] of F_k(p) = L_k p + t_k with I_k(F_k(p)) ~= I_0(p) -- content at p of image 0
 * sits at F_k(p) in image k, the convention of srmap_problem_set_affine_motion and of MotionShift.  Image 0 gets the
 * identity.  All arithmetic is f64.
 *   pyramid   2 x 2 box means of every image (an odd last row / column is dropped), halved while min(w, h) >= 64 (the
 *             coarsest level's shorter side is 32...63), at most 12 levels; max_levels caps the count;
 *   seed      coarsest level: exhaustive integer search, R = max(4, min(16, min side / 4)), mean squared difference over
 *             the fixed template window [R, w-R) x [R, h-R), first minimum in row-major order; skipped when
 *             initial_affine_2x3 is given (the matrices are then taken down the pyramid);
 *   steps     inverse-compositional Gauss-Newton, coarse to fine, over the template pixels at least 1 px from the border
 *             whose four bilinear taps in image k are inside it (others are left out, not sampled as zero); a level ends
 *             when the four image corners move less than step_tolerance (pixels of that level) or after max_iterations.
 * With hr_scale = s the returned t is s * t and L is unchanged: the matrices of LR frames in the HR pixel units that
 * srmap_problem_set_affine_motion takes (the decimation samples HR pixel s u for LR pixel u: no offset term).
 * What this estimator is and is NOT: it is DENSE (every pixel votes, no features); it has NO outlier rejection (moving
 * objects, occlusions and saturated regions bias it); its domain is the affine model's, max(|a-1|+|b|, |c|+|d-1|)
 * <= 0.25, and a translation within R pixels of the coarsest level unless initial matrices are given; PERIODIC texture
 * can alias to a wrong period (the separation below shows it); it registers ONE plane per image.
 * quality_out (optional, 4 doubles per image): [4i] separation of the coarse minimum as srmap_register_translational_ex
 * defines it (1 when an initial matrix was given), [4i+1] root mean squared residual I_k(F(p)) - I_0(p) at the result
 * (full resolution), [4i+2] the fraction n / (w h) of pixels that pass used, [4i+3] Gauss-Newton passes over all levels.
 * Image 0: (1, 0, 1, 0).
 * num_images == 0 returns SRMAP_OK and writes nothing.  SRMAP_EINVAL: width or height < 8; a pixel of any image that is not
 * finite ("affine registration: image %d is not finite"; nothing is written); a struct_size that is not this
 * library's; hr_scale < 1, max_iterations < 1, max_levels < 0 or a negative step_tolerance; an initial matrix (rows
 * 1...num_images-1; row 0 is ignored) that is not finite or outside the domain; and "Could not determine motion between
 * images." when a pass has fewer than 0.25 w h usable pixels or an iterate leaves the domain.  A level without texture
 * (the 6 x 6 Cholesky factorisation fails) keeps its matrix and is not an error.  Results are bit-identical run to run and
 * do not depend on the other images of the stack. */
typedef struct {
  int struct_size;                   /* filled by the _default call; a mismatch is SRMAP_EINVAL */
  int hr_scale;                      /* 1 */
  int max_iterations;                /* 30, per level */
  double step_tolerance;             /* 1e-4 px */
  int max_levels;                    /* 0 = automatic; 1 = full resolution only */
  const double* initial_affine_2x3;  /* NULL = coarse search; else num_images x 6, input-pixel units */
} srmap_affine_registration_options;
void srmap_affine_registration_options_default(srmap_affine_registration_options* options);
int srmap_register_affine(srmap_ctx* ctx, int num_images, int width, int height, const double* images_host,
                          const srmap_affine_registration_options* options /* NULL = defaults */,
                          double* affine_2x3_out /* num_images x 6 */, double* quality_out /* optional, 4 per image */);

/* Dense flow registration (no reference counterpart; csrc/registration_flow.hip; it closes what DESIGN.md
 * 3.11 left out: the estimate of the fields srmap_problem_set_flow takes).  For every image k >= 1 a displacement field u_k
 * on image k's grid with I_0(q + u_k(q)) ~= I_k(q) -- the convention of srmap_problem_set_flow, image 0 playing x.  Image 0
 * gets u = 0.  All arithmetic is f64, every operation rounded on its own (no fused multiply-adds).
 *   pyramid   2 x 2 box means of every image (an odd last row / column is dropped), halved while min(w, h) >= 32 (the
 *             coarsest level's shorter side is 16...31: the field needs the coarse levels for its range), at most 12
 *             levels; max_levels caps the count;
 *   start     u = 0 at the coarsest level; with initial_affine_2x3 (the matrices of srmap_register_affine, input pixels)
 *             u(q) = F_k^-1(q) - q of the matrix taken down the pyramid -- rotations and shifts beyond the pyramid's range;
 *   transfer  u_fine(q) = 2 * bilinear(u_coarse at (q - 1/2) / 2), coordinates clamped to the coarse image;
 *   pass      `warps` passes per level, a fixed count (no convergence test, nothing returns to the host).  At s = q + u(q):
 *             Tw and the central-difference gradient planes (Tx, Ty) of I_0 (one-sided at the border), four-tap bilinear
 *             samples; where a tap is outside I_0, e = Tx = Ty = 0; e = Tw - I_k(q).  Window sums (a, b, c, p, q) of
 *             (Tx Tx, Tx Ty, Ty Ty, Tx e, Ty e), the window separable and triangular, weight 2 r + 1 - |d| per axis for
 *             |d| <= 2 r (r = window_radius), along x then along y, d ascending, pixels outside the image contributing 0.
 *             lambda = damping (a + c) / 2, a' = a + lambda, c' = c + lambda, det = a' c' - b b;
 *             du = -(c' p - b q, a' q - b p) / det where det > 0, else 0; each component clipped to +-1 px of the level;
 *             u <- the box mean of u + du over radius smooth_radius, divided by the number of in-image pixels of the box.
 *   output    flow_out [num_images][2][s h][s w] (x then y component, the K*2*H*W layout of srmap_problem_set_flow) with
 *             s = hr_scale: U_k(Q) = s * bilinear(u_k at Q / s), clamped -- LR pixel q is HR pixel s q, as in
 *             srmap_register_affine.
 * valid_out (optional, [num_images][h][w] doubles, input resolution): 1 where the four taps of I_0 at q + u_k(q) are inside
 * AND q is at least valid_margin pixels from every edge, else 0; image 0 is all 1.  The field is wrong by pixels in the few
 * border pixels whose content image 0 does not hold: pass the mask on as data weights (srmap_set_data_weights).
 * quality_out (optional, 3 doubles per image): [3i] root mean squared residual I_0(q + u) - I_k(q) over the valid pixels,
 * [3i+1] the valid fraction, [3i+2] the largest horizontal plus the largest vertical neighbour difference of the returned
 * field (what the sufficient condition of srmap_problem_set_flow reads).  Image 0: (0, 1, 0).
 * What this estimator is NOT: it is dense, LOCAL and unregularised beyond the window and the box mean, so it cannot resolve
 * motion finer than the window; it has NO occlusion handling; it registers ONE plane per image; and it is NOT fitted through
 * the blur and decimation of the forward model -- on aliased LR frames it plateaus near 0.2 HR px.  A flow leg of
 * srmap_refine_motion was prototyped (a windowed per-pixel Gauss-Newton through D B, and a bilinear control lattice of
 * 8...32 px fitted by Levenberg-Marquardt): both lower the data energy and both RAISE the endpoint error (0.210 ->
 * 0.24...0.50 HR px), because the fit follows the noise of x; neither beats the unrefined masked solve, so none is built.
 * num_images == 0 returns SRMAP_OK and writes nothing.  SRMAP_EINVAL: width or height < 16; a struct_size that is not this
 * library's; hr_scale < 1, warps < 1, window_radius outside 1...8, smooth_radius outside 0...8, a negative or non-finite
 * damping, a negative valid_margin or max_levels; an output grid beyond 2^30 pixels; an image that is not finite; an initial
 * matrix (rows 1...num_images-1; row 0 is ignored) that is not finite or outside the affine model's domain.  Results are
 * bit-identical run to run and do not depend on the other images of the stack. */
typedef struct {
  int struct_size;                   /* filled by the _default call; a mismatch is SRMAP_EINVAL */
  int hr_scale;                      /* 1 */
  int warps;                         /* 8, per level */
  int window_radius;                 /* 4 (1...8): the triangular window spans 2 r pixels to each side */
  double damping;                    /* 0.05 */
  int smooth_radius;                 /* 2 (0...8) */
  int valid_margin;                  /* 3 px */
  int max_levels;                    /* 0 = automatic; 1 = full resolution only */
  const double* initial_affine_2x3;  /* NULL = start from u = 0; else num_images x 6, input-pixel units */
} srmap_flow_registration_options;
void srmap_flow_registration_options_default(srmap_flow_registration_options* options);
int srmap_register_flow(srmap_ctx* ctx, int num_images, int width, int height, const double* images_host,
                        const srmap_flow_registration_options* options /* NULL = defaults */,
                        double* flow_out /* num_images x 2 x (s h) x (s w) */, double* valid_out /* optional */,
                        double* quality_out /* optional, 3 per image */);
/* The same registration of a stack that is already on the device: images_dev [num_images][h][w] doubles, read on
 * hip_stream (NULL = the context's stream); flow_dev_out / valid_dev_out (optional) are device buffers of the sizes above.
 * The same kernels in the same order: flow, valid and quality are bit-identical to srmap_register_flow on the same
 * doubles.  Nothing is uploaded and no field is copied back; image 0's planes are written on the device; the scan for
 * non-finite pixels is a device count that returns with the quality records (one stream wait per call; complete on
 * return).  A non-finite image answers SRMAP_EINVAL naming the first one; the output buffers are then unspecified. */
int srmap_register_flow_device(srmap_ctx* ctx, int num_images, int width, int height, const double* images_dev,
                               void* hip_stream, const srmap_flow_registration_options* options /* NULL = defaults */,
                               double* flow_dev_out, double* valid_dev_out /* optional */,
                               double* quality_out /* host, optional, 3 per image */);
/* Registration from the problem's own observations: the plane [K][h][w] is taken in double from the observation buffer the
 * evaluations read (the photometrically normalised one while parameters are set) -- channel >= 0 that channel, -1 the mean
 * over the channels (the sum in ascending channel order, one division by C, no fused operation; f32 observations convert
 * exactly) -- and registered as above at the problem's scale (options->hr_scale must be 1 or that scale).  The double field
 * is rounded once to the problem's dtype (as srmap_problem_set_flow rounds host doubles) and installed with the checks and
 * answers of srmap_problem_set_flow_device; quality [3i+2] is that of the double field.  install_prior != 0: the validity
 * masks, one plane per frame broadcast over the channels, become the data prior (srmap_set_data_prior), replacing any in
 * force.  When the field is refused (SRMAP_EUNSUPPORTED) the problem keeps the motion and the prior it had, and
 * quality_out is still written.  SRMAP_EINVAL: no observations; an LR side < 16; a bad channel; an HR size that is not
 * LR size * scale; the options' errors of srmap_register_flow.  Sharded problems are out of scope. */
int srmap_problem_register_flow(srmap_problem* p, int channel /* -1 = channel mean */,
                                const srmap_flow_registration_options* options /* NULL = defaults */, int install_prior,
                                double* quality_out /* optional, K x 3 */);
/* The same registration -- plane rule, options, prior and errors -- that stops at the input level: the nodes s u are
 * installed as a lattice with step = scale, lw = w, lh = h (srmap_problem_set_flow_lattice_device).  No HR resample, no
 * rounding pass and no HR-sized buffer; quality [3i+2] comes from the nodes, (largest node difference along x + along y) /
 * step, which equals the expanded field's figure to rounding.  At a scale that is a power of two the installed motion
 * evaluates bit for bit as srmap_problem_register_flow's. */
int srmap_problem_register_flow_lattice(srmap_problem* p, int channel /* -1 = channel mean */,
                                        const srmap_flow_registration_options* options /* NULL = defaults */, int install_prior,
                                        double* quality_out /* optional, K x 3 */);

/* Joint motion refinement (no reference counterpart; csrc/motion_refinement.hip; it closes what DESIGN.md
 * 3.7 left out: a registration that honours the forward model and the data weights).  With an HR estimate x, every frame
 * k >= 1 has its matrix re-fitted THROUGH the affine forward model of 3.6 (srmap_problem_set_affine_motion):
 *   energy    E_k(G) = sum_c sum_u w_k(c,u) r^2, r = (D B M(G) x)(c,u) - y_k(c,u), G = F_k^-1 (formed as
 *             srmap_problem_set_affine_motion forms it), over EVERY LR pixel of every channel: the rows of
 *             srmap_problem_set_cost_rows are ignored.  w: the problem's data weights as they stand (the caller's, or the
 *             last Huber weights -- a refinement after a Huber solve is an outlier-robust registration), 1 when none are set.
 *             Always the affine model, exact double coordinates, no 1/32-px quantisation, also for a problem created with
 *             shifts_xy.  All arithmetic after the loads is double in both dtypes.
 *   start     F_k from initial_affine_2x3; else the problem's affine motion; else [I | shifts_xy[k]]; else the identity.
 *   step      G <- G + dL (q - c0) + dt, c0 = ((W-1)/2, (H-1)/2), parameters (da, db, dtx, dc, dd, dty); the pass sums
 *             H = sum w J J^T (21 entries, upper triangle row-major), g = sum w J r (6) and E: 28 numbers per frame, J the
 *             exact derivative of the model (the derivative of the four-tap sample, from the sample's own four taps).
 *   LM        per frame, on the host: (H + lambda diag H) d = -g by the 6 x 6 Cholesky of srmap_register_affine (dof = 2:
 *             the 2 x 2 system of (dtx, dty), L stays bit-identical); E' < E accepts (lambda <- max(lambda / 10, 1e-9)) and
 *             stops with status 0 when the four HR image corners moved less than step_tolerance; otherwise lambda <- 10
 *             lambda, status 2 once lambda > 1e6.  A trial outside 3.6's domain or not finite is a rejection that spends no
 *             pass.  A failed Cholesky (no texture, or a frame whose weights are all 0) keeps the matrix: status 3.  The
 *             iteration cap: status 1 (also what max_iterations = 0 answers).  No status is an error of the call.
 * Frame 0 is the gauge: never changed, quality (cost, cost, 0, 0).
 * affine_2x3_out (optional, K x 6): the matrices F_k.  quality_out (optional, K x 4): E at the start, E at the result, passes
 * run, status.  normal_equations_out (optional, K x 28): the sums at the returned matrix.  apply = 1 installs the result as
 * srmap_problem_set_affine_motion(result) would (the problem then evaluates the affine model); apply = 0 leaves the problem
 * alone.  SRMAP_EINVAL: no observations set; a struct_size that is not this library's; dof not 2 or 6; negative
 * max_iterations, step_tolerance or initial_damping; a starting matrix that is not finite.  SRMAP_EUNSUPPORTED: a starting
 * matrix outside the domain.  Every error leaves the problem unchanged.  Results are bit-identical run to run and a frame's
 * answer does not depend on the other frames.  Sharded problems are out of scope.  Not thread-safe against evaluations of the
 * same problem, as srmap_problem_set_affine_motion.  The _device form takes x in the problem's dtype and enqueues on
 * hip_stream (NULL = the context's stream); both forms are complete when they return. */
typedef struct {
  int struct_size;          /* filled by the _default call; a mismatch is SRMAP_EINVAL */
  int dof;                  /* 6 = full 2 x 3 (default); 2 = translation only (tx, ty) */
  int max_iterations;       /* 30: trial passes per frame after the initial pass; 0 = evaluate only */
  double step_tolerance;    /* 1e-4 HR px */
  double initial_damping;   /* 1e-3; >= 0 */
  int apply;                /* 1 */
  const double* initial_affine_2x3; /* NULL = the problem's current motion; else K x 6 */
} srmap_motion_refinement_options;
void srmap_motion_refinement_options_default(srmap_motion_refinement_options* options);
int srmap_refine_motion(srmap_problem* p, const double* x_host, const srmap_motion_refinement_options* options /* NULL = defaults */,
                        double* affine_2x3_out, double* quality_out, double* normal_equations_out);
int srmap_refine_motion_device(srmap_problem* p, const void* x_dev, void* hip_stream,
                               const srmap_motion_refinement_options* options /* NULL = defaults */,
                               double* affine_2x3_out, double* quality_out, double* normal_equations_out);

/* Calibration fit of the blur kernel (no reference counterpart: blur_module.cpp takes (radius, sigma) and nothing is
 * estimated; csrc/blur_fit.hip).  With a KNOWN HR image x (a chart, a calibration pair) the ksize x ksize taps
 * h of B are the minimiser of the quadratic
 *   energy    E(h) = sum_k sum_c sum_u w (sum_t h_t s_t - y)^2, s_t = (M_k x)(R0 + a - hb, C0 + e - hb) the warped image at
 *             tap t = (a, e) of LR pixel u (0 outside the image), (R0, C0) the decimation source of u, M_k sampled exactly as
 *             the forward kernel of the problem's motion samples it (the 1/32-px table of shifts_xy, double coordinates for
 *             an affine motion, the identity without motion), over EVERY LR pixel of every channel and frame: the rows of
 *             srmap_problem_set_cost_rows are ignored.  w: the problem's data weights as they stand, 1 when none are set.
 *             The sums are double in both dtypes.
 *   solve     one pass, one solve: (G + mu I) h = b + mu h_current by Cholesky on the host, G = sum w s s^T, b = sum w s y,
 *             mu = ridge trace(G) / ksize^2, h_current the kernel in force zero-padded or centre-cropped to ksize;
 *             sum_to_one adds the constraint sum h = 1 (its KKT system).  A failed factorisation (no texture, every
 *             weight 0) keeps the kernel: status 3, not an error of the call.
 * taps_out (optional, ksize^2): the fitted taps (the kernel in force, padded / cropped, for status 3).  quality_out
 * (optional, 5): E at the kernel in force, E at the fit, smallest and largest pivot of the factorisation, status (0 or 3).
 * normal_equations_out (optional, (n + 1)(n + 2) / 2 with n = ksize^2): the upper triangle, row-major, of the Gram of
 * [s_0 ... s_{n-1}, y] under w.  apply = 1 installs the fit as srmap_problem_set_blur_kernel(p, ksize, taps) would.
 * SRMAP_EINVAL: no observations set; a struct_size that is not this library's; an even ksize or ksize < 0; a negative or
 * non-finite ridge.  SRMAP_EUNSUPPORTED: ksize > 7.  Every error leaves the problem unchanged.  Results are bit-identical
 * run to run.  Sharded problems are out of scope.  Blind estimation (x unknown) is NOT offered: alternating a solve and this
 * fit drifts.  The _device form takes x in the problem's dtype and enqueues on hip_stream (NULL = the
 * context's stream); both forms are complete when they return. */
typedef struct {
  int struct_size;  /* filled by the _default call; a mismatch is SRMAP_EINVAL */
  int ksize;        /* 0 = the size of the kernel in force (default) */
  int sum_to_one;   /* 1 */
  double ridge;     /* 0 */
  int apply;        /* 1 */
} srmap_blur_fit_options;
void srmap_blur_fit_options_default(srmap_blur_fit_options* options);
int srmap_fit_blur(srmap_problem* p, const double* x_host, const srmap_blur_fit_options* options /* NULL = defaults */,
                   double* taps_out, double* quality_out, double* normal_equations_out);
int srmap_fit_blur_device(srmap_problem* p, const void* x_dev, void* hip_stream,
                          const srmap_blur_fit_options* options /* NULL = defaults */, double* taps_out, double* quality_out,
                          double* normal_equations_out);

/* Calibration fit of a blur-kernel bank (csrc/blur_fit.hip): srmap_fit_blur's quadratic, solved separately
 * over the observations of each entry of `mode` (srmap_blur_bank_mode) -- frame k's for PER_FRAME, channel c's of every
 * frame for PER_CHANNEL, those of (k, c) for PER_FRAME_CHANNEL.  One launch forms a Gram record per (frame, channel, chunk),
 * a reduce kernel adds the records of each entry in index order (frame, channel, chunk); double sums, a fixed order, no
 * atomics: bit-identical run to run.  The host solves entry by entry with srmap_fit_blur's Cholesky / KKT code.
 *   ridge     pulls entry e towards the kernel in force for it, zero-padded or centre-cropped to ksize: the bank's entry of
 *             (k, c) -- with (k, 0), (0, c), (k, c) standing for entry k, c, (k, c) of `mode` -- or the single / created
 *             kernel when no bank is set.  options->ksize = 0: the size of the blur in force.
 *   status    per entry: 0 fitted, 3 degenerate (no texture, every weight of the entry 0: a frame masked out).  A
 *             degenerate entry keeps the kernel in force for it and is not an error of the call.
 * taps_out (optional, entries x ksize^2), quality_out (optional, entries x 5, srmap_fit_blur's layout per entry),
 * normal_equations_out (optional, entries x (n + 1)(n + 2) / 2, srmap_fit_blur's layout per entry).  apply = 1 installs the
 * result as srmap_problem_set_blur_bank(p, mode, ksize, taps_out) would, unless every entry is degenerate.  The errors are
 * srmap_fit_blur's, and an unknown mode is SRMAP_EINVAL; every error leaves the problem unchanged.  Like srmap_fit_blur
 * this is a CALIBRATION fit from a known HR image: blind alternation of a solve and this fit is NOT offered (it drifts,
 * DESIGN.md 3.9).  A displacement field answers SRMAP_EUNSUPPORTED, as for srmap_fit_blur. */
int srmap_fit_blur_bank(srmap_problem* p, const double* x_host, int mode, const srmap_blur_fit_options* options /* NULL = defaults */,
                        double* taps_out, double* quality_out, double* normal_equations_out);
int srmap_fit_blur_bank_device(srmap_problem* p, const void* x_dev, void* hip_stream, int mode,
                               const srmap_blur_fit_options* options /* NULL = defaults */, double* taps_out,
                               double* quality_out, double* normal_equations_out);

/* Photometric frame model: per-frame gain and bias (no reference counterpart: image_model.cpp:86-91 gives every frame the
 * photometry of the HR image; csrc/photometric_fit.hip).  Frame k is modelled as
 *   y_k = a_k (D B M_k x) + b_k + noise,
 * and while parameters are set the problem solves against the NORMALISED frames yn_k = (y_k - b_k) / a_k: the data cost is
 * s^2 sum_k sum w (A_k x - yn_k)^2, today's formula with yn in place of y.
 *   units     the cost is measured in the normalised units.  It is NOT the maximum-likelihood weighting of the model
 *             above, which would carry a factor a_k^2 per frame.  huber_delta and the Huber weights therefore act on
 *             normalised residuals.
 *   storage   the raw frames are kept; yn lives in a second [K][C][h][w] buffer that exists only while parameters are set.
 *             Per element, in double on the stored value: the subtraction, then a true division, then one rounding to the
 *             problem's dtype (no reciprocal, no contraction).  NULL switches back to the raw buffer bit for bit.
 *   scope     one (gain, bias) pair per frame, shared by all channels; gain_bias is K x 2 = {a_k, b_k}.  Only the
 *             observation buffer changes, so every path that reads observations honours the parameters: both kernel
 *             families, the sub-pixel path, an affine motion, a free-form blur, data weights and the Huber loss, CG /
 *             L-BFGS / split_channels, the traces, cost rows, sharded evaluations and solves (each rank normalises its own
 *             frames), srmap_refine_motion and srmap_fit_blur (which then see yn).  srmap_problem_active_impl is unchanged.
 *   persists  across srmap_set_observations* (the new frames are normalised), the data-weight calls,
 *             srmap_problem_set_affine_motion and srmap_problem_set_blur_kernel.
 * A number that is not finite, or a gain <= 0: SRMAP_EINVAL, and nothing changes.  Not thread-safe against evaluations of
 * the same problem; evaluations already enqueued are waited for. */
int srmap_problem_set_photometric(srmap_problem* p, const double* gain_bias /* K x 2; NULL restores */);
/* The parameters in force: gain_bias_out (optional, K x 2; {1, 0} per frame when none are set), *is_set (optional). */
int srmap_problem_get_photometric(const srmap_problem* p, double* gain_bias_out /* K x 2 */, int* is_set);

/* Fit of the photometric parameters to an HR image x (no reference counterpart; csrc/photometric_fit.hip):
 * per frame the minimiser of
 *   energy    E_k(a, b) = sum_c sum_u w (a s + b - y_raw)^2, s = (D B M_k x)(c, u), M_k sampled exactly as the forward
 *             kernel of the problem's motion samples it (the 1/32-px table of shifts_xy, double coordinates for an affine
 *             motion, the identity without motion), B the blur in force (Gaussian or free-form), over EVERY LR pixel of
 *             every channel: the rows of srmap_problem_set_cost_rows are ignored.  y_raw: the frames as given, whatever
 *             parameters are in force -- the result is absolute, not an increment, and fitting twice at the same x gives
 *             the same answer.  w: the problem's data weights as they stand (1 when none are set), so a fit after a Huber
 *             solve is outlier-robust.
 *   sums      one kernel launch over all frames: sum w, sum w s, sum w y, sum w s^2, sum w s y, sum w y^2 per frame, double
 *             in both dtypes, no atomics; bit-identical run to run, and a frame's sums do not depend on the other frames.
 *   solve     on the host: model 0 the 2 x 2 system in (a, b); model 1 the gain alone with the bias in force held; model 2
 *             the bias alone with the gain in force held.
 *   status    per frame, none of them an error of the call: 0 fitted; 2 the fitted gain is outside [min_gain, max_gain],
 *             the parameters in force are kept; 3 degenerate -- sum w = 0, or a determinant <= 1e-12 sum w sum w s^2 (a flat
 *             frame) -- the parameters in force are kept.  The gauge frame keeps its parameters with status 0.
 * gain_bias_out (optional, K x 2): the result.  quality_out (optional, K x 4): E at the parameters in force, E at the
 * result (both from the six sums), sum w, status.  sums_out (optional, K x 6): the sums in the order above.  apply = 1
 * installs the result as srmap_problem_set_photometric would.  SRMAP_EINVAL: no observations set; a struct_size that is not
 * this library's; a model outside 0..2; a gauge_frame outside -1..K-1; gain bounds that are not finite with
 * 0 < min_gain <= max_gain.  Every error leaves the problem unchanged.  A problem sharded over more than one rank is out of
 * scope (a rank would fit its own frames alone).  The _device form takes x in the problem's dtype and enqueues on hip_stream
 * (NULL = the context's stream); both forms are complete when they return. */
typedef struct {
  int struct_size;  /* filled by the _default call; a mismatch is SRMAP_EINVAL */
  int model;        /* 0 gain and bias (default), 1 gain only, 2 bias only */
  int gauge_frame;  /* 0 (default): this frame keeps its parameters; -1: none */
  double min_gain;  /* 0.25 */
  double max_gain;  /* 4 */
  int apply;        /* 1 */
} srmap_photometric_fit_options;
void srmap_photometric_fit_options_default(srmap_photometric_fit_options* options);
int srmap_fit_photometric(srmap_problem* p, const double* x_host, const srmap_photometric_fit_options* options /* NULL = defaults */,
                          double* gain_bias_out, double* quality_out /* K x 4 */, double* sums_out /* K x 6 */);
int srmap_fit_photometric_device(srmap_problem* p, const void* x_dev, void* hip_stream,
                                 const srmap_photometric_fit_options* options /* NULL = defaults */, double* gain_bias_out,
                                 double* quality_out /* K x 4 */, double* sums_out /* K x 6 */);

/* ------------------------------------------------------------- solver */
/* IRLSMapSolverOptions (irls_map_solver.h:14-36) + MapSolverOptions
 * (map_solver.h:28-79); srmap_irls_options_default() fills the reference
 * defaults.  Analytic differentiation only: numeric differentiation is a
 * test-only alternative in the reference and is out of scope.  The inner
 * minimiser (CG or L-BFGS) is chosen on the problem: srmap_problem_set_solver. */
typedef struct {
  int struct_size;                       /* sizeof(srmap_irls_options) of the header the caller was built with: filled by
                                            srmap_irls_options_default(); srmap_solve answers SRMAP_EINVAL when it is
                                            not this library's (a caller built against another version of this header
                                            would otherwise have its fields read at the wrong offsets) */
  int max_num_solver_iterations;         /* 50 */
  double gradient_norm_threshold;        /* 1e-6 */
  double cost_decrease_threshold;        /* 1e-6 */
  double parameter_variation_threshold;  /* 1e-6 */
  int split_channels;                    /* 0 */
  int max_num_irls_iterations;           /* 20 */
  double irls_cost_difference_threshold; /* 1e-5 */
  int host_paced_passes;                 /* 0.  No reference counterpart: 1 = every CG pass waits for the host's
                                            answer before the next is queued (the order up to round 3) instead of
                                            chaining the passes whose inputs are already on the device, and every
                                            trial point of the line search is formed by its own n-vector pass
                                            instead of inside the evaluation.  Same arithmetic, same result bit
                                            for bit: a debugging / measurement switch. */
} srmap_irls_options;
void srmap_irls_options_default(srmap_irls_options* o);

typedef struct {
  int irls_rounds;
  int cg_iterations;      /* inner iterations of whichever minimiser ran (CG or L-BFGS, srmap_problem_set_solver) */
  int evaluations;       /* cost+gradient evaluations ("MAP gradient iterations") */
  int last_termination;  /* ALGLIB-style code of the last inner run (mincg / minlbfgs termination type) */
  double final_cost;
  double loop_seconds;   /* wall time of the IRLS / CG loop itself (device-resident part: no allocation,
                            no upload / download of x) */
  double wait_seconds;   /* part of loop_seconds the host spent waiting for device scalars */
  int waits;             /* number of such waits (2 + nfev per CG iteration) */
} srmap_solve_report;

/* IRLSMapSolver::Solve(initial_estimate) irls_map_solver.cpp:192-265:
 * x0 / x_out are [C][H][W] host doubles.  The iterate, gradient and CG vectors
 * stay on the GPU; only scalars cross PCIe per evaluation.  Passes whose inputs are
 * already on the device are queued without waiting for the host (un-sharded solves;
 * options->host_paced_passes = 1 restores the host-paced order).  The library reads no
 * environment variable. */
int srmap_solve(srmap_problem* p, const srmap_irls_options* options,
                const double* x0, double* x_out, srmap_solve_report* report);

/* The regularisation weight by hold-out validation (no reference counterpart): one solve per multiplier
 * of the problem's lambdas, each scored on the held-out observations, and the best kept.  Needs a hold-out
 * (srmap_problem_set_holdout), at least one regulariser with lambda > 0 and observations: SRMAP_EINVAL otherwise, the
 * message naming the missing call.  scales[0 .. num_scales): finite, > 0, strictly decreasing multipliers applied to the
 * lambda of EVERY regulariser as it stands at the call.  Row j: the lambdas are set (srmap_problem_set_regularizer_lambda),
 * srmap_solve's loop runs from x0 -- always from x0: warm starts cost more evaluations than they save --, and the
 * solution is scored (srmap_holdout_score) with the path's delta: 0 under L2; the problem's under HUBER / FIXED; under
 * HUBER / MAD the delta of the last Huber step of row 0, held for every row so that the rows are comparable.  Row j is bit
 * for bit what the caller gets from those three calls.  patience: 0 runs every row; n > 0 stops after the score rose n
 * rows in a row.  *chosen: the FIRST minimum of the score, so a tie goes to the larger lambda.  final_solve != 0: the
 * hold-out is lifted, the chosen lambdas are set and one more solve from x0 on ALL observations gives x_out (bit for bit
 * srmap_problem_set_holdout(0), srmap_solve), then the hold-out is set again; final_solve == 0: x_out is the chosen row's
 * solution.  On return the chosen lambdas stay set and the hold-out is as it was; on an error the lambdas of the call's
 * start are restored.  x0 is staged once; the iterates and the best solution so far stay on the device.
 * table: num_scales rows of SRMAP_LAMBDA_PATH_ROW doubles, *rows_run of them written:
 *   {scale, score, S1, S2, S0, n, IRLS rounds, inner iterations, evaluations, final cost, delta used}.
 * final_report (optional): the final solve's report, or the chosen row's without one. */
#define SRMAP_LAMBDA_PATH_MAX_SCALES 32
#define SRMAP_LAMBDA_PATH_ROW 11
typedef struct {
  int struct_size;   /* filled by srmap_lambda_path_options_default(); another size is refused */
  int num_scales;    /* 8 */
  double scales[SRMAP_LAMBDA_PATH_MAX_SCALES]; /* 1, 1/2, ..., 1/128 */
  int patience;      /* 0 */
  int final_solve;   /* 1 */
} srmap_lambda_path_options;
void srmap_lambda_path_options_default(srmap_lambda_path_options* options);
int srmap_solve_lambda_path(srmap_problem* p, const srmap_irls_options* irls_options /* NULL = defaults */,
                            const srmap_lambda_path_options* path_options /* NULL = defaults */, const double* x0, double* x_out,
                            double* table, int* rows_run, int* chosen, srmap_solve_report* final_report);

/* The cross-validated path: srmap_solve_lambda_path over the `folds` folds of a partition of the
 * observations, and the one-standard-error rule.  Needs at least one regulariser with lambda > 0 and observations, and NO
 * hold-out beforehand: whatever hold-out is set at the call -- none, a fraction or a fold -- is in force again on return,
 * on success and on an error.  scales: as above.  Rows are the outer loop, folds the inner one; row j, fold f is bit for bit
 *     srmap_problem_set_regularizer_lambda for every regulariser,  srmap_problem_set_holdout_fold(folds, f, seed),
 *     srmap_solve from x0,  srmap_holdout_score
 * with the path's delta as above (under HUBER / MAD the delta of row 0, fold 0, held for every row and fold).  A fold whose
 * score call fails -- no held-out observation with a base weight above 0, say -- fails the path.  With s[j][f] that
 * fold's score[0] (its S1 / S0 over all frames):
 *     mean[j] = (sum_f s[j][f]) / folds                                   (added in fold order)
 *     se[j]   = sqrt(sum_f (s[j][f] - mean[j])^2 / (folds - 1) / folds)   (the standard error of that mean)
 *     j*      = the FIRST minimum of mean, so a tie goes to the larger lambda
 * SRMAP_LAMBDA_RULE_MIN chooses j*.  SRMAP_LAMBDA_RULE_ONE_SE chooses the smallest j -- the largest lambda among the rows
 * run -- with mean[j] <= mean[j*] + se_factor * se[j*] (se_factor finite, >= 0; 0 is MIN but for exact ties): the score
 * under-counts the high-frequency error of too little regularisation because A blurs, so among rows the folds cannot tell
 * apart the larger lambda is the better one.  A row with a fold score that is not a number is neither j* nor eligible.
 * patience reads mean.  The standard error is the spread OVER THE FOLDS, not the per-pixel one that S2 and n give: under
 * outliers the per-pixel error is dominated by the corrupted held-out pixels (several times the fold error) and a rule
 * built on it picks the largest lambda of any grid.  That is why srmap_solve_lambda_path, which has one split, has no
 * one-standard-error rule.
 * final_solve != 0: the hold-out is lifted and one solve from x0 at the chosen lambdas on ALL observations gives x_out and
 * *final_report; final_solve == 0: neither is written (a row has one solution per fold, none of them the row's), and x_out
 * may be NULL.  The chosen lambdas stay set; on an error the lambdas of the call's start are restored.  x0 is staged once;
 * the iterates stay on the device.
 * table: num_scales rows of SRMAP_LAMBDA_PATH_ROW doubles, *rows_run of them written:
 *   {scale, mean, se, pooled S1, S2, S0, n (each added in fold order), sum of IRLS rounds, of inner iterations, of
 *    evaluations over the folds, delta used}.
 * fold_table (optional): num_scales x folds rows, [scale][fold], each in srmap_solve_lambda_path's layout. */
#define SRMAP_LAMBDA_RULE_MIN 0
#define SRMAP_LAMBDA_RULE_ONE_SE 1
typedef struct {
  int struct_size;   /* filled by srmap_lambda_cv_options_default(); another size is refused */
  int num_scales;    /* 8 */
  double scales[SRMAP_LAMBDA_PATH_MAX_SCALES]; /* 1, 1/2, ..., 1/128 */
  int folds;         /* 5; 2...32 */
  int rule;          /* SRMAP_LAMBDA_RULE_ONE_SE */
  unsigned long long seed; /* 1 */
  double se_factor;  /* 1.0 */
  int patience;      /* 0 */
  int final_solve;   /* 1 */
} srmap_lambda_cv_options;
void srmap_lambda_cv_options_default(srmap_lambda_cv_options* options);
int srmap_solve_lambda_path_folds(srmap_problem* p, const srmap_irls_options* irls_options /* NULL = defaults */,
                                  const srmap_lambda_cv_options* cv_options /* NULL = defaults */, const double* x0,
                                  double* x_out, double* table, double* fold_table /* optional */, int* rows_run, int* chosen,
                                  srmap_solve_report* final_report /* optional */);

/* Self-check of the solver's derived sums (no reference counterpart).  mincg forms the DY / HS betas with the
 * denominator y.dk summed over the vectors (optimization.cpp:17700-17760); this solver derives it from sums it already
 * holds, y.dk = (g.d) / (s1 s2) - g_prev.dk.  With srmap_irls_options::host_paced_passes = 1 the beta pass ALSO sums y.dk
 * directly; *beta_denominator_rel_dev receives the largest relative deviation |derived - direct| / |direct| seen by the
 * host-paced solves of this problem so far (0 if none ran).  Expected: reduction-order level (<= 1e-12 f64, <= 1e-6 f32). */
int srmap_problem_selfcheck(const srmap_problem* p, double* beta_denominator_rel_dev);

/* ------------------------------------------------- multi-GPU (one rank per GPU) */
/* The reference is single-process.  Its objective shards three ways (SURVEY.md
 * section 8e); a communicator carries the exchanges the sharded evaluation and the
 * sharded solve need, INSIDE the library, on the evaluation's HIP stream:
 *   - RCCL over xGMI (the production backend, ncclAllReduce / ncclSend / ncclRecv),
 *   - or caller-supplied host callbacks (MPI / gloo harnesses and the one-GPU
 *     tests: the library stages device buffers through pinned host memory). */
typedef struct srmap_comm srmap_comm;
#define SRMAP_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to every rank. */
int srmap_comm_get_unique_id(srmap_ctx* ctx, char* id128);
/* ncclCommInitRank on this context's device. */
int srmap_comm_create_rccl(srmap_ctx* ctx, const char* id128, int rank, int world,
                           srmap_comm** out);
/* op: 0 = sum, 1 = max.  dtype: srmap_dtype of the elements.  In place, all ranks. */
typedef int (*srmap_host_allreduce_fn)(void* buf, size_t count, int dtype, int op, void* user);
/* Send `send_bytes` to rank dst (skip if dst < 0) and receive `recv_bytes` from rank
 * src (skip if src < 0); must not deadlock when every rank calls it at once. */
typedef int (*srmap_host_sendrecv_fn)(const void* send, size_t send_bytes, int dst,
                                      void* recv, size_t recv_bytes, int src, void* user);
int srmap_comm_create_host(srmap_ctx* ctx, int rank, int world,
                           srmap_host_allreduce_fn allreduce,
                           srmap_host_sendrecv_fn sendrecv, void* user, srmap_comm** out);
void srmap_comm_destroy(srmap_comm* comm);
/* What the communicator itself reports: rank, size (ncclCommCount for RCCL), backend (1 = RCCL, 0 = host
 * callbacks).  Any out pointer may be NULL.  No reference counterpart (the reference is single-process). */
int srmap_comm_info(srmap_comm* comm, int* rank, int* world, int* backend);
/* Row shards: post the halo exchange of x on the communicator's side stream UNDER the tile rows that read no halo row
 * (on != 0), or exchange first and evaluate afterwards (on == 0).  Default: on for the host-callback backend (whose
 * callbacks block anyway), off for RCCL -- the overlapped form uses one ncclComm_t from two streams and is opt-in until
 * it has been validated on the deployment's RCCL.  No reference counterpart. */
int srmap_comm_set_overlap(srmap_comm* comm, int on);
/* Which collective library the communicator runs on, as text: "rccl <ncclGetVersion> <path of the loaded librccl>" or
 * "host callbacks" (a process may carry several librccl copies: PyTorch ships its own).  No reference counterpart. */
int srmap_comm_describe(srmap_comm* comm, char* buf, size_t cap);
/* ncclCommSplit: ranks passing the same color form a new communicator ordered by key; the caller states its rank
 * and size in it (RCCL backend; host-callback harnesses build the sub-communicator themselves).  Collective. */
int srmap_comm_split(srmap_comm* comm, int color, int key, int new_rank, int new_world, srmap_comm** out);
/* In-place all-reduce of a device buffer (op 0 = sum, 1 = max) on `hip_stream`: what the sharded evaluation
 * and solver use internally, exposed for harnesses. */
int srmap_comm_allreduce(srmap_comm* comm, void* dev_buf, size_t count, int dtype, int op,
                         void* hip_stream);

typedef enum {
  SRMAP_SHARD_NONE = 0,
  SRMAP_SHARD_FRAMES = 1,   /* rank owns a frame subset + a replica of x: all-reduce of the
                               gradient (C*N elements) and of the cost (one group) after every
                               evaluation (objective_data_term.cpp:98-116 summed over ranks).
                               The regulariser is split over the ranks by HR row band (whole
                               tile rows) when the tile kernels produce it in their one pass;
                               otherwise (3-D TV, a second regulariser, direct kernels) rank
                               reg_rank evaluates it */
  SRMAP_SHARD_ROWS = 2,     /* rank owns a band of HR rows; its problem is the band + halo
                               rows; halo rows of x are exchanged with the two neighbours
                               before every evaluation, scalars all-reduced */
  SRMAP_SHARD_CHANNELS = 3, /* rank owns a channel block (+ one halo channel plane per
                               neighbour when a 3-D TV regulariser couples them,
                               tv_regularizer.cpp:205-222); scalars all-reduced */
  SRMAP_SHARD_GRID = 4      /* frames x channels (BASELINE configs[4]): world rank =
                               channel_block * frame_groups + frame_group.  The rank owns a
                               channel block (as CHANNELS) and a frame subset (as FRAMES) of
                               it: the gradient of the block is all-reduced over the
                               frame_groups ranks that share the block (frame_comm), halo
                               planes travel between ranks rank +- frame_groups, the
                               regulariser terms are evaluated by frame group 0, scalars
                               are all-reduced over the world communicator */
} srmap_shard_mode;

typedef struct {
  int mode;                        /* srmap_shard_mode */
  int own_row0, own_row1;          /* ROWS: HR rows of THIS problem the rank owns (the rest is halo) */
  int send_up_rows, send_down_rows;/* ROWS: owned boundary rows the upper / lower neighbour's halo holds */
  int own_ch0, own_ch1;            /* CHANNELS: channels of THIS problem the rank owns (others: halo planes) */
  int reg_rank;                    /* FRAMES: the rank whose evaluation carries the regulariser terms when they
                                      cannot be split by row band (see SRMAP_SHARD_FRAMES) */
  int frame_groups;                /* GRID: ranks per channel block (0 / 1 elsewhere) */
  srmap_comm* frame_comm;          /* GRID: communicator of the frame_groups ranks sharing this rank's channel
                                      block (srmap_comm_split, or a host communicator of that group) */
} srmap_shard_desc;

/* One ObjectiveFunction::ComputeAllTerms of the JOINT objective on device buffers of
 * this rank's shard: halo exchange (ROWS / CHANNELS), the local evaluation, the
 * gradient all-reduce (FRAMES) and -- when cost != NULL -- the all-reduced cost.
 * comm == NULL or mode NONE: plain srmap_eval_device. */
int srmap_eval_sharded_device(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard,
                              unsigned terms, void* x_dev, void* g_dev, double* cost,
                              void* hip_stream);
/* IRLSMapSolver::Solve of the joint problem with the unknowns sharded as described:
 * every rank calls it with its shard of x0 and receives its shard of the result (halo
 * rows / planes of x_out are valid copies of the neighbours' values).  The CG scalars
 * (dot products, max-norm) are reduced over owned elements only and all-reduced, so
 * every rank follows the trajectory of the single-GPU solve up to reduction order. */
int srmap_solve_sharded(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard,
                        const srmap_irls_options* options, const double* x0, double* x_out,
                        srmap_solve_report* report);

/* One run of the nonlinear CG (alglib_objective.cpp:47-75 / mincg, no IRLS re-weighting) on
 * the problem's current objective, with the cost of EVERY evaluation recorded in order
 * (f_trace[0 .. min(*trace_len, trace_cap))): the trajectory the parity tests compare with
 * ALGLIB's.  epsg / epsf / epsx / maxits are mincgsetcond's arguments. */
int srmap_cg_trace(srmap_problem* p, double epsg, double epsf, double epsx, int maxits,
                   const double* x0, double* x_out, int* iterations, int* nfev,
                   int* termination, double* f_trace, int trace_cap, int* trace_len);

/* srmap_cg_trace's twin for L-BFGS: one minlbfgs run (optimization.cpp:21640 ff.; driven as
 * alglib_objective.cpp:111-140 drives it, m = num_lbfgs_hessian_corrections, map_solver.h:51) on the problem's current
 * objective, with the cost of every evaluation recorded in order.  m outside 1..8 as srmap_problem_set_solver. */
int srmap_lbfgs_trace(srmap_problem* p, int m, double epsg, double epsf, double epsx, int maxits,
                      const double* x0, double* x_out, int* iterations, int* nfev,
                      int* termination, double* f_trace, int trace_cap, int* trace_len);

#ifdef __cplusplus
}
#endif
#endif  /* SRMAP_H_ */
