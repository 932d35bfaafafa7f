// problem.hip -- problem set-up (what the reference's ImageModel / MapSolver constructors do on the host) and the
// setters of the model: motion, blur, solver, implementation, cost rows, regularisers.
#include <algorithm>
#include <cmath>
#include <new>

#include "affine_map.hpp"
#include "model_tables.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

int model_drain(srmap_problem* p) {
  if (p->use_stream) SRMAP_HIP(p->ctx, hipStreamSynchronize(p->use_stream));
  SRMAP_HIP(p->ctx, hipStreamSynchronize(p->ctx->stream));
  return SRMAP_OK;
}

void model_replan(srmap_problem* p) {
  p->plan_gen++;
  if (ztile_plan(p)) ztile_preload(p);
}

// srmap_problem_set_affine_motion (below) and the motion refinement: validate K 2x3 matrices and fill the per-frame
// records (inverse in double, formed once here).
int affine_records(srmap_ctx* ctx, int K, const double* a23, std::vector<double>* recs) {
  for (int i = 0; i < 6 * K; ++i)
    if (!std::isfinite(a23[i]))
      return set_error(ctx, SRMAP_EINVAL, "affine motion: entry %d of frame %d is not finite", i % 6, i / 6);
  recs->assign((size_t)K * kAffineRec, 0.0);
  for (int k = 0; k < K; ++k) {
    AffineMap F;
    std::copy(a23 + 6 * k, a23 + 6 * (k + 1), F.m);
    const double a = F.m[0], b = F.m[1], tx = F.m[2], c = F.m[3], d = F.m[4], ty = F.m[5];
    const double dev = deviation(F);
    if (!(dev <= kAffineMaxDeviation))
      return set_error(ctx, SRMAP_EUNSUPPORTED,
                       "affine motion of frame %d: max(|a-1|+|b|, |c|+|d-1|) = %g exceeds %g (the transpose gathers 3 x 3 candidates)",
                       k, dev, kAffineMaxDeviation);
    if (!(std::fabs(tx) < 1.0e9) || !(std::fabs(ty) < 1.0e9))
      return set_error(ctx, SRMAP_EUNSUPPORTED, "affine motion of frame %d: translation (%g, %g) too large", k, tx, ty);
    double* m = recs->data() + (size_t)k * kAffineRec;
    const AffineMap G = inverse(F);
    std::copy(G.m, G.m + 6, m);
    std::copy(F.m, F.m + 6, m + 6);
    // candidate radii, widened so that rounding of F(p) can drop no candidate (2 * (1.25 + 1e-9) < 3: still three integers)
    m[12] = std::fabs(a) + std::fabs(b) + 1.0e-9;
    m[13] = std::fabs(c) + std::fabs(d) + 1.0e-9;
  }
  return SRMAP_OK;
}

}  // namespace srmap

extern "C" {

int srmap_problem_create(srmap_ctx* ctx, const srmap_problem_desc* d, srmap_problem** out) {
  if (!ctx || !d || !out) return SRMAP_EINVAL;
  *out = nullptr;
  if (d->hr_width <= 0 || d->hr_height <= 0 || d->channels <= 0)
    return set_error(ctx, SRMAP_EINVAL, "image size and channel count must be positive");
  if (d->scale < 1) return set_error(ctx, SRMAP_EINVAL, "downsampling scale must be >= 1");  // image_model.cpp:66
  if (d->frames < 1) return set_error(ctx, SRMAP_EINVAL, "at least one frame is required");
  if (d->dtype != SRMAP_F64 && d->dtype != SRMAP_F32) return set_error(ctx, SRMAP_EINVAL, "bad dtype");
  if (d->hr_width > 32000 || d->hr_height > 32000)
    return set_error(ctx, SRMAP_EUNSUPPORTED, "image larger than warpAffine's 16-bit coordinates");
  const bool blur = d->blur_ksize > 0 && d->blur_sigma > 0.0;  // image_model.cpp:42
  if (blur && (d->blur_ksize % 2 != 1))
    return set_error(ctx, SRMAP_EINVAL, "blur radius must be an odd number");  // blur_module.cpp:18
  if (blur && d->blur_ksize * d->blur_ksize > kMaxBlurTaps)
    return set_error(ctx, SRMAP_EUNSUPPORTED, "blur kernel larger than %d taps", kMaxBlurTaps);
  if ((size_t)d->channels * d->hr_width * d->hr_height > (size_t)2147483647)
    return set_error(ctx, SRMAP_EINVAL, "number of data points exceeds INT_MAX");  // map_solver.cpp:96-101
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));

  srmap_problem* p = new (std::nothrow) srmap_problem();
  if (!p) return SRMAP_ENOMEM;
  p->ctx = ctx;
  p->dtype = d->dtype;
  Geometry& g = p->geo;
  g.W = d->hr_width; g.H = d->hr_height; g.C = d->channels; g.K = d->frames; g.s = d->scale;
  const double scale_factor = 1.0 / (double)g.s;  // downsampling_module.cpp:24
  g.w = (int)(g.W * scale_factor);
  g.h = (int)(g.H * scale_factor);
  if (g.w <= 0 || g.h <= 0) { delete p; return set_error(ctx, SRMAP_EINVAL, "image smaller than the scale"); }
  g.cr0 = 0; g.cr1 = g.H;
  g.rr0 = 0; g.rr1 = g.H;
  g.zlo = 0; g.zhi = 0;
  std::vector<int> cmap, rmap;
  nearest_map(g.W, g.w, &cmap);
  nearest_map(g.H, g.h, &rmap);
  p->maps_regular = maps_regular(g.W, g.H, g.w, g.h, g.s, cmap, rmap);
  auto fail = [&](int code) { srmap_problem_destroy(p); return code; };
  if (int rc = p->motion.create(p, d->shifts_xy)) return fail(rc);
  if (int rc = p->blur.create(p, blur ? d->blur_ksize : 0, d->blur_sigma)) return fail(rc);
  if (p->d_col_map.alloc(sizeof(int) * g.w) != hipSuccess || p->d_row_map.alloc(sizeof(int) * g.h) != hipSuccess ||
      p->d_cost.alloc(sizeof(double) * kCostSlots) != hipSuccess)
    return fail(set_error(ctx, SRMAP_ENOMEM, "hipMalloc failed"));
  (void)hipMemcpy(p->d_col_map.as<int>(), cmap.data(), sizeof(int) * g.w, hipMemcpyHostToDevice);
  (void)hipMemcpy(p->d_row_map.as<int>(), rmap.data(), sizeof(int) * g.h, hipMemcpyHostToDevice);
  // everything above used blocking copies; d_cost is first touched by kernels on caller streams: clear it on the
  // context's (non-blocking) stream and wait, so no legacy-stream work is left behind the creation
  if (hipMemsetAsync(p->d_cost.as<double>(), 0, sizeof(double) * kCostSlots, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
    return fail(set_error(ctx, SRMAP_EHIP, "clearing the cost scalars failed"));
  model_replan(p);
  *out = p;
  return SRMAP_OK;
}

void srmap_problem_destroy(srmap_problem* p) {
  if (!p) return;
  holdout_pass_release(p);
  if (p->state_ev) (void)hipEventDestroy(p->state_ev);
  delete p;  // and every device buffer it owns
}

int srmap_problem_set_impl(srmap_problem* p, int impl) {
  if (!p) return SRMAP_EINVAL;
  if (impl < SRMAP_IMPL_AUTO || impl > SRMAP_IMPL_TILED) return set_error(p->ctx, SRMAP_EINVAL, "bad impl");
  p->impl = impl;
  p->plan_gen++;
  return SRMAP_OK;
}

// ---- affine per-frame motion model (no reference counterpart; generalises motion_module.cpp:18-51) ----
int srmap_problem_set_affine_motion(srmap_problem* p, const double* affine_2x3) {
  if (!p) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  MotionModel::Replacement r;  // stays empty for NULL: the created motion is restored
  if (affine_2x3) {
    if (int rc = affine_records(p->ctx, p->geo.K, affine_2x3, &r.recs)) return rc;  // the problem keeps the motion it had
    if (int rc = upload_vector(p, r.recs, &r.d_recs)) return rc;
    r.kind = kMotionAffine;
  }
  return p->motion.install(p, std::move(r));
}

// ---- free-form blur kernel (no reference counterpart; BlurModule builds a Gaussian only, blur_module.cpp:13-22) ----
int srmap_problem_set_blur_kernel(srmap_problem* p, int ksize, const double* taps) {
  if (!p) return SRMAP_EINVAL;
  return p->blur.install(p, 0, ksize, taps);
}

int srmap_problem_get_blur_kernel(const srmap_problem* p, int* ksize, double* taps_out) {
  if (!p) return SRMAP_EINVAL;
  if (ksize) *ksize = p->geo.b;
  if (taps_out && p->blur.is_bank())
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "a blur bank is set: no single kernel is in force (srmap_problem_get_blur_bank returns its entries)");
  if (taps_out) std::copy(p->blur.taps().begin(), p->blur.taps().end(), taps_out);
  return SRMAP_OK;
}

// ---- blur-kernel bank: a kernel per frame, per channel or per (frame, channel) (no reference counterpart) ----
int srmap_problem_set_blur_bank(srmap_problem* p, int mode, int ksize, const double* taps) {
  if (!p) return SRMAP_EINVAL;
  if (!taps) return p->blur.install(p, 0, 0, nullptr);
  if (int rc = BlurModel::check_bank_mode(p->ctx, mode)) return rc;
  return p->blur.install(p, mode, ksize, taps);
}

int srmap_problem_get_blur_bank(const srmap_problem* p, int* mode, int* ksize, double* taps_out) {
  if (!p) return SRMAP_EINVAL;
  if (mode) *mode = p->blur.bank_mode();
  if (ksize) *ksize = p->geo.b;
  if (taps_out && p->blur.is_bank()) std::copy(p->blur.taps().begin(), p->blur.taps().end(), taps_out);
  return SRMAP_OK;
}

int srmap_problem_set_solver(srmap_problem* p, int least_squares_solver, int num_lbfgs_hessian_corrections) {
  if (!p) return SRMAP_EINVAL;
  if (least_squares_solver != SRMAP_SOLVER_CG && least_squares_solver != SRMAP_SOLVER_LBFGS)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown least-squares solver %d", least_squares_solver);
  if (num_lbfgs_hessian_corrections < 1)
    return set_error(p->ctx, SRMAP_EINVAL, "num_lbfgs_hessian_corrections must be >= 1 (got %d)", num_lbfgs_hessian_corrections);
  if (num_lbfgs_hessian_corrections > kLbfgsMaxM)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "num_lbfgs_hessian_corrections %d: at most %d are supported",
                     num_lbfgs_hessian_corrections, kLbfgsMaxM);
  p->solver = least_squares_solver;
  p->lbfgs_m = num_lbfgs_hessian_corrections;
  return SRMAP_OK;
}

int srmap_problem_active_impl(const srmap_problem* p, int* impl) {
  if (!p || !impl) return SRMAP_EINVAL;
  *impl = ztile_active(p) ? SRMAP_IMPL_TILED : SRMAP_IMPL_DIRECT;
  return SRMAP_OK;
}

int srmap_problem_set_cost_rows(srmap_problem* p, int hr_row0, int hr_row1) {
  if (!p) return SRMAP_EINVAL;
  const Geometry& g = p->geo;
  if (hr_row0 < 0 || hr_row1 > g.H || hr_row0 >= hr_row1)
    return set_error(p->ctx, SRMAP_EINVAL, "cost rows [%d, %d) outside the image", hr_row0, hr_row1);
  if (hr_row0 % g.s != 0 || (hr_row1 % g.s != 0 && hr_row1 != g.H))
    return set_error(p->ctx, SRMAP_EINVAL, "cost rows must be multiples of the scale %d", g.s);
  p->geo.cr0 = hr_row0;
  p->geo.cr1 = hr_row1;
  return SRMAP_OK;
}

int srmap_problem_lr_size(const srmap_problem* p, int* lw, int* lh) {
  if (!p) return SRMAP_EINVAL;
  if (lw) *lw = p->geo.w;
  if (lh) *lh = p->geo.h;
  return SRMAP_OK;
}

int srmap_add_regularizer(srmap_problem* p, int kind, double lambda, int btv_range, double btv_decay,
                          int* reg_index) {
  if (!p) return SRMAP_EINVAL;
  if (kind != SRMAP_REG_TV && kind != SRMAP_REG_TV3D && kind != SRMAP_REG_BTV)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown regularizer kind %d", kind);
  if (p->nreg >= kMaxRegularizers) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "too many regularizers");
  RegSpec& rs = p->reg[p->nreg];
  rs = RegSpec{};
  rs.kind = kind;
  rs.lambda = lambda;
  if (kind == SRMAP_REG_BTV) {
    if (btv_range < 1) return set_error(p->ctx, SRMAP_EINVAL, "BTV range must be at least 1");  // btv_regularizer.cpp:58
    if (!(0 < btv_decay && btv_decay <= 1)) return set_error(p->ctx, SRMAP_EINVAL, "BTV decay must be in (0, 1]");
    if (btv_range > kMaxBtvRange) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "BTV range > %d", kMaxBtvRange);
    rs.range = btv_range;
    rs.decay = btv_decay;
    for (int i = 0; i < 2 * kMaxBtvRange + 1; ++i) rs.pow_table[i] = std::pow(btv_decay, i);
  }
  if (reg_index) *reg_index = p->nreg;
  p->nreg++;
  model_replan(p);
  return SRMAP_OK;
}

int srmap_problem_set_regularizer_lambda(srmap_problem* p, int reg, double lambda) {
  if (!p) return SRMAP_EINVAL;
  if (reg < 0 || reg >= p->nreg) return set_error(p->ctx, SRMAP_EINVAL, "no regularizer %d (the problem has %d)", reg, p->nreg);
  if (!(lambda >= 0.0 && std::isfinite(lambda)))
    return set_error(p->ctx, SRMAP_EINVAL, "the regularization parameter must be finite and >= 0 (got %g)", lambda);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (int rc = model_drain(p)) return rc;
  p->reg[reg].lambda = lambda;  // the IRLS weights stay as they are
  model_replan(p);
  return SRMAP_OK;
}

int srmap_problem_get_regularizer_lambda(const srmap_problem* p, int reg, double* lambda) {
  if (!p || !lambda) return SRMAP_EINVAL;
  if (reg < 0 || reg >= p->nreg) return set_error(p->ctx, SRMAP_EINVAL, "no regularizer %d (the problem has %d)", reg, p->nreg);
  *lambda = p->reg[reg].lambda;
  return SRMAP_OK;
}

int srmap_problem_set_regularizer_gradient(srmap_problem* p, int reg, int mode) {
  if (!p) return SRMAP_EINVAL;
  if (reg < 0 || reg >= p->nreg) return set_error(p->ctx, SRMAP_EINVAL, "no regularizer %d (the problem has %d)", reg, p->nreg);
  if (mode != SRMAP_REG_GRADIENT_REFERENCE && mode != SRMAP_REG_GRADIENT_EXACT)
    return set_error(p->ctx, SRMAP_EINVAL, "unknown regularizer gradient mode %d", mode);
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  if (int rc = model_drain(p)) return rc;
  p->reg[reg].gradient = mode;  // the cost, the values and the IRLS weights stay as they are
  model_replan(p);              // an exact BTV regulariser is not fused into the tiles (pick_fused_reg)
  return SRMAP_OK;
}

int srmap_problem_get_regularizer_gradient(const srmap_problem* p, int reg, int* mode) {
  if (!p || !mode) return SRMAP_EINVAL;
  if (reg < 0 || reg >= p->nreg) return set_error(p->ctx, SRMAP_EINVAL, "no regularizer %d (the problem has %d)", reg, p->nreg);
  *mode = p->reg[reg].gradient;
  return SRMAP_OK;
}

int srmap_clear_regularizers(srmap_problem* p) {
  if (!p) return SRMAP_EINVAL;
  for (int r = 0; r < p->nreg; ++r) p->reg[r].weights.reset();
  p->nreg = 0;
  model_replan(p);
  return SRMAP_OK;
}

}  // extern "C"
