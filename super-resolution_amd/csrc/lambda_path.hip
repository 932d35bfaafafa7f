// lambda_path.hip -- the regularisation weight by hold-out validation (no reference counterpart):
// srmap_solve_lambda_path solves the problem once per multiplier of its lambdas, scores every solution on the held-out
// observations (holdout.hip) and keeps the best.  Host-paced orchestration of calls that exist on their own: row j is bit
// for bit srmap_problem_set_regularizer_lambda, srmap_solve from x0, srmap_holdout_score; the final solve is
// srmap_problem_set_holdout(0), srmap_solve from x0.  The start is staged once; the iterates and the best image so far stay
// on the device, and per row only the solve's scalars and the score's sums return.  The rules of the choice and of the
// early stop are holdout_host.hpp's.  No kernel of its own.  srmap_solve_lambda_path_folds is the cross-validated form: per
// multiplier one solve and score for every fold of a partition of the observations (srmap_problem_set_holdout_fold), the
// mean and the standard error over the folds, and the one-standard-error rule.
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "holdout_host.hpp"
#include "srmap_internal.hpp"

using namespace srmap;

extern "C" {

void srmap_lambda_path_options_default(srmap_lambda_path_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_lambda_path_options);
  o->num_scales = 8;
  for (int j = 0; j < SRMAP_LAMBDA_PATH_MAX_SCALES; ++j) o->scales[j] = j < 8 ? std::ldexp(1.0, -j) : 0.0;
  o->patience = 0;
  o->final_solve = 1;
}

int srmap_solve_lambda_path(srmap_problem* p, const srmap_irls_options* irls_options, const srmap_lambda_path_options* path_options,
                            const double* x0, double* x_out, double* table, int* rows_run, int* chosen,
                            srmap_solve_report* final_report) {
  if (!p || !x0 || !x_out || !table || !rows_run || !chosen) return SRMAP_EINVAL;
  *rows_run = 0;
  *chosen = -1;
  srmap_lambda_path_options po;
  if (int rc = options_in_force(p->ctx, path_options, srmap_lambda_path_options_default, "srmap_lambda_path_options", &po)) return rc;
  srmap_irls_options io;
  if (int rc = irls_options_in_force(p, irls_options, &io)) return rc;
  if (po.num_scales < 1 || po.num_scales > SRMAP_LAMBDA_PATH_MAX_SCALES)
    return set_error(p->ctx, SRMAP_EINVAL, "lambda path: num_scales must be in 1...%d (got %d)", SRMAP_LAMBDA_PATH_MAX_SCALES, po.num_scales);
  for (int j = 0; j < po.num_scales; ++j)
    if (!(po.scales[j] > 0.0 && std::isfinite(po.scales[j])) || (j > 0 && !(po.scales[j] < po.scales[j - 1])))
      return set_error(p->ctx, SRMAP_EINVAL, "lambda path: the scales must be finite, > 0 and strictly decreasing (scale %d is %g)", j, po.scales[j]);
  if (po.patience < 0) return set_error(p->ctx, SRMAP_EINVAL, "lambda path: patience must be >= 0 (got %d)", po.patience);
  const DataWeights::Holdout hold = p->dw.holdout();
  if (!hold.threshold) return set_error(p->ctx, SRMAP_EINVAL, "lambda path: no hold-out set (srmap_problem_set_holdout)");
  bool any = false;
  for (int r = 0; r < p->nreg; ++r) any = any || p->reg[r].lambda > 0.0;
  if (!any) return set_error(p->ctx, SRMAP_EINVAL, "lambda path: no regularizer with lambda > 0 (srmap_add_regularizer)");
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "lambda path: no observations set (srmap_set_observations)");
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));

  const int K = p->geo.K, nreg = p->nreg;
  const hipStream_t st = p->ctx->stream;
  double lambda0[kMaxRegularizers];
  for (int r = 0; r < nreg; ++r) lambda0[r] = p->reg[r].lambda;
  auto set_lambdas = [&](double scale) {
    for (int r = 0; r < nreg; ++r)
      if (int rc = srmap_problem_set_regularizer_lambda(p, r, lambda0[r] * scale)) return rc;
    return (int)SRMAP_OK;
  };
  bool lifted = false;
  // an error: the lambdas of the call's start again, and the hold-out if the final solve had lifted it; the first error
  // stands.  Best effort: should one of these setters fail in turn (a device error), its status is dropped and the
  // problem may be left with the lambdas or without the hold-out of the row that failed
  auto fail = [&](int rc) {
    const std::string msg = p->ctx->error;
    (void)set_lambdas(1.0);
    if (lifted) (void)p->dw.set_holdout(p, hold);
    p->ctx->error = msg;
    return rc;
  };

  const size_t n = p->hr_count(), bytes = n * p->elem();
  DevBuf x0d, xrow, xbest;
  if (x0d.alloc(bytes) != hipSuccess || xrow.alloc(bytes) != hipSuccess || xbest.alloc(bytes) != hipSuccess)
    return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (lambda path: 3 x %zu bytes)", bytes);
  if (int rc = convert_upload(p, x0, x0d.as(), n, st)) return rc;  // staged once (waited for: x0 is the caller's)

  // the path's delta: 0 under L2, the problem's under Huber / FIXED, row 0's last Huber step's under MAD -- held for every row
  const bool huber = p->dw.loss() == SRMAP_DATA_LOSS_HUBER;
  const bool mad = huber && p->dw.scale_mode() == SRMAP_HUBER_DELTA_MAD;
  double delta = huber && !mad ? p->dw.delta() : 0.0;
  std::vector<double> scores, score(1 + K), sums((size_t)(1 + K) * 4);
  std::vector<srmap_solve_report> reports;
  int best = -1;
  for (int j = 0; j < po.num_scales; ++j) {
    if (int rc = set_lambdas(po.scales[j])) return fail(rc);
    srmap_solve_report rep;
    if (int rc = solve_device(p, &io, x0d.as(), xrow.as(), &rep)) return fail(rc);
    if (mad && j == 0)
      if (int rc = srmap_problem_get_huber_delta(p, nullptr, &delta, nullptr, nullptr)) return fail(rc);
    if (int rc = srmap_holdout_score_device(p, xrow.as(), st, delta, score.data(), sums.data())) return fail(rc);
    double* row = table + (size_t)j * SRMAP_LAMBDA_PATH_ROW;
    row[0] = po.scales[j];
    row[1] = score[0];
    for (int q = 0; q < 4; ++q) row[2 + q] = sums[q];
    row[6] = rep.irls_rounds;
    row[7] = rep.cg_iterations;
    row[8] = rep.evaluations;
    row[9] = rep.final_cost;
    row[10] = delta;
    scores.push_back(score[0]);
    reports.push_back(rep);
    *rows_run = j + 1;
    const int now = holdout_choose(scores.data(), j + 1);
    if (now == j) std::swap(xrow, xbest);  // the best image so far stays where it is: the buffers change roles
    best = now;
    if (holdout_patience_stop(scores.data(), j + 1, po.patience)) break;
  }
  if (best < 0) return fail(set_error(p->ctx, SRMAP_EINVAL, "lambda path: no row has a score that is a number"));
  *chosen = best;
  if (int rc = set_lambdas(po.scales[best])) return fail(rc);
  srmap_solve_report rep = reports[best];
  if (po.final_solve) {  // on all observations: the hold-out is lifted for this solve alone
    if (int rc = p->dw.set_holdout(p, DataWeights::Holdout())) return fail(rc);
    lifted = true;
    if (int rc = solve_device(p, &io, x0d.as(), xrow.as(), &rep)) return fail(rc);
    if (int rc = p->dw.set_holdout(p, hold)) return fail(rc);
    lifted = false;
    if (int rc = convert_download(p, xrow.as(), x_out, n, st)) return fail(rc);
  } else {
    if (int rc = convert_download(p, xbest.as(), x_out, n, st)) return fail(rc);
  }
  if (final_report) *final_report = rep;
  return SRMAP_OK;
}

void srmap_lambda_cv_options_default(srmap_lambda_cv_options* o) {
  if (!o) return;
  o->struct_size = (int)sizeof(srmap_lambda_cv_options);
  o->num_scales = 8;
  for (int j = 0; j < SRMAP_LAMBDA_PATH_MAX_SCALES; ++j) o->scales[j] = j < 8 ? std::ldexp(1.0, -j) : 0.0;
  o->folds = 5;
  o->seed = 1;
  o->rule = SRMAP_LAMBDA_RULE_ONE_SE;
  o->se_factor = 1.0;
  o->patience = 0;
  o->final_solve = 1;
}

// The cross-validated path: rows outside, folds inside.  Row j, fold f is bit for bit srmap_problem_set_regularizer_lambda
// for every regulariser, srmap_problem_set_holdout_fold(folds, f, seed), srmap_solve from x0, srmap_holdout_score.  The
// statistics of a row and the choice are holdout_host.hpp's
int srmap_solve_lambda_path_folds(srmap_problem* p, const srmap_irls_options* irls_options, const srmap_lambda_cv_options* cv_options,
                                  const double* x0, double* x_out, double* table, double* fold_table, int* rows_run, int* chosen,
                                  srmap_solve_report* final_report) {
  if (!p || !x0 || !table || !rows_run || !chosen) return SRMAP_EINVAL;
  *rows_run = 0;
  *chosen = -1;
  srmap_lambda_cv_options po;
  if (int rc = options_in_force(p->ctx, cv_options, srmap_lambda_cv_options_default, "srmap_lambda_cv_options", &po)) return rc;
  if (po.final_solve && !x_out) return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): the final solve needs x_out");
  srmap_irls_options io;
  if (int rc = irls_options_in_force(p, irls_options, &io)) return rc;
  if (po.num_scales < 1 || po.num_scales > SRMAP_LAMBDA_PATH_MAX_SCALES)
    return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): num_scales must be in 1...%d (got %d)", SRMAP_LAMBDA_PATH_MAX_SCALES, po.num_scales);
  for (int j = 0; j < po.num_scales; ++j)
    if (!(po.scales[j] > 0.0 && std::isfinite(po.scales[j])) || (j > 0 && !(po.scales[j] < po.scales[j - 1])))
      return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): the scales must be finite, > 0 and strictly decreasing (scale %d is %g)", j, po.scales[j]);
  if (po.folds < kHoldoutMinFolds || po.folds > kHoldoutMaxFolds)
    return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): folds must be in %d...%d (got %d)", kHoldoutMinFolds, kHoldoutMaxFolds, po.folds);
  if (po.rule != SRMAP_LAMBDA_RULE_MIN && po.rule != SRMAP_LAMBDA_RULE_ONE_SE)
    return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): rule must be SRMAP_LAMBDA_RULE_MIN or SRMAP_LAMBDA_RULE_ONE_SE (got %d)", po.rule);
  if (!(po.se_factor >= 0.0 && std::isfinite(po.se_factor)))
    return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): se_factor must be finite and >= 0 (got %g)", po.se_factor);
  if (po.patience < 0) return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): patience must be >= 0 (got %d)", po.patience);
  bool any = false;
  for (int r = 0; r < p->nreg; ++r) any = any || p->reg[r].lambda > 0.0;
  if (!any) return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): no regularizer with lambda > 0 (srmap_add_regularizer)");
  if (!p->have_obs) return set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): no observations set (srmap_set_observations)");
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));

  const int K = p->geo.K, nreg = p->nreg, F = po.folds;
  const hipStream_t st = p->ctx->stream;
  const DataWeights::Holdout hold = p->dw.holdout();  // as it is at the call -- maybe none --, and as it is on every return
  double lambda0[kMaxRegularizers];
  for (int r = 0; r < nreg; ++r) lambda0[r] = p->reg[r].lambda;
  auto set_lambdas = [&](double scale) {
    for (int r = 0; r < nreg; ++r)
      if (int rc = srmap_problem_set_regularizer_lambda(p, r, lambda0[r] * scale)) return rc;
    return (int)SRMAP_OK;
  };
  // an error: the lambdas and the hold-out of the call's start again; the first error stands (best effort, as
  // srmap_solve_lambda_path's)
  auto fail = [&](int rc) {
    const std::string msg = p->ctx->error;
    (void)set_lambdas(1.0);
    (void)p->dw.set_holdout(p, hold);
    p->ctx->error = msg;
    return rc;
  };

  const size_t n = p->hr_count(), bytes = n * p->elem();
  DevBuf x0d, xrow;
  if (x0d.alloc(bytes) != hipSuccess || xrow.alloc(bytes) != hipSuccess)
    return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed (lambda path (folds): 2 x %zu bytes)", bytes);
  if (int rc = convert_upload(p, x0, x0d.as(), n, st)) return rc;  // staged once (waited for: x0 is the caller's)

  // the path's delta: srmap_solve_lambda_path's rule; under MAD the last Huber step's of row 0, fold 0 -- held for every row and fold
  const bool huber = p->dw.loss() == SRMAP_DATA_LOSS_HUBER;
  const bool mad = huber && p->dw.scale_mode() == SRMAP_HUBER_DELTA_MAD;
  double delta = huber && !mad ? p->dw.delta() : 0.0;
  std::vector<double> means, ses, s(F), score(1 + K), sums((size_t)(1 + K) * 4);
  for (int j = 0; j < po.num_scales; ++j) {
    if (int rc = set_lambdas(po.scales[j])) return fail(rc);
    double pooled[4] = {0.0, 0.0, 0.0, 0.0}, counts[3] = {0.0, 0.0, 0.0};
    for (int f = 0; f < F; ++f) {
      if (int rc = srmap_problem_set_holdout_fold(p, F, f, po.seed)) return fail(rc);
      srmap_solve_report rep;
      if (int rc = solve_device(p, &io, x0d.as(), xrow.as(), &rep)) return fail(rc);
      if (mad && j == 0 && f == 0)
        if (int rc = srmap_problem_get_huber_delta(p, nullptr, &delta, nullptr, nullptr)) return fail(rc);
      if (int rc = srmap_holdout_score_device(p, xrow.as(), st, delta, score.data(), sums.data())) return fail(rc);
      s[f] = score[0];
      for (int q = 0; q < 4; ++q) pooled[q] += sums[q];
      counts[0] += rep.irls_rounds;
      counts[1] += rep.cg_iterations;
      counts[2] += rep.evaluations;
      if (fold_table) {
        double* row = fold_table + ((size_t)j * F + f) * SRMAP_LAMBDA_PATH_ROW;
        row[0] = po.scales[j];
        row[1] = score[0];
        for (int q = 0; q < 4; ++q) row[2 + q] = sums[q];
        row[6] = rep.irls_rounds;
        row[7] = rep.cg_iterations;
        row[8] = rep.evaluations;
        row[9] = rep.final_cost;
        row[10] = delta;
      }
    }
    double mean = 0.0, se = 0.0;
    holdout_fold_stats(s.data(), F, &mean, &se);
    double* row = table + (size_t)j * SRMAP_LAMBDA_PATH_ROW;
    row[0] = po.scales[j];
    row[1] = mean;
    row[2] = se;
    for (int q = 0; q < 4; ++q) row[3 + q] = pooled[q];
    for (int q = 0; q < 3; ++q) row[7 + q] = counts[q];
    row[10] = delta;
    means.push_back(mean);
    ses.push_back(se);
    *rows_run = j + 1;
    if (holdout_patience_stop(means.data(), j + 1, po.patience)) break;
  }
  const int best = holdout_choose_folds(means.data(), ses.data(), *rows_run, po.rule, po.se_factor, nullptr);
  if (best < 0) return fail(set_error(p->ctx, SRMAP_EINVAL, "lambda path (folds): no row has a mean score that is a number"));
  *chosen = best;
  if (int rc = set_lambdas(po.scales[best])) return fail(rc);
  if (po.final_solve) {  // on all observations
    if (int rc = p->dw.set_holdout(p, DataWeights::Holdout())) return fail(rc);
    srmap_solve_report rep;
    if (int rc = solve_device(p, &io, x0d.as(), xrow.as(), &rep)) return fail(rc);
    if (int rc = convert_download(p, xrow.as(), x_out, n, st)) return fail(rc);
    if (final_report) *final_report = rep;
  }
  if (int rc = p->dw.set_holdout(p, hold)) return fail(rc);
  return SRMAP_OK;
}

}  // extern "C"
