// lambda_path.hip -- the regularisation weight by hold-out validation (no reference counterpart):
// srmap_solve_lambda_path solves the problem once per multiplier of its lambdas, scores every solution on the held-out
// observations (holdout.hip) and keeps the best.  Host-paced orchestration of calls that exist on their own: row j is bit
// for bit srmap_problem_set_regularizer_lambda, srmap_solve from x0, srmap_holdout_score; the final solve is
// srmap_problem_set_holdout(0), srmap_solve from x0.  The start is staged once; the iterates and the best image so far stay
// on the device, and per row only the solve's scalars and the score's sums return.  The rules of the choice and of the
// early stop are holdout_host.hpp's.  No kernel of its own.
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

}  // extern "C"
