// solver_host.hpp -- the host arithmetic of the inner solvers (solver.hip) that touches no device: the More'-Thuente
// safeguarded step of the line search, the L-BFGS two-loop recursion on coefficients and its Gram tables.  Plain C++ in double, in
// ALGLIB's order of operations; tests/cpp/solver_host_test.cpp runs it without a GPU against the numpy restatement
// (tests/lbfgs_restatement.py), bit for bit.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

#include "solver_mailbox.hpp"

namespace srmap {

inline double dmax(double a, double b) { return a > b ? a : b; }
inline double dmin(double a, double b) { return a < b ? a : b; }

// More'-Thuente safeguarded step (MINPACK-2 dcstep; ALGLIB linmin_mcstep,
// alglibinternal.cpp:12972-13232).
struct Bracket { double stx, fx, dx, sty, fy, dy; };

inline double cubic_gamma(double theta, double da, double db, bool clamp0) {
  const double s = dmax(std::fabs(theta), dmax(std::fabs(da), std::fabs(db)));
  double t = (theta / s) * (theta / s) - da / s * (db / s);
  if (clamp0) t = dmax(0.0, t);
  return s * std::sqrt(t);
}

inline void mt_step(Bracket* b, double* stp, double fp, double dp, bool* brackt, double stmin,
                    double stmax, int* info) {
  *info = 0;
  if ((*brackt && (*stp <= dmin(b->stx, b->sty) || *stp >= dmax(b->stx, b->sty))) ||
      b->dx * (*stp - b->stx) >= 0 || stmax < stmin)
    return;
  const double sgnd = dp * (b->dx / std::fabs(b->dx));
  bool bound;
  double stpf;
  if (fp > b->fx) {
    *info = 1; bound = true;
    const double theta = 3 * (b->fx - fp) / (*stp - b->stx) + b->dx + dp;
    double gamma = cubic_gamma(theta, b->dx, dp, false);
    if (*stp < b->stx) gamma = -gamma;
    const double pp = gamma - b->dx + theta, q = gamma - b->dx + gamma + dp, r = pp / q;
    const double stpc = b->stx + r * (*stp - b->stx);
    const double stpq = b->stx + b->dx / ((b->fx - fp) / (*stp - b->stx) + b->dx) / 2 * (*stp - b->stx);
    stpf = std::fabs(stpc - b->stx) < std::fabs(stpq - b->stx) ? stpc : stpc + (stpq - stpc) / 2;
    *brackt = true;
  } else if (sgnd < 0) {
    *info = 2; bound = false;
    const double theta = 3 * (b->fx - fp) / (*stp - b->stx) + b->dx + dp;
    double gamma = cubic_gamma(theta, b->dx, dp, false);
    if (*stp > b->stx) gamma = -gamma;
    const double pp = gamma - dp + theta, q = gamma - dp + gamma + b->dx, r = pp / q;
    const double stpc = *stp + r * (b->stx - *stp);
    const double stpq = *stp + dp / (dp - b->dx) * (b->stx - *stp);
    stpf = std::fabs(stpc - *stp) > std::fabs(stpq - *stp) ? stpc : stpq;
    *brackt = true;
  } else if (std::fabs(dp) < std::fabs(b->dx)) {
    *info = 3; bound = true;
    const double theta = 3 * (b->fx - fp) / (*stp - b->stx) + b->dx + dp;
    double gamma = cubic_gamma(theta, b->dx, dp, true);
    if (*stp > b->stx) gamma = -gamma;
    const double pp = gamma - dp + theta, q = gamma + (b->dx - dp) + gamma, r = pp / q;
    double stpc;
    if (r < 0 && gamma != 0) stpc = *stp + r * (b->stx - *stp);
    else stpc = *stp > b->stx ? stmax : stmin;
    const double stpq = *stp + dp / (dp - b->dx) * (b->stx - *stp);
    if (*brackt) stpf = std::fabs(*stp - stpc) < std::fabs(*stp - stpq) ? stpc : stpq;
    else stpf = std::fabs(*stp - stpc) > std::fabs(*stp - stpq) ? stpc : stpq;
  } else {
    *info = 4; bound = false;
    if (*brackt) {
      const double theta = 3 * (fp - b->fy) / (b->sty - *stp) + b->dy + dp;
      double gamma = cubic_gamma(theta, b->dy, dp, false);
      if (*stp > b->sty) gamma = -gamma;
      const double pp = gamma - dp + theta, q = gamma - dp + gamma + b->dy, r = pp / q;
      stpf = *stp + r * (b->sty - *stp);
    } else {
      stpf = *stp > b->stx ? stmax : stmin;
    }
  }
  if (fp > b->fx) {
    b->sty = *stp; b->fy = fp; b->dy = dp;
  } else {
    if (sgnd < 0.0) { b->sty = b->stx; b->fy = b->fx; b->dy = b->dx; }
    b->stx = *stp; b->fx = fp; b->dx = dp;
  }
  stpf = dmin(stmax, stpf);
  stpf = dmax(stmin, stpf);
  *stp = stpf;
  if (*brackt && bound) {
    if (b->sty > b->stx) *stp = dmin(b->stx + 0.66 * (b->sty - b->stx), *stp);
    else *stp = dmax(b->stx + 0.66 * (b->sty - b->stx), *stp);
  }
}


// ALGLIB's two loops of minlbfgs (optimization.cpp:21640 ff.) on the COEFFICIENTS of work = cgc g + sum_j (cs_j s_j +
// cy_j y_j) over the ring slots, starting from work = g, every dot product taken from the Gram tables SY[a * m + b] =
// s_a.y_b, YY[a * m + b] = y_a.y_b, gs[j] = g.s_j, gy[j] = g.y_j (g the current gradient).  k: pairs accepted before this
// one (slot p = k % m holds the newest), q = min(k, m - 1), q + 1 live slots.  Sets rho[p] and fills coef[0] = cgc,
// coef[1 + 2j] = cs_j, coef[2 + 2j] = cy_j for j <= q (LbfgsCoef's layout; the direction is -work).  Returns false, with
// nothing written, when s_p.y_p == 0 or y_p.y_p == 0 (ALGLIB ends the run with -2).
inline bool lbfgs_two_loop(const double* SY, const double* YY, const double* gs, const double* gy, double* rho, int k,
                           int q, int m, double* coef) {
  const int p = k % m, live = q + 1;
  const double v = SY[(size_t)p * m + p], vv = YY[(size_t)p * m + p];
  if (v == 0 || vv == 0) return false;
  rho[p] = 1 / v;
  const double gammak = v / vv;
  std::vector<double> cs(m, 0.0), cy(m, 0.0), theta(m, 0.0);
  double cgc = 1.0;
  for (int i = k; i >= k - q; --i) {
    const int ic = i % m;
    double t = cgc * gs[ic];  // s_ic.work (the s coefficients are still 0)
    for (int j = 0; j < live; ++j) t += cy[j] * SY[(size_t)ic * m + j];
    theta[ic] = t;
    cy[ic] -= t * rho[ic];
  }
  cgc *= gammak;
  for (int j = 0; j < live; ++j) cy[j] *= gammak;
  for (int i = k - q; i <= k; ++i) {
    const int ic = i % m;
    double t = cgc * gy[ic];  // y_ic.work
    for (int j = 0; j < live; ++j) t += cs[j] * SY[(size_t)j * m + ic] + cy[j] * YY[(size_t)ic * m + j];
    cs[ic] += rho[ic] * (-t + theta[ic]);
  }
  coef[0] = cgc;
  for (int j = 0; j < live; ++j) { coef[1 + 2 * j] = cs[j]; coef[2 + 2 * j] = cy[j]; }
  return true;
}

// The rows r of the update pass that wrote the new pair to ring slot p (solver_mailbox.hpp: lb_row) into the tables above,
// `live` slots holding pairs.  The pass recomputes every entry that involves slot p; the older pairs' entries stay.
inline void lbfgs_unpack_rows(const double* r, int p, int live, int m, double* SY, double* YY, double* gs, double* gy) {
  for (int j = 0; j < live; ++j) {
    SY[(size_t)p * m + j] = r[lb_row(j, kLbSyj)];
    SY[(size_t)j * m + p] = r[lb_row(j, kLbYsj)];
    YY[(size_t)p * m + j] = YY[(size_t)j * m + p] = r[lb_row(j, kLbYyj)];
    gs[j] = r[lb_row(j, kLbGsj)];
    gy[j] = r[lb_row(j, kLbGyj)];
  }
}

}  // namespace srmap
