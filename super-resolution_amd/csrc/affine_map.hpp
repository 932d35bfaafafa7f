// affine_map.hpp -- host algebra of the 2 x 3 frame maps [a b tx; c d ty] that problem.hip (affine_records), registration.hip,
// registration_affine.hip and motion_refinement.hip share: ONE copy of each expression, so that the records, the
// registration and the refinement cannot drift apart.  Plain C++17, no HIP header (tests/cpp/affine_map_test.cpp compiles
// it alone); the checkers are tests/affine_registration_restatement.py and tests/motion_refinement_restatement.py.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace srmap {

struct AffineMap { double m[6]; };

// max(|a-1|+|b|, |c|+|d-1|): the model's domain is deviation <= kAffineMaxDeviation
inline double deviation(const AffineMap& F) {
  return std::max(std::fabs(F.m[0] - 1.0) + std::fabs(F.m[1]), std::fabs(F.m[3]) + std::fabs(F.m[4] - 1.0));
}
inline bool all_finite(const AffineMap& F) {
  for (double v : F.m) if (!std::isfinite(v)) return false;
  return true;
}
inline AffineMap inverse(const AffineMap& F) {
  const double a = F.m[0], b = F.m[1], tx = F.m[2], c = F.m[3], d = F.m[4], ty = F.m[5];
  const double det = a * d - b * c;  // >= 0.75^2 - 0.25^2 inside the domain
  const double ia = d / det, ib = -b / det, ic = -c / det, id = a / det;
  AffineMap G;
  G.m[0] = ia; G.m[1] = ib; G.m[2] = -(ia * tx + ib * ty);
  G.m[3] = ic; G.m[4] = id; G.m[5] = -(ic * tx + id * ty);
  return G;
}
// one pyramid level down: fine p = 2 u + 1/2: L unchanged, t_fine = 2 t + (1/2, 1/2) - L (1/2, 1/2)
inline AffineMap to_finer(const AffineMap& F) {
  AffineMap G = F;
  G.m[2] = 2.0 * F.m[2] + 0.5 - (F.m[0] * 0.5 + F.m[1] * 0.5);
  G.m[5] = 2.0 * F.m[5] + 0.5 - (F.m[3] * 0.5 + F.m[4] * 0.5);
  return G;
}
inline AffineMap to_coarser(const AffineMap& F) {
  AffineMap G = F;
  G.m[2] = 0.5 * (F.m[2] - 0.5 + (F.m[0] * 0.5 + F.m[1] * 0.5));
  G.m[5] = 0.5 * (F.m[5] - 0.5 + (F.m[3] * 0.5 + F.m[4] * 0.5));
  return G;
}
// largest distance between A(p) and B(p) over the four corners p of a w x h image
inline double corner_displacement(const AffineMap& A, const AffineMap& B, int w, int h) {
  double worst = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double x = (i & 1) ? w - 1.0 : 0.0, y = (i & 2) ? h - 1.0 : 0.0;
    const double dx = (A.m[0] - B.m[0]) * x + (A.m[1] - B.m[1]) * y + (A.m[2] - B.m[2]);
    const double dy = (A.m[3] - B.m[3]) * x + (A.m[4] - B.m[4]) * y + (A.m[5] - B.m[5]);
    worst = std::max(worst, std::hypot(dx, dy));
  }
  return worst;
}
// The inverse-compositional update F o W^-1, W(p) = p + D (p - c) + d with D = [D0 D1; D3 D4], d = (D2, D5),
// c = ((w-1)/2, (h-1)/2)
inline AffineMap compose_with_inverse(const AffineMap& F, const double* delta, int w, int h) {
  const double cx = 0.5 * (w - 1), cy = 0.5 * (h - 1);
  const double A00 = 1.0 + delta[0], A01 = delta[1], A10 = delta[3], A11 = 1.0 + delta[4];
  const double tx = delta[2] - (delta[0] * cx + delta[1] * cy), ty = delta[5] - (delta[3] * cx + delta[4] * cy);
  const double det = A00 * A11 - A01 * A10;
  const double i00 = A11 / det, i01 = -A01 / det, i10 = -A10 / det, i11 = A00 / det;
  AffineMap G;
  G.m[0] = F.m[0] * i00 + F.m[1] * i10;
  G.m[1] = F.m[0] * i01 + F.m[1] * i11;
  G.m[3] = F.m[3] * i00 + F.m[4] * i10;
  G.m[4] = F.m[3] * i01 + F.m[4] * i11;
  G.m[2] = F.m[2] - (G.m[0] * tx + G.m[1] * ty);
  G.m[5] = F.m[5] - (G.m[3] * tx + G.m[4] * ty);
  return G;
}
// The additive update of the refinement: G + dL (q - c0) + dt as a map of q
inline AffineMap increment(const AffineMap& G, const double* d, double c0x, double c0y) {
  AffineMap N;
  N.m[0] = G.m[0] + d[0]; N.m[1] = G.m[1] + d[1]; N.m[2] = G.m[2] + (d[2] - (d[0] * c0x + d[1] * c0y));
  N.m[3] = G.m[3] + d[3]; N.m[4] = G.m[4] + d[4]; N.m[5] = G.m[5] + (d[5] - (d[3] * c0x + d[4] * c0y));
  return N;
}

// A x = rhs over the leading n x n block of A (n <= 6) by Cholesky; false (no texture) where a pivot is not above
// kCholeskyPivotRtol of its diagonal entry.  The callers build their own system.
constexpr double kCholeskyPivotRtol = 1e-12;
inline bool cholesky_solve(const double A[6][6], const double* rhs, int n, double* x) {
  double Lc[6][6] = {}, y[6];
  for (int j = 0; j < n; ++j) {
    double p = A[j][j];
    for (int k = 0; k < j; ++k) p -= Lc[j][k] * Lc[j][k];
    if (!(A[j][j] > 0.0 && p > kCholeskyPivotRtol * A[j][j])) return false;
    Lc[j][j] = std::sqrt(p);
    for (int i = j + 1; i < n; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= Lc[i][k] * Lc[j][k];
      Lc[i][j] = s / Lc[j][j];
    }
  }
  for (int i = 0; i < n; ++i) {
    double s = rhs[i];
    for (int k = 0; k < i; ++k) s -= Lc[i][k] * y[k];
    y[i] = s / Lc[i][i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < n; ++k) s -= Lc[k][i] * x[k];
    x[i] = s / Lc[i][i];
  }
  return true;
}

// The sized copy of the factorisation above for the blur fit (blur_fit.hip: n = ksize^2 <= 49): A = L L^T over the n x n
// row-major matrix A, the same pivot test.  L replaces nothing: it goes to Lc (n x n, lower triangle).  pivot_min /
// pivot_max receive the smallest / largest pivot (the squares of L's diagonal).  false: no texture.
inline bool cholesky_factor_n(const double* A, int n, double* Lc, double* pivot_min, double* pivot_max) {
  double lo = 0.0, hi = 0.0;
  for (int j = 0; j < n; ++j) {
    double p = A[j * n + j];
    for (int k = 0; k < j; ++k) p -= Lc[j * n + k] * Lc[j * n + k];
    if (!(A[j * n + j] > 0.0 && p > kCholeskyPivotRtol * A[j * n + j])) return false;
    lo = j == 0 ? p : std::min(lo, p);
    hi = j == 0 ? p : std::max(hi, p);
    Lc[j * n + j] = std::sqrt(p);
    for (int i = j + 1; i < n; ++i) {
      double s = A[i * n + j];
      for (int k = 0; k < j; ++k) s -= Lc[i * n + k] * Lc[j * n + k];
      Lc[i * n + j] = s / Lc[j * n + j];
    }
  }
  if (pivot_min) *pivot_min = lo;
  if (pivot_max) *pivot_max = hi;
  return true;
}
// x = (L L^T)^-1 rhs by the two triangular solves of cholesky_solve
inline void cholesky_apply_n(const double* Lc, int n, const double* rhs, double* x) {
  for (int i = 0; i < n; ++i) {
    double s = rhs[i];
    for (int k = 0; k < i; ++k) s -= Lc[i * n + k] * x[k];
    x[i] = s / Lc[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = x[i];
    for (int k = i + 1; k < n; ++k) s -= Lc[k * n + i] * x[k];
    x[i] = s / Lc[i * n + i];
  }
}

// Separation of a coarse search's minimum: 1 - msd[best] / runner-up, the runner-up being the smallest entry of the
// n1 x n1 table (row-major) at least 2 cells away from `best`; entries < 0 (a candidate that was not evaluated) are
// skipped.  Near 1 = one clear minimum, near 0 = ambiguous; 0 where no runner-up is positive.
inline double search_separation(const double* msd, int n1, int best) {
  double runner = -1.0;
  for (int c = 0; c < n1 * n1; ++c) {
    if (msd[c] < 0 || std::max(std::abs(c % n1 - best % n1), std::abs(c / n1 - best / n1)) < 2) continue;
    if (runner < 0 || msd[c] < runner) runner = msd[c];
  }
  return runner > 0 ? 1.0 - msd[best] / runner : 0.0;
}

}  // namespace srmap
