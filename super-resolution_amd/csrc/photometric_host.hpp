// photometric_host.hpp -- host algebra of the photometric fit (srmap_fit_photometric, photometric_fit.hip):
// the per-frame gain / bias from the six weighted sums of one frame, and the energy those sums give at a parameter pair.
// Plain C++17, no HIP header (tests/cpp/photometric_test.cpp compiles it alone); the checker is
// tests/photometric_restatement.py.
#pragma once

#include <cmath>

namespace srmap {

// S = {sum w, sum w s, sum w y, sum w s^2, sum w s y, sum w y^2} of one frame (s the model's prediction, y the raw frame)
enum { kPhotoW = 0, kPhotoS = 1, kPhotoY = 2, kPhotoSS = 3, kPhotoSY = 4, kPhotoYY = 5, kPhotoSums = 6 };
enum { kPhotoGainBias = 0, kPhotoGainOnly = 1, kPhotoBiasOnly = 2 };
constexpr double kPhotoDetRtol = 1e-12;  // flat frame: determinant <= this * (sum w) (sum w s^2)

// E(a, b) = sum w (a s + b - y)^2, expanded over the sums
inline double photometric_energy(const double* S, double a, double b) {
  return ((a * a * S[kPhotoSS] + 2.0 * a * b * S[kPhotoS]) + b * b * S[kPhotoW]) -
         2.0 * (a * S[kPhotoSY] + b * S[kPhotoY]) + S[kPhotoYY];
}

struct PhotometricFit {
  double gain, bias;  // the result; the parameters in force for status 2 and 3
  double e0, e1;      // E at the parameters in force, E at the result
  int status;         // 0 fitted, 2 gain outside [min_gain, max_gain], 3 degenerate (no weight, a flat frame)
};

// The minimiser of E over (a, b) (model 0), over a with b held at b_cur (model 1), over b with a held at a_cur (model 2).
inline PhotometricFit photometric_solve(const double* S, int model, double a_cur, double b_cur, double min_gain,
                                        double max_gain) {
  PhotometricFit f;
  f.gain = a_cur;
  f.bias = b_cur;
  f.e0 = f.e1 = photometric_energy(S, a_cur, b_cur);
  f.status = 3;
  const double sw = S[kPhotoW], ss = S[kPhotoS], sy = S[kPhotoY], sss = S[kPhotoSS], ssy = S[kPhotoSY];
  if (!(sw > 0.0)) return f;
  double a = a_cur, b = b_cur;
  if (model == kPhotoGainBias) {
    const double det = sw * sss - ss * ss;
    if (!(det > kPhotoDetRtol * sw * sss)) return f;
    a = (sw * ssy - ss * sy) / det;
    b = (sss * sy - ss * ssy) / det;
  } else if (model == kPhotoGainOnly) {
    if (!(sss > 0.0)) return f;
    a = (ssy - b_cur * ss) / sss;
  } else {
    b = (sy - a_cur * ss) / sw;
  }
  if (!std::isfinite(a) || !std::isfinite(b)) return f;
  if (!(a >= min_gain && a <= max_gain)) {
    f.status = 2;
    return f;
  }
  f.gain = a;
  f.bias = b;
  f.e1 = photometric_energy(S, a, b);
  f.status = 0;
  return f;
}

}  // namespace srmap
