// holdout_host.hpp -- the host arithmetic of hold-out validation (holdout.hip, lambda_path.hip): which
// observations a hold-out keeps out of the data term, the threshold of a fraction, the band of a fold, and the rules of the
// lambda paths (the chosen row, the early stop; per row of the cross-validated path the mean and the standard error over
// the folds, and the one-standard-error rule).  Plain C++17, includes nothing of HIP: the library's host code and
// tests/cpp/holdout_test.cpp share this one copy; the device twin of holdout_hash is holdout_dev.hpp's, and the checker of
// both is tests/holdout_restatement.py.
//
// Observation i -- the flat index into the whole problem's [K][C][h][w], the same under a split_channels view -- is held
// out iff the top 24 bits of a 64-bit mix of (i, seed) are below T = floor(fraction * 2^24).  The mix is the splitmix64
// finaliser over i + seed * the golden-ratio increment: a pure function of the index, so no mask stream exists anywhere,
// and the kernels that need h recompute it.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace srmap {

constexpr int kHoldoutBits = 24;  // the share of held-out observations is T / 2^24

inline uint64_t holdout_hash(uint64_t i, uint64_t seed) {
  uint64_t z = i + seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

inline bool holdout_held(uint64_t i, uint64_t seed, uint32_t threshold) {
  return (uint32_t)(holdout_hash(i, seed) >> (64 - kHoldoutBits)) < threshold;
}

// T of a fraction in (0, 0.5], formed in double; 0: the fraction is refused (outside the interval, not a number, or so
// small that nothing could be held out)
inline uint32_t holdout_threshold(double fraction) {
  if (!(fraction > 0.0 && fraction <= 0.5)) return 0u;
  return (uint32_t)std::floor(fraction * (double)(1u << kHoldoutBits));
}

// The band form of the same test: held out iff lo <= hash24(i, seed) < hi, lo <= hi <= 2^24.  [0, T) is holdout_held
inline bool holdout_held_band(uint64_t i, uint64_t seed, uint32_t lo, uint32_t hi) {
  const uint32_t v = (uint32_t)(holdout_hash(i, seed) >> (64 - kHoldoutBits));
  return v >= lo && v < hi;
}

// Fold `fold` of `folds` (srmap_problem_set_holdout_fold): the band [floor(fold 2^24 / folds), floor((fold + 1) 2^24 / folds))
// in integer arithmetic.  The bands of a partition meet end to start, the first begins at 0 and the last ends at 2^24: every
// observation is in exactly one fold.  false: folds outside 2 ... 32 or fold outside 0 ... folds - 1
constexpr int kHoldoutMinFolds = 2, kHoldoutMaxFolds = 32;
inline bool holdout_fold_band(int folds, int fold, uint32_t* lo, uint32_t* hi) {
  if (folds < kHoldoutMinFolds || folds > kHoldoutMaxFolds || fold < 0 || fold >= folds) return false;
  const uint64_t span = (uint64_t)1 << kHoldoutBits;
  *lo = (uint32_t)((uint64_t)fold * span / (uint64_t)folds);
  *hi = (uint32_t)((uint64_t)(fold + 1) * span / (uint64_t)folds);
  return true;
}

// The row of a lambda path a caller is given: the FIRST minimum of the scores.  The rows run from the largest lambda to the
// smallest, so a tie goes to the larger lambda.  A score that is not a number is never chosen; -1: no row has one
inline int holdout_choose(const double* scores, int rows) {
  int best = -1;
  for (int j = 0; j < rows; ++j)
    if (scores[j] == scores[j] && (best < 0 || scores[j] < scores[best])) best = j;
  return best;
}

// Whether a path stops after `rows` rows: patience n > 0 stops once the score rose n rows in a row (row j rose when its
// score is above row j - 1's); 0 never stops
inline bool holdout_patience_stop(const double* scores, int rows, int patience) {
  if (patience <= 0 || rows <= patience) return false;
  for (int j = rows - patience; j < rows; ++j)
    if (!(scores[j] > scores[j - 1])) return false;
  return true;
}

// ---- the cross-validated path (srmap_solve_lambda_path_folds): the statistics of a row over its folds, and the choice ----
// mean = (sum_f s[f]) / F added in fold order; se = sqrt(sum_f (s[f] - mean)^2 / (F - 1) / F), the standard error of that
// mean from the spread OVER THE FOLDS (not the per-pixel one S2 and n give: DESIGN.md 3.17).  One fold score that is not a
// number makes both not a number.  F >= 2
inline void holdout_fold_stats(const double* s, int folds, double* mean, double* se) {
  double sum = 0.0;
  for (int f = 0; f < folds; ++f) sum += s[f];
  const double m = sum / (double)folds;
  double ss = 0.0;
  for (int f = 0; f < folds; ++f) ss += (s[f] - m) * (s[f] - m);
  *mean = m;
  *se = std::sqrt(ss / (double)(folds - 1) / (double)folds);
}

constexpr int kLambdaRuleMin = 0, kLambdaRuleOneSe = 1;  // SRMAP_LAMBDA_RULE_MIN, SRMAP_LAMBDA_RULE_ONE_SE

// The chosen row of a cross-validated path.  *jstar: the first minimum of the means (holdout_choose).  MIN: jstar.  ONE_SE:
// the smallest j -- the largest lambda among the rows run -- with mean[j] <= mean[jstar] + se_factor * se[jstar]; jstar
// itself satisfies it, so the choice is never below jstar.  A row whose mean is not a number is neither jstar nor eligible.
// -1: no row has a mean that is a number
inline int holdout_choose_folds(const double* mean, const double* se, int rows, int rule, double se_factor, int* jstar) {
  const int best = holdout_choose(mean, rows);
  if (jstar) *jstar = best;
  if (best < 0 || rule != kLambdaRuleOneSe) return best;
  const double bar = mean[best] + se_factor * se[best];
  for (int j = 0; j < best; ++j)
    if (mean[j] <= bar) return j;  // false for a mean that is not a number
  return best;
}

// "min" / "one_se" of a command line; false: another word
inline bool holdout_parse_rule(const char* text, int* rule) {
  if (!text) return false;
  const bool mn = std::strcmp(text, "min") == 0, one = std::strcmp(text, "one_se") == 0;
  if (!mn && !one) return false;
  *rule = one ? kLambdaRuleOneSe : kLambdaRuleMin;
  return true;
}

// --lambda_se_factor of a command line: a finite number >= 0 and nothing after it; false: anything else
inline bool holdout_parse_se_factor(const char* text, double* factor) {
  if (!text || !*text || *text == ' ') return false;
  char* end = nullptr;
  const double v = std::strtod(text, &end);
  if (end == text || *end != '\0' || !(v >= 0.0 && std::isfinite(v))) return false;
  if (factor) *factor = v;
  return true;
}

// "<largest>:<ratio>:<count>" of a command line: `count` lambdas largest * ratio^j, j = 0 ... count - 1.  largest finite and
// > 0, 0 < ratio < 1, 1 <= count <= 32, nothing before, between or after the three numbers; false: malformed
inline bool holdout_parse_lambda_path(const char* text, double* largest, double* ratio, int* count) {
  if (!text || !*text || *text == ' ') return false;
  char* end = nullptr;
  const double a = std::strtod(text, &end);
  if (end == text || *end != ':') return false;
  const char* second = end + 1;
  const double r = std::strtod(second, &end);
  if (end == second || *end != ':' || *second == ' ') return false;
  const char* third = end + 1;
  const long n = std::strtol(third, &end, 10);
  if (end == third || *end != '\0' || *third == ' ' || *third == '+' || *third == '-') return false;
  if (!(a > 0.0 && std::isfinite(a)) || !(r > 0.0 && r < 1.0) || n < 1 || n > 32) return false;
  *largest = a;
  *ratio = r;
  *count = (int)n;
  return true;
}

}  // namespace srmap
