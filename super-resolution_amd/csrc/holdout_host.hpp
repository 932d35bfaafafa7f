// holdout_host.hpp -- the host arithmetic of hold-out validation (holdout.hip, lambda_path.hip): which
// observations a hold-out keeps out of the data term, the threshold of a fraction, and the rules of the lambda path (the
// chosen row, the early stop).  Plain C++17, includes nothing of HIP: the library's host code and
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
