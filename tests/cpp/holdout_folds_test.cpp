// holdout_folds_test -- csrc/holdout_host.hpp's part for the hold-out given as a fold and for the cross-validated lambda
// path (the band test, the band of a fold, the mean and the standard error over the folds, the one-standard-error rule,
// the command line's words) in plain C++.  CPU only: includes nothing but that header and links nothing of the library
// (tests/test_holdout_folds_cpu.py).
//   holdout_folds_test                          everything against literals; prints "ok", exits 3 on a miss
//   holdout_folds_test band FOLDS FOLD          prints "lo hi", or "refused"
//   holdout_folds_test mask N FOLDS FOLD SEED   prints h of observations 0 ... N - 1 as a string of 0 / 1
//   holdout_folds_test stats S0 S1 ...          prints "mean se" (%.17g) of these fold scores ("nan" is not a number)
//   holdout_folds_test choose RULE FACTOR M0 E0 M1 E1 ...   prints "chosen jstar" of the rows (mean, se)
//   holdout_folds_test rule TEXT / factor TEXT  prints the parsed value, or "refused"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "holdout_host.hpp"

using namespace srmap;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("MISS line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static int literals() {
  uint32_t lo = 7, hi = 7;
  // the bands: integer floors, the first from 0, the last to exactly 2^24
  EXPECT(holdout_fold_band(2, 0, &lo, &hi) && lo == 0u && hi == 8388608u);
  EXPECT(holdout_fold_band(2, 1, &lo, &hi) && lo == 8388608u && hi == 16777216u);
  EXPECT(holdout_fold_band(3, 0, &lo, &hi) && lo == 0u && hi == 5592405u);
  EXPECT(holdout_fold_band(3, 1, &lo, &hi) && lo == 5592405u && hi == 11184810u);
  EXPECT(holdout_fold_band(3, 2, &lo, &hi) && lo == 11184810u && hi == 16777216u);
  EXPECT(holdout_fold_band(5, 0, &lo, &hi) && lo == 0u && hi == 3355443u);
  EXPECT(holdout_fold_band(5, 3, &lo, &hi) && lo == 10066329u && hi == 13421772u);
  EXPECT(holdout_fold_band(5, 4, &lo, &hi) && lo == 13421772u && hi == 16777216u);
  EXPECT(holdout_fold_band(7, 6, &lo, &hi) && lo == 14380470u && hi == 16777216u);
  EXPECT(holdout_fold_band(32, 31, &lo, &hi) && lo == 16252928u && hi == 16777216u);
  EXPECT(holdout_fold_band(4, 0, &lo, &hi) && lo == 0u && hi == holdout_threshold(0.25));  // fold 0 of 4 is the fraction 0.25
  lo = hi = 7;
  const int bad_pairs[][2] = {{1, 0}, {0, 0}, {33, 0}, {5, 5}, {5, -1}, {-5, 0}, {2, 2}};
  for (const auto& bad : bad_pairs) EXPECT(!holdout_fold_band(bad[0], bad[1], &lo, &hi) && lo == 7u && hi == 7u);
  // the band test against the hash's literals: hash24(12345, 1) = 0x221182, hash24(0, 1) = 0xe220a8, hash24(0, 0) = 0
  EXPECT(holdout_held_band(12345, 1, 0x221182u, 0x221183u) && !holdout_held_band(12345, 1, 0x221183u, 0x221184u));
  EXPECT(!holdout_held_band(12345, 1, 0x221181u, 0x221182u) && holdout_held_band(12345, 1, 0u, 1u << 24));
  EXPECT(holdout_held_band(0, 1, 0xe220a8u, 1u << 24) && !holdout_held_band(0, 1, 0u, 0xe220a8u));
  EXPECT(holdout_held_band(0, 0, 0u, 1u) && !holdout_held_band(0, 0, 1u, 1u << 24) && !holdout_held_band(0, 0, 0u, 0u));
  // [0, T) is the old predicate
  for (const double fraction : {0.1, 0.25, 0.5, std::ldexp(1.0, -24)})
    for (const uint64_t seed : {1ull, 2ull, 0x8000000000000005ull}) {
      const uint32_t T = holdout_threshold(fraction);
      int differ = 0;
      for (uint64_t i = 0; i < 100000; ++i) differ += holdout_held(i, seed, T) != holdout_held_band(i, seed, 0u, T);
      EXPECT(differ == 0);
    }
  // the partition: every index is in exactly one fold, and the bands meet end to start
  for (const int F : {2, 3, 5, 7, 32}) {
    uint32_t end = 0;
    for (int f = 0; f < F; ++f) {
      EXPECT(holdout_fold_band(F, f, &lo, &hi) && lo == end && hi > lo);
      end = hi;
    }
    EXPECT(end == 1u << 24);
    int wrong = 0;
    std::vector<long> size(F, 0);
    for (uint64_t i = 0; i < 100000; ++i) {
      int in = 0;
      for (int f = 0; f < F; ++f) {
        holdout_fold_band(F, f, &lo, &hi);
        if (holdout_held_band(i, 3, lo, hi)) { ++in; ++size[f]; }
      }
      wrong += in != 1;
    }
    EXPECT(wrong == 0);
    for (int f = 0; f < F; ++f) EXPECT(std::fabs((double)size[f] - 1e5 / F) <= 5.0 * std::sqrt(1e5 / F));  // five binomial sigmas
  }
  // the statistics of a row: {1, 2, 3, 4, 5} has mean 3 and sample variance 2.5, so se = sqrt(2.5 / 5)
  double mean = 0.0, se = 0.0;
  {
    const double s[] = {1.0, 2.0, 3.0, 4.0, 5.0};
    holdout_fold_stats(s, 5, &mean, &se);
    EXPECT(mean == 3.0 && se == std::sqrt(0.5));
    const double t[] = {2.0, 4.0};  // variance 2, se = sqrt(2 / 2) = 1
    holdout_fold_stats(t, 2, &mean, &se);
    EXPECT(mean == 3.0 && se == 1.0);
    const double c[] = {0.25, 0.25, 0.25};
    holdout_fold_stats(c, 3, &mean, &se);
    EXPECT(mean == 0.25 && se == 0.0);
    const double n[] = {1.0, std::nan(""), 3.0};  // one fold that is not a number: neither is the row
    holdout_fold_stats(n, 3, &mean, &se);
    EXPECT(mean != mean && se != se);
    const double o[] = {0.1, 0.2, 0.3};  // the order of the sum is the folds': ((0.1 + 0.2) + 0.3) / 3
    holdout_fold_stats(o, 3, &mean, &se);
    EXPECT(mean == ((0.1 + 0.2) + 0.3) / 3.0);
  }
  // the choice
  int js = -2;
  {
    const double m[] = {5.0, 3.4, 3.0, 3.2, 4.0}, e[] = {0.1, 0.1, 0.5, 0.1, 0.1};  // the bar is 3.5: row 1 is the first inside
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleMin, 1.0, &js) == 2 && js == 2);
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleOneSe, 1.0, &js) == 1 && js == 2);
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleOneSe, 0.5, &js) == 2 && js == 2);   // bar 3.25: nothing above row 2 is inside
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleOneSe, 4.0, &js) == 0 && js == 2);   // bar 5: row 0 is on it (<=)
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleOneSe, 0.0, &js) == holdout_choose_folds(m, e, 5, kLambdaRuleMin, 0.0, nullptr));
    EXPECT(holdout_choose_folds(m, e, 2, kLambdaRuleOneSe, 1.0, &js) == 1 && js == 1);   // the rows run: a prefix
    EXPECT(holdout_choose_folds(m, e, 0, kLambdaRuleOneSe, 1.0, &js) == -1 && js == -1);
  }
  {
    const double m[] = {3.0, 1.0, 1.0, 2.0}, e[] = {0.0, 0.0, 9.0, 0.0};  // a tie: jstar is the earlier row, and its se counts
    EXPECT(holdout_choose_folds(m, e, 4, kLambdaRuleMin, 1.0, &js) == 1 && js == 1);
    EXPECT(holdout_choose_folds(m, e, 4, kLambdaRuleOneSe, 1.0, &js) == 1 && js == 1);
  }
  {
    const double nan = std::nan("");
    const double m[] = {nan, 2.05, nan, 2.0, 2.5}, e[] = {nan, 0.1, nan, 0.1, 0.1};  // rows with a fold that is not a number
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleMin, 1.0, &js) == 3 && js == 3);
    EXPECT(holdout_choose_folds(m, e, 5, kLambdaRuleOneSe, 1.0, &js) == 1 && js == 3);   // row 0 is not eligible
    EXPECT(holdout_choose_folds(m, e, 1, kLambdaRuleOneSe, 1.0, &js) == -1 && js == -1);
    const double m2[] = {nan, nan, 2.0}, e2[] = {nan, nan, nan};  // jstar's own se is not a number: nothing else is inside
    EXPECT(holdout_choose_folds(m2, e2, 3, kLambdaRuleOneSe, 1.0, &js) == 2 && js == 2);
  }
  {
    const double m[] = {1.0, 2.0, 3.0}, e[] = {5.0, 5.0, 5.0};  // jstar at row 0: nothing lies above it
    EXPECT(holdout_choose_folds(m, e, 3, kLambdaRuleOneSe, 1.0, &js) == 0 && js == 0);
    EXPECT(holdout_choose_folds(m, e, 3, kLambdaRuleMin, 1.0, &js) == 0 && js == 0);
  }
  // the command line's words and their refusals
  {
    int rule = -1;
    EXPECT(holdout_parse_rule("min", &rule) && rule == kLambdaRuleMin);
    EXPECT(holdout_parse_rule("one_se", &rule) && rule == kLambdaRuleOneSe);
    for (const char* bad : {"", "MIN", "one-se", "onese", "one_se ", " min", "mini", "1", "one_sd"}) {
      rule = -1;
      EXPECT(!holdout_parse_rule(bad, &rule) && rule == -1);
    }
    EXPECT(!holdout_parse_rule(nullptr, &rule));
    double f = -1.0;
    EXPECT(holdout_parse_se_factor("1", &f) && f == 1.0);
    EXPECT(holdout_parse_se_factor("0", &f) && f == 0.0);
    EXPECT(holdout_parse_se_factor("0.5", &f) && f == 0.5);
    EXPECT(holdout_parse_se_factor("2e0", nullptr));
    for (const char* bad : {"", "-1", "nan", "inf", "1x", " 1", "x", "1 "}) {
      f = -1.0;
      EXPECT(!holdout_parse_se_factor(bad, &f) && f == -1.0);
    }
    EXPECT(!holdout_parse_se_factor(nullptr, &f));
  }
  if (fails) return 3;
  std::printf("ok\n");
  return 0;
}

static double score_arg(const char* s) { return std::strcmp(s, "nan") == 0 ? std::nan("") : std::strtod(s, nullptr); }

int main(int argc, char** argv) {
  if (argc == 1) return literals();
  const std::string mode = argv[1];
  if (mode == "band" && argc == 4) {
    uint32_t lo = 0, hi = 0;
    if (holdout_fold_band(std::atoi(argv[2]), std::atoi(argv[3]), &lo, &hi)) std::printf("%u %u\n", lo, hi);
    else std::printf("refused\n");
    return 0;
  }
  if (mode == "mask" && argc == 6) {
    const unsigned long long n = std::strtoull(argv[2], nullptr, 10), seed = std::strtoull(argv[5], nullptr, 10);
    uint32_t lo = 0, hi = 0;
    if (!holdout_fold_band(std::atoi(argv[3]), std::atoi(argv[4]), &lo, &hi)) return 2;
    std::string bits(n, '0');
    for (unsigned long long i = 0; i < n; ++i)
      if (holdout_held_band(i, seed, lo, hi)) bits[i] = '1';
    std::printf("%s\n", bits.c_str());
    return 0;
  }
  if (mode == "stats" && argc >= 4) {
    std::vector<double> s;
    for (int i = 2; i < argc; ++i) s.push_back(score_arg(argv[i]));
    double mean = 0.0, se = 0.0;
    holdout_fold_stats(s.data(), (int)s.size(), &mean, &se);
    std::printf("%.17g %.17g\n", mean, se);
    return 0;
  }
  if (mode == "choose" && argc >= 4 && (argc - 4) % 2 == 0) {
    int rule = 0, jstar = -1;
    if (!holdout_parse_rule(argv[2], &rule)) return 2;
    std::vector<double> m, e;
    for (int i = 4; i + 1 < argc; i += 2) {
      m.push_back(score_arg(argv[i]));
      e.push_back(score_arg(argv[i + 1]));
    }
    const int chosen = holdout_choose_folds(m.data(), e.data(), (int)m.size(), rule, std::strtod(argv[3], nullptr), &jstar);
    std::printf("%d %d\n", chosen, jstar);
    return 0;
  }
  if (mode == "rule" && argc == 3) {
    int rule = -1;
    if (holdout_parse_rule(argv[2], &rule)) std::printf("%d\n", rule);
    else std::printf("refused\n");
    return 0;
  }
  if (mode == "factor" && argc == 3) {
    double f = 0.0;
    if (holdout_parse_se_factor(argv[2], &f)) std::printf("%.17g\n", f);
    else std::printf("refused\n");
    return 0;
  }
  std::fprintf(stderr, "usage: holdout_folds_test [band FOLDS FOLD | mask N FOLDS FOLD SEED | stats S... | choose RULE FACTOR M E ... | rule TEXT | factor TEXT]\n");
  return 2;
}
