// holdout_test -- csrc/holdout_host.hpp (the index hash of the hold-out, the threshold of a fraction, the chosen row and
// the early stop of the lambda path) in plain C++.  CPU only: includes nothing but that header and links nothing of the
// library (tests/test_holdout_host.py).
//   holdout_test                       the hash, the threshold and the rules against literals; prints "ok", exits 3 on a miss
//   holdout_test mask N FRACTION SEED  prints T, then h of observations 0 ... N - 1 as a string of 0 / 1
//   holdout_test choose S0 S1 ...      prints the chosen row of these scores ("nan" is a score that is not a number)
//   holdout_test stop PATIENCE S0 ...  prints, per prefix of the scores, whether the path stops after it (0 / 1)
//   holdout_test triple TEXT           prints "largest ratio count" (%.17g) of a --lambda_path value, or "refused"
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
  // the mix: splitmix64's first output from state 0 is the published 0xe220a8397b1dcdaf
  EXPECT(holdout_hash(0, 0) == 0x0ull);
  EXPECT(holdout_hash(0, 1) == 0xe220a8397b1dcdafull);
  EXPECT(holdout_hash(1, 1) == 0x910a2dec89025cc1ull);
  EXPECT(holdout_hash(12345, 1) == 0x22118258a9d111a0ull);
  EXPECT(holdout_hash(4294967303ull, 2) == 0xecb65194b1e2b74eull);  // an index past 2^32
  EXPECT(holdout_hash(9223372036854775808ull, 0xFFFFFFFFFFFFFFFFull) == 0xf768bd32e7db96ebull);  // wraps mod 2^64
  EXPECT(holdout_hash(18431, 1) == 0xaaf47178f405b877ull);
  // the threshold
  EXPECT(holdout_threshold(0.1) == 1677721u);
  EXPECT(holdout_threshold(0.5) == 8388608u);
  EXPECT(holdout_threshold(std::ldexp(1.0, -24)) == 1u);
  EXPECT(holdout_threshold(std::ldexp(1.0, -25)) == 0u);  // nothing could be held out
  EXPECT(holdout_threshold(0.0) == 0u && holdout_threshold(-0.1) == 0u && holdout_threshold(0.6) == 0u);
  EXPECT(holdout_threshold(std::nan("")) == 0u && holdout_threshold(INFINITY) == 0u);
  // held: the top 24 bits against T
  EXPECT(holdout_held(0, 0, 1u));              // hash 0: below every T >= 1
  EXPECT(!holdout_held(0, 1, 8388608u));       // top bits 0xe220a8 >= 0x800000
  EXPECT(holdout_held(12345, 1, 0x221183u) && !holdout_held(12345, 1, 0x221182u));
  {  // 6 x 1 x 48 x 64 at 10 %, seed 1: 1867 of 18432
    int n = 0;
    for (uint64_t i = 0; i < 18432; ++i) n += holdout_held(i, 1, holdout_threshold(0.1));
    EXPECT(n == 1867);
  }
  // the chosen row: the first minimum, a tie to the earlier row (the larger lambda), a NaN never
  {
    const double a[] = {3.0, 2.0, 1.0, 1.0, 2.0};
    EXPECT(holdout_choose(a, 5) == 2);
    EXPECT(holdout_choose(a, 1) == 0);
    const double b[] = {std::nan(""), 5.0, std::nan(""), 4.0};
    EXPECT(holdout_choose(b, 4) == 3 && holdout_choose(b, 1) == -1 && holdout_choose(b, 3) == 1);
    EXPECT(holdout_choose(a, 0) == -1);
  }
  // the early stop
  {
    const double s[] = {5.0, 4.0, 4.5, 4.6, 4.7};
    EXPECT(!holdout_patience_stop(s, 5, 0));
    EXPECT(!holdout_patience_stop(s, 2, 1) && holdout_patience_stop(s, 3, 1));
    EXPECT(!holdout_patience_stop(s, 3, 2) && holdout_patience_stop(s, 4, 2));
    EXPECT(!holdout_patience_stop(s, 4, 4) && !holdout_patience_stop(s, 5, 4));  // row 1 fell
    const double t[] = {1.0, 1.0, 1.0};
    EXPECT(!holdout_patience_stop(t, 3, 1));  // equal is not a rise
  }
  // the command line's triple and its refusals
  {
    double a = 0.0, r = 0.0;
    int n = 0;
    EXPECT(holdout_parse_lambda_path("0.08:0.5:8", &a, &r, &n) && a == 0.08 && r == 0.5 && n == 8);
    EXPECT(holdout_parse_lambda_path("1e-1:.25:1", &a, &r, &n) && a == 0.1 && r == 0.25 && n == 1);
    EXPECT(holdout_parse_lambda_path("2:0.999:32", &a, &r, &n) && n == 32);
    for (const char* bad : {"", "0.08", "0.08:0.5", "0.08:0.5:", "0.08:0.5:8:1", "0.08:0.5:8x", "x:0.5:8", "0.08:x:8", "0.08;0.5;8",
                            "0:0.5:8", "-0.08:0.5:8", "inf:0.5:8", "nan:0.5:8", "0.08:1:8", "0.08:0:8", "0.08:1.5:8", "0.08:-0.5:8",
                            "0.08:0.5:0", "0.08:0.5:33", "0.08:0.5:-2", "0.08:0.5:2.5", "0.08:0.5: 8", " 0.08:0.5:8 ", " 0.08:0.5:8", "0.08: 0.5:8"}) {
      a = r = -1.0;
      n = -1;
      EXPECT(!holdout_parse_lambda_path(bad, &a, &r, &n) && a == -1.0 && r == -1.0 && n == -1);
    }
    EXPECT(!holdout_parse_lambda_path(nullptr, &a, &r, &n));
  }
  if (fails) return 3;
  std::printf("ok\n");
  return 0;
}

static double score_arg(const char* s) { return std::strcmp(s, "nan") == 0 ? std::nan("") : std::strtod(s, nullptr); }

int main(int argc, char** argv) {
  if (argc == 1) return literals();
  const std::string mode = argv[1];
  if (mode == "mask" && argc == 5) {
    const unsigned long long n = std::strtoull(argv[2], nullptr, 10), seed = std::strtoull(argv[4], nullptr, 10);
    const uint32_t T = holdout_threshold(std::strtod(argv[3], nullptr));
    std::printf("%u\n", T);
    std::string bits(n, '0');
    for (unsigned long long i = 0; i < n; ++i)
      if (holdout_held(i, seed, T)) bits[i] = '1';
    std::printf("%s\n", bits.c_str());
    return 0;
  }
  if (mode == "choose" && argc >= 2) {
    std::vector<double> s;
    for (int i = 2; i < argc; ++i) s.push_back(score_arg(argv[i]));
    std::printf("%d\n", holdout_choose(s.data(), (int)s.size()));
    return 0;
  }
  if (mode == "stop" && argc >= 3) {
    const int patience = std::atoi(argv[2]);
    std::vector<double> s;
    for (int i = 3; i < argc; ++i) s.push_back(score_arg(argv[i]));
    for (size_t n = 1; n <= s.size(); ++n) std::printf("%d", holdout_patience_stop(s.data(), (int)n, patience) ? 1 : 0);
    std::printf("\n");
    return 0;
  }
  if (mode == "triple" && argc == 3) {
    double a = 0.0, r = 0.0;
    int n = 0;
    if (holdout_parse_lambda_path(argv[2], &a, &r, &n)) std::printf("%.17g %.17g %d\n", a, r, n);
    else std::printf("refused\n");
    return 0;
  }
  std::fprintf(stderr, "usage: holdout_test [mask N FRACTION SEED | choose S... | stop PATIENCE S...]\n");
  return 2;
}
