// residual_scale_test -- csrc/select_host.hpp (the key, the digit schedule and the bin pick of the exact median select)
// in plain C++ against std::nth_element.  CPU only: includes nothing but that header and links nothing of the library
// (tests/test_residual_scale_cpu.py).  Reads cases on stdin:
//   f32|f64 n  then n pairs  <bit pattern, hex> <mask, 0 or 1>
// runs the digit passes over the counted elements, and prints per case
//   <key of the lower median of |v|, hex> <n counted> <1.4826 * median, %a> <delta for tuning 1.345, floor 1e-4, %a>
// It exits with 3 when the passes disagree with std::nth_element on the keys, or when the result is not the order
// statistic of rank (n - 1) / 2 of the VALUES |v| (checked by counting, on cases without a NaN).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "select_host.hpp"

using namespace srmap;

template <typename T>
static int run_case(const std::vector<unsigned long long>& bits, const std::vector<int>& mask) {
  typedef typename SelectKey<T>::type K;
  std::vector<K> keys;
  std::vector<T> vals;
  bool any_nan = false;
  for (size_t i = 0; i < bits.size(); ++i) {
    if (!mask[i]) continue;
    const K u = (K)bits[i];
    T v;
    std::memcpy(&v, &u, sizeof v);
    keys.push_back(select_key(v));
    vals.push_back(std::fabs(v));
    any_nan = any_nan || std::isnan(v);
  }
  const uint64_t n = keys.size();
  if (n == 0) {
    std::printf("0 0 %a %a\n", 0.0, select_mad_delta(0.0, 1.345, 1e-4));
    return 0;
  }
  uint64_t rank = select_median_rank(n);
  K prefix = 0;
  for (int pass = 0; pass < SelectKey<T>::passes; ++pass) {
    const SelectDigit d = select_digit<T>(pass);
    if (d.bits > 11 || d.shift < 0 || (1 << d.bits) > kSelectMaxBins) return 3;
    std::vector<unsigned> hist((size_t)1 << d.bits, 0u);
    for (K key : keys)
      if (select_matches(key, prefix, d)) hist[select_bin(key, d)]++;
    const int bin = select_pick(hist.data(), (int)hist.size(), &rank);
    if (bin < 0) return 3;
    prefix = select_extend(prefix, d, bin);
    if (pass == SelectKey<T>::passes - 1 && d.shift != 0) return 3;
  }
  std::vector<K> sorted(keys);
  const uint64_t r = select_median_rank(n);
  std::nth_element(sorted.begin(), sorted.begin() + r, sorted.end());
  if (sorted[r] != prefix) return 3;
  const double med = select_value<T>(prefix);
  if (!any_nan) {
    uint64_t below = 0, upto = 0;
    for (T v : vals) {
      below += (double)v < med;
      upto += (double)v <= med;
    }
    if (!(below <= r && r < upto)) return 3;
  }
  const double scale = kMadToSigma * med;
  std::printf("%llx %llu %a %a\n", (unsigned long long)prefix, (unsigned long long)n, scale, select_mad_delta(scale, 1.345, 1e-4));
  return 0;
}

int main() {
  char what[8];
  long long n = 0;
  while (std::scanf("%7s %lld", what, &n) == 2) {
    if (n < 0) return 2;
    std::vector<unsigned long long> bits((size_t)n);
    std::vector<int> mask((size_t)n);
    for (long long i = 0; i < n; ++i)
      if (std::scanf("%llx %d", &bits[i], &mask[i]) != 2) return 2;
    int rc = 2;
    if (std::strcmp(what, "f32") == 0) rc = run_case<float>(bits, mask);
    else if (std::strcmp(what, "f64") == 0) rc = run_case<double>(bits, mask);
    if (rc) return rc;
  }
  return 0;
}
