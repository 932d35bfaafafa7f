// select_host.hpp -- the arithmetic of the exact median select of |r| (residual_scale.hip): the key of a
// value, the digit schedule of the radix passes, the rank of the lower median and the pick of the bin that holds a rank.
// Plain C++17, compiles with and without a HIP compiler: the kernels and tests/cpp/residual_scale_test.cpp share this one
// copy; the checker is tests/residual_scale_restatement.py.
//
// The lower median of n values is the order statistic of 0-based rank (n - 1) / 2: an element of the input, never an
// average.  |v| as an unsigned integer -- the bit pattern with the sign bit cleared -- orders as the non-negative IEEE values
// do (-0.0 becomes 0, NaNs sort above +inf by their bits), so the select works on integers and its result does not depend
// on any order of arrival.  A pass fixes one digit of the key, most significant first: it counts, per value of the digit,
// the elements whose higher digits equal the prefix found so far, and picks the bin the remaining rank falls into.  After
// the last pass the prefix is the median's key.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SRMAP_SELECT_HD __host__ __device__ inline
#else
#define SRMAP_SELECT_HD inline
#endif

namespace srmap {

constexpr int kSelectMaxBins = 2048;      // bins of the widest digit (11 bits)
constexpr double kMadToSigma = 1.4826;    // 1 / Phi^-1(3/4): median |r| -> the standard deviation of a normal r

template <typename T>
struct SelectKey;
template <>
struct SelectKey<float> {
  typedef uint32_t type;
  static constexpr int passes = 3;  // 11 + 10 + 10 = the 31 bits below the sign
};
template <>
struct SelectKey<double> {
  typedef uint64_t type;
  static constexpr int passes = 6;  // 11 + 11 + 11 + 10 + 10 + 10 = 63
};

// the key of v: the bits of |v|
SRMAP_SELECT_HD uint32_t select_key(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, sizeof u);
  return u & 0x7fffffffu;
}
SRMAP_SELECT_HD uint64_t select_key(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof u);
  return u & 0x7fffffffffffffffull;
}
// the value of a key, as a double (exact for both types)
template <typename T>
SRMAP_SELECT_HD double select_value(uint64_t key) {
  typename SelectKey<T>::type u = (typename SelectKey<T>::type)key;
  T v;
  __builtin_memcpy(&v, &u, sizeof v);
  return (double)v;
}

// digit `pass` (0 = most significant) of a key of T: bits [shift, shift + bits)
struct SelectDigit {
  int shift, bits;
};
template <typename T>
SRMAP_SELECT_HD SelectDigit select_digit(int pass) {
  const int total = (int)sizeof(T) * 8 - 1, passes = SelectKey<T>::passes;
  const int wide = total - 10 * passes;  // this many leading digits have 11 bits, the others 10
  int shift = total;
  SelectDigit d = {0, 0};
  for (int i = 0; i <= pass; ++i) {
    d.bits = i < wide ? 11 : 10;
    shift -= d.bits;
  }
  d.shift = shift;
  return d;
}
// whether the digits of `key` above digit d equal those of `prefix` (always, for the first pass)
template <typename K>
SRMAP_SELECT_HD bool select_matches(K key, K prefix, SelectDigit d) {
  const int hb = d.shift + d.bits;
  return (key >> hb) == (prefix >> hb);
}
template <typename K>
SRMAP_SELECT_HD unsigned select_bin(K key, SelectDigit d) {
  return (unsigned)(key >> d.shift) & ((1u << d.bits) - 1u);
}

// 0-based rank of the lower median of n elements (n >= 1)
SRMAP_SELECT_HD uint64_t select_median_rank(uint64_t n) { return (n - 1) / 2; }

// The bin of counts[0 .. nbins) that holds 0-based rank *rank, and the rank within that bin left in *rank; -1 (rank
// reduced by the total) when the bins hold no more than *rank elements
template <typename C>
SRMAP_SELECT_HD int select_pick(const C* counts, int nbins, uint64_t* rank) {
  uint64_t r = *rank;
  for (int b = 0; b < nbins; ++b) {
    const uint64_t c = (uint64_t)counts[b];
    if (r < c) {
      *rank = r;
      return b;
    }
    r -= c;
  }
  *rank = r;
  return -1;
}

// prefix with digit d set to bin
template <typename K>
SRMAP_SELECT_HD K select_extend(K prefix, SelectDigit d, int bin) {
  return prefix | ((K)bin << d.shift);
}

// The Huber threshold of the scale mode SRMAP_HUBER_DELTA_MAD from the scale 1.4826 median|r| over all frames
SRMAP_SELECT_HD double select_mad_delta(double scale, double tuning, double min_delta) {
  const double d = tuning * scale;
  return d > min_delta ? d : min_delta;  // a NaN scale gives the floor
}

}  // namespace srmap
