// reg_gradient_host.hpp -- the host arithmetic of the regularisers' gradient mode (srmap_problem_set_regularizer_gradient):
// the word a command line names a mode by, and the rule that sends an exact BTV gradient to k_btv_gradient_exact4.  Plain
// C++, no HIP: tests/cpp/reg_exact_test.cpp compiles it alone.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace srmap {

constexpr int kRegGradientReference = 0, kRegGradientExact = 1;  // srmap_reg_gradient (include/srmap.h)

// "reference" | "exact" -> the mode; any other text (a prefix, another case, an empty or null one): false, *mode untouched
inline bool reg_gradient_parse(const char* text, int* mode) {
  if (text == nullptr) return false;
  int m;
  if (std::strcmp(text, "reference") == 0) m = kRegGradientReference;
  else if (std::strcmp(text, "exact") == 0) m = kRegGradientExact;
  else return false;
  if (mode) *mode = m;
  return true;
}

inline const char* reg_gradient_name(int mode) {
  return mode == kRegGradientReference ? "reference" : mode == kRegGradientExact ? "exact" : nullptr;
}

// k_btv_gradient_exact4 (kernels_reg_direct.hip): four consecutive pixels per thread, 4-element vector requests.  It serves
// ranges 1 .. 3 on whole cells (W % 4 == 0) whose count fits the kernel's 32-bit cell index, given the values, when every
// array starts on a 4-element boundary (elem = sizeof of the dtype; g and gc may be null); else the Exact leg of
// k_reg_gradient_direct runs.
inline bool btv_exact4_serves(int range, int W, int H, size_t elem, uintptr_t x, uintptr_t values, uintptr_t gc, uintptr_t g) {
  if (range < 1 || range > 3 || W < 4 || H < 1 || (W & 3) != 0 || values == 0 || x == 0) return false;
  if ((long long)W * H / 4 >= (long long)INT_MAX) return false;
  const uintptr_t align = 4 * elem;
  return x % align == 0 && values % align == 0 && gc % align == 0 && g % align == 0;
}

}  // namespace srmap
