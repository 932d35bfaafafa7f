// The text formats of the facade's own files, read and written once: one record of numbers per line (AffineMotionSequence,
// PhotometricSequence) and a header followed by kernel taps (BlurKernel, BlurKernelBank).  Every error names the file.
#pragma once
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "util/srmap_host.h"

namespace super_resolution {
namespace srmap_host {

// One record of `count` numbers per line; blank lines are skipped, anything else is an error "<path> line <n>: expected
// <what>".  each(values, where) takes every record in file order, with where = "<path> line <n>" for its own checks.
template <class Each>
inline void ReadNumberLines(const std::string& path, const int count, const char* what, Each each) {
  std::ifstream fin(path);
  if (!fin.is_open()) Fail(("Could not open file " + path).c_str());
  std::string line;
  int number = 0;
  while (std::getline(fin, line)) {
    ++number;
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    const std::string where = path + " line " + std::to_string(number);
    std::istringstream in(line);
    std::vector<double> values(count);
    std::string rest;
    bool complete = true;
    for (int i = 0; i < count && complete; ++i) complete = static_cast<bool>(in >> values[i]);
    if (!complete || (in >> rest)) Fail((where + ": expected " + what).c_str());
    each(values.data(), where);
  }
}

// Exactly n taps up to the end of the file, which `after` ("the size", "the header") precedes.
inline std::vector<double> ReadTaps(std::ifstream& fin, const std::string& path, const size_t n, const std::string& after) {
  std::vector<double> taps(n);
  for (size_t i = 0; i < n; ++i)
    if (!(fin >> taps[i]))
      Fail((path + ": expected " + std::to_string(n) + " taps after " + after + ", read " + std::to_string(i)).c_str());
  std::string rest;
  if (fin >> rest) Fail((path + ": more than " + std::to_string(n) + " taps after " + after).c_str());
  return taps;
}

// One ksize x ksize kernel, a row per line, every tap with 17 significant digits (it loads again bit for bit).
inline void WriteKernelRows(std::FILE* f, const double* taps, const int ksize) {
  for (int a = 0; a < ksize; ++a)
    for (int e = 0; e < ksize; ++e) std::fprintf(f, "%.17g%c", taps[static_cast<size_t>(a) * ksize + e], e + 1 < ksize ? ' ' : '\n');
}

}  // namespace srmap_host
}  // namespace super_resolution
