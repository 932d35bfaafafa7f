// BlurKernel: a free-form point-spread function for BlurModule -- ksize x ksize taps, row-major, ksize odd.  It stands in
// for the square odd cv::Mat a caller of the reference would hand to a blur; the forward model correlates with it and the
// transpose uses its flip in both axes (srmap_problem_set_blur_kernel, include/srmap.h, which states the domain).  No
// reference counterpart: BlurModule there builds a Gaussian from (radius, sigma) only (blur_module.cpp:13-22).  Loadable
// from a text file: the first number is ksize, then ksize * ksize numbers in row-major order, separated by any white space
// (a reader of its own, written as AffineMotionSequence's is, motion/affine_motion.h).
#pragma once
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "util/srmap_host.h"

namespace super_resolution {

class BlurKernel {
 public:
  BlurKernel() {}
  BlurKernel(const int ksize, const std::vector<double>& taps) : ksize_(ksize), taps_(taps) {
    if (ksize < 1 || ksize % 2 != 1) srmap_host::Fail("BlurKernel: the size must be odd and >= 1");
    if (taps.size() != static_cast<size_t>(ksize) * ksize) srmap_host::Fail("BlurKernel: expected ksize * ksize taps");
  }
  void LoadFromFile(const std::string& path) {
    std::ifstream fin(path);
    if (!fin.is_open()) srmap_host::Fail(("Could not open file " + path).c_str());
    double size = 0.0;
    if (!(fin >> size) || size < 1.0 || size != std::floor(size) || static_cast<int>(size) % 2 != 1 || size > 99.0)
      srmap_host::Fail((path + ": expected an odd kernel size first").c_str());
    const int ksize = static_cast<int>(size);
    std::vector<double> taps(static_cast<size_t>(ksize) * ksize);
    for (size_t i = 0; i < taps.size(); ++i)
      if (!(fin >> taps[i]))
        srmap_host::Fail((path + ": expected " + std::to_string(taps.size()) + " taps after the size, read " + std::to_string(i)).c_str());
    std::string rest;
    if (fin >> rest) srmap_host::Fail((path + ": more than " + std::to_string(taps.size()) + " taps after the size").c_str());
    ksize_ = ksize;
    taps_.swap(taps);
  }
  // the same format, one kernel row per line, every tap with 17 significant digits (it loads again bit for bit)
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "%d\n", ksize_);
    for (int a = 0; a < ksize_; ++a)
      for (int e = 0; e < ksize_; ++e) std::fprintf(f, "%.17g%c", taps_[static_cast<size_t>(a) * ksize_ + e], e + 1 < ksize_ ? ' ' : '\n');
    return std::fclose(f) == 0;
  }
  bool Empty() const { return taps_.empty(); }
  int GetSize() const { return ksize_; }
  const std::vector<double>& GetTaps() const { return taps_; }
  double operator()(const int row, const int col) const {
    if (row < 0 || row >= ksize_ || col < 0 || col >= ksize_) srmap_host::Fail("blur kernel index out of range");
    return taps_[static_cast<size_t>(row) * ksize_ + col];
  }

 private:
  int ksize_ = 0;
  std::vector<double> taps_;
};

}  // namespace super_resolution
