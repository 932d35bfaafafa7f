// BlurKernel: a free-form point-spread function for BlurModule -- ksize x ksize taps, row-major, ksize odd.  It stands in
// for the square odd cv::Mat a caller of the reference would hand to a blur; the forward model correlates with it and the
// transpose uses its flip in both axes (srmap_problem_set_blur_kernel, include/srmap.h, which states the domain).  No
// reference counterpart: BlurModule there builds a Gaussian from (radius, sigma) only (blur_module.cpp:13-22).  Loadable
// from a text file: the first number is ksize, then ksize * ksize numbers in row-major order, separated by any white space
// (the taps reader and row writer it shares with BlurKernelBank are in util/number_file.h).
#pragma once
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "util/number_file.h"
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
    taps_ = srmap_host::ReadTaps(fin, path, static_cast<size_t>(ksize) * ksize, "the size");
    ksize_ = ksize;
  }
  // the same format, one kernel row per line, every tap with 17 significant digits (it loads again bit for bit)
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "%d\n", ksize_);
    srmap_host::WriteKernelRows(f, taps_.data(), ksize_);
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

// BlurKernelBank: a point-spread function per frame (mode 1), per channel (2) or per (frame, channel) (3, stored [k][c]) --
// srmap_problem_set_blur_bank, include/srmap.h, whose srmap_blur_bank_mode the mode is.  One ksize for the bank: a smaller
// kernel goes in zero-padded (Padded()).  Text file: the three integers `mode ksize entries`, then entries * ksize * ksize
// taps, entry by entry in row-major order, separated by any white space.  No reference counterpart.
class BlurKernelBank {
 public:
  BlurKernelBank() {}
  BlurKernelBank(const int mode, const int ksize, const int entries, const std::vector<double>& taps)
      : mode_(mode), ksize_(ksize), entries_(entries), taps_(taps) {
    if (mode < 1 || mode > 3) srmap_host::Fail("BlurKernelBank: the mode is 1 (per frame), 2 (per channel) or 3 (per frame and channel)");
    if (ksize < 1 || ksize % 2 != 1) srmap_host::Fail("BlurKernelBank: the size must be odd and >= 1");
    if (entries < 1) srmap_host::Fail("BlurKernelBank: at least one entry is needed");
    if (taps.size() != static_cast<size_t>(entries) * ksize * ksize) srmap_host::Fail("BlurKernelBank: expected entries * ksize * ksize taps");
  }
  // a bank of the given mode from kernels of any odd sizes: each zero-padded to the largest
  static BlurKernelBank Padded(const int mode, const std::vector<BlurKernel>& kernels) {
    int ksize = 1;
    for (const BlurKernel& k : kernels) ksize = k.GetSize() > ksize ? k.GetSize() : ksize;
    std::vector<double> taps(kernels.size() * static_cast<size_t>(ksize) * ksize, 0.0);
    for (size_t q = 0; q < kernels.size(); ++q) {
      if (kernels[q].Empty()) srmap_host::Fail("BlurKernelBank: an entry is empty");
      const int b = kernels[q].GetSize(), off = (ksize - b) / 2;
      for (int a = 0; a < b; ++a)
        for (int e = 0; e < b; ++e) taps[(q * ksize + a + off) * ksize + e + off] = kernels[q](a, e);
    }
    return BlurKernelBank(mode, ksize, static_cast<int>(kernels.size()), taps);
  }
  void LoadFromFile(const std::string& path) {
    std::ifstream fin(path);
    if (!fin.is_open()) srmap_host::Fail(("Could not open file " + path).c_str());
    double mode = 0.0, size = 0.0, entries = 0.0;
    if (!(fin >> mode) || mode != std::floor(mode) || mode < 1.0 || mode > 3.0)
      srmap_host::Fail((path + ": expected the bank mode 1, 2 or 3 first").c_str());
    if (!(fin >> size) || size < 1.0 || size != std::floor(size) || static_cast<int>(size) % 2 != 1 || size > 99.0)
      srmap_host::Fail((path + ": expected an odd kernel size after the mode").c_str());
    if (!(fin >> entries) || entries < 1.0 || entries != std::floor(entries) || entries > 1.0e6)
      srmap_host::Fail((path + ": expected the number of entries after the size").c_str());
    taps_ = srmap_host::ReadTaps(fin, path, static_cast<size_t>(entries) * static_cast<size_t>(size) * static_cast<size_t>(size), "the header");
    mode_ = static_cast<int>(mode);
    ksize_ = static_cast<int>(size);
    entries_ = static_cast<int>(entries);
  }
  // the same format, one kernel row per line, a blank line between entries, 17 significant digits (it loads again bit for bit)
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "%d %d %d\n", mode_, ksize_, entries_);
    for (int q = 0; q < entries_; ++q) {
      srmap_host::WriteKernelRows(f, taps_.data() + static_cast<size_t>(q) * ksize_ * ksize_, ksize_);
      if (q + 1 < entries_) std::fprintf(f, "\n");
    }
    return std::fclose(f) == 0;
  }
  bool Empty() const { return taps_.empty(); }
  int GetMode() const { return mode_; }
  int GetSize() const { return ksize_; }
  int GetNumEntries() const { return entries_; }
  const std::vector<double>& GetTaps() const { return taps_; }
  BlurKernel Entry(const int q) const {
    if (q < 0 || q >= entries_) srmap_host::Fail("blur bank entry out of range");
    const size_t bb = static_cast<size_t>(ksize_) * ksize_;
    return BlurKernel(ksize_, std::vector<double>(taps_.begin() + q * bb, taps_.begin() + (q + 1) * bb));
  }

 private:
  int mode_ = 0, ksize_ = 0, entries_ = 0;
  std::vector<double> taps_;
};

}  // namespace super_resolution
