// Photometric / PhotometricSequence: per-frame gain and bias of the photometric frame model -- frame k shows
// gain_k * (D B M_k x) + bias_k, one pair per frame shared by all channels, the bias in the solver's pixel units (ImageData
// scales 8-bit input to 0..1).  No reference counterpart: there every frame has the photometry of the HR image
// (image_model.cpp:86-91).  The pairs go to srmap_problem_set_photometric (include/srmap.h), which states the domain.
// Loadable from a text file of "gain bias" lines (AffineMotionSequence's line reader, util/number_file.h).
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "image/image_data.h"
#include "util/number_file.h"
#include "util/srmap_host.h"

namespace super_resolution {

struct Photometric {
  Photometric(const double gain, const double bias) : gain(gain), bias(bias) {}
  double gain, bias;
};

class PhotometricSequence {
 public:
  PhotometricSequence() {}
  explicit PhotometricSequence(const std::vector<Photometric>& frames) : frames_(frames) {}
  // K x 2 numbers {gain, bias}, as the C ABI holds them
  PhotometricSequence(const double* gain_bias, const int num_frames) {
    for (int i = 0; i < num_frames; ++i) frames_.push_back(Photometric(gain_bias[2 * i], gain_bias[2 * i + 1]));
  }
  // one frame per line, two numbers; blank lines are skipped, anything else is an error
  void LoadSequenceFromFile(const std::string& path) {
    frames_.clear();
    srmap_host::ReadNumberLines(path, 2, "two numbers 'gain bias'", [this](const double* v, const std::string& where) {
      if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !(v[0] > 0.0))
        srmap_host::Fail((where + ": the gain must be > 0 and both numbers finite").c_str());
      frames_.push_back(Photometric(v[0], v[1]));
    });
  }
  // the same format, every number with 17 significant digits (it loads again bit for bit)
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    for (const Photometric& p : frames_) std::fprintf(f, "%.17g %.17g\n", p.gain, p.bias);
    return std::fclose(f) == 0;
  }
  int GetNumFrames() const { return static_cast<int>(frames_.size()); }
  bool Empty() const { return frames_.empty(); }
  const Photometric& GetPhotometric(const int index) const {
    if (index < 0 || index >= GetNumFrames()) srmap_host::Fail("photometric index out of range");
    return frames_[index];
  }
  const Photometric& operator[](const int index) const { return GetPhotometric(index); }
  std::vector<double> Flat() const {
    std::vector<double> f;
    for (const Photometric& p : frames_) { f.push_back(p.gain); f.push_back(p.bias); }
    return f;
  }
  // data generation: pixel <- gain * pixel + bias on every channel of frame `index` (before any noise is added)
  void ApplyToImage(ImageData* image_data, const int index) const {
    if (!image_data) srmap_host::Fail("CHECK_NOTNULL(image_data)");
    const Photometric& p = GetPhotometric(index);
    for (int c = 0; c < image_data->GetNumChannels(); ++c) {
      double* px = image_data->GetMutableChannelData(c);
      for (int i = 0; i < image_data->GetNumPixels(); ++i) px[i] = p.gain * px[i] + p.bias;
    }
  }

 private:
  std::vector<Photometric> frames_;
};

}  // namespace super_resolution
