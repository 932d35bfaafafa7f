// FlowMotionSequence: a dense displacement field per frame, (ux, uy) in HR pixels on the frame's HR-grid image -- frame k
// at pixel q is the HR image sampled bilinearly at q + u_k(q) (MotionShift (dx, dy) is u = (-dx, -dy) everywhere).  No
// reference counterpart (its MotionModule warps by a MotionShift only, motion_module.cpp:18-51).  The file is raw
// little-endian float64 in [K][2][H][W] order, no header: its size is checked against the geometry the caller states, and
// K is what the size leaves.  The field goes to srmap_problem_set_flow (include/srmap.h), which states and verifies the
// domain.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "util/srmap_host.h"

namespace super_resolution {

class FlowMotionSequence {
 public:
  FlowMotionSequence() {}
  // flow: [K][2][height][width]
  FlowMotionSequence(const std::vector<double>& flow, const int width, const int height) { SetFlow(flow, width, height); }
  void SetFlow(const std::vector<double>& flow, const int width, const int height) {
    if (width < 1 || height < 1) srmap_host::Fail("flow motion: the image size must be positive");
    const size_t frame = 2 * static_cast<size_t>(width) * static_cast<size_t>(height);
    if (flow.empty() || flow.size() % frame != 0)
      srmap_host::Fail(("flow motion: " + std::to_string(flow.size()) + " values are no whole number of frames of 2 x " +
                        std::to_string(height) + " x " + std::to_string(width)).c_str());
    flow_ = flow;
    width_ = width;
    height_ = height;
  }
  // the file must hold K x 2 x height x width float64 values for some K >= 1
  void LoadSequenceFromFile(const std::string& path, const int width, const int height) {
    if (width < 1 || height < 1) srmap_host::Fail("flow motion: the image size must be positive");
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) srmap_host::Fail(("Could not open file " + path).c_str());
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    const size_t frame_bytes = 2 * static_cast<size_t>(width) * static_cast<size_t>(height) * sizeof(double);
    if (bytes <= 0 || static_cast<size_t>(bytes) % frame_bytes != 0) {
      std::fclose(f);
      srmap_host::Fail((path + ": " + std::to_string(bytes) + " bytes are no whole number of frames of 2 x " + std::to_string(height) +
                        " x " + std::to_string(width) + " float64 values (" + std::to_string(frame_bytes) + " bytes each)").c_str());
    }
    std::vector<double> flow(static_cast<size_t>(bytes) / sizeof(double));
    const size_t got = std::fread(flow.data(), sizeof(double), flow.size(), f);
    std::fclose(f);
    if (got != flow.size()) srmap_host::Fail((path + ": short read").c_str());
    flow_.swap(flow);
    width_ = width;
    height_ = height;
  }
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(flow_.data(), sizeof(double), flow_.size(), f) == flow_.size();
    return std::fclose(f) == 0 && ok;
  }
  bool Empty() const { return flow_.empty(); }
  int GetWidth() const { return width_; }
  int GetHeight() const { return height_; }
  int GetNumMotions() const {
    return flow_.empty() ? 0 : static_cast<int>(flow_.size() / (2 * static_cast<size_t>(width_) * static_cast<size_t>(height_)));
  }
  // (ux, uy) of frame `index` at pixel (x, y)
  void GetDisplacement(const int index, const int x, const int y, double* ux, double* uy) const {
    if (index < 0 || index >= GetNumMotions()) srmap_host::Fail("flow motion index out of range");
    if (x < 0 || x >= width_ || y < 0 || y >= height_) srmap_host::Fail("flow motion pixel out of range");
    const size_t plane = static_cast<size_t>(width_) * height_, at = static_cast<size_t>(y) * width_ + x;
    if (ux) *ux = flow_[(2 * static_cast<size_t>(index)) * plane + at];
    if (uy) *uy = flow_[(2 * static_cast<size_t>(index) + 1) * plane + at];
  }
  void CheckIndex(const int index) const {
    if (index < 0 || index >= GetNumMotions()) srmap_host::Fail("flow motion index out of range");
  }
  const std::vector<double>& Flat() const { return flow_; }

 private:
  std::vector<double> flow_;
  int width_ = 0, height_ = 0;
};

}  // namespace super_resolution
