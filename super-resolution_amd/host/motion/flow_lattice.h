// FlowLatticeSequence: a displacement field per frame kept on a control lattice -- lw x lh nodes per component, `step` HR
// pixels apart, node (i, j) at HR pixel (i step, j step); the field at a pixel is the bilinear interpolant of the nodes,
// constant beyond the last node (srmap_problem_set_flow_lattice, include/srmap.h, states the rule).  The compact form of a
// FlowMotionSequence (motion/flow_motion.h) and exactly what the flow registration estimates.  No reference counterpart.
// The file is one text line `step lw lh frames` followed by the raw little-endian float64 nodes in [frames][2][lh][lw]
// order; its size is checked against the header.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "motion/flow_motion.h"
#include "util/srmap_host.h"

namespace super_resolution {

class FlowLatticeSequence {
 public:
  FlowLatticeSequence() {}
  // nodes: [K][2][lh][lw]
  FlowLatticeSequence(const std::vector<double>& nodes, const int step, const int lw, const int lh) { SetNodes(nodes, step, lw, lh); }
  void SetNodes(const std::vector<double>& nodes, const int step, const int lw, const int lh) {
    CheckShape(step, lw, lh, "flow lattice");
    const size_t frame = 2 * static_cast<size_t>(lw) * static_cast<size_t>(lh);
    if (nodes.empty() || nodes.size() % frame != 0)
      srmap_host::Fail(("flow lattice: " + std::to_string(nodes.size()) + " values are no whole number of frames of 2 x " +
                        std::to_string(lh) + " x " + std::to_string(lw)).c_str());
    nodes_ = nodes;
    step_ = step;
    lw_ = lw;
    lh_ = lh;
  }
  void LoadSequenceFromFile(const std::string& path) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) srmap_host::Fail(("Could not open file " + path).c_str());
    char line[128];
    int step = 0, lw = 0, lh = 0, frames = 0;
    char extra = 0;
    const bool header = std::fgets(line, sizeof(line), f) != nullptr &&
                        std::sscanf(line, "%d %d %d %d %c", &step, &lw, &lh, &frames, &extra) == 4;
    if (!header) {
      std::fclose(f);
      srmap_host::Fail((path + ": the first line is not `step lw lh frames`").c_str());
    }
    const long start = std::ftell(f);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f) - start;
    std::fseek(f, start, SEEK_SET);
    if (step < 1 || step > kMaxStep || lw < 2 || lh < 2 || frames < 1) {
      std::fclose(f);
      srmap_host::Fail((path + ": a lattice has a step of 1 ... 1024, at least 2 x 2 nodes and at least one frame").c_str());
    }
    if (lw > kMaxCount || lh > kMaxCount || frames > kMaxCount) {  // the product below stays inside 64 bits
      std::fclose(f);
      srmap_host::Fail((path + ": more than 2^20 nodes along an axis, or frames").c_str());
    }
    const size_t want = static_cast<size_t>(frames) * 2 * static_cast<size_t>(lw) * static_cast<size_t>(lh);
    if (bytes < 0 || static_cast<size_t>(bytes) != want * sizeof(double)) {
      std::fclose(f);
      srmap_host::Fail((path + ": " + std::to_string(bytes) + " bytes follow the header, " + std::to_string(frames) + " frames of 2 x " +
                        std::to_string(lh) + " x " + std::to_string(lw) + " float64 nodes are " + std::to_string(want * sizeof(double))).c_str());
    }
    std::vector<double> nodes(want);
    const size_t got = std::fread(nodes.data(), sizeof(double), nodes.size(), f);
    std::fclose(f);
    if (got != nodes.size()) srmap_host::Fail((path + ": short read").c_str());
    nodes_.swap(nodes);
    step_ = step;
    lw_ = lw;
    lh_ = lh;
  }
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = std::fprintf(f, "%d %d %d %d\n", step_, lw_, lh_, GetNumMotions()) > 0;
    ok = ok && std::fwrite(nodes_.data(), sizeof(double), nodes_.size(), f) == nodes_.size();
    return std::fclose(f) == 0 && ok;
  }
  bool Empty() const { return nodes_.empty(); }
  int GetStep() const { return step_; }
  int GetLatticeWidth() const { return lw_; }
  int GetLatticeHeight() const { return lh_; }
  int GetNumMotions() const {
    return nodes_.empty() ? 0 : static_cast<int>(nodes_.size() / (2 * static_cast<size_t>(lw_) * static_cast<size_t>(lh_)));
  }
  const std::vector<double>& Flat() const { return nodes_; }
  // the first n frames
  void Trim(const int n) {
    if (n < GetNumMotions()) nodes_.resize(static_cast<size_t>(n) * 2 * static_cast<size_t>(lw_) * static_cast<size_t>(lh_));
  }
  // The dense field [K][2][height][width] the kernels interpolate, in double: per pixel (x, y)
  //   cx = min(max(x / step, 0), lw - 1), xi = min(floor(cx), lw - 2), fx = cx - xi (cy, yi, fy likewise),
  //   v = (1 - fy) ((1 - fx) n[yi][xi] + fx n[yi][xi+1]) + fy ((1 - fx) n[yi+1][xi] + fx n[yi+1][xi+1])
  // in this order.  The lattice may reach at most one cell beyond the image (the domain of srmap_problem_set_flow_lattice).
  FlowMotionSequence Expand(const int width, const int height) const {
    if (nodes_.empty()) srmap_host::Fail("flow lattice: the sequence is empty");
    if (width < 1 || height < 1) srmap_host::Fail("flow lattice: the image size must be positive");
    if (static_cast<long long>(lw_ - 1) * step_ >= static_cast<long long>(width) + step_ ||
        static_cast<long long>(lh_ - 1) * step_ >= static_cast<long long>(height) + step_)
      srmap_host::Fail(("flow lattice: " + std::to_string(lw_) + " x " + std::to_string(lh_) + " nodes at step " + std::to_string(step_) +
                        " reach more than a cell beyond the " + std::to_string(width) + " x " + std::to_string(height) + " image").c_str());
    const size_t plane = static_cast<size_t>(width) * height, lplane = static_cast<size_t>(lw_) * lh_;
    const int planes = 2 * GetNumMotions();
    std::vector<double> out(plane * planes);
    for (int y = 0; y < height; ++y) {
      const double cy = std::fmin(std::fmax(static_cast<double>(y) / static_cast<double>(step_), 0.0), static_cast<double>(lh_ - 1));
      const int yi = std::min(static_cast<int>(std::floor(cy)), lh_ - 2);
      const double fy = cy - static_cast<double>(yi);
      for (int x = 0; x < width; ++x) {
        const double cx = std::fmin(std::fmax(static_cast<double>(x) / static_cast<double>(step_), 0.0), static_cast<double>(lw_ - 1));
        const int xi = std::min(static_cast<int>(std::floor(cx)), lw_ - 2);
        const double fx = cx - static_cast<double>(xi);
        for (int p = 0; p < planes; ++p) {
          const double* n = nodes_.data() + p * lplane + static_cast<size_t>(yi) * lw_ + xi;
          // volatile: every product and sum is rounded on its own (no fused multiply-add), as the kernels form them
          volatile double a = (1.0 - fx) * n[0], b = fx * n[1], c = (1.0 - fx) * n[lw_], d = fx * n[lw_ + 1];
          volatile double top = a + b, bottom = c + d;
          volatile double t = (1.0 - fy) * top, u = fy * bottom;
          out[p * plane + static_cast<size_t>(y) * width + x] = t + u;
        }
      }
    }
    return FlowMotionSequence(out, width, height);
  }

  static constexpr int kMaxStep = 1024;
  static constexpr int kMaxCount = 1 << 20;  // of lw, lh and frames in a file's header

 private:
  static void CheckShape(const int step, const int lw, const int lh, const char* what) {
    if (step < 1 || step > kMaxStep || lw < 2 || lh < 2)
      srmap_host::Fail((std::string(what) + ": a lattice has a step of 1 ... 1024 and at least 2 x 2 nodes").c_str());
  }
  std::vector<double> nodes_;
  int step_ = 0, lw_ = 0, lh_ = 0;
};

}  // namespace super_resolution
