// Shared plumbing of the C++ facade: one srmap context per process and the
// reference's error convention (a failed CHECK aborts the process with a
// message -- glog semantics; the C ABI itself never aborts).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "srmap.h"

namespace super_resolution {
namespace srmap_host {

inline srmap_ctx* Context() {
  static srmap_ctx* ctx = [] {
    srmap_ctx* c = nullptr;
    const char* dev = std::getenv("SRMAP_DEVICE");
    if (srmap_ctx_create(dev ? std::atoi(dev) : 0, &c) != SRMAP_OK) {
      std::fprintf(stderr, "Check failed: no usable MI355X / HIP device (this library has no CPU path)\n");
      std::abort();
    }
    return c;
  }();
  return ctx;
}

// CHECK-style failure of a HOST-side precondition (bad size, null image, channel mismatch): print the given
// message and abort.  Does not touch the GPU context, so argument errors read the same on a box without a device.
[[noreturn]] inline void Fail(const char* what) {
  std::fprintf(stderr, "Check failed: %s\n", what);
  std::abort();
}

// CHECK-style on the status of a LIBRARY call: abort with the library's message.
inline void Check(int status, const char* what) {
  if (status == SRMAP_OK) return;
  std::fprintf(stderr, "Check failed: %s: %s (srmap status %d)\n", what, srmap_last_error(Context()), status);
  std::abort();
}

struct ProblemDeleter {
  void operator()(srmap_problem* p) const { srmap_problem_destroy(p); }
};
using ProblemPtr = std::unique_ptr<srmap_problem, ProblemDeleter>;

// Entries of a blur-kernel bank of `mode` (srmap_blur_bank_mode) over the given frames and channels.
inline size_t BankEntryCount(const int mode, const int frames, const int channels) {
  return mode == SRMAP_BLUR_PER_FRAME ? static_cast<size_t>(frames)
         : mode == SRMAP_BLUR_PER_CHANNEL ? static_cast<size_t>(channels) : static_cast<size_t>(frames) * channels;
}

// Parameters of one operator chain  D(scale) . B(ksize, sigma | free-form taps) . M(shifts | matrices | displacement fields).
struct ChainParams {
  int scale = 1;
  std::vector<double> shifts_xy;  // empty = no translational MotionModule
  std::vector<double> affine_2x3;  // K x [a b tx; c d ty]: a MotionModule over an AffineMotionSequence (then shifts_xy is empty)
  // K x 2 x flow_height x flow_width: a MotionModule over a FlowMotionSequence (then shifts_xy and affine_2x3 are empty);
  // the HR image a chain is applied to must have that size
  std::vector<double> flow;
  int flow_width = 0, flow_height = 0;
  int frames = 1;
  int blur_ksize = 0;
  double blur_sigma = 0.0;
  std::vector<double> blur_taps;  // blur_taps_ksize^2 taps of a free-form kernel (then blur_ksize / blur_sigma are unused); empty = the Gaussian
  int blur_taps_ksize = 0;
  // a blur-kernel bank (srmap_problem_set_blur_bank; then the three blur members above are unused): the mode (0 = none),
  // its kernel size and entries x blur_bank_ksize^2 taps
  int blur_bank_mode = 0, blur_bank_ksize = 0;
  std::vector<double> blur_bank;
  bool BankPerFrame() const { return blur_bank_mode == SRMAP_BLUR_PER_FRAME || blur_bank_mode == SRMAP_BLUR_PER_FRAME_CHANNEL; }
  size_t BankEntries() const { return blur_bank_mode ? blur_bank.size() / (static_cast<size_t>(blur_bank_ksize) * blur_bank_ksize) : 0; }
  bool HasMotion() const { return !shifts_xy.empty() || !affine_2x3.empty() || !flow.empty(); }
  size_t FlowFrame() const { return 2 * static_cast<size_t>(flow_width) * static_cast<size_t>(flow_height); }
  int NumMotions() const {
    if (!flow.empty()) return static_cast<int>(flow.size() / FlowFrame());
    return static_cast<int>(affine_2x3.empty() ? shifts_xy.size() / 2 : affine_2x3.size() / 6);
  }
  // solvers: n observations need at least n motions; the rest is dropped
  void TrimMotions(size_t n) {
    if (!shifts_xy.empty()) shifts_xy.resize(2 * n);
    if (!affine_2x3.empty()) affine_2x3.resize(6 * n);
    if (!flow.empty()) flow.resize(FlowFrame() * n);
    // a per-frame bank with more entries than observations: the first n (a per-(frame, channel) bank must fit as given)
    if (blur_bank_mode == SRMAP_BLUR_PER_FRAME && BankEntries() > n) blur_bank.resize(n * static_cast<size_t>(blur_bank_ksize) * blur_bank_ksize);
  }
};

inline ProblemPtr MakeProblem(const ChainParams& c, int width, int height, int channels) {
  srmap_problem_desc d;
  d.hr_width = width; d.hr_height = height; d.channels = channels;
  if (!c.shifts_xy.empty() && !c.affine_2x3.empty()) Fail("a chain has either motion shifts or affine motions, not both");
  if (!c.flow.empty() && (!c.shifts_xy.empty() || !c.affine_2x3.empty()))
    Fail("a chain has either a flow motion or motion shifts / affine motions, not both");
  if (!c.flow.empty() && (c.flow_width != width || c.flow_height != height))
    Fail(("the flow motion is given for a " + std::to_string(c.flow_width) + " x " + std::to_string(c.flow_height) +
          " high-resolution image, the model is applied at " + std::to_string(width) + " x " + std::to_string(height)).c_str());
  d.frames = c.HasMotion() ? c.NumMotions() : c.frames;
  const bool bank = c.blur_bank_mode != 0;
  if (bank) {
    // a chain without motion and without a frame count takes its frames from a per-frame bank
    const int per_frame = c.blur_bank_mode == SRMAP_BLUR_PER_FRAME_CHANNEL ? channels : 1;
    if (!c.HasMotion() && c.frames <= 1 && c.BankPerFrame()) d.frames = static_cast<int>(c.BankEntries()) / per_frame;
    const size_t want = BankEntryCount(c.blur_bank_mode, d.frames, channels);
    if (c.BankEntries() != want)
      Fail(("the blur bank holds " + std::to_string(c.BankEntries()) + " entries, the model has " + std::to_string(d.frames) + " frames and " +
            std::to_string(channels) + " channels: its mode " + std::to_string(c.blur_bank_mode) + " needs " + std::to_string(want)).c_str());
  }
  d.scale = c.scale;
  d.shifts_xy = c.shifts_xy.empty() ? nullptr : c.shifts_xy.data();
  const bool gaussian = c.blur_taps.empty() && !bank;
  d.blur_ksize = gaussian ? c.blur_ksize : 0; d.blur_sigma = gaussian ? c.blur_sigma : 0.0;
  d.dtype = SRMAP_F64;  // the reference computes in double
  srmap_problem* p = nullptr;
  Check(srmap_problem_create(Context(), &d, &p), "srmap_problem_create");
  ProblemPtr problem(p);
  if (!c.affine_2x3.empty())
    Check(srmap_problem_set_affine_motion(p, c.affine_2x3.data()), "srmap_problem_set_affine_motion");
  if (!c.flow.empty()) Check(srmap_problem_set_flow(p, c.flow.data()), "srmap_problem_set_flow");
  if (bank)
    Check(srmap_problem_set_blur_bank(p, c.blur_bank_mode, c.blur_bank_ksize, c.blur_bank.data()), "srmap_problem_set_blur_bank");
  else if (!c.blur_taps.empty())
    Check(srmap_problem_set_blur_kernel(p, c.blur_taps_ksize, c.blur_taps.data()), "srmap_problem_set_blur_kernel");
  return problem;
}

}  // namespace srmap_host
}  // namespace super_resolution
