// registration::TranslationalRegistration (src/motion/registration.h:19-22, registration.cpp:161-201): shifts of a
// list of images relative to the first one, as a MotionShiftSequence.  Same signature and calling conventions as the
// reference -- NOT the same estimator: a dense pure-translation search (up to a quarter of the frame) with no
// outlier rejection, where the reference fits a feature-based RANSAC homography / rigid transform and keeps its
// translation.  Rotation, scale or periodic texture between real frames can give different (wrong) shifts without
// an error; include/srmap.h (srmap_register_translational_ex) reports a per-frame quality to check, and
// TranslationalRegistrationWithQuality below exposes it.  (channel 0 is the registration image, registration.cpp:41-46; an empty list gives an empty sequence,
// :165-168; image 0 gets (0, 0), :170-172; failure to determine a shift is a CHECK failure, :193-194).  The
// estimate itself comes from the GPU (srmap_register_translational, csrc/registration.hip) instead of the
// reference's OpenCV feature pipeline; the contract is the reference's own test (test/test_registration.cpp:
// shifts applied with MotionModule recovered to 0.01 px).
#pragma once
#include <vector>

#include "image/image_data.h"
#include "motion/affine_motion.h"
#include "motion/flow_motion.h"
#include "motion/motion_shift.h"
#include "util/srmap_host.h"

namespace super_resolution {
namespace registration {

namespace internal {
// Channel 0 of every image, stacked [images][height][width]: what the C entry points register.  The images are of one
// size with at least one channel; `images` is not empty.
inline std::vector<double> ChannelZeroStack(const std::vector<ImageData>& images, cv::Size* size) {
  *size = images[0].GetImageSize();
  const size_t npx = static_cast<size_t>(size->width) * size->height;
  std::vector<double> stack(npx * images.size());
  for (size_t i = 0; i < images.size(); ++i) {
    if (images[i].GetNumChannels() < 1 || images[i].GetImageSize().width != size->width ||
        images[i].GetImageSize().height != size->height)
      srmap_host::Fail("registration needs images of one size with at least one channel");
    const double* ch = images[i].GetChannelData(0);
    std::copy(ch, ch + npx, stack.begin() + i * npx);
  }
  return stack;
}

// The body of the two translational functions: quality == nullptr is the reference's call (srmap_register_translational).
inline MotionShiftSequence Translational(const std::vector<ImageData>& images, std::vector<double>* quality) {
  cv::Size size;
  const std::vector<double> stack = ChannelZeroStack(images, &size);
  const int n = static_cast<int>(images.size());
  std::vector<double> xy(2 * images.size());
  if (quality) quality->assign(2 * images.size(), 0.0);
  srmap_host::Check(quality ? srmap_register_translational_ex(srmap_host::Context(), n, size.width, size.height, stack.data(),
                                                              xy.data(), quality->data())
                            : srmap_register_translational(srmap_host::Context(), n, size.width, size.height, stack.data(),
                                                           xy.data()),
                    "Could not determine motion shift between images.");
  std::vector<MotionShift> shifts;
  for (size_t i = 0; i < images.size(); ++i) shifts.push_back(MotionShift(xy[2 * i], xy[2 * i + 1]));
  return MotionShiftSequence(shifts);
}
}  // namespace internal

inline MotionShiftSequence TranslationalRegistration(const std::vector<ImageData>& images) {
  if (images.empty()) {
    std::fprintf(stderr, "WARNING: No images given. Returning an empty motion sequence.\n");
    return MotionShiftSequence();
  }
  return internal::Translational(images, nullptr);
}

// The same with the estimator's per-image quality: quality[2i] = separation of the coarse minimum (near 1 = clear,
// near 0 = ambiguous), quality[2i + 1] = RMS residual at the returned shift.
inline MotionShiftSequence TranslationalRegistrationWithQuality(const std::vector<ImageData>& images,
                                                                std::vector<double>* quality) {
  if (images.empty()) return MotionShiftSequence();
  return internal::Translational(images, quality);
}

// Not in the reference: the affine motion of every image relative to the first one (srmap_register_affine,
// csrc/registration_affine.hip), as an AffineMotionSequence in units of `scale` input pixels -- register the LR frames
// with scale = the upsampling scale and the result is what MotionModule(AffineMotionSequence) takes.  Channel 0 is the
// registration image; an empty list gives an empty sequence; image 0 gets the identity.  Dense, no outlier rejection,
// one plane: include/srmap.h states the domain.  quality (WithQuality): 4 per image -- separation of the coarse minimum,
// RMS residual, fraction of pixels used, Gauss-Newton passes.
inline AffineMotionSequence AffineRegistrationWithQuality(const std::vector<ImageData>& images, const int scale,
                                                          std::vector<double>* quality) {
  if (images.empty()) {
    std::fprintf(stderr, "WARNING: No images given. Returning an empty motion sequence.\n");
    return AffineMotionSequence();
  }
  cv::Size size;
  const std::vector<double> stack = internal::ChannelZeroStack(images, &size);
  srmap_affine_registration_options options;
  srmap_affine_registration_options_default(&options);
  options.hr_scale = scale;
  std::vector<double> m(6 * images.size());
  if (quality) quality->assign(4 * images.size(), 0.0);
  srmap_host::Check(srmap_register_affine(srmap_host::Context(), static_cast<int>(images.size()), size.width, size.height,
                                          stack.data(), &options, m.data(), quality ? quality->data() : nullptr),
                    "Could not determine motion between images.");
  std::vector<AffineMotion> motions;
  for (size_t i = 0; i < images.size(); ++i)
    motions.push_back(AffineMotion(m[6 * i], m[6 * i + 1], m[6 * i + 2], m[6 * i + 3], m[6 * i + 4], m[6 * i + 5]));
  return AffineMotionSequence(motions);
}

inline AffineMotionSequence AffineRegistration(const std::vector<ImageData>& images, const int scale = 1) {
  return AffineRegistrationWithQuality(images, scale, nullptr);
}

// Options of FlowRegistration (srmap_flow_registration_options, include/srmap.h).
struct FlowRegistrationOptions {
  int warps = 8;
  int window_radius = 4;
  double damping = 0.05;
  int smooth_radius = 2;
  int valid_margin = 3;
  int max_levels = 0;
  AffineMotionSequence initial_motion;  // empty: start from u = 0; else one matrix per image, INPUT-pixel units
};

// Not in the reference: a dense displacement field for every image relative to the first one (srmap_register_flow,
// csrc/registration_flow.hip), as a FlowMotionSequence at `scale` times the input size in units of `scale` input pixels --
// register the LR frames with scale = the upsampling scale and the result is what MotionModule(FlowMotionSequence) takes.
// Channel 0 is the registration image; an empty list gives an empty sequence; image 0 gets u = 0.  valid (optional):
// [images][h][w] at INPUT resolution, 1 where the field can be trusted, else 0 -- hand it to
// IRLSMapSolver::MultiplyDataWeights, the field is wrong at the frame border where image 0 does not hold the content.
// quality (optional): 3 per image -- RMS residual over the valid pixels, the valid fraction, the largest neighbour
// difference dx + dy of the field.  Dense, local, no occlusion handling, one plane: include/srmap.h states what it is not.
inline FlowMotionSequence FlowRegistration(const std::vector<ImageData>& images, const int scale = 1,
                                           std::vector<double>* valid = nullptr, std::vector<double>* quality = nullptr,
                                           const FlowRegistrationOptions& registration_options = FlowRegistrationOptions()) {
  if (images.empty()) {
    std::fprintf(stderr, "WARNING: No images given. Returning an empty motion sequence.\n");
    if (valid) valid->clear();
    if (quality) quality->clear();
    return FlowMotionSequence();
  }
  if (scale < 1) srmap_host::Fail("flow registration: the scale must be at least 1");
  cv::Size size;
  const std::vector<double> stack = internal::ChannelZeroStack(images, &size);
  const size_t npx = static_cast<size_t>(size.width) * size.height;
  srmap_flow_registration_options options;
  srmap_flow_registration_options_default(&options);
  options.hr_scale = scale;
  options.warps = registration_options.warps;
  options.window_radius = registration_options.window_radius;
  options.damping = registration_options.damping;
  options.smooth_radius = registration_options.smooth_radius;
  options.valid_margin = registration_options.valid_margin;
  options.max_levels = registration_options.max_levels;
  std::vector<double> initial;
  if (registration_options.initial_motion.GetNumMotions() > 0) {
    if (static_cast<size_t>(registration_options.initial_motion.GetNumMotions()) < images.size())
      srmap_host::Fail("flow registration: fewer initial matrices than images");
    for (size_t i = 0; i < images.size(); ++i) {
      const AffineMotion& m = registration_options.initial_motion[static_cast<int>(i)];
      const double row[6] = {m.a, m.b, m.tx, m.c, m.d, m.ty};
      initial.insert(initial.end(), row, row + 6);
    }
    options.initial_affine_2x3 = initial.data();
  }
  std::vector<double> flow(2 * npx * scale * scale * images.size());
  if (valid) valid->assign(npx * images.size(), 0.0);
  if (quality) quality->assign(3 * images.size(), 0.0);
  srmap_host::Check(srmap_register_flow(srmap_host::Context(), static_cast<int>(images.size()), size.width, size.height,
                                        stack.data(), &options, flow.data(), valid ? valid->data() : nullptr,
                                        quality ? quality->data() : nullptr),
                    "Could not determine motion between images.");
  return FlowMotionSequence(flow, size.width * scale, size.height * scale);
}

}  // namespace registration
}  // namespace super_resolution
