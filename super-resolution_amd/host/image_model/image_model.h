// The reference's forward-model interface for the MAP path, forwarding to the
// HIP library through the C ABI:
//   DegradationOperator  src/image_model/degradation_operator.h:17-57
//   MotionModule         src/image_model/motion_module.{h,cpp}; also constructible from an AffineMotionSequence
//                        (motion/affine_motion.h) or a FlowMotionSequence (motion/flow_motion.h); no reference counterpart
//   BlurModule           src/image_model/blur_module.{h,cpp}; also constructible from a BlurKernel, a free-form PSF
//                        (image_model/blur_kernel.h; no reference counterpart)
//   DownsamplingModule   src/image_model/downsampling_module.{h,cpp}
//   ImageModel, ImageModelParameters, CreateImageModel
//                        src/image_model/image_model.{h,cpp}
//   AdditiveNoiseModule  src/image_model/additive_noise_module.{h,cpp} (data generation: host-side N(0, sigma/255)
//                        per pixel; cv::randn's global stream cannot be reproduced, the generator is seedable)
// Dense operator matrices (GetOperatorMatrix / GetModelMatrix) are test helpers of
// the reference and are not provided.
#pragma once
#include <cstdint>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "image/image_data.h"
#include "image_model/blur_kernel.h"
#include "motion/affine_motion.h"
#include "motion/flow_motion.h"
#include "motion/motion_shift.h"
#include "util/srmap_host.h"

namespace super_resolution {

namespace srmap_host {
// Runs srmap_apply / srmap_apply_transpose for one chain on an ImageData.
inline void RunChain(const ChainParams& c, ImageData* image, int index, bool transpose) {
  if (!image) Fail("CHECK_NOTNULL(image_data)");
  const cv::Size in = image->GetImageSize();
  const int C = image->GetNumChannels();
  const std::vector<double> src = image->ToPlanar();
  if (!transpose) {
    ProblemPtr p = MakeProblem(c, in.width, in.height, C);
    int lw = 0, lh = 0;
    srmap_problem_lr_size(p.get(), &lw, &lh);
    std::vector<double> dst(static_cast<size_t>(lw) * lh * C);
    Check(srmap_apply(p.get(), index, src.data(), dst.data()), "srmap_apply");
    image->FromPlanar(dst, cv::Size(lw, lh), C);
  } else {
    const cv::Size out(in.width * c.scale, in.height * c.scale);
    ProblemPtr p = MakeProblem(c, out.width, out.height, C);
    std::vector<double> dst(static_cast<size_t>(out.area()) * C);
    Check(srmap_apply_transpose(p.get(), index, src.data(), dst.data()), "srmap_apply_transpose");
    image->FromPlanar(dst, out, C);
  }
}
}  // namespace srmap_host

class DegradationOperator {
 public:
  virtual ~DegradationOperator() = default;
  virtual void ApplyToImage(ImageData* image_data, const int index) const = 0;
  virtual void ApplyTransposeToImage(ImageData* image_data, const int index) const = 0;
  // What this operator contributes to a fused chain.  The reference's interface has no such member
  // (degradation_operator.h:17-57) and its callers subclass DegradationOperator (test/test_image_model.cpp:31-46): the
  // default is "nothing" -- ImageModel::Canonical() does not recognise such an operator, so a model that contains one is
  // applied operator by operator on the host side of the ABI, exactly as the reference's loop does.
  virtual void Describe(srmap_host::ChainParams* chain) const { (void)chain; }

 protected:
  // the chain of this operator alone: what its own ApplyToImage / ApplyTransposeToImage run
  srmap_host::ChainParams Chain() const { srmap_host::ChainParams c; Describe(&c); return c; }
};

class MotionModule : public DegradationOperator {
 public:
  explicit MotionModule(const MotionShiftSequence& sequence) : sequence_(sequence), affine_(false), flow_(false) {}
  // not in the reference: per-frame affine warps (the exact-coordinate bilinear warp and its exact adjoint, include/srmap.h)
  explicit MotionModule(const AffineMotionSequence& sequence) : affine_sequence_(sequence), affine_(true), flow_(false) {}
  // not in the reference: a dense displacement field per frame (srmap_problem_set_flow, include/srmap.h); the transpose
  // runs at the field's own size only
  explicit MotionModule(const FlowMotionSequence& sequence) : flow_sequence_(sequence), affine_(false), flow_(true) {
    if (sequence.Empty()) srmap_host::Fail("MotionModule: the flow motion sequence is empty");
  }
  void ApplyToImage(ImageData* image_data, const int index) const override {
    CheckIndex(index);
    srmap_host::RunChain(Chain(), image_data, index, false);
  }
  void ApplyTransposeToImage(ImageData* image_data, const int index) const override {
    CheckIndex(index);
    srmap_host::RunChain(Chain(), image_data, index, true);
  }
  void Describe(srmap_host::ChainParams* c) const override {
    c->shifts_xy.clear();
    c->affine_2x3.clear();
    c->flow.clear();
    if (flow_) { c->flow = flow_sequence_.Flat(); c->flow_width = flow_sequence_.GetWidth(); c->flow_height = flow_sequence_.GetHeight(); }
    else if (affine_) c->affine_2x3 = affine_sequence_.Flat();
    else c->shifts_xy = sequence_.Flat();
  }
  bool IsAffine() const { return affine_; }
  bool IsFlow() const { return flow_; }

 private:
  void CheckIndex(const int index) const {
    if (flow_) flow_sequence_.CheckIndex(index);
    else if (affine_) affine_sequence_.GetAffineMotion(index);
    else sequence_.GetMotionShift(index);
  }
  const MotionShiftSequence sequence_;
  const AffineMotionSequence affine_sequence_;
  const FlowMotionSequence flow_sequence_;
  const bool affine_, flow_;
};

class BlurModule : public DegradationOperator {
 public:
  // blur_radius is the (odd) kernel size, sigma > 0 (blur_module.cpp:13-23).
  BlurModule(const int blur_radius, const double sigma) : blur_radius_(blur_radius), sigma_(sigma) {
    if (blur_radius < 1 || !(sigma > 0.0) || blur_radius % 2 != 1)
      srmap_host::Fail("BlurModule: radius must be odd and >= 1, sigma > 0");
  }
  // not in the reference: a free-form kernel (square, odd; the forward model correlates with it, the transpose with its
  // flip in both axes -- the exact adjoint; srmap_problem_set_blur_kernel, include/srmap.h)
  explicit BlurModule(const BlurKernel& kernel) : blur_radius_(kernel.GetSize()), sigma_(0.0), kernel_(kernel) {
    if (kernel.Empty()) srmap_host::Fail("BlurModule: the blur kernel is empty");
  }
  // not in the reference: a bank of free-form kernels, one per frame, per channel or per (frame, channel)
  // (srmap_problem_set_blur_bank, include/srmap.h); a per-frame entry goes by the index the operator is applied with
  explicit BlurModule(const BlurKernelBank& bank) : blur_radius_(bank.GetSize()), sigma_(0.0), bank_(bank) {
    if (bank.Empty()) srmap_host::Fail("BlurModule: the blur bank is empty");
  }
  void ApplyToImage(ImageData* image_data, const int index) const override {
    srmap_host::RunChain(Chain(), image_data, Chain().BankPerFrame() ? index : 0, false);
  }
  void ApplyTransposeToImage(ImageData* image_data, const int index) const override {
    srmap_host::RunChain(Chain(), image_data, Chain().BankPerFrame() ? index : 0, true);
  }
  void Describe(srmap_host::ChainParams* c) const override {
    c->blur_bank_mode = 0; c->blur_bank_ksize = 0; c->blur_bank.clear();
    if (!bank_.Empty()) {
      c->blur_ksize = 0; c->blur_sigma = 0.0; c->blur_taps.clear(); c->blur_taps_ksize = 0;
      c->blur_bank_mode = bank_.GetMode(); c->blur_bank_ksize = bank_.GetSize(); c->blur_bank = bank_.GetTaps();
    } else if (kernel_.Empty()) { c->blur_ksize = blur_radius_; c->blur_sigma = sigma_; c->blur_taps.clear(); c->blur_taps_ksize = 0; }
    else { c->blur_ksize = 0; c->blur_sigma = 0.0; c->blur_taps = kernel_.GetTaps(); c->blur_taps_ksize = kernel_.GetSize(); }
  }
  bool IsFreeForm() const { return !kernel_.Empty() || !bank_.Empty(); }
  bool IsBank() const { return !bank_.Empty(); }

 private:
  const int blur_radius_;
  const double sigma_;
  const BlurKernel kernel_;
  const BlurKernelBank bank_;
};

class DownsamplingModule : public DegradationOperator {
 public:
  explicit DownsamplingModule(const int scale) : scale_(scale) {
    if (scale < 1) srmap_host::Fail("DownsamplingModule: scale must be >= 1");
  }
  void ApplyToImage(ImageData* image_data, const int index) const override {
    srmap_host::RunChain(Chain(), image_data, 0, false);
  }
  void ApplyTransposeToImage(ImageData* image_data, const int index) const override {
    srmap_host::RunChain(Chain(), image_data, 0, true);
  }
  void Describe(srmap_host::ChainParams* c) const override { c->scale = scale_; }

 private:
  const int scale_;
};

// additive_noise_module.cpp:19-36: zero-mean Gaussian noise of standard deviation sigma / 255 (the pixels are scaled
// to [0, 1]) on every channel; the transpose is a no-op (:38-44).  Last operator of a data-generation chain only.
class AdditiveNoiseModule : public DegradationOperator {
 public:
  explicit AdditiveNoiseModule(const double sigma, const uint64_t seed = 0x5eedULL) : sigma_(sigma), rng_(seed) {
    if (!(sigma > 0.0)) srmap_host::Fail("Check failed: sigma_ > 0.0");
  }
  void ApplyToImage(ImageData* image_data, const int /*index*/) const override {
    if (!image_data) srmap_host::Fail("CHECK_NOTNULL(image_data)");
    std::normal_distribution<double> gauss(0.0, sigma_ / 255.0);
    for (int c = 0; c < image_data->GetNumChannels(); ++c) {
      double* px = image_data->GetMutableChannelData(c);
      for (int i = 0; i < image_data->GetNumPixels(); ++i) px[i] += gauss(rng_);
    }
  }
  void ApplyTransposeToImage(ImageData* image_data, const int /*index*/) const override {
    if (!image_data) srmap_host::Fail("CHECK_NOTNULL(image_data)");
  }
  void Describe(srmap_host::ChainParams*) const override {}
  void SetSeed(const uint64_t seed) const { rng_.seed(seed); }

 private:
  const double sigma_;
  mutable std::mt19937_64 rng_;
};

struct ImageModelParameters {
  int scale = 2;
  int blur_radius = 0;
  double blur_sigma = 0.0;
  std::string motion_sequence_path = "";
  MotionShiftSequence motion_sequence;
  // not in the reference: per-frame affine motion ("a b tx c d ty" per line); excludes motion_sequence(_path)
  std::string affine_motion_sequence_path = "";
  AffineMotionSequence affine_motion_sequence;
  // not in the reference: a dense displacement field per frame (motion/flow_motion.h).  The file has no header, so the
  // caller loads it with the HR geometry (FlowMotionSequence::LoadSequenceFromFile); excludes the two sequences above
  FlowMotionSequence flow_motion_sequence;
  // not in the reference: a free-form blur kernel (text file: ksize, then ksize^2 taps); it replaces the Gaussian of
  // blur_radius / blur_sigma
  std::string blur_kernel_path = "";
  BlurKernel blur_kernel;
  // not in the reference: a blur-kernel bank (text file: `mode ksize entries`, then the taps; image_model/blur_kernel.h); it
  // replaces the Gaussian and excludes blur_kernel(_path)
  std::string blur_bank_path = "";
  BlurKernelBank blur_bank;
  double noise_sigma = 0.0;
  uint64_t noise_seed = 0x5eedULL;  // not in the reference (cv::randn draws from OpenCV's global generator)
};

class ImageModel {
 public:
  explicit ImageModel(const int downsampling_scale) : downsampling_scale_(downsampling_scale) {
    if (downsampling_scale < 1) srmap_host::Fail("Downsampling scale must be at least 1");
  }
  // image_model.cpp:17-61
  static ImageModel CreateImageModel(const ImageModelParameters& parameters) {
    ImageModel model(parameters.scale);
    const bool affine = !parameters.affine_motion_sequence_path.empty() || parameters.affine_motion_sequence.GetNumMotions() > 0;
    if (affine && (!parameters.motion_sequence_path.empty() || parameters.motion_sequence.GetNumMotionShifts() > 0))
      srmap_host::Fail("both an affine motion sequence and a motion shift sequence were given: a model has one MotionModule");
    if (!parameters.flow_motion_sequence.Empty()) {
      if (affine || !parameters.motion_sequence_path.empty() || parameters.motion_sequence.GetNumMotionShifts() > 0)
        srmap_host::Fail("a flow motion sequence and another motion sequence were given: a model has one MotionModule");
      model.AddDegradationOperator(std::make_shared<MotionModule>(parameters.flow_motion_sequence));
    }
    if (affine) {
      AffineMotionSequence seq = parameters.affine_motion_sequence;
      if (seq.GetNumMotions() == 0) seq.LoadSequenceFromFile(parameters.affine_motion_sequence_path);
      model.AddDegradationOperator(std::make_shared<MotionModule>(seq));
    }
    if (!parameters.motion_sequence_path.empty() || parameters.motion_sequence.GetNumMotionShifts() > 0) {
      MotionShiftSequence seq = parameters.motion_sequence;
      if (seq.GetNumMotionShifts() == 0) seq.LoadSequenceFromFile(parameters.motion_sequence_path);
      model.AddDegradationOperator(std::make_shared<MotionModule>(seq));
    }
    if (!parameters.blur_bank_path.empty() || !parameters.blur_bank.Empty()) {
      if (!parameters.blur_kernel_path.empty() || !parameters.blur_kernel.Empty())
        srmap_host::Fail("both a blur bank and a blur kernel were given: a model has one BlurModule");
      BlurKernelBank bank = parameters.blur_bank;
      if (bank.Empty()) bank.LoadFromFile(parameters.blur_bank_path);
      model.AddDegradationOperator(std::make_shared<BlurModule>(bank));
    } else if (!parameters.blur_kernel_path.empty() || !parameters.blur_kernel.Empty()) {
      BlurKernel kernel = parameters.blur_kernel;
      if (kernel.Empty()) kernel.LoadFromFile(parameters.blur_kernel_path);
      model.AddDegradationOperator(std::make_shared<BlurModule>(kernel));
    } else if (parameters.blur_radius > 0 && parameters.blur_sigma > 0.0)
      model.AddDegradationOperator(std::make_shared<BlurModule>(parameters.blur_radius, parameters.blur_sigma));
    model.AddDegradationOperator(std::make_shared<DownsamplingModule>(parameters.scale));
    if (parameters.noise_sigma > 0.0)  // image_model.cpp:53-58
      model.AddDegradationOperator(std::make_shared<AdditiveNoiseModule>(parameters.noise_sigma, parameters.noise_seed));
    return model;
  }
  void AddDegradationOperator(std::shared_ptr<DegradationOperator> op) { operators_.push_back(op); }
  ImageData ApplyToImage(const ImageData& image_data, const int index) const {
    ImageData degraded = image_data;
    ApplyToImage(&degraded, index);
    return degraded;
  }
  // image_model.cpp:86-91: operators in insertion order.  The canonical chain
  // [Motion][Blur]Downsampling runs as ONE fused device pass.
  void ApplyToImage(ImageData* image_data, const int index) const {
    srmap_host::ChainParams chain;
    // Blur and downsampling ignore the index (blur_module.cpp:25-28, downsampling_module.cpp:19-27): without a
    // MotionModule the fused problem has ONE frame, whatever index the caller passes
    const AdditiveNoiseModule* noise = nullptr;
    if (Canonical(&chain, &noise)) {
      srmap_host::RunChain(chain, image_data, (chain.HasMotion() || chain.BankPerFrame()) ? index : 0, false);
      if (noise) noise->ApplyToImage(image_data, index);
      return;
    }
    for (const auto& op : operators_) op->ApplyToImage(image_data, index);
  }
  // image_model.cpp:93-101: transposes in reverse order.
  void ApplyTransposeToImage(ImageData* image_data, const int index) const {
    srmap_host::ChainParams chain;
    if (Canonical(&chain)) { srmap_host::RunChain(chain, image_data, (chain.HasMotion() || chain.BankPerFrame()) ? index : 0, true); return; }  // a trailing noise module's transpose is a no-op
    for (int i = static_cast<int>(operators_.size()) - 1; i >= 0; --i) operators_[i]->ApplyTransposeToImage(image_data, index);
  }
  int GetDownsamplingScale() const { return downsampling_scale_; }
  // The fused chain description (valid when the operator list is canonical: [Motion][Blur]Downsampling, optionally
  // followed by an AdditiveNoiseModule, which is returned separately and applied on the host).
  bool Canonical(srmap_host::ChainParams* chain, const AdditiveNoiseModule** noise = nullptr) const {
    int stage = 0;  // 0: expect motion/blur/down, 1: after motion, 2: after blur, 3: after down, 5: after noise
    for (const auto& op : operators_) {
      if (const auto* nm = dynamic_cast<const AdditiveNoiseModule*>(op.get())) {
        if (stage != 3) return false;
        stage = 5;
        if (noise) *noise = nm;
        continue;
      }
      const int kind = dynamic_cast<const MotionModule*>(op.get()) ? 1
                       : dynamic_cast<const BlurModule*>(op.get()) ? 2
                       : dynamic_cast<const DownsamplingModule*>(op.get()) ? 3 : 4;
      if (kind == 4 || kind <= stage) return false;
      stage = kind;
      op->Describe(chain);
    }
    return stage == 3 || stage == 5;
  }

 private:
  std::vector<std::shared_ptr<DegradationOperator>> operators_;
  const int downsampling_scale_;
};

namespace srmap_host {
// The problem of a solver over n observations: the model's canonical chain with n frames and the first n of its motions.
// `who` names the caller in the refusal of any other operator list.
inline ProblemPtr MakeSolverProblem(const ImageModel& image_model, const size_t n, const cv::Size& image_size, const int channels,
                                    const char* who) {
  ChainParams chain;
  if (!image_model.Canonical(&chain)) Fail((std::string(who) + " needs the [Motion][Blur]Downsampling operator chain").c_str());
  chain.frames = static_cast<int>(n);
  if (chain.HasMotion() && static_cast<size_t>(chain.NumMotions()) < n) Fail("fewer motion shifts than observations");
  chain.TrimMotions(n);
  return MakeProblem(chain, image_size.width, image_size.height, channels);
}
}  // namespace srmap_host

}  // namespace super_resolution
