// super_resolution -- the caller of the MAP path (reference:
// src/super_resolution.cpp:38-115 flags, :126-199 SetupAndRunSolver, :269-453
// main), on the drop-in classes: load or generate the LR frames, bilinear
// initial estimate, IRLS-MAP solve on the GPU, optional PSNR against the ground
// truth, save.  Same flag names and defaults.  --solver=cg|lbfgs selects the
// least-squares solver as the reference does (super_resolution.cpp:134-141; any
// other value warns and runs CG).  --data_loss=l2|huber and --huber_delta are NOT
// reference flags: the robust data term of include/srmap.h.  Nor is --affine_motion_path: per-frame affine motion.  Nor is
// --flow_motion_path: a dense displacement field per frame (srmap_problem_set_flow).  Nor are
// --registration=translational|affine|flow (the solver's motion estimated from the LR frames on the GPU; flow: dense
// displacement fields and their validity masks as data weights, srmap_register_flow), --save_flow_path and
// --save_motion_path, nor --refine_motion_rounds / --refine_motion_dof (the joint motion refinement, srmap_refine_motion), nor
// --blur_kernel_path (a free-form blur kernel, srmap_problem_set_blur_kernel) and --fit_blur_from / --fit_blur_ksize /
// --save_blur_kernel_path (its calibration fit from a known HR image, srmap_fit_blur), nor --blur_bank_path (a blur kernel
// per frame and / or channel, srmap_problem_set_blur_bank) and --fit_blur_bank_from / --fit_blur_bank_mode /
// --save_blur_bank_path (its calibration fit, srmap_fit_blur_bank), nor --photometric_path /
// --photometric_rounds / --save_photometric_path (per-frame gain and bias, srmap_problem_set_photometric and
// srmap_fit_photometric).
// Not carried over (out of scope, DESIGN.md
// section 7): wavelet-domain solve, numerical differentiation, SSIM, display.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "apps/app_flags.h"
#include "evaluation/peak_signal_to_noise_ratio.h"
#include "evaluation/structural_similarity.h"
#include "hyperspectral/spectral_pca.h"
#include "image/image_io.h"
#include "image_model/image_model.h"
#include "motion/registration.h"
#include "optimization/irls_map_solver.h"
#include "optimization/regularizer.h"

using namespace super_resolution;

int main(int argc, char** argv) {
  app::Flags flags(argc, argv,
      "super_resolution --data_path=<dir of LR frames | HR image with --generate_lr_images>\n"
      "  [--generate_lr_images] [--noise_sigma=0] [--noise_seed=1] [--number_of_frames=4]\n"
      "  [--ground_truth_image=<path>] [--upsampling_scale=2] [--blur_radius=3] [--blur_sigma=1]\n"
      "  [--motion_sequence_path=<file>] [--optimization_iterations=20] [--split_channels]\n"
      "  [--regularizer=tv|3dtv|btv] [--btv_scale_range=3] [--btv_spatial_decay=0.5]\n"
      "  [--regularization_parameter=0.01] [--solver=cg] [--solver_iterations=50]\n"
      "  [--interpolate_color] [--solve_in_pca_space] [--num_pca_components=0] [--pca_retained_variance=0]\n"
      "  [--evaluators=psnr,ssim] [--result_path=<path>] [--verbose]\n"
      "  not reference flags: [--data_loss=l2|huber] [--huber_delta=0.02] (robust data term, pixel units 0..1)\n"
      "                       [--affine_motion_path=<file>] (per-frame affine motion, 'a b tx c d ty' per line, HR pixels;\n"
      "                       an error together with --motion_sequence_path)\n"
      "                       [--flow_motion_path=<file>] (a dense displacement field per frame: raw little-endian float64,\n"
      "                       [frames][2][H][W] = the (ux, uy) planes in HR pixels at the high-resolution size; an error\n"
      "                       together with --motion_sequence_path, --affine_motion_path, --registration,\n"
      "                       --refine_motion_rounds, --fit_blur_from and --photometric_rounds)\n"
      "                       [--registration=translational|affine|flow] (estimate the solver's motion from the LR frames, in\n"
      "                       HR pixels; with --generate_lr_images the motion files still generate the frames, without it\n"
      "                       an error together with either motion file.  flow: a dense displacement field per frame, and\n"
      "                       its validity masks as data weights of a least-squares solve (--data_loss=huber derives its own\n"
      "                       weights and runs without the masks); an error together with --motion_sequence_path,\n"
      "                       --affine_motion_path, --refine_motion_rounds, --fit_blur_from and --photometric_rounds)\n"
      "                       [--save_flow_path=<file>] (the estimated fields, in --flow_motion_path's format; needs\n"
      "                       --registration=flow)\n"
      "                       [--flow_valid_prior] (install the validity masks of --registration=flow as a persistent prior\n"
      "                       on the data weights instead of multiplying them in, so that they hold under --data_loss=huber\n"
      "                       too; needs --registration=flow)\n"
      "                       [--save_motion_path=<file>] (the estimate, 'a b tx c d ty' per line; needs --registration or\n"
      "                       --refine_motion_rounds, and holds the final matrices)\n"
      "                       [--refine_motion_rounds=0] (after the solve, N times: re-fit the frame matrices to the estimate\n"
      "                       through the forward model, then solve again from it; 0 = off; works with every motion source)\n"
      "                       [--refine_motion_dof=6] (6: the full matrices; 2: translations only)\n"
      "                       [--blur_kernel_path=<file>] (a free-form blur kernel instead of the Gaussian of --blur_radius /\n"
      "                       --blur_sigma: text, the odd size ksize <= 7, then ksize * ksize taps in row-major order)\n"
      "                       [--fit_blur_from=<HR image>] (before solving, fit the blur kernel to the frames from this KNOWN\n"
      "                       high-resolution image of the scene -- a calibration pair -- and solve with it)\n"
      "                       [--fit_blur_ksize=0] (size of the fitted kernel; 0 = the size of the blur in force)\n"
      "                       [--save_blur_kernel_path=<file>] (the fitted kernel, in --blur_kernel_path's format)\n"
      "                       [--blur_bank_path=<file>] (a blur kernel per frame, per channel or per both: text, `mode ksize\n"
      "                       entries` with mode 1 = per frame, 2 = per channel, 3 = per frame and channel, then the taps)\n"
      "                       [--fit_blur_bank_from=<HR image>] --fit_blur_bank_mode=frame|channel|frame_channel (before solving,\n"
      "                       fit a bank to the frames from this KNOWN high-resolution image, one kernel per entry, of\n"
      "                       --fit_blur_ksize; solve with it) [--save_blur_bank_path=<file>] (the fitted bank, in\n"
      "                       --blur_bank_path's format).  The bank flags exclude --blur_kernel_path and --fit_blur_from.\n"
      "                       [--photometric_path=<file>] (known per-frame exposure, 'gain bias' per line, the bias in pixel\n"
      "                       units 0..1: the solve runs against (frame - bias) / gain)\n"
      "                       [--photometric_rounds=-1] (N >= 0: fit gain and bias of every frame but the first at the initial\n"
      "                       estimate, solve, then N times: fit at the estimate, solve again from it; with\n"
      "                       --refine_motion_rounds each round fits, refines the motion, then solves; -1 = off; an error\n"
      "                       together with --photometric_path)\n"
      "                       [--save_photometric_path=<file>] (the parameters in force after the solve, in\n"
      "                       --photometric_path's format; needs one of the two flags above)\n"
      "                       [--noise_seed=1] [--save_initial_estimate=<path>]");
  const std::string data_path = flags.Str("data_path");
  const bool generate_lr_images = flags.Bool("generate_lr_images", false);
  const double noise_sigma = flags.Double("noise_sigma", 0.0);
  const int noise_seed = flags.Int("noise_seed", 1);
  const int number_of_frames = flags.Int("number_of_frames", 4);
  const std::string ground_truth_image = flags.Str("ground_truth_image");
  const int upsampling_scale = flags.Int("upsampling_scale", 2);
  ImageModelParameters model_parameters;
  model_parameters.scale = upsampling_scale;
  model_parameters.blur_radius = flags.Int("blur_radius", 3);
  model_parameters.blur_sigma = flags.Double("blur_sigma", 1.0);
  model_parameters.motion_sequence_path = flags.Str("motion_sequence_path");
  // not a reference flag: the affine motion model of include/srmap.h (srmap_problem_set_affine_motion)
  model_parameters.affine_motion_sequence_path = flags.Str("affine_motion_path");
  // not a reference flag: the displacement-field motion model of include/srmap.h (srmap_problem_set_flow)
  const std::string flow_motion_path = flags.Str("flow_motion_path");
  IRLSMapSolverOptions solver_options;
  solver_options.max_num_irls_iterations = flags.Int("optimization_iterations", 20);
  solver_options.max_num_solver_iterations = flags.Int("solver_iterations", 50);
  solver_options.split_channels = flags.Bool("split_channels", false);
  std::string regularizer_name = flags.Str("regularizer", "tv");
  const int btv_scale_range = flags.Int("btv_scale_range", 3);
  const double btv_spatial_decay = flags.Double("btv_spatial_decay", 0.5);
  const double regularization_parameter = flags.Double("regularization_parameter", 0.01);
  const std::string solver_name = flags.Str("solver", "cg");
  // not reference flags: the loss of the data term (the reference's is plain least squares) and the Huber threshold in the
  // solver's pixel units (ImageData scales 8-bit input to 0..1)
  const std::string data_loss_name = flags.Str("data_loss", "l2");
  const double huber_delta = flags.Double("huber_delta", 0.02);
  const bool interpolate_color = flags.Bool("interpolate_color", false);
  const bool solve_in_pca_space = flags.Bool("solve_in_pca_space", false);
  const int num_pca_components = flags.Int("num_pca_components", 0);
  const double pca_retained_variance = flags.Double("pca_retained_variance", 0.0);
  const std::string evaluators = flags.Str("evaluators");
  const std::string result_path = flags.Str("result_path");
  // not a reference flag: the solver's start x0 as raw little-endian float64 [C][H][W], so that a CPU run of the
  // reference algorithm can start from the IDENTICAL estimate (tests/test_gpu_apps.py compares the two results)
  const std::string save_initial_estimate = flags.Str("save_initial_estimate");
  // not reference flags: estimate the solver's motion from the LR frames (srmap_register_translational /
  // srmap_register_affine) instead of reading it from a file, and write the estimate out
  const std::string registration_name = flags.Str("registration");
  const std::string save_motion_path = flags.Str("save_motion_path");
  const std::string save_flow_path = flags.Str("save_flow_path");
  // not a reference flag: the validity masks as the persistent prior of srmap_set_data_prior (they hold under Huber too)
  const bool flow_valid_prior = flags.Bool("flow_valid_prior", false);
  // not reference flags: joint motion refinement (srmap_refine_motion) around the solve
  const int refine_motion_rounds = flags.Int("refine_motion_rounds", 0);
  const int refine_motion_dof = flags.Int("refine_motion_dof", 6);
  // not reference flags: a free-form blur kernel (srmap_problem_set_blur_kernel) and its calibration fit (srmap_fit_blur)
  model_parameters.blur_kernel_path = flags.Str("blur_kernel_path");
  const std::string fit_blur_from = flags.Str("fit_blur_from");
  const int fit_blur_ksize = flags.Int("fit_blur_ksize", 0);
  const std::string save_blur_kernel_path = flags.Str("save_blur_kernel_path");
  // not reference flags: a blur-kernel bank (srmap_problem_set_blur_bank) and its calibration fit (srmap_fit_blur_bank)
  model_parameters.blur_bank_path = flags.Str("blur_bank_path");
  const std::string fit_blur_bank_from = flags.Str("fit_blur_bank_from");
  const std::string fit_blur_bank_mode = flags.Str("fit_blur_bank_mode");
  const std::string save_blur_bank_path = flags.Str("save_blur_bank_path");
  // not reference flags: the photometric frame model (srmap_problem_set_photometric) and its fit (srmap_fit_photometric)
  const std::string photometric_path = flags.Str("photometric_path");
  const int photometric_rounds = flags.Int("photometric_rounds", -1);
  const std::string save_photometric_path = flags.Str("save_photometric_path");
  const bool verbose = flags.Bool("verbose", false);
  flags.RejectUnknown();
  flags.Require("data_path");
  if (!model_parameters.affine_motion_sequence_path.empty() && !model_parameters.motion_sequence_path.empty()) {
    std::fprintf(stderr, "ERROR: --affine_motion_path and --motion_sequence_path exclude each other.\n");
    return 1;
  }
  if (!flow_motion_path.empty()) {
    // the field IS the motion: nothing else may give or estimate one, and the three fits have no sampling leg for a field
    const char* other = !model_parameters.motion_sequence_path.empty() ? "--motion_sequence_path"
                        : !model_parameters.affine_motion_sequence_path.empty() ? "--affine_motion_path"
                        : !registration_name.empty() ? "--registration"
                        : refine_motion_rounds != 0 ? "--refine_motion_rounds"
                        : !fit_blur_from.empty() ? "--fit_blur_from"
                        : photometric_rounds >= 0 ? "--photometric_rounds" : nullptr;
    if (other) {
      std::fprintf(stderr, "ERROR: --flow_motion_path and %s exclude each other.\n", other);
      return 1;
    }
  }
  if (!registration_name.empty() && registration_name != "translational" && registration_name != "affine" &&
      registration_name != "flow") {
    std::fprintf(stderr, "ERROR: --registration is 'translational' or 'affine', or 'flow'.\n");
    return 1;
  }
  const bool register_flow = registration_name == "flow";
  if (register_flow) {
    // the estimated field IS the motion, as --flow_motion_path's: the same flags are refused (--registration itself aside)
    const char* other = !model_parameters.motion_sequence_path.empty() ? "--motion_sequence_path"
                        : !model_parameters.affine_motion_sequence_path.empty() ? "--affine_motion_path"
                        : refine_motion_rounds != 0 ? "--refine_motion_rounds"
                        : !fit_blur_from.empty() ? "--fit_blur_from"
                        : photometric_rounds >= 0 ? "--photometric_rounds" : nullptr;
    if (other) {
      std::fprintf(stderr, "ERROR: --registration=flow and %s exclude each other.\n", other);
      return 1;
    }
    if (!save_motion_path.empty()) {
      std::fprintf(stderr, "ERROR: --save_motion_path holds matrices; the fields of --registration=flow go to --save_flow_path.\n");
      return 1;
    }
  }
  if (!save_flow_path.empty() && !register_flow) {
    std::fprintf(stderr, "ERROR: --save_flow_path needs --registration=flow.\n");
    return 1;
  }
  if (flow_valid_prior && !register_flow) {
    std::fprintf(stderr, "ERROR: --flow_valid_prior needs --registration=flow.\n");
    return 1;
  }
  if (!registration_name.empty() && !generate_lr_images &&
      (!model_parameters.affine_motion_sequence_path.empty() || !model_parameters.motion_sequence_path.empty())) {
    std::fprintf(stderr, "ERROR: --registration estimates the motion; it excludes --motion_sequence_path and --affine_motion_path "
                         "(except with --generate_lr_images, where the files generate the frames).\n");
    return 1;
  }
  if (refine_motion_rounds < 0 || (refine_motion_dof != 2 && refine_motion_dof != 6)) {
    std::fprintf(stderr, "ERROR: --refine_motion_rounds is >= 0 and --refine_motion_dof is 2 or 6.\n");
    return 1;
  }
  if (!save_motion_path.empty() && registration_name.empty() && refine_motion_rounds == 0) {
    std::fprintf(stderr, "ERROR: --save_motion_path needs --registration or --refine_motion_rounds.\n");
    return 1;
  }
  if (fit_blur_ksize < 0 || (fit_blur_ksize != 0 && fit_blur_ksize % 2 != 1) || fit_blur_ksize > 7) {
    std::fprintf(stderr, "ERROR: --fit_blur_ksize is 0 or an odd size up to 7.\n");
    return 1;
  }
  if ((fit_blur_from.empty() && !save_blur_kernel_path.empty()) || (fit_blur_from.empty() && fit_blur_bank_from.empty() && fit_blur_ksize != 0)) {
    std::fprintf(stderr, "ERROR: --save_blur_kernel_path and --fit_blur_ksize need --fit_blur_from (--fit_blur_ksize also goes with --fit_blur_bank_from).\n");
    return 1;
  }
  {
    // the bank and the single kernel are alternatives, and so are their fits
    const bool bank_flag = !model_parameters.blur_bank_path.empty() || !fit_blur_bank_from.empty();
    const char* other = !model_parameters.blur_kernel_path.empty() ? "--blur_kernel_path" : !fit_blur_from.empty() ? "--fit_blur_from" : nullptr;
    if (bank_flag && other) {
      std::fprintf(stderr, "ERROR: %s and %s exclude each other.\n", !model_parameters.blur_bank_path.empty() ? "--blur_bank_path" : "--fit_blur_bank_from", other);
      return 1;
    }
  }
  if (fit_blur_bank_from.empty() && (!fit_blur_bank_mode.empty() || !save_blur_bank_path.empty())) {
    std::fprintf(stderr, "ERROR: --fit_blur_bank_mode and --save_blur_bank_path need --fit_blur_bank_from.\n");
    return 1;
  }
  const int fit_bank_mode = fit_blur_bank_mode == "frame" ? 1 : fit_blur_bank_mode == "channel" ? 2 : fit_blur_bank_mode == "frame_channel" ? 3 : 0;
  if (!fit_blur_bank_from.empty() && fit_bank_mode == 0) {
    std::fprintf(stderr, "ERROR: --fit_blur_bank_from needs --fit_blur_bank_mode=frame|channel|frame_channel.\n");
    return 1;
  }
  if (!fit_blur_bank_from.empty() && (!flow_motion_path.empty() || registration_name == "flow")) {
    std::fprintf(stderr, "ERROR: --fit_blur_bank_from has no sampling leg for a displacement field: not with --flow_motion_path or --registration=flow.\n");
    return 1;
  }
  if (photometric_rounds < -1) {
    std::fprintf(stderr, "ERROR: --photometric_rounds is >= 0 (or -1: off).\n");
    return 1;
  }
  if (!photometric_path.empty() && photometric_rounds >= 0) {
    std::fprintf(stderr, "ERROR: --photometric_path gives the parameters, --photometric_rounds fits them: they exclude each other.\n");
    return 1;
  }
  if (!save_photometric_path.empty() && photometric_path.empty() && photometric_rounds < 0) {
    std::fprintf(stderr, "ERROR: --save_photometric_path needs --photometric_path or --photometric_rounds.\n");
    return 1;
  }
  // super_resolution.cpp:134-141: "lbfgs" selects L-BFGS, anything but "cg" warns and falls back to CG
  if (solver_name == "lbfgs") {
    solver_options.least_squares_solver = LBFGS_SOLVER;
  } else if (solver_name != "cg") {
    std::fprintf(stderr, "WARNING: Invalid solver flag. Using conjugate gradient solver.\n");
  }

  // as --solver: "huber" selects the Huber loss, anything but "l2" warns and runs least squares
  if (data_loss_name == "huber") {
    solver_options.data_loss = HUBER_DATA_LOSS;
    solver_options.huber_delta = huber_delta;
  } else if (data_loss_name != "l2") {
    std::fprintf(stderr, "WARNING: Invalid data_loss flag. Using the least-squares (l2) data term.\n");
  }

  ImageData high_res_image;
  std::vector<ImageData> low_res_images;
  if (generate_lr_images) high_res_image = util::LoadImage(data_path);
  else low_res_images = util::LoadImages(data_path);
  if (!flow_motion_path.empty()) {  // the file has no header: its size is checked against the HR geometry
    if (!generate_lr_images && low_res_images.empty()) {
      std::fprintf(stderr, "Check failed: At least one low-resolution image is required for super-resolution.\n");
      return 1;
    }
    const cv::Size hr = generate_lr_images ? high_res_image.GetImageSize()
                                           : cv::Size(low_res_images[0].GetImageSize().width * upsampling_scale,
                                                      low_res_images[0].GetImageSize().height * upsampling_scale);
    model_parameters.flow_motion_sequence.LoadSequenceFromFile(flow_motion_path, hr.width, hr.height);
  }
  const ImageModel image_model = ImageModel::CreateImageModel(model_parameters);

  if (generate_lr_images) {  // data_path is the ground truth (super_resolution.cpp:285-299)
    // the generating model carries the AdditiveNoiseModule (sigma in 0..255 units), the solver's does not
    ImageModelParameters with_noise = model_parameters;
    with_noise.noise_sigma = noise_sigma;
    with_noise.noise_seed = static_cast<uint64_t>(noise_seed);
    const ImageModel image_model_with_noise = ImageModel::CreateImageModel(with_noise);
    for (int i = 0; i < number_of_frames; ++i) low_res_images.push_back(image_model_with_noise.ApplyToImage(high_res_image, i));
  } else {
    if (!ground_truth_image.empty()) high_res_image = util::LoadImage(ground_truth_image);
  }
  if (low_res_images.empty()) {
    std::fprintf(stderr, "Check failed: At least one low-resolution image is required for super-resolution.\n");
    return 1;
  }
  const bool has_ground_truth = !ground_truth_image.empty() || generate_lr_images;
  const bool evaluate_results = has_ground_truth && !evaluators.empty();

  // bilinear upsampling of frame 0 in the original spectral space: the evaluation baseline
  ImageData upsampled_image = low_res_images[0];
  upsampled_image.ResizeImage(upsampling_scale, INTERPOLATE_LINEAR);

  // luminance-only colour path (super_resolution.cpp:330-342, 392-395): solve Y, interpolate Cr / Cb
  if (interpolate_color) {
    std::printf("Super-resolving only the luminance channel.\n");
    for (auto& frame : low_res_images) frame.ChangeColorSpace(SPECTRAL_MODE_COLOR_YCRCB, true);
  }

  // spectral PCA (super_resolution.cpp:344-366): solve on the leading components, reconstruct afterwards
  std::unique_ptr<SpectralPCA> spectral_pca;
  if (solve_in_pca_space && !interpolate_color) {
    if (pca_retained_variance > 0.0) spectral_pca.reset(new SpectralPCA(low_res_images, pca_retained_variance));
    else spectral_pca.reset(new SpectralPCA(low_res_images, num_pca_components));
    for (auto& frame : low_res_images) frame = spectral_pca->GetPCAImage(frame);
    std::printf("Super-resolving in PCA space with %d PCA components.\n", low_res_images[0].GetNumChannels());
  }

  ImageData initial_estimate = low_res_images[0];
  initial_estimate.ResizeImage(upsampling_scale, INTERPOLATE_LINEAR);

  if (!save_initial_estimate.empty()) {
    const std::vector<double> planar = initial_estimate.ToPlanar();
    std::FILE* f = std::fopen(save_initial_estimate.c_str(), "wb");
    if (!f || std::fwrite(planar.data(), sizeof(double), planar.size(), f) != planar.size()) {
      std::fprintf(stderr, "ERROR: cannot write '%s'.\n", save_initial_estimate.c_str());
      return 1;
    }
    std::fclose(f);
  }

  // --registration: the solver's model takes its motion from the frames it is about to solve (channel 0), in HR pixels;
  // the generating model above keeps the motion files
  auto save_motion = [&](const AffineMotionSequence& sequence) -> bool {
    std::FILE* f = std::fopen(save_motion_path.c_str(), "w");
    if (!f) {
      std::fprintf(stderr, "ERROR: cannot write '%s'.\n", save_motion_path.c_str());
      return false;
    }
    for (int i = 0; i < sequence.GetNumMotions(); ++i) {
      const AffineMotion& m = sequence[i];
      std::fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", m.a, m.b, m.tx, m.c, m.d, m.ty);
    }
    std::fclose(f);
    return true;
  };
  ImageModelParameters solver_parameters = model_parameters;
  std::vector<double> flow_valid;  // --registration=flow: the validity masks, [frames][h][w] at LR resolution
  if (register_flow) {
    solver_parameters.flow_motion_sequence = registration::FlowRegistration(low_res_images, upsampling_scale, &flow_valid);
    double kept = 0.0;
    for (const double v : flow_valid) kept += v;
    std::printf("Estimated flow motion of %d frames from the low-resolution images; %.1f %% of the pixels are valid.\n",
                solver_parameters.flow_motion_sequence.GetNumMotions(), 100.0 * kept / static_cast<double>(flow_valid.size()));
    if (!save_flow_path.empty() && !solver_parameters.flow_motion_sequence.SaveToFile(save_flow_path)) {
      std::fprintf(stderr, "ERROR: cannot write '%s'.\n", save_flow_path.c_str());
      return 1;
    }
  } else if (!registration_name.empty()) {
    solver_parameters.motion_sequence_path.clear();
    solver_parameters.affine_motion_sequence_path.clear();
    AffineMotionSequence estimate;
    if (registration_name == "affine") {
      estimate = registration::AffineRegistration(low_res_images, upsampling_scale);
      solver_parameters.affine_motion_sequence = estimate;
    } else {
      const MotionShiftSequence lr_shifts = registration::TranslationalRegistration(low_res_images);
      std::vector<MotionShift> shifts;
      std::vector<AffineMotion> motions;
      for (int i = 0; i < lr_shifts.GetNumMotionShifts(); ++i) {
        shifts.push_back(MotionShift(upsampling_scale * lr_shifts[i].dx, upsampling_scale * lr_shifts[i].dy));
        motions.push_back(AffineMotion(1.0, 0.0, shifts.back().dx, 0.0, 1.0, shifts.back().dy));
      }
      solver_parameters.motion_sequence = MotionShiftSequence(shifts);
      estimate = AffineMotionSequence(motions);
    }
    std::printf("Estimated %s motion of %d frames from the low-resolution images.\n", registration_name.c_str(),
                estimate.GetNumMotions());
    // with refinement rounds the file holds the FINAL matrices: written after the solve
    if (!save_motion_path.empty() && refine_motion_rounds == 0 && !save_motion(estimate)) return 1;
  }
  const ImageModel solver_model = registration_name.empty() ? image_model : ImageModel::CreateImageModel(solver_parameters);

  IRLSMapSolver solver(solver_options, solver_model, low_res_images, verbose);
  if (regularization_parameter > 0.0) {
    std::shared_ptr<Regularizer> regularizer;
    if (regularizer_name == "btv") {
      regularizer = std::make_shared<BilateralTotalVariationRegularizer>(initial_estimate.GetImageSize(),
                                                                         btv_scale_range, btv_spatial_decay);
    } else {
      if (regularizer_name != "tv" && regularizer_name != "3dtv") {
        std::fprintf(stderr, "WARNING: Unknown regularizer option '%s'. Using default Total Variation regularizer.\n",
                     regularizer_name.c_str());
        regularizer_name = "tv";
      }
      auto tv = std::make_shared<TotalVariationRegularizer>(initial_estimate.GetImageSize());
      if (regularizer_name == "3dtv") tv->SetUse3dTotalVariation(true);
      regularizer = tv;
    }
    solver.AddRegularizer(regularizer, regularization_parameter);
  }
  // --registration=flow: the field is wrong where frame 0 does not hold the content; those pixels get weight 0.  A Huber
  // solve derives its own weights and resets the buffer (include/srmap.h) -- unless the masks are the persistent prior
  // (--flow_valid_prior, srmap_set_data_prior), which a Huber solve resets to and multiplies its weights by
  if (register_flow && flow_valid_prior) solver.SetDataPrior(flow_valid);
  else if (register_flow && solver_options.data_loss == L2_DATA_LOSS) solver.MultiplyDataWeights(flow_valid);

  // --fit_blur_from: the calibration fit, before the solve, from a known HR image of what the frames show
  if (!fit_blur_from.empty()) {
    if (interpolate_color || spectral_pca) {
      std::fprintf(stderr, "ERROR: --fit_blur_from works in the frames' own channels: not with --interpolate_color or --solve_in_pca_space.\n");
      return 1;
    }
    BlurFitOptions fit_options;
    fit_options.ksize = fit_blur_ksize;
    std::vector<double> quality;
    const BlurKernel fitted = solver.FitBlur(util::LoadImage(fit_blur_from), fit_options, &quality);
    std::printf("Fitted a %d x %d blur kernel: cost %g -> %g, status %g.\n", fitted.GetSize(), fitted.GetSize(), quality[0], quality[1], quality[4]);
    if (!save_blur_kernel_path.empty() && !fitted.SaveToFile(save_blur_kernel_path)) {
      std::fprintf(stderr, "ERROR: cannot write '%s'.\n", save_blur_kernel_path.c_str());
      return 1;
    }
  }

  // --fit_blur_bank_from: the same calibration fit per entry of a bank (a kernel per frame, per channel or per both)
  if (!fit_blur_bank_from.empty()) {
    if (interpolate_color || spectral_pca) {
      std::fprintf(stderr, "ERROR: --fit_blur_bank_from works in the frames' own channels: not with --interpolate_color or --solve_in_pca_space.\n");
      return 1;
    }
    BlurFitOptions fit_options;
    fit_options.ksize = fit_blur_ksize;
    std::vector<double> quality;
    const BlurKernelBank fitted = solver.FitBlurBank(util::LoadImage(fit_blur_bank_from), fit_bank_mode, fit_options, &quality);
    int degenerate = 0;
    for (int e = 0; e < fitted.GetNumEntries(); ++e) degenerate += quality[5 * e + 4] != 0.0;
    std::printf("Fitted a bank of %d %d x %d blur kernels (mode %s): %d degenerate.\n", fitted.GetNumEntries(), fitted.GetSize(),
                fitted.GetSize(), fit_blur_bank_mode.c_str(), degenerate);
    if (!save_blur_bank_path.empty() && !fitted.SaveToFile(save_blur_bank_path)) {
      std::fprintf(stderr, "ERROR: cannot write '%s'.\n", save_blur_bank_path.c_str());
      return 1;
    }
  }

  // --photometric_path: known exposure, in force for every solve below
  const bool photometric = !photometric_path.empty() || photometric_rounds >= 0;
  if (photometric && (interpolate_color || spectral_pca)) {
    std::fprintf(stderr, "ERROR: the photometric flags work in the frames' own channels: not with --interpolate_color or --solve_in_pca_space.\n");
    return 1;
  }
  if (!photometric_path.empty()) {
    PhotometricSequence known;
    known.LoadSequenceFromFile(photometric_path);
    solver.SetPhotometric(known);
  }

  std::printf("Super-resolving from %zu images...\n", low_res_images.size());
  const auto start_time = std::chrono::steady_clock::now();
  ImageData result;
  if (photometric_rounds >= 0) {
    MotionRefinementOptions refinement;
    refinement.dof = refine_motion_dof;
    AffineMotionSequence refined;
    PhotometricSequence fitted;
    // with --refine_motion_rounds every round fits the exposure, refines the motion, then solves; the larger count rules
    const int rounds = refine_motion_rounds > photometric_rounds ? refine_motion_rounds : photometric_rounds;
    result = solver.SolvePhotometricJoint(initial_estimate, rounds, refine_motion_rounds > 0, PhotometricFitOptions(), refinement,
                                          &fitted, &refined);
    std::printf("Fitted gain and bias of %d frames in %d rounds.\n", fitted.GetNumFrames(), rounds);
    if (refine_motion_rounds > 0) {
      std::printf("Refined the motion of %d frames in %d rounds.\n", refined.GetNumMotions(), rounds);
      if (!save_motion_path.empty() && !save_motion(refined)) return 1;
    }
  } else if (refine_motion_rounds > 0) {
    MotionRefinementOptions refinement;
    refinement.dof = refine_motion_dof;
    AffineMotionSequence refined;
    result = solver.SolveJoint(initial_estimate, refine_motion_rounds, refinement, &refined);
    std::printf("Refined the motion of %d frames in %d rounds.\n", refined.GetNumMotions(), refine_motion_rounds);
    if (!save_motion_path.empty() && !save_motion(refined)) return 1;
  } else {
    result = solver.Solve(initial_estimate);
  }
  if (!save_photometric_path.empty() && !solver.GetPhotometric().SaveToFile(save_photometric_path)) {
    std::fprintf(stderr, "ERROR: cannot write '%s'.\n", save_photometric_path.c_str());
    return 1;
  }
  const std::chrono::duration<double> elapsed = std::chrono::steady_clock::now() - start_time;
  std::printf("Done! Finished in %g seconds.\n", elapsed.count());
  if (interpolate_color) {
    result.InterpolateColorFrom(initial_estimate);
    result.ChangeColorSpace(SPECTRAL_MODE_COLOR_BGR);
  }
  if (spectral_pca) result = spectral_pca->ReconstructImage(result);

  if (evaluate_results) {
    size_t pos = 0;
    while (pos <= evaluators.size()) {
      const size_t comma = evaluators.find(',', pos);
      const std::string evaluator = util::TrimString(evaluators.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
      if (evaluator == "psnr") {
        const PeakSignalToNoiseRatioEvaluator psnr_evaluator(high_res_image);
        std::cout << "PSNR score on upsampled: " << psnr_evaluator.Evaluate(upsampled_image) << std::endl;
        std::cout << "PSNR score on result:    " << psnr_evaluator.Evaluate(result) << std::endl;
      } else if (evaluator == "ssim") {
        const StructuralSimilarityEvaluator ssim_evaluator(high_res_image);
        std::cout << "SSIM score on upsampled: " << ssim_evaluator.Evaluate(upsampled_image) << std::endl;
        std::cout << "SSIM score on result:    " << ssim_evaluator.Evaluate(result) << std::endl;
      } else if (!evaluator.empty()) {
        std::fprintf(stderr, "ERROR: Unknown/unsupported evaluator '%s'.\n", evaluator.c_str());
      }
      if (comma == std::string::npos) break;
      pos = comma + 1;
    }
  }
  if (!result_path.empty()) util::SaveImage(result, result_path);
  return 0;
}
