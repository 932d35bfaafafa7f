// super_resolution -- the caller of the MAP path (reference:
// src/super_resolution.cpp:38-115 flags, :126-199 SetupAndRunSolver, :269-453
// main), on the drop-in classes: load or generate the LR frames, bilinear
// initial estimate, IRLS-MAP solve on the GPU, optional PSNR against the ground
// truth, save.  Same flag names and defaults.  --solver=cg|lbfgs selects the
// least-squares solver as the reference does (super_resolution.cpp:134-141; any
// other value warns and runs CG).  --data_loss=l2|huber and --huber_delta are NOT
// reference flags: the robust data term of include/srmap.h; nor are --huber_scale=fixed|mad / --huber_tuning /
// --huber_min_delta (the Huber threshold from the residual scale) and --print_residual_scale.  Nor is --affine_motion_path: per-frame affine motion.  Nor is
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
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "apps/model_flags.h"
#include "evaluation/peak_signal_to_noise_ratio.h"
#include "evaluation/structural_similarity.h"
#include "hyperspectral/spectral_pca.h"
#include "image/image_io.h"
#include "image_model/image_model.h"
#include "motion/registration.h"
#include "optimization/irls_map_solver.h"
#include "optimization/regularizer.h"

#include <cmath>
#include <cstdlib>

#include "holdout_host.hpp"  // csrc/: the rules of hold-out validation, plain C++
#include "reg_gradient_host.hpp"  // csrc/: the words of --regularizer_gradient, plain C++

using namespace super_resolution;

namespace {

const char kUsage[] =
      "super_resolution --data_path=<dir of LR frames | HR image with --generate_lr_images>\n"
      "  [--generate_lr_images] [--noise_sigma=0] [--noise_seed=1] [--number_of_frames=4]\n"
      "  [--ground_truth_image=<path>] [--upsampling_scale=2] [--blur_radius=3] [--blur_sigma=1]\n"
      "  [--motion_sequence_path=<file>] [--optimization_iterations=20] [--split_channels]\n"
      "  [--regularizer=tv|3dtv|btv] [--btv_scale_range=3] [--btv_spatial_decay=0.5]\n"
      "  [--regularization_parameter=0.01] [--solver=cg] [--solver_iterations=50]\n"
      "  [--interpolate_color] [--solve_in_pca_space] [--num_pca_components=0] [--pca_retained_variance=0]\n"
      "  [--evaluators=psnr,ssim] [--result_path=<path>] [--verbose]\n"
      "  not reference flags: [--data_loss=l2|huber] [--huber_delta=0.02] (robust data term, pixel units 0..1)\n"
      "                       [--huber_scale=fixed|mad] [--huber_tuning=1.345] [--huber_min_delta=1e-4] (mad: the Huber threshold\n"
      "                       is max(tuning * 1.4826 * median|residual|, min_delta) over all frames, re-estimated at every\n"
      "                       re-weighting, instead of --huber_delta)\n"
      "                       [--print_residual_scale] (1.4826 * median|residual| of the result over all frames and per frame:\n"
      "                       a frame that stands out fits badly)\n"
      "                       [--holdout_fraction=0.1] [--holdout_seed=1] --lambda_path=<largest>:<ratio>:<count>\n"
      "                       [--lambda_patience=0] [--print_lambda_path] (the regularization parameter by hold-out validation:\n"
      "                       <count> solves at lambda = <largest> * <ratio>^j with that share of the pixels held out, each\n"
      "                       scored on the held-out pixels; the result is the solve on all pixels at the best lambda;\n"
      "                       --regularization_parameter is then unused; --lambda_path needs --holdout_fraction)\n"
      "                       [--holdout_folds=5] [--lambda_rule=min|one_se] [--lambda_se_factor=1] (instead of\n"
      "                       --holdout_fraction: k-fold cross-validation, every lambda solved and scored once per fold of a\n"
      "                       partition of the pixels into 2...32 folds; one_se, the default, takes the largest lambda whose\n"
      "                       mean score is within <factor> standard errors over the folds of the least, min the least)\n"
      "                       [--regularizer_gradient=reference|exact] (reference, the default: the reference's regulariser\n"
      "                       gradients, bug for bug -- BTV of --btv_scale_range=1 then has none at all; exact: the gradient\n"
      "                       of the cost, srmap_problem_set_regularizer_gradient)\n"
      "                       [--affine_motion_path=<file>] (per-frame affine motion, 'a b tx c d ty' per line, HR pixels;\n"
      "                       an error together with --motion_sequence_path)\n"
      "                       [--flow_motion_path=<file>] (a dense displacement field per frame: raw little-endian float64,\n"
      "                       [frames][2][H][W] = the (ux, uy) planes in HR pixels at the high-resolution size; an error\n"
      "                       together with --motion_sequence_path, --affine_motion_path, --registration,\n"
      "                       --refine_motion_rounds, --fit_blur_from and --photometric_rounds)\n"
      "                       [--flow_lattice_path=<file>] (the same motion on a control lattice, generate_data's format: the\n"
      "                       solver keeps the nodes and interpolates them, srmap_problem_set_flow_lattice; an error with what\n"
      "                       --flow_motion_path is an error with, and with --flow_motion_path)\n"
      "                       [--registration=translational|affine|flow] (estimate the solver's motion from the LR frames, in\n"
      "                       HR pixels; with --generate_lr_images the motion files still generate the frames, without it\n"
      "                       an error together with either motion file.  flow: a dense displacement field per frame, and\n"
      "                       its validity masks as data weights of a least-squares solve (--data_loss=huber derives its own\n"
      "                       weights and runs without the masks); an error together with --motion_sequence_path,\n"
      "                       --affine_motion_path, --refine_motion_rounds, --fit_blur_from and --photometric_rounds)\n"
      "                       [--save_flow_path=<file>] (the estimated fields, in --flow_motion_path's format; needs\n"
      "                       --registration=flow)\n"
      "                       [--flow_lattice] (with --registration=flow: the estimate stays at the frames' resolution and is\n"
      "                       installed as a control lattice, srmap_problem_register_flow_lattice; --save_flow_path then\n"
      "                       writes the expanded field) [--save_flow_lattice_path=<file>] (the lattice itself, in\n"
      "                       --flow_lattice_path's format; needs --flow_lattice)\n"
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
      "                       [--noise_seed=1] [--save_initial_estimate=<path>]";

// The parsed command line; ParseFlags states the defaults.
struct Options {
  std::string data_path, ground_truth_image;
  bool generate_lr_images;
  double noise_sigma;
  int noise_seed, number_of_frames, upsampling_scale;
  // the model flags; --affine_motion_path and --flow_motion_path (srmap_problem_set_affine_motion, srmap_problem_set_flow) and
  // the free-form blur flags (srmap_problem_set_blur_kernel, srmap_problem_set_blur_bank) are not reference flags
  app::ModelFlags model;
  IRLSMapSolverOptions solver;
  std::string regularizer, solver_name;
  int btv_scale_range;
  double btv_spatial_decay, regularization_parameter;
  // not reference flags: the loss of the data term (the reference's is plain least squares) and the Huber threshold in the
  // solver's pixel units (ImageData scales 8-bit input to 0..1)
  std::string data_loss;
  double huber_delta;
  // not reference flags: the Huber threshold estimated from the residuals (srmap_problem_set_huber_scale; tuning and floor go
  // straight into `solver`), and the per-frame residual scales of the final estimate (srmap_residual_scale)
  std::string huber_scale;
  bool print_residual_scale;
  // not reference flags: the regularization parameter by hold-out validation (srmap_problem_set_holdout,
  // srmap_solve_lambda_path); lambda_path is the raw "<largest>:<ratio>:<count>"
  double holdout_fraction;
  unsigned long long holdout_seed;
  std::string holdout_seed_text;
  std::string lambda_path;
  // not reference flags: the same by k-fold cross-validation (srmap_solve_lambda_path_folds); an empty text: not given
  int holdout_folds;
  std::string lambda_rule, lambda_se_factor_text;
  int lambda_patience;
  bool print_lambda_path;
  // not a reference flag: the regulariser's gradient mode (srmap_problem_set_regularizer_gradient); empty: not given
  std::string regularizer_gradient;
  bool LambdaPath() const { return !lambda_path.empty(); }
  bool interpolate_color, solve_in_pca_space;
  int num_pca_components;
  double pca_retained_variance;
  std::string evaluators, result_path;
  // not a reference flag: the solver's start x0 as raw little-endian float64 [C][H][W], so that a CPU run of the
  // reference algorithm can start from the IDENTICAL estimate (tests/test_gpu_apps.py compares the two results)
  std::string save_initial_estimate;
  // not reference flags: estimate the solver's motion from the LR frames (srmap_register_translational /
  // srmap_register_affine / srmap_register_flow) instead of reading it from a file, and write the estimate out
  std::string registration, save_motion_path, save_flow_path;
  // not reference flags: --registration=flow kept on a control lattice (srmap_problem_register_flow_lattice), and its file
  bool flow_lattice;
  std::string save_flow_lattice_path;
  // not a reference flag: the validity masks as the persistent prior of srmap_set_data_prior (they hold under Huber too)
  bool flow_valid_prior;
  // not reference flags: joint motion refinement (srmap_refine_motion) around the solve
  int refine_motion_rounds, refine_motion_dof;
  // not reference flags: the calibration fits of the blur kernel (srmap_fit_blur) and of a bank (srmap_fit_blur_bank)
  std::string fit_blur_from, save_blur_kernel_path, fit_blur_bank_from, fit_blur_bank_mode, save_blur_bank_path;
  int fit_blur_ksize;
  // not reference flags: the photometric frame model (srmap_problem_set_photometric) and its fit (srmap_fit_photometric)
  std::string photometric_path, save_photometric_path;
  int photometric_rounds;
  bool verbose;

  bool RegisterFlow() const { return registration == "flow"; }
  bool RegisterFlowLattice() const { return RegisterFlow() && flow_lattice; }
  int FitBankMode() const {
    return fit_blur_bank_mode == "frame" ? 1 : fit_blur_bank_mode == "channel" ? 2 : fit_blur_bank_mode == "frame_channel" ? 3 : 0;
  }
};

// The images of a run, as the steps of main() hand them on.
struct Frames {
  ImageData high_res_image;  // the ground truth, if there is one
  std::vector<ImageData> low_res_images;
  ImageData upsampled_image;   // bilinear upsampling of frame 0 in the original spectral space: the evaluation baseline
  ImageData initial_estimate;  // the same in the space the solve runs in
  std::unique_ptr<SpectralPCA> spectral_pca;
  std::vector<double> flow_valid;  // --registration=flow: the validity masks, [frames][h][w] at LR resolution
  FlowLatticeSequence flow_lattice;  // --flow_lattice_path: the solver's motion, set once the solver exists
};

Options ParseFlags(int argc, char** argv) {
  app::Flags flags(argc, argv, kUsage);
  Options o{};
  o.data_path = flags.Str("data_path");
  o.generate_lr_images = flags.Bool("generate_lr_images", false);
  o.noise_sigma = flags.Double("noise_sigma", 0.0);
  o.noise_seed = flags.Int("noise_seed", 1);
  o.number_of_frames = flags.Int("number_of_frames", 4);
  o.ground_truth_image = flags.Str("ground_truth_image");
  o.upsampling_scale = flags.Int("upsampling_scale", 2);
  o.model = app::ReadModelFlags(&flags, 3, 1.0);
  o.model.parameters.scale = o.upsampling_scale;
  o.solver.max_num_irls_iterations = flags.Int("optimization_iterations", 20);
  o.solver.max_num_solver_iterations = flags.Int("solver_iterations", 50);
  o.solver.split_channels = flags.Bool("split_channels", false);
  o.regularizer = flags.Str("regularizer", "tv");
  o.btv_scale_range = flags.Int("btv_scale_range", 3);
  o.btv_spatial_decay = flags.Double("btv_spatial_decay", 0.5);
  o.regularization_parameter = flags.Double("regularization_parameter", 0.01);
  o.solver_name = flags.Str("solver", "cg");
  o.data_loss = flags.Str("data_loss", "l2");
  o.huber_delta = flags.Double("huber_delta", 0.02);
  o.huber_scale = flags.Str("huber_scale", "fixed");
  o.solver.huber_tuning = flags.Double("huber_tuning", 1.345);
  o.solver.huber_min_delta = flags.Double("huber_min_delta", 1.0e-4);
  o.print_residual_scale = flags.Bool("print_residual_scale", false);
  o.holdout_fraction = flags.Double("holdout_fraction", 0.0);
  o.holdout_seed_text = flags.Str("holdout_seed", "1");
  o.holdout_seed = std::strtoull(o.holdout_seed_text.c_str(), nullptr, 10);
  o.lambda_path = flags.Str("lambda_path", "");
  o.holdout_folds = flags.Int("holdout_folds", 0);
  o.lambda_rule = flags.Str("lambda_rule", "");
  o.lambda_se_factor_text = flags.Str("lambda_se_factor", "");
  o.lambda_patience = flags.Int("lambda_patience", 0);
  o.print_lambda_path = flags.Bool("print_lambda_path", false);
  o.regularizer_gradient = flags.Str("regularizer_gradient", "");
  o.interpolate_color = flags.Bool("interpolate_color", false);
  o.solve_in_pca_space = flags.Bool("solve_in_pca_space", false);
  o.num_pca_components = flags.Int("num_pca_components", 0);
  o.pca_retained_variance = flags.Double("pca_retained_variance", 0.0);
  o.evaluators = flags.Str("evaluators");
  o.result_path = flags.Str("result_path");
  o.save_initial_estimate = flags.Str("save_initial_estimate");
  o.registration = flags.Str("registration");
  o.save_motion_path = flags.Str("save_motion_path");
  o.save_flow_path = flags.Str("save_flow_path");
  o.flow_valid_prior = flags.Bool("flow_valid_prior", false);
  o.flow_lattice = flags.Bool("flow_lattice", false);
  o.save_flow_lattice_path = flags.Str("save_flow_lattice_path");
  o.refine_motion_rounds = flags.Int("refine_motion_rounds", 0);
  o.refine_motion_dof = flags.Int("refine_motion_dof", 6);
  o.fit_blur_from = flags.Str("fit_blur_from");
  o.fit_blur_ksize = flags.Int("fit_blur_ksize", 0);
  o.save_blur_kernel_path = flags.Str("save_blur_kernel_path");
  o.fit_blur_bank_from = flags.Str("fit_blur_bank_from");
  o.fit_blur_bank_mode = flags.Str("fit_blur_bank_mode");
  o.save_blur_bank_path = flags.Str("save_blur_bank_path");
  o.photometric_path = flags.Str("photometric_path");
  o.photometric_rounds = flags.Int("photometric_rounds", -1);
  o.save_photometric_path = flags.Str("save_photometric_path");
  o.verbose = flags.Bool("verbose", false);
  flags.RejectUnknown();
  flags.Require("data_path");
  return o;
}

// A displacement field IS the motion, whether --flow_motion_path reads it or --registration=flow estimates it: nothing else
// may give or estimate one, and the three fits have no sampling leg for a field.  The first such flag given, or nullptr.
const char* FlagExcludedByFlow(const Options& o, const bool registration_too) {
  const struct { const char* name; bool given; } excluded[] = {
      {"--motion_sequence_path", !o.model.parameters.motion_sequence_path.empty()},
      {"--affine_motion_path", !o.model.parameters.affine_motion_sequence_path.empty()},
      {"--registration", registration_too && !o.registration.empty()},
      {"--refine_motion_rounds", o.refine_motion_rounds != 0},
      {"--fit_blur_from", !o.fit_blur_from.empty()},
      {"--photometric_rounds", o.photometric_rounds >= 0}};
  for (const auto& flag : excluded)
    if (flag.given) return flag.name;
  return nullptr;
}

// The flag combinations that are refused before anything is loaded, in the order in which they win.
int CheckFlags(const Options& o) {
  using app::Refuse;
  const ImageModelParameters& model = o.model.parameters;
  const bool motion_file = !model.affine_motion_sequence_path.empty() || !model.motion_sequence_path.empty();
  if (app::RefuseBothMotionFiles(o.model)) return 1;
  if (!o.model.flow_motion_path.empty())
    if (const char* other = FlagExcludedByFlow(o, true)) return app::RefuseBoth("--flow_motion_path", other);
  if (app::RefuseBothFlowFiles(o.model)) return 1;
  if (!o.model.flow_lattice_path.empty())
    if (const char* other = FlagExcludedByFlow(o, true)) return app::RefuseBoth("--flow_lattice_path", other);
  if (!o.registration.empty() && o.registration != "translational" && o.registration != "affine" && !o.RegisterFlow())
    return Refuse("--registration is 'translational' or 'affine', or 'flow'.");
  if (o.RegisterFlow()) {
    if (const char* other = FlagExcludedByFlow(o, false)) return app::RefuseBoth("--registration=flow", other);
    if (!o.save_motion_path.empty())
      return Refuse("--save_motion_path holds matrices; the fields of --registration=flow go to --save_flow_path.");
  }
  if (!o.save_flow_path.empty() && !o.RegisterFlow()) return Refuse("--save_flow_path needs --registration=flow.");
  if (o.flow_valid_prior && !o.RegisterFlow()) return Refuse("--flow_valid_prior needs --registration=flow.");
  if (o.flow_lattice && !o.RegisterFlow()) return Refuse("--flow_lattice needs --registration=flow.");
  if (!o.save_flow_lattice_path.empty() && !o.RegisterFlowLattice()) return Refuse("--save_flow_lattice_path needs --registration=flow --flow_lattice.");
  if (!o.registration.empty() && !o.generate_lr_images && motion_file)
    return Refuse("--registration estimates the motion; it excludes --motion_sequence_path and --affine_motion_path "
                  "(except with --generate_lr_images, where the files generate the frames).");
  if (o.refine_motion_rounds < 0 || (o.refine_motion_dof != 2 && o.refine_motion_dof != 6))
    return Refuse("--refine_motion_rounds is >= 0 and --refine_motion_dof is 2 or 6.");
  if (!o.save_motion_path.empty() && o.registration.empty() && o.refine_motion_rounds == 0)
    return Refuse("--save_motion_path needs --registration or --refine_motion_rounds.");
  if (o.fit_blur_ksize < 0 || (o.fit_blur_ksize != 0 && o.fit_blur_ksize % 2 != 1) || o.fit_blur_ksize > 7)
    return Refuse("--fit_blur_ksize is 0 or an odd size up to 7.");
  if ((o.fit_blur_from.empty() && !o.save_blur_kernel_path.empty()) ||
      (o.fit_blur_from.empty() && o.fit_blur_bank_from.empty() && o.fit_blur_ksize != 0))
    return Refuse("--save_blur_kernel_path and --fit_blur_ksize need --fit_blur_from (--fit_blur_ksize also goes with --fit_blur_bank_from).");
  // the bank and the single kernel are alternatives, and so are their fits
  const char* bank_flag = !model.blur_bank_path.empty() ? "--blur_bank_path" : !o.fit_blur_bank_from.empty() ? "--fit_blur_bank_from" : nullptr;
  const char* kernel_flag = !model.blur_kernel_path.empty() ? "--blur_kernel_path" : !o.fit_blur_from.empty() ? "--fit_blur_from" : nullptr;
  if (bank_flag && kernel_flag) return app::RefuseBoth(bank_flag, kernel_flag);
  if (o.fit_blur_bank_from.empty() && (!o.fit_blur_bank_mode.empty() || !o.save_blur_bank_path.empty()))
    return Refuse("--fit_blur_bank_mode and --save_blur_bank_path need --fit_blur_bank_from.");
  if (!o.fit_blur_bank_from.empty() && o.FitBankMode() == 0)
    return Refuse("--fit_blur_bank_from needs --fit_blur_bank_mode=frame|channel|frame_channel.");
  if (!o.fit_blur_bank_from.empty() && (!o.model.flow_motion_path.empty() || !o.model.flow_lattice_path.empty() || o.RegisterFlow()))
    return Refuse("--fit_blur_bank_from has no sampling leg for a displacement field: not with --flow_motion_path or --registration=flow.");
  if (o.photometric_rounds < -1) return Refuse("--photometric_rounds is >= 0 (or -1: off).");
  if (!o.photometric_path.empty() && o.photometric_rounds >= 0)
    return Refuse("--photometric_path gives the parameters, --photometric_rounds fits them: they exclude each other.");
  if (!o.save_photometric_path.empty() && o.photometric_path.empty() && o.photometric_rounds < 0)
    return Refuse("--save_photometric_path needs --photometric_path or --photometric_rounds.");
  if (!o.regularizer_gradient.empty() && !srmap::reg_gradient_parse(o.regularizer_gradient.c_str(), nullptr))
    return Refuse("--regularizer_gradient is reference or exact.");
  // hold-out validation: refused here, before any GPU work
  if (o.holdout_fraction != 0.0 && srmap::holdout_threshold(o.holdout_fraction) == 0)
    return Refuse("--holdout_fraction is in (0, 0.5].");
  if (o.holdout_seed_text.empty() || o.holdout_seed_text.size() > 19 ||
      o.holdout_seed_text.find_first_not_of("0123456789") != std::string::npos)
    return Refuse("--holdout_seed is a non-negative integer of at most 19 digits.");
  if (o.holdout_folds != 0 && o.holdout_fraction != 0.0)
    return Refuse("--holdout_folds and --holdout_fraction exclude each other: folds partition the pixels, a fraction is one split.");
  if (o.holdout_folds != 0 && (o.holdout_folds < srmap::kHoldoutMinFolds || o.holdout_folds > srmap::kHoldoutMaxFolds))
    return Refuse("--holdout_folds is in 2...32.");
  if (o.holdout_folds == 0 && (!o.lambda_rule.empty() || !o.lambda_se_factor_text.empty()))
    return Refuse("--lambda_rule and --lambda_se_factor need --holdout_folds: one split gives no standard error over folds.");
  if (o.holdout_folds != 0) {
    int rule = 0;
    if (!o.lambda_rule.empty() && !srmap::holdout_parse_rule(o.lambda_rule.c_str(), &rule)) return Refuse("--lambda_rule is min or one_se.");
    if (!o.lambda_se_factor_text.empty() && !srmap::holdout_parse_se_factor(o.lambda_se_factor_text.c_str(), nullptr))
      return Refuse("--lambda_se_factor is a finite number >= 0.");
    if (!o.LambdaPath()) return Refuse("--holdout_folds needs --lambda_path.");
  }
  if (o.holdout_seed_text != "1" && o.holdout_fraction == 0.0 && o.holdout_folds == 0) return Refuse("--holdout_seed needs --holdout_fraction.");
  if (o.LambdaPath()) {
    double largest = 0.0, ratio = 0.0;
    int count = 0;
    if (!srmap::holdout_parse_lambda_path(o.lambda_path.c_str(), &largest, &ratio, &count))
      return Refuse("--lambda_path is <largest>:<ratio>:<count> with largest > 0, 0 < ratio < 1 and 1 <= count <= 32.");
    if (o.holdout_fraction == 0.0 && o.holdout_folds == 0) return Refuse("--lambda_path needs --holdout_fraction.");
    if (o.lambda_patience < 0) return Refuse("--lambda_patience is >= 0.");
    if (o.refine_motion_rounds > 0 || o.photometric_rounds >= 0)
      return Refuse("--lambda_path runs plain solves: not with --refine_motion_rounds or --photometric_rounds.");
  } else if (o.lambda_patience != 0 || o.print_lambda_path) {
    return Refuse("--lambda_patience and --print_lambda_path need --lambda_path.");
  }
  return 0;
}

// --solver and --data_loss: a name that is not known warns and runs the default
void ChooseSolverAndLoss(Options* o) {
  // super_resolution.cpp:134-141: "lbfgs" selects L-BFGS, anything but "cg" warns and falls back to CG
  if (o->solver_name == "lbfgs") o->solver.least_squares_solver = LBFGS_SOLVER;
  else if (o->solver_name != "cg") std::fprintf(stderr, "WARNING: Invalid solver flag. Using conjugate gradient solver.\n");
  // as --solver: "huber" selects the Huber loss, anything but "l2" warns and runs least squares
  if (o->data_loss == "huber") {
    o->solver.data_loss = HUBER_DATA_LOSS;
    o->solver.huber_delta = o->huber_delta;
  } else if (o->data_loss != "l2") {
    std::fprintf(stderr, "WARNING: Invalid data_loss flag. Using the least-squares (l2) data term.\n");
  }
  // likewise: "mad" estimates the Huber threshold from the residuals, anything but "fixed" warns and keeps --huber_delta
  if (o->huber_scale == "mad") o->solver.huber_scale = MAD_HUBER_SCALE;
  else if (o->huber_scale != "fixed") std::fprintf(stderr, "WARNING: Invalid huber_scale flag. Using the fixed --huber_delta.\n");
}

int NoLowResImages() {
  std::fprintf(stderr, "Check failed: At least one low-resolution image is required for super-resolution.\n");
  return 1;
}

// The HR image or the LR frames of --data_path, and the field of --flow_motion_path into the model parameters.
int LoadImages(Options* o, Frames* f) {
  if (o->generate_lr_images) f->high_res_image = util::LoadImage(o->data_path);
  else f->low_res_images = util::LoadImages(o->data_path);
  if (o->model.flow_motion_path.empty() && o->model.flow_lattice_path.empty()) return 0;
  // the field's file has no header: its size is checked against the HR geometry; the lattice is expanded at it
  if (!o->generate_lr_images && f->low_res_images.empty()) return NoLowResImages();
  const cv::Size hr = o->generate_lr_images ? f->high_res_image.GetImageSize()
                                            : cv::Size(f->low_res_images[0].GetImageSize().width * o->upsampling_scale,
                                                       f->low_res_images[0].GetImageSize().height * o->upsampling_scale);
  if (!o->model.flow_lattice_path.empty()) {
    // the solver is given the lattice itself (InstallLattice) and its model no motion; only a model that generates the
    // frames carries the expanded field
    f->flow_lattice.LoadSequenceFromFile(o->model.flow_lattice_path);
    if (o->generate_lr_images) o->model.parameters.flow_motion_sequence = f->flow_lattice.Expand(hr.width, hr.height);
    return 0;
  }
  o->model.parameters.flow_motion_sequence.LoadSequenceFromFile(o->model.flow_motion_path, hr.width, hr.height);
  return 0;
}

// The frames as the solver takes them: generated if asked for, in the space the solve runs in, with the initial estimate.
int PrepareFrames(const Options& o, Frames* f) {
  if (o.generate_lr_images) {  // data_path is the ground truth (super_resolution.cpp:285-299)
    // the generating model carries the AdditiveNoiseModule (sigma in 0..255 units), the solver's does not
    ImageModelParameters with_noise = o.model.parameters;
    with_noise.noise_sigma = o.noise_sigma;
    with_noise.noise_seed = static_cast<uint64_t>(o.noise_seed);
    const ImageModel image_model_with_noise = ImageModel::CreateImageModel(with_noise);
    for (int i = 0; i < o.number_of_frames; ++i)
      f->low_res_images.push_back(image_model_with_noise.ApplyToImage(f->high_res_image, i));
  } else if (!o.ground_truth_image.empty()) {
    f->high_res_image = util::LoadImage(o.ground_truth_image);
  }
  if (f->low_res_images.empty()) return NoLowResImages();

  f->upsampled_image = f->low_res_images[0];
  f->upsampled_image.ResizeImage(o.upsampling_scale, INTERPOLATE_LINEAR);

  // luminance-only colour path (super_resolution.cpp:330-342, 392-395): solve Y, interpolate Cr / Cb
  if (o.interpolate_color) {
    std::printf("Super-resolving only the luminance channel.\n");
    for (auto& frame : f->low_res_images) frame.ChangeColorSpace(SPECTRAL_MODE_COLOR_YCRCB, true);
  }
  // spectral PCA (super_resolution.cpp:344-366): solve on the leading components, reconstruct afterwards
  if (o.solve_in_pca_space && !o.interpolate_color) {
    if (o.pca_retained_variance > 0.0) f->spectral_pca.reset(new SpectralPCA(f->low_res_images, o.pca_retained_variance));
    else f->spectral_pca.reset(new SpectralPCA(f->low_res_images, o.num_pca_components));
    for (auto& frame : f->low_res_images) frame = f->spectral_pca->GetPCAImage(frame);
    std::printf("Super-resolving in PCA space with %d PCA components.\n", f->low_res_images[0].GetNumChannels());
  }

  f->initial_estimate = f->low_res_images[0];
  f->initial_estimate.ResizeImage(o.upsampling_scale, INTERPOLATE_LINEAR);
  if (!o.save_initial_estimate.empty()) {
    const std::vector<double> planar = f->initial_estimate.ToPlanar();
    std::FILE* file = std::fopen(o.save_initial_estimate.c_str(), "wb");
    if (!file || std::fwrite(planar.data(), sizeof(double), planar.size(), file) != planar.size())
      return app::CannotWrite(o.save_initial_estimate);
    std::fclose(file);
  }
  return 0;
}

int SaveMotion(const Options& o, const AffineMotionSequence& sequence) {
  return sequence.SaveToFile(o.save_motion_path) ? 0 : app::CannotWrite(o.save_motion_path);
}

// --registration: the solver's model takes its motion from the frames it is about to solve (channel 0), in HR pixels; the
// generating model keeps the motion files
int EstimateMotion(const Options& o, Frames* f, ImageModelParameters* solver_parameters) {
  if (o.RegisterFlowLattice()) {
    // the solver registers its own observations once it exists (InstallLattice); its model starts without a motion
  } else if (o.RegisterFlow()) {
    solver_parameters->flow_motion_sequence = registration::FlowRegistration(f->low_res_images, o.upsampling_scale, &f->flow_valid);
    double kept = 0.0;
    for (const double v : f->flow_valid) kept += v;
    std::printf("Estimated flow motion of %d frames from the low-resolution images; %.1f %% of the pixels are valid.\n",
                solver_parameters->flow_motion_sequence.GetNumMotions(), 100.0 * kept / static_cast<double>(f->flow_valid.size()));
    if (!o.save_flow_path.empty() && !solver_parameters->flow_motion_sequence.SaveToFile(o.save_flow_path))
      return app::CannotWrite(o.save_flow_path);
  } else if (!o.registration.empty()) {
    solver_parameters->motion_sequence_path.clear();
    solver_parameters->affine_motion_sequence_path.clear();
    AffineMotionSequence estimate;
    if (o.registration == "affine") {
      estimate = registration::AffineRegistration(f->low_res_images, o.upsampling_scale);
      solver_parameters->affine_motion_sequence = estimate;
    } else {
      const MotionShiftSequence lr_shifts = registration::TranslationalRegistration(f->low_res_images);
      std::vector<MotionShift> shifts;
      std::vector<AffineMotion> motions;
      for (int i = 0; i < lr_shifts.GetNumMotionShifts(); ++i) {
        shifts.push_back(MotionShift(o.upsampling_scale * lr_shifts[i].dx, o.upsampling_scale * lr_shifts[i].dy));
        motions.push_back(AffineMotion(1.0, 0.0, shifts.back().dx, 0.0, 1.0, shifts.back().dy));
      }
      solver_parameters->motion_sequence = MotionShiftSequence(shifts);
      estimate = AffineMotionSequence(motions);
    }
    std::printf("Estimated %s motion of %d frames from the low-resolution images.\n", o.registration.c_str(), estimate.GetNumMotions());
    // with refinement rounds the file holds the FINAL matrices: written after the solve
    if (!o.save_motion_path.empty() && o.refine_motion_rounds == 0) return SaveMotion(o, estimate);
  }
  return 0;
}

// --registration=flow --flow_lattice: channel 0 of the solver's own observations is registered on the device and the
// estimate installed as a control lattice, the validity masks as the data prior; the masks come back as f->flow_valid for
// SetUpSolver, which places them as the dense route does.  --flow_lattice_path: the lattice replaces the expanded field.
int InstallLattice(const Options& o, Frames* f, IRLSMapSolver* solver) {
  if (!f->flow_lattice.Empty()) {
    f->flow_lattice.Trim(solver->GetNumImages());
    solver->SetFlowLattice(f->flow_lattice);
  }
  if (!o.RegisterFlowLattice()) return 0;
  solver->RegisterFlowLattice(0, nullptr, true);
  const std::vector<double> prior = solver->GetDataPrior();  // [K][C][h][w], every channel the frame's mask
  solver->SetDataPrior(std::vector<double>());
  const size_t frames = static_cast<size_t>(solver->GetNumImages()), plane = prior.size() / (frames * solver->GetNumChannels());
  f->flow_valid.resize(frames * plane);
  double kept = 0.0;
  for (size_t k = 0; k < frames; ++k)
    for (size_t i = 0; i < plane; ++i) kept += f->flow_valid[k * plane + i] = prior[k * solver->GetNumChannels() * plane + i];
  const FlowLatticeSequence lattice = solver->GetFlowLattice();
  std::printf("Estimated flow motion of %d frames from the low-resolution images; %.1f %% of the pixels are valid.\n",
              lattice.GetNumMotions(), 100.0 * kept / static_cast<double>(f->flow_valid.size()));
  if (!o.save_flow_lattice_path.empty() && !lattice.SaveToFile(o.save_flow_lattice_path)) return app::CannotWrite(o.save_flow_lattice_path);
  if (!o.save_flow_path.empty()) {
    const cv::Size hr = f->initial_estimate.GetImageSize();
    if (!lattice.Expand(hr.width, hr.height).SaveToFile(o.save_flow_path)) return app::CannotWrite(o.save_flow_path);
  }
  return 0;
}

// --regularizer, and the validity masks of --registration=flow
void SetUpSolver(const Options& o, const Frames& f, IRLSMapSolver* solver) {
  double lambda = o.regularization_parameter, ratio = 0.0;
  int count = 0;
  if (o.LambdaPath()) srmap::holdout_parse_lambda_path(o.lambda_path.c_str(), &lambda, &ratio, &count);  // the largest: the path scales it
  if (lambda > 0.0) {
    std::shared_ptr<Regularizer> regularizer;
    if (o.regularizer == "btv") {
      regularizer = std::make_shared<BilateralTotalVariationRegularizer>(f.initial_estimate.GetImageSize(), o.btv_scale_range,
                                                                         o.btv_spatial_decay);
    } else {
      if (o.regularizer != "tv" && o.regularizer != "3dtv")
        std::fprintf(stderr, "WARNING: Unknown regularizer option '%s'. Using default Total Variation regularizer.\n",
                     o.regularizer.c_str());
      auto tv = std::make_shared<TotalVariationRegularizer>(f.initial_estimate.GetImageSize());
      if (o.regularizer == "3dtv") tv->SetUse3dTotalVariation(true);
      regularizer = tv;
    }
    solver->AddRegularizer(regularizer, lambda);
    int gradient_mode = 0;
    if (srmap::reg_gradient_parse(o.regularizer_gradient.c_str(), &gradient_mode)) solver->SetRegularizerGradient(0, gradient_mode);
  }
  // --registration=flow: the field is wrong where frame 0 does not hold the content; those pixels get weight 0.  A Huber
  // solve derives its own weights and resets the buffer (include/srmap.h) -- unless the masks are the persistent prior
  // (--flow_valid_prior, srmap_set_data_prior), which a Huber solve resets to and multiplies its weights by
  if (o.RegisterFlow() && o.flow_valid_prior) solver->SetDataPrior(f.flow_valid);
  else if (o.RegisterFlow() && o.solver.data_loss == L2_DATA_LOSS) solver->MultiplyDataWeights(f.flow_valid);
  // --holdout_fraction: that share of the pixels stays out of the data term (a factor of the prior, whatever the above set)
  if (o.holdout_fraction != 0.0) solver->SetHoldout(o.holdout_fraction, o.holdout_seed);
}

// The fits and the photometric model compare the frames with images in the frames' own channels.
int RefuseTransformedChannels(const Frames& f, const Options& o, const char* subject) {
  if (!o.interpolate_color && !f.spectral_pca) return 0;
  return app::Refuse("%s in the frames' own channels: not with --interpolate_color or --solve_in_pca_space.", subject);
}

// The calibration fits before the solve, from a known HR image of what the frames show, and --photometric_path
int CalibrateSolver(const Options& o, const Frames& f, IRLSMapSolver* solver) {
  BlurFitOptions fit_options;
  fit_options.ksize = o.fit_blur_ksize;
  std::vector<double> quality;
  if (!o.fit_blur_from.empty()) {
    if (RefuseTransformedChannels(f, o, "--fit_blur_from works")) return 1;
    const BlurKernel fitted = solver->FitBlur(util::LoadImage(o.fit_blur_from), fit_options, &quality);
    std::printf("Fitted a %d x %d blur kernel: cost %g -> %g, status %g.\n", fitted.GetSize(), fitted.GetSize(), quality[0], quality[1], quality[4]);
    if (!o.save_blur_kernel_path.empty() && !fitted.SaveToFile(o.save_blur_kernel_path)) return app::CannotWrite(o.save_blur_kernel_path);
  }
  // --fit_blur_bank_from: the same calibration fit per entry of a bank (a kernel per frame, per channel or per both)
  if (!o.fit_blur_bank_from.empty()) {
    if (RefuseTransformedChannels(f, o, "--fit_blur_bank_from works")) return 1;
    const BlurKernelBank fitted = solver->FitBlurBank(util::LoadImage(o.fit_blur_bank_from), o.FitBankMode(), fit_options, &quality);
    int degenerate = 0;
    for (int e = 0; e < fitted.GetNumEntries(); ++e) degenerate += quality[5 * e + 4] != 0.0;
    std::printf("Fitted a bank of %d %d x %d blur kernels (mode %s): %d degenerate.\n", fitted.GetNumEntries(), fitted.GetSize(),
                fitted.GetSize(), o.fit_blur_bank_mode.c_str(), degenerate);
    if (!o.save_blur_bank_path.empty() && !fitted.SaveToFile(o.save_blur_bank_path)) return app::CannotWrite(o.save_blur_bank_path);
  }
  if (!o.photometric_path.empty() || o.photometric_rounds >= 0)
    if (RefuseTransformedChannels(f, o, "the photometric flags work")) return 1;
  if (!o.photometric_path.empty()) {  // known exposure, in force for every solve below
    PhotometricSequence known;
    known.LoadSequenceFromFile(o.photometric_path);
    solver->SetPhotometric(known);
  }
  return 0;
}

// The solve, with the photometric and motion refinement rounds asked for, back in the frames' original channels.
int Solve(const Options& o, const Frames& f, IRLSMapSolver* solver, ImageData* result) {
  std::printf("Super-resolving from %zu images...\n", f.low_res_images.size());
  const auto start_time = std::chrono::steady_clock::now();
  MotionRefinementOptions refinement;
  refinement.dof = o.refine_motion_dof;
  AffineMotionSequence refined;
  // with --photometric_rounds every round fits the exposure, refines the motion, then solves; the larger count rules
  const int rounds = std::max(o.refine_motion_rounds, o.photometric_rounds);
  if (o.photometric_rounds >= 0) {
    PhotometricSequence fitted;
    *result = solver->SolvePhotometricJoint(f.initial_estimate, rounds, o.refine_motion_rounds > 0, PhotometricFitOptions(), refinement,
                                            &fitted, &refined);
    std::printf("Fitted gain and bias of %d frames in %d rounds.\n", fitted.GetNumFrames(), rounds);
  } else if (o.refine_motion_rounds > 0) {
    *result = solver->SolveJoint(f.initial_estimate, rounds, refinement, &refined);
  } else if (o.LambdaPath() && o.holdout_folds != 0) {
    double largest = 0.0, ratio = 0.0, se_factor = 1.0;
    int count = 0, chosen = -1, rule = SRMAP_LAMBDA_RULE_ONE_SE;
    srmap::holdout_parse_lambda_path(o.lambda_path.c_str(), &largest, &ratio, &count);
    if (!o.lambda_rule.empty()) srmap::holdout_parse_rule(o.lambda_rule.c_str(), &rule);
    if (!o.lambda_se_factor_text.empty()) srmap::holdout_parse_se_factor(o.lambda_se_factor_text.c_str(), &se_factor);
    std::vector<double> scales(count), table;
    for (int j = 0; j < count; ++j) scales[j] = std::pow(ratio, j);
    *result = solver->SolveLambdaPathFolds(f.initial_estimate, scales, o.holdout_folds, o.holdout_seed, rule, se_factor, o.lambda_patience,
                                           &table, nullptr, &chosen);
    const size_t rows = table.size() / SRMAP_LAMBDA_PATH_ROW;
    std::vector<double> mean(rows), se(rows);
    for (size_t j = 0; j < rows; ++j) {
      mean[j] = table[j * SRMAP_LAMBDA_PATH_ROW + 1];
      se[j] = table[j * SRMAP_LAMBDA_PATH_ROW + 2];
    }
    const int least = srmap::holdout_choose(mean.data(), static_cast<int>(rows));
    std::printf("Lambda path, %d folds, rule %s: %zu of %d rows, chosen lambda %.9g (row %d, mean score %.9g +- %.9g; least mean at row %d).\n",
                o.holdout_folds, rule == SRMAP_LAMBDA_RULE_ONE_SE ? "one_se" : "min", rows, count, largest * scales[chosen], chosen,
                mean[chosen], se[chosen], least);
    if (o.print_lambda_path)
      for (size_t j = 0; j < rows; ++j) {
        const double* r = table.data() + j * SRMAP_LAMBDA_PATH_ROW;
        std::printf("  lambda %.9g: mean score %.9g +- %.9g over %.0f held-out pixels, %.0f IRLS rounds, %.0f iterations, %.0f evaluations, "
                    "delta %.9g%s%s\n", largest * r[0], r[1], r[2], r[6], r[7], r[8], r[9], r[10],
                    static_cast<int>(j) == least ? "  <- least mean" : "", static_cast<int>(j) == chosen ? "  <- chosen" : "");
      }
  } else if (o.LambdaPath()) {
    double largest = 0.0, ratio = 0.0;
    int count = 0, chosen = -1;
    srmap::holdout_parse_lambda_path(o.lambda_path.c_str(), &largest, &ratio, &count);
    std::vector<double> scales(count), table;
    for (int j = 0; j < count; ++j) scales[j] = std::pow(ratio, j);
    *result = solver->SolveLambdaPath(f.initial_estimate, scales, o.lambda_patience, true, &table, &chosen);
    const size_t rows = table.size() / SRMAP_LAMBDA_PATH_ROW;
    std::printf("Lambda path: %zu of %d rows, chosen lambda %.9g (row %d, hold-out score %.9g).\n", rows, count,
                largest * scales[chosen], chosen, table[chosen * SRMAP_LAMBDA_PATH_ROW + 1]);
    if (o.print_lambda_path)
      for (size_t j = 0; j < rows; ++j) {
        const double* r = table.data() + j * SRMAP_LAMBDA_PATH_ROW;
        std::printf("  lambda %.9g: score %.9g over %.0f held-out pixels, %.0f IRLS rounds, %.0f iterations, %.0f evaluations, "
                    "final cost %.9g, delta %.9g\n", largest * r[0], r[1], r[5], r[6], r[7], r[8], r[9], r[10]);
      }
  } else {
    *result = solver->Solve(f.initial_estimate);
  }
  if (o.refine_motion_rounds > 0) {
    std::printf("Refined the motion of %d frames in %d rounds.\n", refined.GetNumMotions(), rounds);
    if (!o.save_motion_path.empty() && SaveMotion(o, refined)) return 1;
  }
  if (!o.save_photometric_path.empty() && !solver->GetPhotometric().SaveToFile(o.save_photometric_path))
    return app::CannotWrite(o.save_photometric_path);
  const std::chrono::duration<double> elapsed = std::chrono::steady_clock::now() - start_time;
  std::printf("Done! Finished in %g seconds.\n", elapsed.count());
  if (o.solver.data_loss == HUBER_DATA_LOSS && o.solver.huber_scale == MAD_HUBER_SCALE)
    std::printf("Huber delta of the last re-weighting: %.9g\n", solver->HuberDelta());
  if (o.holdout_fraction != 0.0)  // of the final estimate, with the loss the solve ran with
    std::printf("Hold-out score of the result: %.9g\n", solver->HoldoutScore(*result)[0]);
  if (o.print_residual_scale) {  // of the final estimate, in the space the solve ran in: a frame that stands out fits badly
    const std::vector<double> scales = solver->ResidualScale(*result);
    std::printf("Residual scale (1.4826 median|r|) over all frames: %.9g\n", scales[0]);
    for (size_t k = 1; k < scales.size(); ++k) std::printf("  frame %zu: %.9g\n", k - 1, scales[k]);
  }
  if (o.interpolate_color) {
    result->InterpolateColorFrom(f.initial_estimate);
    result->ChangeColorSpace(SPECTRAL_MODE_COLOR_BGR);
  }
  if (f.spectral_pca) *result = f.spectral_pca->ReconstructImage(*result);
  return 0;
}

// --evaluators against the ground truth: the bilinear baseline and the result
void Evaluate(const Options& o, const Frames& f, const ImageData& result) {
  size_t pos = 0;
  while (pos <= o.evaluators.size()) {
    const size_t comma = o.evaluators.find(',', pos);
    const std::string evaluator = util::TrimString(o.evaluators.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
    if (evaluator == "psnr") {
      const PeakSignalToNoiseRatioEvaluator psnr_evaluator(f.high_res_image);
      std::cout << "PSNR score on upsampled: " << psnr_evaluator.Evaluate(f.upsampled_image) << std::endl;
      std::cout << "PSNR score on result:    " << psnr_evaluator.Evaluate(result) << std::endl;
    } else if (evaluator == "ssim") {
      const StructuralSimilarityEvaluator ssim_evaluator(f.high_res_image);
      std::cout << "SSIM score on upsampled: " << ssim_evaluator.Evaluate(f.upsampled_image) << std::endl;
      std::cout << "SSIM score on result:    " << ssim_evaluator.Evaluate(result) << std::endl;
    } else if (!evaluator.empty()) {
      std::fprintf(stderr, "ERROR: Unknown/unsupported evaluator '%s'.\n", evaluator.c_str());
    }
    if (comma == std::string::npos) break;
    pos = comma + 1;
  }
}

}  // namespace

int main(int argc, char** argv) {
  Options options = ParseFlags(argc, argv);
  if (CheckFlags(options)) return 1;
  ChooseSolverAndLoss(&options);

  Frames frames;
  if (LoadImages(&options, &frames)) return 1;
  const ImageModel image_model = ImageModel::CreateImageModel(options.model.parameters);
  if (PrepareFrames(options, &frames)) return 1;

  ImageModelParameters solver_parameters = options.model.parameters;
  if (EstimateMotion(options, &frames, &solver_parameters)) return 1;
  // --flow_lattice_path: the solver never holds the expanded field, on the host or on the device
  if (!frames.flow_lattice.Empty()) solver_parameters.flow_motion_sequence = FlowMotionSequence();
  const bool own_model = !options.registration.empty() || !frames.flow_lattice.Empty();
  const ImageModel solver_model = own_model ? ImageModel::CreateImageModel(solver_parameters) : image_model;

  IRLSMapSolver solver(options.solver, solver_model, frames.low_res_images, options.verbose);
  if (InstallLattice(options, &frames, &solver)) return 1;
  SetUpSolver(options, frames, &solver);
  if (CalibrateSolver(options, frames, &solver)) return 1;

  ImageData result;
  if (Solve(options, frames, &solver, &result)) return 1;
  const bool has_ground_truth = !options.ground_truth_image.empty() || options.generate_lr_images;
  if (has_ground_truth && !options.evaluators.empty()) Evaluate(options, frames, result);
  if (!options.result_path.empty()) util::SaveImage(result, options.result_path);
  return 0;
}
