// Solver / MapSolver / IRLSMapSolver and their option structs
// (src/optimization/solver.h:14-43, map_solver.{h,cpp}, irls_map_solver.{h,cpp}),
// evaluated on the GPU through the C ABI; the term-by-term classes
// (ObjectiveFunction / ObjectiveTerm / ObjectiveDataTerm /
// ObjectiveIRLSRegularizationTerm) live in optimization/objective_function.h.
// Both least-squares solvers of the reference run on the GPU: CG (mincg) and
// L-BFGS (minlbfgs, num_lbfgs_hessian_corrections pairs), chosen as in
// irls_map_solver.cpp:97-113.  Analytical differentiation only: the reference's
// numeric-difference variant is a test-only alternative outside the path.
// Not in the reference: RefineMotion / SolveJoint, the joint motion refinement of include/srmap.h (srmap_refine_motion),
// FitBlur, the calibration fit of the blur kernel (srmap_fit_blur), SetBlurBank / FitBlurBank, a blur kernel per frame and /
// or channel and its fit (srmap_problem_set_blur_bank, srmap_fit_blur_bank), and SetPhotometric / FitPhotometric / SolvePhotometric /
// SolvePhotometricJoint, the photometric frame model (srmap_problem_set_photometric, srmap_fit_photometric).
#pragma once
#include <cmath>
#include <iostream>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "image/image_data.h"
#include "image_model/image_model.h"
#include "image_model/photometric.h"
#include "motion/affine_motion.h"
#include "motion/flow_lattice.h"
#include "optimization/objective_function.h"
#include "optimization/regularizer.h"
#include "util/srmap_host.h"

namespace super_resolution {

enum LeastSquaresSolver { CG_SOLVER, LBFGS_SOLVER };
// Loss of the data term.  Not in the reference (its data term is plain least squares): HUBER_DATA_LOSS re-weights the
// observations between the inner solves as the regulariser is re-weighted (srmap_problem_set_data_loss, include/srmap.h).
enum DataLoss { L2_DATA_LOSS, HUBER_DATA_LOSS };
enum HuberScale { FIXED_HUBER_SCALE, MAD_HUBER_SCALE };

struct MapSolverOptions {
  MapSolverOptions() {}
  virtual ~MapSolverOptions() = default;
  virtual void AdjustThresholdsAdaptively(const int num_parameters, const double regularization_parameter_sum) {
    const double threshold_scale = num_parameters * regularization_parameter_sum;
    if (threshold_scale < 1.0) return;
    gradient_norm_threshold *= threshold_scale;
    cost_decrease_threshold *= threshold_scale;
    parameter_variation_threshold *= threshold_scale;
  }
  virtual void PrintSolverOptions() const {
    std::cout << "  Least squares solver:                "
              << (least_squares_solver == LBFGS_SOLVER ? "L-BFGS" : "conjugate gradient") << " (analytical differentiation)\n"
              << "  Threshold 1 (gradient norm):         " << gradient_norm_threshold << "\n"
              << "  Threshold 2 (cost decrease):         " << cost_decrease_threshold << "\n"
              << "  Threshold 3 (parameter variation):   " << parameter_variation_threshold << std::endl;
  }
  LeastSquaresSolver least_squares_solver = CG_SOLVER;
  int num_lbfgs_hessian_corrections = 5;
  int max_num_solver_iterations = 50;
  double gradient_norm_threshold = 1.0e-6;
  double cost_decrease_threshold = 1.0e-6;
  double parameter_variation_threshold = 1.0e-6;
  bool use_numerical_differentiation = false;
  double numerical_differentiation_step = 1.0e-6;
  bool split_channels = false;
};

struct IRLSMapSolverOptions : public MapSolverOptions {
  IRLSMapSolverOptions() {}
  void AdjustThresholdsAdaptively(const int num_parameters, const double regularization_parameter_sum) override {
    const double threshold_scale = num_parameters * regularization_parameter_sum;
    if (threshold_scale < 1.0) return;
    MapSolverOptions::AdjustThresholdsAdaptively(num_parameters, regularization_parameter_sum);
    irls_cost_difference_threshold *= threshold_scale;
  }
  int max_num_irls_iterations = 20;
  double irls_cost_difference_threshold = 1.0e-5;
  // not in the reference: robust data term (default: the reference's least squares)
  DataLoss data_loss = L2_DATA_LOSS;
  double huber_delta = 0.02;  // in the units of the observations; read for HUBER_DATA_LOSS only
  // where a Huber solve takes its delta from (srmap_problem_set_huber_scale): huber_delta above, or -- MAD_HUBER_SCALE --
  // max(huber_tuning * 1.4826 median|r|, huber_min_delta) of the residuals over all frames, re-estimated at every re-weighting
  HuberScale huber_scale = FIXED_HUBER_SCALE;
  double huber_tuning = 1.345;
  double huber_min_delta = 1.0e-4;
};

// Options of IRLSMapSolver::RefineMotion (srmap_motion_refinement_options, include/srmap.h).  Not in the reference.
struct MotionRefinementOptions {
  int dof = 6;                    // 6: the full 2 x 3 matrix; 2: the translation only
  int max_iterations = 30;        // trial passes per frame after the initial pass
  double step_tolerance = 1.0e-4; // HR px at the image corners
  double initial_damping = 1.0e-3;
};

// Options of IRLSMapSolver::FitBlur (srmap_blur_fit_options, include/srmap.h).  Not in the reference.
struct BlurFitOptions {
  int ksize = 0;           // 0: the size of the solver's current kernel
  bool sum_to_one = true;
  double ridge = 0.0;
};

// Options of IRLSMapSolver::FitPhotometric (srmap_photometric_fit_options, include/srmap.h).  Not in the reference.
struct PhotometricFitOptions {
  int model = 0;         // 0: gain and bias; 1: gain only; 2: bias only
  int gauge_frame = 0;   // this frame keeps its parameters; -1: none
  double min_gain = 0.25;
  double max_gain = 4.0;
};

class Solver {
 public:
  explicit Solver(const ImageModel& image_model, const bool verbose = true)
      : image_model_(image_model), is_verbose_(verbose) {}
  virtual ~Solver() = default;
  virtual ImageData Solve(const ImageData& initial_estimate) = 0;
  virtual void Stfu() { is_verbose_ = false; }
  virtual bool IsVerbose() const { return is_verbose_; }

 protected:
  const ImageModel& image_model_;  // the caller keeps the model alive (solver.h:37)
  bool is_verbose_ = true;
};

class MapSolver : public Solver {
 public:
  MapSolver(const ImageModel& image_model, const std::vector<ImageData>& low_res_images,
            const bool print_solver_output = true)
      : Solver(image_model, print_solver_output) {
    if (low_res_images.empty()) srmap_host::Fail("Cannot super-resolve with 0 low-res images.");
    num_channels_ = low_res_images[0].GetNumChannels();
    for (const ImageData& im : low_res_images)
      if (im.GetNumChannels() != num_channels_) srmap_host::Fail("Image channel counts do not match up.");
    const int s = image_model_.GetDownsamplingScale();
    const cv::Size lr = low_res_images[0].GetImageSize();
    image_size_ = cv::Size(lr.width * s, lr.height * s);
    // The library keeps the observations at LR resolution (the reference stores
    // them NN-upsampled, map_solver.cpp:80-85; algebraically identical).
    problem_ = srmap_host::MakeSolverProblem(image_model_, low_res_images.size(), image_size_, num_channels_, "MapSolver");
    std::vector<double> stack;
    for (const ImageData& im : low_res_images) {
      if (im.GetImageSize() != lr) srmap_host::Fail("observation sizes differ");
      const std::vector<double> planar = im.ToPlanar();
      stack.insert(stack.end(), planar.begin(), planar.end());
    }
    num_images_ = static_cast<int>(low_res_images.size());
    srmap_host::Check(srmap_set_observations(problem_.get(), stack.data()), "srmap_set_observations");
  }
  virtual void AddRegularizer(std::shared_ptr<Regularizer> regularizer, const double regularization_parameter) {
    regularizers_.push_back(std::make_pair(regularizer, regularization_parameter));
    int kind = 0, range = 0;
    double decay = 0;
    regularizer->Describe(&kind, &range, &decay);
    srmap_host::Check(srmap_add_regularizer(problem_.get(), kind, regularization_parameter, range, decay, nullptr),
                      "srmap_add_regularizer");
  }
  int GetNumPixels() const { return image_size_.width * image_size_.height; }
  cv::Size GetImageSize() const { return image_size_; }
  int GetNumChannels() const { return num_channels_; }
  int GetNumImages() const { return num_images_; }
  int GetNumDataPoints() const {
    const long n = static_cast<long>(GetNumPixels()) * GetNumChannels();
    if (n > std::numeric_limits<int>::max()) srmap_host::Fail("Number of data points exceeds maximum size.");
    return static_cast<int>(n);
  }
  double GetRegularizationParameterSum() const {
    double sum = 0.0;
    for (const auto& r : regularizers_) sum += r.second;
    return sum;
  }
  // ObjectiveFunction::ComputeAllTerms on the current term set
  // (objective_function.cpp:5-20); gradient may be nullptr.
  double ComputeAllTerms(const double* estimated_image_data, double* gradient = nullptr) const {
    double cost = 0;
    srmap_host::Check(srmap_eval(problem_.get(), SRMAP_TERM_ALL, estimated_image_data, &cost, gradient), "srmap_eval");
    return cost;
  }
  srmap_problem* problem() const { return problem_.get(); }

 protected:
  std::vector<std::pair<std::shared_ptr<Regularizer>, double>> regularizers_;
  srmap_host::ProblemPtr problem_;

 private:
  cv::Size image_size_;
  int num_channels_ = 0;
  int num_images_ = 0;
};

class IRLSMapSolver : public MapSolver {
 public:
  IRLSMapSolver(const IRLSMapSolverOptions& solver_options, const ImageModel& image_model,
                const std::vector<ImageData>& low_res_images, const bool print_solver_output = true)
      : MapSolver(image_model, low_res_images, print_solver_output), solver_options_(solver_options) {}

  // irls_map_solver.cpp:192-265
  ImageData Solve(const ImageData& initial_estimate) override {
    CheckGeometry(initial_estimate, "initial estimate does not match the HR geometry");
    const srmap_irls_options o = PrepareSolve();
    const std::vector<double> x0 = initial_estimate.ToPlanar();
    std::vector<double> x(x0.size());
    srmap_host::Check(srmap_solve(problem_.get(), &o, x0.data(), x.data(), &report_), "srmap_solve");
    ReportSolve();
    ImageData result;
    result.FromPlanar(x, GetImageSize(), GetNumChannels());
    return result;
  }
  const srmap_solve_report& GetReport() const { return report_; }
  // Hold-out validation (srmap_problem_set_holdout; not in the reference): the share `fraction` (0 < fraction <= 0.5) of the
  // observations, chosen by a hash of (index, seed), is kept out of the data term of every later solve and evaluation;
  // 0 lifts the hold-out.
  void SetHoldout(const double fraction, const unsigned long long seed = 1) {
    srmap_host::Check(srmap_problem_set_holdout(problem_.get(), fraction, seed), "srmap_problem_set_holdout");
  }
  // The score of the held-out observations at `estimate` (srmap_holdout_score): 1 + K numbers, [0] over all frames, [1 + k]
  // of frame k.  delta 0: the mean squared residual; > 0: the mean Huber function; < 0: the loss the solver would solve
  // with (solver_options: 0 under L2, huber_delta under a fixed Huber scale, the last Huber step's delta under MAD).
  // sums (optional): (1 + K) x 4 = S1, S2, S0, n.
  std::vector<double> HoldoutScore(const ImageData& estimate, const double delta = -1.0, std::vector<double>* sums = nullptr) {
    CheckGeometry(estimate, "estimate does not match the HR geometry");
    if (delta < 0.0) PrepareSolve();  // "the problem's" loss is the options'
    const std::vector<double> x = estimate.ToPlanar();
    std::vector<double> score(1 + static_cast<size_t>(GetNumImages())), s(4 * score.size());
    srmap_host::Check(srmap_holdout_score(problem_.get(), x.data(), delta, score.data(), s.data()), "srmap_holdout_score");
    if (sums) *sums = s;
    return score;
  }
  // The regularization parameter of regulariser `index` (the order of AddRegularizer), changed in place
  // (srmap_problem_set_regularizer_lambda; the reference fixes it at AddRegularizer).
  void SetRegularizationParameter(const int index, const double regularization_parameter) {
    srmap_host::Check(srmap_problem_set_regularizer_lambda(problem_.get(), index, regularization_parameter),
                      "srmap_problem_set_regularizer_lambda");
  }
  double GetRegularizationParameter(const int index) const {
    double lambda = 0.0;
    srmap_host::Check(srmap_problem_get_regularizer_lambda(problem_.get(), index, &lambda), "srmap_problem_get_regularizer_lambda");
    return lambda;
  }
  // The gradient regulariser `index` contributes (srmap_problem_set_regularizer_gradient; no reference counterpart):
  // SRMAP_REG_GRADIENT_REFERENCE, the reference's bug for bug (the default), or SRMAP_REG_GRADIENT_EXACT, the gradient of
  // the cost.  The cost, the values and the IRLS weights are the same in both.
  void SetRegularizerGradient(const int index, const int mode) {
    srmap_host::Check(srmap_problem_set_regularizer_gradient(problem_.get(), index, mode), "srmap_problem_set_regularizer_gradient");
  }
  int GetRegularizerGradient(const int index) const {
    int mode = 0;
    srmap_host::Check(srmap_problem_get_regularizer_gradient(problem_.get(), index, &mode), "srmap_problem_get_regularizer_gradient");
    return mode;
  }
  // The regularization parameters by hold-out validation (srmap_solve_lambda_path): one solve from initial_estimate per
  // multiplier in `scales` (strictly decreasing) of every regulariser's parameter, scored on the held-out observations;
  // the result is the solve on all observations at the chosen parameters (final_solve) or the chosen row's solution.  The
  // chosen parameters stay set.  table (optional): rows of SRMAP_LAMBDA_PATH_ROW doubles; chosen (optional): the row.
  ImageData SolveLambdaPath(const ImageData& initial_estimate, const std::vector<double>& scales, const int patience = 0,
                            const bool final_solve = true, std::vector<double>* table = nullptr, int* chosen = nullptr) {
    CheckGeometry(initial_estimate, "initial estimate does not match the HR geometry");
    const srmap_irls_options o = PrepareSolve();
    srmap_lambda_path_options po;
    srmap_lambda_path_options_default(&po);
    if (scales.empty() || scales.size() > SRMAP_LAMBDA_PATH_MAX_SCALES) srmap_host::Fail("SolveLambdaPath: between 1 and 32 scales");
    po.num_scales = static_cast<int>(scales.size());
    for (int j = 0; j < SRMAP_LAMBDA_PATH_MAX_SCALES; ++j) po.scales[j] = j < po.num_scales ? scales[j] : 0.0;
    po.patience = patience;
    po.final_solve = final_solve ? 1 : 0;
    const std::vector<double> x0 = initial_estimate.ToPlanar();
    std::vector<double> x(x0.size()), rows(scales.size() * SRMAP_LAMBDA_PATH_ROW);
    int rows_run = 0, row = -1;
    srmap_host::Check(srmap_solve_lambda_path(problem_.get(), &o, &po, x0.data(), x.data(), rows.data(), &rows_run, &row, &report_),
                      "srmap_solve_lambda_path");
    rows.resize(static_cast<size_t>(rows_run) * SRMAP_LAMBDA_PATH_ROW);
    if (table) *table = rows;
    if (chosen) *chosen = row;
    if (IsVerbose()) std::cout << "IRLSMapSolver: lambda path, " << rows_run << " rows, chosen scale " << scales[row] << std::endl;
    ReportSolve();
    ImageData result;
    result.FromPlanar(x, GetImageSize(), GetNumChannels());
    return result;
  }
  // A hold-out given as fold `fold` of the partition of the observations into `folds` (2...32) folds
  // (srmap_problem_set_holdout_fold); folds 0 lifts the hold-out.  A fold and a fraction replace each other.
  void SetHoldoutFold(const int folds, const int fold, const unsigned long long seed = 1) {
    srmap_host::Check(srmap_problem_set_holdout_fold(problem_.get(), folds, fold, seed), "srmap_problem_set_holdout_fold");
  }
  // The regularization parameters by k-fold cross-validation (srmap_solve_lambda_path_folds): per multiplier in `scales`
  // one solve from initial_estimate and one score for every fold; rule SRMAP_LAMBDA_RULE_MIN chooses the least mean score,
  // SRMAP_LAMBDA_RULE_ONE_SE the largest parameter whose mean is within se_factor standard errors over the folds of it.
  // The result is the solve on all observations at the chosen parameters, which stay set; the hold-out is as it was.
  // table (optional): rows {scale, mean, se, pooled S1, S2, S0, n, rounds, iterations, evaluations, delta}; fold_table
  // (optional): [scale][fold] rows in SolveLambdaPath's layout; chosen (optional): the row.
  ImageData SolveLambdaPathFolds(const ImageData& initial_estimate, const std::vector<double>& scales, const int folds = 5,
                                 const unsigned long long seed = 1, const int rule = SRMAP_LAMBDA_RULE_ONE_SE,
                                 const double se_factor = 1.0, const int patience = 0, std::vector<double>* table = nullptr,
                                 std::vector<double>* fold_table = nullptr, int* chosen = nullptr) {
    CheckGeometry(initial_estimate, "initial estimate does not match the HR geometry");
    const srmap_irls_options o = PrepareSolve();
    srmap_lambda_cv_options po;
    srmap_lambda_cv_options_default(&po);
    if (scales.empty() || scales.size() > SRMAP_LAMBDA_PATH_MAX_SCALES) srmap_host::Fail("SolveLambdaPathFolds: between 1 and 32 scales");
    if (folds < 2 || folds > 32) srmap_host::Fail("SolveLambdaPathFolds: between 2 and 32 folds");
    po.num_scales = static_cast<int>(scales.size());
    for (int j = 0; j < SRMAP_LAMBDA_PATH_MAX_SCALES; ++j) po.scales[j] = j < po.num_scales ? scales[j] : 0.0;
    po.folds = folds;
    po.seed = seed;
    po.rule = rule;
    po.se_factor = se_factor;
    po.patience = patience;
    const std::vector<double> x0 = initial_estimate.ToPlanar();
    std::vector<double> x(x0.size()), rows(scales.size() * SRMAP_LAMBDA_PATH_ROW), fold_rows(rows.size() * static_cast<size_t>(folds));
    int rows_run = 0, row = -1;
    srmap_host::Check(srmap_solve_lambda_path_folds(problem_.get(), &o, &po, x0.data(), x.data(), rows.data(), fold_rows.data(),
                                                    &rows_run, &row, &report_),
                      "srmap_solve_lambda_path_folds");
    rows.resize(static_cast<size_t>(rows_run) * SRMAP_LAMBDA_PATH_ROW);
    fold_rows.resize(rows.size() * static_cast<size_t>(folds));
    if (table) *table = rows;
    if (fold_table) *fold_table = fold_rows;
    if (chosen) *chosen = row;
    if (IsVerbose())
      std::cout << "IRLSMapSolver: lambda path, " << folds << " folds, " << rows_run << " rows, chosen scale " << scales[row] << std::endl;
    ReportSolve();
    ImageData result;
    result.FromPlanar(x, GetImageSize(), GetNumChannels());
    return result;
  }

 private:
  // solver_options as srmap_irls_options, and the solver, loss and Huber scale they name set on the problem
  srmap_irls_options PrepareSolve() {
    srmap_irls_options o;
    srmap_irls_options_default(&o);
    o.max_num_solver_iterations = solver_options_.max_num_solver_iterations;
    o.gradient_norm_threshold = solver_options_.gradient_norm_threshold;
    o.cost_decrease_threshold = solver_options_.cost_decrease_threshold;
    o.parameter_variation_threshold = solver_options_.parameter_variation_threshold;
    o.split_channels = solver_options_.split_channels ? 1 : 0;
    o.max_num_irls_iterations = solver_options_.max_num_irls_iterations;
    o.irls_cost_difference_threshold = solver_options_.irls_cost_difference_threshold;
    if (solver_options_.use_numerical_differentiation)
      srmap_host::Fail("only analytical differentiation is provided");
    // LeastSquaresSolver -> srmap_solver (irls_map_solver.cpp:97-113); an out-of-range value is refused by the library
    srmap_host::Check(srmap_problem_set_solver(problem_.get(),
                                               solver_options_.least_squares_solver == LBFGS_SOLVER ? SRMAP_SOLVER_LBFGS
                                               : solver_options_.least_squares_solver == CG_SOLVER  ? SRMAP_SOLVER_CG
                                                                                                     : -1,
                                               solver_options_.num_lbfgs_hessian_corrections),
                      "srmap_problem_set_solver");
    srmap_host::Check(srmap_problem_set_data_loss(problem_.get(),
                                                  solver_options_.data_loss == HUBER_DATA_LOSS ? SRMAP_DATA_LOSS_HUBER
                                                  : solver_options_.data_loss == L2_DATA_LOSS  ? SRMAP_DATA_LOSS_L2
                                                                                               : -1,
                                                  solver_options_.huber_delta),
                      "srmap_problem_set_data_loss");
    srmap_host::Check(srmap_problem_set_huber_scale(problem_.get(),
                                                    solver_options_.huber_scale == MAD_HUBER_SCALE     ? SRMAP_HUBER_DELTA_MAD
                                                    : solver_options_.huber_scale == FIXED_HUBER_SCALE ? SRMAP_HUBER_DELTA_FIXED
                                                                                                       : -1,
                                                    solver_options_.huber_tuning, solver_options_.huber_min_delta),
                      "srmap_problem_set_huber_scale");
    return o;
  }
  void ReportSolve() const {
    if (IsVerbose())
      std::cout << "IRLSMapSolver: " << report_.irls_rounds << " IRLS rounds, " << report_.cg_iterations
                << (solver_options_.least_squares_solver == LBFGS_SOLVER ? " L-BFGS" : " CG") << " iterations, " << report_.evaluations << " cost+gradient evaluations, final cost "
                << report_.final_cost << std::endl;
  }

 public:
  // Joint motion refinement (srmap_refine_motion; not in the reference): the frame matrices re-fitted to `estimate`
  // through the forward model, starting from the solver's current motion, and INSTALLED as the solver's motion (later
  // solves and ComputeAllTerms run the affine model with them).  quality (optional): 4 numbers per frame -- cost at the
  // start, cost at the result, passes, status.
  AffineMotionSequence RefineMotion(const ImageData& estimate, const MotionRefinementOptions& options = MotionRefinementOptions(),
                                    std::vector<double>* quality = nullptr) {
    CheckGeometry(estimate, "estimate does not match the HR geometry");
    srmap_motion_refinement_options o;
    srmap_motion_refinement_options_default(&o);
    o.dof = options.dof;
    o.max_iterations = options.max_iterations;
    o.step_tolerance = options.step_tolerance;
    o.initial_damping = options.initial_damping;
    o.apply = 1;
    const std::vector<double> x = estimate.ToPlanar();
    std::vector<double> flat(static_cast<size_t>(GetNumImages()) * 6), q(static_cast<size_t>(GetNumImages()) * 4);
    srmap_host::Check(srmap_refine_motion(problem_.get(), x.data(), &o, flat.data(), q.data(), nullptr), "srmap_refine_motion");
    std::vector<AffineMotion> motions;
    for (int i = 0; i < GetNumImages(); ++i) {
      const double* m = flat.data() + 6 * static_cast<size_t>(i);
      motions.push_back(AffineMotion(m[0], m[1], m[2], m[3], m[4], m[5]));
      if (IsVerbose())
        std::cout << "  frame " << i << ": cost " << q[4 * i] << " -> " << q[4 * i + 1] << ", " << q[4 * i + 2] << " passes, status "
                  << q[4 * i + 3] << std::endl;
    }
    if (quality) *quality = q;
    return AffineMotionSequence(motions);
  }
  // Calibration fit of the blur kernel (srmap_fit_blur; not in the reference): the taps that best explain the solver's
  // observations from the KNOWN high-resolution image `hr` under the solver's motion and data weights, INSTALLED as the
  // solver's blur (later solves and ComputeAllTerms use them).  quality (optional): E at the kernel in force, E at the fit,
  // smallest / largest pivot, status (3: no texture -- the kernel stays and is returned).
  BlurKernel FitBlur(const ImageData& hr, const BlurFitOptions& options = BlurFitOptions(), std::vector<double>* quality = nullptr) {
    CheckGeometry(hr, "the high-resolution image does not match the HR geometry");
    int ksize = 0;
    const srmap_blur_fit_options o = BlurFit(options, &ksize);
    const std::vector<double> x = hr.ToPlanar();
    std::vector<double> taps(TapsOf(ksize)), q(5);
    srmap_host::Check(srmap_fit_blur(problem_.get(), x.data(), &o, taps.data(), q.data(), nullptr), "srmap_fit_blur");
    if (IsVerbose())
      std::cout << "Blur fit (" << ksize << " x " << ksize << "): cost " << q[0] << " -> " << q[1] << ", pivots " << q[2] << " ... " << q[3]
                << ", status " << q[4] << std::endl;
    if (quality) *quality = q;
    return BlurKernel(ksize, taps);
  }
  // A blur-kernel bank for the solver (srmap_problem_set_blur_bank; not in the reference): it replaces the model's blur
  // for later solves, fits and ComputeAllTerms.  The entries must fit the solver's frames and channels.
  void SetBlurBank(const BlurKernelBank& bank) {
    if (bank.Empty()) srmap_host::Fail("SetBlurBank: the blur bank is empty");
    if (static_cast<size_t>(bank.GetNumEntries()) != srmap_host::BankEntryCount(bank.GetMode(), GetNumImages(), GetNumChannels()))
      srmap_host::Fail("SetBlurBank: the number of entries does not fit the solver's frames and channels");
    srmap_host::Check(srmap_problem_set_blur_bank(problem_.get(), bank.GetMode(), bank.GetSize(), bank.GetTaps().data()), "srmap_problem_set_blur_bank");
  }
  // Calibration fit of a blur-kernel bank (srmap_fit_blur_bank; not in the reference): FitBlur's fit, separately over the
  // observations of each entry of `mode` (1 per frame, 2 per channel, 3 per frame and channel), from the KNOWN
  // high-resolution image `hr`, INSTALLED as the solver's blur.  quality (optional): 5 numbers per entry, FitBlur's (status
  // 3: the entry is degenerate and keeps its kernel).  Like FitBlur a calibration fit: blind alternation is not offered.
  BlurKernelBank FitBlurBank(const ImageData& hr, const int mode, const BlurFitOptions& options = BlurFitOptions(), std::vector<double>* quality = nullptr) {
    CheckGeometry(hr, "the high-resolution image does not match the HR geometry");
    if (mode < SRMAP_BLUR_PER_FRAME || mode > SRMAP_BLUR_PER_FRAME_CHANNEL) srmap_host::Fail("FitBlurBank: the mode is 1, 2 or 3");
    int ksize = 0;
    const srmap_blur_fit_options o = BlurFit(options, &ksize);
    const int entries = static_cast<int>(srmap_host::BankEntryCount(mode, GetNumImages(), GetNumChannels()));
    const std::vector<double> x = hr.ToPlanar();
    std::vector<double> taps(TapsOf(ksize) * entries), q(5 * static_cast<size_t>(entries));
    srmap_host::Check(srmap_fit_blur_bank(problem_.get(), x.data(), mode, &o, taps.data(), q.data(), nullptr), "srmap_fit_blur_bank");
    if (IsVerbose())
      for (int e = 0; e < entries; ++e)
        std::cout << "Blur bank fit, entry " << e << " (" << ksize << " x " << ksize << "): cost " << q[5 * e] << " -> " << q[5 * e + 1]
                  << ", status " << q[5 * e + 4] << std::endl;
    if (quality) *quality = q;
    return BlurKernelBank(mode, ksize, entries, taps);
  }
  // Solve, then `rounds` times (RefineMotion at the current estimate, Solve warm-started from it).  motion (optional)
  // receives the final matrices (untouched when rounds == 0).  Not in the reference.
  ImageData SolveJoint(const ImageData& initial_estimate, const int rounds,
                       const MotionRefinementOptions& options = MotionRefinementOptions(), AffineMotionSequence* motion = nullptr) {
    if (rounds < 0) srmap_host::Fail("the number of motion refinement rounds must not be negative");
    ImageData x = Solve(initial_estimate);
    for (int r = 0; r < rounds; ++r) {
      if (IsVerbose()) std::cout << "Motion refinement round " << (r + 1) << " of " << rounds << ":" << std::endl;
      const AffineMotionSequence refined = RefineMotion(x, options);
      if (motion) *motion = refined;
      x = Solve(x);
    }
    return x;
  }
  // Photometric frame model (srmap_problem_set_photometric; not in the reference): later solves and ComputeAllTerms run
  // against the frames normalised by these per-frame (gain, bias) pairs.  An empty sequence restores the raw frames.
  void SetPhotometric(const PhotometricSequence& photometric) {
    if (photometric.Empty()) {
      srmap_host::Check(srmap_problem_set_photometric(problem_.get(), nullptr), "srmap_problem_set_photometric");
      return;
    }
    if (photometric.GetNumFrames() < GetNumImages()) srmap_host::Fail("fewer photometric (gain, bias) pairs than observations");
    std::vector<double> flat = photometric.Flat();
    flat.resize(static_cast<size_t>(GetNumImages()) * 2);
    srmap_host::Check(srmap_problem_set_photometric(problem_.get(), flat.data()), "srmap_problem_set_photometric");
  }
  // The parameters in force (ones and zeros when none are set).
  PhotometricSequence GetPhotometric() const {
    std::vector<double> flat(static_cast<size_t>(GetNumImages()) * 2);
    srmap_host::Check(srmap_problem_get_photometric(problem_.get(), flat.data(), nullptr), "srmap_problem_get_photometric");
    return PhotometricSequence(flat.data(), GetNumImages());
  }
  // Fit of the per-frame gain and bias to `estimate` (srmap_fit_photometric; not in the reference), from the RAW frames
  // under the solver's motion, blur and data weights, INSTALLED as SetPhotometric would.  quality (optional): 4 numbers per
  // frame -- cost at the parameters in force, cost at the result, sum of the weights, status.
  PhotometricSequence FitPhotometric(const ImageData& estimate, const PhotometricFitOptions& options = PhotometricFitOptions(),
                                     std::vector<double>* quality = nullptr) {
    CheckGeometry(estimate, "estimate does not match the HR geometry");
    srmap_photometric_fit_options o;
    srmap_photometric_fit_options_default(&o);
    o.model = options.model;
    o.gauge_frame = options.gauge_frame;
    o.min_gain = options.min_gain;
    o.max_gain = options.max_gain;
    o.apply = 1;
    const std::vector<double> x = estimate.ToPlanar();
    std::vector<double> flat(static_cast<size_t>(GetNumImages()) * 2), q(static_cast<size_t>(GetNumImages()) * 4);
    srmap_host::Check(srmap_fit_photometric(problem_.get(), x.data(), &o, flat.data(), q.data(), nullptr), "srmap_fit_photometric");
    if (IsVerbose())
      for (int i = 0; i < GetNumImages(); ++i)
        std::cout << "  frame " << i << ": gain " << flat[2 * i] << ", bias " << flat[2 * i + 1] << ", cost " << q[4 * i] << " -> "
                  << q[4 * i + 1] << ", status " << q[4 * i + 3] << std::endl;
    if (quality) *quality = q;
    return PhotometricSequence(flat.data(), GetNumImages());
  }
  // FitPhotometric at the initial estimate, Solve, then `rounds` times (FitPhotometric at the current estimate, Solve
  // warm-started from it).  photometric (optional) receives the final parameters.  Not in the reference.
  ImageData SolvePhotometric(const ImageData& initial_estimate, const int rounds,
                             const PhotometricFitOptions& options = PhotometricFitOptions(), PhotometricSequence* photometric = nullptr) {
    return SolvePhotometricJoint(initial_estimate, rounds, false, options, MotionRefinementOptions(), photometric, nullptr);
  }
  // The same with the motion refined as well: every round runs FitPhotometric, then (refine_motion) RefineMotion, then the
  // warm Solve.  SolveJoint above is the motion-only loop.  Not in the reference.
  ImageData SolvePhotometricJoint(const ImageData& initial_estimate, const int rounds, const bool refine_motion,
                                  const PhotometricFitOptions& fit_options = PhotometricFitOptions(),
                                  const MotionRefinementOptions& refinement_options = MotionRefinementOptions(),
                                  PhotometricSequence* photometric = nullptr, AffineMotionSequence* motion = nullptr) {
    if (rounds < 0) srmap_host::Fail("the number of photometric rounds must not be negative");
    if (IsVerbose()) std::cout << "Photometric fit at the initial estimate:" << std::endl;
    PhotometricSequence fitted = FitPhotometric(initial_estimate, fit_options);
    ImageData x = Solve(initial_estimate);
    for (int r = 0; r < rounds; ++r) {
      if (IsVerbose()) std::cout << "Photometric round " << (r + 1) << " of " << rounds << ":" << std::endl;
      fitted = FitPhotometric(x, fit_options);
      if (refine_motion) {
        const AffineMotionSequence refined = RefineMotion(x, refinement_options);
        if (motion) *motion = refined;
      }
      x = Solve(x);
    }
    if (photometric) *photometric = fitted;
    return x;
  }
  // The data weights, one planar [C][h][w] block per observation ([K][C][h][w]): after a Huber solve the outlier map (the
  // pixels the solve down-weighted); all ones for a least-squares solve.  Not in the reference.
  std::vector<double> GetDataWeights() const {
    std::vector<double> w(static_cast<size_t>(GetNumImages()) * GetNumChannels() * LrPlane());
    srmap_host::Check(srmap_get_data_weights(problem_.get(), w.data()), "srmap_get_data_weights");
    return w;
  }
  // The residual scale of `estimate` (srmap_residual_scale; not in the reference): 1 + K numbers, [0] 1.4826 x the median of
  // |A x - y| over all counted observations, [1 + k] the same of frame k alone -- a frame that fits worse than the others
  // stands out.  counts (optional): the 1 + K numbers of counted observations.
  std::vector<double> ResidualScale(const ImageData& estimate, std::vector<double>* counts = nullptr) {
    CheckGeometry(estimate, "estimate does not match the HR geometry");
    const std::vector<double> x = estimate.ToPlanar();
    std::vector<double> scales(1 + static_cast<size_t>(GetNumImages())), n(scales.size());
    srmap_host::Check(srmap_residual_scale(problem_.get(), x.data(), scales.data(), n.data()), "srmap_residual_scale");
    if (counts) *counts = n;
    return scales;
  }
  // The delta of the last Huber re-weighting (srmap_problem_get_huber_delta): the fixed one, or the last estimate of the
  // MAD_HUBER_SCALE mode; scales / counts (optional): the 1 + K scales and counts it was formed from (zeros in the fixed mode).
  double HuberDelta(std::vector<double>* scales = nullptr, std::vector<double>* counts = nullptr) const {
    std::vector<double> s(1 + static_cast<size_t>(GetNumImages())), n(s.size());
    double delta = 0.0;
    srmap_host::Check(srmap_problem_get_huber_delta(problem_.get(), nullptr, &delta, s.data(), n.data()), "srmap_problem_get_huber_delta");
    if (scales) *scales = s;
    if (counts) *counts = n;
    return delta;
  }
  // Multiplies per-observation masks [K][h][w] at LR resolution (registration::FlowRegistration's validity masks) into the
  // data weights, broadcast over the channels: the weights in force (the caller's, ones if none were set) times the mask.
  // Not in the reference.  A Huber solve owns the weight buffer and resets it (include/srmap.h): masks act on
  // least-squares solves only.
  void MultiplyDataWeights(const std::vector<double>& masks) {
    const std::vector<double> m = BroadcastMasks(masks, "data weight masks: one [h][w] plane per observation at the low-resolution size is needed");
    std::vector<double> w = GetDataWeights();
    for (size_t i = 0; i < w.size(); ++i) w[i] *= m[i];
    srmap_host::Check(srmap_set_data_weights(problem_.get(), w.data()), "srmap_set_data_weights");
  }
  // Installs per-observation masks [K][h][w] at LR resolution, broadcast over the channels as MultiplyDataWeights does, as
  // the PERSISTENT prior on the data weights (srmap_set_data_prior, include/srmap.h): every kernel reads prior .* weights,
  // and a Huber solve resets to the prior and re-weights to prior .* huber(r) -- the masks hold under both losses.  An
  // empty vector removes the prior.  Not in the reference.
  void SetDataPrior(const std::vector<double>& masks) {
    if (masks.empty()) {
      srmap_host::Check(srmap_set_data_prior(problem_.get(), nullptr), "srmap_set_data_prior");
      return;
    }
    const std::vector<double> m = BroadcastMasks(masks, "data prior masks: one [h][w] plane per observation at the low-resolution size is needed");
    srmap_host::Check(srmap_set_data_prior(problem_.get(), m.data()), "srmap_set_data_prior");
  }
  // The prior in force, [K][C][h][w]; empty when none is set.  Not in the reference.
  std::vector<double> GetDataPrior() const {
    int set = 0;
    srmap_host::Check(srmap_get_data_prior(problem_.get(), nullptr, &set), "srmap_get_data_prior");
    if (!set) return std::vector<double>();
    std::vector<double> m(static_cast<size_t>(GetNumImages()) * GetNumChannels() * LrPlane());
    srmap_host::Check(srmap_get_data_prior(problem_.get(), m.data(), &set), "srmap_get_data_prior");
    return m;
  }
  // Registers the solver's own observations on the device (srmap_problem_register_flow): the plane of `channel` (-1: the
  // channel mean), the field installed as the problem's motion and -- with `prior` -- the validity masks as the data
  // prior.  options (optional): a filled srmap_flow_registration_options.  Returns the quality, 3 per image.  Not in the
  // reference.
  std::vector<double> RegisterFlow(const int channel = -1, const srmap_flow_registration_options* options = nullptr,
                                   const bool prior = true) {
    std::vector<double> quality(3 * static_cast<size_t>(GetNumImages()), 0.0);
    srmap_host::Check(srmap_problem_register_flow(problem_.get(), channel, options, prior ? 1 : 0, quality.data()),
                      "srmap_problem_register_flow");
    return quality;
  }
  // Installs a displacement field on a control lattice as the solver's motion (srmap_problem_set_flow_lattice): it replaces
  // whatever motion the model gave, and evaluates bit for bit as the model over lattice.Expand(HR size) does.  An empty
  // sequence restores the model's motion.  The lattice holds at least one frame per observation; the rest is dropped.  Not
  // in the reference.
  void SetFlowLattice(const FlowLatticeSequence& lattice) {
    if (lattice.Empty()) {
      srmap_host::Check(srmap_problem_set_flow_lattice(problem_.get(), 0, 0, 0, nullptr), "srmap_problem_set_flow_lattice");
      return;
    }
    if (lattice.GetNumMotions() < GetNumImages()) srmap_host::Fail("flow lattice: fewer frames than observations");
    srmap_host::Check(srmap_problem_set_flow_lattice(problem_.get(), lattice.GetStep(), lattice.GetLatticeWidth(), lattice.GetLatticeHeight(),
                                                     lattice.Flat().data()),
                      "srmap_problem_set_flow_lattice");
  }
  // The lattice in force; empty when none is set.  Not in the reference.
  FlowLatticeSequence GetFlowLattice() const {
    int step = 0, lw = 0, lh = 0;
    srmap_host::Check(srmap_problem_get_flow_lattice(problem_.get(), &step, &lw, &lh, nullptr), "srmap_problem_get_flow_lattice");
    if (step == 0) return FlowLatticeSequence();
    std::vector<double> nodes(static_cast<size_t>(GetNumImages()) * 2 * lw * lh);
    srmap_host::Check(srmap_problem_get_flow_lattice(problem_.get(), &step, &lw, &lh, nodes.data()), "srmap_problem_get_flow_lattice");
    return FlowLatticeSequence(nodes, step, lw, lh);
  }
  // RegisterFlow that stops at the input level (srmap_problem_register_flow_lattice): the estimate is installed as a
  // lattice with step = the scale on the LR grid, without forming the HR field.  Not in the reference.
  std::vector<double> RegisterFlowLattice(const int channel = -1, const srmap_flow_registration_options* options = nullptr,
                                          const bool prior = true) {
    std::vector<double> quality(3 * static_cast<size_t>(GetNumImages()), 0.0);
    srmap_host::Check(srmap_problem_register_flow_lattice(problem_.get(), channel, options, prior ? 1 : 0, quality.data()),
                      "srmap_problem_register_flow_lattice");
    return quality;
  }

 private:
  void CheckGeometry(const ImageData& image, const char* message) const {
    if (image.GetNumChannels() != GetNumChannels() || image.GetImageSize() != GetImageSize()) srmap_host::Fail(message);
  }
  // BlurFitOptions as the library takes them, applied; *ksize: the size of the fit (ksize 0: that of the kernel in force)
  srmap_blur_fit_options BlurFit(const BlurFitOptions& options, int* ksize) const {
    srmap_blur_fit_options o;
    srmap_blur_fit_options_default(&o);
    o.ksize = options.ksize;
    o.sum_to_one = options.sum_to_one ? 1 : 0;
    o.ridge = options.ridge;
    o.apply = 1;
    *ksize = options.ksize;
    if (*ksize == 0) srmap_host::Check(srmap_problem_get_blur_kernel(problem_.get(), ksize, nullptr), "srmap_problem_get_blur_kernel");
    return o;
  }
  static size_t TapsOf(const int ksize) { return static_cast<size_t>(ksize > 0 ? ksize : 1) * (ksize > 0 ? ksize : 1); }
  // pixels of one low-resolution plane
  size_t LrPlane() const {
    int lw = 0, lh = 0;
    srmap_host::Check(srmap_problem_lr_size(problem_.get(), &lw, &lh), "srmap_problem_lr_size");
    return static_cast<size_t>(lw) * lh;
  }
  // [K][h][w] masks at LR resolution as [K][C][h][w]: every channel of an observation gets its mask
  std::vector<double> BroadcastMasks(const std::vector<double>& masks, const char* message) const {
    const size_t plane = LrPlane(), channels = static_cast<size_t>(GetNumChannels());
    if (masks.size() != static_cast<size_t>(GetNumImages()) * plane) srmap_host::Fail(message);
    std::vector<double> m(static_cast<size_t>(GetNumImages()) * channels * plane);
    for (size_t k = 0; k < static_cast<size_t>(GetNumImages()); ++k)
      for (size_t c = 0; c < channels; ++c)
        for (size_t i = 0; i < plane; ++i) m[(k * channels + c) * plane + i] = masks[k * plane + i];
    return m;
  }
  const IRLSMapSolverOptions solver_options_;
  srmap_solve_report report_ = {};
};

}  // namespace super_resolution
