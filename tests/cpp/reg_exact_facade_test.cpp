// reg_exact_facade_test.cpp -- the host side of the regularisers' gradient mode.  Without an argument (no GPU needed;
// tests/test_reg_exact_host.py): the mode words and the dispatch rule of csrc/reg_gradient_host.hpp.  With the argument
// `gpu` (tests/test_gpu_reg_exact.py): IRLSMapSolver::SetRegularizerGradient / GetRegularizerGradient must be, bit for bit,
// srmap_problem_set_regularizer_gradient on a second solver's problem.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "image_model/image_model.h"
#include "optimization/irls_map_solver.h"
#include "optimization/regularizer.h"
#include "reg_gradient_host.hpp"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static void HostRules() {
  int mode = 7;
  EXPECT(srmap::reg_gradient_parse("reference", &mode) && mode == SRMAP_REG_GRADIENT_REFERENCE);
  EXPECT(srmap::reg_gradient_parse("exact", &mode) && mode == SRMAP_REG_GRADIENT_EXACT);
  EXPECT(srmap::reg_gradient_parse("exact", nullptr));
  mode = 7;
  for (const char* bad : {"", "Exact", "EXACT", "exact ", " exact", "exac", "exactly", "ref", "1", "0", "true"})
    EXPECT(!srmap::reg_gradient_parse(bad, &mode) && mode == 7);
  EXPECT(!srmap::reg_gradient_parse(nullptr, &mode) && mode == 7);
  EXPECT(std::strcmp(srmap::reg_gradient_name(SRMAP_REG_GRADIENT_REFERENCE), "reference") == 0);
  EXPECT(std::strcmp(srmap::reg_gradient_name(SRMAP_REG_GRADIENT_EXACT), "exact") == 0);
  EXPECT(srmap::reg_gradient_name(2) == nullptr && srmap::reg_gradient_name(-1) == nullptr);
  EXPECT(srmap::kRegGradientReference == SRMAP_REG_GRADIENT_REFERENCE && srmap::kRegGradientExact == SRMAP_REG_GRADIENT_EXACT);
  // the four-pixel kernel: ranges 1 .. 3, whole cells, every array on a 4-element boundary
  const uintptr_t a = 4096;
  for (int R = 0; R <= 5; ++R) EXPECT(srmap::btv_exact4_serves(R, 64, 16, 8, a, a, a, a) == (R >= 1 && R <= 3));
  for (int W = 1; W <= 13; ++W) EXPECT(srmap::btv_exact4_serves(2, W, 5, 4, a, a, 0, 0) == (W % 4 == 0));
  EXPECT(srmap::btv_exact4_serves(3, 4, 1, 8, a, a, 0, 0));      // one cell; no weights, cost only
  EXPECT(!srmap::btv_exact4_serves(3, 64, 16, 8, a, 0, a, a));    // no values: nothing to gather
  EXPECT(!srmap::btv_exact4_serves(3, 64, 16, 8, a + 8, a, a, a));  // f64: 32-byte boundary
  EXPECT(!srmap::btv_exact4_serves(3, 64, 16, 8, a, a + 16, a, a));
  EXPECT(!srmap::btv_exact4_serves(3, 64, 16, 8, a, a, a + 24, a));
  EXPECT(!srmap::btv_exact4_serves(3, 64, 16, 8, a, a, a, a + 8));
  EXPECT(srmap::btv_exact4_serves(3, 64, 16, 4, a + 16, a + 32, a, a + 48));  // f32: 16-byte boundary
  EXPECT(!srmap::btv_exact4_serves(3, 64, 16, 4, a + 4, a, a, a));
  EXPECT(srmap::btv_exact4_serves(1, 65536, 131068, 4, a, a, 0, a));   // cells just below 2^31 - 1
  EXPECT(!srmap::btv_exact4_serves(1, 65536, 131072, 4, a, a, 0, a));  // 2^31 cells
}

// frame k: a smooth scene moved by (0.5 k, -0.25 k) LR pixels, plus a deterministic ripple standing in for noise
static std::vector<double> Frame(const int k, const int W, const int H) {
  std::vector<double> px(static_cast<size_t>(W) * H);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double x = c + 0.5 * k, y = r - 0.25 * k;
      px[static_cast<size_t>(r) * W + c] = 0.5 + 0.2 * std::sin(0.31 * x) * std::cos(0.23 * y) + 0.15 * std::sin(0.13 * (x + y)) +
                                           0.03 * std::sin(12.9898 * c + 78.233 * r + 37.719 * k);
    }
  return px;
}

static int Gpu() {
  const int w = 32, h = 24, K = 4, scale = 2;
  std::vector<ImageData> frames;
  std::vector<MotionShift> shifts;
  for (int k = 0; k < K; ++k) {
    const std::vector<double> px = Frame(k, w, h);
    frames.push_back(ImageData(px.data(), cv::Size(w, h)));
    shifts.push_back(MotionShift(1.0 * k, -1.0 * (k % 2)));
  }
  ImageModelParameters params;
  params.scale = scale;
  params.blur_radius = 3;
  params.blur_sigma = 1.0;
  params.motion_sequence = MotionShiftSequence(shifts);
  const ImageModel model = ImageModel::CreateImageModel(params);
  IRLSMapSolverOptions options;
  options.max_num_irls_iterations = 3;
  options.max_num_solver_iterations = 10;
  ImageData start = frames[0];
  start.ResizeImage(scale, INTERPOLATE_LINEAR);
  for (const int range : {1, 3}) {
    IRLSMapSolver facade(options, model, frames, false), calls(options, model, frames, false), reference(options, model, frames, false);
    for (IRLSMapSolver* s : {&facade, &calls, &reference})
      s->AddRegularizer(std::make_shared<BilateralTotalVariationRegularizer>(start.GetImageSize(), range, 0.5), 0.02);
    EXPECT(facade.GetRegularizerGradient(0) == SRMAP_REG_GRADIENT_REFERENCE);
    facade.SetRegularizerGradient(0, SRMAP_REG_GRADIENT_EXACT);
    EXPECT(facade.GetRegularizerGradient(0) == SRMAP_REG_GRADIENT_EXACT);
    EXPECT(srmap_problem_set_regularizer_gradient(calls.problem(), 0, SRMAP_REG_GRADIENT_EXACT) == SRMAP_OK);
    int mode = -1;
    EXPECT(srmap_problem_get_regularizer_gradient(facade.problem(), 0, &mode) == SRMAP_OK && mode == SRMAP_REG_GRADIENT_EXACT);
    const ImageData a = facade.Solve(start), b = calls.Solve(start), c = reference.Solve(start);
    EXPECT(a.ToPlanar() == b.ToPlanar());
    EXPECT(facade.GetReport().final_cost == calls.GetReport().final_cost && facade.GetReport().evaluations == calls.GetReport().evaluations);
    EXPECT(a.ToPlanar() != c.ToPlanar());
    EXPECT(facade.GetRegularizerGradient(0) == SRMAP_REG_GRADIENT_EXACT);  // it persists across the solve
    // what the facade's Check would abort on (as the reference's CHECKs do): the C calls' answers
    EXPECT(srmap_problem_set_regularizer_gradient(facade.problem(), 0, 2) == SRMAP_EINVAL);
    EXPECT(srmap_problem_set_regularizer_gradient(facade.problem(), 1, SRMAP_REG_GRADIENT_EXACT) == SRMAP_EINVAL);
    EXPECT(facade.GetRegularizerGradient(0) == SRMAP_REG_GRADIENT_EXACT);
  }
  return 0;
}

int main(int argc, char** argv) {
  HostRules();
  if (argc > 1 && std::strcmp(argv[1], "gpu") == 0) Gpu();
  std::printf(g_fail ? "REG EXACT FACADE TESTS FAILED (%d)\n" : "REG EXACT FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
