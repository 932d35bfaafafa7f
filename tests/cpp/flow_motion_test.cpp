// flow_motion_test.cpp -- host side of the displacement-field motion model (super-resolution_amd/host/motion/flow_motion.h,
// the MotionModule constructor over it, ImageModelParameters::flow_motion_sequence): the raw float64 file and its size check
// against the geometry, index errors, the error for a model given two kinds of motion, and ImageModel::Canonical() carrying
// the field to the C ABI's chain.  No GPU needed: nothing here applies an operator.  argv[1] = scratch directory; argv[2]
// (optional) names ONE case that must abort the process with a "Check failed" message:
// index | pixel | both | wrong_size | empty_file | missing_file | wrong_geometry -- or `gpu`: the MotionModule and
// IRLSMapSolver over a flow sequence against the C entry points (tests/test_gpu_flow.py).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "image_model/image_model.h"
#include "motion/flow_motion.h"
#include "optimization/irls_map_solver.h"
#include "optimization/regularizer.h"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static std::vector<double> Field(const int K, const int W, const int H) {
  std::vector<double> f(static_cast<size_t>(K) * 2 * W * H);
  for (size_t i = 0; i < f.size(); ++i) f[i] = 0.001 * static_cast<double>(i) - 0.25;
  return f;
}

static std::string WriteRaw(const std::string& dir, const std::string& name, const void* data, const size_t bytes) {
  const std::string path = dir + "/" + name;
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (f) {
    if (bytes) std::fwrite(data, 1, bytes, f);
    std::fclose(f);
  }
  return path;
}

static void TestFile(const std::string& dir) {
  const int K = 3, W = 7, H = 5;
  const std::vector<double> f = Field(K, W, H);
  FlowMotionSequence seq;
  EXPECT(seq.Empty() && seq.GetNumMotions() == 0);
  seq.LoadSequenceFromFile(WriteRaw(dir, "flow3.bin", f.data(), f.size() * sizeof(double)), W, H);
  EXPECT(!seq.Empty() && seq.GetNumMotions() == K && seq.GetWidth() == W && seq.GetHeight() == H);
  EXPECT(seq.Flat() == f);
  double ux = 0, uy = 0;
  seq.GetDisplacement(2, 6, 4, &ux, &uy);  // [k][0][y][x], [k][1][y][x]
  EXPECT(ux == f[(2 * 2 + 0) * W * H + 4 * W + 6] && uy == f[(2 * 2 + 1) * W * H + 4 * W + 6]);
  seq.GetDisplacement(0, 0, 0, &ux, &uy);
  EXPECT(ux == f[0] && uy == f[W * H]);
  // the same bytes read at the transposed geometry are another (valid) sequence: the size is all a raw file can show
  FlowMotionSequence swapped;
  swapped.LoadSequenceFromFile(dir + "/flow3.bin", H, W);
  EXPECT(swapped.GetNumMotions() == K && swapped.GetWidth() == H);
  // one frame of a 21 x 5 image has the size of three frames of 7 x 5
  FlowMotionSequence one;
  one.LoadSequenceFromFile(dir + "/flow3.bin", 3 * W, H);
  EXPECT(one.GetNumMotions() == 1);
  // save / load round trip, and loading again replaces the sequence
  EXPECT(seq.SaveToFile(dir + "/flow3_copy.bin"));
  FlowMotionSequence copy(Field(1, 2, 2), 2, 2);
  EXPECT(copy.GetNumMotions() == 1);
  copy.LoadSequenceFromFile(dir + "/flow3_copy.bin", W, H);
  EXPECT(copy.GetNumMotions() == K && copy.Flat() == f);
}

static void TestCanonicalCarriesTheField() {
  const int K = 3, W = 6, H = 4;
  ImageModelParameters params;
  params.scale = 2;
  params.blur_radius = 5;
  params.blur_sigma = 1.5;
  params.flow_motion_sequence.SetFlow(Field(K, W, H), W, H);
  const ImageModel model = ImageModel::CreateImageModel(params);
  srmap_host::ChainParams chain;
  EXPECT(model.Canonical(&chain));
  EXPECT(chain.scale == 2 && chain.blur_ksize == 5 && chain.blur_sigma == 1.5);
  EXPECT(chain.shifts_xy.empty() && chain.affine_2x3.empty());
  EXPECT(chain.flow == Field(K, W, H) && chain.flow_width == W && chain.flow_height == H);
  EXPECT(chain.HasMotion() && chain.NumMotions() == K);
  chain.TrimMotions(2);
  EXPECT(chain.NumMotions() == 2 && chain.flow.size() == static_cast<size_t>(2 * 2 * W * H));
  EXPECT(chain.flow[2 * 2 * W * H - 1] == Field(K, W, H)[2 * 2 * W * H - 1]);
  // the other two models are untouched
  ImageModelParameters shifts;
  shifts.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1.5, -2)});
  srmap_host::ChainParams c2;
  EXPECT(ImageModel::CreateImageModel(shifts).Canonical(&c2));
  EXPECT(c2.flow.empty() && c2.affine_2x3.empty() && c2.shifts_xy.size() == 4 && c2.NumMotions() == 2);
  ImageModelParameters affine;
  affine.affine_motion_sequence.SetMotionSequence({AffineMotion(1, 0, 0.5, 0, 1, -0.5)});
  srmap_host::ChainParams c3;
  EXPECT(ImageModel::CreateImageModel(affine).Canonical(&c3));
  EXPECT(c3.flow.empty() && c3.affine_2x3.size() == 6 && c3.NumMotions() == 1);
  // a MotionModule says which sequence it is over
  const MotionModule flow_module(FlowMotionSequence(Field(1, W, H), W, H));
  EXPECT(flow_module.IsFlow() && !flow_module.IsAffine());
  EXPECT(!MotionModule(AffineMotionSequence({AffineMotion(1, 0, 0, 0, 1, 0)})).IsFlow());
  EXPECT(!MotionModule(MotionShiftSequence({MotionShift(0, 0)})).IsFlow());
}

// smooth fields: per frame a translation plus a slow sinusoid of amplitude 1.2 px (neighbour differences below 0.1 px)
static std::vector<double> SmoothField(const int K, const int W, const int H) {
  std::vector<double> f(static_cast<size_t>(K) * 2 * W * H);
  for (int k = 0; k < K; ++k)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t at = static_cast<size_t>(y) * W + x, plane = static_cast<size_t>(W) * H;
        f[(2 * static_cast<size_t>(k)) * plane + at] = -0.5 * k + (k ? 1.2 * std::sin(0.07 * y + k) : 0.0);
        f[(2 * static_cast<size_t>(k) + 1) * plane + at] = 0.25 * k + (k ? 1.2 * std::sin(0.06 * x + 2 * k) : 0.0);
      }
  return f;
}

static int TestOnTheGpu() {
  const int W = 64, H = 48, K = 4, scale = 2;
  std::vector<double> px(static_cast<size_t>(W) * H);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) px[static_cast<size_t>(r) * W + c] = 0.5 + 0.3 * std::sin(0.21 * c) * std::cos(0.17 * r) + 0.1 * std::sin(0.05 * c * r);
  const ImageData original(px.data(), cv::Size(W, H));
  const std::vector<double> field = SmoothField(K, W, H);
  const FlowMotionSequence sequence(field, W, H);
  // the C calls, directly
  srmap_problem_desc d;
  d.hr_width = W; d.hr_height = H; d.channels = 1; d.frames = K; d.scale = scale; d.shifts_xy = nullptr;
  d.blur_ksize = 3; d.blur_sigma = 1.0; d.dtype = SRMAP_F64;
  srmap_problem* raw = nullptr;
  EXPECT(srmap_problem_create(srmap_host::Context(), &d, &raw) == SRMAP_OK);
  srmap_host::ProblemPtr direct(raw);
  EXPECT(srmap_problem_set_flow(direct.get(), field.data()) == SRMAP_OK);
  ImageModelParameters params;
  params.scale = scale;
  params.blur_radius = 3;
  params.blur_sigma = 1.0;
  params.flow_motion_sequence = sequence;
  const ImageModel model = ImageModel::CreateImageModel(params);
  const int w = W / scale, h = H / scale;
  std::vector<ImageData> frames;
  std::vector<double> stack;
  for (int k = 0; k < K; ++k) {
    std::vector<double> lr(static_cast<size_t>(w) * h);
    EXPECT(srmap_apply(direct.get(), k, px.data(), lr.data()) == SRMAP_OK);
    frames.push_back(model.ApplyToImage(original, k));
    EXPECT(frames.back().GetImageSize() == cv::Size(w, h) && frames.back().ToPlanar() == lr);  // the same bits
    stack.insert(stack.end(), lr.begin(), lr.end());
    // the transpose, and the MotionModule alone
    std::vector<double> back(px.size());
    EXPECT(srmap_apply_transpose(direct.get(), k, lr.data(), back.data()) == SRMAP_OK);
    ImageData up = frames.back();
    model.ApplyTransposeToImage(&up, k);
    EXPECT(up.ToPlanar() == back);
  }
  {
    srmap_problem_desc dm = d;
    dm.scale = 1; dm.blur_ksize = 0; dm.blur_sigma = 0.0;
    srmap_problem* rm = nullptr;
    EXPECT(srmap_problem_create(srmap_host::Context(), &dm, &rm) == SRMAP_OK);
    srmap_host::ProblemPtr motion_only(rm);
    EXPECT(srmap_problem_set_flow(motion_only.get(), field.data()) == SRMAP_OK);
    std::vector<double> warped(px.size());
    EXPECT(srmap_apply(motion_only.get(), 2, px.data(), warped.data()) == SRMAP_OK);
    ImageData moved = original;
    MotionModule(sequence).ApplyToImage(&moved, 2);
    EXPECT(moved.ToPlanar() == warped);
  }
  // the solver over the flow model evaluates and solves what the C calls do
  EXPECT(srmap_set_observations(direct.get(), stack.data()) == SRMAP_OK);
  EXPECT(srmap_add_regularizer(direct.get(), SRMAP_REG_TV, 0.01, 0, 0.0, nullptr) == SRMAP_OK);
  IRLSMapSolverOptions options;
  options.max_num_irls_iterations = 3;
  IRLSMapSolver solver(options, model, frames, false);
  solver.AddRegularizer(std::make_shared<TotalVariationRegularizer>(cv::Size(W, H)), 0.01);
  ImageData start = frames[0];
  start.ResizeImage(scale, INTERPOLATE_LINEAR);
  const std::vector<double> x0 = start.ToPlanar();
  std::vector<double> g_direct(x0.size()), g_solver(x0.size());
  double f_direct = 0.0;
  EXPECT(srmap_eval(direct.get(), SRMAP_TERM_ALL, x0.data(), &f_direct, g_direct.data()) == SRMAP_OK);
  EXPECT(solver.ComputeAllTerms(x0.data(), g_solver.data()) == f_direct && g_solver == g_direct);
  int is_set = 0;
  EXPECT(srmap_problem_get_flow(solver.problem(), nullptr, &is_set) == SRMAP_OK && is_set == 1);
  srmap_irls_options o;
  srmap_irls_options_default(&o);
  o.max_num_irls_iterations = 3;
  std::vector<double> x_direct(x0.size());
  srmap_solve_report report;
  EXPECT(srmap_solve(direct.get(), &o, x0.data(), x_direct.data(), &report) == SRMAP_OK);
  const ImageData result = solver.Solve(start);
  EXPECT(result.ToPlanar() == x_direct && solver.GetReport().cg_iterations == report.cg_iterations);
  double err0 = 0.0, err1 = 0.0;
  for (size_t i = 0; i < px.size(); ++i) { err0 += (x0[i] - px[i]) * (x0[i] - px[i]); err1 += (x_direct[i] - px[i]) * (x_direct[i] - px[i]); }
  std::printf("squared error against the scene: %.4e at the start, %.4e after the solve (%d iterations)\n", err0, err1, report.cg_iterations);
  // the restatement's solve of this input (tests/flow_restatement.py, the same scene, field, TV 0.01 and 3 IRLS rounds) goes
  // 18.612181 -> 8.858077 in 127 iterations: the scene's chirp lies above the LR Nyquist rate and sets that floor.  Held to
  // 0.01 dB = 0.23 %, the bar of the table's solves
  EXPECT(std::fabs(err0 - 18.612181) <= 1e-5 && std::fabs(err1 - 8.858077) <= 0.0023 * 8.858077 && report.cg_iterations == 127);
  std::printf(g_fail ? "FLOW MOTION FACADE TESTS FAILED (%d)\n" : "FLOW MOTION FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: flow_motion_test <scratch dir> [gpu|index|pixel|both|wrong_size|empty_file|missing_file|wrong_geometry]\n");
    return 2;
  }
  const std::string dir = argv[1];
  if (argc > 2) {  // each of these must abort inside the call; reaching the end is the failure
    const std::string which = argv[2];
    if (which == "gpu") return TestOnTheGpu();
    const int W = 6, H = 4;
    const std::vector<double> f = Field(2, W, H);
    if (which == "index") {
      FlowMotionSequence seq(f, W, H);
      double ux, uy;
      seq.GetDisplacement(2, 0, 0, &ux, &uy);
    } else if (which == "pixel") {
      FlowMotionSequence seq(f, W, H);
      double ux, uy;
      seq.GetDisplacement(1, W, 0, &ux, &uy);
    } else if (which == "both") {
      ImageModelParameters params;
      params.flow_motion_sequence.SetFlow(f, W, H);
      params.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1, 1)});
      ImageModel::CreateImageModel(params);
    } else if (which == "wrong_size") {  // one double short of two frames
      FlowMotionSequence seq;
      seq.LoadSequenceFromFile(WriteRaw(dir, "flow_short.bin", f.data(), (f.size() - 1) * sizeof(double)), W, H);
    } else if (which == "empty_file") {
      FlowMotionSequence seq;
      seq.LoadSequenceFromFile(WriteRaw(dir, "flow_empty.bin", nullptr, 0), W, H);
    } else if (which == "missing_file") {
      FlowMotionSequence seq;
      seq.LoadSequenceFromFile(dir + "/no_such_flow_file.bin", W, H);
    } else if (which == "wrong_geometry") {  // a field for 6 x 4 in a chain applied at 8 x 4: refused before any device call
      srmap_host::ChainParams chain;
      MotionModule(FlowMotionSequence(f, W, H)).Describe(&chain);
      srmap_host::MakeProblem(chain, W + 2, H, 1);
    }
    std::printf("case '%s' did not abort\n", which.c_str());
    return 0;
  }
  TestFile(dir);
  TestCanonicalCarriesTheField();
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("FLOW MOTION HOST TESTS PASSED\n");
  return 0;
}
