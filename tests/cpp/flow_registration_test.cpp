// flow_registration_test.cpp -- host side of the dense flow registration (registration::FlowRegistration of
// super-resolution_amd/host/motion/registration.h, IRLSMapSolver::MultiplyDataWeights): what needs no GPU -- the empty list,
// the file --save_flow_path writes and --flow_motion_path reads, and the calls that must abort before any device call.
// argv[1] = scratch directory; argv[2] (optional) names ONE case that must abort the process with a "Check failed" message:
// scale | sizes | no_channel | few_initial -- or `gpu`: FlowRegistration against the C entry point and the masks as data
// weights of a solver (tests/test_gpu_flow_registration.py).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "image_model/image_model.h"
#include "motion/flow_motion.h"
#include "motion/registration.h"
#include "optimization/irls_map_solver.h"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

// frame k of a smooth scene moved by (0.4 k, -0.3 k) px plus a slow sinusoid
static std::vector<double> Frame(const int k, const int W, const int H) {
  std::vector<double> px(static_cast<size_t>(W) * H);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double x = c + 0.4 * k + (k ? 0.3 * std::sin(0.11 * r + k) : 0.0), y = r - 0.3 * k + (k ? 0.3 * std::sin(0.09 * c - k) : 0.0);
      px[static_cast<size_t>(r) * W + c] = 0.5 + 0.2 * std::sin(0.31 * x) * std::cos(0.23 * y) + 0.15 * std::sin(0.13 * (x + y)) + 0.1 * std::cos(0.47 * x - 0.29 * y);
    }
  return px;
}

static void TestWithoutAGpu(const std::string& dir) {
  // an empty list: an empty sequence, empty outputs, no device call
  std::vector<double> valid(3, 1.0), quality(3, 1.0);
  const FlowMotionSequence none = registration::FlowRegistration(std::vector<ImageData>(), 2, &valid, &quality);
  EXPECT(none.Empty() && none.GetNumMotions() == 0 && valid.empty() && quality.empty());
  // the defaults are the C ABI's
  srmap_flow_registration_options o;
  srmap_flow_registration_options_default(&o);
  const registration::FlowRegistrationOptions d;
  EXPECT(o.struct_size == static_cast<int>(sizeof(o)) && o.hr_scale == 1 && o.initial_affine_2x3 == nullptr);
  EXPECT(d.warps == o.warps && d.window_radius == o.window_radius && d.damping == o.damping && d.smooth_radius == o.smooth_radius &&
         d.valid_margin == o.valid_margin && d.max_levels == o.max_levels && d.initial_motion.GetNumMotions() == 0);
  // what --save_flow_path writes is what --flow_motion_path reads: raw float64 [K][2][H][W] at the HR size, no header
  const int K = 3, W = 8, H = 6;
  std::vector<double> f(static_cast<size_t>(K) * 2 * W * H);
  for (size_t i = 0; i < f.size(); ++i) f[i] = 0.01 * static_cast<double>(i) - 1.0 / 3.0;
  const FlowMotionSequence seq(f, W, H);
  const std::string path = dir + "/saved_flow.bin";
  EXPECT(seq.SaveToFile(path));
  std::FILE* fp = std::fopen(path.c_str(), "rb");
  EXPECT(fp != nullptr);
  if (fp) {
    std::fseek(fp, 0, SEEK_END);
    EXPECT(static_cast<size_t>(std::ftell(fp)) == f.size() * sizeof(double));
    std::fclose(fp);
  }
  FlowMotionSequence back;
  back.LoadSequenceFromFile(path, W, H);
  EXPECT(back.GetNumMotions() == K && back.Flat() == f);
  EXPECT(!seq.SaveToFile(dir + "/no_such_directory/flow.bin"));
}

static int TestOnTheGpu() {
  const int w = 40, h = 28, K = 3, scale = 2;
  std::vector<ImageData> frames;
  std::vector<double> stack;
  for (int k = 0; k < K; ++k) {
    const std::vector<double> px = Frame(k, w, h);
    ImageData im(px.data(), cv::Size(w, h));
    std::vector<double> second(px);
    for (double& v : second) v = 1.0 - v;  // a second channel: the registration reads channel 0 only
    im.AddChannel(second.data(), cv::Size(w, h));
    frames.push_back(im);
    stack.insert(stack.end(), px.begin(), px.end());
  }
  const size_t n = static_cast<size_t>(w) * h, N = n * scale * scale;
  // the C call, directly
  srmap_flow_registration_options o;
  srmap_flow_registration_options_default(&o);
  o.hr_scale = scale;
  std::vector<double> flow(K * 2 * N), valid(K * n), quality(3 * K);
  EXPECT(srmap_register_flow(srmap_host::Context(), K, w, h, stack.data(), &o, flow.data(), valid.data(), quality.data()) == SRMAP_OK);
  std::vector<double> v2, q2;
  const FlowMotionSequence sequence = registration::FlowRegistration(frames, scale, &v2, &q2);
  EXPECT(sequence.GetNumMotions() == K && sequence.GetWidth() == w * scale && sequence.GetHeight() == h * scale);
  EXPECT(sequence.Flat() == flow && v2 == valid && q2 == quality);  // the same bits
  EXPECT(registration::FlowRegistration(frames, scale).Flat() == flow);
  double moved = 0.0, kept = 0.0;
  for (size_t i = 2 * N; i < flow.size(); ++i) moved = std::fmax(moved, std::fabs(flow[i]));
  for (const double v : valid) kept += v;
  std::printf("largest displacement %.3f HR px, %.1f %% valid, residuals %.2e %.2e\n", moved, 100.0 * kept / valid.size(), quality[3], quality[6]);
  EXPECT(moved > 0.5 && moved < 4.0 && kept < valid.size() && kept > 0.5 * valid.size());
  // options reach the C call
  registration::FlowRegistrationOptions ro;
  ro.warps = 3;
  ro.window_radius = 2;
  ro.valid_margin = 0;
  ro.initial_motion = AffineMotionSequence({AffineMotion(1, 0, 0, 0, 1, 0), AffineMotion(1, 0, 0.4, 0, 1, -0.3), AffineMotion(1, 0, 0.8, 0, 1, -0.6)});
  o.warps = 3;
  o.window_radius = 2;
  o.valid_margin = 0;
  const double init[18] = {1, 0, 0, 0, 1, 0, 1, 0, 0.4, 0, 1, -0.3, 1, 0, 0.8, 0, 1, -0.6};
  o.initial_affine_2x3 = init;
  std::vector<double> flow3(flow.size()), valid3(valid.size());
  EXPECT(srmap_register_flow(srmap_host::Context(), K, w, h, stack.data(), &o, flow3.data(), valid3.data(), nullptr) == SRMAP_OK);
  std::vector<double> v3;
  EXPECT(registration::FlowRegistration(frames, scale, &v3, nullptr, ro).Flat() == flow3 && v3 == valid3 && flow3 != flow);

  // the sequence and the masks in a solver: the weights are the masks over both channels, times what was there
  ImageModelParameters params;
  params.scale = scale;
  params.blur_radius = 3;
  params.blur_sigma = 1.0;
  params.flow_motion_sequence = sequence;
  const ImageModel model = ImageModel::CreateImageModel(params);
  IRLSMapSolverOptions options;
  options.max_num_irls_iterations = 2;
  IRLSMapSolver solver(options, model, frames, false);
  solver.MultiplyDataWeights(valid);
  std::vector<double> wts = solver.GetDataWeights();
  EXPECT(wts.size() == 2 * valid.size());
  bool same = true;
  for (int k = 0; k < K; ++k)
    for (int c = 0; c < 2; ++c)
      for (size_t i = 0; i < n; ++i) same = same && wts[(static_cast<size_t>(k) * 2 + c) * n + i] == valid[k * n + i];
  EXPECT(same);
  std::vector<double> half(valid.size(), 0.5);
  solver.MultiplyDataWeights(half);
  wts = solver.GetDataWeights();
  same = true;
  for (int k = 0; k < K; ++k)
    for (size_t i = 0; i < n; ++i) same = same && wts[(static_cast<size_t>(k) * 2 + 1) * n + i] == 0.5 * valid[k * n + i];
  EXPECT(same);
  ImageData start = frames[0];
  start.ResizeImage(scale, INTERPOLATE_LINEAR);
  const ImageData result = solver.Solve(start);
  EXPECT(result.GetImageSize() == cv::Size(w * scale, h * scale) && solver.GetReport().cg_iterations > 0);
  EXPECT(solver.GetDataWeights() == wts);  // a least-squares solve leaves them
  std::printf(g_fail ? "FLOW REGISTRATION FACADE TESTS FAILED (%d)\n" : "FLOW REGISTRATION FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: flow_registration_test <scratch dir> [gpu|scale|sizes|no_channel|few_initial]\n");
    return 2;
  }
  const std::string dir = argv[1];
  if (argc > 2) {  // each of these must abort inside the call, before any device call; reaching the end is the failure
    const std::string which = argv[2];
    if (which == "gpu") return TestOnTheGpu();
    const int w = 20, h = 16;
    const std::vector<double> a = Frame(0, w, h), b = Frame(1, w + 1, h);
    if (which == "scale") {
      registration::FlowRegistration({ImageData(a.data(), cv::Size(w, h)), ImageData(a.data(), cv::Size(w, h))}, 0);
    } else if (which == "sizes") {
      registration::FlowRegistration({ImageData(a.data(), cv::Size(w, h)), ImageData(b.data(), cv::Size(w + 1, h))}, 2);
    } else if (which == "no_channel") {
      registration::FlowRegistration({ImageData(a.data(), cv::Size(w, h)), ImageData()}, 2);
    } else if (which == "few_initial") {
      registration::FlowRegistrationOptions ro;
      ro.initial_motion = AffineMotionSequence({AffineMotion(1, 0, 0, 0, 1, 0)});
      registration::FlowRegistration({ImageData(a.data(), cv::Size(w, h)), ImageData(a.data(), cv::Size(w, h))}, 2, nullptr, nullptr, ro);
    }
    std::printf("case '%s' did not abort\n", which.c_str());
    return 0;
  }
  TestWithoutAGpu(dir);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("FLOW REGISTRATION HOST TESTS PASSED\n");
  return 0;
}
