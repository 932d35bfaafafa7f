// blur_kernel_test.cpp -- host side of the free-form blur kernel (super-resolution_amd/host/image_model/blur_kernel.h, the
// BlurModule constructor over it, ImageModelParameters::blur_kernel_path, IRLSMapSolver::FitBlur).
//   blur_kernel_test <scratch dir>            file format, round trip, ImageModel::Canonical() carrying the taps to the C
//                                             ABI's chain.  No GPU needed: nothing here applies an operator.
//   blur_kernel_test <scratch dir> <case>     ONE case that must abort the process with a "Check failed" message:
//                                             even_size | short_file | long_file | missing_file | empty_module | index
//   blur_kernel_test <scratch dir> gpu        (needs the GPU; run by tests/test_gpu_blur_kernel.py) BlurModule over a kernel
//                                             applies what srmap_apply applies; FitBlur returns what srmap_fit_blur returns,
//                                             bit for bit, recovers the kernel that made the frames, and installs it.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "image_model/blur_kernel.h"
#include "image_model/image_model.h"
#include "optimization/irls_map_solver.h"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static std::string WriteFile(const std::string& dir, const std::string& name, const std::string& text) {
  const std::string path = dir + "/" + name;
  std::ofstream out(path);
  out << text;
  return path;
}

static const char* kStreak3 = "3\n0 0 0\n0\t0.5 0.3125\r\n-0.0625 0 2.5e-1\n";

static void TestFileFormat(const std::string& dir) {
  BlurKernel k;
  EXPECT(k.Empty() && k.GetSize() == 0);
  k.LoadFromFile(WriteFile(dir, "streak3.txt", kStreak3));
  EXPECT(!k.Empty() && k.GetSize() == 3 && k.GetTaps().size() == 9);
  EXPECT(k(0, 0) == 0.0 && k(1, 1) == 0.5 && k(1, 2) == 0.3125 && k(2, 0) == -0.0625 && k(2, 2) == 0.25);
  // the size and the taps may share lines: any white space separates
  BlurKernel one;
  one.LoadFromFile(WriteFile(dir, "one.txt", "1 0.75"));
  EXPECT(one.GetSize() == 1 && one(0, 0) == 0.75);
  // a saved kernel loads again bit for bit
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  std::vector<double> taps(49);
  for (auto& v : taps) v = uni(rng) / 3.0;
  const BlurKernel seven(7, taps);
  EXPECT(seven.SaveToFile(dir + "/seven.txt"));
  BlurKernel back;
  back.LoadFromFile(dir + "/seven.txt");
  EXPECT(back.GetSize() == 7 && back.GetTaps() == taps);
  EXPECT(!seven.SaveToFile(dir + "/no_such_dir/seven.txt"));
}

static void TestCanonicalCarriesTheTaps(const std::string& dir) {
  ImageModelParameters params;
  params.scale = 3;
  params.blur_radius = 5;  // replaced by the kernel
  params.blur_sigma = 1.5;
  params.blur_kernel_path = WriteFile(dir, "streak3b.txt", kStreak3);
  params.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1.5, -2)});
  srmap_host::ChainParams chain;
  EXPECT(ImageModel::CreateImageModel(params).Canonical(&chain));
  EXPECT(chain.scale == 3 && chain.blur_ksize == 0 && chain.blur_sigma == 0.0);
  EXPECT(chain.blur_taps_ksize == 3 && chain.blur_taps.size() == 9 && chain.blur_taps[4] == 0.5 && chain.blur_taps[6] == -0.0625);
  EXPECT(chain.shifts_xy.size() == 4);
  // a kernel given directly needs no file
  ImageModelParameters direct;
  direct.blur_kernel = BlurKernel(1, {2.0});
  srmap_host::ChainParams c2;
  EXPECT(ImageModel::CreateImageModel(direct).Canonical(&c2));
  EXPECT(c2.blur_taps_ksize == 1 && c2.blur_taps.size() == 1 && c2.blur_taps[0] == 2.0);
  // the Gaussian model is untouched: (radius, sigma), no taps
  ImageModelParameters gauss;
  gauss.blur_radius = 5;
  gauss.blur_sigma = 1.5;
  srmap_host::ChainParams c3;
  EXPECT(ImageModel::CreateImageModel(gauss).Canonical(&c3));
  EXPECT(c3.blur_ksize == 5 && c3.blur_sigma == 1.5 && c3.blur_taps.empty() && c3.blur_taps_ksize == 0);
  EXPECT(BlurModule(BlurKernel(1, {1.0})).IsFreeForm() && !BlurModule(3, 1.0).IsFreeForm());
}

// ---- GPU part ----
static std::vector<double> Scene(const int W, const int H) {
  std::vector<double> px(static_cast<size_t>(W) * H);
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<double> coarse(34 * 26);
  for (auto& v : coarse) v = uni(rng);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double u = c / 4.0, v = r / 4.0;  // bilinear blow-up of a random grid + two sinusoids
      const int u0 = (int)u, v0 = (int)v;
      const double a = u - u0, b = v - v0;
      const double g = (1 - b) * ((1 - a) * coarse[v0 * 34 + u0] + a * coarse[v0 * 34 + u0 + 1]) +
                       b * ((1 - a) * coarse[(v0 + 1) * 34 + u0] + a * coarse[(v0 + 1) * 34 + u0 + 1]);
      px[static_cast<size_t>(r) * W + c] = 0.6 * g + 0.2 + 0.1 * std::sin(0.21 * c) * std::cos(0.17 * r);
    }
  return px;
}

static int TestOnTheGpu() {
  const int W = 128, H = 96, K = 4, scale = 2;
  const std::vector<double> px = Scene(W, H);
  const ImageData original(px.data(), cv::Size(W, H));
  // an asymmetric 5 x 5 kernel: a diagonal streak over a small pedestal, sum 1
  std::vector<double> taps(25, 0.01);
  taps[2 * 5 + 2] = 0.36; taps[1 * 5 + 3] = 0.24; taps[0 * 5 + 4] = 0.16;
  double sum = 0.0;
  for (const double v : taps) sum += v;
  for (double& v : taps) v /= sum;
  const BlurKernel truth(5, taps);
  ImageModelParameters generating;
  generating.scale = scale;
  generating.blur_kernel = truth;
  generating.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1.25, 0.75), MotionShift(0.5, 1), MotionShift(1, 0.25)});
  const ImageModel generator = ImageModel::CreateImageModel(generating);
  std::vector<ImageData> frames;
  for (int i = 0; i < K; ++i) frames.push_back(generator.ApplyToImage(original, i));
  {  // the module alone applies the C ABI's operator
    srmap_host::ChainParams chain;
    chain.blur_taps = taps;
    chain.blur_taps_ksize = 5;
    srmap_host::ProblemPtr p = srmap_host::MakeProblem(chain, W, H, 1);
    std::vector<double> direct(px.size());
    EXPECT(srmap_apply(p.get(), 0, px.data(), direct.data()) == SRMAP_OK);
    ImageData blurred = original;
    BlurModule(truth).ApplyToImage(&blurred, 0);
    EXPECT(blurred.ToPlanar() == direct);
    double moved = 0.0;
    for (size_t i = 0; i < px.size(); ++i) moved = std::max(moved, std::fabs(direct[i] - px[i]));
    EXPECT(moved > 1e-3);
  }
  // the solver starts from a guessed Gaussian; FitBlur at the image that made the frames recovers the kernel
  ImageModelParameters solving = generating;
  solving.blur_kernel = BlurKernel();
  solving.blur_radius = 3;
  solving.blur_sigma = 1.0;
  const ImageModel solver_model = ImageModel::CreateImageModel(solving);
  IRLSMapSolverOptions options;
  IRLSMapSolver solver(options, solver_model, frames, false);
  srmap_blur_fit_options o;
  srmap_blur_fit_options_default(&o);
  o.ksize = 5;
  o.apply = 0;
  std::vector<double> direct(25), direct_quality(5);
  const std::vector<double> x = original.ToPlanar();
  EXPECT(srmap_fit_blur(solver.problem(), x.data(), &o, direct.data(), direct_quality.data(), nullptr) == SRMAP_OK);
  const double before = solver.ComputeAllTerms(x.data());
  BlurFitOptions fit;
  fit.ksize = 5;
  std::vector<double> quality;
  const BlurKernel got = solver.FitBlur(original, fit, &quality);
  EXPECT(got.GetSize() == 5 && got.GetTaps() == direct && quality == direct_quality);  // the same numbers, bit for bit
  double err = 0.0;
  for (int i = 0; i < 25; ++i) err = std::max(err, std::fabs(got.GetTaps()[i] - taps[i]));
  const double after = solver.ComputeAllTerms(x.data());
  std::printf("largest tap error %.2e; data cost at the generating image %.6e with the guessed Gaussian, %.6e with the fit\n", err, before, after);
  EXPECT(quality[4] == 0.0 && err <= 1e-9);
  EXPECT(after < 1e-12 * before);  // installed: the frames are noise-free, the fitted kernel explains them
  int ksize = 0;
  std::vector<double> in_force(25);
  EXPECT(srmap_problem_get_blur_kernel(solver.problem(), &ksize, in_force.data()) == SRMAP_OK && ksize == 5 && in_force == direct);
  // ksize 0: the size of the kernel in force, now 5
  const BlurKernel again = solver.FitBlur(original);
  EXPECT(again.GetSize() == 5);
  std::printf(g_fail ? "BLUR KERNEL FACADE TESTS FAILED (%d)\n" : "BLUR KERNEL FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: blur_kernel_test <scratch dir> [gpu|even_size|short_file|long_file|missing_file|empty_module|index]\n");
    return 2;
  }
  const std::string dir = argv[1];
  if (argc > 2) {
    const std::string which = argv[2];
    if (which == "gpu") return TestOnTheGpu();
    // each of these must abort inside the call; reaching the end is the failure
    BlurKernel k;
    if (which == "even_size") k.LoadFromFile(WriteFile(dir, "even.txt", "2\n1 0\n0 1\n"));
    else if (which == "short_file") k.LoadFromFile(WriteFile(dir, "short.txt", "3\n1 2 3\n4 5 6\n7 8\n"));
    else if (which == "long_file") k.LoadFromFile(WriteFile(dir, "long.txt", "1\n1 2\n"));
    else if (which == "missing_file") k.LoadFromFile(dir + "/no_such_kernel_file.txt");
    else if (which == "empty_module") BlurModule module(k);
    else if (which == "index") BlurKernel(1, {1.0})(0, 1);
    std::printf("case '%s' did not abort\n", which.c_str());
    return 0;
  }
  TestFileFormat(dir);
  TestCanonicalCarriesTheTaps(dir);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("BLUR KERNEL HOST TESTS PASSED\n");
  return 0;
}
