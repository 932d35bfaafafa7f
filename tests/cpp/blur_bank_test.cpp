// blur_bank_test.cpp -- host side of the blur-kernel bank (super-resolution_amd/host/image_model/blur_kernel.h:
// BlurKernelBank, the BlurModule constructor over it, ImageModelParameters::blur_bank(_path), IRLSMapSolver::SetBlurBank /
// FitBlurBank).
//   blur_bank_test <scratch dir>            file format, round trip, padding, ImageModel::Canonical() carrying the bank to the
//                                           C ABI's chain.  No GPU needed: nothing here applies an operator.
//   blur_bank_test <scratch dir> <case>     ONE case that must abort the process with a "Check failed" message:
//                                           bad_mode | even_size | no_entries | short_file | long_file | missing_file |
//                                           empty_module | entry | both_blurs
//   blur_bank_test <scratch dir> gpu        (needs the GPU; run by tests/test_gpu_blur_bank_host.py) the model over a bank
//                                           applies what srmap_apply applies under srmap_problem_set_blur_bank; SetBlurBank
//                                           and FitBlurBank do what the C calls do, bit for bit.
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

// two frames, 3 x 3: a one-sided streak and a kernel with a negative tap
static const char* kTwoFrames = "1 3 2\n0 0 0\n0\t0.5 0.3125\r\n-0.0625 0 2.5e-1\n\n0 1 0\n0 0 0\n0 0 -0.5\n";

static void TestFileFormat(const std::string& dir) {
  BlurKernelBank b;
  EXPECT(b.Empty() && b.GetSize() == 0 && b.GetMode() == 0 && b.GetNumEntries() == 0);
  b.LoadFromFile(WriteFile(dir, "two.txt", kTwoFrames));
  EXPECT(!b.Empty() && b.GetMode() == 1 && b.GetSize() == 3 && b.GetNumEntries() == 2 && b.GetTaps().size() == 18);
  EXPECT(b.Entry(0)(1, 2) == 0.3125 && b.Entry(0)(2, 0) == -0.0625 && b.Entry(1)(0, 1) == 1.0 && b.Entry(1)(2, 2) == -0.5);
  // header and taps may share a line: any white space separates
  BlurKernelBank one;
  one.LoadFromFile(WriteFile(dir, "one.txt", "2 1 3 0.75 0.5 0.25"));
  EXPECT(one.GetMode() == 2 && one.GetSize() == 1 && one.GetNumEntries() == 3 && one.Entry(2)(0, 0) == 0.25);
  // a saved bank loads again bit for bit
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  std::vector<double> taps(6 * 49);
  for (auto& v : taps) v = uni(rng) / 3.0;
  const BlurKernelBank six(3, 7, 6, taps);
  EXPECT(six.SaveToFile(dir + "/six.txt"));
  BlurKernelBank back;
  back.LoadFromFile(dir + "/six.txt");
  EXPECT(back.GetMode() == 3 && back.GetSize() == 7 && back.GetNumEntries() == 6 && back.GetTaps() == taps);
  EXPECT(!six.SaveToFile(dir + "/no_such_dir/six.txt"));
  // kernels of different sizes go in zero-padded to the largest, centred
  const BlurKernelBank padded = BlurKernelBank::Padded(1, {BlurKernel(1, {2.0}), BlurKernel(3, {1, 2, 3, 4, 5, 6, 7, 8, 9})});
  EXPECT(padded.GetSize() == 3 && padded.GetNumEntries() == 2);
  EXPECT(padded.Entry(0)(1, 1) == 2.0 && padded.Entry(0)(0, 0) == 0.0 && padded.Entry(0)(2, 1) == 0.0 && padded.Entry(1)(2, 0) == 7.0);
}

static void TestCanonicalCarriesTheBank(const std::string& dir) {
  ImageModelParameters params;
  params.scale = 3;
  params.blur_radius = 5;  // replaced by the bank
  params.blur_sigma = 1.5;
  params.blur_bank_path = WriteFile(dir, "two_b.txt", kTwoFrames);
  params.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1.5, -2)});
  srmap_host::ChainParams chain;
  EXPECT(ImageModel::CreateImageModel(params).Canonical(&chain));
  EXPECT(chain.scale == 3 && chain.blur_ksize == 0 && chain.blur_sigma == 0.0 && chain.blur_taps.empty());
  EXPECT(chain.blur_bank_mode == 1 && chain.blur_bank_ksize == 3 && chain.blur_bank.size() == 18 && chain.BankEntries() == 2);
  EXPECT(chain.blur_bank[4] == 0.5 && chain.blur_bank[17] == -0.5 && chain.BankPerFrame() && chain.shifts_xy.size() == 4);
  // fewer observations than entries of a per-frame bank: the first n, as for the motions
  chain.TrimMotions(1);
  EXPECT(chain.BankEntries() == 1 && chain.shifts_xy.size() == 2);
  // a bank given directly needs no file; a per-channel bank is not per frame
  ImageModelParameters direct;
  direct.blur_bank = BlurKernelBank(2, 1, 3, {1.0, 2.0, 3.0});
  srmap_host::ChainParams c2;
  EXPECT(ImageModel::CreateImageModel(direct).Canonical(&c2));
  EXPECT(c2.blur_bank_mode == 2 && c2.blur_bank_ksize == 1 && c2.BankEntries() == 3 && !c2.BankPerFrame());
  // the single kernel and the Gaussian carry no bank
  ImageModelParameters gauss;
  gauss.blur_radius = 5;
  gauss.blur_sigma = 1.5;
  srmap_host::ChainParams c3;
  EXPECT(ImageModel::CreateImageModel(gauss).Canonical(&c3));
  EXPECT(c3.blur_ksize == 5 && c3.blur_bank_mode == 0 && c3.blur_bank.empty() && c3.BankEntries() == 0);
  EXPECT(BlurModule(direct.blur_bank).IsBank() && BlurModule(direct.blur_bank).IsFreeForm() && !BlurModule(BlurKernel(1, {1.0})).IsBank());
}

// ---- GPU part ----
static std::vector<double> Scene(const int W, const int H, const int C) {
  std::vector<double> px(static_cast<size_t>(W) * H * C);
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  for (auto& v : px) v = uni(rng);
  return px;
}

static int TestOnTheGpu() {
  const int W = 64, H = 48, K = 4, scale = 2;
  const std::vector<double> px = Scene(W, H, 1);
  const ImageData original(px.data(), cv::Size(W, H));
  // four different asymmetric 5 x 5 kernels, each of sum 1
  std::vector<double> taps(K * 25, 0.01);
  for (int k = 0; k < K; ++k) {
    taps[k * 25 + 2 * 5 + 2] = 0.36; taps[k * 25 + 1 * 5 + (k % 5)] = 0.24; taps[k * 25 + (k + 1) * 5 + 4] = 0.16;
    double sum = 0.0;
    for (int i = 0; i < 25; ++i) sum += taps[k * 25 + i];
    for (int i = 0; i < 25; ++i) taps[k * 25 + i] /= sum;
  }
  const BlurKernelBank truth(SRMAP_BLUR_PER_FRAME, 5, K, taps);
  ImageModelParameters generating;
  generating.scale = scale;
  generating.blur_bank = truth;
  const std::vector<double> shifts = {0, 0, 1.25, 0.75, 0.5, 1, 1, 0.25};
  generating.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1.25, 0.75), MotionShift(0.5, 1), MotionShift(1, 0.25)});
  const ImageModel generator = ImageModel::CreateImageModel(generating);
  std::vector<ImageData> frames;
  for (int i = 0; i < K; ++i) frames.push_back(generator.ApplyToImage(original, i));
  {  // the model applies the C ABI's operator, frame by frame; the module alone (no motion) goes by the index too
    srmap_problem_desc d;
    d.hr_width = W; d.hr_height = H; d.channels = 1; d.frames = K; d.scale = scale; d.shifts_xy = shifts.data();
    d.blur_ksize = 0; d.blur_sigma = 0.0; d.dtype = SRMAP_F64;
    srmap_problem* raw = nullptr;
    EXPECT(srmap_problem_create(srmap_host::Context(), &d, &raw) == SRMAP_OK);
    srmap_host::ProblemPtr p(raw);
    EXPECT(srmap_problem_set_blur_bank(raw, SRMAP_BLUR_PER_FRAME, 5, taps.data()) == SRMAP_OK);
    std::vector<double> direct(static_cast<size_t>(W / scale) * (H / scale));
    for (int i = 0; i < K; ++i) {
      EXPECT(srmap_apply(raw, i, px.data(), direct.data()) == SRMAP_OK);
      EXPECT(frames[i].ToPlanar() == direct);
    }
    srmap_host::ChainParams chain;
    chain.blur_bank_mode = SRMAP_BLUR_PER_FRAME; chain.blur_bank_ksize = 5; chain.blur_bank = taps;
    srmap_host::ProblemPtr q = srmap_host::MakeProblem(chain, W, H, 1);
    std::vector<double> blurred_direct(px.size());
    EXPECT(srmap_apply(q.get(), 2, px.data(), blurred_direct.data()) == SRMAP_OK);
    ImageData blurred = original;
    BlurModule(truth).ApplyToImage(&blurred, 2);
    EXPECT(blurred.ToPlanar() == blurred_direct);
  }
  // the solver starts from a guessed Gaussian; FitBlurBank at the image that made the frames recovers every entry
  ImageModelParameters solving = generating;
  solving.blur_bank = BlurKernelBank();
  solving.blur_radius = 3;
  solving.blur_sigma = 1.0;
  const ImageModel solver_model = ImageModel::CreateImageModel(solving);
  IRLSMapSolverOptions options;
  IRLSMapSolver solver(options, solver_model, frames, false);
  srmap_blur_fit_options o;
  srmap_blur_fit_options_default(&o);
  o.ksize = 5;
  o.apply = 0;
  std::vector<double> direct(K * 25), direct_quality(K * 5);
  const std::vector<double> x = original.ToPlanar();
  EXPECT(srmap_fit_blur_bank(solver.problem(), x.data(), SRMAP_BLUR_PER_FRAME, &o, direct.data(), direct_quality.data(), nullptr) == SRMAP_OK);
  const double before = solver.ComputeAllTerms(x.data());
  BlurFitOptions fit;
  fit.ksize = 5;
  std::vector<double> quality;
  const BlurKernelBank got = solver.FitBlurBank(original, SRMAP_BLUR_PER_FRAME, fit, &quality);
  EXPECT(got.GetSize() == 5 && got.GetNumEntries() == K && got.GetTaps() == direct && quality == direct_quality);  // bit for bit
  double err = 0.0;
  for (int i = 0; i < K * 25; ++i) err = std::max(err, std::fabs(got.GetTaps()[i] - taps[i]));
  const double after = solver.ComputeAllTerms(x.data());
  std::printf("largest tap error %.2e; data cost at the generating image %.6e with the guessed Gaussian, %.6e with the fitted bank\n", err, before, after);
  for (int k = 0; k < K; ++k) EXPECT(quality[5 * k + 4] == 0.0);
  EXPECT(err <= 1e-9 && after < 1e-12 * before);  // installed: the frames are noise-free, the fitted bank explains them
  int mode = 0, ksize = 0;
  std::vector<double> in_force(K * 25);
  EXPECT(srmap_problem_get_blur_bank(solver.problem(), &mode, &ksize, in_force.data()) == SRMAP_OK && mode == SRMAP_BLUR_PER_FRAME && ksize == 5 && in_force == direct);
  // SetBlurBank installs what srmap_problem_set_blur_bank installs
  solver.SetBlurBank(truth);
  EXPECT(srmap_problem_get_blur_bank(solver.problem(), &mode, &ksize, in_force.data()) == SRMAP_OK && in_force == taps);
  const double with_truth = solver.ComputeAllTerms(x.data());
  EXPECT(srmap_problem_set_blur_bank(solver.problem(), SRMAP_BLUR_PER_FRAME, 5, taps.data()) == SRMAP_OK);
  EXPECT(solver.ComputeAllTerms(x.data()) == with_truth);
  std::printf(g_fail ? "BLUR BANK FACADE TESTS FAILED (%d)\n" : "BLUR BANK FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: blur_bank_test <scratch dir> [gpu|bad_mode|even_size|no_entries|short_file|long_file|missing_file|empty_module|entry|both_blurs]\n");
    return 2;
  }
  const std::string dir = argv[1];
  if (argc > 2) {
    const std::string which = argv[2];
    if (which == "gpu") return TestOnTheGpu();
    // each of these must abort inside the call; reaching the end is the failure
    BlurKernelBank b;
    if (which == "bad_mode") b.LoadFromFile(WriteFile(dir, "mode.txt", "4 1 1\n1\n"));
    else if (which == "even_size") b.LoadFromFile(WriteFile(dir, "even.txt", "1 2 1\n1 0\n0 1\n"));
    else if (which == "no_entries") b.LoadFromFile(WriteFile(dir, "none.txt", "1 3 0\n"));
    else if (which == "short_file") b.LoadFromFile(WriteFile(dir, "short.txt", "1 3 2\n1 2 3\n4 5 6\n7 8 9\n1 2 3\n"));
    else if (which == "long_file") b.LoadFromFile(WriteFile(dir, "long.txt", "2 1 2\n1 2 3\n"));
    else if (which == "missing_file") b.LoadFromFile(dir + "/no_such_bank_file.txt");
    else if (which == "empty_module") BlurModule module(b);
    else if (which == "entry") BlurKernelBank(1, 1, 2, {1.0, 2.0}).Entry(2);
    else if (which == "both_blurs") {
      ImageModelParameters params;
      params.blur_bank = BlurKernelBank(2, 1, 1, {1.0});
      params.blur_kernel = BlurKernel(1, {1.0});
      ImageModel::CreateImageModel(params);
    }
    std::printf("case '%s' did not abort\n", which.c_str());
    return 0;
  }
  TestFileFormat(dir);
  TestCanonicalCarriesTheBank(dir);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("BLUR BANK HOST TESTS PASSED\n");
  return 0;
}
