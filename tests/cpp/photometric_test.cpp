// photometric_test.cpp -- host side of the photometric frame model (super-resolution_amd/host/image_model/photometric.h,
// csrc/photometric_host.hpp, IRLSMapSolver::SetPhotometric / FitPhotometric / SolvePhotometric).
//   photometric_test <scratch dir>            file format and round trip; the plain-C++ per-frame solve against closed forms,
//                                             with its statuses.  No GPU needed.
//   photometric_test <scratch dir> <case>     ONE case that must abort the process with a "Check failed" message:
//                                             short_line | long_line | bad_gain | not_a_number | missing_file | index
//   photometric_test <scratch dir> gpu        (needs the GPU; run by tests/test_gpu_photometric.py) the facade returns what
//                                             the C entry points return, bit for bit, recovers the exposure that made the
//                                             frames, and installs it.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "image_model/image_model.h"
#include "image_model/photometric.h"
#include "optimization/irls_map_solver.h"
#include "photometric_host.hpp"

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

static void TestFileFormat(const std::string& dir) {
  PhotometricSequence seq;
  EXPECT(seq.Empty() && seq.GetNumFrames() == 0);
  seq.LoadSequenceFromFile(WriteFile(dir, "three.txt", "1 0\n\n1.08\t0.03\r\n  0.9 -2.5e-2  \n"));
  EXPECT(seq.GetNumFrames() == 3);
  EXPECT(seq[0].gain == 1.0 && seq[0].bias == 0.0 && seq[1].gain == 1.08 && seq[1].bias == 0.03 && seq[2].gain == 0.9 && seq[2].bias == -0.025);
  EXPECT((seq.Flat() == std::vector<double>{1.0, 0.0, 1.08, 0.03, 0.9, -0.025}));
  // a saved sequence loads again bit for bit
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> uni(-0.1, 0.1);
  std::vector<Photometric> frames;
  for (int i = 0; i < 7; ++i) frames.push_back(Photometric(1.0 + uni(rng), uni(rng)));
  const PhotometricSequence seven(frames);
  EXPECT(seven.SaveToFile(dir + "/seven.txt"));
  PhotometricSequence back;
  back.LoadSequenceFromFile(dir + "/seven.txt");
  EXPECT(back.GetNumFrames() == 7 && back.Flat() == seven.Flat());
  EXPECT(!seven.SaveToFile(dir + "/no_such_dir/seven.txt"));
  // from the C ABI's K x 2 block
  const double flat[4] = {1.5, 0.25, 0.75, -0.5};
  const PhotometricSequence two(flat, 2);
  EXPECT(two.GetNumFrames() == 2 && two[1].gain == 0.75 && two[1].bias == -0.5);
  // data generation: gain * pixel + bias
  const double px[6] = {0.0, 0.25, 0.5, 0.75, 1.0, 0.125};
  ImageData image(px, cv::Size(3, 2));
  two.ApplyToImage(&image, 0);
  EXPECT(image.GetPixelValue(0, 0) == 0.25 && image.GetPixelValue(0, 2) == 1.0 && image.GetPixelValue(0, 4) == 1.75);
}

// the six sums of y = a s + b + noise over a small set, accumulated directly
static void Sums(const std::vector<double>& s, const std::vector<double>& y, const std::vector<double>& w, double* S) {
  for (int q = 0; q < srmap::kPhotoSums; ++q) S[q] = 0.0;
  for (size_t i = 0; i < s.size(); ++i) {
    S[0] += w[i]; S[1] += w[i] * s[i]; S[2] += w[i] * y[i];
    S[3] += w[i] * s[i] * s[i]; S[4] += w[i] * s[i] * y[i]; S[5] += w[i] * y[i] * y[i];
  }
}

static void TestSolve() {
  using namespace srmap;
  const std::vector<double> s = {0.0, 1.0, 2.0, 3.0}, w1(4, 1.0);
  double S[kPhotoSums];
  {  // exact data: y = 2 s + 0.5
    std::vector<double> y;
    for (const double v : s) y.push_back(2.0 * v + 0.5);
    Sums(s, y, w1, S);
    const PhotometricFit f = photometric_solve(S, kPhotoGainBias, 1.0, 0.0, 0.25, 4.0);
    EXPECT(f.status == 0 && std::fabs(f.gain - 2.0) <= 1e-14 && std::fabs(f.bias - 0.5) <= 1e-14);
    // E at (1, 0): sum (s + 0.5)^2 = 0.25 + 2.25 + 6.25 + 12.25
    EXPECT(std::fabs(f.e0 - 21.0) <= 1e-12 && std::fabs(f.e1) <= 1e-12);
    EXPECT(std::fabs(photometric_energy(S, 2.0, 0.0) - 4 * 0.25) <= 1e-12);
    // the bounds: status 2 keeps the parameters in force, and E stays
    const PhotometricFit lo = photometric_solve(S, kPhotoGainBias, 1.25, 0.125, 0.25, 1.5);
    EXPECT(lo.status == 2 && lo.gain == 1.25 && lo.bias == 0.125 && lo.e1 == lo.e0);
    const PhotometricFit hi = photometric_solve(S, kPhotoGainBias, 1.0, 0.0, 2.5, 4.0);
    EXPECT(hi.status == 2 && hi.gain == 1.0 && hi.bias == 0.0);
    // the bounds are inclusive
    EXPECT(photometric_solve(S, kPhotoGainOnly, 1.0, 0.5, 2.0, 2.0).status == 0);
  }
  {  // closed forms of the line through noisy points: y = {1, 3, 2, 6}: slope 1.4, intercept 0.9
    const std::vector<double> y = {1.0, 3.0, 2.0, 6.0};
    Sums(s, y, w1, S);
    const PhotometricFit f = photometric_solve(S, kPhotoGainBias, 1.0, 0.0, 0.25, 4.0);
    EXPECT(f.status == 0 && std::fabs(f.gain - 1.4) <= 1e-14 && std::fabs(f.bias - 0.9) <= 1e-14);
    EXPECT(std::fabs(f.e1 - 4.2) <= 1e-12);  // residuals 0.1, -0.7, 1.7, -0.9... squared: 0.01 + 0.49 + 2.89 + 0.81
    // gain only, the bias in force held: a = sum s (y - b) / sum s^2
    const PhotometricFit g = photometric_solve(S, kPhotoGainOnly, 1.0, 0.5, 0.25, 4.0);
    EXPECT(g.status == 0 && g.bias == 0.5 && std::fabs(g.gain - (25.0 - 0.5 * 6.0) / 14.0) <= 1e-14);
    // bias only, the gain in force held: b = mean(y - a s)
    const PhotometricFit b = photometric_solve(S, kPhotoBiasOnly, 1.5, 0.0, 0.25, 4.0);
    EXPECT(b.status == 0 && b.gain == 1.5 && std::fabs(b.bias - (12.0 - 1.5 * 6.0) / 4.0) <= 1e-14);
    // weights: a zero weight removes the point (the line through the remaining three)
    const std::vector<double> w = {1.0, 1.0, 1.0, 0.0};
    Sums(s, y, w, S);
    const PhotometricFit f3 = photometric_solve(S, kPhotoGainBias, 1.0, 0.0, 0.25, 4.0);
    EXPECT(f3.status == 0 && std::fabs(f3.gain - 0.5) <= 1e-14 && std::fabs(f3.bias - 1.5) <= 1e-14);
  }
  {  // degenerate: no weight; a flat frame
    const std::vector<double> y = {1.0, 3.0, 2.0, 6.0}, w0(4, 0.0), flat(4, 0.75);
    Sums(s, y, w0, S);
    const PhotometricFit none = photometric_solve(S, kPhotoGainBias, 1.25, 0.125, 0.25, 4.0);
    EXPECT(none.status == 3 && none.gain == 1.25 && none.bias == 0.125);
    EXPECT(photometric_solve(S, kPhotoBiasOnly, 1.25, 0.125, 0.25, 4.0).status == 3);
    Sums(flat, y, w1, S);
    const PhotometricFit fl = photometric_solve(S, kPhotoGainBias, 1.25, 0.125, 0.25, 4.0);
    EXPECT(fl.status == 3 && fl.gain == 1.25 && fl.bias == 0.125 && fl.e1 == fl.e0);
    EXPECT(photometric_solve(S, kPhotoBiasOnly, 1.0, 0.0, 0.25, 4.0).status == 0);  // the mean offset is still defined
    const std::vector<double> zero(4, 0.0);
    Sums(zero, y, w1, S);
    EXPECT(photometric_solve(S, kPhotoGainOnly, 1.0, 0.0, 0.25, 4.0).status == 3);
  }
}

// ---- GPU part ----
static std::vector<double> Scene(const int W, const int H) {
  std::vector<double> px(static_cast<size_t>(W) * H);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c)
      px[static_cast<size_t>(r) * W + c] = 0.5 + 0.25 * std::sin(0.21 * c) * std::cos(0.17 * r) + 0.15 * std::sin(0.05 * (c + 2 * r));
  return px;
}

static int TestOnTheGpu() {
  const int W = 64, H = 48, K = 4, scale = 2;
  const std::vector<double> px = Scene(W, H);
  const ImageData original(px.data(), cv::Size(W, H));
  ImageModelParameters parameters;
  parameters.scale = scale;
  parameters.blur_radius = 3;
  parameters.blur_sigma = 1.0;
  parameters.motion_sequence.SetMotionSequence({MotionShift(0, 0), MotionShift(1.25, 0.75), MotionShift(0.5, 1), MotionShift(1, 0.25)});
  const ImageModel model = ImageModel::CreateImageModel(parameters);
  const PhotometricSequence truth({Photometric(1.0, 0.0), Photometric(1.08, 0.03), Photometric(0.94, -0.02), Photometric(1.05, 0.01)});
  std::vector<ImageData> frames;
  for (int i = 0; i < K; ++i) {
    frames.push_back(model.ApplyToImage(original, i));
    truth.ApplyToImage(&frames.back(), i);
  }
  IRLSMapSolverOptions options;
  IRLSMapSolver solver(options, model, frames, false);
  const std::vector<double> x = original.ToPlanar();
  const double ignored = solver.ComputeAllTerms(x.data());
  // nothing set: ones and zeros
  EXPECT((solver.GetPhotometric().Flat() == std::vector<double>{1, 0, 1, 0, 1, 0, 1, 0}));
  // the facade returns the C entry point's numbers
  srmap_photometric_fit_options o;
  srmap_photometric_fit_options_default(&o);
  o.apply = 0;
  std::vector<double> direct(2 * K), direct_quality(4 * K);
  EXPECT(srmap_fit_photometric(solver.problem(), x.data(), &o, direct.data(), direct_quality.data(), nullptr) == SRMAP_OK);
  std::vector<double> quality;
  const PhotometricSequence got = solver.FitPhotometric(original, PhotometricFitOptions(), &quality);
  EXPECT(got.Flat() == direct && quality == direct_quality);
  double err = 0.0;
  for (int i = 0; i < 2 * K; ++i) err = std::max(err, std::fabs(got.Flat()[i] - truth.Flat()[i]));
  const double fitted = solver.ComputeAllTerms(x.data());
  std::printf("largest parameter error %.2e; data cost at the generating image %.6e ignoring the exposure, %.6e with the fit\n", err, ignored, fitted);
  EXPECT(err <= 1e-12);
  EXPECT(fitted < 1e-20 * ignored + 1e-24);  // installed: the frames are noise-free, the normalised frames match the model
  EXPECT(solver.GetPhotometric().Flat() == direct);
  // SetPhotometric with the truth gives the same cost; an empty sequence restores the raw frames bit for bit
  solver.SetPhotometric(PhotometricSequence());
  EXPECT(solver.ComputeAllTerms(x.data()) == ignored);
  solver.SetPhotometric(truth);
  EXPECT(solver.ComputeAllTerms(x.data()) < 1e-20 * ignored + 1e-24);
  solver.SetPhotometric(PhotometricSequence());
  // SolvePhotometric ends with parameters in force and a finite estimate
  ImageData x0 = frames[0];
  x0.ResizeImage(scale, INTERPOLATE_LINEAR);
  PhotometricSequence last;
  const ImageData result = solver.SolvePhotometric(x0, 1, PhotometricFitOptions(), &last);
  EXPECT(last.GetNumFrames() == K && last.Flat() == solver.GetPhotometric().Flat());
  EXPECT(last[0].gain == 1.0 && last[0].bias == 0.0);  // the gauge
  double gain_err = 0.0;
  for (int i = 0; i < K; ++i) gain_err = std::max(gain_err, std::fabs(last[i].gain - truth[i].gain));
  std::printf("SolvePhotometric(1 round): largest gain error %.4f\n", gain_err);
  EXPECT(gain_err <= 0.05);
  EXPECT(std::isfinite(result.GetPixelValue(0, 0)));
  std::printf(g_fail ? "PHOTOMETRIC FACADE TESTS FAILED (%d)\n" : "PHOTOMETRIC FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: photometric_test <scratch dir> [gpu|short_line|long_line|bad_gain|not_a_number|missing_file|index]\n");
    return 2;
  }
  const std::string dir = argv[1];
  if (argc > 2) {
    const std::string which = argv[2];
    if (which == "gpu") return TestOnTheGpu();
    // each of these must abort inside the call; reaching the end is the failure
    PhotometricSequence seq;
    if (which == "short_line") seq.LoadSequenceFromFile(WriteFile(dir, "short.txt", "1 0\n1.05\n"));
    else if (which == "long_line") seq.LoadSequenceFromFile(WriteFile(dir, "long.txt", "1 0 0\n"));
    else if (which == "bad_gain") seq.LoadSequenceFromFile(WriteFile(dir, "bad.txt", "1 0\n1 0\n0 0.5\n"));
    else if (which == "not_a_number") seq.LoadSequenceFromFile(WriteFile(dir, "nan.txt", "1 zero\n"));
    else if (which == "missing_file") seq.LoadSequenceFromFile(dir + "/no_such_photometric_file.txt");
    else if (which == "index") PhotometricSequence({Photometric(1.0, 0.0)})[1];
    std::printf("case '%s' did not abort\n", which.c_str());
    return 0;
  }
  TestFileFormat(dir);
  TestSolve();
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("PHOTOMETRIC HOST TESTS PASSED\n");
  return 0;
}
