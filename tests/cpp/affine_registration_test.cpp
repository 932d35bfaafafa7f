// GPU self-test of registration::AffineRegistration (host/motion/registration.h): frames warped with the library's own
// affine MotionModule are registered through the facade and through srmap_register_affine directly; the two answers must
// be the same numbers, and both close to the matrices that made the frames.  Run by tests/test_gpu_affine_registration.py.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "image_model/image_model.h"
#include "motion/registration.h"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      ++g_fail;                                                              \
    }                                                                        \
  } while (0)

int main() {
  const int W = 160, H = 120;
  std::vector<double> px(static_cast<size_t>(W) * H);
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<double> coarse(22 * 17);
  for (auto& v : coarse) v = uni(rng);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double u = c / 8.0, v = r / 8.0;  // bilinear blow-up of a random grid + two sinusoids
      const int u0 = (int)u, v0 = (int)v;
      const double a = u - u0, b = v - v0;
      const double g = (1 - b) * ((1 - a) * coarse[v0 * 22 + u0] + a * coarse[v0 * 22 + u0 + 1]) +
                       b * ((1 - a) * coarse[(v0 + 1) * 22 + u0] + a * coarse[(v0 + 1) * 22 + u0 + 1]);
      px[static_cast<size_t>(r) * W + c] = 0.6 * g + 0.2 + 0.1 * std::sin(0.21 * c) * std::cos(0.17 * r);
    }
  const ImageData original(px.data(), cv::Size(W, H));
  // rotations about the image centre plus a shift
  const double cx = (W - 1) / 2.0, cy = (H - 1) / 2.0;
  const double degs[4] = {0.0, 2.0, -3.0, 0.5}, shifts[4][2] = {{0, 0}, {-3, 2}, {4.5, -2.25}, {1.25, 0.75}};
  std::vector<AffineMotion> truth;
  for (int i = 0; i < 4; ++i) {
    const double t = degs[i] * 3.14159265358979323846 / 180.0, co = std::cos(t), si = std::sin(t);
    truth.push_back(AffineMotion(co, -si, cx - (co * cx - si * cy) + shifts[i][0], si, co, cy - (si * cx + co * cy) + shifts[i][1]));
  }
  const MotionModule motion((AffineMotionSequence(truth)));
  std::vector<ImageData> frames;
  std::vector<double> stack;
  for (int i = 0; i < 4; ++i) {
    ImageData im = original;
    motion.ApplyToImage(&im, i);
    frames.push_back(im);
    stack.insert(stack.end(), im.GetChannelData(0), im.GetChannelData(0) + static_cast<size_t>(W) * H);
  }

  for (int scale = 1; scale <= 2; ++scale) {
    std::vector<double> quality;
    const AffineMotionSequence got = registration::AffineRegistrationWithQuality(frames, scale, &quality);
    const AffineMotionSequence plain = registration::AffineRegistration(frames, scale);
    srmap_affine_registration_options options;
    srmap_affine_registration_options_default(&options);
    options.hr_scale = scale;
    std::vector<double> direct(24), direct_quality(16);
    EXPECT(srmap_register_affine(srmap_host::Context(), 4, W, H, stack.data(), &options, direct.data(), direct_quality.data()) == SRMAP_OK);
    EXPECT(got.GetNumMotions() == 4 && plain.GetNumMotions() == 4);
    EXPECT(got.Flat() == direct);    // the same numbers, bit for bit
    EXPECT(plain.Flat() == direct);
    EXPECT(quality == direct_quality);
    for (int i = 0; i < 4; ++i) {
      const AffineMotion& m = got[i];
      std::printf("scale %d frame %d: %.6f %.6f %.4f %.6f %.6f %.4f  quality %.3f %.2e %.3f %g\n", scale, i, m.a, m.b, m.tx, m.c,
                  m.d, m.ty, quality[4 * i], quality[4 * i + 1], quality[4 * i + 2], quality[4 * i + 3]);
      // against the generating matrices: corner displacement in input pixels (t comes back times scale)
      double worst = 0.0;
      for (int k = 0; k < 4; ++k) {
        const double x = (k & 1) ? W - 1.0 : 0.0, y = (k & 2) ? H - 1.0 : 0.0;
        const double dx = (m.a - truth[i].a) * x + (m.b - truth[i].b) * y + (m.tx / scale - truth[i].tx);
        const double dy = (m.c - truth[i].c) * x + (m.d - truth[i].d) * y + (m.ty / scale - truth[i].ty);
        worst = std::max(worst, std::hypot(dx, dy));
      }
      EXPECT(worst <= 0.05);
    }
  }
  EXPECT(registration::AffineRegistration({}, 2).GetNumMotions() == 0);
  std::printf(g_fail ? "AFFINE REGISTRATION FACADE TESTS FAILED (%d)\n" : "AFFINE REGISTRATION FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
