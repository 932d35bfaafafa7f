// GPU self-test of IRLSMapSolver::RefineMotion / SolveJoint (host/optimization/irls_map_solver.h): LR frames made by the
// library's own affine model are given to a solver whose motion is off by a fraction of a pixel; RefineMotion at the
// image that made the frames must return what srmap_refine_motion returns on the same problem, bit for bit, recover the
// generating matrices, and install them; SolveJoint must end at a lower cost than the plain solve.  Run by
// tests/test_gpu_motion_refinement.py.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "image_model/image_model.h"
#include "optimization/irls_map_solver.h"
#include "optimization/regularizer.h"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      ++g_fail;                                                              \
    }                                                                        \
  } while (0)

static double CornerError(const AffineMotion& m, const AffineMotion& t, const int W, const int H) {
  double worst = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double x = (k & 1) ? W - 1.0 : 0.0, y = (k & 2) ? H - 1.0 : 0.0;
    const double dx = (m.a - t.a) * x + (m.b - t.b) * y + (m.tx - t.tx);
    const double dy = (m.c - t.c) * x + (m.d - t.d) * y + (m.ty - t.ty);
    worst = std::max(worst, std::hypot(dx, dy));
  }
  return worst;
}

int main() {
  const int W = 128, H = 96, K = 4, scale = 2;
  std::vector<double> px(static_cast<size_t>(W) * H);
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<double> coarse(18 * 14);
  for (auto& v : coarse) v = uni(rng);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double u = c / 8.0, v = r / 8.0;  // bilinear blow-up of a random grid + two sinusoids
      const int u0 = (int)u, v0 = (int)v;
      const double a = u - u0, b = v - v0;
      const double g = (1 - b) * ((1 - a) * coarse[v0 * 18 + u0] + a * coarse[v0 * 18 + u0 + 1]) +
                       b * ((1 - a) * coarse[(v0 + 1) * 18 + u0] + a * coarse[(v0 + 1) * 18 + u0 + 1]);
      px[static_cast<size_t>(r) * W + c] = 0.6 * g + 0.2 + 0.1 * std::sin(0.21 * c) * std::cos(0.17 * r);
    }
  const ImageData original(px.data(), cv::Size(W, H));
  const double cx = (W - 1) / 2.0, cy = (H - 1) / 2.0;
  const double degs[K] = {0.0, 2.0, -3.0, 0.5}, shifts[K][2] = {{0, 0}, {-3, 2}, {4.5, -2.25}, {1.25, 0.75}};
  std::vector<AffineMotion> truth, start;
  for (int i = 0; i < K; ++i) {
    const double t = degs[i] * 3.14159265358979323846 / 180.0, co = std::cos(t), si = std::sin(t);
    truth.push_back(AffineMotion(co, -si, cx - (co * cx - si * cy) + shifts[i][0], si, co, cy - (si * cx + co * cy) + shifts[i][1]));
    start.push_back(truth.back());
    if (i > 0) {  // off by (0.4, -0.3) px and a little rotation
      start.back().tx += 0.4;
      start.back().ty -= 0.3;
      start.back().b += 0.002;
      start.back().c -= 0.002;
    }
  }
  ImageModelParameters generating;
  generating.scale = scale;
  generating.blur_radius = 3;
  generating.blur_sigma = 1.0;
  generating.affine_motion_sequence = AffineMotionSequence(truth);
  const ImageModel generator = ImageModel::CreateImageModel(generating);
  std::vector<ImageData> frames;
  for (int i = 0; i < K; ++i) frames.push_back(generator.ApplyToImage(original, i));
  ImageModelParameters solving = generating;
  solving.affine_motion_sequence = AffineMotionSequence(start);
  const ImageModel solver_model = ImageModel::CreateImageModel(solving);

  IRLSMapSolverOptions options;
  {
    IRLSMapSolver solver(options, solver_model, frames, false);
    // the C entry point on the same problem, nothing installed
    srmap_motion_refinement_options o;
    srmap_motion_refinement_options_default(&o);
    o.apply = 0;
    std::vector<double> direct(6 * K), direct_quality(4 * K);
    const std::vector<double> x = original.ToPlanar();
    EXPECT(srmap_refine_motion(solver.problem(), x.data(), &o, direct.data(), direct_quality.data(), nullptr) == SRMAP_OK);
    const double before = solver.ComputeAllTerms(x.data());
    std::vector<double> quality;
    const AffineMotionSequence got = solver.RefineMotion(original, MotionRefinementOptions(), &quality);
    EXPECT(got.GetNumMotions() == K);
    EXPECT(got.Flat() == direct);  // the same numbers, bit for bit
    EXPECT(quality == direct_quality);
    const double after = solver.ComputeAllTerms(x.data());
    std::printf("data cost at the generating image: %.6e with the starting motion, %.6e with the refined one\n", before, after);
    EXPECT(after < 1e-6 * before);  // installed: the frames are noise-free, the generating matrices explain them
    for (int i = 0; i < K; ++i) {
      const double err = CornerError(got[i], truth[i], W, H);
      std::printf("frame %d: corner error %.2e HR px, cost %.3e -> %.3e, %g passes, status %g\n", i, err, quality[4 * i],
                  quality[4 * i + 1], quality[4 * i + 2], quality[4 * i + 3]);
      EXPECT(err <= 0.05);
    }
    EXPECT(got.Flat()[0] == 1.0 && got.Flat()[2] == 0.0 && quality[2] == 0.0);  // frame 0 is the gauge
    // translation only
    MotionRefinementOptions two;
    two.dof = 2;
    const AffineMotionSequence again = solver.RefineMotion(original, two);
    for (int i = 0; i < K; ++i) EXPECT(again[i].a == got[i].a && again[i].b == got[i].b && again[i].c == got[i].c && again[i].d == got[i].d);
  }
  {
    ImageData initial = frames[0];
    initial.ResizeImage(scale, INTERPOLATE_LINEAR);
    IRLSMapSolver plain(options, solver_model, frames, false), joint(options, solver_model, frames, false);
    for (IRLSMapSolver* s : {&plain, &joint})
      s->AddRegularizer(std::make_shared<BilateralTotalVariationRegularizer>(initial.GetImageSize(), 2, 0.5), 0.005);
    plain.Solve(initial);
    AffineMotionSequence refined;
    joint.SolveJoint(initial, 2, MotionRefinementOptions(), &refined);
    std::printf("final cost: plain solve %.6e, joint solve (2 rounds) %.6e\n", plain.GetReport().final_cost, joint.GetReport().final_cost);
    EXPECT(joint.GetReport().final_cost < plain.GetReport().final_cost);
    EXPECT(refined.GetNumMotions() == K);
    double worst = 0.0, worst_start = 0.0;
    for (int i = 1; i < K; ++i) {
      worst = std::max(worst, CornerError(refined[i], truth[i], W, H));
      worst_start = std::max(worst_start, CornerError(start[i], truth[i], W, H));
    }
    std::printf("largest corner error: %.3f HR px at the start, %.3f after the joint solve\n", worst_start, worst);
    EXPECT(worst < worst_start);
  }
  std::printf(g_fail ? "MOTION REFINEMENT FACADE TESTS FAILED (%d)\n" : "MOTION REFINEMENT FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
