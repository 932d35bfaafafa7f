// data_prior_test.cpp -- the facade side of the persistent prior on the data weights and of the registration from a
// solver's own observations (IRLSMapSolver::SetDataPrior / GetDataPrior / RegisterFlow of
// super-resolution_amd/host/optimization/irls_map_solver.h) against the C entry points.  Needs a GPU
// (tests/test_gpu_data_prior.py runs it).
#include <cmath>
#include <cstdio>
#include <vector>

#include "image_model/image_model.h"
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

int main() {
  const int w = 40, h = 28, K = 3, scale = 2;
  std::vector<ImageData> frames;
  for (int k = 0; k < K; ++k) {
    const std::vector<double> px = Frame(k, w, h);
    ImageData im(px.data(), cv::Size(w, h));
    std::vector<double> second(px);
    for (double& v : second) v = 0.8 * v;
    im.AddChannel(second.data(), cv::Size(w, h));
    frames.push_back(im);
  }
  const size_t n = static_cast<size_t>(w) * h;
  std::vector<double> valid;
  const FlowMotionSequence sequence = registration::FlowRegistration(frames, scale, &valid);
  ImageModelParameters params;
  params.scale = scale;
  params.blur_radius = 3;
  params.blur_sigma = 1.0;
  params.flow_motion_sequence = sequence;
  const ImageModel model = ImageModel::CreateImageModel(params);
  IRLSMapSolverOptions options;
  options.max_num_irls_iterations = 2;
  options.data_loss = HUBER_DATA_LOSS;
  options.huber_delta = 0.02;
  IRLSMapSolver solver(options, model, frames, false);
  EXPECT(solver.GetDataPrior().empty());
  // the masks broadcast over both channels are the prior, and the weights
  solver.SetDataPrior(valid);
  const std::vector<double> prior = solver.GetDataPrior();
  EXPECT(prior.size() == 2 * valid.size());
  bool same = true, any_zero = false;
  for (int k = 0; k < K; ++k)
    for (int c = 0; c < 2; ++c)
      for (size_t i = 0; i < n; ++i) {
        same = same && prior[(static_cast<size_t>(k) * 2 + c) * n + i] == valid[k * n + i];
        any_zero = any_zero || valid[k * n + i] == 0.0;
      }
  EXPECT(same && any_zero);
  EXPECT(solver.GetDataWeights() == prior);
  // a Huber solve keeps what the masks remove, and down-weights elsewhere
  ImageData start = frames[0];
  start.ResizeImage(scale, INTERPOLATE_LINEAR);
  const ImageData result = solver.Solve(start);
  EXPECT(result.GetImageSize() == cv::Size(w * scale, h * scale) && solver.GetReport().cg_iterations > 0);
  const std::vector<double> after = solver.GetDataWeights();
  bool held = true, bounded = true;
  for (size_t i = 0; i < after.size(); ++i) {
    held = held && (prior[i] != 0.0 || after[i] == 0.0);
    bounded = bounded && after[i] <= prior[i];
  }
  EXPECT(held && bounded);
  EXPECT(solver.GetDataPrior() == prior);
  // an empty vector removes it
  solver.SetDataPrior(std::vector<double>());
  EXPECT(solver.GetDataPrior().empty());
  // RegisterFlow: the first channel's registration at the solver's scale is FlowRegistration's, bit for bit
  std::vector<double> q_host;
  registration::FlowRegistration(frames, scale, nullptr, &q_host);
  const std::vector<double> q = solver.RegisterFlow(0);
  EXPECT(q == q_host);
  const std::vector<double> installed = solver.GetDataPrior();
  EXPECT(installed == prior);
  EXPECT(solver.RegisterFlow(-1, nullptr, false).size() == 3 * static_cast<size_t>(K) && solver.GetDataPrior() == prior);
  std::printf(g_fail ? "DATA PRIOR FACADE TESTS FAILED (%d)\n" : "DATA PRIOR FACADE TESTS PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
