// flow_lattice_test.cpp -- host side of the displacement field on a control lattice
// (super-resolution_amd/host/motion/flow_lattice.h): the file round trip and the reader's checks, Expand() against literals
// the numpy restatement (tests/flow_lattice_restatement.py) printed, the clamp and the degenerate forms.  No GPU needed.
// argv[1] = scratch directory; argv[2] (optional) names ONE case that must abort the process with a "Check failed" message:
// missing_file | bad_header | bad_step | few_nodes | wrong_size | trailing | empty_expand | reach | shape -- or `gpu`:
// IRLSMapSolver::SetFlowLattice / GetFlowLattice / RegisterFlowLattice against the model over the expanded field and the
// C entry points (tests/test_gpu_flow_lattice.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "image_model/image_model.h"
#include "motion/flow_lattice.h"
#include "optimization/irls_map_solver.h"
#include "optimization/regularizer.h"

using namespace super_resolution;

static int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

// exact in double: the restatement forms the same values
static std::vector<double> Nodes(const int K, const int lw, const int lh) {
  std::vector<double> n(static_cast<size_t>(K) * 2 * lw * lh);
  for (size_t i = 0; i < n.size(); ++i) n[i] = static_cast<double>((i * 37) % 101) / 8.0 - 3.0;
  return n;
}

static std::string WriteFile(const std::string& dir, const std::string& name, const std::string& header, const void* data,
                             const size_t bytes) {
  const std::string path = dir + "/" + name;
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (f) {
    std::fwrite(header.data(), 1, header.size(), f);
    if (bytes) std::fwrite(data, 1, bytes, f);
    std::fclose(f);
  }
  return path;
}

static void TestFile(const std::string& dir) {
  const int K = 2, lw = 4, lh = 3, step = 3;
  const std::vector<double> n = Nodes(K, lw, lh);
  FlowLatticeSequence seq;
  EXPECT(seq.Empty() && seq.GetNumMotions() == 0 && seq.GetStep() == 0);
  seq.LoadSequenceFromFile(WriteFile(dir, "lattice.bin", "3 4 3 2\n", n.data(), n.size() * sizeof(double)));
  EXPECT(!seq.Empty() && seq.GetNumMotions() == K && seq.GetStep() == step && seq.GetLatticeWidth() == lw && seq.GetLatticeHeight() == lh);
  EXPECT(seq.Flat() == n);
  // save / load round trip; loading replaces the sequence; the file is the header line and the raw nodes
  EXPECT(seq.SaveToFile(dir + "/lattice_copy.bin"));
  FlowLatticeSequence copy(Nodes(1, 2, 2), 64, 2, 2);
  EXPECT(copy.GetNumMotions() == 1 && copy.GetStep() == 64);
  copy.LoadSequenceFromFile(dir + "/lattice_copy.bin");
  EXPECT(copy.GetNumMotions() == K && copy.GetStep() == step && copy.Flat() == n);
  std::FILE* f = std::fopen((dir + "/lattice_copy.bin").c_str(), "rb");
  char head[16] = {0};
  EXPECT(f && std::fread(head, 1, 8, f) == 8 && std::memcmp(head, "3 4 3 2\n", 8) == 0);
  if (f) {
    std::fseek(f, 0, SEEK_END);
    EXPECT(std::ftell(f) == static_cast<long>(8 + n.size() * sizeof(double)));
    std::fclose(f);
  }
  EXPECT(!seq.SaveToFile(dir + "/no_such_directory/lattice.bin"));
  copy.Trim(1);
  EXPECT(copy.GetNumMotions() == 1 && copy.Flat() == std::vector<double>(n.begin(), n.begin() + 2 * lw * lh));
  copy.Trim(5);
  EXPECT(copy.GetNumMotions() == 1);
}

static void TestExpand() {
  const int K = 2, lw = 4, lh = 3, step = 3, W = 11, H = 8;
  const FlowLatticeSequence seq(Nodes(K, lw, lh), step, lw, lh);
  const FlowMotionSequence dense = seq.Expand(W, H);
  EXPECT(dense.GetNumMotions() == K && dense.GetWidth() == W && dense.GetHeight() == H);
  // tests/flow_lattice_restatement.py: expand(nodes, 3, 8, 11)[k][c][y][x]
  const struct { int k, c, y, x; double v; } literals[] = {
      {0, 0, 0, 0, -3.0},
      {0, 0, 1, 1, 0.4999999999999999},
      {0, 1, 2, 4, 2.2638888888888893},
      {1, 0, 5, 7, 5.138888888888889},
      {1, 1, 7, 10, -0.25},
      {0, 0, 6, 9, -2.625},
      {1, 1, 3, 3, -2.75},
      {0, 1, 7, 0, 1.125},
      {1, 0, 4, 10, 3.4583333333333326},
      {0, 0, 2, 5, 3.013888888888889},
      {1, 1, 5, 8, 3.2638888888888893},
      {0, 1, 1, 7, 2.1250000000000004},
  };
  for (const auto& l : literals) {
    double u[2] = {0, 0};
    dense.GetDisplacement(l.k, l.x, l.y, &u[0], &u[1]);
    if (u[l.c] != l.v) std::printf("expand[%d][%d][%d][%d] = %.17g, the restatement's %.17g\n", l.k, l.c, l.y, l.x, u[l.c], l.v);
    EXPECT(u[l.c] == l.v);
  }
  // beyond the last node (x >= 9, y >= 6) the field is constant
  for (int k = 0; k < K; ++k)
    for (int y = 0; y < H; ++y) {
      double a[2], b[2];
      dense.GetDisplacement(k, 9, y, &a[0], &a[1]);
      dense.GetDisplacement(k, 10, y, &b[0], &b[1]);
      EXPECT(a[0] == b[0] && a[1] == b[1]);
    }
  // step 1 with a node per pixel is the identity
  const std::vector<double> field = Nodes(1, 5, 4);
  EXPECT(FlowLatticeSequence(field, 1, 5, 4).Expand(5, 4).Flat() == field);
  // a step beyond the image with 2 x 2 nodes: one bilinear patch; the corner is node (0, 0)
  const FlowLatticeSequence two(Nodes(1, 2, 2), 64, 2, 2);
  double ux = 0, uy = 0;
  two.Expand(7, 5).GetDisplacement(0, 0, 0, &ux, &uy);
  EXPECT(ux == two.Flat()[0] && uy == two.Flat()[4]);
  // the covering lattice of an 11 x 8 image at step 3 may overhang by less than a cell: 5 x 4 nodes
  EXPECT(FlowLatticeSequence(Nodes(1, 5, 4), 3, 5, 4).Expand(11, 8).GetNumMotions() == 1);
}

static int MustAbort(const std::string& dir, const std::string& which) {
  const std::vector<double> n = Nodes(2, 4, 3);
  const size_t bytes = n.size() * sizeof(double);
  FlowLatticeSequence seq;
  if (which == "missing_file") seq.LoadSequenceFromFile(dir + "/no_such_lattice.bin");
  else if (which == "bad_header") seq.LoadSequenceFromFile(WriteFile(dir, "bad_header.bin", "3 4 3\n", n.data(), bytes));
  else if (which == "bad_step") seq.LoadSequenceFromFile(WriteFile(dir, "bad_step.bin", "0 4 3 2\n", n.data(), bytes));
  else if (which == "few_nodes") seq.LoadSequenceFromFile(WriteFile(dir, "few_nodes.bin", "3 1 12 2\n", n.data(), bytes));
  else if (which == "wrong_size") seq.LoadSequenceFromFile(WriteFile(dir, "wrong_size.bin", "3 4 3 2\n", n.data(), bytes - 8));
  else if (which == "trailing") seq.LoadSequenceFromFile(WriteFile(dir, "trailing.bin", "3 4 3 2 1\n", n.data(), bytes));
  else if (which == "empty_expand") seq.Expand(8, 8);
  else if (which == "reach") FlowLatticeSequence(n, 3, 4, 3).Expand(5, 8);  // (4 - 1) * 3 = 9 >= 5 + 3
  else if (which == "shape") FlowLatticeSequence(n, 3, 5, 3);             // 48 values are no frames of 2 x 3 x 5
  else return 2;
  std::printf("case %s did not abort\n", which.c_str());
  return 3;
}

// the facade against the model over the expanded field and against the C entry points: the same bits
static void TestSolverOnTheGpu() {
  const int K = 3, s = 2, w = 24, h = 18, W = w * s, H = h * s, step = 4;
  const int lw = (W - 1 + step - 1) / step + 1, lh = (H - 1 + step - 1) / step + 1;
  std::vector<double> n(static_cast<size_t>(K) * 2 * lw * lh);
  for (size_t i = 0; i < n.size(); ++i) n[i] = 0.3 * static_cast<double>((i * 37) % 101) / 101.0 + 0.25 * static_cast<double>(i / (2 * lw * lh));
  const FlowLatticeSequence lattice(n, step, lw, lh);
  std::vector<ImageData> frames;
  for (int k = 0; k < K; ++k) {
    std::vector<double> px(static_cast<size_t>(w) * h);
    for (size_t i = 0; i < px.size(); ++i) px[i] = 0.5 + 0.4 * std::sin(0.37 * static_cast<double>(i % w) + 0.21 * static_cast<double>(i / w) + 0.1 * k);
    frames.push_back(ImageData(px.data(), cv::Size(w, h), 1));
  }
  ImageData x0 = frames[0];
  x0.ResizeImage(s, INTERPOLATE_LINEAR);
  ImageModelParameters dense_params, plain_params;
  dense_params.scale = plain_params.scale = s;
  dense_params.blur_radius = plain_params.blur_radius = 3;
  dense_params.blur_sigma = plain_params.blur_sigma = 1.0;
  dense_params.flow_motion_sequence = lattice.Expand(W, H);
  IRLSMapSolverOptions options;
  options.max_num_irls_iterations = 2;
  options.max_num_solver_iterations = 8;
  IRLSMapSolver dense(options, ImageModel::CreateImageModel(dense_params), frames, false);
  IRLSMapSolver on_lattice(options, ImageModel::CreateImageModel(plain_params), frames, false);
  on_lattice.SetFlowLattice(lattice);
  for (IRLSMapSolver* solver : {&dense, &on_lattice})
    solver->AddRegularizer(std::make_shared<TotalVariationRegularizer>(cv::Size(W, H)), 0.01);
  const FlowLatticeSequence back = on_lattice.GetFlowLattice();
  EXPECT(back.GetStep() == step && back.GetLatticeWidth() == lw && back.GetLatticeHeight() == lh && back.Flat() == n);
  EXPECT(dense.GetFlowLattice().Empty());
  EXPECT(dense.Solve(x0).ToPlanar() == on_lattice.Solve(x0).ToPlanar());
  // an empty sequence restores the model's motion: the solver without any
  IRLSMapSolver plain(options, ImageModel::CreateImageModel(plain_params), frames, false);
  plain.AddRegularizer(std::make_shared<TotalVariationRegularizer>(cv::Size(W, H)), 0.01);
  on_lattice.SetFlowLattice(FlowLatticeSequence());
  EXPECT(on_lattice.GetFlowLattice().Empty());
  EXPECT(plain.Solve(x0).ToPlanar() == on_lattice.Solve(x0).ToPlanar());
  // RegisterFlowLattice: the registration's form (step = scale on the LR grid), image 0 at rest, the masks as the prior
  srmap_flow_registration_options registration;
  srmap_flow_registration_options_default(&registration);
  registration.smooth_radius = 4;
  const std::vector<double> quality = on_lattice.RegisterFlowLattice(0, &registration);
  const FlowLatticeSequence estimate = on_lattice.GetFlowLattice();
  EXPECT(quality.size() == 3u * K && quality[1] == 1.0);
  EXPECT(estimate.GetStep() == s && estimate.GetLatticeWidth() == w && estimate.GetLatticeHeight() == h && estimate.GetNumMotions() == K);
  bool rest = true;
  for (int i = 0; i < 2 * w * h; ++i) rest = rest && estimate.Flat()[i] == 0.0;
  EXPECT(rest && !on_lattice.GetDataPrior().empty());
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  if (argc > 2 && std::string(argv[2]) == "gpu") {
    TestSolverOnTheGpu();
    if (g_fail) return 1;
    std::printf("FLOW LATTICE GPU TESTS PASSED\n");
    return 0;
  }
  if (argc > 2) return MustAbort(dir, argv[2]);
  TestFile(dir);
  TestExpand();
  if (g_fail) return 1;
  std::printf("FLOW LATTICE HOST TESTS PASSED\n");
  return 0;
}
