// model_tables.hpp -- the host arithmetic of problem creation (problem.hip): a restatement of the OpenCV 3.x parameter
// arithmetic the reference relies on, which must match it bit for bit (the per-pixel work itself happens in the
// kernels).  Plain C++, no HIP: tests/cpp/model_tables_test.cpp runs it on the CPU (tests/test_model_tables_cpu.py).
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace srmap {

inline int cv_round(double v) { return (int)std::lrint(v); }

// cv::warpAffine fixed-point coordinate tables for M = [1 0 dx; 0 1 dy]
// (motion_module.cpp:18-25): AB_BITS = 10, INTER_BITS = 5.
inline void warp_tables(int W, int H, double dx, double dy, std::vector<int>* X, std::vector<int>* Y) {
  double M[6] = {1.0, 0.0, dx, 0.0, 1.0, dy};
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1.0 / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
  X->resize(W);
  Y->resize(H);
  for (int x = 0; x < W; ++x)
    (*X)[x] = (cv_round((M[1] * 0 + M[2]) * 1024) + 16 + cv_round(M[0] * x * 1024)) >> 5;
  for (int y = 0; y < H; ++y)
    (*Y)[y] = (cv_round((M[4] * y + M[5]) * 1024) + 16 + cv_round(M[3] * 0 * 1024)) >> 5;
}

// One warp of one frame as the kernels take it (WarpTaps, motion_model.hpp): the integer offset, the x fraction index
// and the four bilinear weights; ytab is empty unless the y table is not uniform.
struct WarpTable {
  int ox = 0, oy = 0, ntaps = 1, fx = 0;
  double w[4] = {1.0, 0.0, 0.0, 0.0};
  std::vector<int> ytab;  // per destination row: source row << 5 | fraction index (absolute)
};
enum WarpRefusal { kWarpOk = 0, kWarpShiftTooLarge, kWarpNonUniformX };

inline WarpRefusal make_warp(int W, int H, double dx, double dy, WarpTable* out) {
  if (!(std::fabs(dx) < 16000.0) || !(std::fabs(dy) < 16000.0)) return kWarpShiftTooLarge;
  std::vector<int> X, Y;
  warp_tables(W, H, dx, dy, &X, &Y);
  for (int x = 0; x < W; ++x)
    if (X[x] != X[0] + 32 * x) return kWarpNonUniformX;  // adelta[x] + a constant: cannot happen for a pure translation
  bool uniform_y = true;
  for (int y = 0; y < H; ++y)
    if (Y[y] != Y[0] + 32 * y) uniform_y = false;
  out->ox = X[0] >> 5;
  out->oy = Y[0] >> 5;
  const int fx = X[0] & 31, fy = Y[0] & 31;
  // BilinearTab_f: float32 table; the products are exact multiples of 1/1024.
  const float tx1 = (float)fx * (1.f / 32), tx0 = 1.f - tx1;
  const float ty1 = (float)fy * (1.f / 32), ty0 = 1.f - ty1;
  out->w[0] = ty0 * tx0; out->w[1] = ty0 * tx1; out->w[2] = ty1 * tx0; out->w[3] = ty1 * tx1;
  out->ntaps = (fx == 0 && fy == 0) ? 1 : 4;
  out->fx = fx;
  out->ytab.clear();
  if (!uniform_y) {
    // dy within floating-point rounding of a 1/32-px quantisation tie: warpAffine's per-row y coordinate
    // (cvRound((y + b) * 1024) evaluated in double) lands on either side of the tie depending on the row.  The
    // kernels then read the source row and fraction of every destination row from a table.
    out->ytab = Y;
    out->ntaps = 4;
  }
  return kWarpOk;
}

// cv::resize(INTER_NEAREST) source index per destination index
// (image_data.cpp:338-350).
inline void nearest_map(int src_len, int dst_len, std::vector<int>* map) {
  const double inv_scale = (double)dst_len / src_len;
  const double ifx = 1.0 / inv_scale;
  map->resize(dst_len);
  for (int x = 0; x < dst_len; ++x) {
    const int sx = (int)std::floor(x * ifx);
    (*map)[x] = sx < src_len - 1 ? sx : src_len - 1;
  }
}

// Gaussian kernel: cv::getGaussianKernel (sigma > 0) and k * k^T, blur_module.cpp:20-22
inline void gaussian_kernel(int b, double sigma, std::vector<double>* k1, std::vector<double>* k2) {
  k1->resize(b);
  const double scale2x = -0.5 / (sigma * sigma);
  double sum = 0;
  for (int i = 0; i < b; ++i) {
    const double xx = i - (b - 1) * 0.5;
    (*k1)[i] = std::exp(scale2x * xx * xx);
    sum += (*k1)[i];
  }
  sum = 1.0 / sum;
  for (int i = 0; i < b; ++i) (*k1)[i] *= sum;
  k2->resize((size_t)b * b);
  for (int a = 0; a < b; ++a)
    for (int e = 0; e < b; ++e) (*k2)[(size_t)a * b + e] = (*k1)[a] * (*k1)[e];
}

// Whether the decimation map is s * j on both axes (cmap / rmap: nearest_map(W, w) / nearest_map(H, h)) and the NN
// upsampling used by the HR-resolution residual replicates each LR pixel exactly s * s times
// (objective_data_term.cpp:29, map_solver.cpp:80-85).
inline bool maps_regular(int W, int H, int w, int h, int s, const std::vector<int>& cmap, const std::vector<int>& rmap) {
  bool ok = (W == w * s) && (H == h * s);
  for (int j = 0; j < w && ok; ++j) ok = cmap[j] == j * s;
  for (int i = 0; i < h && ok; ++i) ok = rmap[i] == i * s;
  if (ok) {
    std::vector<int> up;
    nearest_map(w, W, &up);
    for (int x = 0; x < W && ok; ++x) ok = up[x] == x / s;
    nearest_map(h, H, &up);
    for (int y = 0; y < H && ok; ++y) ok = up[y] == y / s;
  }
  return ok;
}

}  // namespace srmap
