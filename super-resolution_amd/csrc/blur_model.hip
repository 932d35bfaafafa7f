// blur_model.hip -- the moves of the problem's blur state (blur_model.hpp): the created Gaussian (what the reference's
// BlurModule builds, blur_module.cpp:13-22) and the one install of a free-form kernel, a bank, or the created blur again.
#include <cmath>
#include <utility>

#include "model_tables.hpp"
#include "srmap_internal.hpp"

namespace srmap {

// the two device tables, in the problem's dtype, of host taps and their transposes / flips
static int upload_tables(srmap_problem* p, const std::vector<double>& taps, const std::vector<double>& taps_t, DevBuf* table, DevBuf* table_t) {
  return dispatch_dtype(p->dtype, [&](auto t) {
    if (int r = upload_vector(p, std::vector<decltype(t)>(taps.begin(), taps.end()), table)) return r;
    return upload_vector(p, std::vector<decltype(t)>(taps_t.begin(), taps_t.end()), table_t);
  });
}

int BlurModel::check_bank_mode(srmap_ctx* ctx, int mode) {
  if (mode == SRMAP_BLUR_PER_FRAME || mode == SRMAP_BLUR_PER_CHANNEL || mode == SRMAP_BLUR_PER_FRAME_CHANNEL) return SRMAP_OK;
  return set_error(ctx, SRMAP_EINVAL, "unknown blur bank mode %d", mode);
}

int BlurModel::entries(int mode, int K, int C) {
  return mode == SRMAP_BLUR_PER_FRAME ? K : mode == SRMAP_BLUR_PER_CHANNEL ? C : mode == SRMAP_BLUR_PER_FRAME_CHANNEL ? K * C : 1;
}

const char* BlurModel::sharded_name() const { return is_bank() ? "a blur-kernel bank" : is_created() ? nullptr : "a free-form blur kernel"; }

int BlurModel::create(srmap_problem* p, int ksize, double sigma) {
  Geometry& g = p->geo;
  g.b = ksize > 0 ? ksize : 1;
  g.hb = (g.b - 1) / 2;
  created_.taps.assign((size_t)g.b * g.b, 1.0);
  created_.factor.assign((size_t)g.b, 1.0);
  if (ksize > 0) gaussian_kernel(g.b, sigma, &created_.factor, &created_.taps);
  taps_ = created_.taps;
  factor_ = created_.factor;
  // the created blur is the outer product of its factor with itself, so it is its own transpose bit for bit (IEEE
  // products commute) and one host array fills both tables
  return upload_tables(p, created_.taps, created_.taps, &d_table_, &d_table_t_);
}

int BlurModel::install(srmap_problem* p, int bank_mode, int ksize, const double* taps) {
  const char* what = bank_mode ? "blur bank" : "blur kernel";
  const int n = entries(bank_mode, p->geo.K, p->geo.C);
  if (taps) {
    if (ksize < 1 || ksize % 2 != 1) return set_error(p->ctx, SRMAP_EINVAL, "%s size must be odd and >= 1 (got %d)", what, ksize);
    if (ksize > kMaxCustomBlur)
      return set_error(p->ctx, SRMAP_EUNSUPPORTED, "%s size %d: a free-form kernel has at most %d x %d taps", what, ksize, kMaxCustomBlur, kMaxCustomBlur);
    for (int i = 0; i < n * ksize * ksize; ++i)
      if (!std::isfinite(taps[i])) return set_error(p->ctx, SRMAP_EINVAL, "%s: tap %d is not finite", what, i);
  }
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const int b = taps ? ksize : (int)created_.factor.size();
  const size_t bb = (size_t)b * b;
  std::vector<double> k2 = created_.taps, k2t = created_.taps;  // (its own transpose: create())
  if (taps) {
    k2.assign(taps, taps + (size_t)n * bb);
    k2t.resize(k2.size());
    for (int q = 0; q < n; ++q)  // the flip in both axes, per entry of a bank
      for (int a = 0; a < b; ++a)
        for (int e = 0; e < b; ++e) k2t[q * bb + (size_t)a * b + e] = k2[q * bb + (size_t)(b - 1 - a) * b + (b - 1 - e)];
  }
  // the new tables first: a failed allocation leaves the problem as it was
  DevBuf nb, nbt;
  if (int rc = upload_tables(p, k2, k2t, &nb, &nbt)) return rc;
  // evaluations in flight read the old tables: drain them before the buffers change
  if (int rc = model_drain(p)) return rc;
  d_table_ = std::move(nb);  // the new tables move in; the old ones are freed
  d_table_t_ = std::move(nbt);
  kind_ = taps ? bank_mode : kCreated;
  entry_ = {kind_ == SRMAP_BLUR_PER_FRAME ? 1 : kind_ == SRMAP_BLUR_PER_FRAME_CHANNEL ? p->geo.C : 0,
            kind_ == SRMAP_BLUR_PER_CHANNEL || kind_ == SRMAP_BLUR_PER_FRAME_CHANNEL ? 1 : 0};
  taps_.swap(k2);
  factor_ = taps ? std::vector<double>((size_t)b, 0.0) : created_.factor;  // a free-form kernel has no separable factor
  p->geo.b = b;
  p->geo.hb = (b - 1) / 2;
  model_replan(p);  // "not covered" while a free-form kernel or a bank is set
  return SRMAP_OK;
}

}  // namespace srmap
