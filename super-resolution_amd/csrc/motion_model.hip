// motion_model.hip -- the moves of the problem's motion state (motion_model.hpp): the created tap tables, the one
// install of a replacement, and the words the refusals name a replacement by.
#include <algorithm>
#include <utility>

#include "model_tables.hpp"
#include "srmap_internal.hpp"

namespace srmap {

int MotionModel::create(srmap_problem* p, const double* shifts_xy) {
  if (!shifts_xy) return SRMAP_OK;
  const Geometry& g = p->geo;
  shifts_.assign(shifts_xy, shifts_xy + 2 * (size_t)g.K);
  fwd_.resize(g.K);
  bwd_.resize(g.K);
  kind_ = kMotionTable;
  // one warp of one frame: the tables of model_tables.hpp into the problem's tap record, the y table onto the device
  auto warp = [&](int W, int H, double dx, double dy, WarpTaps<double>* wt) -> int {
    WarpTable t;
    switch (make_warp(W, H, dx, dy, &t)) {
      case kWarpShiftTooLarge: return set_error(p->ctx, SRMAP_EUNSUPPORTED, "motion shift (%g, %g) too large", dx, dy);
      case kWarpNonUniformX: return set_error(p->ctx, SRMAP_EUNSUPPORTED, "non-uniform warpAffine x table");
      case kWarpOk: break;
    }
    wt->ox = t.ox; wt->oy = t.oy; wt->ntaps = t.ntaps; wt->fx = t.fx;
    std::copy(t.w, t.w + 4, wt->w);
    wt->ytab = nullptr;
    if (t.ytab.empty()) return SRMAP_OK;
    DevBuf d;
    if (d.alloc(sizeof(int) * t.ytab.size()) != hipSuccess ||
        hipMemcpy(d.as(), t.ytab.data(), sizeof(int) * t.ytab.size(), hipMemcpyHostToDevice) != hipSuccess)
      return set_error(p->ctx, SRMAP_ENOMEM, "hipMalloc failed");
    wt->ytab = d.as<const int>();
    d_ytabs_.push_back(std::move(d));
    return SRMAP_OK;
  };
  for (int k = 0; k < g.K; ++k) {
    if (int rc = warp(g.W, g.H, shifts_[2 * k], shifts_[2 * k + 1], &fwd_[k])) return rc;
    // the transpose warps an image of size (w*s, h*s)
    if (int rc = warp(g.w * g.s, g.h * g.s, -shifts_[2 * k], -shifts_[2 * k + 1], &bwd_[k])) return rc;
  }
  return dispatch_dtype(p->dtype, [&](auto t) {
    auto upload = [&](const std::vector<WarpTaps<double>>& src, DevBuf* dst) {  // the taps in the problem's dtype
      std::vector<WarpTaps<decltype(t)>> tmp(src.size());
      for (size_t i = 0; i < src.size(); ++i) {
        tmp[i].ox = src[i].ox; tmp[i].oy = src[i].oy; tmp[i].ntaps = src[i].ntaps; tmp[i].fx = src[i].fx;
        tmp[i].ytab = src[i].ytab;
        for (int j = 0; j < 4; ++j) tmp[i].w[j] = (decltype(t))src[i].w[j];
      }
      return upload_vector(p, tmp, dst);
    };
    if (int r = upload(fwd_, &d_fwd_)) return r;
    return upload(bwd_, &d_bwd_);
  });
}

int MotionModel::install(srmap_problem* p, Replacement&& r) {
  // evaluations in flight read the buffers about to go: drain them first
  if (int rc = model_drain(p)) return rc;
  rep_ = std::move(r);  // every buffer of the replacement before is freed
  kind_ = rep_.kind != kMotionNone ? rep_.kind : has_table() ? kMotionTable : kMotionNone;
  model_replan(p);  // "not covered" while a replacement is set
  return SRMAP_OK;
}

// per replacement kind (affine, flow, lattice): name(), setter(), sharded_name()
static const char* const kWords[3][3] = {
    {"an affine motion", "srmap_problem_set_affine_motion", "an affine motion model"},
    {"a displacement field", "srmap_problem_set_flow", "a displacement-field motion model"},
    {"a displacement field on a control lattice", "srmap_problem_set_flow_lattice", "a displacement-field motion model on a control lattice"}};
static const char* words(MotionKind kind, int column) { return kind >= kMotionAffine ? kWords[kind - kMotionAffine][column] : nullptr; }
const char* MotionModel::name() const { return words(kind_, 0); }
const char* MotionModel::setter() const { return words(kind_, 1); }
const char* MotionModel::sharded_name() const { return words(kind_, 2); }

int MotionModel::refuse(srmap_ctx* ctx, int status, const char* clause) const { return set_error(ctx, status, clause, name(), setter()); }

}  // namespace srmap
