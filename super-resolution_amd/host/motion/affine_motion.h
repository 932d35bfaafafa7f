// AffineMotion / AffineMotionSequence: per-frame 2 x 3 matrices [a b tx; c d ty] in HR pixel coordinates, (x, y) order --
// content at p in the HR image sits at L p + t in the frame's HR-grid image (MotionShift's convention: the shift (dx, dy)
// is [1 0 dx; 0 1 dy]).  No reference counterpart (its MotionModule warps by a MotionShift only, motion_module.cpp:18-51);
// the class mirrors MotionShiftSequence (src/motion/motion_shift.h:14-57), loadable from a text file of
// "a b tx c d ty" lines and writable as one (SaveToFile).  The matrices go to srmap_problem_set_affine_motion (include/srmap.h), which states the domain.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "util/number_file.h"
#include "util/srmap_host.h"

namespace super_resolution {

struct AffineMotion {
  AffineMotion(const double a, const double b, const double tx, const double c, const double d, const double ty)
      : a(a), b(b), tx(tx), c(c), d(d), ty(ty) {}
  double a, b, tx, c, d, ty;
};

class AffineMotionSequence {
 public:
  AffineMotionSequence() {}
  explicit AffineMotionSequence(const std::vector<AffineMotion>& motions) : motions_(motions) {}
  void SetMotionSequence(const std::vector<AffineMotion>& motions) { motions_ = motions; }
  // one frame per line, six numbers; blank lines are skipped, anything else is an error
  void LoadSequenceFromFile(const std::string& path) {
    motions_.clear();
    srmap_host::ReadNumberLines(path, 6, "six numbers 'a b tx c d ty'", [this](const double* v, const std::string&) {
      motions_.push_back(AffineMotion(v[0], v[1], v[2], v[3], v[4], v[5]));
    });
  }
  // the same format, every number with 17 significant digits (it loads again bit for bit)
  bool SaveToFile(const std::string& path) const {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    for (const AffineMotion& m : motions_) std::fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", m.a, m.b, m.tx, m.c, m.d, m.ty);
    return std::fclose(f) == 0;
  }
  int GetNumMotions() const { return static_cast<int>(motions_.size()); }
  const AffineMotion& GetAffineMotion(const int index) const {
    if (index < 0 || index >= GetNumMotions()) srmap_host::Fail("affine motion index out of range");
    return motions_[index];
  }
  const AffineMotion& operator[](const int index) const { return GetAffineMotion(index); }
  std::vector<double> Flat() const {
    std::vector<double> f;
    for (const auto& m : motions_) for (const double v : {m.a, m.b, m.tx, m.c, m.d, m.ty}) f.push_back(v);
    return f;
  }

 private:
  std::vector<AffineMotion> motions_;
};

}  // namespace super_resolution
