// blur_model.hpp -- the blur B of A_k = D B M_k: the one owner of the problem's blur state.  The state changes in
// BlurModel::create (once, from srmap_problem_create) and BlurModel::install (blur_model.hip) and nowhere else; both also
// write the size of the kernel in force to the problem's Geometry (geo.b, geo.hb), which is a kernel argument.
//
//   kind in force  set by                               taps() holds                       factor()   tables (device, dtype)
//   Created        srmap_problem_create, NULL to a      the Gaussian of the descriptor     its 1-D    [b*b]; table_t: the
//                  setter                               (no blur: b = 1, the one tap 1)    factor     transpose (the same bits)
//   FreeForm       srmap_problem_set_blur_kernel        the caller's b x b taps            zeros      [b*b]; table_t: the flip
//   a bank mode    srmap_problem_set_blur_bank          the caller's [entries][b][b] taps  zeros      [entries][b*b]; table_t:
//                                                                                                     the flip of every entry
//
// The free-form kernel and the bank are alternatives: installing either frees the tables of the one before, and NULL to
// either setter restores the created blur bit for bit (its taps and factor are kept for that).  table_t of a
// caller's kernel is its flip in both axes: the adjoint of a correlation (kernel.t(), the reference's form, is that only
// for a kernel symmetric under both).  install() makes every check and uploads the new tables first -- a refusal or
// failure leaves the problem exactly as it was --, then drains the evaluations in flight (model_drain), moves the tables
// in and re-plans (model_replan): the tile planner answers "not covered" for every kind but Created.
#pragma once

#include <type_traits>
#include <vector>

#include "dev_mem.hpp"
#include "srmap.h"

struct srmap_ctx;
struct srmap_problem;

namespace srmap {

constexpr int kMaxBlurTaps = 15 * 15;  // b*b taps kept in kernel-argument space
constexpr int kMaxCustomBlur = 7;      // largest size of a free-form kernel (srmap_problem_set_blur_kernel, srmap_fit_blur)

// Blur-kernel bank (srmap_problem_set_blur_bank): the blur tables hold one b x b entry per frame, per channel or per
// (frame, channel), stored [k][c]; a kernel reads entry (k, c) at table + k * frame + c * channel (elements; c the
// ABSOLUTE channel of the problem, k the absolute frame).  {0, 0} without a bank: every (k, c) reads the one kernel.
struct BlurStride {
  int frame, channel;
};
static_assert(std::is_trivially_copyable_v<BlurStride>, "a kernel argument: no owner inside");

class BlurModel {
 public:
  // the blur in force, ONE value: the created one, the free-form kernel, or (> 0) a bank by its srmap_blur_bank_mode
  enum Kind { kCreated = -1, kFreeForm = 0 };
  bool is_created() const { return kind_ == kCreated; }
  bool is_bank() const { return kind_ > kFreeForm; }
  int bank_mode() const { return is_bank() ? kind_ : 0; }  // the srmap_blur_bank_mode; 0: no bank
  const char* sharded_name() const;  // in the words of refuse_sharded (shard_eval.hip); nullptr for the created blur
  // SRMAP_EINVAL unless `mode` is a srmap_blur_bank_mode; the entries of a bank of that mode (1 for mode 0)
  static int check_bank_mode(srmap_ctx* ctx, int mode);
  static int entries(int mode, int K, int C);
  // host taps: every entry in force ([entries][b][b]; one entry without a bank, which is also entry 0's place), the
  // separable factor (b; zeros unless created), the b*b of the entry that frame k, channel c read
  const std::vector<double>& taps() const { return taps_; }
  const double* factor() const { return factor_.data(); }
  const double* entry_taps(int k, int c) const { return taps_.data() + (size_t)(k * entry_.frame + c * entry_.channel) * bb(); }
  BlurStride stride() const { return {entry_.frame * bb(), entry_.channel * bb()}; }
  template <typename T = void>
  const T* table() const { return d_table_.as<const T>(); }
  template <typename T>
  const T* table_t() const { return d_table_t_.as<const T>(); }

  // srmap_problem_create: the Gaussian of (ksize, sigma), or no blur (ksize 0)
  int create(srmap_problem* p, int ksize, double sigma);
  // The blur from the caller's taps: the tables of a bank of `bank_mode` (0: the one free-form kernel) of ksize x ksize,
  // or the created blur for taps == NULL
  int install(srmap_problem* p, int bank_mode, int ksize, const double* taps);

 private:
  int bb() const { return (int)(factor_.size() * factor_.size()); }  // taps per entry
  int kind_ = kCreated;
  BlurStride entry_ = {0, 0};  // entry (k, c) of the bank in force: k * frame + c * channel
  std::vector<double> taps_, factor_;
  struct { std::vector<double> taps, factor; } created_;  // taps: also their own transpose (create())
  DevBuf d_table_, d_table_t_;
};

}  // namespace srmap
