// data_weights.hpp -- the per-observation weights of the data term ([K][C][h][w], problem dtype): the caller's weights
// w (srmap_set_data_weights*), the persistent prior m (srmap_set_data_prior*) and the loss (srmap_problem_set_data_loss).
// One type owns the three buffers; the moves between them happen in data_weights.hip and nowhere else.
//
// Buffers.  eff: what every kernel reads (effective<T>(); none = all ones, the unweighted kernels).  user: the caller's
// factor while a prior is set (none = ones).  prior: m.
//
//   prior  user's w  loss   | eff holds                    user holds   robust()
//   -      -         L2     | nothing                      nothing      no      (*)
//   -      w         L2     | w                            nothing      yes
//   -      -         Huber  | ones, then huber(r)          nothing      yes
//   -      w         Huber  | w, then huber(r)             nothing      yes
//   m      - / w     L2     | m .* w (one rounding)        w / nothing  yes
//   m      - / w     Huber  | m .* w, then m .* huber(r)   w / nothing  yes
//
// Without a prior eff IS the caller's buffer, and a Huber loss owns it as well: huber_step() overwrites the caller's
// weights, and setting "no weights" under Huber gives a buffer of ones instead of none.  (*) Going from Huber back to L2
// keeps eff and its contents (the last outlier map): the first row is reached again by setting "no weights".
// The first prior of a problem moves eff -- whatever it holds -- to user and makes eff the product's buffer; removing the
// prior moves user back (ones under Huber if it was empty).  A Huber step leaves user alone: the next set_user or
// set_prior forms m .* w from it again.
//
// A hold-out (srmap_problem_set_holdout; holdout_host.hpp: h[i] in {0, 1} from the index) is a FACTOR OF THE PRIOR.  While
// one is set every row above is read with m replaced by m .* (1 - h) -- exact, h being 0 or 1 --, and the rows without a
// prior become rows with the prior (1 - h):
//
//   hold-out  caller's m | prior holds       caller holds   prior() (what every reader sees)   caller_prior()
//   -         -          | nothing           nothing        none                                none
//   -         m          | m                 nothing        m                                   m
//   h         -          | 1 - h             nothing        1 - h                               none
//   h         m          | m .* (1 - h)      m              m .* (1 - h)                        m
//
// The product is formed once per change of either factor by one elementwise kernel (holdout.hip) that computes h from the
// index and reads m only if there is one.  Setting a hold-out on a problem without a prior is the move "the first prior"
// below; lifting it gives the caller's m back as it was given, or is the move "removing the prior".  A problem with a
// hold-out therefore evaluates bit for bit as one whose caller set the prior m .* (1 - h) itself.
//
// robust() == (eff is allocated || Huber): every evaluation then runs a WEIGHTED forward kernel, and the tile plan takes
// its forward-residual form for integer shifts too (ztile_plan.hip).  A transition re-plans
// (model_replan) exactly when it changes robust(): into or out of the first row.
//
// Writes are ordered as include/srmap.h "Streams" says: a setter drains the last evaluation's stream before it writes
// and is complete on return; huber_step() and reset() are enqueued.
#pragma once

#include <hip/hip_runtime.h>

#include "dev_mem.hpp"
#include "srmap.h"

struct srmap_problem;

namespace srmap {

// Where a factor comes from: host doubles (converted to the dtype), a device array of the dtype (copied on st), or
// nothing (the factor is removed).  st: the stream the write is enqueued on and waited for
struct WeightSource {
  const double* host = nullptr;
  const void* dev = nullptr;
  hipStream_t st = nullptr;
  bool none() const { return !host && !dev; }
};

class DataWeights {
 public:
  template <typename T>
  const T* effective() const { return eff_.as<const T>(); }  // nullptr: all ones
  template <typename T>
  const T* prior() const { return prior_.as<const T>(); }  // nullptr: none; with a hold-out, the product with 1 - h
  // what the caller set (srmap_get_data_prior, and the base weight of the hold-out score); nullptr: none
  template <typename T>
  const T* caller_prior() const { return (hold_.threshold ? caller_ : prior_).as<const T>(); }
  // the caller's weights while a prior or a hold-out keeps them in the second buffer; nullptr: none, or not kept apart
  template <typename T>
  const T* user() const { return user_.as<const T>(); }
  // the hold-out in force: observation i is held out iff lo <= hash24(i, seed) < threshold (holdout_host.hpp); threshold
  // 0 = none.  A fraction is the band [0, T), folds = 0; fold `fold` of `folds` (srmap_problem_set_holdout_fold) is its
  // band of the partition, fraction = (threshold - lo) / 2^24
  struct Holdout { unsigned threshold = 0; unsigned long long seed = 0; double fraction = 0.0; unsigned lo = 0; int folds = 0, fold = 0; };
  const Holdout& holdout() const { return hold_; }
  // whether a Huber step in the MAD mode has left its delta in the problem's record (residual_scale.hip) since the loss
  // and the scale rule in force were set
  bool mad_delta_recorded() const { return mad_recorded_; }
  bool robust() const { return eff_ || loss_ == SRMAP_DATA_LOSS_HUBER; }
  int loss() const { return loss_; }
  double delta() const { return delta_; }
  // Where a Huber step takes its delta from (srmap_problem_set_huber_scale): SRMAP_HUBER_DELTA_FIXED -- delta() --, or
  // SRMAP_HUBER_DELTA_MAD: max(tuning * 1.4826 median|r|, min_delta) of the step's own residuals, formed on the device
  // (residual_scale.hip).  Read under a Huber loss only; no other setter touches it
  int scale_mode() const { return scale_mode_; }
  void set_scale(int mode, double tuning, double min_delta) {
    // a change of the rule forgets the last step's delta: "the problem's delta" is then unknown until a step has run
    // (setting the rule in force again, as a caller does before every solve, keeps it)
    if (mode != scale_mode_ || tuning != tuning_ || min_delta != min_delta_) mad_recorded_ = false;
    scale_mode_ = mode; tuning_ = tuning; min_delta_ = min_delta;
  }

  int set_user(srmap_problem* p, const WeightSource& src);
  int set_prior(srmap_problem* p, const WeightSource& src);
  int set_loss(srmap_problem* p, int loss, double huber_delta);
  // the hold-out {threshold, seed, fraction}; threshold 0 lifts it.  On the context's stream, complete on return
  int set_holdout(srmap_problem* p, const Holdout& h);
  // the start of a Huber solve on the channels [c0, c0 + C) (C = 0: all): eff <- the prior, or 1 without one; enqueued on st
  int reset(srmap_problem* p, int c0, int C, hipStream_t st);
  // Huber IRLS step on the channels [c0, c0 + C) (C = 0: all): eff <- prior .* huber(A x - y), enqueued on st
  // (srmap_update_data_weights_device with a view: split_channels solves re-weight one channel at a time).  In the MAD
  // mode the select runs over the view's residuals between the two kernels and the weights read delta from its record
  int huber_step(srmap_problem* p, int c0, int C, const void* x, hipStream_t st);

 private:
  int ensure_ones(srmap_problem* p, hipStream_t st);
  int rebuild(srmap_problem* p, hipStream_t st);
  int enter_prior(srmap_problem* p, hipStream_t st);
  int leave_prior(srmap_problem* p, hipStream_t st);
  int form_held_prior(srmap_problem* p, hipStream_t st);
  DevBuf eff_, user_, prior_, caller_;
  Holdout hold_;
  bool mad_recorded_ = false;
  int loss_ = SRMAP_DATA_LOSS_L2;
  double delta_ = 0.0;
  int scale_mode_ = SRMAP_HUBER_DELTA_FIXED;
  double tuning_ = 0.0, min_delta_ = 0.0;
};

}  // namespace srmap
