// motion_model.hpp -- the motion M_k of A_k = D B M_k: what the kernels that sample it take (WarpTaps, MotionArgs) and
// the one owner of the problem's motion state.  The state changes in MotionModel::create (once, from
// srmap_problem_create) and MotionModel::install (motion_model.hip) and nowhere else.
//
// The CREATED part is fixed after srmap_problem_create: the shift table of the problem's descriptor (or none: the
// identity), its warp taps on host and device and the per-row y tables of the frames that need one.  The REPLACEMENT
// holds at most one alternative to it, whole:
//
//   kind() in force   set by                                  replacement holds                      created part
//   None / Table      srmap_problem_create, NULL to a setter  nothing                                sampled
//   Affine            srmap_problem_set_affine_motion         recs, d_recs                           kept, not read
//   Flow              srmap_problem_set_flow[_device]         d_flow, d_seeds                        kept, not read
//   Lattice           srmap_problem_set_flow_lattice[_device] d_lattice, d_seeds, step / lw / lh     kept, not read
//
// The three are alternatives: installing one frees every buffer of the one before, and NULL to ANY of the three setters
// installs the empty replacement, which restores the created motion bit for bit.  A setter makes every check,
// allocation, upload and the seed / check pass on a Replacement of its own first; a refusal or failure there leaves the
// problem exactly as it was.  install() then drains the evaluations in flight (model_drain), moves the replacement in and
// re-plans (model_replan): the tile planner answers "not covered" for every kind but None / Table.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "dev_mem.hpp"

struct srmap_ctx;
struct srmap_problem;

namespace srmap {

// Affine motion (srmap_problem_set_affine_motion): doubles per frame record -- [0..5] the inverse map
// [ia ib itx; ic id ity], [6..11] the forward map [a b tx; c d ty], [12..13] the candidate radii of the transpose gather
constexpr int kAffineRec = 16;
constexpr double kAffineMaxDeviation = 0.25;  // max(|a-1|+|b|, |c|+|d-1|): bounds the gather at 3 x 3 candidates
// Displacement-field motion (srmap_problem_set_flow, kernels_flow.hip): the transpose gathers the (2 r + 1)^2 candidates
// around a stored seed
constexpr int kFlowRadius = 2;

// One MotionModule warp (forward or transpose) of one frame, as cv::warpAffine
// evaluates it (motion_module.cpp:18-51): source pixel = destination + (ox, oy)
// plus up to four bilinear taps with 1/32-pixel quantised weights.
template <typename T>
struct WarpTaps {
  int ox, oy;
  int ntaps;  // 1 = integer shift (weights 1,0,0,0), 4 = bilinear
  int fx;     // x fraction index 0..31 (1/32 px) -- used with ytab
  T w[4];     // (0,0) (1,0) (0,1) (1,1) as (dx,dy) tap offsets
  // warpAffine evaluates the y coordinate of every row in floating point before quantising it to 1/32 px; for a dy
  // within rounding distance of a quantisation tie the fraction index differs from row to row.  Then ytab (device,
  // one int per destination row: source row << 5 | fraction index) replaces oy and the y half of w.
  const int* ytab;
};
static_assert(std::is_trivially_copyable_v<WarpTaps<float>> && std::is_trivially_copyable_v<WarpTaps<double>>,
              "a kernel argument: no owner inside");

// The forms of M_k in A_k = D B M_k: none (the identity), the translational tap table, an affine matrix per frame, a dense
// displacement field per frame, a displacement field on a control lattice per frame.  MotionArgs: what the kernels that
// sample M_k (MotionSampler, sample_dev.hpp) take for it, by value as ONE kernel argument; a kind reads its own members
// only.
enum MotionKind { kMotionNone = 0, kMotionTable = 1, kMotionAffine = 2, kMotionFlow = 3, kMotionLattice = 4 };
// The control lattice of a displacement field (srmap_problem_set_flow_lattice, kernels_flow.hip): lw x lh nodes
// per component, node (i, j) at HR pixel (i * step, j * step); nodes [K][2][lh][lw] doubles in both dtypes
constexpr int kLatticeMaxStep = 1024;
struct LatticeDesc {
  const double* nodes;
  int step, lw, lh;
};
static_assert(std::is_trivially_copyable_v<LatticeDesc>, "a kernel argument: no owner inside");
template <typename T>
struct MotionArgs {
  const WarpTaps<T>* warps;  // [K] forward taps (table); nullptr: the identity
  const double* recs;        // [K][kAffineRec] (affine)
  const T* flow;             // [K][2][H][W] (flow)
  const int* seeds;          // [K][H][W] packed seeds of the transpose gather (flow, lattice)
  LatticeDesc lat;           // (lattice)
};
static_assert(std::is_trivially_copyable_v<MotionArgs<float>> && std::is_trivially_copyable_v<MotionArgs<double>>,
              "a kernel argument: no owner inside");

class MotionModel {
 public:
  // kind == kMotionNone: the empty replacement.  Built by a setter in locals, validated there, then moved into install()
  struct Replacement {
    MotionKind kind = kMotionNone;
    std::vector<double> recs;      // affine: K x kAffineRec, the host mirror of d_recs
    DevBuf d_recs;                 // affine: double[K][kAffineRec]
    DevBuf d_flow;                 // flow: [K][2][H][W] dtype, the (ux, uy) planes per frame
    DevBuf d_lattice;              // lattice: double[K][2][lh][lw] in both dtypes
    DevBuf d_seeds;                // flow, lattice: int[K][H][W] packed seeds of the transpose gather, validated with the field
    int step = 0, lw = 0, lh = 0;  // lattice
  };

  MotionKind kind() const { return kind_; }  // stored by create() and install(), never derived
  bool is_created() const { return rep_.kind == kMotionNone; }  // no replacement: the identity or the table
  bool is_field() const { return kind_ == kMotionFlow || kind_ == kMotionLattice; }
  // the replacement in force in the words of the refusals, and the entry point that set it (nullptr: none is set)
  const char* name() const;
  const char* setter() const;
  const char* sharded_name() const;  // in the words of refuse_sharded (shard_eval.hip)
  // "this call has no leg for the motion in force": `status` with the caller's clause, a format over name() and
  // setter() in that order
  int refuse(srmap_ctx* ctx, int status, const char* clause) const;
  template <typename T>
  MotionArgs<T> args() const {
    return {d_fwd_.as<const WarpTaps<T>>(), rep_.d_recs.as<double>(), rep_.d_flow.as<const T>(), rep_.d_seeds.as<int>(),
            {rep_.d_lattice.as<double>(), rep_.step, rep_.lw, rep_.lh}};
  }
  // the created part, for the planners and the fits
  bool has_table() const { return !shifts_.empty(); }
  bool has_ytabs() const { return !d_ytabs_.empty(); }
  const std::vector<double>& shifts() const { return shifts_; }  // K x 2; empty without a table
  const std::vector<WarpTaps<double>>& fwd() const { return fwd_; }
  const std::vector<WarpTaps<double>>& bwd() const { return bwd_; }
  template <typename T>
  const WarpTaps<T>* bwd_dev() const { return d_bwd_.as<const WarpTaps<T>>(); }  // nullptr without a table
  const Replacement& replacement() const { return rep_; }

  // srmap_problem_create: the tap tables of the descriptor's shifts (nullptr: none) onto host and device
  int create(srmap_problem* p, const double* shifts_xy);
  int install(srmap_problem* p, Replacement&& r);

 private:
  MotionKind kind_ = kMotionNone;
  std::vector<double> shifts_;
  std::vector<WarpTaps<double>> fwd_, bwd_;  // host mirrors of the taps (double), for tile planning
  DevBuf d_fwd_, d_bwd_;                     // WarpTaps<T>[K]
  std::vector<DevBuf> d_ytabs_;              // the y tables of the frames whose warpAffine y table is not uniform
  Replacement rep_;
};

}  // namespace srmap
