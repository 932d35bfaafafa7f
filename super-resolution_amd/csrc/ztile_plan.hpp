// ztile_plan.hpp -- the plan of the tile path (per problem, owned by the problem: srmap_problem::zplan), what only reads
// it (ztile_plan.hip), and the typed entry points of the kernel file (kernels_ztile.hip) that the sequence of a tile
// evaluation (eval.hip) calls.  The arithmetic of the tables: ztile_tables.hpp.
#pragma once
#include "srmap_internal.hpp"
#include "ztile_tables.hpp"

namespace srmap {

struct ZPlan {
  int regk = 0, regr = 0, reg_index = -1;  // the regulariser fused into the tiles: 0 none, 1 TV, 2 BTV of range regr; -1: none
  bool subpix = false;  // sub-pixel shifts: residuals from k_forward_direct, z by 4-tap tables, exact ring by k_gather_direct
  int Dr = 0;           //   ring width
  DevBuf d_ringbuf;            //   [C][ring pixels] data gradient of the ring pixels (the ring pass ahead of the tile kernel)
  ZSourceTable st;             //   source-major tap table (its spn / spmax travel in the kernel arguments) ...
  DevBuf d_spsrc;              //   ... and its srctab on the device: ZSrc [S][spmax] (z_row_sp2)
  SpForwardPlan spf;    //   forward tile kernel (kernels_spfwd.hip); the direct forward kernel when it does not apply
  int E = 0;   // max |shift|
  ZFrameTables ft;             // integer shifts: the frame table (MS, cnt0 / off0 / aux0 are handed to the kernel by value) ...
  DevBuf d_hdr;                // ... and its vectors on the device: ZHdr, flat table of the border blocks
  DevBuf d_ent;                // ZEntry
  DevBuf d_cnt;                // tile kernel: int [S][8]
  DevBuf d_off;                //              long long [MS][S][S]
  DevBuf d_aux;                //              ZEntry [MS][S][S]
  int n_ring = 0;              // pixels of the border frame (0 when no shift produces border work)
  RingRects ring = {{0, 0, 0, 0, 0, 0}};
  DevBuf d_corr;               // [C][n_ring] border corrections of the gradient
  DevBuf d_bd;                 // BorderArgs<T> (device)
  DevBuf d_mpart;              // double: write-through partial granules of the in-kernel cost reduction, [2][mpart_cap] (cost, g.d); sentinel = unpublished
  size_t mpart_cap = 0;
};

// Up to this many cost partials (tiles + border blocks of all channels) one workgroup reduces them -- the tile kernel's
// last one, or k_finish_eval's block 0 -- and the solver gets g.d out of the same launch; beyond it the caller reduces in
// two stages.  64 K covers configs[2] (RGB 4096^2: 24 576 tiles), which at 16 K paid two more launches per evaluation and
// a separate 400 MB dot-product pass per trial point of a solve.
constexpr size_t kMaxFusedPartials = 65536;

// Upper bound of the cost partials one tile launch over C channels produces (tiles + border blocks, which fill whole
// grid rows) -- ONE definition for the granule allocation, the launch and the solver's decisions.
size_t ztile_est_partials(const ZPlan* z, int w, int H, int C);
// an active regulariser other than the one fused into the plan's tiles: direct kernels run behind the tile launch
bool ztile_more_regs(const srmap_problem* p, const ZPlan& z);
// Whether the tile launch of an evaluation with `terms` over C channels is the g.d instance (k_eval_z<..., WD>): it must
// produce the WHOLE gradient (no further regulariser kernel behind it) and few enough partials for its in-kernel
// reduction.  The tile evaluation asks it for the launch, ztile_can_fold for the solver (a folded trial point exists only
// inside that instance): the two cannot drift apart.
bool ztile_gd_instance_ok(const srmap_problem* p, const ZPlan& z, int w, int H, int C, unsigned terms);

// ---- kernels_ztile.hip ----
// in-kernel finish of this launch; publish {cost, g.d} to the solver's host words; plain partials of an earlier launch to add
struct MFin { bool on, publish; const double* xpart; int n_xpart; };
// The tile launch of an evaluation (k_eval_z<T, S, B, regk, regr, dvec != nullptr, sub-pixel data>; under a row shard's
// overlap request its two halves around the halo exchange): zterms of terms, regulariser (regk, regr) with IRLS weights
// wts fused.  *nblocks: the partials it leaves at partials (and partials_gd)
template <typename T>
int launch_ztiles(srmap_problem* p, const EvalReq& req, const Geometry& geo, int obs_c0, unsigned zterms, int regk, int regr,
                  const T* x, T* g, const T* wts, const ZPlan& z, double* partials, int* nblocks, hipStream_t st,
                  const T* dvec, double* partials_gd, MFin mfin, bool ring_ahead);
// k_finish_eval: cost_out[kCostValue] <- the n partials in index order (and [kCostGd] <- those of partials_gd, published
// to pub_out with the tag when given); corr_g != nullptr: the border corrections of the plan subtracted from it
template <typename T>
int launch_zfinish(srmap_problem* p, const ZPlan& z, const Geometry& geo, T* corr_g, const double* partials, int n,
                   double* cost_out, const double* partials_gd, double* pub_out, double* tag_slot, double tag, hipStream_t st);

}  // namespace srmap
