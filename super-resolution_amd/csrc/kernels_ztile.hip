// kernels_ztile.hip -- the hot path: one MAP gradient iteration
// (ObjectiveFunction::ComputeAllTerms, objective_function.cpp:5-20) as ONE
// LDS-tiled launch (border blocks ride at the front of its grid; the cost
// partials are reduced by its last workgroup -- a finish launch follows only when
// in-image border corrections have to be subtracted), for the common geometry:
// integer motion shifts, HR = LR * S, S in {2,3,4}, blur size B in {1,3}, first
// regulariser 2-D TV or BTV with range <= 3.  Everything else is evaluated by
// kernels_data_direct.hip / kernels_reg_direct.hip.
//
// Formulation.  With integer shifts the warp M_k and the
// blur B are shift-invariant, so AWAY FROM THE IMAGE BORDER they commute and the
// data term (objective_data_term.cpp:15-116, image_model.cpp:86-101) collapses
// onto the HR grid:
//     r_k(i,j) = (B x)(p) - y_k(i,j),   p = (S i + oy_k, S j + ox_k)   ("z position")
//     z(p)     = sum over the frames k whose LR grid hits p of r_k
//     g_data   = 2 S^2 * B^T z,         cost_data = S^2 * sum r_k^2
// i.e. every residual is evaluated ONCE, by the thread that owns HR pixel p
// ("owner computes"), from a full-resolution blur of x at its own pixels; the
// K per-frame transposes become one blur of z.  Per HR pixel this is 9 + 9 FMAs
// and K/S^2 observation loads instead of K gathers.  The reference clips every
// stage to the H x W domain separately (SURVEY.md section 8a'); in owner-computes
// form the clips are:
//   (a) warp zero fill: x outside the image reads 0            -> zero-filled tile;
//   (b) blur zero padding on the WARPED image: blur taps whose warped coordinate
//       leaves the image are dropped.  With B <= S + 1 that is blur tap row 0 of LR
//       row 0 and tap column 0 of LR column 0 only              -> subtracted for those
//       residuals in tiles at the top / left image edge (EDGE code path);
//   (c) LR pixels exist only inside the LR image                -> validity mask (EDGE);
//   (d) the transpose warp clips its SOURCE: frame k contributes to output pixel q
//       only if q - o_k is inside the image.  That depends on (q, k), so it cannot
//       be folded into the frame-summed z: the tiles add every frame and the
//       border blocks collect the excluded contributions for the pixels within
//       E = max|shift| of the image edge (k_finish_eval subtracts them), and the
//       cost of the residuals whose z position lies outside the image (they have
//       no owner).
//
// Tile kernel k_eval_z: a workgroup of 8 waves owns 8 HR rows x 64*S columns;
// wave = HR row, lane = LR cell, a thread owns the S consecutive pixels of its
// cell.  x tile (+halo) in LDS in polyphase layout xs[row][col mod S][cell]
// (unit stride across lanes for every window read, offsets are immediates).
//   phase 1  B x at S+2 pixels (own + one neighbour each side), residuals of
//            the matching frames (host-built table per (row phase, col phase)),
//            horizontal half of B^T in registers -> zh to LDS; regulariser
//            pass 1 (values, self term, 2*lambda*w*r -> LDS); halo rows of zh /
//            2*lambda*w*r by whole waves (0-1 / 2-3), the left halo columns one per
//            wave (4 / 5, lanes = rows); their IRLS weights wait in LDS;
//   barrier  the cost terms are complete: the workgroup's cost partial is published here, at the barrier between the
//            phases (the g.d partial of the WD instances needs the finished gradient and follows the g store);
//   phase 2  vertical half of B^T from zh; regulariser pass 2; g store.
// The frame table's counts and round 0 travel by value in the kernel arguments
// (scalar loads only); later rounds are read through the constant address space.
// No MFMA: stencil path.  Cost partials are reduced in fixed order
// (deterministic).


#include <type_traits>

#include "ztile_dev.hpp"
#include "ztile_plan.hpp"

namespace srmap {

namespace {

template <typename T, int S, int B, int REGK, int R, bool WD, bool SP>
__global__ __launch_bounds__((ZCfg<T, S, B, REGK, R>::NT), (sizeof(T) == 4 || S == 2 ? 6 : 4)) void k_eval_z(
    ZArgs<T, B, ZCfg<T, S, B, REGK, R>::NP> A) {
  using C = ZCfg<T, S, B, REGK, R>;
  constexpr int HB = C::HB, NV = C::NV, RU = C::RU;
  // border blocks borrow the x tile's LDS for the frame table
  constexpr int kBorderLds = (int)((16 * sizeof(int2) + kBorderTabEntries * sizeof(ZEntry) + 16 * sizeof(double) + sizeof(T) - 1) / sizeof(T));
  __shared__ T xs[C::XS_ELEMS > kBorderLds ? C::XS_ELEMS : kBorderLds];
  __shared__ T zs[C::ZS_ELEMS > 0 ? C::ZS_ELEMS : 1];
  __shared__ T cs[C::CS_ELEMS > 0 ? C::CS_ELEMS : 1];
  __shared__ double red[2][C::NW];
  __shared__ T wcs[32];  // IRLS weights of the left-halo-column pixels (two columns x up to 16 rows)
  __shared__ T whs[(C::RU > 0 ? C::RU : 1) * S * C::CW];  // IRLS weights of the halo rows of 2*lambda*w*r

  // Every argument the head of a workgroup reads -- up to its first memory requests -- is requested HERE, in one batch
  // ahead of the first branch.  Left to the compiler each uniform early-out below (border block? selected tile row?
  // edge tile?) fetched its own word behind its own s_waitcnt: six dependent scalar-load round trips (~250 cycles
  // each) stood between the start of a workgroup and its first x request (profiles/r03_phase_clock.txt: "issue x
  // loads" 2.1 K cycles).  The empty asm makes all of them live at this point; later reads of the same fields reuse
  // the registers.
  {
    const T* a_x = A.x; const T* a_y = A.y; const T* a_w = A.w; T* a_g = A.g;
    const int a_W = A.W, a_H = A.H, a_wl = A.wl, a_hl = A.hl, a_nby = A.nby, a_E = A.E, a_terms = A.terms, a_obsC = A.obs_C;
    const int a_cr0 = A.cr0, a_cr1 = A.cr1, a_rr0 = A.rr0, a_rr1 = A.rr1, a_sm = A.sel_mode, a_s0 = A.sel0, a_s1 = A.sel1;
    const unsigned a_gx = gridDim.x, a_gy = gridDim.y;
    asm volatile("" ::"s"(a_x), "s"(a_y), "s"(a_w), "s"(a_g), "s"(a_W), "s"(a_H), "s"(a_wl), "s"(a_hl), "s"(a_nby), "s"(a_E),
                 "s"(a_terms), "s"(a_obsC), "s"(a_cr0), "s"(a_cr1), "s"(a_rr0), "s"(a_rr1), "s"(a_sm), "s"(a_s0), "s"(a_s1),
                 "s"(a_gx), "s"(a_gy));
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave = HR row of the tile (SGPR)
  // XCD-aware tile order: workgroups are dealt to the 8 XCDs round robin in launch order and every XCD has its
  // own L2; with the tile ROW on blockIdx.x and launch index n -> row band (n mod 8) the workgroups an XCD runs at
  // the same time are vertical neighbours and share their x halo rows in that L2.  Bijective for any row count.
  if ((int)blockIdx.y < A.nby) {  // border blocks come first in dispatch order (uniform branch)
    if (A.sel_mode == 1) return;
    const int bidx = blockIdx.y * gridDim.x + blockIdx.x;
    const BorderArgs<T>& Bd = *A.bd;
    if (bidx * C::NT < Bd.n_ring) {
      if (WD && A.fold_xk != nullptr) border_block<T, S, B, C::NT, WD, WD>(A, Bd, bidx, blockIdx.z, xs, A.nby * gridDim.x);
      else border_block<T, S, B, C::NT, WD, false>(A, Bd, bidx, blockIdx.z, xs, A.nby * gridDim.x);
    }
    else if (threadIdx.x == 0) {
      const int nbb = A.nby * gridDim.x;
      put_partial<WD>(A, (size_t)A.n_tile_partials + (size_t)blockIdx.z * nbb + bidx, 0.0, 0.0);
    }
    return;
  }
  const int by = blockIdx.y - A.nby, nby_t = gridDim.y - A.nby;
  int tby = by, tbx = blockIdx.x;
  {
    // ... with launch index 1 and the launch index of the BOTTOM tile row swapped: the bottom row (masked edge path in
    // every column, the slowest tiles) would otherwise be among the last workgroups of every tile column -- of the last
    // column too, where it sets the end of the launch.  It is dispatched second now, like the top row first.  The
    // bottom row is the last row of band 7: launch index 8 q - 1 (= the last index when the row count is a multiple
    // of 8; with a remainder the last index maps to another band's last row).
    const int q = gridDim.x >> 3, rem = gridDim.x & 7;
    const int n0 = blockIdx.x, nbot = (rem == 0) ? (int)gridDim.x - 1 : 8 * q - 1;
    const int n = (nbot > 1) ? (n0 == 1 ? nbot : (n0 == nbot ? 1 : n0)) : n0;
    const int bnd = n & 7;
    tby = bnd * q + (bnd < rem ? bnd : rem) + (n >> 3);
    // tile columns in the order first, last, second, ...: the masked edge columns (longest-lived tiles) are not the
    // launch's last generation
    tbx = (by == 0) ? 0 : (by == 1 ? nby_t - 1 : by - 1);
  }
  if (A.sel_mode != 0 && ((A.sel_mode == 1) != (tby >= A.sel0 && tby < A.sel1))) return;  // uniform; before any barrier
  const int R0 = tby * C::TH, CJ0 = tbx * C::CW, C0 = CJ0 * S;
  const int ch = blockIdx.z;
  const size_t N = (size_t)A.W * A.H;
  const size_t nl = (size_t)A.wl * A.hl;
  const bool fold = WD && A.fold_xk != nullptr;   // uniform: the window is xk + stp * d (solver line search)
  const T* xplane = (fold ? A.fold_xk : A.x) + (size_t)ch * N;
  const int gr = R0 + wv;          // global HR row of this thread
  const int gc0 = C0 + S * lane;   // first global HR column of this thread
  const int cellg = CJ0 + lane;
  const bool want_data = (A.terms & SRMAP_TERM_DATA) != 0;
  // frame shards evaluate the regulariser of their own row band only (whole tiles: the band is tile aligned)
  const bool want_reg = REGK != 0 && (A.terms & SRMAP_TERM_REG) != 0 && R0 >= A.rr0 && R0 < A.rr1;
  const T* ybase = A.y + (size_t)ch * nl;
  // ---------------- global loads whose addresses are known now: x tile, observations, IRLS weights ----------------
  constexpr int ARI = (C::XR + C::NW - 1) / C::NW;  // x rows per wave
  constexpr int EXTRA = C::XC - C::CW;              // halo cells, staged by the first lanes
  // XT: the EXTRA halo cells of ALL rows are requested by the last wave in its (otherwise idle) last round -- one lane per
  // (row, cell) -- instead of by the first EXTRA lanes of every wave in every round (half of a wave's x requests
  // served two lanes each)
  constexpr bool XT = ARI >= 2 && (C::NW - 1) + (ARI - 1) * C::NW >= C::XR && C::XR * EXTRA <= 64;
  T va[ARI][S], vb[ARI][S], ma[ARI], mb[ARI];
  T vda[WD ? ARI : 1][S], vdb[WD ? ARI : 1][S];   // WD: the direction at the window's elements (fold)
  bool owna[ARI] = {}, ownb[ARI] = {};
  size_t xoa[ARI] = {}, xob[ARI] = {};
#pragma unroll
  for (int it = 0; it < ARI; ++it) {
    const bool xt_slot = XT && it == ARI - 1 && wv == C::NW - 1;  // uniform
    const int row = xt_slot ? lane / EXTRA : wv + it * C::NW;
    const int grr = R0 - C::HU + row;
    const bool row_in = row < C::XR && (unsigned)grr < (unsigned)A.H;  // uniform (XT slot: per lane)
    const int gca = xt_slot ? CJ0 - C::XCL + C::CW + lane % EXTRA : CJ0 - C::XCL + lane, gcb = gca + C::CW;
    const bool ina = row_in && (unsigned)gca < (unsigned)A.wl;
    const bool inb = !XT && row_in && lane < EXTRA && (unsigned)gcb < (unsigned)A.wl;
    const T* sa = xplane + (ina ? (size_t)grr * A.W + (size_t)gca * S : (size_t)0);
    const T* sb = xplane + (inb ? (size_t)grr * A.W + (size_t)gcb * S : (size_t)0);
#pragma unroll
    for (int pc = 0; pc < S; ++pc) va[it][pc] = sa[pc];
    if (!XT) {
#pragma unroll
      for (int pc = 0; pc < S; ++pc) vb[it][pc] = sb[pc];
    }
    if (WD) {  // the direction at the same elements (requested with the window; combined when the window goes to LDS)
#pragma unroll
      for (int pc = 0; pc < S; ++pc) { vda[it][pc] = T(0); vdb[it][pc] = T(0); }
      if (fold) {
        const T* dpl = A.dvec + (size_t)ch * N;
        const T* da = dpl + (sa - xplane);
        const T* db = dpl + (sb - xplane);
#pragma unroll
        for (int pc = 0; pc < S; ++pc) vda[it][pc] = da[pc];
        if (!XT) {
#pragma unroll
          for (int pc = 0; pc < S; ++pc) vdb[it][pc] = db[pc];
        }
        // where the window element is one of the tile's OWN pixels (not a halo element, inside the image) the trial point
        // is also written out: the solver's x holds it after the evaluation, as after k_axpy_out
        const int orow = row - C::HU;
        owna[it] = ina && orow >= 0 && orow < C::TH && gca >= CJ0 && gca < CJ0 + C::CW;
        ownb[it] = inb && orow >= 0 && orow < C::TH && gcb >= CJ0 && gcb < CJ0 + C::CW;
        xoa[it] = (size_t)grr * A.W + (size_t)gca * S;
        xob[it] = (size_t)grr * A.W + (size_t)gcb * S;
      }
    }
    // scale 2^Q inside the image, 0 outside: applied as ONE multiply when the tile goes to LDS -- a select on the
    // loaded value makes the compiler wait for this row group before it requests the next one
    ma[it] = ina ? Pre<T>::up(T(1)) : T(0);
    mb[it] = inb ? Pre<T>::up(T(1)) : T(0);
  }
  T ypre[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) ypre[v] = T(0);
  // tiles whose residuals can touch LR row / column 0 or leave the LR image take the masked path (uniform);
  // so do row-band problems (cost rows restricted)
  const int rm = A.E + HB + 1, cm = (A.E + HB + S) / S + 1;
  const bool edge = (R0 - rm < 0) || (R0 + C::TH + rm > A.H) || (CJ0 - cm < 0) || (CJ0 + C::CW + cm > A.wl) ||
                    A.cr0 > 0 || A.cr1 < A.H;  // partial tiles (bottom / right) are edge tiles by the first two tests
  const int hrowz = wv == 0 ? -HB : C::TH - 1 + HB;  // halo rows of zh: tile rows -1 (wave 0) and TH (wave 1)
  const bool has_z_halo = want_data && B > 1 && A.g != nullptr && wv < 2;
  T ypre2[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) ypre2[v] = T(0);
  if (!SP && want_data) z_row_prefetch<T, S, B, C>(A, wv, R0, CJ0, lane, edge, ybase, ypre);
  if (!SP && has_z_halo) z_row_prefetch<T, S, B, C>(A, hrowz, R0, CJ0, lane, edge, ybase, ypre2);
  const T* wplane = (want_reg && A.w) ? A.w + (size_t)ch * N : nullptr;
  T wreg[S];
#pragma unroll
  for (int pc = 0; pc < S; ++pc) wreg[pc] = T(1);
  if (wplane != nullptr && gr < A.H && gc0 < A.W) {
#pragma unroll
    for (int pc = 0; pc < S; ++pc) wreg[pc] = wplane[(size_t)gr * A.W + gc0 + pc];
  }
  // halo row of 2*lambda*w*r this wave evaluates (waves 2 .. 2+RU-1: tile rows -1 .. -RU) and its weights
  const bool reg_halo_on = want_reg && A.g != nullptr && RU > 0;
  const int hrow = -(wv - 1);  // wave 2 -> -1, wave 3 -> -2
  const bool has_reg_halo = reg_halo_on && wv >= 2 && wv < 2 + RU;
  T whalo[S];
#pragma unroll
  for (int pc = 0; pc < S; ++pc) whalo[pc] = T(1);
  if (has_reg_halo && wplane != nullptr && R0 + hrow >= 0 && gc0 < A.W) {
#pragma unroll
    for (int pc = 0; pc < S; ++pc) whalo[pc] = wplane[(size_t)(R0 + hrow) * A.W + gc0 + pc];
  }

  // weight of the left-halo-column pixel this lane evaluates in phase 1 (waves 4 / 5, one row per lane): requested
  // with the tile's other inputs and parked in LDS with the x tile -- a load inside the task stalled these two waves,
  // and with them the workgroup's second barrier, for a memory round trip
  T wcolv = T(1);
  const bool col_task = reg_halo_on && (wv == 4 || wv == 5) && lane < C::TH + RU;
  if (col_task && wplane != nullptr) {
    const int hgr = R0 + lane - RU, hgc = C0 - (wv == 4 ? 1 : 2);
    if (hgr >= 0 && hgr < A.H && hgc >= 0) wcolv = wplane[(size_t)hgr * A.W + hgc];
  }

  // WD: how elements of the direction are read (as given, or normalised on the fly from the unnormalised direction)
  const DirScale dsc = dir_scale(WD ? A.fold_norms : nullptr);
  if (WD && fold) {  // trial point: x = xk + stp * d, element by element the expression of solver_passes.hip's k_axpy_out
    T* xout = A.fold_x + (size_t)ch * N;
#pragma unroll
    for (int it = 0; it < ARI; ++it) {
#pragma unroll
      for (int pc = 0; pc < S; ++pc) va[it][pc] = va[it][pc] + A.fold_stp * dir_elem<T>(vda[it][pc], dsc);
      if (owna[it]) {
#pragma unroll
        for (int pc = 0; pc < S; ++pc) xout[xoa[it] + pc] = va[it][pc];
      }
      if (!XT) {
#pragma unroll
        for (int pc = 0; pc < S; ++pc) vb[it][pc] = vb[it][pc] + A.fold_stp * dir_elem<T>(vdb[it][pc], dsc);
        if (ownb[it]) {
#pragma unroll
          for (int pc = 0; pc < S; ++pc) xout[xob[it] + pc] = vb[it][pc];
        }
      }
    }
  }
  // ---------------- x tile -> LDS, polyphase ----------------
#pragma unroll
  for (int it = 0; it < ARI; ++it) {
    const bool xt_slot = XT && it == ARI - 1 && wv == C::NW - 1;  // uniform
    if (xt_slot) {
      const int xrow = lane / EXTRA;
      if (xrow < C::XR) {
#pragma unroll
        for (int pc = 0; pc < S; ++pc) xs[xrow * C::XROW + pc * C::XC + C::CW + lane % EXTRA] = va[it][pc] * ma[it];
      }
      continue;
    }
    const int row = wv + it * C::NW;
    if (row < C::XR) {  // uniform
#pragma unroll
      for (int pc = 0; pc < S; ++pc) xs[row * C::XROW + pc * C::XC + lane] = va[it][pc] * ma[it];
      if (!XT && lane < EXTRA) {
#pragma unroll
        for (int pc = 0; pc < S; ++pc) xs[row * C::XROW + pc * C::XC + C::CW + lane] = vb[it][pc] * mb[it];
      }
    }
  }
  if (col_task) wcs[(wv - 4) * 16 + lane] = wcolv;
  if (has_reg_halo) {  // the halo row's weights wait in LDS too (eight registers less across the data term)
#pragma unroll
    for (int pc = 0; pc < S; ++pc) whs[((wv - 2) * S + pc) * C::CW + lane] = whalo[pc];
  }
  __syncthreads();

  // in-image mask of this thread's pixels (partial tiles at the right / bottom edge)
  T mk[S];
#pragma unroll
  for (int pc = 0; pc < S; ++pc) mk[pc] = (gr < A.H && gc0 + pc < A.W) ? T(1) : T(0);

  T acc[S], zown[S];
#pragma unroll
  for (int j = 0; j < S; ++j) { acc[j] = T(0); zown[j] = T(0); }
  double cost_data = 0.0, cost_reg = 0.0;

  // ---------------- phase 1: data term ----------------
  // kept as an always-inline lambda called once: written as a plain block the compiler schedules every instance differently
  auto phase1_data = [&]() __attribute__((always_inline)) {
  if (SP && want_data) {
    T dummy[S];
    // table rows reach (Dr + S) / S LR rows around the tile's own: only the top / bottom tile rows can leave the image
    const bool row_edge = (R0 - A.Dr - 2 * S < 0) || (R0 + C::TH + A.Dr + 2 * S > A.H);
    // table columns reach Dr / S + 1 LR cells around a pixel's own (+ 1 for the neighbour pixels of the cell)
    const int mj = A.Dr / S + 3;
    const bool col_inner = (CJ0 - mj >= 0) && (CJ0 + C::CW + mj <= A.wl);
    if (row_edge) {
      z_row_sp2<T, S, B, C, true, true>(A, zs, wv, R0, CJ0, lane, ch, zown);
      if (has_z_halo) z_row_sp2<T, S, B, C, true, true>(A, zs, hrowz, R0, CJ0, lane, ch, dummy);
    } else if (!col_inner) {
      z_row_sp2<T, S, B, C, false, true>(A, zs, wv, R0, CJ0, lane, ch, zown);
      if (has_z_halo) z_row_sp2<T, S, B, C, false, true>(A, zs, hrowz, R0, CJ0, lane, ch, dummy);
    } else {
      z_row_sp2<T, S, B, C, false, false>(A, zs, wv, R0, CJ0, lane, ch, zown);
      if (has_z_halo) z_row_sp2<T, S, B, C, false, false>(A, zs, hrowz, R0, CJ0, lane, ch, dummy);
    }
  }
  if (!SP && want_data) {
    T dummy[S];
    double dcost = 0.0;
    if (edge) {
      z_row<T, S, B, C, true>(A, xs, zs, wv, R0, CJ0, lane, ybase, true, ypre, true, mk, zown, cost_data);
      if (has_z_halo) z_row<T, S, B, C, true>(A, xs, zs, hrowz, R0, CJ0, lane, ybase, true, ypre2, false, mk, dummy, dcost);
    } else {
      z_row<T, S, B, C, false>(A, xs, zs, wv, R0, CJ0, lane, ybase, true, ypre, true, mk, zown, cost_data);
      if (has_z_halo) z_row<T, S, B, C, false>(A, xs, zs, hrowz, R0, CJ0, lane, ybase, true, ypre2, false, mk, dummy, dcost);
    }
  }
  };
  phase1_data();
  // ---------------- phase 1: regulariser ----------------
  if (want_reg) {
    const bool reg_border = (R0 + C::TH + C::WIN > A.H) || (C0 + C::TW + C::WIN > A.W);
    const bool cost_row = gr >= A.cr0 && gr < A.cr1;
    if (reg_border)
      reg_row<T, S, REGK, R, C, true, true>(acc, cost_reg, xs, cs, wreg, wv, lane, gr, gc0, A.W, A.H, A.lambda, A.powtab, A.pwsum, cost_row);
    else
      reg_row<T, S, REGK, R, C, false, true>(acc, cost_reg, xs, cs, wreg, wv, lane, gr, gc0, A.W, A.H, A.lambda, A.powtab, A.pwsum, cost_row);
    if (has_reg_halo) {
      T dacc[S];
      double dc = 0.0;
      T whl[S];
#pragma unroll
      for (int pc = 0; pc < S; ++pc) whl[pc] = whs[((wv - 2) * S + pc) * C::CW + lane];
      // right-edge masks follow the tile's; the rows above a tile reach below the image only when the tile keeps
      // fewer than WIN rows of it (a partial bottom tile: found by tests/test_gpu_fuzz.py, H - R0 = 2 with BTV(3))
      if (C0 + C::TW + C::WIN > A.W || R0 + C::WIN > A.H)
        reg_row<T, S, REGK, R, C, true, false>(dacc, dc, xs, cs, whl, hrow, lane, R0 + hrow, gc0, A.W, A.H, A.lambda, A.powtab, A.pwsum, false);
      else
        reg_row<T, S, REGK, R, C, false, false>(dacc, dc, xs, cs, whl, hrow, lane, R0 + hrow, gc0, A.W, A.H, A.lambda, A.powtab, A.pwsum, false);
    }
    // left halo columns -1 .. -RU, one row per lane, one column per wave (a few-lane task with a
    // long dependent chain -- both columns on one wave made the whole workgroup wait for it at the barrier)
    if (col_task) {  // waves 4 / 5: their SIMDs carry the z halo rows only
      const T wcol = wcs[(wv - 4) * 16 + lane];
      const int rowrel = lane - RU;
      const int lo = rowrel * C::XROW, lc = rowrel * C::CROW;  // per-lane row offsets
      if (reg_border) {
        if (RU >= 1 && wv == 4) reg_halo_col<T, S, REGK, R, C, -1, true>(xs + lo, cs + lc, wcol, rowrel, R0, C0, A.W, A.H, A.lambda, A.powtab);
        if (RU >= 2 && wv == 5) reg_halo_col<T, S, REGK, R, C, -2, true>(xs + lo, cs + lc, wcol, rowrel, R0, C0, A.W, A.H, A.lambda, A.powtab);
      } else {
        if (RU >= 1 && wv == 4) reg_halo_col<T, S, REGK, R, C, -1, false>(xs + lo, cs + lc, wcol, rowrel, R0, C0, A.W, A.H, A.lambda, A.powtab);
        if (RU >= 2 && wv == 5) reg_halo_col<T, S, REGK, R, C, -2, false>(xs + lo, cs + lc, wcol, rowrel, R0, C0, A.W, A.H, A.lambda, A.powtab);
      }
    }
  }
  // ---------------- cost partial of this workgroup ----------------
  // The cost terms are complete here (phase 2 adds to the gradient only), so the partial leaves at the barrier the
  // workgroup holds anyway: behind the g stores it cost a wave sum, a third barrier -- at which the waves that finish
  // phase 2 early waited for the others -- and the publishing store's round trip at the very end of the workgroup's life.
  // Same wave sum, same order of the eight additions as before: the cost is unchanged bit for bit.
  {
    const double cw = wave_sum_d((double)(S * S) * cost_data + cost_reg);
    if (lane == 0) red[0][wv] = cw;
  }
  __syncthreads();
  const size_t pidx = ((size_t)blockIdx.z * nby_t + by) * gridDim.x + blockIdx.x;  // this workgroup's partial
  if (!WD && tid == 0) {
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < C::NW; ++i) c += red[0][i];
    put_partial<false>(A, pidx, c, 0.0);
  }

  // ---------------- phase 2 ----------------
  T dreg[S];  // WD: the search direction at this thread's pixels (g.d is produced with g)
#pragma unroll
  for (int pc = 0; pc < S; ++pc) dreg[pc] = T(0);
  if (WD && gr < A.H && gc0 < A.W && gr >= A.cr0 && gr < A.cr1) {
    const T* dp = A.dvec + (size_t)ch * N + (size_t)gr * A.W + gc0;
#pragma unroll
    for (int pc = 0; pc < S; ++pc) dreg[pc] = dir_elem<T>(dp[pc], dsc);
  }
  if (want_data && A.g != nullptr) {
    const T sc = (T)(2 * S * S);  // g += 2 * (s*s block sum) (objective_data_term.cpp:55-71)
#pragma unroll
    for (int pc = 0; pc < S; ++pc) {
      T zz;
      if (B == 1) {
        zz = zown[pc];
      } else {
        zz = T(0);
#pragma unroll
        for (int a = 0; a < B; ++a) zz += k1_tap<B>(A, a) * zs[(wv + a) * C::ZROW + pc * C::CW + lane];  // rows wv-HB+a
      }
      if (SP)  // the ring pass owns the pixels within Dr of the image edge
        zz = ((unsigned)(gr - A.Dr) < (unsigned)(A.H - 2 * A.Dr) && (unsigned)(gc0 + pc - A.Dr) < (unsigned)(A.W - 2 * A.Dr)) ? zz : T(0);
      acc[pc] += sc * zz;
    }
  }
  if (want_reg && A.g != nullptr) reg_pass2z<T, S, REGK, R, C>(acc, xs, cs, wv, lane, A.powtab);

  if (SP && want_data && A.g != nullptr && A.ringbuf != nullptr) {
    // the ring pass ran AHEAD of this launch (k_gather_ring into the plan's buffer): its exact data gradient of the pixels
    // within Dr of the image edge is added LAST, as the pass added it to the stored g when it ran behind the launch
    // (uniform test first: only edge tiles hold such pixels)
    const int Dr = A.Dr;
    if (R0 < Dr || R0 + C::TH > A.H - Dr || C0 < Dr || C0 + C::TW > A.W - Dr) {
      const int band = Dr * A.W, mid = A.H - 2 * Dr;
      const T* rb = A.ringbuf + (size_t)ch * (size_t)(2 * band + 2 * Dr * mid);
#pragma unroll
      for (int pc = 0; pc < S; ++pc) {
        const int gc = gc0 + pc;
        if (gr < A.H && gc < A.W) {
          int t = -1;
          if (gr < Dr) t = gr * A.W + gc;
          else if (gr >= A.H - Dr) t = band + (gr - (A.H - Dr)) * A.W + gc;
          else if (gc < Dr) t = 2 * band + (gr - Dr) * 2 * Dr + gc;
          else if (gc >= A.W - Dr) t = 2 * band + (gr - Dr) * 2 * Dr + Dr + (gc - (A.W - Dr));
          if (t >= 0) acc[pc] += rb[t];
        }
      }
    }
  }
  if (A.g != nullptr && gr < A.H && gc0 < A.W) {
    T* dst = A.g + (size_t)ch * N + (size_t)gr * A.W + gc0;
#pragma unroll
    for (int pc = 0; pc < S; ++pc) __builtin_nontemporal_store(acc[pc], &dst[pc]);  // written once, not re-read here
  }

  // ---------------- g.d partial (WD instances: needs the finished gradient) ----------------
  if (WD) {
    double gd = 0.0;
#pragma unroll
    for (int pc = 0; pc < S; ++pc) gd += (double)acc[pc] * (double)dreg[pc];
    gd = wave_sum_d(gd);
    if (lane == 0) red[1][wv] = gd;
    __syncthreads();
    if (tid == 0) {
      double c = 0.0, d = 0.0;
#pragma unroll
      for (int i = 0; i < C::NW; ++i) { c += red[0][i]; d += red[1][i]; }
      put_partial<true>(A, pidx, c, d);
    }
  }
  // in-kernel finish: the last workgroup of the grid gathers the granules of the evaluation (after its own g stores)
  if (A.mfinish && blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1 && blockIdx.z == gridDim.z - 1) {
    __syncthreads();
    finish_block<WD, C::NT>(A, &red[0][0]);
  }
}

// After the tile kernel: subtract the border corrections from g and reduce every cost partial of the evaluation
// in index order (deterministic).  Block 0 reduces; all blocks apply corrections.
template <typename T>
__global__ __launch_bounds__(256) void k_finish_eval(T* __restrict__ g, const T* __restrict__ corr, int n_ring, int W,
                                                     int H, RingRects ring, int C, const double* __restrict__ partials,
                                                     int n_partials, double* __restrict__ cost_out,
                                                     const double* __restrict__ partials_gd, double* pub,
                                                     double* tag_slot, double tag) {
  __shared__ double red[4], red2[4];
  double v = 0.0, v2 = 0.0;
  if (blockIdx.x == 0) {
    // eight requests in flight per thread (one load per iteration was one memory round trip per 256 partials);
    // the order of the additions is fixed
    constexpr int U = 8;
    for (int base = threadIdx.x; base < n_partials; base += 256 * U) {
      double a[U], b2[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * 256;
        a[u] = i < n_partials ? partials[i] : 0.0;
        b2[u] = (partials_gd != nullptr && i < n_partials) ? partials_gd[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) { v += a[u]; v2 += b2[u]; }
    }
  }
  // block 0 only reduces (its chain of dependent steps is the kernel's duration); the corrections start at block 1
  const int t = ((int)blockIdx.x - 1) * 256 + (int)threadIdx.x;
  if (g != nullptr && blockIdx.x > 0 && t < n_ring) {
    int qr, qc;
    ring_pixel(t, W, H, ring, qr, qc);
    if (qr >= 0 && qr < H && qc >= 0 && qc < W) {
      for (int ch = 0; ch < C; ++ch) {
        const T c = corr[(size_t)ch * n_ring + t];
        if (c != T(0)) g[((size_t)ch * H + qr) * W + qc] -= c;
      }
    }
  }
  if (blockIdx.x == 0) {
    v = wave_sum_d(v);
    if (partials_gd != nullptr) v2 = wave_sum_d(v2);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid] = v; red2[wid] = v2; }
    __syncthreads();
    if (threadIdx.x == 0) cost_out[kCostValue] = (red[0] + red[1]) + (red[2] + red[3]);
    if (partials_gd != nullptr) {  // g.d of the same evaluation (solver line search)
      if (threadIdx.x == 0) {
        const double gd = (red2[0] + red2[1]) + (red2[2] + red2[3]);
        cost_out[kCostGd] = gd;
        if (pub != nullptr) {  // solver line search: {cost, g.d} straight to the host-mapped words, then the arrival tag
          pub[0] = cost_out[kCostValue];
          pub[1] = gd;
          __threadfence_system();
          *(volatile double*)tag_slot = tag;
        }
      }
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// host side: launch -- only what has to name a kernel instance (the plan: ztile_plan.hip; the sequence of a tile
// evaluation: eval.hip)

// Kernel arguments of the tile kernel (everything but the grid-dependent fields).
template <typename T, int S, int B, int REGK, int R>
static void fill_zargs(ZArgs<T, B, ZCfg<T, S, B, REGK, R>::NP>& A, srmap_problem* p, const Geometry& geo, int obs_c0,
                       unsigned terms, const T* x, T* g, const T* wts, const ZPlan& z, double* partials, const T* dvec,
                       double* partials_gd) {
  using C = ZCfg<T, S, B, REGK, R>;
  A.x = x; A.y = p->d_obs.as<const T>() + (size_t)obs_c0 * geo.w * geo.h; A.w = wts; A.g = g; A.partials = partials;
  A.dvec = dvec; A.partials_gd = partials_gd;
  A.cnt = z.d_cnt.as<int>(); A.off = z.d_off.as<long long>(); A.aux = z.d_aux.as<ZEntry>(); A.MS = z.ft.MS;
  A.spsrc = z.d_spsrc.as<ZSrc>(); A.spmax = z.st.spmax;
  for (int pr = 0; pr < 4; ++pr) A.spn[pr] = z.st.spn[pr];
  for (int pr = 0; pr < 4; ++pr) {
    for (int i = 0; i < 8; ++i) A.cntk[pr][i] = z.ft.cnt0[pr * 8 + i];
    for (int pc = 0; pc < 4; ++pc) { A.off0[pr][pc] = z.ft.off0[pr * 4 + pc]; A.aux0[pr][pc] = z.ft.aux0[pr * 4 + pc]; }
  }
  A.W = geo.W; A.H = geo.H; A.wl = geo.w; A.hl = geo.h;
  A.obs_C = p->geo.C;
  A.E = z.E;
  A.ring = z.ring;
  A.cr0 = geo.cr0; A.cr1 = geo.cr1;
  A.rr0 = geo.rr0; A.rr1 = geo.rr1;
  A.terms = (int)terms;
  if (B == 1) { A.blur3[0] = A.blur3[1] = A.blur3[2] = T(1); A.k1s[0] = A.k1s[1] = T(1); }
  else {
    const int hb = (B - 1) / 2;
    A.blur3[0] = (T)p->blur.taps()[0]; A.blur3[1] = (T)p->blur.taps()[hb]; A.blur3[2] = (T)p->blur.taps()[hb * B + hb];
    A.k1s[0] = (T)p->blur.factor()[0]; A.k1s[1] = (T)p->blur.factor()[hb];
  }
  A.lambda = T(0);
  for (int i = 0; i < C::NP; ++i) A.powtab[i] = T(1);
  if (REGK != 0) {
    const RegSpec& rs = p->reg[z.reg_index];
    A.lambda = (T)rs.lambda;
    if (REGK == 2) for (int i = 0; i < C::NP; ++i) A.powtab[i] = (T)rs.pow_table[i];
  }
  A.pwsum = T(0);
  if (REGK == 2)
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < R; ++j)
        if (i + j > 0) A.pwsum += A.powtab[i + j];
  A.fold_xk = nullptr; A.fold_x = nullptr; A.fold_stp = T(0); A.fold_norms = nullptr;
}

// The four (WD, SP) legs of a tile kernel instance I: f(kernel) for the leg (wd, sp), or for every leg.  Preloading and
// launching both go through here.
template <typename T, class I, class F>
static void with_legs(bool every, bool wd, bool sp, F&& f) {
  if (every || (!wd && !sp)) f(&k_eval_z<T, I::S, I::B, I::REGK, I::R, false, false>);
  if (every || (wd && !sp)) f(&k_eval_z<T, I::S, I::B, I::REGK, I::R, true, false>);
  if (every || (!wd && sp)) f(&k_eval_z<T, I::S, I::B, I::REGK, I::R, false, true>);
  if (every || (wd && sp)) f(&k_eval_z<T, I::S, I::B, I::REGK, I::R, true, true>);
}

template <typename T, class I>
static int launch_z(srmap_problem* p, const EvalReq& req, const Geometry& geo, int obs_c0, unsigned terms, const T* x, T* g,
                    const T* wts, const ZPlan& z, double* partials, int* nblocks, hipStream_t st, const T* dvec,
                    double* partials_gd, MFin mfin, bool ring_ahead) {
  constexpr int S = I::S, B = I::B, REGK = I::REGK, R = I::R;
  using C = ZCfg<T, S, B, REGK, R>;
  ZArgs<T, B, C::NP> A;
  fill_zargs<T, S, B, REGK, R>(A, p, geo, obs_c0, terms, x, g, wts, z, partials, dvec, partials_gd);
  if (dvec != nullptr && req.fold.xk != nullptr) {  // line search: the point is xk + stp * d; its own pixels go to x
    A.fold_norms = req.fold.norms;
    if (!(z.subpix && (terms & SRMAP_TERM_DATA))) {
      A.fold_xk = (const T*)req.fold.xk; A.fold_x = const_cast<T*>(x); A.fold_stp = (T)req.fold.stp;
    }  // sub-pixel plans: the forward kernel ahead of this launch formed the point and wrote x (the tile evaluation,
       // eval.hip); dvec is still the unnormalised direction here (fold_norms)
  }
  dim3 grid((geo.w + C::CW - 1) / C::CW, (geo.H + C::TH - 1) / C::TH, geo.C);
  { const unsigned t = grid.x; grid.x = grid.y; grid.y = t; }
  const int n_tile_partials = (int)(grid.x * grid.y * grid.z);
  // border blocks: whole rows of the grid in front of the tiles
  A.bd = z.d_bd.as<const BorderArgs<T>>();
  A.nby = 0; A.n_tile_partials = n_tile_partials;
  int nbb = 0;
  if ((terms & SRMAP_TERM_DATA) && z.n_ring > 0) {
    const int need = (z.n_ring + C::NT - 1) / C::NT;
    A.nby = (need + (int)grid.x - 1) / (int)grid.x;
    nbb = A.nby * (int)grid.x;
    grid.y += A.nby;
  }
  A.rbuf = nullptr; A.Dr = z.Dr; A.ringbuf = nullptr;

  A.mfinish = mfin.on ? 1 : 0;
  A.n_partials = n_tile_partials + nbb * (int)grid.z;
  A.mpart = z.d_mpart.as<double>();
  A.mpart_gd = z.d_mpart ? z.d_mpart.as<double>() + z.mpart_cap : nullptr;
  A.cost_out = p->d_cost.as<double>();
  A.pub = mfin.publish ? req.pub.out : nullptr;
  A.tag_slot = req.pub.tag_slot;
  A.tag = req.pub.tag;
  A.to_host = req.pub.timeout_host;
  A.xpart = mfin.xpart; A.n_xpart = mfin.n_xpart;
  if (mfin.on && (size_t)A.n_partials > z.mpart_cap) return set_error(p->ctx, SRMAP_EHIP, "granule capacity");
  A.sel_mode = 0; A.sel0 = 0; A.sel1 = 0;
  const bool sp = z.subpix && (terms & SRMAP_TERM_DATA);
  auto launch = [&]() {
    with_legs<T, I>(false, dvec != nullptr, sp,
                    [&](auto* kernel) { hipLaunchKernelGGL(kernel, grid, dim3(C::NT), 0, st, A); });
  };
  if (sp) {
    A.rbuf = p->d_resid.as<const T>();
    A.obs_C = geo.C;  // layout of the residual buffer written by the forward kernel for this evaluation
    A.ringbuf = ring_ahead ? z.d_ringbuf.as<const T>() : nullptr;
    launch();
  } else if (req.overlap.fn != nullptr) {
    // Row shard: a tile row [8 t, 8 t + 8) reads x rows within the halo width of itself, so the tile rows t with
    // 8 t >= 2 * top and 8 t + 8 <= H - 2 * bot touch no halo row.  They run first, the halo exchange is
    // posted on its own stream under them, and the boundary tile rows (and the border blocks) follow the event.
    const int th = C::TH;
    A.sel0 = (2 * req.overlap.top + th - 1) / th;
    A.sel1 = (geo.H - 2 * req.overlap.bot) / th;
    if (A.sel1 > A.sel0) { A.sel_mode = 1; launch(); }
    const int rch = req.overlap.fn(req.overlap.arg);
    if (rch) return rch;
    SRMAP_HIP(p->ctx, hipStreamWaitEvent(st, req.overlap.event, 0));
    if (A.sel1 > A.sel0) { A.sel_mode = 2; launch(); } else { A.sel_mode = 0; launch(); }
  } else {
    launch();
  }
  *nblocks = n_tile_partials + nbb * (int)grid.z;
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

// The tile kernel's instances: runtime (S, B, regulariser) -> f(ZInst<S, B, REGK, R>()).  Preloading and launching both
// go through here, so this is the one list of what is instantiated (REGK 0 = no fused regulariser, 1 = TV, 2 = BTV of
// range R).  Returns false when no instance covers the arguments.
template <int S_, int B_, int REGK_, int R_>
struct ZInst { static constexpr int S = S_, B = B_, REGK = REGK_, R = R_; };

template <int S, int B, class F>
static bool with_reg_instance(int regk, int regr, F& f) {
  if (regk == 0) f(ZInst<S, B, 0, 0>());
  else if (regk == 1) f(ZInst<S, B, 1, 0>());
  else if (regk == 2 && regr == 1) f(ZInst<S, B, 2, 1>());
  else if (regk == 2 && regr == 2) f(ZInst<S, B, 2, 2>());
  else if (regk == 2 && regr == 3) f(ZInst<S, B, 2, 3>());
  else return false;
  return true;
}

template <typename T, class F>
static bool with_instance(int S, int B, int regk, int regr, F&& f) {
#ifdef SRMAP_ZT_ONLY_CFG2
  // measurement builds (tools/exp_build.sh): the one instance k_eval_z<SRMAP_ZT_ONLY_T, 4, SRMAP_ZT_ONLY_B, BTV, 3>
  // (seconds instead of minutes per variant); SRMAP_ZT_ONLY_T defaults to double, SRMAP_ZT_ONLY_B to 3 (1: cfg3 / cfg5)
#ifndef SRMAP_ZT_ONLY_T
#define SRMAP_ZT_ONLY_T double
#endif
#ifndef SRMAP_ZT_ONLY_B
#define SRMAP_ZT_ONLY_B 3
#endif
  if constexpr (std::is_same<T, SRMAP_ZT_ONLY_T>::value) {
    if (S == 4 && B == SRMAP_ZT_ONLY_B && regk == 2 && regr == 3) { f(ZInst<4, SRMAP_ZT_ONLY_B, 2, 3>()); return true; }
  }
  return false;
#else
  bool hit = false;
  auto regs = [&](auto s, auto b) { hit = with_reg_instance<decltype(s)::value, decltype(b)::value>(regk, regr, f); };
  return dispatch_scale_blur(S, B, regs) && hit;
#endif
}

// HIP loads a kernel's code object lazily at its first launch (milliseconds): touch the instances when the plan is
// made, not inside the first evaluation of a solve -- the plan's regulariser instance and the one without (evaluations
// that leave the regulariser out).
template <typename T>
static void preload_instances(int S, int B, int regk, int regr) {
  hipFuncAttributes attr;
  auto get = [&](auto* kernel) { (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)); };
  auto touch = [&](auto inst) { with_legs<T, decltype(inst)>(true, false, false, get); };
  (void)with_instance<T>(S, B, 0, 0, touch);
  (void)with_instance<T>(S, B, regk, regr, touch);
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&k_finish_eval<T>));
}
void ztile_preload(const srmap_problem* p) {
  const ZPlan* z = p->zplan.get();
  if (!z) return;
  dispatch_dtype(p->dtype, [&](auto t) { preload_instances<decltype(t)>(p->geo.s, p->geo.b, z->regk, z->regr); });
}

template <typename T>
int launch_ztiles(srmap_problem* p, const EvalReq& req, const Geometry& geo, int obs_c0, unsigned zterms, int regk, int regr,
                  const T* x, T* g, const T* wts, const ZPlan& z, double* partials, int* nblocks, hipStream_t st,
                  const T* dvec, double* partials_gd, MFin mfin, bool ring_ahead) {
  int rc = SRMAP_OK;
  const bool have = with_instance<T>(geo.s, geo.b, regk, regr, [&](auto inst) {
    rc = launch_z<T, decltype(inst)>(p, req, geo, obs_c0, zterms, x, g, wts, z, partials, nblocks, st, dvec, partials_gd, mfin, ring_ahead);
  });
  if (!have) return set_error(p->ctx, SRMAP_EUNSUPPORTED, "no tile kernel for scale %d blur %d regulariser %d/%d", geo.s, geo.b, regk, regr);
  return rc;
}

template <typename T>
int launch_zfinish(srmap_problem* p, const ZPlan& z, const Geometry& geo, T* corr_g, const double* partials, int n,
                   double* cost_out, const double* partials_gd, double* pub_out, double* tag_slot, double tag, hipStream_t st) {
  const unsigned blocks = 1u + (unsigned)(((corr_g != nullptr ? z.n_ring : 0) + 255) / 256);
  hipLaunchKernelGGL(k_finish_eval<T>, dim3(blocks), dim3(256), 0, st, corr_g, z.d_corr.as<const T>(), z.n_ring, geo.W, geo.H,
                     z.ring, geo.C, partials, n, cost_out, partials_gd, pub_out, tag_slot, tag);
  SRMAP_HIP(p->ctx, hipGetLastError());
  return SRMAP_OK;
}

#define SRMAP_ZTILE_ENTRY_POINTS(T)                                                                                          \
  template int launch_ztiles<T>(srmap_problem*, const EvalReq&, const Geometry&, int, unsigned, int, int, const T*, T*,      \
                                const T*, const ZPlan&, double*, int*, hipStream_t, const T*, double*, MFin, bool);          \
  template int launch_zfinish<T>(srmap_problem*, const ZPlan&, const Geometry&, T*, const double*, int, double*,             \
                                 const double*, double*, double*, double, hipStream_t);
SRMAP_ZTILE_ENTRY_POINTS(float)
SRMAP_ZTILE_ENTRY_POINTS(double)
#undef SRMAP_ZTILE_ENTRY_POINTS

}  // namespace srmap
