// ztile_plan.hip -- the plan of the tile path: whether k_eval_z (kernels_ztile.hip) covers the problem, its tables
// (arithmetic: ztile_tables.hpp) on the device, and every decision that only reads the plan.  No kernel here.
#include "ztile_plan.hpp"

#include "ztile_dev.hpp"  // BorderArgs: the device-resident constants of the border blocks

namespace srmap {

static_assert(sizeof(ZHdr) == sizeof(int2), "the border blocks read the flat table's headers as int2");

void ZPlanDelete::operator()(ZPlan* z) const { delete z; }  // and every table it owns

static bool arm_granules(ZPlan* z) {
  return hipMemsetD32((hipDeviceptr_t)z->d_mpart.as<double>(), (int)kSentinel32, 4 * z->mpart_cap) == hipSuccess;
}

void ztile_rearm(srmap_problem* p) {
  if (p->zplan && p->zplan->d_mpart) (void)arm_granules(p->zplan.get());
}

// granules of the in-kernel cost reduction (one per tile + one per border block), up to a cap beyond which the caller's
// two-stage reduction is used anyway
static bool alloc_granules(const srmap_problem* p, ZPlan* z) {
  const size_t cap = std::min<size_t>(ztile_est_partials(z, p->geo.w, p->geo.H, p->geo.C), kMaxFusedPartials);
  if (z->d_mpart.alloc(2 * cap * sizeof(double)) != hipSuccess) return false;
  z->mpart_cap = cap;
  return arm_granules(z);
}

// the one regulariser handled in-kernel: the first active one (order of accumulation), when it is TV or BTV of range <= 3
// in the reference's gradient mode (the tiles carry no exact BTV leg: such a regulariser goes through launch_regs_direct)
static void pick_fused_reg(const srmap_problem* p, ZPlan* z) {
  for (int r = 0; r < p->nreg && z->regk == 0; ++r) {
    const RegSpec& rs = p->reg[r];
    if (rs.lambda <= 0) continue;
    if (rs.kind == SRMAP_REG_TV) { z->regk = 1; z->reg_index = r; }
    else if (rs.kind == SRMAP_REG_BTV && rs.range >= 1 && rs.range <= 3 && !rs.exact()) { z->regk = 2; z->regr = rs.range; z->reg_index = r; }
    break;
  }
}

// Decide whether k_eval_z covers the problem; build the frame table.  The plan is installed in the problem only when it
// is complete; nothing it calls on the way (gather_ring_kernel_ok, spfwd_plan, the granules) reads p->zplan.  A failed
// allocation or copy of a table (upload_vector) leaves its text in the context's last error although the problem then
// runs the direct kernels and the call that planned succeeds: the text is read only after a failed call, which sets its own.
bool ztile_plan(srmap_problem* p) {
  p->zplan.reset();
  const Geometry& g = p->geo;
  const int S = g.s, B = g.b, K = g.K;
  const MotionModel& m = p->motion;
  if (!m.is_created()) return false;  // affine motion or a displacement field: the tiles' frame table holds translations only
  if (!p->blur.is_created()) return false;  // free-form kernel or bank: the tiles carry a symmetric 3 x 3 kernel's three values
  if (!p->maps_regular) return false;
  if (S < 2 || S > 4) return false;
  if (B != 1 && B != 3) return false;
  if (B == 3 && !ztile_blur3_symmetric(p->blur.taps().data(), p->blur.factor())) return false;
  std::vector<int> ox(K, 0), oy(K, 0);
  int amax = 0;
  // Data weights / a Huber loss: the plan takes the forward-residual form below whatever the shifts are.  The integer-shift
  // tiles recompute residuals inside the tile (z_row / border_residual, ztile_dev.hpp) and carry no weighted leg; the
  // forward-residual form gathers a residual BUFFER, which the weighted forward kernel fills with w .* r.  An integer
  // shift is its one-tap case: the source table and the forward kernel's stencils walk ntaps taps.  Without a
  // MotionModule there are no warp records for that form (ring kernel, forward tile kernel): the direct family runs.
  const bool robust = p->dw.robust();
  if (robust && !m.has_table()) return false;
  bool subpix = robust;
  if (m.has_table()) {
    for (int k = 0; k < K; ++k) {
      const WarpTaps<double>& f = m.fwd()[k];
      const WarpTaps<double>& b = m.bwd()[k];
      if (f.ytab != nullptr || b.ytab != nullptr) return false;  // rounding-tie shifts: per-row tables, direct kernels
      if (f.ntaps != 1 || b.ntaps != 1) subpix = true;
      else if (b.ox != -f.ox || b.oy != -f.oy) return false;
      ox[k] = f.ox; oy[k] = f.oy;
      amax = std::max(amax, std::max(std::abs(f.ox), std::abs(f.oy)));
      amax = std::max(amax, std::max(std::abs(b.ox), std::abs(b.oy)));
    }
  }
  if (amax > kMaxTileShift) return false;
  if ((long long)g.W * g.H >= (long long)INT_MAX) return false;  // the border blocks index a plane with 32 bits
  std::unique_ptr<ZPlan, ZPlanDelete> zp(new ZPlan());
  ZPlan* z = zp.get();
  z->E = amax;
  pick_fused_reg(p, z);
  if (subpix) {
    // ---- sub-pixel plan: z(p) = sum over (frame, bilinear tap of the TRANSPOSE warp) pairs that land on the LR grid ----
    z->subpix = true;
    z->E = 0;  // no border blocks: the forward kernel counts the cost, the ring pass evaluates the border exactly
    z->Dr = amax + 2 + g.hb;
    if (!ztile_frame_fits(g.W, g.H, z->Dr, S)) return false;
    z->st = ztile_source_table(S, K, m.bwd().data(), g.hb);
    // the only table an SP instance reads (z_row_sp2: spsrc, spn, spmax); the integer-shift frame table (cnt, off, aux) and
    // the border blocks' tables stay unset -- no border blocks with E = 0
    bool ok = upload_vector(p, z->st.srctab, &z->d_spsrc) == SRMAP_OK;
    if (ok && gather_ring_kernel_ok(p, g, K, z->Dr)) {
      // the ring pass runs ahead of the tile kernel into this buffer (g.d and the cost then finish inside the tile launch)
      const size_t nring = 2 * (size_t)z->Dr * g.W + 2 * (size_t)z->Dr * (g.H - 2 * z->Dr);
      ok = z->d_ringbuf.alloc(nring * g.C * p->elem()) == hipSuccess;
    }
    if (!(ok && alloc_granules(p, z))) return false;
    (void)spfwd_plan(p, &z->spf);
    p->zplan = std::move(zp);
    return true;
  }
  // the border frame (border blocks, width 2E) must stay a small part of the image
  if (!ztile_frame_fits(g.W, g.H, z->E, S)) return false;
  const ZFrameTables& t = z->ft;
  if (!z->ft.build(S, K, ox.data(), oy.data(), g.C, g.w, g.h)) return false;
  bool ok = upload_vector(p, t.hdr, &z->d_hdr) == SRMAP_OK && upload_vector(p, t.ent, &z->d_ent) == SRMAP_OK &&
            upload_vector(p, t.cnt, &z->d_cnt) == SRMAP_OK && upload_vector(p, t.off, &z->d_off) == SRMAP_OK &&
            upload_vector(p, t.aux, &z->d_aux) == SRMAP_OK;
  if (ok && z->E > 0) {
    // the rectangles of the border frame that can carry work
    z->ring = ztile_ring_rects(S, B, K, ox.data(), oy.data());
    z->n_ring = (int)ring_count(z->ring, g.W, g.H);
    if (z->n_ring > 0) ok = z->d_corr.alloc((size_t)g.C * z->n_ring * p->elem()) == hipSuccess;
  }
  if (ok) {
    ok = dispatch_dtype(p->dtype, [&](auto dt) {
      BorderArgs<decltype(dt)> bd{};
      bd.hdr = z->d_hdr.as<int2>(); bd.ent = z->d_ent.as<ZEntry>(); bd.blur_d = (decltype(bd.blur_d))p->blur.table(); bd.corr = (decltype(bd.corr))z->d_corr.as();
      bd.S = S; bd.b = B; bd.hb = g.hb; bd.n_ring = z->n_ring; bd.n_ent = (int)t.ent.size(); bd.obs_C = g.C;
      return upload_vector(p, std::vector<BorderArgs<decltype(dt)>>(1, bd), &z->d_bd) == SRMAP_OK;
    });
  }
  if (!(ok && alloc_granules(p, z))) return false;
  p->zplan = std::move(zp);  // installed complete or not at all
  return true;  // the caller preloads the kernel instance (ztile_preload)
}

// Row sharding: the integer-shift tiles can run their interior rows under the halo exchange (launch_z, sel_mode).
bool ztile_overlaps_halo(const srmap_problem* p) {
  const ZPlan* z = ztile_active(p);
  return z != nullptr && !z->subpix;
}

bool ztile_more_regs(const srmap_problem* p, const ZPlan& z) {
  for (int r = 0; r < p->nreg; ++r)
    if (r != z.reg_index && p->reg[r].lambda > 0.0) return true;
  return false;
}

// Frame sharding may split the regulariser by row band when the tile kernel alone produces it: one active
// regulariser, the one fused into the plan (no 3-D TV / second regulariser / wide BTV pass of the direct kernels).
bool ztile_reg_band_ok(const srmap_problem* p, unsigned terms) {
  const ZPlan* z = ztile_active(p);
  if (!z) return false;
  if (!(terms & SRMAP_TERM_REG)) return false;
  return z->regk != 0 && p->reg[z->reg_index].lambda > 0.0 && !ztile_more_regs(p, *z);
}

size_t ztile_est_partials(const ZPlan* z, int w, int H, int C) {
  const size_t tiles = (size_t)((w + 63) / 64) * ((H + 7) / 8) * C;
  const size_t ring = (z && z->n_ring > 0) ? (size_t)((z->n_ring + 511) / 512 + (H + 7) / 8) * C : (size_t)0;
  return tiles + ring;
}

bool ztile_gd_instance_ok(const srmap_problem* p, const ZPlan& z, int w, int H, int C, unsigned terms) {
  // sub-pixel plans: the ring pass must be able to run AHEAD of the tile launch (into z.d_ringbuf) -- a pass that adds to g
  // behind it would leave the launch's g.d without the ring's share
  if (z.subpix && !z.d_ringbuf) return false;
  if ((terms & SRMAP_TERM_REG) && ztile_more_regs(p, z)) return false;
  return ztile_est_partials(&z, w, H, C) <= kMaxFusedPartials;
}

bool ztile_can_fold(const srmap_problem* p, int C) {
  const ZPlan* z = ztile_active(p);
  if (!z) return false;
  // sub-pixel plans: the trial point is formed by the forward tile kernel, whose window has to hold a workgroup's own pixels
  if (z->subpix && !(z->spf.ok && z->spf.can_fold)) return false;
  return ztile_gd_instance_ok(p, *z, p->geo.w, p->geo.H, C, SRMAP_TERM_ALL);
}

}  // namespace srmap
