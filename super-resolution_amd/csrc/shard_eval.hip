// shard_eval.hip -- the evaluation sharded over one rank per GPU (comm.hpp): the halo refresh of
// x, the local evaluation each shard mode asks for, and the gradient / cost all-reduce of frame shards.  Host code only:
// the kernels are the evaluation's, the collectives the communicator's (comm.hip).
#include <cstring>
#include <vector>

#include "comm.hpp"

namespace srmap {

int shard_mode(const srmap_comm* c, const srmap_shard_desc* sd) {
  return (c && sd && comm_world(c) > 1) ? sd->mode : SRMAP_SHARD_NONE;
}

int refuse_sharded(srmap_problem* p, int mode, const char* what) {
  if (mode == SRMAP_SHARD_NONE) return SRMAP_OK;
  const bool solve = std::strcmp(what, "solve") == 0;
  const char* tail = solve ? "run the solve unsharded" : "evaluate unsharded";
  if (p->dw.holdout().threshold)
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "a hold-out is not sharded over a communicator%s: %s",
                     solve ? " (the held-out observations are a function of the whole problem's index)" : "", tail);
  if (p->dw.robust())
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "data weights / a Huber loss are not sharded over a communicator%s: %s",
                     solve ? " (the weights are not split with the frames or rows)" : "", tail);
  // a replaced motion, then a replaced blur, in the owners' words
  if (const char* model = p->motion.sharded_name() ? p->motion.sharded_name() : p->blur.sharded_name())
    return set_error(p->ctx, SRMAP_EUNSUPPORTED, "%s is not sharded over a communicator%s: %s", model,
                     solve ? " (only the direct family runs it)" : "", tail);
  // an exact BTV gradient reaches R halo rows where the shard description promises R - 1; exact 3-D TV goes with it
  for (int r = 0; r < p->nreg; ++r)
    if (p->reg[r].exact())
      return set_error(p->ctx, SRMAP_EUNSUPPORTED,
                       "an exact regulariser gradient (srmap_problem_set_regularizer_gradient, regulariser %d) is not sharded over a communicator: %s",
                       r, tail);
  return SRMAP_OK;
}

int shard_exchange_x(srmap_problem* p, srmap_comm* c, const srmap_shard_desc* sd, void* x_dev, hipStream_t st) {
  if (!c || !sd || comm_world(c) <= 1) return SRMAP_OK;
  const Geometry& g = p->geo;
  const size_t N = (size_t)g.W * g.H, es = p->elem();
  const int rank = comm_rank(c), world = comm_world(c);
  const int up = rank > 0 ? rank - 1 : -1, down = rank + 1 < world ? rank + 1 : -1;
  char* x = (char*)x_dev;
  if (sd->mode == SRMAP_SHARD_ROWS) {
    // a frame whose warpAffine y coordinate sits on a 1/32-px rounding tie carries a per-row table built from the row
    // index of THIS problem (model_tables.hpp make_warp): a band problem would evaluate the tie at its local rows, not
    // the joint image's
    if (p->motion.has_ytabs())
      return set_error(p->ctx, SRMAP_EUNSUPPORTED, "row shard: a sub-pixel shift on a 1/32-px rounding tie needs the joint image's row index; shard such problems by frames or channels");
    const int hu = sd->own_row0, hd = g.H - sd->own_row1;  // my halo rows above / below
    if ((up >= 0 && hu == 0) || (down >= 0 && hd == 0) || sd->send_down_rows > sd->own_row1 - sd->own_row0 ||
        sd->send_up_rows > sd->own_row1 - sd->own_row0)
      return set_error(p->ctx, SRMAP_EINVAL, "row shard: halo description inconsistent");
    if ((up >= 0 && sd->send_up_rows <= 0) || (down >= 0 && sd->send_down_rows <= 0))
      return set_error(p->ctx, SRMAP_EINVAL, "row shard: a neighbour exists but no rows are sent to it (it would wait for them)");
    std::vector<const void*> sa(g.C), sb(g.C);
    std::vector<void*> ra(g.C), rb(g.C);
    for (int ch = 0; ch < g.C; ++ch) {
      // downward traffic: my last owned rows -> lower neighbour's top halo; my top halo <- upper neighbour
      sa[ch] = x + ((size_t)ch * N + (size_t)(sd->own_row1 - sd->send_down_rows) * g.W) * es;
      ra[ch] = x + ((size_t)ch * N) * es;
      // upward traffic: my first owned rows -> upper neighbour's bottom halo; my bottom halo <- lower neighbour
      sb[ch] = x + ((size_t)ch * N + (size_t)sd->own_row0 * g.W) * es;
      rb[ch] = x + ((size_t)ch * N + (size_t)sd->own_row1 * g.W) * es;
    }
    // both directions in ONE group (one launch on the stream)
    return comm_exchange2(c, sa.data(), ra.data(), (size_t)sd->send_down_rows * g.W, (size_t)hu * g.W, sb.data(), rb.data(),
                          (size_t)sd->send_up_rows * g.W, (size_t)hd * g.W, up, down, g.C, p->dtype, st);
  }
  if (sd->mode == SRMAP_SHARD_CHANNELS || sd->mode == SRMAP_SHARD_GRID) {
    const bool lo = sd->own_ch0 > 0, hi = sd->own_ch1 < g.C;  // halo planes present (3-D TV coupling)
    if (!lo && !hi) return SRMAP_OK;
    // GRID: the channel neighbours are the ranks of the same frame group in the adjacent channel blocks
    const int stride = sd->mode == SRMAP_SHARD_GRID ? (sd->frame_groups > 0 ? sd->frame_groups : 1) : 1;
    const int cup = rank - stride >= 0 ? rank - stride : -1, cdown = rank + stride < world ? rank + stride : -1;
    // downward: my last owned plane -> lower neighbour's low halo plane; my low halo <- upper neighbour
    const void* s1 = x + (size_t)(sd->own_ch1 - 1) * N * es;
    void* r1 = x + (size_t)(sd->own_ch0 - 1) * N * es;
    // upward: my first owned plane -> upper neighbour's high halo plane; my high halo <- lower neighbour
    const void* s2 = x + (size_t)sd->own_ch0 * N * es;
    void* r2 = x + (size_t)sd->own_ch1 * N * es;
    return comm_exchange2(c, &s1, &r1, hi ? N : 0, lo ? N : 0, &s2, &r2, lo ? N : 0, hi ? N : 0, lo ? cup : -1, hi ? cdown : -1, 1,
                          p->dtype, st);
  }
  return SRMAP_OK;
}

int shard_eval(srmap_problem* p, srmap_comm* c, const srmap_shard_desc* sd, EvalReq req, EvalOut* out, unsigned terms,
               void* x_dev, void* g_dev, hipStream_t st) {
  const int mode = shard_mode(c, sd);
  if (mode == SRMAP_SHARD_NONE) return eval_dispatch(p, req, out, terms, x_dev, g_dev, st);
  const size_t N = (size_t)p->geo.W * p->geo.H, es = p->elem();
  if (mode == SRMAP_SHARD_ROWS) {
    // The halo rows of x travel on the communicator's side stream while the evaluation's stream runs the tile rows
    // that read none of them; the boundary tile rows wait for the event (kernels_ztile.hip launch_z; paths without
    // that split exchange first).  x is ready when `st` reaches this point; the next exchange cannot start before
    // this evaluation (which reads the halos) is behind the next ev_x.
    // Overlap only where it is both enabled on the communicator and SAFE: the caller's halo must be at least the tile
    // kernel's reach (x rows 2 above / 3 below a tile row: blur transpose + regulariser window), otherwise an
    // "interior" tile row would read a row the exchange is still writing.
    const int hu = sd->own_row0, hd = p->geo.H - sd->own_row1;
    constexpr int kReach = 4;
    const bool overlap = comm_overlap(c) && ztile_overlaps_halo(p) && (hu == 0 || hu >= kReach) && (hd == 0 || hd >= kReach);
    if (!overlap) {
      int rc = shard_exchange_x(p, c, sd, x_dev, st);
      if (rc) return rc;
      return eval_dispatch(p, req, out, terms, x_dev, g_dev, st);
    }
    struct Hook { srmap_problem* p; srmap_comm* c; const srmap_shard_desc* sd; void* x; hipStream_t side; hipEvent_t ev; bool called; };
    hipStream_t side; hipEvent_t ev_x, ev_halo;
    int rc = comm_side(c, &side, &ev_x, &ev_halo);
    if (rc) return rc;
    SRMAP_HIP(p->ctx, hipEventRecord(ev_x, st));
    SRMAP_HIP(p->ctx, hipStreamWaitEvent(side, ev_x, 0));
    Hook h{p, c, sd, x_dev, side, ev_halo, false};
    req.overlap.fn = [](void* a) -> int {
      Hook* k = static_cast<Hook*>(a);
      k->called = true;
      int r = shard_exchange_x(k->p, k->c, k->sd, k->x, k->side);
      if (r) return r;
      SRMAP_HIP(k->p->ctx, hipEventRecord(k->ev, k->side));
      return SRMAP_OK;
    };
    req.overlap.arg = &h;
    req.overlap.event = ev_halo;
    req.overlap.top = hu;
    req.overlap.bot = hd;
    rc = eval_dispatch(p, req, out, terms, x_dev, g_dev, st);  // cost rows were set on the problem
    // An evaluation that failed before it reached the hook has not posted this rank's half of the exchange: post it
    // now, so that the neighbours' receives complete and they see an error code instead of a hang.
    if (!h.called) {
      const int rx = shard_exchange_x(p, c, sd, x_dev, side);
      if (rc == SRMAP_OK) rc = rx;
    }
    return rc;
  }
  int rc = shard_exchange_x(p, c, sd, x_dev, st);
  if (rc) return rc;
  if (mode == SRMAP_SHARD_FRAMES) {
    // Every rank adds its frames' data term.  The regulariser is evaluated once over the ranks: split by row band
    // (whole tile rows, balanced) when the tile kernel alone produces it -- at cfg2-class mixes it is more than half of
    // the arithmetic, so leaving it to one rank would make that rank the critical path -- else on reg_rank.
    const int rank = comm_rank(c), world = comm_world(c);
    unsigned t = terms;
    // The split is a COLLECTIVE decision: a rank whose own frame subset has no tile plan (a shift on a 1/32-px rounding
    // tie, a per-rank SRMAP_IMPL_DIRECT, ...) cannot evaluate a band, and if it went its own way the regulariser would
    // be counted twice or not at all.  The ranks agree once (minimum of their flags over the communicator; cached on
    // the problem until its plan generation -- bumped by every re-plan and every srmap_problem_set_impl --, term set or
    // communicator changes); any rank that cannot band-split sends everybody to reg_rank.  The agreement is itself a
    // collective: under frame sharding srmap_problem_set_impl and the regulariser calls are COLLECTIVE too (every rank
    // makes them in the same order between the same evaluations; include/srmap.h), or one rank would enter it alone.
    const bool mine = ztile_reg_band_ok(p, terms);
    if (p->band_comm != (const void*)c || p->band_terms != terms || p->band_gen != p->plan_gen) {
      double flag = mine ? 0.0 : 1.0;  // max over the ranks of "I cannot" == 0  <=>  every rank can
      SRMAP_HIP(p->ctx, hipMemcpyAsync(p->d_cost.as<double>() + kCostBand, &flag, sizeof(double), hipMemcpyHostToDevice, st));
      rc = comm_allreduce(c, p->d_cost.as<double>() + kCostBand, 1, SRMAP_F64, 1, st);
      if (rc) return rc;
      SRMAP_HIP(p->ctx, hipMemcpyAsync(&flag, p->d_cost.as<double>() + kCostBand, sizeof(double), hipMemcpyDeviceToHost, st));
      SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
      p->band_all = flag == 0.0;
      p->band_comm = c; p->band_terms = terms; p->band_gen = p->plan_gen;
    }
    const bool band = mine && p->band_all;
    if (band) {
      const int tiles = (p->geo.H + 7) / 8, per = (tiles + world - 1) / world;
      req.rr0 = rank * per * 8;
      req.rr1 = (rank + 1) * per * 8;
    } else if (rank != sd->reg_rank) {
      t = terms & SRMAP_TERM_DATA;
    }
    if (t == 0) {
      SRMAP_HIP(p->ctx, hipMemsetAsync(p->d_cost.as<double>(), 0, sizeof(double), st));
      if (g_dev) SRMAP_HIP(p->ctx, hipMemsetAsync(g_dev, 0, p->hr_count() * es, st));
    } else {
      rc = eval_dispatch(p, req, out, t, x_dev, g_dev, st);
    }
    if (rc) return rc;
    // the north-star's gradient all-reduce, with the cost in the same group (one launch)
    return comm_allreduce_grad_cost(c, g_dev, g_dev ? p->hr_count() : 0, p->dtype, p->d_cost.as<double>(), st);
  }
  if (mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) {
    const int fgs = (mode == SRMAP_SHARD_GRID && sd->frame_groups > 1) ? sd->frame_groups : 1;
    const int fg = comm_rank(c) % fgs;
    // GRID: the regulariser terms of a channel block are evaluated once, by its frame group 0
    const unsigned t = (fg == 0) ? terms : (terms & SRMAP_TERM_DATA);
    req.view.c0 = sd->own_ch0; req.view.C = sd->own_ch1 - sd->own_ch0; req.view.coupled = true;
    const size_t cnt = (size_t)req.view.C * N;
    char* gown = g_dev ? (char*)g_dev + (size_t)sd->own_ch0 * N * es : nullptr;
    if (t == 0) {
      rc = SRMAP_OK;
      SRMAP_HIP(p->ctx, hipMemsetAsync(p->d_cost.as<double>(), 0, sizeof(double), st));
      if (gown) SRMAP_HIP(p->ctx, hipMemsetAsync(gown, 0, cnt * es, st));
    } else {
      rc = eval_dispatch(p, req, out, t, (char*)x_dev + (size_t)sd->own_ch0 * N * es, gown, st);
    }
    if (rc) return rc;
    if (fgs > 1 && gown) {  // sum of the frame groups' data-term gradients of this channel block
      if (!sd->frame_comm) return set_error(p->ctx, SRMAP_EINVAL, "grid shard: frame_comm missing");
      rc = comm_allreduce(sd->frame_comm, gown, cnt, p->dtype, 0, st);
    }
    return rc;
  }
  return eval_dispatch(p, req, out, terms, x_dev, g_dev, st);  // rows: cost rows were set on the problem
}

}  // namespace srmap

using namespace srmap;

extern "C" {

int srmap_eval_sharded_device(srmap_problem* p, srmap_comm* comm, const srmap_shard_desc* shard, unsigned terms,
                              void* x_dev, void* g_dev, double* cost, void* hip_stream) {
  if (!p || !x_dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  hipStream_t st = stream_of(p->ctx, hip_stream);
  const int mode = shard_mode(comm, shard);
  if (int rc = refuse_sharded(p, mode, "evaluate")) return rc;
  EvalOut out;
  int rc = shard_eval(p, comm, shard, EvalReq(), &out, terms, x_dev, g_dev, st);
  if (rc) return rc;
  if (cost) {
    if (mode == SRMAP_SHARD_ROWS || mode == SRMAP_SHARD_CHANNELS || mode == SRMAP_SHARD_GRID) {
      rc = comm_allreduce(comm, p->d_cost.as<double>(), 1, SRMAP_F64, 0, st);
      if (rc) return rc;
    }
    SRMAP_HIP(p->ctx, hipMemcpyAsync(cost, p->d_cost.as<double>(), sizeof(double), hipMemcpyDeviceToHost, st));
    SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  }
  return SRMAP_OK;
}

}  // extern "C"
