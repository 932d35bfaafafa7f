// ztile_tables.hpp -- the host arithmetic of the tile plan (ztile_plan.hip) as functions from numbers to vectors, and the
// table records the tile kernels (ztile_dev.hpp) share with it.  Plain C++: no HIP, no problem, no device
// (tests/cpp/ztile_tables_test.cpp compiles this header alone).  Formulation: DESIGN.md section 3.1.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace srmap {

// integer floor division / modulo (constexpr: host arithmetic, device code and constant expressions alike)
constexpr int fdiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
constexpr int pmod(int a, int b) { return a - fdiv(a, b) * b; }

// Sub-pixel instances, source-major table: one record per (frame, vertical tap of the transpose warp) that lands on a
// row phase -- LR row offset io, the two horizontal tap weights (already multiplied by the vertical one) and what follows
// from the frame's integer column offset ox alone, worked out on the host (the scalar unit of a CU is shared by its
// sixteen waves: per-source divisions and range tests there were a fifth of the kernel): a = (-ox) mod S, the residual
// column offset q = (ox + a) / S of e = 0, and the first of the residual columns e in {-1, 0, 1} a cell's S + 2 HB pixels
// use (am = a | (e_lo + 1) << 8; the kSpSlots(S, HB) columns from e_lo on are requested unconditionally -- no per-column
// test on the scalar unit).  Rows of the table are padded to a multiple of kSpChunk with null records (am = kSpNull,
// weights 0): a chunk's records are loaded back to back without control flow in between (z_row_sp2).
struct ZSrc { int k, io, q, am; double w0, w1; };
constexpr int kSpNull = 0xff;
constexpr int kSpChunk = 4;
struct ZEntry { int k, io, jo, oyx; };  // frame, LR row / column offset of the residual a pixel of this phase owns,
                                         // forward offset packed (oy << 16) | (ox & 0xffff)
struct ZHdr { int n, first; };           // flat frame table: (count, first entry) of a (row phase, column phase); the
                                         // border blocks read it as an int2
constexpr int kBorderTabEntries = 256;   // frame-table entries staged in LDS by the border blocks

// The pixels of the border frame that can carry work, as six rectangles in HR coordinates (ztile_ring_rects()).
// With blur reach (B - 1) / 2 <= 1 < S a frame k with forward offset o_k = (ox, oy) has
//   * a residual whose z position S (i, j) + o_k lies OUTSIDE the image only in the rows [min oy, 0) / [H, H + max oy - S]
//     and the columns [min ox, 0) / [W, W + max ox - S]                                (cost of ownerless residuals),
//   * a contribution to an in-image pixel q that the clipped transpose warp excludes (q - o_k outside, while a residual
//     sits within blur reach of q) only for q - o_k = -1 in a row or column, i.e. rows [0, max oy) and columns [0, max ox)
//     (gradient corrections).
// Everything else of the 2E-wide frame around the image edge evaluates to zero and is not enumerated.
//   rg[0] = ti: TOP-INSIDE     rows [0, ti)       x columns [0, W)
//   rg[1] = li: LEFT-INSIDE    columns [0, li)    x rows [ti, H)
//   rg[2] = to: TOP-OUTSIDE    rows [-to, 0)      x columns [-lo, W + ro)
//   rg[3] = bo: BOTTOM-OUTSIDE rows [H, H + bo)   x columns [-lo, W + ro)
//   rg[4] = lo: LEFT-OUTSIDE   columns [-lo, 0)   x rows [0, H)
//   rg[5] = ro: RIGHT-OUTSIDE  columns [W, W+ro)  x rows [0, H)
struct RingRects { int rg[6]; };
static_assert(std::is_trivially_copyable_v<RingRects>, "a kernel argument: no owner inside");

constexpr long long ring_count(const RingRects& r, int W, int H) {
  const long long ti = r.rg[0], li = r.rg[1], to = r.rg[2], bo = r.rg[3], lo = r.rg[4], ro = r.rg[5];
  return ti * W + li * (H - ti) + (to + bo) * (W + lo + ro) + (lo + ro) * H;
}

// ---- what the plan accepts, as far as it needs no problem state ----
constexpr int kMaxTileShift = 4096;  // largest |integer offset| of a frame
// the tile kernel carries the three distinct values of a symmetric 3 x 3 kernel k2 = k1 k1^T: corner, edge, centre
inline bool ztile_blur3_symmetric(const double* k2, const double* k1) {
  return k2[0] == k2[2] && k2[0] == k2[6] && k2[0] == k2[8] && k2[1] == k2[3] && k2[1] == k2[5] && k2[1] == k2[7] && k1[0] == k1[2];
}
// the frame of width 2 * reach around the image edge (border blocks: reach = E; sub-pixel plans: the ring, reach = Dr)
// must stay a small part of the image
constexpr bool ztile_frame_fits(int W, int H, int reach, int S) { return !(W <= 4 * reach + 2 * S || H <= 4 * reach + 2 * S); }

// ---- integer shifts: the frame table ----
// Pixel (row phase pr, column phase pc) owns the residual of frame k iff (pr - oy) and (pc - ox) are multiples of S; the
// LR pixel is (rc + io, cell + jo).  hdr / ent: the flat table of the border blocks.  cnt / off / aux: the tile kernel's
// layout of the same table, [round t][pr][pc], with the observation's element offset precomputed; cnt [pr][8]: the
// residuals per column phase, [pr][S] their maximum and [pr][S + 1] their minimum.  cnt0 / off0 / aux0: the copies that
// travel by value in the kernel arguments ([4][8] counts, [4][4] round 0).
struct ZFrameTables {
  std::vector<ZHdr> hdr;
  std::vector<ZEntry> ent;
  int MS = 1;  // rounds: slots per (row phase, column phase)
  std::vector<int> cnt;
  std::vector<long long> off;
  std::vector<ZEntry> aux;
  int cnt0[32] = {0};
  long long off0[16] = {0};
  ZEntry aux0[16] = {};
  // ox / oy: the K forward offsets; C channels of w x h LR pixels.  false: more entries than the border blocks stage
  // (the tile kernel's tables are not built then)
  bool build(int S, int K, const int* ox, const int* oy, int C, int w, int h) {
    hdr.assign((size_t)S * S, ZHdr{0, 0});
    ent.clear();
    for (int pr = 0; pr < S; ++pr)
      for (int pc = 0; pc < S; ++pc) {
        ZHdr hd{0, (int)ent.size()};
        for (int k = 0; k < K; ++k) {
          if (pmod(pr - oy[k], S) != 0 || pmod(pc - ox[k], S) != 0) continue;
          ZEntry e; e.k = k; e.io = fdiv(pr - oy[k], S); e.jo = fdiv(pc - ox[k], S);
          e.oyx = (int)(((unsigned)oy[k] << 16) | ((unsigned)ox[k] & 0xffffu));
          ent.push_back(e);
          hd.n++;
        }
        hdr[(size_t)pr * S + pc] = hd;
      }
    if (ent.empty()) { ZEntry e = {0, 0, 0, 0}; ent.push_back(e); }
    if ((int)ent.size() > kBorderTabEntries) return false;  // the border blocks stage the table in LDS
    MS = 1;
    for (const ZHdr& hd : hdr) MS = std::max(MS, hd.n);
    cnt.assign((size_t)S * 8, 0);
    off.assign((size_t)S * MS * S, 0);
    aux.assign((size_t)S * MS * S, ZEntry{0, 0, 0, 0});
    const long long nl = (long long)w * h;
    for (int pr = 0; pr < S; ++pr) {
      int mx = 0;
      for (int pc = 0; pc < S; ++pc) {
        const ZHdr hd = hdr[(size_t)pr * S + pc];
        cnt[(size_t)pr * 8 + pc] = hd.n;
        mx = std::max(mx, hd.n);
        for (int r = 0; r < hd.n; ++r) {
          const ZEntry& e = ent[(size_t)hd.first + r];
          const size_t slot = ((size_t)r * S + pr) * S + pc;
          aux[slot] = e;
          off[slot] = (long long)e.k * C * nl + (long long)e.io * w + e.jo;
        }
      }
      cnt[(size_t)pr * 8 + S] = mx;
      int mn = INT_MAX;
      for (int pc = 0; pc < S; ++pc) mn = std::min(mn, cnt[(size_t)pr * 8 + pc]);
      cnt[(size_t)pr * 8 + S + 1] = mn;
      for (int pc = 0; pc < S; ++pc) {
        off0[pr * 4 + pc] = off[((size_t)0 * S + pr) * S + pc];
        aux0[pr * 4 + pc] = aux[((size_t)0 * S + pr) * S + pc];
      }
    }
    for (size_t i = 0; i < cnt.size(); ++i) cnt0[i] = cnt[i];
    return true;
  }
};

// the rectangles of the border frame that can carry work, from the range of the K forward offsets
inline RingRects ztile_ring_rects(int S, int B, int K, const int* ox, const int* oy) {
  int mnx = 0, mxx = 0, mny = 0, mxy = 0;
  for (int k = 0; k < K; ++k) {
    mnx = std::min(mnx, ox[k]); mxx = std::max(mxx, ox[k]);
    mny = std::min(mny, oy[k]); mxy = std::max(mxy, oy[k]);
  }
  RingRects rr;
  rr.rg[0] = (B > 1) ? std::max(0, mxy) : 0;   // corrections need a blur tap between the pixel and the residual
  rr.rg[1] = (B > 1) ? std::max(0, mxx) : 0;
  rr.rg[2] = std::max(0, -mny);
  rr.rg[3] = std::max(0, mxy - S + 1);
  rr.rg[4] = std::max(0, -mnx);
  rr.rg[5] = std::max(0, mxx - S + 1);
  return rr;
}

// ---- sub-pixel shifts: the source table ----
// z(p) = sum over (frame, bilinear tap of the TRANSPOSE warp) pairs that land on the LR grid.  The taps source-major
// (z_row_sp2): per row phase one record per (frame, vertical tap) on the LR grid, the rows [spmax] records apart and
// padded with null records; spn[pr]: the records of row phase pr that are walked (a multiple of kSpChunk).
struct ZSourceTable {
  std::vector<ZSrc> srctab;  // [S][spmax]
  int spn[4] = {0, 0, 0, 0};
  int spmax = 0;
};
// bwd: the K transpose warps (ox, oy, ntaps, w[4] as (dx, dy) taps (0,0) (1,0) (0,1) (1,1)); hb: the blur's half width
template <typename Warp>
ZSourceTable ztile_source_table(int S, int K, const Warp* bwd, int hb) {
  std::vector<std::vector<ZSrc>> srcs((size_t)S);
  for (int pr = 0; pr < S; ++pr)
    for (int k = 0; k < K; ++k) {
      const Warp& b = bwd[k];
      for (int dy = 0; dy < 2; ++dy) {
        double w0 = 0.0, w1 = 0.0;
        for (int t = 0; t < b.ntaps; ++t)
          if ((t >> 1) == dy) { if (t & 1) w1 = b.w[t]; else w0 = b.w[t]; }
        if (w0 == 0.0 && w1 == 0.0) continue;
        const int rr = pr + b.oy + dy;
        if (pmod(rr, S) != 0) continue;
        ZSrc q; q.k = k; q.io = fdiv(rr, S); q.w0 = w0; q.w1 = w1;
        const int a = pmod(-b.ox, S);
        q.q = (b.ox + a) / S;  // exact
        // the first residual column e in {-1, 0, 1} that a cell's S + 2 HB pixels use (sp_apply derives the same from a)
        const bool lo = (a - S >= -hb) || (a - 1 - S >= -hb);
        q.am = a | ((lo ? 0 : 1) << 8);  // (e_lo + 1) << 8
        srcs[(size_t)pr].push_back(q);
      }
    }
  ZSourceTable t;
  int spmax = kSpChunk;
  for (const auto& l : srcs) spmax = std::max(spmax, (int)((l.size() + kSpChunk - 1) / kSpChunk) * kSpChunk);
  t.spmax = spmax;
  t.srctab.assign((size_t)S * spmax, ZSrc{0, 0, 0, kSpNull, 0.0, 0.0});   // null records behind the sources
  for (int pr = 0; pr < S; ++pr) {
    t.spn[pr] = (int)((srcs[(size_t)pr].size() + kSpChunk - 1) / kSpChunk) * kSpChunk;
    for (size_t n = 0; n < srcs[(size_t)pr].size(); ++n) t.srctab[(size_t)pr * spmax + n] = srcs[(size_t)pr][n];
  }
  return t;
}

}  // namespace srmap
