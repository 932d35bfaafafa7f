// ztile_tables_test -- csrc/ztile_tables.hpp (the host arithmetic of the tile plan) for the brute-force checks of
// tests/test_ztile_tables_cpu.py.  CPU only: includes nothing but that header and links nothing of the library.  Reads
// cases on stdin and prints one result line per case, integers in decimal and doubles with %a:
//   ft S C w h K {ox oy}[K]               ->  ok MS n_ent hdr[S*S]{n first} ent[n_ent]{k io jo oyx} cnt[S*8] off[MS*S*S]
//                                             aux[MS*S*S]{k io jo oyx} cnt0[32] off0[16] aux0[16]{k io jo oyx}   (ok = 0: "0")
//   st S hb K {ox oy ntaps w[4]}[K]       ->  spmax spn[4] srctab[S*spmax]{k io q am w0 w1}
//   rr S B W H K {ox oy}[K]               ->  rg[6] ring_count
//   ff W H reach S                        ->  0 | 1   (ztile_frame_fits)
//   b3 k2[9] k1[3]                        ->  0 | 1   (ztile_blur3_symmetric)
//   kk                                    ->  kSpChunk kSpNull kBorderTabEntries kMaxTileShift
#include <cstdio>
#include <cstring>
#include <vector>

#include "ztile_tables.hpp"

using namespace srmap;

struct Warp { int ox, oy, ntaps; double w[4]; };

static void entry(const ZEntry& e) { std::printf(" %d %d %d %d", e.k, e.io, e.jo, e.oyx); }

static bool offsets(int K, std::vector<int>* ox, std::vector<int>* oy) {
  ox->resize((size_t)K); oy->resize((size_t)K);
  for (int k = 0; k < K; ++k)
    if (std::scanf("%d %d", &(*ox)[(size_t)k], &(*oy)[(size_t)k]) != 2) return false;
  return true;
}

int main() {
  char what[8];
  std::vector<int> ox, oy;
  while (std::scanf("%7s", what) == 1) {
    if (std::strcmp(what, "ft") == 0) {
      int S = 0, C = 0, w = 0, h = 0, K = 0;
      if (std::scanf("%d %d %d %d %d", &S, &C, &w, &h, &K) != 5 || S < 2 || S > 4 || K < 1 || !offsets(K, &ox, &oy)) return 2;
      ZFrameTables t;
      if (!t.build(S, K, ox.data(), oy.data(), C, w, h)) { std::printf("0\n"); continue; }
      std::printf("1 %d %d", t.MS, (int)t.ent.size());
      for (const ZHdr& hd : t.hdr) std::printf(" %d %d", hd.n, hd.first);
      for (const ZEntry& e : t.ent) entry(e);
      for (int v : t.cnt) std::printf(" %d", v);
      for (long long v : t.off) std::printf(" %lld", v);
      for (const ZEntry& e : t.aux) entry(e);
      for (int v : t.cnt0) std::printf(" %d", v);
      for (long long v : t.off0) std::printf(" %lld", v);
      for (const ZEntry& e : t.aux0) entry(e);
    } else if (std::strcmp(what, "st") == 0) {
      int S = 0, hb = 0, K = 0;
      if (std::scanf("%d %d %d", &S, &hb, &K) != 3 || S < 2 || S > 4 || K < 1) return 2;
      std::vector<Warp> bwd((size_t)K);
      for (Warp& b : bwd)
        if (std::scanf("%d %d %d %lf %lf %lf %lf", &b.ox, &b.oy, &b.ntaps, &b.w[0], &b.w[1], &b.w[2], &b.w[3]) != 7) return 2;
      const ZSourceTable t = ztile_source_table(S, K, bwd.data(), hb);
      std::printf("%d %d %d %d %d", t.spmax, t.spn[0], t.spn[1], t.spn[2], t.spn[3]);
      for (const ZSrc& q : t.srctab) std::printf(" %d %d %d %d %a %a", q.k, q.io, q.q, q.am, q.w0, q.w1);
    } else if (std::strcmp(what, "rr") == 0) {
      int S = 0, B = 0, W = 0, H = 0, K = 0;
      if (std::scanf("%d %d %d %d %d", &S, &B, &W, &H, &K) != 5 || K < 1 || !offsets(K, &ox, &oy)) return 2;
      const RingRects rr = ztile_ring_rects(S, B, K, ox.data(), oy.data());
      for (int v : rr.rg) std::printf(" %d", v);
      std::printf(" %lld", ring_count(rr, W, H));
    } else if (std::strcmp(what, "ff") == 0) {
      int W = 0, H = 0, reach = 0, S = 0;
      if (std::scanf("%d %d %d %d", &W, &H, &reach, &S) != 4) return 2;
      std::printf("%d", (int)ztile_frame_fits(W, H, reach, S));
    } else if (std::strcmp(what, "b3") == 0) {
      double k2[9], k1[3];
      for (double& v : k2) if (std::scanf("%lf", &v) != 1) return 2;
      for (double& v : k1) if (std::scanf("%lf", &v) != 1) return 2;
      std::printf("%d", (int)ztile_blur3_symmetric(k2, k1));
    } else if (std::strcmp(what, "kk") == 0) {
      std::printf("%d %d %d %d", kSpChunk, kSpNull, kBorderTabEntries, kMaxTileShift);
    } else {
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
