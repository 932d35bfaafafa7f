"""Instruments a COPY of csrc/kernels_ztile.hip (written to /tmp/spx/kz_time.hip) with per-wave s_memtime stamps at the
phase boundaries of k_eval_z and a setter srmap_dbg_set_timing(buffer).  Timing-only: see build.sh / run.py."""
import sys
root = sys.argv[1] if len(sys.argv) > 1 else "/root/repo"
# optional 2nd argument: another kernels_ztile.hip to instrument (e.g. the parent commit's, with its headers beside
# it); optional 3rd: where the instrumented copy goes
srcfile = sys.argv[2] if len(sys.argv) > 2 else root + '/super-resolution_amd/csrc/kernels_ztile.hip'
outfile = sys.argv[3] if len(sys.argv) > 3 else '/tmp/spx/kz_time.hip'
src=open(srcfile).read()
s=src
anchor = 'template <typename T, int S, int B, int REGK, int R, bool WD, bool SP>\n__global__'
assert anchor in s
s=s.replace(anchor,'__device__ unsigned long long* g_ztdbg = nullptr;\n#define ZT_STAMP(i) do { zts[i] = __builtin_readcyclecounter(); } while (0)\n\n' + anchor,1)
def rep(old,new):
    global s
    assert old in s, old
    s=s.replace(old,new,1)
# the wave's first instruction (ahead of the argument batch) and its last (behind the cost / g.d partial): the head
# from wave start to the first x request and the tail from the end of phase 2 to the wave's end are stamps 13 and 14
rep('''  __shared__ T whs[(C::RU > 0 ? C::RU : 1) * S * C::CW];  // IRLS weights of the halo rows of 2*lambda*w*r
''','''  __shared__ T whs[(C::RU > 0 ? C::RU : 1) * S * C::CW];  // IRLS weights of the halo rows of 2*lambda*w*r
  const unsigned long long zt_start = __builtin_readcyclecounter();
''')
rep('''  const int R0 = tby * C::TH, CJ0 = tbx * C::CW, C0 = CJ0 * S;''','''  const int R0 = tby * C::TH, CJ0 = tbx * C::CW, C0 = CJ0 * S;
  unsigned long long* dbg = g_ztdbg ? g_ztdbg + ((size_t)(by * gridDim.x + blockIdx.x) * 8 + wv) * 16 : nullptr;
  unsigned long long zts[10];
  const unsigned long long rt0 = wall_clock64();  // s_memrealtime: 100 MHz, common to the whole chip
  const unsigned hwid = __builtin_amdgcn_s_getreg(63492), xccid = __builtin_amdgcn_s_getreg(63508);
  ZT_STAMP(0);''')
rep('''  T ypre[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) ypre[v] = T(0);''','''  ZT_STAMP(1);
  T ypre[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) ypre[v] = T(0);''')
rep('''  if (!SP && has_z_halo) z_row_prefetch<T, S, B, C>(A, hrowz, R0, CJ0, lane, edge, ybase, ypre2);''','''  ZT_STAMP(2);
  if (!SP && has_z_halo) z_row_prefetch<T, S, B, C>(A, hrowz, R0, CJ0, lane, edge, ybase, ypre2);
  ZT_STAMP(3);''')
rep('''  // ---------------- x tile -> LDS, polyphase ----------------''','''  ZT_STAMP(4);
  // ---------------- x tile -> LDS, polyphase ----------------''')
rep('''  // in-image mask of this thread's pixels (partial tiles at the right / bottom edge)''','''  ZT_STAMP(5);
  // in-image mask of this thread's pixels (partial tiles at the right / bottom edge)''')
rep('''  // ---------------- phase 1: regulariser ----------------''','''  ZT_STAMP(6);
  // ---------------- phase 1: regulariser ----------------''')
# barrier 2 = the last __syncthreads() ahead of phase 2 (the cost partial's thread-0 sum may stand between the two)
k = s.rindex('  __syncthreads();\n', 0, s.index('  // ---------------- phase 2 ----------------'))
s = s[:k] + '  ZT_STAMP(7);\n  __syncthreads();\n  ZT_STAMP(8);\n' + s[k + len('  __syncthreads();\n'):]
# stamp 9 = the g stores are issued (whatever follows them: the cost partial of the parent form, the g.d partial)
rep('''    for (int pc = 0; pc < S; ++pc) __builtin_nontemporal_store(acc[pc], &dst[pc]);  // written once, not re-read here
  }
''','''    for (int pc = 0; pc < S; ++pc) __builtin_nontemporal_store(acc[pc], &dst[pc]);  // written once, not re-read here
  }
  ZT_STAMP(9);
''')
i = s.index('finish_block<WD, C::NT>(A, &red[0][0]);')
j = s.index('\n}\n', i)
s = s[:j] + '''
  {
    const unsigned long long zt_end = __builtin_readcyclecounter();
    if (dbg && lane == 0) { for (int q = 0; q < 10; ++q) dbg[q] = zts[q]; dbg[10] = rt0; dbg[11] = wall_clock64(); dbg[12] = ((unsigned long long)xccid << 32) | hwid; dbg[13] = zt_start; dbg[14] = zt_end; }
  }''' + s[j:]
rep('''    if (bidx * C::NT < Bd.n_ring) {''','''    const unsigned long long brt0 = wall_clock64();
    if (bidx * C::NT < Bd.n_ring) {''')
rep('''    else if (threadIdx.x == 0) {
      const int nbb = A.nby * gridDim.x;''','''    if (g_ztdbg && threadIdx.x == 0) { unsigned long long* d = g_ztdbg + ((size_t)(2048 + bidx) * 8) * 16; d[10] = brt0; d[11] = wall_clock64(); d[12] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | __builtin_amdgcn_s_getreg(63492); d[13] = (bidx * C::NT < Bd.n_ring); }
    if (!(bidx * C::NT < Bd.n_ring) && threadIdx.x == 0) {
      const int nbb = A.nby * gridDim.x;''')
rep('// ---------------------------------------------------------------------------------------------------------\n// host side: ','extern "C" int srmap_dbg_set_timing(unsigned long long* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ztdbg), &buf, sizeof(buf)); }\n// ---------------------------------------------------------------------------------------------------------\n// host side: ')
open(outfile,'w').write(s)
