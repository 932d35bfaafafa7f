#!/bin/bash
# tools/phase_clock/build.sh: TIMING-ONLY build of the tile kernel with s_memtime stamps at the phase boundaries
# (patch_kernel.py instruments a COPY of kernels_ztile.hip under /tmp; the product sources and libsrmap.so are not
# touched; further arguments go to the compiler, e.g. -DSRMAP_ZT_ONLY_CFG2).  Output: tools/phase_clock/libsrmap_time.so
# (git-ignored), run with tools/phase_clock/run.py on the GPU box.
set -e
root=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p /tmp/spx
# SRMAP_TIME_SRC: another kernels_ztile.hip (the parent commit's, its headers beside it); SRMAP_TIME_OUT: the library's name
src=${SRMAP_TIME_SRC:-$root/super-resolution_amd/csrc/kernels_ztile.hip}
out=${SRMAP_TIME_OUT:-$root/tools/phase_clock/libsrmap_time.so}
python "$root/tools/phase_clock/patch_kernel.py" "$root" "$src" /tmp/spx/kz_time.hip
cd /tmp/spx && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -mllvm -simplifycfg-sink-common=false -I"$root/include" -I"$(dirname "$src")" -I"$root/super-resolution_amd/csrc" "$@" -c kz_time.hip -o kz_time.o
cd "$root/super-resolution_amd/lib"
objs=$(ls *.hip.o | grep -v kernels_ztile)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out" $objs /tmp/spx/kz_time.o -L/opt/rocm/lib -lrocblas -lrocsolver -ldl -Wl,-rpath,/opt/rocm/lib
echo built "$out"
