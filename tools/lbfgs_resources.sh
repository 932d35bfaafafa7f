#!/bin/bash
# Register / LDS / spill table of every L-BFGS pass instance (kernels_lbfgs.hip; cross-compiles, no GPU needed):
#   tools/lbfgs_resources.sh
# instance = kernel<T, V (elements per request), L (live history slots)>
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
cd "$OUT" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -mllvm -simplifycfg-sink-common=false \
  -I"$ROOT/include" -I"$ROOT/super-resolution_amd/csrc" -c "$ROOT/super-resolution_amd/csrc/kernels_lbfgs.hip" -save-temps -o kl.o 2>/dev/null || exit 1
python3 - kernels_lbfgs-hip-amdgcn-amd-amdhsa-gfx950.s <<'PY'
import re, sys
text = open(sys.argv[1]).read()
meta = text[text.index("amdhsa.kernels:"):]
rows = []
for blk in re.split(r"\n  - ", meta)[1:]:
    f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)", blk, flags=re.M))
    name = f.get("name", "")
    m = re.search(r"(k_lbfgs_\w+?)I([df])Li(\d+)ELi(\d+)E", name)
    if not m:
        continue
    inst = "%s<%s,%s,%s>" % (m.group(1), "f64" if m.group(2) == "d" else "f32", m.group(3), m.group(4))
    rows.append((inst, f.get("group_segment_fixed_size"), f.get("sgpr_count"), f.get("sgpr_spill_count"),
                 f.get("vgpr_count"), f.get("vgpr_spill_count")))
print("%-32s %5s %5s %10s %5s %10s" % ("kernel<T,V,L>", "lds", "sgpr", "sgpr_spill", "vgpr", "vgpr_spill"))
for r in sorted(rows):
    print("%-32s %5s %5s %10s %5s %10s" % r)
PY
