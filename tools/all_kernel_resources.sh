#!/bin/bash
# Register / LDS / scratch table of EVERY kernel of the library (all csrc/*.hip; cross-compiles, no GPU needed):
#   tools/all_kernel_resources.sh [source root, default: this checkout] > table.txt
# Two tables made from two checkouts (the parent commit, e.g. a `git worktree`, and the change) diff kernel by kernel:
# a pre-existing instance must keep its line (profiles/r09_affine_resources.txt).  `code` is a hash of the kernel's
# instruction stream, so a line also shows a kernel whose code changed while its register counts did not.
ROOT=$(cd "${1:-$(dirname "$0")/..}" && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
cd "$OUT" || exit 1
for f in "$ROOT"/super-resolution_amd/csrc/*.hip; do
  b=$(basename "$f" .hip)
  ( mkdir -p "$b" && cd "$b" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -mllvm -simplifycfg-sink-common=false \
      -Wno-invalid-offsetof -I"$ROOT/include" -I"$ROOT/super-resolution_amd/csrc" -c "$f" -save-temps -o "$b.o" 2>/dev/null ) &
done
wait
python3 - "$OUT" <<'PY'
import glob, hashlib, re, subprocess, sys
rows = []
def code_hash(text, name):
    # the kernel's instruction stream: comments, debug / alignment directives out, local labels by order of appearance
    body = re.search(r"^%s:.*?\n(.*?)^\s*\.(amdhsa_kernel|Lfunc_end)" % re.escape(name), text, flags=re.M | re.S).group(1)
    labels, lines = {}, []
    for ln in body.split("\n"):
        ln = ln.split(";")[0].strip()
        if ln and not re.match(r"\.(loc|file|cfi\w*|p2align|align|section)\b", ln):
            lines.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), ln))
    return hashlib.sha1("\n".join(lines).encode()).hexdigest()[:12]

for s in sorted(glob.glob(sys.argv[1] + "/*/*-hip-amdgcn-amd-amdhsa-gfx950.s")):
    text = open(s).read()
    if "amdhsa.kernels:" not in text:
        continue
    meta = text[text.index("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", meta)[1:]:
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)", blk, flags=re.M))
        if "name" in f:
            f["code"] = code_hash(text, f["name"])
            rows.append(f)
names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.split("\n")
out = []
for r, n in zip(rows, names):
    n = re.sub(r"\(.*$", "", n.replace("void ", "").replace("srmap::", "").replace("(anonymous namespace)::", ""))
    out.append("%-72s lds %6s sgpr %3s spill %3s vgpr %3s spill %3s scratch %5s code %s" % (
        n, r.get("group_segment_fixed_size"), r.get("sgpr_count"), r.get("sgpr_spill_count"), r.get("vgpr_count"),
        r.get("vgpr_spill_count"), r.get("private_segment_fixed_size"), r["code"]))
print("\n".join(sorted(out)))
PY
