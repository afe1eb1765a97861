#!/bin/bash
# Device ISA of every product translation unit with the product flags (for
# "the product ISA did not change" checks):  bash tools/isa_snapshot.sh <dir> [tree]
# then  python tools/isa_compare.py <dir1> <dir2>  (comments and blank lines stripped).
# [tree]: another checkout of this repository to snapshot with this script
# (default: the one the script is in).  Every csrc/wk_*.hip is covered; a unit
# without kernels (the C-ABI units) yields an empty file.
set -e
R=$(cd "${2:-$(dirname "$0")/..}" && pwd)
D=${1:?outdir}
mkdir -p "$D"
FL="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -fno-signed-zeros -ffp-contract=fast -fno-slp-vectorize -I $R/include -I $R/esp32-wake-word_amd/csrc"
for src in "$R"/esp32-wake-word_amd/csrc/wk_*.hip; do
  f=$(basename "$src" .hip)
  /opt/rocm/bin/hipcc $FL --cuda-device-only -S "$src" -o "$D/$f.raw.s" 2>/dev/null &
  while [ "$(jobs -rp | wc -l)" -ge 8 ]; do wait -n || true; done
done
wait
for f in "$D"/*.raw.s; do
  grep -v '^\s*;' "$f" | grep -v '^\s*$' | grep -v '\.file\|\.ident\|amdhsa.version\|\.loc\b\|__hip_cuid' > "${f%.raw.s}.s" || true
  rm "$f"
done
