#!/bin/bash
# Diagnostic library with in-kernel s_memtime phase stamps (never the product).
# The unit list is wakeword.build's SOURCES (the product's).
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
cd "$R/esp32-wake-word_amd"
HIPCC=/opt/rocm/bin/hipcc
FL="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -fno-signed-zeros -ffp-contract=fast -fno-slp-vectorize -I $R/include -I csrc -DWK_DIAG"
SRCS=$(python -c "from wakeword.build import SOURCES; print(' '.join(SOURCES))")
mkdir -p build/diag
rm -f build/diag/*.o
for f in $SRCS; do $HIPCC $FL -c csrc/$f -o build/diag/${f%.*}.o & done; wait
for f in $SRCS; do [ -f build/diag/${f%.*}.o ] || { echo "compile of $f failed"; exit 1; }; done
$HIPCC --offload-arch=gfx950 -shared -fPIC build/diag/*.o -Wl,-rpath,/opt/rocm/lib -o build/diag/libwakeword_diag.so
# The K = 32 rule on what was built, as tests/test_isa_rules.py checks the product.
# (tools/isa_rules.py: kernel_stats, k32_violations; prints its per-kernel table, exits 1 on a violation)
python "$R/tools/isa_rules.py" build/diag/libwakeword_diag.so
echo "$R/esp32-wake-word_amd/build/diag/libwakeword_diag.so"
