# CPU-only: csrc/hip/converter.h (the tree uploader's validation and re-layout) in a stand-alone program under AddressSanitizer + UBSan and
# under ThreadSanitizer: the table of rejections, seeded mutants in exactly-sized allocations, the fill pass on 1, 3, 8 and 64 threads; then what
# the restatement (tests/converter_ref.py) makes of the test suite's own mutant set.   bash tools/sanitize_converter.sh [mutants] > profiles/converter.txt
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${TMPDIR:-/tmp}/gpuart_sanitize
mkdir -p $OUT
for san in address,undefined thread; do
  $HIPCC --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -ffp-contract=off -fno-omit-frame-pointer -Wno-unused-function -Wno-bitwise-instead-of-logical \
    -I$ROOT/gpuart_amd/csrc/hip -I$ROOT/include -Xarch_host -fsanitize=$san -Xarch_host -fno-sanitize-recover=all \
    -o $OUT/converter_${san%%,*} $ROOT/tools/converter_sanitize.cpp -lpthread
  echo "== -fsanitize=$san"
  $OUT/converter_${san%%,*} ${1:-200000}
done
echo "== the suite's mutants (tests/converter_cases.py), as the restatement judges them"
(cd $ROOT && python -m tests.converter_cases)
