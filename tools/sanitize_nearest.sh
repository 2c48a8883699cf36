# CPU-only: csrc/hip/nearest_rule.h (the closest-point rule) in a stand-alone program under AddressSanitizer + UBSan: honest and degenerate
# primitives of the four types at scales from 1e-30 to 2^18 against ordinary, coincident, huge and non-finite points; every answer inside
# its box, no NaN, and the lemma (box_d2 <= d2, outer box <= inner box) without exception.   bash tools/sanitize_nearest.sh [rounds]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/gpuart_sanitize
mkdir -p $OUT
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
  -I$ROOT/gpuart_amd/csrc/hip -o $OUT/nearest_sanitize $ROOT/tools/nearest_sanitize.cpp
echo "== -fsanitize=address,undefined"
$OUT/nearest_sanitize ${1:-200000}
