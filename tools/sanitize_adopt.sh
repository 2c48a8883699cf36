# CPU-only: BoundingVolumesHierarchy::AdoptTopology under AddressSanitizer + UBSan (tools/adopt_sanitize.cpp: trees from one primitive to a
# few thousand, their own refs adopted unchanged, then seeded mutants of refs and orders — each refused with the tree untouched, or
# adopted into a consistent tree).   bash tools/sanitize_adopt.sh
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
H=$ROOT/gpuart_amd/csrc/host
OUT=${TMPDIR:-/tmp}/gpuart_sanitize
mkdir -p $OUT
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -I$H -I$ROOT/include -o $OUT/adopt_address $ROOT/tools/adopt_sanitize.cpp $H/bvh.cpp $H/core.cpp -lpthread
echo "== AdoptTopology, -fsanitize=address,undefined"
$OUT/adopt_address
