#!/usr/bin/env bash
# build_dropin.sh — compile tests/cpp/test_multi.cpp (C-ABI, mi355_sw_multi_*) and tests/cpp/test_dropin.cpp against
# include/parseq/*.h:
#   test_dropin.bin        without Eigen on the include path (parseq::Timings / parseq::DenseMatrix signatures)
#   test_multi.bin
# Both are git-ignored.  The builds that need the reference (test_dropin.cpp with the reference's vendored Eigen, the
# reference's own test/*.cpp) are oracle/build_ref.sh's: they land in oracle/_ref/.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
FLAGS=(-std=c++17 -O1 -Wall -Werror -pthread "-I$ROOT/include")
LINK=("-L$ROOT/parallel-genomeseq_amd" -lmi355_sw "-Wl,-rpath,$ROOT/parallel-genomeseq_amd")
g++ "${FLAGS[@]}" -DPARSEQ_NO_EIGEN "$HERE/test_dropin.cpp" "${LINK[@]}" -o "$HERE/test_dropin.bin"
g++ "${FLAGS[@]}" "$HERE/test_multi.cpp" "${LINK[@]}" -o "$HERE/test_multi.bin"
