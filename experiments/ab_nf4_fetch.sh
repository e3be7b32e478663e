#!/bin/bash
# Level-fetch A/B of the NF4 one-token GEMV: the in-tree library (byte permutes)
# against variant builds of csrc/nf4.hip, alternated in one session.
#   build (from torchao-fork_amd/csrc, after `make`), V = 1 (select tree) or 2 (x re-paired):
#     hipcc $CXXFLAGS -DTAO_NF4_FETCH=$V -c nf4.hip -o ../../experiments/ablib/nf4_fetch$V.o
#     hipcc $LDFLAGS $(ls build/*.o | grep -v /nf4.o) ../../experiments/ablib/nf4_fetch$V.o \
#       -o ../../experiments/ablib/libtao_nf4_fetch$V.so
#   run: bash experiments/ab_nf4_fetch.sh [rounds]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq "${1:-2}"); do
  timeout -k 10 90 python3 "$R/experiments/ab_nf4_fetch.py" permutes || exit 1
  for v in 1 2; do
    TORCHAO_MI355X_LIB="$R/experiments/ablib/libtao_nf4_fetch$v.so" \
      timeout -k 10 90 python3 "$R/experiments/ab_nf4_fetch.py" "variant$v" || exit 1
  done
done
