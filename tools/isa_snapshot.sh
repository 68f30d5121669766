#!/bin/bash
# Device assembly of the GEMM units, to answer "did this source change alter the generated code?" without a GPU:
#   tools/isa_snapshot.sh OUTDIR [unit ...]     before and after the change, then diff -r the two directories
# Compiles with build.sh's flags plus --offload-device-only -S and drops the lines that name __hip_cuid_ (a hash of the
# source text, the only thing that differs when comments or line numbers change).
set -e -o pipefail
out=$(mkdir -p "$1" && cd "$1" && pwd); shift
cd "$(dirname "$0")/../simxns_amd/csrc"
eval "$(grep '^FLAGS=' build.sh)"
[ $# -gt 0 ] || set -- gemm gemm_p5 gemm_tn5 gemm_x3 gemm_xp
PIDS=""
for u in "$@"; do
  ( hipcc $FLAGS --offload-device-only -S $u.hip -o - 2> "$out/$u.err" | grep -v __hip_cuid_ > "$out/$u.s" \
      || { grep -v kernel-resource-usage "$out/$u.err" | head -40 >&2; exit 1; }; rm -f "$out/$u.err" ) &
  PIDS="$PIDS $!"
done
for p in $PIDS; do wait $p; done
wc -l "$out"/*.s
