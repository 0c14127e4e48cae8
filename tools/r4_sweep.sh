#!/bin/bash
# r = 4 sweep: tile configuration x rank method through bench.py (tools/r4_sweep.sh cfg...)
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
sides=(); for cfg in "$@"; do for rk in 0 2; do sides+=(--side "cfg=$cfg rank=$rk" "--rank-method $rk --tile-config $cfg"); done; done
python $REPO/tools/ab.py --rounds 2 --bench $REPO/bench.py \
  --common "--full --radix-bits 4 --steps 10 --warmup 2 --no-cpu-baseline --no-extra" "${sides[@]}"
