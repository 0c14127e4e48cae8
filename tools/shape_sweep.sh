#!/bin/bash
# bench.py over tile configurations, interleaved, two rounds: tools/shape_sweep.sh "<bench args>" cfg...
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
ARGS=$1; shift
sides=(); for cfg in "$@"; do sides+=(--side "cfg=$cfg" "--tile-config $cfg"); done
python $REPO/tools/ab.py --rounds 2 --bench $REPO/bench.py \
  --common "--full $ARGS --steps 20 --warmup 3 --no-cpu-baseline --no-extra" "${sides[@]}"
