#!/bin/bash
# A/B an environment switch with bench.py itself: tools/ab_env.sh VAR=a VAR=b ...   (interleaved, three rounds)
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
sides=(); for kv in "$@"; do sides+=(--side "$kv" "$kv"); done
python $REPO/tools/ab.py --rounds 3 --bench $REPO/bench.py "${sides[@]}"
